"""numpy restatement of the short multi-tap delay line (signals_amd/chain/ext.py: Delay), the build-defined node the reference has no
counterpart of.  float64 arithmetic in numpy's operator order, no fused multiply-add, over an explicit window of `c0` context rows
followed by the block(s); x[m] = 0 for an absolute frame m < 0, i.e. for a window row < 0:

    t   = time[0, v]
    d_u = clip((t * rate) * m_u, 0, 99)            # np.clip: NaN stays NaN, +inf -> 99, -inf -> 0
    i_u = floor(d_u);  f_u = d_u - i_u
    s_u[n] = x[n - i_u] + f_u * (x[n - i_u - 1] - x[n - i_u])
    out[n] = g_0 * s_0[n]  (+ g_1 * s_1[n] + ...  added in ascending u)      # every row NaN for a voice with a NaN d_u

`taps_of` is the per-block part, `delay_block` one block over its window, `delay` K blocks with per-block time rows, the way the
node reads its control port once per block (forward_at_block_rate); `delay_loop` is the same definition one sample at a time in
Python floats, for the host test; `oracle_node` is the node for oracle.chain_ref graphs."""
import math

import numpy as np

CONTEXT = 100
MAX_FRAMES = 99


def taps_of(time, rate, taps):
    """(i, f, nan) of the taps for one block: int64 (U, V), float64 (U, V), bool (V,) -- `time` a (1, V | 1) row, `taps` (U, 2)"""
    t = np.asarray(time, dtype=np.float64).reshape(1, -1)
    m = np.asarray(taps, dtype=np.float64)[:, :1]
    with np.errstate(invalid='ignore', over='ignore'):
        d = np.clip((t * float(rate)) * m, 0.0, float(MAX_FRAMES))
    nan = np.isnan(d)
    whole = np.floor(np.where(nan, 0.0, d))                                    # (no index is formed from a NaN)
    f = np.where(nan, 0.0, d - whole)
    return whole.astype(np.int64), f, nan.any(axis=0)


def delay_block(window, c0, frames, time, rate, taps, first=0) -> np.ndarray:
    """float64 (frames, V): the block whose row n is window row c0 + first + n; `window` float64 (>= c0 + first + frames, V | 1) whose
    row 0 is absolute frame position - c0, rows in front of it read as zeros"""
    x = np.asarray(window, dtype=np.float64)
    g = np.asarray(taps, dtype=np.float64)[:, 1]
    i, f, nan = taps_of(time, rate, taps)
    V = max(x.shape[1], i.shape[1])
    x = np.broadcast_to(x, (x.shape[0], V))
    padded = np.concatenate([np.zeros((CONTEXT + 1, V)), x])                   # the zero fill, explicit
    rows = (CONTEXT + 1 + c0 + first + np.arange(frames))[:, None]
    cols = np.arange(V)[None, :]
    out = None
    with np.errstate(invalid='ignore', over='ignore'):
        for u in range(i.shape[0]):
            iu = np.broadcast_to(i[u], (V,))[None, :]
            x0, x1 = padded[rows - iu, cols], padded[rows - iu - 1, cols]
            s = x0 + f[u][None, :] * (x1 - x0)
            p = g[u] * s
            out = p if out is None else out + p
    out = np.array(np.broadcast_to(out, (frames, V)))
    out[:, np.broadcast_to(nan, (V,))] = np.nan
    return out


def delay(window, c0, frames, time, rate, taps, blocks=1) -> np.ndarray:
    """float64 (blocks * frames, V): `window` is c0 context rows and then blocks * frames rows, `time` (1 | blocks, V | 1) rows, row b
    serving block b"""
    time = np.atleast_2d(np.asarray(time, dtype=np.float64))
    out = [delay_block(window, c0, frames, time[b if time.shape[0] > 1 else 0][None, :], rate, taps, first=b * frames)
           for b in range(blocks)]
    return np.concatenate(out, axis=0)


def delay_loop(x: list, at: int, t: float, rate: float, taps: list) -> float:
    """one sample, straight from the definition: x a list of Python floats whose entry k is absolute frame k (frames < 0: zero),
    `at` the frame, taps a list of (m, g)"""
    def sample(k):
        return x[k] if k >= 0 else 0.0
    out = None
    for m, g in taps:
        d = (t * rate) * m
        if math.isnan(d):
            return math.nan
        d = 0.0 if d <= 0.0 else (float(MAX_FRAMES) if d > MAX_FRAMES else d)      # (<=: f = +0 for d = -0 too, as d - floor(d) gives)
        i = math.floor(d)
        f = d - i
        x0, x1 = sample(at - i), sample(at - i - 1)
        p = g * (x0 + f * (x1 - x0))
        out = p if out is None else out + p
    return out


def oracle_node():
    """the oracle Node class of the delay line (imported lazily: the functions above need numpy alone)"""
    from oracle import chain_ref as R

    class Delay(R.Node):
        """takes part in render_stream's cache and context semantics like a Filter: the same three requests"""

        def __init__(self, input=None, time=None, taps=((1.0, 1.0),)):
            super().__init__(input=input, time=time)
            self.taps = np.asarray(taps, dtype=np.float64)

        def eval(self, position, frames, channels, rate):
            time = self._ctrl('time', position, channels, rate)
            window = self._with_context('input', position, frames, channels, rate, CONTEXT)
            c0 = min(CONTEXT, position)
            return delay_block(window[:c0 + frames], c0, frames, time[:, :channels], rate, self.taps)
    return Delay
