"""numpy restatement of the dense FIR filter (signals_amd/chain/ext.py: FIR), the build-defined node the reference has no counterpart
of.  The state `taps` is an (L, W) real array, 1 <= L <= 101, W >= 1, L * W <= 4096, all values finite: W impulse responses of L taps.
float64 arithmetic in numpy's operator order, no fused multiply-add, over an explicit window of `c0` context rows followed by the
block(s); per voice v and block:

    w      = clip(floor(select[0, v]), 0, W - 1)       # unplugged, disabled or NaN: column 0
    x[m]   = +0.0  for an absolute frame m < 0         # i.e. for a window row < 0
    acc    = h[0, w] * x[n]
    acc    = acc + h[k, w] * x[n - k]                  # k = 1 .. L - 1, ascending
    out[n] = acc

No tap is skipped: zero taps and the zero-filled rows are multiplied and added like the rest, so NaN and +-inf propagate as written.

`columns_of` is the per-block part, `fir_block` one block over its window, `fir` K blocks with per-block select rows, the way the
node reads its control port once per block (forward_at_block_rate); `fir_loop` is the same definition one sample at a time in
Python floats, for the host test; `oracle_node` is the node for oracle.chain_ref graphs."""
import math

import numpy as np

CONTEXT = 100
MAX_TAPS = 101
MAX_POINTS = 4096


def columns_of(select, W) -> np.ndarray:
    """int64 (V | 1,): the column each voice reads for one block -- `select` a (1, V | 1) row"""
    s = np.asarray(select, dtype=np.float64).reshape(-1)
    with np.errstate(invalid='ignore'):
        w = np.clip(np.floor(np.where(np.isnan(s), 0.0, s)), 0.0, float(W - 1))
    return w.astype(np.int64)


def fir_block(window, c0, frames, select, taps, first=0) -> np.ndarray:
    """float64 (frames, V): the block whose row n is window row c0 + first + n; `window` float64 (>= c0 + first + frames, V | 1) whose
    row 0 is absolute frame position - c0, rows in front of it read as zeros"""
    x = np.asarray(window, dtype=np.float64)
    h = np.asarray(taps, dtype=np.float64)
    L, W = h.shape
    assert 1 <= L <= MAX_TAPS and W >= 1 and L * W <= MAX_POINTS
    w = columns_of(select, W)
    V = max(x.shape[1], w.shape[0])
    x = np.broadcast_to(x, (x.shape[0], V))
    hv = h[:, np.broadcast_to(w, (V,))]                                        # (L, V): every voice's own column
    padded = np.concatenate([np.zeros((CONTEXT, V)), x])                       # the zero fill, explicit
    at = CONTEXT + c0 + first
    with np.errstate(invalid='ignore', over='ignore'):
        acc = hv[0][None, :] * padded[at:at + frames]
        for k in range(1, L):
            acc = acc + hv[k][None, :] * padded[at - k:at - k + frames]
    return np.array(acc)


def fir(window, c0, frames, select, taps, blocks=1) -> np.ndarray:
    """float64 (blocks * frames, V): `window` is c0 context rows and then blocks * frames rows, `select` (1 | blocks, V | 1) rows, row b
    serving block b"""
    select = np.atleast_2d(np.asarray(select, dtype=np.float64))
    out = [fir_block(window, c0, frames, select[b if select.shape[0] > 1 else 0][None, :], taps, first=b * frames)
           for b in range(blocks)]
    return np.concatenate(out, axis=0)


def fir_loop(x: list, at: int, select: float, taps) -> float:
    """one sample, straight from the definition: x a list of Python floats whose entry k is absolute frame k (frames < 0: zero),
    `at` the frame, taps an (L, W) nested list or array"""
    L, W = len(taps), len(taps[0])
    if math.isnan(select):
        w = 0
    else:
        s = math.floor(select) if math.isfinite(select) else select
        w = 0 if s < 1 else (W - 1 if s >= W - 1 else int(s))
    acc = None
    for k in range(L):
        xv = x[at - k] if at - k >= 0 else 0.0
        p = float(taps[k][w]) * xv
        acc = p if acc is None else acc + p
    return acc


def oracle_node():
    """the oracle Node class of the FIR filter (imported lazily: the functions above need numpy alone)"""
    from oracle import chain_ref as R

    class FIR(R.Node):
        """takes part in render_stream's cache and context semantics like a Filter: the same three requests"""

        def __init__(self, input=None, select=None, taps=((1.0,),)):
            super().__init__(input=input, select=select)
            self.taps = np.asarray(taps, dtype=np.float64)

        def eval(self, position, frames, channels, rate):
            select = self._ctrl('select', position, channels, rate)
            window = self._with_context('input', position, frames, channels, rate, CONTEXT)
            c0 = min(CONTEXT, position)
            return fir_block(window[:c0 + frames], c0, frames, select[:, :channels], self.taps)
    return FIR
