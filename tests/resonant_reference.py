"""numpy restatement of the resonant low-pass / high-pass (signals_amd/chain/ext.py: ResonantLowPass / ResonantHighPass), the
build-defined filters the reference has no counterpart of (its filters are Butterworth, q = 1/sqrt2).  Per voice and block, float64:

    wn  = clip(cutoff / (rate / 2), 0, 1)          # as fx.py:99-102; ValueError unless 0 < wn < 1 (NaN too)
    q   = resonance                                 # ValueError unless finite and q > 0; unplugged: d = sqrt2 (q = 1/sqrt2)
    k   = tan(pi * wn / 2);  d = 1 / q;  nrm = 1 / (1 + d*k + k*k)
    lp:  b = (k*k, 2*k*k, k*k) * nrm        hp:  b = (1, -2, 1) * nrm
    a   = (1, 2*(k*k - 1)*nrm, (1 - d*k + k*k)*nrm)

then the block semantics of `oracle.chain_ref.crit_filter` (fx.py:85-106): the window [before | block | after] filtered from zero
state with scipy.signal.sosfilt, one section, the block kept.  `rbj_sos` is the RBJ cookbook's form of the same two filters, which
the host test compares against; `oracle_node` takes part in `render_stream`'s cache and context semantics like `chain_ref.Filter`."""
import math

import numpy as np
import scipy.signal

CONTEXT_FRAMES = 100


def resonant_sos(wn: float, q, btype: str) -> np.ndarray:
    """(1, 6) second-order section; `q` None: unplugged, the damping is sqrt2 itself (chain_ref.butter2_sos's arithmetic)"""
    if not (0.0 < wn < 1.0):
        raise ValueError('Digital filter critical frequencies must be 0 < Wn < 1')
    if q is None:
        d = math.sqrt(2.0)
    else:
        q = float(q)
        if not (math.isfinite(q) and q > 0.0):
            raise ValueError('filter resonance must be finite and > 0')
        d = 1.0 / q
    k = math.tan(math.pi * wn / 2.0)
    k2 = k * k
    nrm = 1.0 / (1.0 + d * k + k2)
    if btype == 'lp':
        b = (k2 * nrm, 2.0 * k2 * nrm, k2 * nrm)
    elif btype == 'hp':
        b = (nrm, -2.0 * nrm, nrm)
    else:
        raise ValueError(btype)
    return np.array([[b[0], b[1], b[2], 1.0, 2.0 * (k2 - 1.0) * nrm, (1.0 - d * k + k2) * nrm]])


def rbj_sos(wn: float, q: float, btype: str) -> np.ndarray:
    """the RBJ cookbook's low-pass / high-pass, normalised by a0: w0 = pi wn, alpha = sin(w0) / (2 q)"""
    w0 = math.pi * wn
    cs, alpha = math.cos(w0), math.sin(w0) / (2.0 * q)
    if btype == 'lp':
        b = ((1.0 - cs) / 2.0, 1.0 - cs, (1.0 - cs) / 2.0)
    else:
        b = ((1.0 + cs) / 2.0, -(1.0 + cs), (1.0 + cs) / 2.0)
    a0 = 1.0 + alpha
    return np.array([[b[0] / a0, b[1] / a0, b[2] / a0, 1.0, -2.0 * cs / a0, (1.0 - alpha) / a0]])


def scaled(cutoff: float, rate: int) -> float:
    """fx.py:99-101: the critical frequency over rate / 2, clipped to [0, 1]"""
    wn = np.array([cutoff], dtype=float)
    wn /= rate / 2
    wn.clip(0, 1, out=wn)
    return float(wn[0])


def resonant_filter(btype: str, window: np.ndarray, cutoff: np.ndarray, resonance, rate: int, frames: int,
                    ctx: int = CONTEXT_FRAMES) -> np.ndarray:
    """chain_ref.crit_filter with the resonant design: `window` is [before | block | after], `cutoff` and `resonance` one-row
    controls (IndexError where narrower than the window, like fx.py:99); `resonance` None: unplugged"""
    channels = window.shape[1]
    result = np.empty((frames, channels))
    for i in range(channels):
        sos = resonant_sos(scaled(cutoff[0, i], rate), None if resonance is None else resonance[0, i], btype)
        result[:, i] = scipy.signal.sosfilt(sos, window[:, i], axis=0)[-(frames + ctx):-ctx]
    return result


def filter_blocks(btype: str, x: np.ndarray, history: int, frames: int, blocks: int, cutoff, resonance, rate: int,
                  ctx: int = CONTEXT_FRAMES) -> np.ndarray:
    """what sig_biquad_coldstart_q computes: `x` holds `history` = min(ctx, position) rows in front of blocks * frames rows;
    block b is filtered from zero state over [min(ctx, position + b frames) rows | block], with row b (or the only row) of `cutoff`
    and `resonance` ((1 | blocks, V); `resonance` None: unplugged)"""
    out = np.empty((blocks * frames, x.shape[1]))
    for b in range(blocks):
        start = history + b * frames
        c = min(ctx, start)
        window = np.concatenate([x[start - c:start + frames], np.zeros((ctx, x.shape[1]))])      # (the `after` rows never reach the block)
        cut = cutoff[b if cutoff.shape[0] > 1 else 0][None, :]
        res = None if resonance is None else resonance[b if resonance.shape[0] > 1 else 0][None, :]
        out[b * frames:(b + 1) * frames] = resonant_filter(btype, window, np.broadcast_to(cut, (1, x.shape[1])),
                                                           None if res is None else np.broadcast_to(res, (1, x.shape[1])), rate, frames, ctx)
    return out


def oracle_node():
    """the oracle Node class of the resonant filters (imported lazily: the functions above need numpy and scipy alone)"""
    from oracle import chain_ref as R

    class ResonantFilter(R.Node):
        """chain_ref.Filter with a second block-rate control; `resonance` None: unplugged"""

        def __init__(self, btype, input=None, cutoff=None, resonance=None):
            super().__init__(input=input, cutoff=cutoff, resonance=resonance)
            self.btype = btype

        def eval(self, position, frames, channels, rate):
            cutoff = self._ctrl('cutoff', position, channels, rate)
            resonance = self._ctrl('resonance', position, channels, rate) if self.inputs.get('resonance') is not None else None
            window = self._with_context('input', position, frames, channels, rate, R.CONTEXT_FRAMES)
            if window.shape[1] != channels:
                raise IndexError('filter input narrower than the request (fx.py:98-105)')
            return resonant_filter(self.btype, window, cutoff, resonance, rate, frames)
    return ResonantFilter
