"""numpy restatement of the RBJ equaliser biquads (signals_amd/chain/ext.py: ResonantBandPass, Notch, AllPass, Peaking, LowShelf,
HighShelf), build-defined filters the reference has no counterpart of.  Per voice and block, float64:

    wn  = clip(cutoff / (rate / 2), 0, 1)          # as fx.py:99-102; ValueError unless 0 < wn < 1 (NaN too)
    q   = resonance                                 # ValueError unless finite and q > 0; unplugged: d = sqrt2 (q = 1/sqrt2)
    k   = tan(pi * wn / 2);  d = 1 / q
    A   = exp(gain * ln(10) / 40);  g = sqrt(A) * d # gain in dB: ValueError unless finite; unplugged: 0 dB (the three gain kinds only)
    sos = [b * nrm, 1, a1 * nrm, a2 * nrm]

    kind   b                                                    a1, a2                              1 / nrm
    bp     (d k, 0, -d k)                                       2 (k k - 1), 1 - d k + k k          1 + d k + k k
    notch  (1 + k k, 2 (k k - 1), 1 + k k)                      as bp                               as bp
    ap     (1 - d k + k k, 2 (k k - 1), 1 + d k + k k)          as bp                               as bp
    peak   (1 + d A k + k k, 2 (k k - 1), 1 - d A k + k k)      2 (k k - 1), 1 - (d / A) k + k k    1 + (d / A) k + k k
    ls     A (1 + g k + A k k, 2 (A k k - 1), 1 - g k + A k k)  2 (k k - A), A - g k + k k          A + g k + k k
    hs     A (A + g k + k k, 2 (k k - A), A - g k + k k)        2 (A k k - 1), 1 - g k + A k k      1 + g k + A k k

-- the bilinear transform s -> (1 - 1/z) / (k (1 + 1/z)) of the RBJ cookbook's analogue prototypes (BPF with a constant 0 dB peak,
notch, APF, peakingEQ, lowShelf, highShelf) -- then the block semantics of `oracle.chain_ref.crit_filter` (fx.py:85-106): the window
[before | block | after] filtered from zero state with scipy.signal.sosfilt, one section, the block kept.  `rbj_sos` is the
cookbook's trigonometric form of the same six filters, which the host test compares against; `oracle_node` takes part in
`render_stream`'s cache and context semantics like `chain_ref.Filter`."""
import math

import numpy as np
import scipy.signal

CONTEXT_FRAMES = 100
KINDS = ('bp', 'notch', 'ap', 'peak', 'ls', 'hs')
GAIN_KINDS = ('peak', 'ls', 'hs')


def eq_sos(wn: float, q, gain, kind: str) -> np.ndarray:
    """(1, 6) second-order section; `q` None: unplugged, the damping is sqrt2 itself; `gain` None (or a kind without the port): 0 dB"""
    if kind not in KINDS:
        raise ValueError(kind)
    if not (0.0 < wn < 1.0):
        raise ValueError('Digital filter critical frequencies must be 0 < Wn < 1')
    if q is None:
        d = math.sqrt(2.0)
    else:
        q = float(q)
        if not (math.isfinite(q) and q > 0.0):
            raise ValueError('filter resonance must be finite and > 0')
        d = 1.0 / q
    db = 0.0 if gain is None or kind not in GAIN_KINDS else float(gain)
    if not math.isfinite(db):
        raise ValueError('filter gain must be finite')
    A = math.exp(db * (math.log(10.0) / 40.0))
    g = math.sqrt(A) * d
    k = math.tan(math.pi * wn / 2.0)
    k2 = k * k
    if kind in ('bp', 'notch', 'ap'):
        a0, a1, a2 = 1.0 + d * k + k2, 2.0 * (k2 - 1.0), 1.0 - d * k + k2
        b = {'bp': (d * k, 0.0, -(d * k)), 'notch': (1.0 + k2, a1, 1.0 + k2), 'ap': (a2, a1, a0)}[kind]
    elif kind == 'peak':
        a0, a1, a2 = 1.0 + (d / A) * k + k2, 2.0 * (k2 - 1.0), 1.0 - (d / A) * k + k2
        b = (1.0 + d * A * k + k2, a1, 1.0 - d * A * k + k2)
    elif kind == 'ls':
        a0, a1, a2 = A + g * k + k2, 2.0 * (k2 - A), A - g * k + k2
        b = (A * (1.0 + g * k + A * k2), A * (2.0 * (A * k2 - 1.0)), A * (1.0 - g * k + A * k2))
    else:
        a0, a1, a2 = 1.0 + g * k + A * k2, 2.0 * (A * k2 - 1.0), 1.0 - g * k + A * k2
        b = (A * (A + g * k + k2), A * (2.0 * (k2 - A)), A * (A - g * k + k2))
    nrm = 1.0 / a0
    return np.array([[b[0] * nrm, b[1] * nrm, b[2] * nrm, 1.0, a1 * nrm, a2 * nrm]])


def rbj_sos(wn: float, q: float, gain: float, kind: str) -> np.ndarray:
    """the RBJ cookbook's tables, normalised by a0: w0 = pi wn, alpha = sin(w0) / (2 q), A = 10 ** (gain / 40)"""
    w0 = math.pi * wn
    cs, alpha = math.cos(w0), math.sin(w0) / (2.0 * q)
    A = 10.0 ** (gain / 40.0)
    if kind == 'bp':
        b, a = (alpha, 0.0, -alpha), (1.0 + alpha, -2.0 * cs, 1.0 - alpha)
    elif kind == 'notch':
        b, a = (1.0, -2.0 * cs, 1.0), (1.0 + alpha, -2.0 * cs, 1.0 - alpha)
    elif kind == 'ap':
        b, a = (1.0 - alpha, -2.0 * cs, 1.0 + alpha), (1.0 + alpha, -2.0 * cs, 1.0 - alpha)
    elif kind == 'peak':
        b, a = (1.0 + alpha * A, -2.0 * cs, 1.0 - alpha * A), (1.0 + alpha / A, -2.0 * cs, 1.0 - alpha / A)
    elif kind == 'ls':
        s = 2.0 * math.sqrt(A) * alpha
        b = (A * ((A + 1.0) - (A - 1.0) * cs + s), 2.0 * A * ((A - 1.0) - (A + 1.0) * cs), A * ((A + 1.0) - (A - 1.0) * cs - s))
        a = ((A + 1.0) + (A - 1.0) * cs + s, -2.0 * ((A - 1.0) + (A + 1.0) * cs), (A + 1.0) + (A - 1.0) * cs - s)
    elif kind == 'hs':
        s = 2.0 * math.sqrt(A) * alpha
        b = (A * ((A + 1.0) + (A - 1.0) * cs + s), -2.0 * A * ((A - 1.0) + (A + 1.0) * cs), A * ((A + 1.0) + (A - 1.0) * cs - s))
        a = ((A + 1.0) - (A - 1.0) * cs + s, 2.0 * ((A - 1.0) - (A + 1.0) * cs), (A + 1.0) - (A - 1.0) * cs - s)
    else:
        raise ValueError(kind)
    return np.array([[b[0] / a[0], b[1] / a[0], b[2] / a[0], 1.0, a[1] / a[0], a[2] / a[0]]])


def scaled(cutoff: float, rate: int) -> float:
    """fx.py:99-101: the critical frequency over rate / 2, clipped to [0, 1]"""
    wn = np.array([cutoff], dtype=float)
    wn /= rate / 2
    wn.clip(0, 1, out=wn)
    return float(wn[0])


def eq_filter(kind: str, window: np.ndarray, cutoff: np.ndarray, resonance, gain, rate: int, frames: int,
              ctx: int = CONTEXT_FRAMES) -> np.ndarray:
    """chain_ref.crit_filter with the equaliser design: `window` is [before | block | after], `cutoff`, `resonance` and `gain`
    one-row controls (IndexError where narrower than the window, like fx.py:99); `resonance` / `gain` None: unplugged"""
    channels = window.shape[1]
    result = np.empty((frames, channels))
    for i in range(channels):
        sos = eq_sos(scaled(cutoff[0, i], rate), None if resonance is None else resonance[0, i], None if gain is None else gain[0, i], kind)
        result[:, i] = scipy.signal.sosfilt(sos, window[:, i], axis=0)[-(frames + ctx):-ctx]
    return result


def filter_blocks(kind: str, x: np.ndarray, history: int, frames: int, blocks: int, cutoff, resonance, gain, rate: int,
                  ctx: int = CONTEXT_FRAMES, lenient: bool = False) -> np.ndarray:
    """what sig_biquad_coldstart_eq computes: `x` holds `history` = min(ctx, position) rows in front of blocks * frames rows; block b
    is filtered from zero state over [min(ctx, position + b frames) rows | block], with row b (or the only row) of `cutoff`,
    `resonance` and `gain` ((1 | blocks, V | 1); None: unplugged).  `lenient`: a voice whose design is refused answers NaN rows (what
    the kernels store) instead of raising"""
    V = x.shape[1]
    out = np.empty((blocks * frames, V))
    wide = lambda t, b: None if t is None else np.broadcast_to(t[b if t.shape[0] > 1 else 0][None, :], (1, V))
    for b in range(blocks):
        start = history + b * frames
        c = min(ctx, start)
        window = np.concatenate([x[start - c:start + frames], np.zeros((ctx, V))])      # (the `after` rows never reach the block)
        cut, res, gn = wide(cutoff, b), wide(resonance, b), wide(gain, b)
        for v in range(V):
            col = slice(v, v + 1)
            try:
                out[b * frames:(b + 1) * frames, col] = eq_filter(kind, window[:, col], cut[:, col], None if res is None else res[:, col],
                                                                  None if gn is None else gn[:, col], rate, frames, ctx)
            except ValueError:
                if not lenient:
                    raise
                out[b * frames:(b + 1) * frames, col] = np.nan
    return out


def oracle_node():
    """the oracle Node class of the equaliser filters (imported lazily: the functions above need numpy and scipy alone)"""
    from oracle import chain_ref as R

    class EqFilter(R.Node):
        """chain_ref.Filter with a second and a third block-rate control; `resonance` / `gain` None: unplugged"""

        def __init__(self, kind, input=None, cutoff=None, resonance=None, gain=None):
            super().__init__(input=input, cutoff=cutoff, resonance=resonance, gain=gain)
            self.kind = kind

        def eval(self, position, frames, channels, rate):
            cutoff = self._ctrl('cutoff', position, channels, rate)
            resonance = self._ctrl('resonance', position, channels, rate) if self.inputs.get('resonance') is not None else None
            gain = self._ctrl('gain', position, channels, rate) if self.inputs.get('gain') is not None else None
            window = self._with_context('input', position, frames, channels, rate, R.CONTEXT_FRAMES)
            if window.shape[1] != channels:
                raise IndexError('filter input narrower than the request (fx.py:98-105)')
            return eq_filter(self.kind, window, cutoff, resonance, gain, rate, frames)
    return EqFilter
