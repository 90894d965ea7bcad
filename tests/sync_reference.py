"""numpy restatement of the hard-sync oscillators (signals_amd/chain/ext.py: SyncSawtooth / SyncSquare), build-defined nodes the
reference has no counterpart of, on tests/blep_reference.py's `step` / `increment` and oracle.chain_ref's own functions.  float64
arithmetic in numpy's operator order, no fused multiply-add.  A slave oscillator at `ratio` times the master's pitch is reset at
every cycle of the master; the master's phase is the band-limited oscillator's (tests/blep_reference.py), bit for bit.  `copies` is
(U, 2) as there; hertz, phase, spread and ratio are read at block rate:

    r_u, h_u, q_u, t_u, d   as blep_reference              # t = frame_range / rate * h_u + q_u;  d = min(|h_u| / rate, 0.5)
    R  = max(ratio, 1.0)                                   # a ratio that is not finite: a NaN row
    m  = mod(t, 1);  s = m * R;  k = floor(s);  f = s - k  # the slave's phase f in its k-th cycle since the reset
    ds = min(d * R, 0.5)                                   # the slave's increment per sample
    g  = R - (ceil(R) - 1)                                 # the length of the last, cut slave cycle, in (0, 1]

    estep(p, lo_ok, hi_ok) = 2x - x*x - 1   with x = p / ds         if p < ds      and lo_ok
                           = y*y + 2y + 1   with y = (p - 1) / ds   if p > 1 - ds  and hi_ok
                           = 0                                      otherwise

    Sawtooth: w = (2f - 1) - estep(f, k >= 1, k + 1 < R) - g * step(m, d)
    Square:   sb = s + 0.5;  kb = floor(sb);  fb = sb - kb
              w  = (f < 0.5 ? 1 : -1) + estep(f, k >= 1, k + 1 < R) - estep(fb, kb >= 1, kb + 0.5 < R)
                   + (g <= 0.5 ? 0 : 1) * step(m, d)

    out = (sum over u ascending of w_u) / U

The slave's edges strictly inside the master's cycle take the residual at the slave's rate (estep), the reset at m = 0 -- of height
2 g for the Sawtooth, 0 or 2 for the Square -- the one at the master's (blep_reference.step).  Every choice is a select (np.where):
d == 0 selects no window, a non-finite t gives NaN.  `naive=True` drops every residual: the plain hard-synced waveform, for the
aliasing comparison.  With ratio <= 1 (or unplugged: zeros) the Sawtooth is blep_reference's at phase + 0.5 and the Square
blep_reference's own.  Continuous in t but for one case: where the last interior edge lies closer to the reset than one window (the
Sawtooth: g < ds; the Square: 0 < (g mod 0.5) < ds) that edge's trailing window is cut at the reset.  The formula is the definition
there too.

`sync` renders K blocks of N frames with per-block parameter rows like blep_reference.blep; `SyncOsc` is the same as an oracle
Node."""
import numpy as np

from oracle import chain_ref as R

from blep_reference import RATE, alias_ratio_db, default_copies, increment, step     # noqa: F401  (re-exported for the tests)

KINDS = ('Sawtooth', 'Square')


def estep(p, ds, lo_ok, hi_ok):
    """the residual of a unit step at the slave's rate, each side taken only where that edge is the slave's own"""
    with np.errstate(all='ignore'):
        x = p / ds
        y = (p - 1.0) / ds
        lo = 2.0 * x - x * x - 1.0
        hi = y * y + 2.0 * y + 1.0
        return np.where((p < ds) & lo_ok, lo, np.where((p > 1.0 - ds) & hi_ok, hi, 0.0))


def effective_ratio(ratio):
    """R = max(ratio, 1); NaN where the ratio is not finite (np.maximum would keep an inf, fmax would drop a NaN: a select)"""
    ratio = np.asarray(ratio, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        return np.where(np.isfinite(ratio), np.maximum(ratio, 1.0), np.nan)


def in_window(kind: str, t, d, ratio):
    """True where a sample of master phase t lies in a window that the definition takes -- the reset's, or an interior edge's on the
    side that is the slave's own (elsewhere the value is the naive one's)"""
    t, d, ratio = np.broadcast_arrays(np.asarray(t, dtype=np.float64), np.asarray(d, dtype=np.float64), np.asarray(ratio, dtype=np.float64))
    Rr = effective_ratio(ratio)
    with np.errstate(all='ignore'):
        m = np.mod(t, 1.0)
        s = m * Rr
        ds = np.minimum(d * Rr, 0.5)

        def near(x, first):
            k = np.floor(x)
            p = x - k
            return ((p < ds) & (k >= 1.0)) | ((p > 1.0 - ds) & (k + first < Rr))
        inside = (m < d) | (m > 1.0 - d) | near(s, 1.0)
        if kind == 'Square':
            inside = inside | near(s + 0.5, 0.5)
    return inside


def sync_wave(kind: str, t, d, ratio, naive: bool = False):
    """one copy's sample: float64 arrays t (the master's phase in cycles), d (cycles per sample, 0 <= d <= 0.5) and ratio, broadcast
    together"""
    t, d, ratio = np.broadcast_arrays(np.asarray(t, dtype=np.float64), np.asarray(d, dtype=np.float64), np.asarray(ratio, dtype=np.float64))
    Rr = effective_ratio(ratio)
    with np.errstate(all='ignore'):
        m = np.mod(t, 1.0)
        s = m * Rr
        k = np.floor(s)
        f = s - k
        ds = np.minimum(d * Rr, 0.5)
        g = Rr - (np.ceil(Rr) - 1.0)
        if kind == 'Sawtooth':
            w = 2.0 * f - 1.0
            if not naive:
                w = w - estep(f, ds, k >= 1.0, k + 1.0 < Rr) - g * step(m, d)
        elif kind == 'Square':
            w = np.where(f < 0.5, 1.0, -1.0)
            if not naive:
                sb = s + 0.5
                kb = np.floor(sb)
                fb = sb - kb
                w = w + estep(f, ds, k >= 1.0, k + 1.0 < Rr) - estep(fb, ds, kb >= 1.0, kb + 0.5 < Rr) + np.where(g <= 0.5, 0.0, 1.0) * step(m, d)
        else:
            raise ValueError(f'no hard-sync {kind}')
    return np.where(np.isnan(m) | np.isnan(Rr), np.nan, w)


def sync_sum(kind: str, frames: np.ndarray, rate: int, hertz, phase, spread, ratio, copies, naive: bool = False) -> np.ndarray:
    """the definition over a column of frame numbers (int64 (rows, 1)) and one row of each control: float64 (rows, V | 1)"""
    copies = np.asarray(copies, dtype=np.float64)
    total = None
    for d, p in copies:
        r = 1.0 + spread * d
        h = hertz * r
        q = phase + p
        w = sync_wave(kind, frames / rate * h + q, increment(h, rate), ratio, naive)
        total = w if total is None else total + w
    return total / copies.shape[0]


def sync(kind: str, copies, position: int, frames: int, hertz, phase=0.0, spread=0.0, ratio=0.0, rate: int = RATE, blocks: int = 1,
         step: int = 1, naive: bool = False) -> np.ndarray:
    """float64 (blocks * frames, V): row r is frame position + r * step; hertz / phase / spread / ratio are (1 | blocks, V | 1) rows,
    row b serving the `frames` output rows of block b"""
    rows = [np.atleast_2d(np.asarray(x, dtype=np.float64)) for x in (hertz, phase, spread, ratio)]
    out = []
    for b in range(blocks):
        hz, ph, sp, ra = (r[b if r.shape[0] > 1 else 0][None, :] for r in rows)
        n = np.arange(position + b * frames * step, position + (b + 1) * frames * step, step, dtype=np.int64)[:, None]
        out.append(sync_sum(kind, n, rate, hz, ph, sp, ra, copies, naive))
    width = max(o.shape[1] for o in out)
    return np.concatenate([np.broadcast_to(o, (o.shape[0], width)) for o in out], axis=0)


class SyncOsc(R.Node):
    """takes part in render_stream's cache and context semantics like any oracle node; `copies` is read at every evaluation; an
    unplugged `ratio` answers zeros like every port"""

    def __init__(self, kind, copies, hertz=None, phase=None, spread=None, ratio=None, naive=False):
        super().__init__(hertz=hertz, phase=phase, spread=spread, ratio=ratio)
        self.kind, self.copies, self.naive = kind, copies, naive

    def eval(self, position, frames, channels, rate):
        phase = self._ctrl('phase', position, channels, rate)
        hertz = self._ctrl('hertz', position, channels, rate)
        spread = self._ctrl('spread', position, channels, rate)
        ratio = self._ctrl('ratio', position, channels, rate)
        return sync_sum(self.kind, R.frame_range(position, frames), rate, hertz, phase, spread, ratio, self.copies, self.naive)
