"""numpy restatement of the band-limited oscillators (signals_amd/chain/ext.py: BlepSquare / BlepSawtooth / BlepTriangle),
build-defined nodes the reference has no counterpart of, on oracle.chain_ref's own functions.  float64 arithmetic in numpy's
operator order, no fused multiply-add.  The phase is the unison oscillator's (tests/unison_reference.py), bit for bit; `copies` is
(U, 2): column 0 the relative detune d[u], column 1 the phase offset p[u] in cycles; hertz, phase and spread are read at block rate:

    r_u = 1.0 + spread * d[u]
    h_u = hertz * r_u
    q_u = phase + p[u]
    t_u = frame_range / rate * h_u + q_u           # Osc._eval's expression, osc.py:26-33
    d   = min(|h_u| / rate, 0.5)                   # the phase increment per sample, in cycles

    step(m)   = 2x - x*x - 1      with x = m / d            if m < d
              = y*y + 2y + 1      with y = (m - 1) / d      if m > 1 - d
              = 0                                            otherwise
    corner(m) = (1 - m/d)^3                                  if m < d
              = ((m - 1)/d + 1)^3                            if m > 1 - d
              = 0                                            otherwise

    Sawtooth: m = mod(t - 0.5, 1);  w = (2m - 1) - step(m)
    Square:   m = mod(t, 1);        w = (m < 0.5 ? 1 : -1) + step(m) - step(mod(t + 0.5, 1))
    Triangle: m = mod(t - 0.25, 1); w = tri(t - 0.25) + (4/3) d (corner(mod(t + 0.25, 1)) - corner(m))
              tri(u) = (4 mod(u, 0.5) - 1) * (m < 0.5 ? -1 : 1)       # = 4|m - 0.5| - 1, in osc.py's own order

    out = (sum over u ascending of w_u) / U

step is the two-sample polynomial residual of a unit step (PolyBLEP), corner its integral (the residual of a unit change of
slope).  The naive parts are osc.py's closed forms without np.sign's isolated zero at the edge; the Triangle's is written in
osc.py's order (4 |m - 0.5| - 1 rounds m - 0.5 below m = 1/4 and is an ulp off now and then), so that outside the windows every kind
is R.osc_wave bit for bit.  A non-finite t gives NaN.  d == 0 selects no window: the naive value.  Every choice is a select (np.where): what the
branch not taken computed -- an infinity or a NaN at d == 0 -- never reaches the result.

`blep` renders K blocks of N frames with per-block parameter rows, the way a node reads its control ports once per block
(forward_at_block_rate); `BlepOsc` is the same as an oracle Node, so that graphs with filters around it render as the reference's
pull protocol would."""
import numpy as np

from oracle import chain_ref as R

RATE = 48000
KINDS = ('Square', 'Sawtooth', 'Triangle')


def default_copies() -> np.ndarray:
    return np.zeros((1, 2))


def increment(h, rate: int):
    """d: the phase increment per sample in cycles, at most half a cycle"""
    return np.minimum(np.abs(h) / rate, 0.5)


def step(m, d):
    with np.errstate(all='ignore'):
        x = m / d
        y = (m - 1.0) / d
        lo = 2.0 * x - x * x - 1.0
        hi = y * y + 2.0 * y + 1.0
    return np.where(m < d, lo, np.where(m > 1.0 - d, hi, 0.0))


def corner(m, d):
    with np.errstate(all='ignore'):
        a = 1.0 - m / d
        b = (m - 1.0) / d + 1.0
        lo = a * a * a
        hi = b * b * b
    return np.where(m < d, lo, np.where(m > 1.0 - d, hi, 0.0))


def in_window(kind: str, t, d):
    """True where a sample of phase t lies in one of the kind's correction windows (elsewhere the value is the naive waveform's)"""
    def near(m):
        return (m < d) | (m > 1.0 - d)
    with np.errstate(invalid='ignore'):
        if kind == 'Sawtooth':
            return near(np.mod(t - 0.5, 1.0))
        if kind == 'Square':
            return near(np.mod(t, 1.0)) | near(np.mod(t + 0.5, 1.0))
        return near(np.mod(t - 0.25, 1.0)) | near(np.mod(t + 0.25, 1.0))


def blep_wave(kind: str, t, d):
    """one copy's sample: float64 arrays t (cycles) and d (cycles per sample, 0 <= d <= 0.5), broadcast together"""
    t, d = np.broadcast_arrays(np.asarray(t, dtype=np.float64), np.asarray(d, dtype=np.float64))
    with np.errstate(invalid='ignore'):
        if kind == 'Sawtooth':
            m = np.mod(t - 0.5, 1.0)
            w = (2.0 * m - 1.0) - step(m, d)
        elif kind == 'Square':
            m = np.mod(t, 1.0)
            w = np.where(m < 0.5, 1.0, -1.0) + step(m, d) - step(np.mod(t + 0.5, 1.0), d)
        elif kind == 'Triangle':
            u = t - 0.25
            m = np.mod(u, 1.0)
            w = (4.0 * np.mod(u, 0.5) - 1.0) * np.where(m < 0.5, -1.0, 1.0) + 4.0 / 3.0 * d * (corner(np.mod(t + 0.25, 1.0), d) - corner(m, d))
        else:
            raise ValueError(f'no band-limited {kind}')
    return np.where(np.isnan(m), np.nan, w)


def blep_sum(kind: str, frames: np.ndarray, rate: int, hertz, phase, spread, copies) -> np.ndarray:
    """the definition over a column of frame numbers (int64 (rows, 1)) and one row of each control: float64 (rows, V | 1)"""
    copies = np.asarray(copies, dtype=np.float64)
    s = None
    for d, p in copies:
        r = 1.0 + spread * d
        h = hertz * r
        q = phase + p
        w = blep_wave(kind, frames / rate * h + q, increment(h, rate))
        s = w if s is None else s + w
    return s / copies.shape[0]


def blep(kind: str, copies, position: int, frames: int, hertz, phase=0.0, spread=0.0, rate: int = RATE, blocks: int = 1,
         step: int = 1) -> np.ndarray:
    """float64 (blocks * frames, V): row r is frame position + r * step; hertz / phase / spread are (1 | blocks, V | 1) rows, row b
    serving the `frames` output rows of block b"""
    rows = [np.atleast_2d(np.asarray(x, dtype=np.float64)) for x in (hertz, phase, spread)]
    out = []
    for b in range(blocks):
        hz, ph, sp = (r[b if r.shape[0] > 1 else 0][None, :] for r in rows)
        n = np.arange(position + b * frames * step, position + (b + 1) * frames * step, step, dtype=np.int64)[:, None]
        out.append(blep_sum(kind, n, rate, hz, ph, sp, copies))
    width = max(o.shape[1] for o in out)
    return np.concatenate([np.broadcast_to(o, (o.shape[0], width)) for o in out], axis=0)


def alias_ratio_db(x) -> float:
    """power outside the harmonics over power in them, in dB, of 4096 frames at hertz = rate * 37 / 1024: an unwindowed rfft, the
    harmonics (and the aliases that fold onto them: 37 and 1024 are coprime, so only every 1024th partial does) in the bins
    k % 148 == 0, every other bin above 0 an alias"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    assert x.shape[0] == 4096
    p = np.abs(np.fft.rfft(x)) ** 2
    k = np.arange(p.shape[0])
    harmonic = k % 148 == 0
    alias = ~harmonic                                                          # (every one of them above bin 0)
    return float(10.0 * np.log10(p[alias].sum() / p[harmonic].sum()))


class BlepOsc(R.Node):
    """takes part in render_stream's cache and context semantics like any oracle node; `copies` is read at every evaluation"""

    def __init__(self, kind, copies, hertz=None, phase=None, spread=None):
        super().__init__(hertz=hertz, phase=phase, spread=spread)
        self.kind, self.copies = kind, copies

    def eval(self, position, frames, channels, rate):
        phase = self._ctrl('phase', position, channels, rate)
        hertz = self._ctrl('hertz', position, channels, rate)
        spread = self._ctrl('spread', position, channels, rate)
        return blep_sum(self.kind, R.frame_range(position, frames), rate, hertz, phase, spread, self.copies)
