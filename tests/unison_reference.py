"""numpy restatement of the unison oscillators (signals_amd/chain/ext.py: UnisonSine / UnisonSquare / UnisonSawtooth /
UnisonTriangle), build-defined nodes the reference has no counterpart of, on oracle.chain_ref's own functions.  float64 arithmetic
in numpy's operator order, no fused multiply-add.  `copies` is (U, 2): column 0 the relative detune d[u], column 1 the phase
offset p[u] in cycles; hertz, phase and spread are read at block rate:

    r_u = 1.0 + spread * d[u]
    h_u = hertz * r_u
    q_u = phase + p[u]
    t_u = frame_range / rate * h_u + q_u           # Osc._eval's expression, osc.py:26-33
    s   = ((w(t_0) + w(t_1)) + w(t_2)) + ...       # u ascending, w = osc_wave of the kind
    out = s / U

`unison` renders K blocks of N frames with per-block parameter rows, the way a node reads its control ports once per block
(forward_at_block_rate); `UnisonOsc` is the same as an oracle Node, so that graphs with filters around it render as the
reference's pull protocol would."""
import numpy as np

from oracle import chain_ref as R

RATE = 48000
DETUNE = (-0.11002313, -0.06288439, -0.01952356, 0.0, 0.01991221, 0.06216538, 0.10745242)


def default_copies() -> np.ndarray:
    return np.stack([np.array(DETUNE), np.mod(np.arange(7) * 0.6180339887498949, 1.0)], axis=1)


def unison_sum(kind: str, frames: np.ndarray, rate: int, hertz, phase, spread, copies) -> np.ndarray:
    """the definition over a column of frame numbers (int64 (rows, 1)) and one row of each control: float64 (rows, V | 1)"""
    copies = np.asarray(copies, dtype=np.float64)
    s = None
    for d, p in copies:
        r = 1.0 + spread * d
        h = hertz * r
        q = phase + p
        w = R.osc_wave(kind, frames / rate * h + q)
        s = w if s is None else s + w
    return s / copies.shape[0]


def unison(kind: str, copies, position: int, frames: int, hertz, phase=0.0, spread=0.0, rate: int = RATE, blocks: int = 1,
           step: int = 1) -> np.ndarray:
    """float64 (blocks * frames, V): row r is frame position + r * step; hertz / phase / spread are (1 | blocks, V | 1) rows, row b
    serving the `frames` output rows of block b"""
    rows = [np.atleast_2d(np.asarray(x, dtype=np.float64)) for x in (hertz, phase, spread)]
    out = []
    for b in range(blocks):
        hz, ph, sp = (r[b if r.shape[0] > 1 else 0][None, :] for r in rows)
        n = np.arange(position + b * frames * step, position + (b + 1) * frames * step, step, dtype=np.int64)[:, None]
        out.append(unison_sum(kind, n, rate, hz, ph, sp, copies))
    width = max(o.shape[1] for o in out)
    return np.concatenate([np.broadcast_to(o, (o.shape[0], width)) for o in out], axis=0)


class UnisonOsc(R.Node):
    """takes part in render_stream's cache and context semantics like any oracle node; `copies` is read at every evaluation"""

    def __init__(self, kind, copies, hertz=None, phase=None, spread=None):
        super().__init__(hertz=hertz, phase=phase, spread=spread)
        self.kind, self.copies = kind, copies

    def eval(self, position, frames, channels, rate):
        phase = self._ctrl('phase', position, channels, rate)
        hertz = self._ctrl('hertz', position, channels, rate)
        spread = self._ctrl('spread', position, channels, rate)
        return unison_sum(self.kind, R.frame_range(position, frames), rate, hertz, phase, spread, self.copies)
