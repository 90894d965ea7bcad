"""numpy restatement of the wavetable oscillator (signals_amd/chain/ext.py: Wavetable), the build-defined node the reference has no
counterpart of.  float64 arithmetic in numpy's operator order, no fused multiply-add; the table is what the device holds,
float32(table) widened to float64:

    t  = frame_range / rate * hertz + phase        # Osc._eval's expression, osc.py:26-33
    m  = np.mod(t, 1.0)                            # in [0, 1]: the rounded sum reaches 1.0 for t in (-2^-54, 0)
    u  = m * T;  i = floor(u);  f = u - i          # exact (T a power of two)
    i0 = i & (T-1);  i1 = (i+1) & (T-1)            # u == T wraps to entry 0
    w  = clip(floor(select), 0, W-1)               # per voice; NaN -> 0; unplugged -> 0
    out = tbl[i0, w] + f * (tbl[i1, w] - tbl[i0, w])

`wavetable` renders K blocks of N frames with per-block parameter rows, the way a node reads its control ports once per block
(forward_at_block_rate); `wavetable_loop` is the same definition one sample at a time in Python floats, for the host test."""
import math

import numpy as np

RATE = 48000


def column(select, waves: int) -> np.ndarray:
    s = np.floor(np.asarray(select, dtype=np.float64))
    return np.clip(np.where(np.isnan(s), 0.0, s), 0, waves - 1).astype(np.int64)


def lookup(table, t, select=0.0) -> np.ndarray:
    """the table read at phase `t` (cycles, float64 (rows, V | 1)), column row `select` (1, V | 1): float64"""
    tbl = np.asarray(table).astype(np.float32).astype(np.float64)
    T, W = tbl.shape
    m = np.mod(np.asarray(t, dtype=np.float64), 1.0)
    u = m * T
    i = np.floor(u)
    f = u - i
    i = i.astype(np.int64)
    i0, i1 = i & (T - 1), (i + 1) & (T - 1)
    w = np.atleast_2d(column(select, W))                   # (1, V | 1): broadcasts against the (rows, V | 1) indices
    lo, hi = tbl[i0, w], tbl[i1, w]
    return lo + f * (hi - lo)


def wavetable(table, position: int, frames: int, hertz, phase=0.0, select=0.0, rate: int = RATE, blocks: int = 1, step: int = 1) -> np.ndarray:
    """float64 (blocks * frames, V): row r is frame position + r * step; hertz / phase / select are (1 | blocks, V | 1) rows, row b
    serving the `frames` output rows of block b"""
    rows = [np.atleast_2d(np.asarray(x, dtype=np.float64)) for x in (hertz, phase, select)]
    out = []
    for b in range(blocks):
        hz, ph, sel = (r[b if r.shape[0] > 1 else 0][None, :] for r in rows)
        frame_range = (np.arange(position + b * frames * step, position + (b + 1) * frames * step, step))[:, None]
        t = frame_range / rate * hz + ph
        out.append(lookup(table, t, sel))
    width = max(o.shape[1] for o in out)
    return np.concatenate([np.broadcast_to(o, (o.shape[0], width)) for o in out], axis=0)


def wavetable_loop(table, t: float, select: float = 0.0) -> float:
    """one sample, straight from the definition"""
    tbl = [[float(np.float32(x)) for x in row] for row in np.asarray(table)]
    T, W = len(tbl), len(tbl[0])
    m = float(np.mod(np.float64(t), 1.0))
    u = m * T
    i = math.floor(u)
    f = u - i
    w = 0 if math.isnan(select) else min(max(math.floor(select), 0), W - 1)
    lo, hi = tbl[i % T][w], tbl[(i + 1) % T][w]
    return lo + f * (hi - lo)


def band_limited_saw(points: int, harmonics: int) -> np.ndarray:
    """(points, 1): a sawtooth's first `harmonics` partials, one period -- a continuous table"""
    k = np.arange(points)[:, None] / points
    h = np.arange(1, harmonics + 1)[None, :]
    return (2.0 / np.pi * np.sum(np.sin(2.0 * np.pi * k * h) / h * (-1.0) ** (h + 1), axis=1, keepdims=True))


def oracle_node():
    """the oracle Node class of the wavetable oscillator (imported lazily: the functions above need numpy alone)"""
    from oracle import chain_ref as R

    class Wavetable(R.Node):
        """takes part in render_stream's cache and context semantics like any oracle node"""

        def __init__(self, table, hertz=None, phase=None, select=None):
            super().__init__(hertz=hertz, phase=phase, select=select)
            self.table = table

        def eval(self, position, frames, channels, rate):
            phase = self._ctrl('phase', position, channels, rate)
            hertz = self._ctrl('hertz', position, channels, rate)
            select = self._ctrl('select', position, channels, rate)
            return lookup(self.table, R.osc_cycles(position, frames, rate, hertz, phase), select)
    return Wavetable
