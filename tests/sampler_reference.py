"""numpy restatement of the sample-playback node (signals_amd/chain/ext.py: Sampler), the build-defined node the reference has no
counterpart of.  float64 arithmetic in numpy's operator order, no fused multiply-add; the table is what the device holds,
float32(table) widened to float64.  For absolute frame n and voice v:

    q  = n / rate                                  # osc.py's order: one IEEE divide
    e  = q - gate_on[v]
    s  = e * rate
    u  = s * ratio[v] + offset[v]                  # two roundings
    not (e >= 0)           -> out = 0              # before the trigger; a NaN gate is silence
    u is NaN or +-inf      -> out = NaN            # no index is formed from it
    no loop:  u < 0 or u > T - 1 -> out = 0        # outside the recording
              i = floor(u); f = u - i; j = min(i + 1, T - 1)
    loop:     u < 0 -> out = 0
              L = loop_end - loop_start
              u >= loop_end:  c = floor((u - loop_start) / L);  u = (u - loop_start) - c * L + loop_start
                              if that rounds to u >= loop_end:  u = loop_start
                              (likewise if it falls below loop_start: from 2**53 frames on the rounded quotient can exceed the true one)
              i = floor(u); f = u - i; j = (i + 1 >= loop_end) ? loop_start : i + 1
    w   = clip(floor(select[v]), 0, W - 1)         # NaN -> 0; unplugged -> 0
    out = tbl[i, w] + f * (tbl[j, w] - tbl[i, w])

`read_position` is the first four lines, `locate` the index part (what tests/native/sampler_index.cpp prints for the header compiled
for the host), `sampler` K blocks of N frames with per-block control rows, the way the node reads its ports once per block
(forward_at_block_rate); `sampler_loop` is the same definition one sample at a time in Python floats, for the host test;
`oracle_node` is the node for oracle.chain_ref graphs."""
import math

import numpy as np

RATE = 48000
SILENCE, NAN, READ = 0, 1, 2


def column(select, waves: int) -> np.ndarray:
    s = np.floor(np.asarray(select, dtype=np.float64))
    return np.clip(np.where(np.isnan(s), 0.0, s), 0, waves - 1).astype(np.int64)


def read_position(n, rate, gate_on, ratio, offset):
    """(u, on): float64 read positions and whether the trigger has passed, broadcast over n (rows, 1) and the (1, V | 1) rows"""
    n = np.asarray(n, dtype=np.int64)
    gate_on, ratio, offset = (np.asarray(x, dtype=np.float64) for x in (gate_on, ratio, offset))
    with np.errstate(invalid='ignore', over='ignore'):
        q = n / rate
        e = q - gate_on
        s = e * rate
        u = s * ratio + offset
        on = e >= 0
    return u, on


def locate(u, frames: int, loop_start: int = 0, loop_end: int = 0):
    """(kind, i, j, f) of read positions u: kind SILENCE | NAN | READ; i, j int64 and f float64, all 0 where nothing is read"""
    u = np.asarray(u, dtype=np.float64)
    finite = np.isfinite(u)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        if loop_end == 0:
            outside = (u < 0) | (u > frames - 1)
        else:
            outside = u < 0
        read = finite & ~outside
        p = np.where(read, u, 0.0)
        if loop_end != 0:
            lo, hi = float(loop_start), float(loop_end)
            L = hi - lo
            c = np.floor((p - lo) / L)
            wrapped = (p - lo) - c * L + lo
            wrapped = np.where((wrapped >= hi) | (wrapped < lo), lo, wrapped)
            p = np.where(p >= hi, wrapped, p)
        whole = np.floor(p)
        f = p - whole
    i = whole.astype(np.int64)
    if loop_end == 0:
        j = np.minimum(i + 1, frames - 1)
    else:
        j = np.where(i + 1 >= loop_end, loop_start, i + 1)
    kind = np.where(read, READ, np.where(finite, SILENCE, NAN))
    return kind, np.where(read, i, 0), np.where(read, j, 0), np.where(read, f, 0.0)


def play(table, n, rate, ratio, offset, gate_on, select, loop_start: int = 0, loop_end: int = 0) -> np.ndarray:
    """float64 (rows, V): the frames n (rows, 1) under one set of (1, V | 1) control rows"""
    tbl = np.asarray(table).astype(np.float32).astype(np.float64)
    T, W = tbl.shape
    u, on = read_position(n, rate, gate_on, ratio, offset)
    kind, i, j, f = locate(u, T, loop_start, loop_end)
    w = np.atleast_2d(column(select, W))
    shape = np.broadcast_shapes(kind.shape, w.shape)
    a, b = tbl[i, w], tbl[j, w]
    value = a + f * (b - a)
    out = np.where(kind == READ, value, np.where(kind == NAN, np.nan, 0.0))
    return np.array(np.broadcast_to(np.where(on, out, 0.0), shape))


def sampler(table, position: int, frames: int, ratio, offset=0.0, gate_on=0.0, select=0.0, loop_start: int = 0, loop_end: int = 0,
            rate: int = RATE, blocks: int = 1, step: int = 1) -> np.ndarray:
    """float64 (blocks * frames, V): row r is frame position + r * step; ratio / offset / gate_on / select are (1 | blocks, V | 1)
    rows, row b serving the `frames` output rows of block b"""
    rows = [np.atleast_2d(np.asarray(x, dtype=np.float64)) for x in (ratio, offset, gate_on, select)]
    out = []
    for b in range(blocks):
        ra, of, ga, se = (r[b if r.shape[0] > 1 else 0][None, :] for r in rows)
        n = np.arange(position + b * frames * step, position + (b + 1) * frames * step, step, dtype=np.int64)[:, None]
        out.append(play(table, n, rate, ra, of, ga, se, loop_start, loop_end))
    width = max(o.shape[1] for o in out)
    return np.concatenate([np.broadcast_to(o, (o.shape[0], width)) for o in out], axis=0)


def sampler_loop(table, n: int, rate: int, ratio: float, offset: float, gate_on: float, select: float = 0.0,
                 loop_start: int = 0, loop_end: int = 0) -> float:
    """one sample, straight from the definition, in Python floats"""
    tbl = [[float(np.float32(x)) for x in row] for row in np.asarray(table)]
    T, W = len(tbl), len(tbl[0])
    q = n / rate
    e = q - gate_on
    s = e * rate
    u = s * ratio + offset
    if not e >= 0:
        return 0.0
    if math.isnan(u) or math.isinf(u):
        return math.nan
    if u < 0:
        return 0.0
    if loop_end == 0:
        if u > T - 1:
            return 0.0
        i = math.floor(u)
        f = u - i
        j = min(i + 1, T - 1)
    else:
        L = loop_end - loop_start
        if u >= loop_end:
            c = math.floor((u - loop_start) / L)
            u = (u - loop_start) - c * L + loop_start
            if u >= loop_end or u < loop_start:
                u = float(loop_start)
        i = math.floor(u)
        f = u - i
        j = loop_start if i + 1 >= loop_end else i + 1
    w = 0 if math.isnan(select) else int(min(max(math.floor(select), 0), W - 1))
    return tbl[i][w] + f * (tbl[j][w] - tbl[i][w])


def burst(frames: int, recordings: int = 1, seed: int = 0) -> np.ndarray:
    """(frames, recordings): decaying sine bursts within +-1, one pitch per recording -- a table with a shape a test can recognise"""
    rng = np.random.default_rng(seed)
    k = np.arange(frames)[:, None] / max(frames - 1, 1)
    cycles = rng.uniform(3.0, 9.0, (1, recordings))
    return np.sin(2.0 * np.pi * cycles * k + rng.uniform(0, 1, (1, recordings))) * np.exp(-3.0 * k) * rng.uniform(0.5, 1.0, (1, recordings))


def oracle_node():
    """the oracle Node class of the sampler (imported lazily: the functions above need numpy alone)"""
    from oracle import chain_ref as R

    class Sampler(R.Node):
        """takes part in render_stream's cache semantics like any oracle node"""

        def __init__(self, table, ratio=None, offset=None, gate_on=None, select=None, loop_start=0, loop_end=0):
            super().__init__(ratio=ratio, offset=offset, gate_on=gate_on, select=select)
            self.table, self.loop_start, self.loop_end = table, loop_start, loop_end

        def eval(self, position, frames, channels, rate):
            ratio, offset, gate_on, select = (self._ctrl(p, position, channels, rate) for p in ('ratio', 'offset', 'gate_on', 'select'))
            return play(self.table, R.frame_range(position, frames), rate, ratio, offset, gate_on, select, self.loop_start, self.loop_end)
    return Sampler
