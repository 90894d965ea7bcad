"""Case tables and float64 references for the base per-node kernels (elementwise.hip, sum_bus.hip, mix_matrix.hip, adsr.hip and
the plain osc_bank_kernel), shared by tests/test_base_kernels_host.py and tests/test_gpu_base_kernels.py.  numpy only.

Every buffer is described by `view(array, pad, ld_extra)`: `pad + V + ld_extra` columns wide, viewed from column `pad`; the GPU
test materialises it inside one allocation and fills what lies outside the view with a sentinel.  The references are the
restatements of oracle/chain_ref.py.  `expected_variant` restates the dispatch rules of the .hip files: it says which kernel a
case is meant to reach (a census for the host test), and never decides pass or fail against a kernel.

Layouts (pad, ld_extra): contig (0, 0); pad4 (4, 0): still 16-byte aligned; pad1 (1, 3): only the base is misaligned, the leading
dimension stays a multiple of 4; ld4 (0, 4); ld1 (0, 1): only the leading dimension breaks the 16-byte rows.  The tables were
drawn once as pairwise coverings of their factors (plus the rows that walk each fast path over its tile edges, which need three
factors at once) and are kept as listed."""
import collections
import zlib

import numpy as np

from oracle import chain_ref as R

RATE = 48000
HOUR = 172_800_000
View = collections.namedtuple('View', 'array pad ld_extra')
LAYOUT = {'contig': (0, 0), 'pad4': (4, 0), 'pad1': (1, 3), 'ld4': (0, 4), 'ld1': (0, 1)}
CAPS = {'elementwise': 150, 'sum_bus': 130, 'mix_matrix': 8, 'adsr': 50, 'osc': 40}      # launches of distinct cases per kernel


def view(array, pad=0, ld_extra=0) -> View:
    """`array` (2-D) as the columns [pad, pad + V) of a buffer pad + V + ld_extra columns wide"""
    array = np.ascontiguousarray(array)
    assert array.ndim == 2 and pad >= 0 and ld_extra >= 0
    return View(array, pad, ld_extra)


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32)


def ld(v: View) -> int:
    return v.pad + v.array.shape[1] + v.ld_extra


def vec4_rows(v: View) -> bool:
    """every row of the view starts on a 4-element boundary of a 4-element-aligned allocation"""
    return v.pad % 4 == 0 and ld(v) % 4 == 0


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


DTYPE = {'f32': np.float32, 'f64': np.float64}

# ---------------------------------------------------------------------------------------------------------------- elementwise
# (op, rows, V, layout, control, dtypes).  layout: one of LAYOUT for the audio operands and `out` alike, or out_ld4 / out_pad1
# (only `out` laid out so) / in_pad4 (only the audio operands).  control (Gain, Amp: b; Mix: c), float64: s11 (1,1), row (1,V),
# blkL (rows / L, V) per-block rows of block length L, frame (rows, V), col (rows, 1).  dtypes: f32 all audio float32; a64:
# operand a float64, out float32; o64: out float64.  rows 18, 20 and 32 are there for the per-block operands (no row count of
# the list is a multiple of 6, and 16 rows leave blocks of 4 and 8 without a tail).
EW_LAYOUT = dict({k: (v, v) for k, v in LAYOUT.items()}, out_ld4=((0, 0), (0, 4)), out_pad1=((0, 0), (1, 3)), in_pad4=((4, 0), (0, 0)))
EW_GRID_STRIDE = ('Gain', 16400, 257, 'contig', 'row', 'f32')       # 4214800 elements > 16384 workgroups x 256: the generic loop iterates
EW_CASES = (
    # each fast kernel over its row and column tile edges
    ('Gain', 1, 4, 'contig', 's11', 'f32'), ('Gain', 3, 252, 'pad4', 'row', 'f32'), ('Gain', 4, 256, 'ld4', 's11', 'f32'),
    ('Gain', 15, 260, 'out_ld4', 'row', 'f32'), ('Gain', 16, 4, 'in_pad4', 's11', 'f32'), ('Gain', 17, 252, 'contig', 'row', 'f32'),
    ('Gain', 67, 256, 'pad4', 's11', 'f32'), ('Gain', 1, 256, 'ld4', 'row', 'f32'), ('Gain', 3, 260, 'out_ld4', 's11', 'f32'),
    ('Gain', 4, 4, 'in_pad4', 'row', 'f32'), ('Gain', 15, 252, 'contig', 's11', 'f32'), ('Gain', 16, 256, 'pad4', 'row', 'f32'),
    ('Gain', 17, 260, 'ld4', 's11', 'f32'), ('Gain', 67, 4, 'out_ld4', 'row', 'f32'), ('Gain', 20, 260, 'in_pad4', 'blk4', 'f32'),
    ('Gain', 32, 256, 'contig', 'blk8', 'f32'), ('Gain', 67, 260, 'contig', 'row', 'f32'), ('Mix', 1, 252, 'pad4', 's11', 'f32'),
    ('Mix', 3, 256, 'ld4', 'row', 'f32'), ('Mix', 4, 260, 'out_ld4', 's11', 'f32'), ('Mix', 15, 4, 'in_pad4', 'row', 'f32'),
    ('Mix', 16, 252, 'contig', 's11', 'f32'), ('Mix', 17, 256, 'pad4', 'row', 'f32'), ('Mix', 67, 260, 'ld4', 's11', 'f32'),
    ('Mix', 1, 260, 'out_ld4', 'row', 'f32'), ('Mix', 3, 4, 'in_pad4', 's11', 'f32'), ('Mix', 4, 252, 'contig', 'row', 'f32'),
    ('Mix', 15, 256, 'pad4', 's11', 'f32'), ('Mix', 16, 260, 'ld4', 'row', 'f32'), ('Mix', 17, 4, 'out_ld4', 's11', 'f32'),
    ('Mix', 67, 252, 'in_pad4', 'row', 'f32'), ('Mix', 20, 260, 'contig', 'blk4', 'f32'), ('Mix', 32, 256, 'pad4', 'blk8', 'f32'),
    ('Mix', 67, 260, 'contig', 'row', 'f32'), ('RingMod', 1, 256, 'ld4', 'none', 'f32'), ('RingMod', 3, 260, 'out_ld4', 'none', 'f32'),
    ('RingMod', 4, 4, 'in_pad4', 'none', 'f32'), ('RingMod', 15, 252, 'contig', 'none', 'f32'),
    ('RingMod', 16, 256, 'pad4', 'none', 'f32'), ('RingMod', 17, 260, 'ld4', 'none', 'f32'),
    ('RingMod', 67, 4, 'out_ld4', 'none', 'f32'), ('RingMod', 1, 4, 'in_pad4', 'none', 'f32'),
    ('RingMod', 3, 252, 'contig', 'none', 'f32'), ('RingMod', 4, 256, 'pad4', 'none', 'f32'),
    ('RingMod', 15, 260, 'ld4', 'none', 'f32'), ('RingMod', 16, 4, 'out_ld4', 'none', 'f32'),
    ('RingMod', 17, 252, 'in_pad4', 'none', 'f32'), ('RingMod', 67, 256, 'contig', 'none', 'f32'),
    ('Amp', 1, 260, 'pad4', 's11', 'f32'), ('Amp', 3, 4, 'ld4', 'row', 'f32'), ('Amp', 4, 252, 'out_ld4', 's11', 'f32'),
    ('Amp', 15, 256, 'in_pad4', 'row', 'f32'), ('Amp', 16, 260, 'contig', 's11', 'f32'), ('Amp', 17, 4, 'pad4', 'row', 'f32'),
    ('Amp', 67, 252, 'ld4', 's11', 'f32'), ('Amp', 1, 252, 'out_ld4', 'row', 'f32'), ('Amp', 3, 256, 'in_pad4', 's11', 'f32'),
    ('Amp', 4, 260, 'contig', 'row', 'f32'), ('Amp', 15, 4, 'pad4', 's11', 'f32'), ('Amp', 16, 252, 'ld4', 'row', 'f32'),
    ('Amp', 17, 256, 'out_ld4', 's11', 'f32'), ('Amp', 67, 260, 'in_pad4', 'row', 'f32'), ('Amp', 20, 260, 'contig', 'blk4', 'f32'),
    ('Amp', 32, 256, 'pad4', 'blk8', 'f32'), ('Amp', 67, 4, 'contig', 'row', 'f32'),
    # pairwise covering of (op, rows, V, layout, control, dtypes)
    ('Amp', 1, 252, 'out_ld4', 'col', 'a64'), ('Amp', 3, 3, 'contig', 'frame', 'a64'), ('Amp', 3, 4, 'ld1', 's11', 'a64'),
    ('Amp', 3, 252, 'in_pad4', 'col', 'a64'), ('Amp', 3, 260, 'ld4', 'row', 'a64'), ('Amp', 4, 1, 'pad1', 'frame', 'o64'),
    ('Amp', 15, 4, 'ld1', 's11', 'a64'), ('Amp', 15, 4, 'pad4', 'frame', 'f32'), ('Amp', 15, 4, 'contig', 'col', 'a64'),
    ('Amp', 15, 260, 'out_ld4', 'row', 'o64'), ('Amp', 16, 252, 'ld1', 'blk8', 'a64'), ('Amp', 16, 252, 'ld1', 'frame', 'a64'),
    ('Amp', 16, 260, 'contig', 'blk8', 'o64'), ('Amp', 17, 256, 'in_pad4', 's11', 'o64'), ('Amp', 18, 1, 'pad4', 'blk6', 'o64'),
    ('Amp', 18, 4, 'out_ld4', 'blk6', 'a64'), ('Amp', 18, 256, 'pad1', 'blk6', 'o64'), ('Amp', 18, 260, 'in_pad4', 'blk6', 'o64'),
    ('Amp', 20, 1, 'contig', 'blk4', 'f32'), ('Amp', 20, 3, 'ld4', 'blk4', 'o64'), ('Amp', 20, 256, 'out_pad1', 'blk4', 'f32'),
    ('Amp', 32, 1, 'ld1', 'blk4', 'o64'), ('Amp', 32, 4, 'pad4', 'blk8', 'a64'), ('Amp', 32, 252, 'in_pad4', 'blk8', 'o64'),
    ('Amp', 32, 260, 'ld4', 'blk8', 'o64'), ('Amp', 67, 3, 'pad4', 'frame', 'f32'), ('Amp', 67, 252, 'out_ld4', 's11', 'f32'),
    ('Amp', 67, 256, 'in_pad4', 'row', 'a64'), ('Mix', 1, 1, 'ld4', 'frame', 'o64'), ('Mix', 1, 252, 'pad1', 'row', 'f32'),
    ('Mix', 1, 256, 'contig', 'row', 'o64'), ('Mix', 1, 260, 'ld1', 's11', 'f32'), ('Mix', 3, 4, 'out_ld4', 'row', 'f32'),
    ('Mix', 3, 256, 'pad4', 'col', 'o64'), ('Mix', 4, 4, 'out_pad1', 'row', 'o64'), ('Mix', 4, 256, 'ld1', 'col', 'a64'),
    ('Mix', 4, 256, 'contig', 's11', 'f32'), ('Mix', 15, 1, 'in_pad4', 'row', 'f32'), ('Mix', 16, 3, 'pad1', 's11', 'a64'),
    ('Mix', 16, 4, 'pad4', 'blk4', 'a64'), ('Mix', 17, 1, 'out_ld4', 'frame', 'f32'), ('Mix', 17, 4, 'pad4', 'row', 'f32'),
    ('Mix', 17, 252, 'contig', 'row', 'f32'), ('Mix', 17, 260, 'out_pad1', 'frame', 'a64'), ('Mix', 18, 252, 'ld4', 'blk6', 'o64'),
    ('Mix', 20, 4, 'in_pad4', 'blk4', 'a64'), ('Mix', 20, 252, 'pad1', 'blk4', 'a64'), ('Mix', 32, 3, 'out_ld4', 'blk8', 'f32'),
    ('Mix', 32, 256, 'contig', 'blk4', 'f32'), ('Mix', 67, 4, 'ld4', 's11', 'f32'), ('Mix', 67, 252, 'out_pad1', 's11', 'f32'),
    ('Mix', 67, 260, 'pad1', 'col', 'f32'), ('Gain', 1, 3, 'out_pad1', 'col', 'o64'), ('Gain', 1, 4, 'in_pad4', 'frame', 'o64'),
    ('Gain', 3, 1, 'out_pad1', 's11', 'a64'), ('Gain', 4, 252, 'pad4', 's11', 'f32'), ('Gain', 15, 3, 'pad1', 'row', 'a64'),
    ('Gain', 15, 256, 'ld4', 'frame', 'a64'), ('Gain', 16, 1, 'ld4', 'col', 'f32'), ('Gain', 16, 252, 'out_pad1', 'row', 'o64'),
    ('Gain', 16, 256, 'in_pad4', 'col', 'f32'), ('Gain', 17, 3, 'ld4', 'col', 'a64'), ('Gain', 18, 3, 'contig', 'blk6', 'f32'),
    ('Gain', 18, 4, 'out_pad1', 'blk6', 'o64'), ('Gain', 18, 252, 'ld1', 'blk6', 'f32'), ('Gain', 20, 1, 'ld1', 'blk4', 'a64'),
    ('Gain', 20, 3, 'pad4', 'blk4', 'a64'), ('Gain', 20, 260, 'out_ld4', 'blk4', 'o64'), ('Gain', 32, 1, 'out_pad1', 'blk8', 'o64'),
    ('Gain', 32, 256, 'pad1', 'blk8', 'a64'), ('Gain', 67, 3, 'ld1', 'row', 'o64'), ('RingMod', 1, 260, 'pad4', 'none', 'f32'),
    ('RingMod', 3, 4, 'pad1', 'none', 'f32'), ('RingMod', 4, 3, 'in_pad4', 'none', 'a64'), ('RingMod', 4, 4, 'out_ld4', 'none', 'o64'),
    ('RingMod', 4, 260, 'ld4', 'none', 'f32'), ('RingMod', 15, 252, 'out_pad1', 'none', 'o64'),
    ('RingMod', 16, 256, 'out_ld4', 'none', 'o64'), ('RingMod', 17, 252, 'pad1', 'none', 'a64'),
    ('RingMod', 17, 256, 'ld1', 'none', 'f32'), ('RingMod', 67, 1, 'contig', 'none', 'a64'),
    # a per-block control operand of block length 6 beside an otherwise fast launch: the generic kernel
    ('Gain', 18, 256, 'contig', 'blk6', 'f32'), ('Mix', 18, 260, 'pad4', 'blk6', 'f32'), ('Amp', 18, 252, 'ld4', 'blk6', 'f32'),
    EW_GRID_STRIDE,
)
EW_BLOCK = {'blk4': 4, 'blk8': 8, 'blk6': 6}
Built = collections.namedtuple('Built', 'operands out ref')     # operands: name -> View | None; out: a View of zeros; ref: float64


def ew_build(case) -> Built:
    """operands a, b, c (Views, None where the operation takes none), `out` and the float64 reference of an elementwise case"""
    op, rows, V, layout, control, dtypes = case
    rng = rng_of('ew', case)
    (ipad, ild), (opad, old) = EW_LAYOUT[layout]
    audio = lambda wide: view(rng.uniform(-1.0, 1.0, (rows, V)) if wide else f32(rng.uniform(-1.0, 1.0, (rows, V))), ipad, ild)
    a = audio(dtypes == 'a64')
    ctl = ctl_full = None
    if control != 'none':
        shape = {'s11': (1, 1), 'row': (1, V), 'frame': (rows, V), 'col': (rows, 1)}.get(control) or (rows // EW_BLOCK[control], V)
        lo, hi = {'Gain': (-2.0, 2.0), 'Mix': (0.0, 1.0), 'Amp': (0.5, 3.0)}[op]
        ctl = rng.uniform(lo, hi, shape)
        if op == 'Amp':                                     # whole exponents too: a negative base is a number only under those
            whole = rng.integers(1, 4, shape).astype(np.float64)
            ctl = np.where(rng.integers(0, 3, shape) == 0, whole, ctl)
        ctl_full = np.repeat(ctl, EW_BLOCK[control], axis=0) if control in EW_BLOCK else ctl
    a64 = a.array.astype(np.float64)
    if op == 'Gain':
        b, c, ref = view(ctl), None, R.gain(a64, ctl_full)
    elif op == 'Amp':
        b, c, ref = view(ctl), None, R.amp(a64, ctl_full)
    elif op == 'RingMod':
        b, c = audio(False), None
        ref = R.ringmod(a64, b.array.astype(np.float64))
    else:
        b, c = audio(False), view(ctl)
        ref = R.mix(a64, b.array.astype(np.float64), ctl_full)
    out = view(np.zeros((rows, V), dtype=np.float64 if dtypes == 'o64' else np.float32), opad, old)
    return Built({'a': a, 'b': b, 'c': c}, out, np.broadcast_to(ref, (rows, V)).copy())


def _ew_audio_fast(v: View, rows: int, V: int) -> bool:
    # (a one-row operand reaches the entry with a zero row stride, as a broadcast row: not the fast kernel's audio operand)
    return v.array.dtype == np.float32 and v.array.shape == (rows, V) and rows > 1 and vec4_rows(v)


def _ew_ctrl_fast(v: View, rows: int) -> bool:
    r = v.array.shape[0]
    block = 0 if r in (1, rows) else rows // r
    return v.array.dtype == np.float64 and (r == 1 or (block >= 4 and block % 4 == 0))


# ------------------------------------------------------------------------------------------------------------------- sum_bus
# (V, rows, C, x dtype, out dtype, x layout, out layout, gains ld_extra).  C 'mono': one channel without gains; 3, 5, 7: split
# by the wrapper into 2+1, 4+1, 4+2+1.  out layout: contig, or padded = (1, 2).
BUS_OUT_LAYOUT = {'contig': (0, 0), 'padded': (1, 2)}
BUS_CAP = (256, 32773, 2, 'f32', 'f32', 'contig', 'contig', 0)     # 8194 row groups of 4 > 2048 workgroups x 4 waves, ragged tail group
BUS_CASES = (
    # the fast kernels (float32 in, C <= 2, V = 256 CHUNKS, 16-byte rows) over ragged row groups; pad1 on V = 256 falls off them
    (256, 1, 'mono', 'f32', 'f32', 'contig', 'contig', 0), (256, 3, 1, 'f32', 'f32', 'pad4', 'contig', 0),
    (256, 5, 2, 'f32', 'f64', 'ld4', 'padded', 3), (256, 7, 2, 'f32', 'f32', 'contig', 'contig', 0),
    (256, 9, 3, 'f32', 'f32', 'contig', 'padded', 0), (256, 33, 7, 'f32', 'f32', 'pad4', 'contig', 3),
    (256, 5, 2, 'f32', 'f32', 'pad1', 'contig', 0), (256, 7, 'mono', 'f32', 'f32', 'pad1', 'contig', 0),
    (256, 5, 2, 'f32', 'f32', 'ld1', 'contig', 0),
    (512, 4, 'mono', 'f32', 'f64', 'pad4', 'contig', 0), (512, 5, 1, 'f32', 'f32', 'contig', 'padded', 3),
    (512, 9, 2, 'f32', 'f32', 'ld4', 'contig', 0), (512, 33, 2, 'f32', 'f64', 'contig', 'contig', 0),
    (768, 3, 2, 'f32', 'f32', 'contig', 'contig', 3), (768, 7, 2, 'f32', 'f32', 'pad4', 'padded', 0),
    (768, 8, 1, 'f32', 'f64', 'ld4', 'contig', 0), (768, 33, 'mono', 'f32', 'f32', 'contig', 'contig', 0),
    (1024, 1, 1, 'f32', 'f32', 'contig', 'contig', 0), (1024, 5, 2, 'f32', 'f32', 'pad4', 'contig', 0),
    (1024, 7, 'mono', 'f32', 'f64', 'ld4', 'padded', 0), (1024, 9, 2, 'f32', 'f32', 'contig', 'contig', 0),
    (1024, 33, 3, 'f32', 'f32', 'contig', 'contig', 0), (1024, 3, 5, 'f32', 'f32', 'contig', 'contig', 0),
    # pairwise covering of the eight factors
    (1, 1, 5, 'f32', 'f64', 'pad1', 'contig', 0), (1, 3, 3, 'f32', 'f32', 'pad4', 'contig', 0),
    (1, 4, 7, 'f32', 'f32', 'ld1', 'contig', 3), (1, 5, 5, 'f64', 'f32', 'ld4', 'padded', 0),
    (1, 7, 2, 'f64', 'f64', 'ld1', 'contig', 0), (1, 8, 'mono', 'f32', 'f32', 'ld1', 'padded', 0),
    (1, 9, 1, 'f32', 'f64', 'pad1', 'padded', 0), (1, 33, 4, 'f32', 'f64', 'contig', 'padded', 0),
    (3, 1, 7, 'f32', 'f64', 'ld4', 'contig', 0), (3, 3, 1, 'f64', 'f64', 'ld1', 'padded', 3),
    (3, 4, 2, 'f64', 'f64', 'pad4', 'contig', 3), (3, 5, 3, 'f32', 'f64', 'pad1', 'padded', 3),
    (3, 7, 4, 'f64', 'f32', 'contig', 'padded', 3), (3, 8, 5, 'f64', 'f32', 'contig', 'padded', 3),
    (3, 9, 'mono', 'f64', 'f32', 'pad4', 'contig', 0), (3, 33, 1, 'f32', 'f32', 'ld4', 'contig', 0),
    (4, 1, 5, 'f64', 'f32', 'contig', 'padded', 3), (4, 3, 1, 'f64', 'f32', 'ld4', 'contig', 3),
    (4, 4, 3, 'f64', 'f32', 'ld4', 'padded', 0), (4, 5, 4, 'f32', 'f64', 'contig', 'contig', 0),
    (4, 7, 7, 'f32', 'f32', 'ld1', 'padded', 3), (4, 8, 'mono', 'f64', 'f64', 'pad4', 'contig', 0),
    (4, 9, 5, 'f64', 'f64', 'pad4', 'padded', 3), (4, 33, 2, 'f32', 'f32', 'pad1', 'padded', 3),
    (255, 1, 7, 'f32', 'f32', 'ld4', 'padded', 0), (255, 3, 1, 'f32', 'f64', 'ld1', 'padded', 0),
    (255, 4, 4, 'f64', 'f32', 'pad4', 'padded', 0), (255, 5, 'mono', 'f64', 'f32', 'contig', 'padded', 0),
    (255, 7, 5, 'f32', 'f64', 'pad1', 'contig', 3), (255, 8, 4, 'f64', 'f64', 'pad4', 'contig', 0),
    (255, 9, 2, 'f64', 'f64', 'ld4', 'contig', 3), (255, 33, 3, 'f32', 'f64', 'ld1', 'padded', 0),
    (256, 1, 1, 'f64', 'f64', 'pad4', 'contig', 0), (256, 3, 4, 'f32', 'f64', 'ld4', 'padded', 3),
    (256, 4, 2, 'f64', 'f32', 'pad4', 'padded', 0), (256, 5, 7, 'f32', 'f32', 'ld1', 'contig', 0),
    (256, 7, 'mono', 'f64', 'f64', 'contig', 'contig', 0), (256, 8, 3, 'f64', 'f32', 'ld1', 'contig', 0),
    (256, 9, 5, 'f64', 'f32', 'ld1', 'contig', 0), (256, 33, 7, 'f32', 'f64', 'pad1', 'padded', 3),
    (260, 1, 3, 'f64', 'f64', 'pad1', 'contig', 3), (260, 3, 5, 'f64', 'f64', 'ld4', 'padded', 0),
    (260, 4, 'mono', 'f64', 'f64', 'pad1', 'contig', 0), (260, 5, 7, 'f32', 'f64', 'pad4', 'padded', 0),
    (260, 7, 4, 'f32', 'f64', 'pad4', 'contig', 0), (260, 8, 1, 'f32', 'f32', 'contig', 'padded', 3),
    (260, 9, 4, 'f32', 'f32', 'ld1', 'padded', 0), (260, 33, 2, 'f32', 'f32', 'ld4', 'padded', 0),
    (512, 1, 3, 'f32', 'f32', 'pad4', 'padded', 3), (512, 3, 2, 'f32', 'f64', 'contig', 'contig', 0),
    (512, 4, 'mono', 'f32', 'f32', 'ld1', 'padded', 0), (512, 5, 4, 'f64', 'f64', 'pad4', 'padded', 3),
    (512, 7, 1, 'f64', 'f64', 'ld4', 'contig', 0), (512, 8, 7, 'f64', 'f64', 'pad1', 'contig', 0),
    (512, 9, 5, 'f32', 'f32', 'ld1', 'contig', 3), (512, 33, 4, 'f64', 'f32', 'ld4', 'contig', 3),
    (768, 1, 'mono', 'f32', 'f64', 'contig', 'contig', 0), (768, 3, 5, 'f64', 'f32', 'ld4', 'padded', 3),
    (768, 4, 1, 'f32', 'f32', 'pad1', 'padded', 3), (768, 5, 2, 'f64', 'f64', 'ld1', 'contig', 3),
    (768, 7, 3, 'f64', 'f32', 'ld4', 'padded', 0), (768, 8, 3, 'f32', 'f64', 'pad1', 'padded', 0),
    (768, 9, 7, 'f32', 'f64', 'pad4', 'padded', 3), (768, 33, 4, 'f32', 'f32', 'ld1', 'contig', 0),
    (1000, 1, 1, 'f64', 'f64', 'pad1', 'padded', 0), (1000, 3, 'mono', 'f64', 'f32', 'ld1', 'contig', 0),
    (1000, 4, 5, 'f32', 'f64', 'ld4', 'contig', 0), (1000, 5, 4, 'f64', 'f32', 'ld1', 'contig', 0),
    (1000, 7, 2, 'f32', 'f32', 'pad4', 'padded', 0), (1000, 8, 'mono', 'f64', 'f32', 'pad4', 'padded', 0),
    (1000, 9, 3, 'f64', 'f64', 'contig', 'contig', 3), (1000, 33, 7, 'f64', 'f64', 'pad1', 'contig', 3),
    (1024, 1, 2, 'f32', 'f64', 'pad1', 'padded', 0), (1024, 3, 7, 'f64', 'f32', 'contig', 'contig', 0),
    (1024, 4, 1, 'f32', 'f32', 'pad1', 'padded', 0), (1024, 5, 4, 'f64', 'f32', 'contig', 'contig', 0),
    (1024, 7, 3, 'f64', 'f32', 'pad1', 'contig', 0), (1024, 8, 4, 'f32', 'f32', 'ld4', 'contig', 3),
    (1024, 9, 'mono', 'f32', 'f32', 'ld1', 'padded', 0), (1024, 33, 5, 'f64', 'f64', 'pad4', 'contig', 3),
    (1028, 1, 7, 'f32', 'f32', 'ld4', 'contig', 0), (1028, 3, 4, 'f64', 'f32', 'pad1', 'contig', 0),
    (1028, 4, 3, 'f64', 'f32', 'pad4', 'contig', 3), (1028, 5, 1, 'f32', 'f64', 'pad1', 'padded', 3),
    (1028, 7, 1, 'f64', 'f64', 'ld1', 'padded', 3), (1028, 8, 2, 'f32', 'f64', 'contig', 'contig', 3),
    (1028, 9, 5, 'f64', 'f64', 'pad1', 'contig', 0), (1028, 33, 'mono', 'f64', 'f32', 'ld1', 'padded', 0),
    (1280, 1, 4, 'f32', 'f32', 'ld1', 'contig', 3), (1280, 3, 'mono', 'f64', 'f32', 'ld4', 'contig', 0),
    (1280, 4, 7, 'f64', 'f64', 'contig', 'padded', 0), (1280, 5, 2, 'f32', 'f32', 'ld4', 'contig', 0),
    (1280, 7, 3, 'f32', 'f64', 'pad4', 'contig', 0), (1280, 8, 5, 'f64', 'f64', 'pad4', 'padded', 3),
    (1280, 9, 2, 'f32', 'f64', 'pad4', 'padded', 0), (1280, 33, 1, 'f64', 'f64', 'pad1', 'padded', 0),
    BUS_CAP,
)


def bus_widths(C) -> tuple:
    """the bus widths of the native calls `_native.sum_bus` makes for C channels"""
    C = 1 if C == 'mono' else C
    widths = []
    while C:
        widths.append(4 if C >= 4 else (2 if C >= 2 else 1))
        C -= widths[-1]
    return tuple(widths)


def bus_build(case, leg: str) -> Built:
    """operands x and gains (None for 'mono'), `out` and the float64 reference.  leg 'exact': integers in [-8, 8] and gains that
    are multiples of 1/8 in [-2, 2], so that every product and every partial sum in any order is exact in float32 and in float64;
    leg 'random': uniform [-1, 1] (rounded to the buffer's type) under cos / sin pans."""
    V, rows, C, xdt, odt, xlayout, olayout, gld_extra = case
    rng = rng_of('bus', case, leg)
    channels = 1 if C == 'mono' else C
    if leg == 'exact':
        x = rng.integers(-8, 9, (rows, V)).astype(DTYPE[xdt])
        gains = rng.integers(-16, 17, (channels, V)) / 8.0
    else:
        x = rng.uniform(-1.0, 1.0, (rows, V)).astype(DTYPE[xdt])
        pan = rng.uniform(0.0, np.pi / 2, (channels, V))
        gains = np.where(np.arange(channels)[:, None] % 2 == 0, np.cos(pan), np.sin(pan))
    gains = None if C == 'mono' else gains
    ref = R.sum_bus(x.astype(np.float64), gains)
    return Built({'x': view(x, *LAYOUT[xlayout]), 'gains': None if gains is None else view(gains, 0, gld_extra)},
                 view(np.zeros((rows, channels), dtype=DTYPE[odt]), *BUS_OUT_LAYOUT[olayout]), ref)


def bus_bound(built: Built) -> np.ndarray:
    """V * 2^-53 * (|x| @ |g|^T): the bound of a length-V float64 sum of products in any order; plus half a float32 unit in the
    last place of the reference where `out` is float32"""
    x, gains = built.operands['x'].array.astype(np.float64), built.operands['gains']
    V = x.shape[1]
    weight = np.ones((built.ref.shape[1], V)) if gains is None else np.abs(gains.array)
    bound = V * 2.0 ** -53 * (np.abs(x) @ weight.T)
    if built.out.array.dtype == np.float32:
        _, e = np.frexp(built.ref)                                          # |ref| in [2^(e-1), 2^e): ulp 2^(e-24)
        bound = bound + 0.5 * np.ldexp(1.0, np.maximum(e - 24, -149))
    return bound


# ---------------------------------------------------------------------------------------------------------------- mix_matrix
# (rows, V, x layout, out layout) as (pad, ld_extra) pairs.  65565 x 64 is 2049 items and 1051 x 4096 is 2112 items against the
# 2048 wave slots of the persistent launch, each with a ragged last row tile.
MIX_CASES = (
    (1, 64, (0, 0), (0, 0)), (31, 64, (0, 4), (0, 0)), (33, 128, (0, 0), (0, 3)), (33, 128, (4, 0), (0, 0)),
    (31, 64, (4, 4), (1, 3)), (65565, 64, (0, 0), (0, 0)), (1051, 4096, (0, 4), (0, 3)),
)
MIX_REFUSED = (31, 64, (1, 3), (0, 0))                  # x one float off a 16-byte boundary: the entry's alignment check


def mix_matrix_of(leg: str) -> np.ndarray:
    """(64, 64) float32: 'exact' an asymmetric table of multiples of 1/8 in [-2, 2], 'random' normal / 8"""
    if leg == 'exact':
        k, j = np.arange(64)[:, None], np.arange(64)[None, :]
        return (((7 * k + 3 * j + (k * j) % 5) % 33 - 16) / 8.0).astype(np.float32)
    return (np.random.default_rng(5).standard_normal((64, 64)) / 8).astype(np.float32)


def mix_build(case, leg: str) -> Built:
    rows, V, xl, ol = case
    rng = rng_of('mix', case, leg)
    x = (rng.integers(-8, 9, (rows, V)) if leg == 'exact' else rng.standard_normal((rows, V))).astype(np.float32)
    m = mix_matrix_of(leg)
    return Built({'x': view(x, *xl), 'm': view(m)}, view(np.zeros((rows, V), dtype=np.float32), *ol),
                 R.mix_matrix(x.astype(np.float64), m.astype(np.float64)))


# ------------------------------------------------------------------------------------------------------- adsr and adsr_apply
# (entry, V, rows, position, out dtype, layout, control rows).  layout: one of LAYOUT for `out` (and x), or for adsr_apply
# x_padded: x at (1, 3) beside a contiguous out (x alone takes the launch off the 16-byte path); out_padded: out at (4, 4) beside
# a contiguous x (both 16-byte, different leading dimensions).  control rows: 'rows' six (1,V) rows; 'mixed' decay, sustain and
# release as (1,1).
ADSR_LAYOUT = dict({k: (v, v) for k, v in LAYOUT.items()}, x_padded=((1, 3), (0, 0)), out_padded=((0, 0), (4, 4)))
FAR = 2 ** 31 + 5
ADSR_CASES = (
    ('adsr', 1, 1, 0, 'f32', 'contig', 'rows'), ('adsr', 1, 1, FAR, 'f64', 'pad1', 'rows'),
    ('adsr', 1, 15, 0, 'f32', 'ld4', 'rows'), ('adsr', 1, 17, 0, 'f32', 'pad4', 'rows'), ('adsr', 1, 65, 0, 'f32', 'ld1', 'rows'),
    ('adsr', 3, 15, FAR, 'f64', 'pad4', 'mixed'), ('adsr', 3, 16, 0, 'f32', 'ld4', 'rows'),
    ('adsr', 3, 17, 0, 'f32', 'ld1', 'rows'), ('adsr', 3, 64, 0, 'f32', 'pad1', 'rows'), ('adsr', 3, 65, 0, 'f32', 'pad1', 'rows'),
    ('adsr', 4, 1, 0, 'f32', 'pad4', 'rows'), ('adsr', 4, 15, 0, 'f32', 'ld1', 'rows'),
    ('adsr', 4, 16, FAR, 'f64', 'contig', 'rows'), ('adsr', 4, 64, 0, 'f32', 'ld4', 'rows'),
    ('adsr', 65, 1, 0, 'f32', 'ld1', 'rows'), ('adsr', 65, 15, 0, 'f32', 'contig', 'rows'), ('adsr', 65, 16, 0, 'f32', 'pad4', 'rows'),
    ('adsr', 65, 17, 0, 'f64', 'pad1', 'mixed'), ('adsr', 65, 64, FAR, 'f32', 'pad4', 'rows'), ('adsr', 256, 1, 0, 'f32', 'ld4', 'rows'),
    ('adsr', 256, 1, 0, 'f32', 'pad4', 'rows'), ('adsr', 256, 15, 0, 'f32', 'pad1', 'rows'), ('adsr', 256, 64, 0, 'f64', 'ld1', 'rows'),
    ('adsr', 256, 65, FAR, 'f32', 'contig', 'rows'), ('adsr', 260, 1, 0, 'f32', 'pad1', 'rows'),
    ('adsr', 260, 16, 0, 'f32', 'ld1', 'rows'), ('adsr', 260, 64, 0, 'f32', 'contig', 'rows'),
    ('adsr', 260, 65, 0, 'f64', 'ld4', 'mixed'), ('adsr', 260, 17, FAR, 'f64', 'contig', 'rows'),
    ('apply', 1, 16, FAR, 'f32', 'out_padded', 'mixed'),
    ('apply', 1, 64, 0, 'f32', 'out_padded', 'rows'), ('apply', 1, 64, FAR, 'f32', 'x_padded', 'mixed'),
    ('apply', 3, 1, 0, 'f32', 'x_padded', 'rows'), ('apply', 3, 15, 0, 'f32', 'out_padded', 'rows'),
    ('apply', 3, 17, 0, 'f32', 'contig', 'mixed'), ('apply', 4, 16, 0, 'f32', 'pad1', 'mixed'),
    ('apply', 4, 17, 0, 'f32', 'x_padded', 'rows'), ('apply', 4, 65, 0, 'f32', 'out_padded', 'rows'),
    ('apply', 65, 1, 0, 'f32', 'out_padded', 'rows'), ('apply', 65, 17, FAR, 'f32', 'ld4', 'rows'),
    ('apply', 65, 65, 0, 'f32', 'x_padded', 'rows'), ('apply', 256, 1, FAR, 'f32', 'ld1', 'mixed'),
    ('apply', 256, 16, 0, 'f32', 'x_padded', 'rows'), ('apply', 256, 17, 0, 'f32', 'out_padded', 'rows'),
    ('apply', 260, 15, 0, 'f32', 'x_padded', 'rows'), ('apply', 260, 17, 0, 'f32', 'out_padded', 'rows'),
    ('apply', 260, 65, FAR, 'f32', 'pad4', 'rows'), ('apply', 260, 64, 0, 'f32', 'contig', 'rows'),
)
ADSR_PARAMS = ('attack', 'decay', 'sustain', 'release', 'gate_on', 'gate_off')


def adsr_rows(V: int, seed: int) -> dict:
    """the envelope rows as `adsr_rows` of tests/test_gpu_engine.py draws them"""
    rng = np.random.default_rng(seed)
    return dict(attack=rng.uniform(0.001, 0.02, (1, V)), decay=rng.uniform(0.001, 0.03, (1, V)),
                sustain=rng.uniform(0.2, 0.9, (1, V)), release=rng.uniform(0.001, 0.05, (1, V)),
                gate_on=rng.uniform(0.0, 0.01, (1, V)), gate_off=rng.uniform(0.03, 0.06, (1, V)))


def adsr_build(case) -> Built:
    """the six control rows (Views), x for adsr_apply, `out` and the float64 reference (the envelope, times float64(x) for apply).
    The rows are drawn as the engine test draws them, with a zero attack, decay and release at voices 0, 1 and 2; then each
    voice's gate is moved so that the few rows of the launch fall somewhere between just before its gate opens and just after its
    release ends, whatever the position: every stage and stage boundary is met by some voice."""
    entry, V, rows, position, odt, layout, control = case
    rng = rng_of('adsr', case)
    p = adsr_rows(V, zlib.crc32(repr(case).encode()))
    for i, name in enumerate(('attack', 'decay', 'release')):
        if i < V:
            p[name][0, i] = 0.0
    if control == 'mixed':
        for name in ('decay', 'sustain', 'release'):
            p[name] = p[name][:, -1:].copy()
    into = rng.uniform(-0.001, (p['gate_off'] - p['gate_on']) + p['release'] + 0.001, (1, V))    # seconds since the gate opened
    move = position / RATE - into - p['gate_on']
    p['gate_on'], p['gate_off'] = p['gate_on'] + move, p['gate_off'] + move
    ref = R.adsr(position, rows, RATE, **p)
    (xpad, xld), (opad, old) = ADSR_LAYOUT[layout]
    operands = {name: view(p[name]) for name in ADSR_PARAMS}
    operands['x'] = None
    if entry == 'apply':
        x = f32(rng.uniform(-1.0, 1.0, (rows, V)))
        operands['x'] = view(x, xpad, xld)
        ref = ref * x.astype(np.float64)
    return Built(operands, view(np.zeros((rows, V), dtype=DTYPE[odt]), opad, old), np.broadcast_to(ref, (rows, V)).copy())


# ------------------------------------------------------------------------------------------------------------------ osc_bank
# (waveform, V, rows, position, out dtype, layout): the plain entry, step 1, one (1,V) row of hertz and of phase
OSC_CASES = (
    ('Sine', 1, 1, 0, 'f32', 'contig'), ('Sine', 1, 15, 0, 'f32', 'pad1'), ('Sine', 3, 1, 0, 'f32', 'ld4'),
    ('Sine', 3, 15, HOUR + 7, 'f64', 'pad4'), ('Sine', 3, 17, 0, 'f32', 'pad4'), ('Sine', 3, 65, 0, 'f32', 'ld1'),
    ('Sine', 4, 1, 0, 'f32', 'pad4'), ('Sine', 4, 17, 0, 'f32', 'ld1'), ('Sine', 4, 64, 0, 'f32', 'ld4'),
    ('Sine', 65, 15, 0, 'f32', 'contig'), ('Sine', 65, 17, 0, 'f64', 'pad1'), ('Sine', 65, 64, HOUR + 7, 'f32', 'contig'),
    ('Sine', 65, 65, 0, 'f32', 'contig'), ('Sine', 256, 16, HOUR + 7, 'f64', 'ld4'), ('Sine', 256, 17, 0, 'f32', 'ld1'),
    ('Sine', 256, 64, 0, 'f32', 'contig'), ('Sine', 260, 16, 0, 'f32', 'contig'), ('Sine', 260, 65, HOUR + 7, 'f32', 'ld4'),
    ('Square', 1, 65, 0, 'f32', 'pad1'), ('Square', 3, 1, 0, 'f32', 'ld1'), ('Square', 4, 16, 0, 'f64', 'pad1'),
    ('Square', 65, 17, HOUR + 7, 'f32', 'ld4'), ('Square', 256, 15, 0, 'f32', 'contig'), ('Square', 260, 64, 0, 'f32', 'pad4'),
    ('Square', 260, 65, HOUR + 7, 'f64', 'contig'),
    ('Sawtooth', 1, 64, HOUR + 7, 'f64', 'ld1'), ('Sawtooth', 3, 16, 0, 'f32', 'contig'), ('Sawtooth', 4, 15, 0, 'f32', 'ld4'),
    ('Sawtooth', 65, 16, 0, 'f32', 'ld1'), ('Sawtooth', 256, 65, 0, 'f32', 'pad4'), ('Sawtooth', 260, 1, HOUR + 7, 'f64', 'pad1'),
    ('Sawtooth', 260, 17, 0, 'f32', 'contig'), ('Triangle', 1, 16, 0, 'f32', 'pad4'), ('Triangle', 1, 17, 0, 'f32', 'ld4'),
    ('Triangle', 3, 64, 0, 'f32', 'pad1'), ('Triangle', 4, 65, HOUR + 7, 'f64', 'contig'), ('Triangle', 65, 1, 0, 'f32', 'pad4'),
    ('Triangle', 256, 1, 0, 'f32', 'pad1'), ('Triangle', 260, 15, 0, 'f32', 'ld1'), ('Triangle', 260, 65, 0, 'f64', 'ld4'),
)


def osc_build(case) -> Built:
    kind, V, rows, position, odt, layout = case
    rng = rng_of('osc', case)
    hertz, phase = rng.uniform(55.0, 1760.0, (1, V)), rng.uniform(0.0, 1.0, (1, V))
    return Built({'hertz': view(hertz), 'phase': view(phase)}, view(np.zeros((rows, V), dtype=DTYPE[odt]), *LAYOUT[layout]),
                 R.osc(kind, position, rows, RATE, hertz, phase))


# --------------------------------------------------------------------------------------------------------------- the census
VARIANTS = {'elementwise': ('fast', 'generic'),
            'sum_bus': ('fast-1', 'fast-2', 'fast-3', 'fast-4', 'generic-vec4', 'generic-scalar'),
            'adsr': ('VEC4', 'VEC1'), 'adsr_apply': ('VEC4', 'VEC1'), 'osc': ('VEC4', 'VEC1')}
CASES = {'elementwise': EW_CASES, 'sum_bus': BUS_CASES, 'adsr': tuple(c for c in ADSR_CASES if c[0] == 'adsr'),
         'adsr_apply': tuple(c for c in ADSR_CASES if c[0] == 'apply'), 'osc': OSC_CASES}


def expected_variant(kernel: str, case):
    """the variant `case` is meant to reach, from the dispatch rules of the .hip files (launch_ew; launch_bus_fast and launch_bus;
    launch_adsr; voice_tiling): a string, for sum_bus one per native call of the wrapper's split"""
    if kernel == 'elementwise':
        op, rows, V = case[:3]
        b = ew_build(case)
        a, bb, c, out = b.operands['a'], b.operands['b'], b.operands['c'], b.out
        fast = out.array.dtype == np.float32 and V % 4 == 0 and vec4_rows(out) and _ew_audio_fast(a, rows, V)
        if op in ('Gain', 'Amp'):
            fast = fast and _ew_ctrl_fast(bb, rows)
        if op in ('RingMod', 'Mix'):
            fast = fast and _ew_audio_fast(bb, rows, V)
        if op == 'Mix':
            fast = fast and _ew_ctrl_fast(c, rows)
        return 'fast' if fast else 'generic'
    if kernel == 'sum_bus':
        V, rows, C, xdt, odt, xlayout = case[:6]
        rows16 = vec4_rows(View(np.zeros((1, V)), *LAYOUT[xlayout]))
        reached = []
        for w in bus_widths(C):
            if xdt == 'f32' and w <= 2 and V % 256 == 0 and 0 < V <= 1024 and rows16:
                reached.append(f'fast-{V // 256}')
            else:
                reached.append('generic-vec4' if V % 4 == 0 and rows16 else 'generic-scalar')
        return tuple(reached)
    if kernel in ('adsr', 'adsr_apply'):
        V, layout = case[1], case[5]
        xl, ol = ADSR_LAYOUT[layout]
        vec4 = V % 4 == 0 and vec4_rows(View(np.zeros((1, V)), *ol))
        if kernel == 'adsr_apply':
            vec4 = vec4 and vec4_rows(View(np.zeros((1, V)), *xl))
        return 'VEC4' if vec4 else 'VEC1'
    if kernel == 'osc':
        V, layout = case[1], case[5]
        return 'VEC4' if V % 4 == 0 and vec4_rows(View(np.zeros((1, V)), *LAYOUT[layout])) else 'VEC1'
    raise ValueError(kernel)
