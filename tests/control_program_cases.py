"""Case table and float64 restatement for the block-rate control program (signals_amd/csrc/control_program.hip: the interpreter
sig_control_program / _windowed / _envelope and the specialised build), shared by tests/test_control_program_host.py and
tests/test_gpu_control_program.py.  numpy and ctypes only; torch is imported by `to_ctl` alone.

A case is a hand-written program: instruction tuples (op, kind, a, b, c, dst, stride, rows, cols, reserved, data) -- data: a ROW's
(rows, cols) float64 array, a NOISE's seed, True for a FILTER with a status word (None: a NULL one) --, outputs (reg, cols, front:
whether it has a front row) and the launch arguments.  `validate` is the gate in front of the GPU: the program lives in device memory
where the library cannot check it, so nothing that fails `validate` is ever uploaded.  `reference` restates include/signals_amd.h
(the sig_control_program comment) with the functions of oracle/chain_ref.py, per output.

An instruction is evaluated at its own width (the broadcast of its operands' widths); `validate` holds every program to operands of
width 1 or the instruction's own, so no case depends on what a register holds beyond its width.

Not in the table, on purpose:
  - a front position beside a ROW with rows = nblocks: the header says the front evaluation runs once more at front_position but not
    which of the nblocks rows it reads (the kernels read row 0).  Such cases are launched without a front position.
  - a one-column window-rate NOISE under a wide filter: the kernel would read channel v where the graph broadcasts channel 0, and the
    engine refuses that shape before it builds a program (`_filter`: a window narrower than the filter).  `validate` refuses it too:
    every instruction of a window run has its filter's width.
  - programs that are malformed on purpose.  The refusals stop in the entry's argument check, in front of any launch.

Structures: a specialised build is keyed by (op, kind, a, b, c, dst, wide bits) per instruction and (reg, wide) per output, so the
cases share a few builders; SPECIALISED names the ten structures that are built and run through sig_control_program_attached (the
edges of that kernel: its 256-column chunks, the one-column filter, window runs, per-block rows, clamp and front row).  What only the
interpreter has -- the count k0 of leading one-column ROWs it loads four in flight, its LDS register file sized by n_ins, the
all-one-column forms at cols = 1 -- runs through the interpreter's variants alone."""
import collections
import ctypes
import functools
import zlib

import numpy as np

from oracle import chain_ref as R

ROW, OSC, GAIN, MIX, RINGMOD, AMP, NOISE, FILTER, ADSRARGS, ADSR = range(10)      # SIG_CTL_*
SINE, SQUARE, SAWTOOTH, TRIANGLE = range(4)                                       # SIG_OSC_*
LOWPASS, HIGHPASS = 0, 1                                                          # SIG_FILT_*
OSC_NAMES = {SINE: 'Sine', SQUARE: 'Square', SAWTOOTH: 'Sawtooth', TRIANGLE: 'Triangle'}
FILT_NAMES = {LOWPASS: 'lp', HIGHPASS: 'hp'}
MAX_INS = 48
CONTEXT = 100
GUARD = 64                                        # cells behind every output and front row
GUARD_VALUE = float(np.frombuffer(np.array([0x7FF8C0DEC0DEC0DE], dtype=np.uint64).tobytes(), dtype=np.float64)[0])    # a NaN with a payload
VARIANTS = ('plain', 'windowed', 'envelope')
INVALID_VALUE = 1                                 # hipErrorInvalidValue

Launch = collections.namedtuple('Launch', 'rate position step nblocks cols front_position min_position')
Case = collections.namedtuple('Case', 'name group ins outs launch structure')
Ins = collections.namedtuple('Ins', 'op kind a b c dst stride rows cols reserved data')


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def launch(position=0, step=256, nblocks=3, cols=1, rate=48000, front=-1, min_position=0) -> Launch:
    return Launch(rate, position, step, nblocks, cols, front, min_position)


class Prog:
    """a program under construction: every method appends one instruction and returns its register"""

    def __init__(self):
        self.ins = []

    def add(self, op, kind=0, a=-1, b=-1, c=-1, cols=1, win=0, stride=0, rows=1, data=None):
        self.ins.append(Ins(op, kind, a, b, c, len(self.ins), stride, rows, cols, win, data))
        return len(self.ins) - 1

    def row(self, data):
        data = np.array(data, dtype=np.float64, ndmin=2)
        return self.add(ROW, cols=data.shape[1], rows=data.shape[0], stride=0 if data.shape[1] == 1 else 1, data=data)

    def width(self, *regs):
        return max([1] + [self.ins[r].cols for r in regs if r >= 0])

    def osc(self, kind, hertz=-1, phase=-1, win=0, cols=None):
        return self.add(OSC, kind, hertz, phase, cols=cols or self.width(hertz, phase), win=win)

    def binary(self, op, a, b, c=-1, win=0):
        return self.add(op, 0, a, b, c, cols=self.width(a, b, c), win=win)

    def noise(self, seed, cols, win=0):
        return self.add(NOISE, cols=cols, win=win, data=int(seed))

    def filter(self, kind, a, cutoff, status=True):
        return self.add(FILTER, kind, a, cutoff, cols=self.width(a, cutoff), data=True if status else None)

    def adsr(self, attack, decay, sustain, release, gate_on, gate_off, win=0):
        cols = self.width(attack, decay, sustain, release, gate_on, gate_off)
        self.add(ADSRARGS, 0, release, gate_on, gate_off, cols=cols, win=win)
        return self.add(ADSR, 0, attack, decay, sustain, cols=cols, win=win)

    def outs(self, *regs, front=True):
        fronts = front if isinstance(front, (tuple, list)) else (front,) * len(regs)
        return tuple((r, self.ins[r].cols, bool(f)) for r, f in zip(regs, fronts))


# ------------------------------------------------------------------------------------------------------------------ structures
def mid_of(cols: int) -> int:
    """the width of the narrower wide output beside a `cols`-wide one: 129 at 257"""
    return 1 if cols == 1 else max(2, (cols + 1) // 2)


def s_plain(cols, nblocks=1, per_block=False, key='plain'):
    """filterless: a one-column LFO, a Gain by a narrower wide ROW, a wide Triangle mixed with the LFO under a wide ROW.
    `per_block`: the LFO's hertz row (one column, stride 0) and the wide mix row (stride 1) have one row per block."""
    rng, p = rng_of(key, cols, nblocks, per_block), Prog()
    rows = nblocks if per_block else 1
    hz = p.row(rng.uniform(1.0, 9.0, (rows, 1)))
    ph = p.row([[0.125]])
    lfo = p.osc(SAWTOOTH, hz, ph)
    depth = p.row(rng.uniform(-2.0, 2.0, (1, mid_of(cols))))
    scaled = p.binary(GAIN, lfo, depth)
    hzv = p.row(rng.uniform(0.5, 40.0, (1, cols)))
    tri = p.osc(TRIANGLE, hzv, ph)
    mixv = p.row(rng.uniform(0.0, 1.0, (rows, cols)))
    out = p.binary(MIX, tri, lfo, mixv)
    return p, (lfo, scaled, out)


def s_filter(cols, kind=LOWPASS, bad_column=None, key='filter'):
    """a wide filter over Osc -> RingMod(wide ROW), its cutoff a wide ROW; then a block-rate Gain"""
    rng, p = rng_of(key, cols, kind), Prog()
    hz = p.row(rng.uniform(200.0, 900.0, (1, cols)))
    ring = p.row(rng.uniform(-1.0, 1.0, (1, cols)))
    cutoff = rng.uniform(50.0, 9000.0, (1, cols))
    if bad_column is not None:
        cutoff[0, bad_column] = 30000.0                   # above Nyquist at both rates
    cut = p.row(cutoff)
    scale = p.row([[1.5]])
    o = p.osc(SAWTOOTH, hz, win=1)
    r = p.binary(RINGMOD, o, ring, win=1)
    f = p.filter(kind, r, cut)
    g = p.binary(GAIN, f, scale)
    return p, (g, f)


def s_noise(cols, key='noise'):
    """wide block-rate Noise, scaled and mixed with a wide ROW"""
    rng, p = rng_of(key, cols), Prog()
    n = p.noise(0x9E3779B97F4A7C15 ^ cols, cols)
    depth = p.row([[0.04]])
    base = p.row(rng.uniform(100.0, 800.0, (1, cols)))
    half = p.row([[0.5]])
    g = p.binary(GAIN, n, depth)
    m = p.binary(MIX, g, base, half)
    return p, (m, n)


def adsr_rows(rng, cols, wide=(True, False, True, False, True, False)):
    """attack, decay, sustain, release, gate_on, gate_off: gates around the first few milliseconds, a zero-length stage in the
    first columns"""
    draw = {'attack': (0.001, 0.02), 'decay': (0.001, 0.03), 'sustain': (0.2, 0.9), 'release': (0.001, 0.05),
            'gate_on': (-0.004, 0.012), 'gate_off': (0.014, 0.03)}
    rows = []
    for (name, (lo, hi)), w in zip(draw.items(), wide):
        x = rng.uniform(lo, hi, (1, cols if w else 1))
        if name in ('attack', 'sustain') and x.shape[1] > 2:
            x[0, 1] = 0.0 if name == 'attack' else 1.0
        rows.append(x)
    return rows


def s_adsr(cols, key='adsr'):
    """a wide ADSR pair over wide and one-column parameter rows, and a Gain behind it"""
    rng, p = rng_of(key, cols), Prog()
    regs = [p.row(x) for x in adsr_rows(rng, cols)]
    amount = p.row([[3000.0]])
    e = p.adsr(*regs)
    g = p.binary(GAIN, e, amount)
    return p, (g, e)


def s_narrow(kind=LOWPASS, key='narrow'):
    """a one-column filter over a Square LFO: thread j evaluates window row j"""
    p = Prog()
    hz = p.row([[701.0]])
    cut = p.row([[1900.0 if kind == LOWPASS else 2600.0]])
    scale = p.row([[-0.75]])
    o = p.osc(SQUARE, hz, win=1)
    f = p.filter(kind, o, cut)
    g = p.binary(GAIN, f, scale)
    return p, (g, f)


def s_windows(cols, key='windows'):
    """five filters with window runs of their own: Osc of each waveform -> Gain by a ROW -> Mix with a ROW, alternately one column
    (Sine, Sawtooth) and wide (Square, Triangle), and a wide window-rate Noise; each followed by a block-rate Gain or Mix"""
    rng, p = rng_of(key, cols), Prog()
    hz, g, other, mix, cut = (p.row([[x]]) for x in (523.0, 0.8, 0.25, 0.7, 2100.0))
    hzw = p.row(rng.uniform(300.0, 1500.0, (1, cols)))
    cutw = p.row(rng.uniform(100.0, 6000.0, (1, cols)))
    scale = p.row([[2.0]])
    outs = []
    for kind, wide, ftype in ((SINE, False, LOWPASS), (SQUARE, True, HIGHPASS), (SAWTOOTH, False, HIGHPASS), (TRIANGLE, True, LOWPASS)):
        o = p.osc(kind, hzw if wide else hz, win=1)
        a = p.binary(GAIN, o, g, win=1)
        m = p.binary(MIX, a, other, mix, win=1)
        f = p.filter(ftype, m, cutw if wide else cut)
        outs.append(p.binary(GAIN, f, scale) if ftype == LOWPASS else p.binary(MIX, f, other, mix))
    n = p.noise(77, cols, win=1)
    f = p.filter(LOWPASS, n, cutw)
    outs.append(p.binary(GAIN, f, scale))
    return p, tuple(outs)


def s_adsr_window(cols, key='adsr_window'):
    """a smoothed envelope twice: a one-column ADSR pair inside a one-column filter's window, a wide pair inside a wide one's"""
    rng, p = rng_of(key, cols), Prog()
    narrow = [p.row(x) for x in adsr_rows(rng, 1, wide=(False,) * 6)]
    wide = [p.row(x) for x in adsr_rows(rng, cols, wide=(True,) * 6)]
    cut = p.row([[900.0]])
    cutw = p.row(rng.uniform(200.0, 4000.0, (1, cols)))
    f1 = p.filter(LOWPASS, p.adsr(*narrow, win=1), cut)
    f2 = p.filter(LOWPASS, p.adsr(*wide, win=1), cutw)
    return p, (f1, f2)


def s_operands(cols, key='operands'):
    """every two- and three-operand op with each operand in turn -1, and Amp of a negative base under fractional and whole exponents"""
    rng, p = rng_of(key, cols), Prog()
    x = p.row([[0.375]])
    y = p.row(rng.uniform(-1.0, 1.0, (1, cols)))
    c = p.row([[0.3]])
    base = p.row(-rng.uniform(0.1, 2.0, (1, cols)))
    expo = rng.uniform(0.5, 3.0, (1, cols))
    expo[0, ::3] = np.rint(expo[0, ::3])                                       # whole exponents: numbers beside the NaNs
    e = p.row(expo)
    outs = [p.osc(SINE, -1, x), p.osc(SQUARE, y, -1), p.osc(SAWTOOTH, -1, -1), p.osc(TRIANGLE, -1, y),
            p.binary(GAIN, -1, y), p.binary(GAIN, y, -1), p.binary(RINGMOD, -1, x), p.binary(RINGMOD, y, -1),
            p.binary(AMP, -1, e), p.binary(AMP, y, -1), p.binary(MIX, -1, y, c), p.binary(MIX, y, -1, c), p.binary(MIX, y, x, -1),
            p.binary(AMP, base, e)]
    return p, tuple(outs)


def s_big(variant, cols, key='big'):
    """48 instructions: 8 one-column ROWs (k0 = 8), a wide ROW, then a dependent chain through every op of the plain variant whose
    tail is wide; `windowed`: a window-rate Osc and a Filter inside the chain; `envelope`: also an ADSR pair"""
    rng, p = rng_of(key, cols), Prog()
    hz, ph, g, m, e, cut, short, off = (p.row([[x]]) for x in (2.0, 0.1, 0.7, 0.3, 2.0, 500.0, 0.004, 0.02))
    w = p.row(rng.uniform(0.2, 1.0, (1, cols)))
    prev, carry = g, None                                  # carry: the chain in front of a Filter or an ADSR, multiplied back in behind it
    while len(p.ins) < MAX_INS:
        k = len(p.ins)
        if variant != 'plain' and k == 20:
            carry, prev = prev, p.filter(LOWPASS, p.osc(SAWTOOTH, cut, win=1), cut)
        elif variant == 'envelope' and k == 30:
            carry, prev = prev, p.adsr(short, short, g, short, -1, off)
        else:
            second = w if k >= 40 else g if carry is None else carry
            carry = carry if k % 8 != 1 else None
            prev = [lambda: p.osc(SINE, hz, prev), lambda: p.binary(GAIN, prev, second), lambda: p.binary(MIX, prev, ph, m),
                    lambda: p.osc(SQUARE, hz, prev), lambda: p.binary(RINGMOD, prev, prev), lambda: p.osc(SAWTOOTH, hz, prev),
                    lambda: p.binary(AMP, prev, e), lambda: p.osc(TRIANGLE, hz, prev)][k % 8]()
    return p, (39, 44, 47)


def s_leading(k0, first_wide=False, key='leading'):
    """k0 leading one-column ROWs (behind a wide ROW when `first_wide`: k0 = 0), their product, and a Sine at that frequency"""
    rng, p = rng_of(key, k0, first_wide), Prog()
    wide = p.row(rng.uniform(0.5, 1.5, (1, 2))) if first_wide else -1
    rows = [p.row([[x]]) for x in rng.uniform(1.05, 1.4, max(k0, 1))]
    acc = rows[0]
    for r in rows[1:]:
        acc = p.binary(RINGMOD, acc, r)
    s = p.osc(SINE, acc)
    outs = (acc, s) + ((p.binary(GAIN, s, wide),) if first_wide else ())
    return p, outs


def leading_rows(ins) -> int:
    """k0: the leading one-column ROWs the interpreter loads four in flight"""
    k0 = 0
    while k0 < len(ins) and ins[k0].op == ROW and ins[k0].cols == 1:
        k0 += 1
    return k0


# ------------------------------------------------------------------------------------------------------------------- the table
COLS = (1, 2, 127, 128, 129, 255, 256, 257, 300)
POSITIONS = (2, 99, 100, 101, 2 ** 31 - 300, 2 ** 40 - 17)
SPECIALISED = ('plain', 'filter', 'noise', 'adsr', 'narrow_lp', 'narrow_hp', 'windows', 'adsr_window', 'operands', 'big_envelope')


def _cases():
    table = []

    def case(name, group, built, L, structure=None, front=True):
        p, regs = built
        table.append(Case(name, group, tuple(p.ins), p.outs(*regs, front=front), L, structure))

    one = lambda s, cols: s if cols > 1 else None                              # (all one column at cols = 1: another structure)
    for cols in COLS:
        case(f'plain_{cols}', 'columns', s_plain(cols), launch(0, 256, 3, cols), one('plain', cols))
        case(f'filter_{cols}', 'columns', s_filter(cols), launch(0, 256, 3, cols), one('filter', cols))
        case(f'filter_{cols}_44100', 'columns', s_filter(cols), launch(0, 256, 3, cols, rate=44100), one('filter', cols))
        case(f'noise_{cols}', 'columns', s_noise(cols), launch(0, 256, 3, cols), one('noise', cols))
        case(f'adsr_{cols}', 'columns', s_adsr(cols), launch(0, 256, 3, cols), one('adsr', cols))
    # window length: h = 0 .. 100 in one launch (and two blocks at h = 100 behind them)
    sweep = dict(position=0, step=1, nblocks=103)
    case('sweep_narrow_lp', 'window length', s_narrow(LOWPASS), launch(**sweep), 'narrow_lp')
    case('sweep_narrow_lp_44100', 'window length', s_narrow(LOWPASS), launch(**sweep, rate=44100), 'narrow_lp')
    case('sweep_narrow_hp', 'window length', s_narrow(HIGHPASS), launch(**sweep), 'narrow_hp')
    case('sweep_wide_lp', 'window length', s_filter(3), launch(**sweep, cols=3), 'filter')
    for q in POSITIONS:
        case(f'position_narrow_{q}', 'window length', s_narrow(LOWPASS), launch(q, 256, 3), 'narrow_lp')
    for q in (2, 2 ** 40 - 17):
        case(f'position_wide_{q}', 'window length', s_filter(3), launch(q, 256, 3, 3), 'filter')
    # window contents
    case('windows_5', 'window contents', s_windows(5), launch(1000, 256, 3, 5), 'windows')
    case('windows_300', 'window contents', s_windows(300), launch(7, 300, 2, 300, front=50), 'windows')
    case('adsr_window_3', 'window contents', s_adsr_window(3), launch(0, 200, 8, 3), 'adsr_window')
    case('adsr_window_257', 'window contents', s_adsr_window(257), launch(700, 128, 2, 257, front=650), 'adsr_window')
    # rows: rows = nblocks, one column (stride 0) and wide (stride 1), a wide ROW narrower than the launch -- no front position
    case('rows_per_block_257', 'rows', s_plain(257, 4, True), launch(100, 300, 4, 257), 'plain')
    case('rows_per_block_3', 'rows', s_plain(3, 9, True), launch(0, 128, 9, 3), 'plain')
    case('rows_per_block_1', 'rows', s_plain(1, 5, True), launch(0, 128, 5, 1))
    # size
    case('one_row', 'size', s_leading(1), launch(480, 256, 2))
    p = Prog(); r = p.row(rng_of('wide_row').uniform(-1, 1, (1, 130)))
    case('one_wide_row', 'size', (p, (r,)), launch(0, 256, 2, 130))
    p = Prog(); r = p.row([[3.0]]); o = p.osc(SQUARE, r)
    case('two', 'size', (p, (o, r)), launch(480, 1000, 5))
    case('leading_0', 'size', s_leading(1, first_wide=True), launch(480, 256, 3, 2))
    for k0 in (3, 4, 5, 8):
        case(f'leading_{k0}', 'size', s_leading(k0), launch(480, 256, 3))
    for variant in VARIANTS:
        case(f'big_{variant}', 'size', s_big(variant, 130), launch(300, 256, 3, 130, front=44),
             'big_envelope' if variant == 'envelope' else None)
    # launch
    for n in (1, 2, 9):
        case(f'nblocks_{n}', 'launch', s_plain(129), launch(123, 256, n, 129, front=11), 'plain')
    case('front_alone', 'launch', s_plain(257), launch(0, 256, 0, 257, front=5000), 'plain')
    case('front_alone_narrow', 'launch', s_narrow(LOWPASS), launch(0, 256, 0, front=57), 'narrow_lp')
    case('no_outputs', 'launch', s_plain(129), launch(0, 256, 3, 129, front=7), 'plain')
    for lo in (0, 37):
        clamp = dict(position=-300, step=128, nblocks=6, min_position=lo, front=lo + 5)
        case(f'clamp_plain_{lo}', 'launch', s_plain(130), launch(cols=130, **clamp), 'plain')
        case(f'clamp_narrow_{lo}', 'launch', s_narrow(HIGHPASS), launch(**clamp), 'narrow_hp')
        case(f'clamp_filter_{lo}', 'launch', s_filter(4), launch(cols=4, **clamp), 'filter')
        case(f'clamp_adsr_{lo}', 'launch', s_adsr(130), launch(cols=130, **clamp), 'adsr')
    case('front_null', 'launch', s_plain(257), launch(512, 256, 2, 257, front=256), 'plain', front=(True, False, True))
    case('front_null_filter', 'launch', s_filter(257), launch(512, 256, 2, 257, front=256), 'filter', front=(False, True))
    case('step_0', 'launch', s_plain(3), launch(4800, 0, 3, 3), 'plain')
    # operands
    case('operands_4', 'operands', s_operands(4), launch(1234, 256, 2, 4), 'operands')
    case('operands_300', 'operands', s_operands(300), launch(1234, 256, 2, 300, front=9), 'operands')
    # status
    case('status_bad', 'status', s_filter(300, bad_column=200), launch(1000, 256, 2, 300, front=5), 'filter')
    case('status_good', 'status', s_filter(300), launch(1000, 256, 2, 300, front=5), 'filter')
    return tuple(table)


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
NO_OUTPUTS = 'no_outputs'                                        # launched with n_outs = 0: returns 0, touches nothing
# refusals: (what, the case whose buffers are passed, the arguments that replace the launch's) -- the entry's argument check
REFUSALS = (('n_ins = 49', 'nblocks_2', dict(n_ins=49)), ('cols = 0', 'nblocks_2', dict(cols=0)), ('rate = 0', 'nblocks_2', dict(rate=0)),
            ('front_position = -2', 'nblocks_2', dict(front_position=-2)), ('min_position = -1', 'nblocks_2', dict(min_position=-1)))


# -------------------------------------------------------------------------------------------------------------------- validate
def variant_of(case) -> str:
    ops = {i.op for i in case.ins}
    return 'envelope' if ops & {ADSRARGS, ADSR} else 'windowed' if ops & {NOISE, FILTER} else 'plain'


def variants_of(case) -> tuple:
    """the interpreter variants that run the case: the one its ops require and the wider ones"""
    return VARIANTS[VARIANTS.index(variant_of(case)):]


def window_runs(case) -> dict:
    """filter index -> the indices of its window run (the contiguous reserved instructions right in front of it)"""
    runs = {}
    for k, i in enumerate(case.ins):
        if i.op == FILTER:
            w = k
            while w > 0 and case.ins[w - 1].reserved:
                w -= 1
            runs[k] = tuple(range(w, k))
    return runs


def operands(i: Ins) -> tuple:
    """the operand registers an instruction reads"""
    return {ROW: (), NOISE: (), OSC: (i.a, i.b), GAIN: (i.a, i.b), RINGMOD: (i.a, i.b), AMP: (i.a, i.b), FILTER: (i.a, i.b)}.get(i.op, (i.a, i.b, i.c))


def validate(case) -> None:
    """the gate in front of the GPU: asserts that the program indexes nothing outside its register file and its row buffers and has
    the form the header describes"""
    ins, L = case.ins, case.launch
    n = len(ins)
    assert 1 <= n <= MAX_INS, (case.name, n)
    assert L.rate > 0 and L.step >= 0 and L.nblocks >= 0 and 1 <= L.cols <= 4096 and L.front_position >= -1 and L.min_position >= 0
    assert L.nblocks <= 128
    runs = window_runs(case)
    run_of = {w: f for f, run in runs.items() for w in run}
    for k, i in enumerate(ins):
        what = (case.name, k)
        assert i.dst == k and i.dst < n, what
        assert 0 <= i.op <= ADSR and i.reserved in (0, 1) and 1 <= i.cols <= L.cols, what
        assert all(r == -1 or 0 <= r < k for r in (i.a, i.b, i.c)), what
        used = operands(i)
        if i.op in (GAIN, RINGMOD, AMP, OSC, FILTER, ROW, NOISE):
            assert i.c == -1, what
        if i.op in (ROW, NOISE):
            assert i.a == -1 and i.b == -1, what
        if i.op == ROW:
            assert not i.reserved, what
            assert isinstance(i.data, np.ndarray) and i.data.dtype == np.float64 and i.data.shape == (i.rows, i.cols), what
            assert i.rows in (1, L.nblocks) and i.rows >= 1 and i.stride == (0 if i.cols == 1 else 1), what
            if i.rows > 1:
                assert L.front_position == -1, what
        elif i.op == NOISE:
            assert isinstance(i.data, int) and 0 <= i.data < 1 << 64, what
        elif i.op == FILTER:
            assert i.data in (True, None) and i.kind in (LOWPASS, HIGHPASS) and not i.reserved, what
            assert i.a >= 0 and i.b >= 0 and ins[i.a].cols == i.cols and not ins[i.b].reserved, what
            assert (i.a in runs[k]) if runs[k] else not ins[i.a].reserved, what
        else:
            assert i.data is None, what
        if i.op == OSC:
            assert i.kind in OSC_NAMES, what
        if i.op not in (ROW, NOISE, ADSRARGS, ADSR, FILTER):
            widths = [ins[r].cols for r in used if r >= 0]
            assert i.cols == max([1] + widths) or (not widths and i.cols >= 1), what
            assert all(w in (1, i.cols) for w in widths), what
        if i.op == ADSR:
            assert k > 0 and ins[k - 1].op == ADSRARGS and (ins[k - 1].cols, ins[k - 1].reserved) == (i.cols, i.reserved), what
            g = ins[k - 1]
            widths = [ins[r].cols for r in (i.a, i.b, i.c, g.a, g.b, g.c) if r >= 0]
            assert i.cols == max([1] + widths) and all(w in (1, i.cols) for w in widths), what
        if i.op == ADSRARGS:
            assert k + 1 < n and ins[k + 1].op == ADSR, what
        if i.reserved:                                    # window-rate: in a run, of its filter's width, over window registers or block-invariant rows
            assert k in run_of and i.cols == ins[run_of[k]].cols, what
            for r in used + ((ins[k - 1].a, ins[k - 1].b, ins[k - 1].c) if i.op == ADSR else ()):
                assert r == -1 or (r in runs[run_of[k]]) or (ins[r].op == ROW and ins[r].rows == 1), what
        else:
            source = used if i.op != FILTER else (i.b,)
            assert all(r == -1 or not ins[r].reserved for r in source), what
            if i.op == ADSR:
                assert all(r == -1 or not ins[r].reserved for r in (ins[k - 1].a, ins[k - 1].b, ins[k - 1].c)), what
    for f, run in runs.items():                            # a window register feeds its own run and its filter, nothing else
        for k, i in enumerate(ins):
            if k not in run and k != f:
                reads = operands(i) + ((ins[k - 1].a, ins[k - 1].b, ins[k - 1].c) if i.op == ADSR else ())
                assert not set(reads) & set(run), (case.name, k, f)
    assert 1 <= len(case.outs) <= 64
    for reg, cols, _ in case.outs:
        assert 0 <= reg < n and not ins[reg].reserved and ins[reg].op != ADSRARGS and cols == ins[reg].cols, (case.name, reg)


# ------------------------------------------------------------------------------------------------------------------- reference
def _round32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def _execute(case, k, regs, frame, block, narrow):
    """instruction k at `frame` (a ROW with one row per block reads row `block`): a (1, cols) float64 array"""
    i, rate = case.ins[k], case.launch.rate
    get = lambda r: np.zeros((1, 1)) if r < 0 else regs[r]
    if i.op == ROW:
        x = i.data[block if i.rows > 1 else 0][None, :]
    elif i.op == OSC:
        x = R.osc_wave(OSC_NAMES[i.kind], R.osc_cycles(frame, 1, rate, get(i.a), get(i.b)))
    elif i.op == GAIN:
        x = R.gain(get(i.a), get(i.b))
    elif i.op == RINGMOD:
        x = R.ringmod(get(i.a), get(i.b))
    elif i.op == MIX:
        x = R.mix(get(i.a), get(i.b), get(i.c))
    elif i.op == AMP:
        with np.errstate(all='ignore'):
            x = R.amp(get(i.a), get(i.b))
    elif i.op == NOISE:
        x = R.white(i.data, frame, 1, i.cols)
    elif i.op == ADSRARGS:
        x = np.zeros((1, 1))
    elif i.op == ADSR:
        g = case.ins[k - 1]
        x = R.adsr(frame, 1, rate, get(i.a), get(i.b), get(i.c), get(g.a), get(g.b), get(g.c))
    else:
        raise ValueError(i.op)
    x = np.broadcast_to(np.asarray(x, dtype=np.float64), (1, i.cols))
    return _round32(x) if narrow else x.copy()


@functools.lru_cache(maxsize=None)
def _sos(kind, wn):
    return R.butter2_sos(wn, FILT_NAMES[kind])


def window_rows(case, k, regs, frame, block=0) -> np.ndarray:
    """the (h + 1, cols) rows a FILTER k steps over for the block at `frame`: its window run at p - h .. p, the h history rows rounded
    to float32 when h > 1; `regs`: the block-rate registers in front of it"""
    i, run = case.ins[k], window_runs(case)[k]
    h = min(CONTEXT, frame)
    window = []
    for j in range(h + 1):
        local = dict(regs)
        for w in run:
            local[w] = _execute(case, w, local, frame - h + j, block, narrow=j < h and h > 1)
        window.append(np.broadcast_to(local[i.a], (1, i.cols)))
    return np.concatenate(window)


def _filter(case, k, regs, frame, block):
    """the header's SIG_CTL_FILTER: a cold-started biquad over the window rows per column, its last output.  A cutoff outside
    (0, Nyquist) gives NaN (the kernel designs NaN coefficients)."""
    i, rate = case.ins[k], case.launch.rate
    window = window_rows(case, k, regs, frame, block)
    cutoff = np.broadcast_to(regs[i.b], (1, i.cols))
    y = np.empty((1, i.cols))
    for v in range(i.cols):
        wn = min(max(float(cutoff[0, v]) / (rate / 2), 0.0), 1.0)
        y[0, v] = R.sosfilt_df2t(_sos(i.kind, wn), window[:, v])[-1] if 0.0 < wn < 1.0 else np.nan
    return y


def evaluate(case, frame, block=0) -> dict:
    """register -> its (1, cols) value for the block evaluated at `frame` (window-rate registers excluded)"""
    regs = {}
    for k, i in enumerate(case.ins):
        if i.reserved:
            continue
        regs[k] = _filter(case, k, regs, frame, block) if i.op == FILTER else _execute(case, k, regs, frame, block, False)
    return regs


@functools.lru_cache(maxsize=None)
def _reference(name):
    case = BY_NAME[name]
    L = case.launch
    blocks = [evaluate(case, max(L.position + b * L.step, L.min_position), b) for b in range(L.nblocks)]
    front = evaluate(case, L.front_position, 0) if L.front_position >= 0 else None
    result = []
    for reg, cols, has_front in case.outs:
        rows = np.concatenate([r[reg] for r in blocks]) if blocks else np.zeros((0, cols))
        rows.setflags(write=False)
        frow = front[reg] if front is not None and has_front else None
        result.append((rows, frow))
    return tuple(result)


def reference(case) -> tuple:
    """per output: ((nblocks, cols) float64 rows, the (1, cols) front row or None).  The block frame is max(position + b * step,
    min_position); the front row is evaluated at front_position, unclamped.  Computed once per case and shared (read-only)."""
    return _reference(case.name)


def frames_of(case) -> list:
    L = case.launch
    return [max(L.position + b * L.step, L.min_position) for b in range(L.nblocks)]


def window_lengths(case) -> set:
    """the h of every filter evaluation of the case (block rows and the front row)"""
    L = case.launch
    frames = frames_of(case) + ([L.front_position] if L.front_position >= 0 else [])
    return {min(CONTEXT, p) for p in frames} if any(i.op == FILTER for i in case.ins) else set()


# ----------------------------------------------------------------------------------------------------- what an output is held to
def cone(case, reg) -> set:
    """the instructions an output register depends on"""
    seen, todo, runs = set(), [reg], window_runs(case)
    while todo:
        k = todo.pop()
        if k < 0 or k in seen:
            continue
        seen.add(k)
        i = case.ins[k]
        todo += list(operands(i)) + list(runs.get(k, ()))
        if i.op == ADSR:
            todo.append(k - 1)
            todo += [case.ins[k - 1].a, case.ins[k - 1].b, case.ins[k - 1].c]
    return seen


def holds_to(case, reg) -> str:
    """'exact': only ROW, Square / Sawtooth / Triangle, Gain / Mix / RingMod, Noise and ADSR, at block rate or in windows without a
    filter behind them -- the definition bit for bit; 'sine': a float64 Sine and neither a Filter nor an Amp; 'bar': the rest"""
    mine = [case.ins[k] for k in cone(case, reg)]
    if any(i.op in (FILTER, AMP) for i in mine):
        return 'bar'
    return 'sine' if any(i.op == OSC and i.kind == SINE for i in mine) else 'exact'


SINE_ULP = 2.0 ** -52            # one unit in the last place of float64 at the waveform's full scale


def sine_bound(case, reg, values) -> np.ndarray:
    """the bound of a 'sine' output: each Sine is within SINE_ULP of the oracle's (include/signals_amd.h, sig_osc_bank); through
    what follows it the error grows by the magnitudes it is multiplied with, read from the case's own registers at each block.
    `values`: the registers of one block (`_evaluate`).  Only what the table contains is propagated: a Sine's own operands are exact."""
    err = {}
    for k in sorted(cone(case, reg)):
        i = case.ins[k]
        e = lambda r: err.get(r, 0.0) if r >= 0 else 0.0
        mag = lambda r: np.abs(values[r]) if r >= 0 else 0.0
        if i.op == OSC:
            assert not np.any(e(i.a)) and not np.any(e(i.b)), 'a modulated oscillator behind a Sine is not propagated'
            err[k] = SINE_ULP if i.kind == SINE else 0.0
        elif i.op in (GAIN, RINGMOD):
            err[k] = mag(i.a) * e(i.b) + mag(i.b) * e(i.a)
        elif i.op == MIX:
            c = values[i.c] if i.c >= 0 else 0.0
            assert not np.any(e(i.c))
            err[k] = np.abs(c) * e(i.a) + np.abs(1.0 - c) * e(i.b)
        else:
            err[k] = 0.0
        if np.any(err[k]):
            err[k] = err[k] + 2.0 ** -53 * np.abs(values[k])       # the rounding of this operation on a changed operand
    return np.broadcast_to(err[reg], values[reg].shape)


def sine_bounds(case) -> tuple:
    """per output, a (nblocks, cols) bound, and the front row's -- for the outputs held to 'sine'"""
    L = case.launch
    blocks = [evaluate(case, p, b) for b, p in enumerate(frames_of(case))]
    front = evaluate(case, L.front_position, 0) if L.front_position >= 0 else None
    out = []
    for reg, cols, has_front in case.outs:
        if holds_to(case, reg) != 'sine':
            out.append(None)
            continue
        out.append((np.concatenate([sine_bound(case, reg, v) for v in blocks]) if blocks else np.zeros((0, cols)),
                    sine_bound(case, reg, front) if front is not None and has_front else None))
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------------- to_ctl
Uploaded = collections.namedtuple('Uploaded', 'program outs ins_list outs_list rows buffers fronts status')


def to_ctl(case, device) -> Uploaded:
    """the case as `_native.CtlIns` / `_native.CtlOut` arrays on `device` (uploaded by `_native.upload_structs` on the GPU; a plain
    byte tensor on the CPU).  `rows` keeps every ROW tensor alive; buffers / fronts: one flat float64 tensor per output, nblocks *
    cols (cols) cells and GUARD cells of GUARD_VALUE behind them, everything in front filled with GUARD_VALUE too (None for a NULL
    front); status: instruction index -> its int32 status word."""
    import torch
    from signals_amd import _native
    validate(case)
    L = case.launch
    rows, status, ins_list = {}, {}, []
    for k, i in enumerate(case.ins):
        pointer = 0
        if i.op == ROW:
            rows[k] = torch.from_numpy(np.ascontiguousarray(i.data)).to(device)
            pointer = rows[k].data_ptr()
        elif i.op == NOISE:
            pointer = i.data
        elif i.op == FILTER and i.data:
            status[k] = torch.zeros(2, dtype=torch.int32, device=device)
            pointer = status[k].data_ptr()
        ins_list.append(_native.CtlIns(i.op, i.kind, i.a, i.b, i.c, i.dst, i.stride, i.rows, i.cols, i.reserved, pointer or None))
    buffers, fronts, outs_list = [], [], []
    guarded = lambda n: torch.from_numpy(np.full(n + GUARD, guard_bits(), dtype=np.uint64).view(np.float64)).to(device)
    for reg, cols, has_front in case.outs:
        buffers.append(guarded(L.nblocks * cols))
        fronts.append(guarded(cols) if has_front else None)
        outs_list.append(_native.CtlOut(reg, cols, buffers[-1].data_ptr(), fronts[-1].data_ptr() if has_front else None))
    if torch.device(device).type == 'cpu':
        pack = lambda items: torch.frombuffer(bytearray(bytes((type(items[0]) * len(items))(*items))), dtype=torch.uint8)
    else:
        pack = _native.upload_structs
    return Uploaded(pack(ins_list), pack(outs_list), ins_list, outs_list, rows, buffers, fronts, status)


def guard_bits() -> int:
    return int(np.array([GUARD_VALUE]).view(np.uint64)[0])
