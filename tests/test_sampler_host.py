"""The sample-playback node without a GPU: the read-position arithmetic and the neighbour rule of sig_sampler.h compiled for the host
(tests/native/sampler_index.cpp) against the numpy restatement (tests/sampler_reference.py) bit for bit, that restatement against a
direct loop and against two identities, the node API of ext.Sampler with its state validation, name resolution, the .sigs loader and
table_from_wav, sig_sampler_play's export, declaration and argument checks, and how the engine's planner classifies and schedules
the node: an oscillator's purity, one kernel per node on every renderer setting, no voice program, the refusal in a control path."""
import ctypes
import math
import pathlib
import shutil
import subprocess
import types

import numpy as np
import pytest

from signals_amd import SignalFlags, _native
from signals_amd.chain import BadStateValue, BlockCachingEmitter
from signals_amd.chain import ext, files, fixed, fx, osc

import sampler_reference as SR

ROOT = pathlib.Path(__file__).resolve().parent.parent
INV = 1     # hipErrorInvalidValue
RATE, V = 48000, 8
HOUR = 172_800_000


@pytest.fixture(autouse=True)
def _cpu_device():
    from signals_amd import runtime
    old = runtime._device
    runtime.set_device('cpu')
    yield
    runtime._device = old


@pytest.fixture(scope='module')
def lib():
    if not _native.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return _native.lib()


def fix(v):
    f = fixed.Fixed()
    f.get_state().value = np.array(v, ndmin=2, dtype=float)
    return f


def row(lo, hi, n=V):
    return np.linspace(lo, hi, n).reshape(1, n)


def mkosc(cls, hz):
    o = cls(); o.hertz = fix(hz)
    return o


def sampler_node(table=None, ratio=1.0, offset=None, gate_on=None, select=None, loop=None):
    n = ext.Sampler()
    if table is not None:
        n.get_state().table = np.asarray(table)
    if loop is not None:
        n.get_state().loop_end, n.get_state().loop_start = loop[1], loop[0]
    for name, value in (('ratio', ratio), ('offset', offset), ('gate_on', gate_on), ('select', select)):
        if value is not None:
            setattr(n, name, value if not isinstance(value, (np.ndarray, list, float, int)) else fix(value))
    return n


def envelope(gate_on=0.0):
    e = ext.ADSR()
    for name, value in (('attack', 0.001), ('decay', 0.01), ('sustain', 0.5), ('release', 0.02), ('gate_on', gate_on), ('gate_off', 0.01)):
        setattr(e, name, fix(value if isinstance(value, np.ndarray) else [[value]]))
    return e


# ---------------------------------------------------------------------------------------------- the header, compiled for the host
@pytest.fixture(scope='module')
def host_index(tmp_path_factory):
    """tests/native/sampler_index.cpp built against signals_amd/csrc/sig_sampler.h, -O2 -ffp-contract=off as the device code is built"""
    cxx = shutil.which('g++') or shutil.which('c++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = tmp_path_factory.mktemp('sampler_index') / 'sampler_index'
    subprocess.run([cxx, '-std=c++17', '-O2', '-ffp-contract=off', '-I', str(ROOT / 'signals_amd' / 'csrc'),
                    str(ROOT / 'tests' / 'native' / 'sampler_index.cpp'), '-o', str(exe)], check=True, capture_output=True, text=True)

    def run(lines):
        done = subprocess.run([str(exe)], input='\n'.join(lines) + '\n', check=True, capture_output=True, text=True, timeout=60)
        return done.stdout.split('\n')[:-1]
    return run


def hexf(x) -> str:
    x = float(x)
    return 'nan' if math.isnan(x) else ('inf' if x == math.inf else ('-inf' if x == -math.inf else x.hex()))


def unhex(s: str) -> float:
    return math.nan if 'nan' in s else (math.inf if s == 'inf' else (-math.inf if s == '-inf' else float.fromhex(s)))


def same_float(a: float, b: float) -> bool:
    """the same bits, any NaN equal to any NaN"""
    return (math.isnan(a) and math.isnan(b)) or (a == b and math.copysign(1.0, a) == math.copysign(1.0, b))


def u_cases(T, ls, le):
    """read positions around every edge of a table of T frames with the loop [ls, le) (le == 0: none)"""
    last = float(T - 1)
    us = [0.0, -0.0, 1.0, 0.5, 2.0 ** -30, last, np.nextafter(last, 0.0), np.nextafter(last, math.inf), last - 0.25, last + 0.5, float(T),
          T + 0.75, 1e6 + 0.125, 2.0 ** 40 + 0.5, 1e300, -1.0, -2.0 ** -1074, -1e-300, -0.5, math.inf, -math.inf, math.nan]
    us += [float(k) for k in range(0, T, max(1, T // 7))] + [k + 0.375 for k in range(0, T - 1, max(1, T // 5))]
    if le:
        L = le - ls
        for turns in (0, 1, 2, 1000, 2 ** 31):
            base = float(ls + turns * L)
            us += [base + (L - 1), base + (L - 1) + 0.75, np.nextafter(base + L, 0.0), base + L, base, base + 0.5,   # le - 1, just under le, le, ls
                   np.nextafter(base, 0.0)]
        us += [float(le), np.nextafter(float(le), 0.0), np.nextafter(float(le), math.inf), float(ls), le + 1e-9, 3.0 * le + 0.1]
    return [float(u) for u in us]


SHAPES = [(2, 0, 0), (5, 0, 0), (1000, 0, 0), (2, 0, 2), (2, 1, 2), (5, 1, 4), (5, 0, 5), (5, 4, 5), (1000, 100, 999), (1000, 0, 1000),
          (1000, 997, 1000), (1 << 26, 0, 0), (1 << 26, 3, (1 << 26) - 5)]


def test_host_locate_equals_the_reference_bit_for_bit(host_index):
    cases = [(u, T, ls, le) for T, ls, le in SHAPES for u in u_cases(T, ls, le)]
    got = host_index([f'U {hexf(u)} {T} {ls} {le}' for u, T, ls, le in cases])
    assert len(got) == len(cases)
    seen = set()
    for (u, T, ls, le), line in zip(cases, got):
        kind, i, j, f = line.split()
        wk, wi, wj, wf = (x.item() for x in SR.locate(np.float64(u), T, ls, le))
        assert (int(kind), int(i), int(j)) == (wk, wi, wj) and same_float(unhex(f), wf), (u, T, ls, le, line, (wk, wi, wj, wf))
        assert 0 <= wi < T and 0 <= wj < T and 0.0 <= wf < 1.0                      # every index inside the table
        if wk == SR.READ and le:
            assert wi < le and (wj == wi + 1 or (wj == ls and wi == le - 1))
            wrapped = u >= le
            seen.add(('end-1' if wi == le - 1 else ('start' if wi == ls and wf == 0 else 'inside')) if wrapped else 'before')
        elif wk == SR.READ:
            seen.add('last' if wi == T - 1 else 'plain')
            assert wj == min(wi + 1, T - 1)
        else:
            seen.add('nan' if wk == SR.NAN else 'silence')
    assert seen == {'end-1', 'start', 'inside', 'before', 'last', 'plain', 'nan', 'silence'}     # the list reaches every branch


def test_a_wrap_that_rounds_out_of_the_loop_reads_loop_start(host_index):
    """from 2^53 frames on u - loop_start and c * L are no longer exact: the wrapped position can round onto loop_end or past it (the
    rule sends it to loop_start) and the rounded quotient can exceed the true one, so that the remainder falls below loop_start
    (loop_start as well: no index leaves the loop).  Below 2^53 neither happens.  Two cases found by search, then a sweep of the
    doubles at and just under whole turns; the restatement and the header agree on each"""
    cases = [(6.933221536099853e+16, 67108855, 67108858), (1.0052640603842147e+18, 0, 5)]
    for ls, le in ((1, 4), (3, 10), (100, 999), (7, 8), (3, (1 << 26) - 5)):
        for turns in (1, 3, 1000, 10 ** 6, 2 ** 31, 2 ** 40, 2 ** 52, 2 ** 55 + 1):
            cases += [(float(np.nextafter(float(ls + turns * (le - ls)), 0.0)), ls, le), (float(ls + turns * (le - ls)), ls, le)]
    got = host_index([f'U {hexf(u)} {1 << 26} {ls} {le}' for u, ls, le in cases])
    above = below = 0
    for (u, ls, le), line in zip(cases, got):
        L = le - ls
        d = u - ls
        w = (d - math.floor(d / L) * L) + ls
        above += w >= le
        below += w < ls
        assert ls <= w < le or u >= 2.0 ** 53, (u, ls, le)
        kind, i, j, f = line.split()
        wk, wi, wj, wf = (x.item() for x in SR.locate(np.float64(u), 1 << 26, ls, le))
        assert (int(kind), int(i), int(j)) == (wk, wi, wj) and same_float(unhex(f), wf), (u, ls, le, line)
        assert wk == SR.READ and ls <= wi < le and ls <= wj < le
        if w >= le or w < ls:
            assert (wi, wf) == (ls, 0.0)
    assert above and below                                                     # the cases reach both halves of the rule


RATIOS = [0.0, 0.5, 1.0, 1.5, 2.75, -1.0]


def test_host_read_position_equals_the_reference_bit_for_bit(host_index):
    cases = []
    for rate in (48000, 44100):
        for n in (0, 1, 37, 4800, 48000, HOUR, HOUR + 255):
            t = n / rate
            for gate in (0.0, t, t - 0.01, t + 0.01, np.nextafter(t, math.inf), t - 0.5, -1.0, math.nan, math.inf):   # before, at, after the frame
                for ratio in RATIOS + [math.nan, math.inf]:
                    for offset in (0.0, 3.25, -2.0):
                        for T, ls, le in ((1000, 0, 0), (1000, 100, 999), (5, 1, 4)):
                            cases.append((n, rate, gate, ratio, offset, T, ls, le))
    got = host_index([f'P {n} {hexf(rate)} {hexf(g)} {hexf(r)} {hexf(o)} {T} {ls} {le}' for n, rate, g, r, o, T, ls, le in cases])
    assert len(got) == len(cases)
    kinds = set()
    for (n, rate, g, r, o, T, ls, le), line in zip(cases, got):
        on, u, kind, i, j, f = line.split()
        wu, won = SR.read_position(np.array([[n]]), rate, [[g]], [[r]], [[o]])
        assert bool(int(on)) == bool(won[0, 0]) and same_float(unhex(u), float(wu[0, 0])), (n, rate, g, r, o, line)
        wk, wi, wj, wf = (x.item() for x in SR.locate(wu[0, 0], T, ls, le))
        assert (int(kind), int(i), int(j)) == (wk, wi, wj) and same_float(unhex(f), wf), (n, rate, g, r, o, line)
        kinds.add((bool(won[0, 0]), wk))
    assert kinds == {(a, b) for a in (False, True) for b in (SR.SILENCE, SR.NAN, SR.READ)}
    # an hour in, ratio 1, the gate at the frame: the read starts at the offset exactly
    line, = host_index([f'P {HOUR} {hexf(48000)} {hexf(3600.0)} {hexf(1.0)} {hexf(3.25)} 1000 0 0'])
    on, u, kind, i, j, f = line.split()
    assert (on, unhex(u), kind, i, j, unhex(f)) == ('1', 3.25, '2', '3', '4', 0.25)


def test_host_column_lerp_and_shape_rule(host_index):
    selects = [0.0, -0.0, 0.99, 1.0, 1.5, 2.0, 2.999, 3.0, 7.0, 1e30, -1.0, -1e30, math.nan, math.inf, -math.inf]
    got = host_index([f'C {hexf(s)} {W}' for W in (1, 3, 64) for s in selects])
    want = [int(SR.column(s, W)) for W in (1, 3, 64) for s in selects]
    assert [int(x) for x in got] == want
    rng = np.random.default_rng(3)
    a, b = (rng.uniform(-1, 1, 300).astype(np.float32).astype(np.float64) for _ in range(2))
    f = rng.uniform(0, 1, 300); f[:10] = 0.0; b[10:20] = a[10:20]
    got = host_index([f'L {hexf(x)} {hexf(y)} {hexf(z)}' for x, y, z in zip(a, b, f)])
    assert np.array_equal(np.array([unhex(s) for s in got]).view(np.uint64), (a + f * (b - a)).view(np.uint64))
    cap = _native.SAMPLER_MAX_POINTS
    rule = [((2, 1, 0, 0), 1), ((1, 1, 0, 0), 0), ((2, 0, 0, 0), 0), ((cap, 1, 0, 0), 1), ((cap, 2, 0, 0), 0), ((cap // 2 + 1, 2, 0, 0), 0),
            ((2, cap // 2, 0, 0), 1), ((10, 1, 0, 10), 1), ((10, 1, 0, 11), 0), ((10, 1, 5, 5), 0), ((10, 1, 6, 5), 0), ((10, 1, -1, 5), 0),
            ((10, 1, 9, 10), 1), ((10, 1, 3, 0), 1), ((10, 1, -1, 0), 0), ((10, 1, 0, -1), 0)]
    got = host_index([f'S {T} {W} {ls} {le}' for (T, W, ls, le), _ in rule])
    assert [int(x) for x in got] == [ok for _, ok in rule]


# ---------------------------------------------------------------------------------------------- the restatement
def test_reference_restatement_against_a_direct_loop():
    rng = np.random.default_rng(5)
    table = rng.uniform(-1, 1, (37, 3))
    ratio = np.array([RATIOS + [math.nan, 1.0, 1.0, 0.25]])
    n_v = ratio.shape[1]
    offset = np.array([[0.0, 1.5, 3.0, 0.0, 2.25, 36.0, 0.0, -4.0, 30.5, 0.0]])
    select = np.array([[0.0, 1.0, 2.0, 7.0, -1.0, 1.9, 0.0, math.nan, 2.0, 1.0]])
    for position in (0, 48000 - 20, HOUR):
        t = position / RATE
        gate = np.array([[t, t + 10 / RATE, t - 5 / RATE, 0.0, t, t + 1.0, t, t, math.nan, t - 100 / RATE]])   # the trigger inside the block on voice 1
        for loop in ((0, 0), (3, 30), (0, 37), (35, 37)):
            got = SR.sampler(table, position, 64, ratio, offset, gate, select, *loop)
            assert got.shape == (64, n_v) and got.dtype == np.float64
            for v in range(n_v):
                for k in range(64):
                    want = SR.sampler_loop(table, position + k, RATE, ratio[0, v], offset[0, v], gate[0, v], select[0, v], *loop)
                    assert same_float(float(got[k, v]), want), (position, loop, v, k, got[k, v], want)
            assert np.isnan(got[:, 6]).all() and not np.isnan(np.delete(got, 6, axis=1)).any()       # the NaN ratio: that voice alone
            assert not got[:, 5].any() and not got[:, 8].any()                 # gated in the future; a NaN gate: silence
            assert not got[:10, 1].any()                                       # before the trigger inside the block
    two = SR.sampler(table, 100, 16, [[1.0, 0.5, 2.0], [0.5, 1.0, 1.0]], [[0.0], [3.0]], 0.0, [[0.0, 1.0, 2.0]], blocks=2)
    want = np.concatenate([SR.sampler(table, 100, 16, [[1.0, 0.5, 2.0]], 0.0, 0.0, [[0.0, 1.0, 2.0]]),
                           SR.sampler(table, 116, 16, [[0.5, 1.0, 1.0]], 3.0, 0.0, [[0.0, 1.0, 2.0]])])
    assert np.array_equal(two, want, equal_nan=True)
    stepped = SR.sampler(table, 0, 4, [[1.0]], 0.0, 0.0, 0.0, step=8)          # block-rate reads: frames 0, 8, 16, 24
    assert np.array_equal(stepped[:, 0], np.float32(table[[0, 8, 16, 24], 0]).astype(np.float64))


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32)


def test_identities_bit_for_bit():
    """in the float32 the node stores.  s = (n / rate - gate_on) * rate is n - gate_on * rate only to within an ulp (one frame in
    twelve at 48 kHz is off by one), so the float64 value is within 2^-50 of the table entry and its float32 IS the entry; where s is
    exact so is the float64 value"""
    rng = np.random.default_rng(6)
    T, W = 100, 3
    table = rng.uniform(-1, 1, (T, W))
    held = table.astype(np.float32)
    n = np.arange(160)
    exact = (n / RATE) * RATE == n
    assert exact[T - 1] and not exact.all()
    out = SR.sampler(table, 0, 160, 1.0, 0.0, 0.0, [[0.0, 1.0, 2.0]])
    assert np.array_equal(f32(out[:T]), held) and not out[T:].any()            # ratio 1, offset 0, gate 0: the table, then zeros
    assert np.array_equal(out[:T][exact[:T]], held.astype(np.float64)[exact[:T]])
    # from a trigger half a second in (q - gate_on is exact there) and an offset: the same, shifted; an hour in q = n / rate carries
    # 2^-42 s, 1e-8 frames: the table to that much
    out = SR.sampler(table, 24000, 64, 1.0, 7.0, 0.5, [[0.0, 1.0, 2.0]])
    assert np.array_equal(f32(out), held[7:71])
    out = SR.sampler(table, HOUR, 64, 1.0, 7.0, HOUR / RATE, [[0.0, 1.0, 2.0]])
    assert np.abs(out - held[7:71]).max() < 2 * 1e-8 * 2
    # a loop over the whole table: periodic in T
    looped = SR.sampler(table, 0, 5 * T, 1.0, 0.0, 0.0, [[0.0, 1.0, 2.0]], 0, T)
    assert np.array_equal(f32(looped), np.tile(held, (5, 1)))
    part = SR.sampler(table, 0, 400, 1.0, 0.0, 0.0, 0.0, 20, 60)               # attack, then the loop's 40 frames for ever
    assert np.array_equal(f32(part[:60, 0]), held[:60, 0]) and np.array_equal(f32(part[60:, 0]), np.tile(held[20:60, 0], 9)[:340])
    assert np.array_equal(SR.sampler(table, 0, 50, 0.0, 17.0, 0.0, 1.0)[:, 0], np.full(50, np.float64(held[17, 1])))      # ratio 0: one frame held
    # the definition's edge: where s rounds above T - 1 at the recording's last frame, that frame is outside
    assert (7 / RATE) * RATE > 7 and SR.sampler(table[:8], 0, 8, 1.0, 0.0, 0.0, 0.0)[7, 0] == 0.0


# ---------------------------------------------------------------------------------------------- the node
def test_node_api():
    cls = ext.Sampler
    assert cls.port_names() == ['gate_on', 'offset', 'ratio', 'select']
    assert cls.flags() & SignalFlags.GENERATOR and cls.flags() & SignalFlags.EPOCH and not cls.flags() & SignalFlags.EFFECT
    assert issubclass(cls, BlockCachingEmitter) and not issubclass(cls, osc.Osc) and not issubclass(cls, ext.Wavetable)
    assert {'table', 'loop_start', 'loop_end'} <= set(cls().state_attrs())
    s = cls().get_state()
    assert np.array_equal(s.table, [[0.0], [0.0]]) and (s.loop_start, s.loop_end) == (0, 0)
    assert _native.SAMPLER_MAX_POINTS == 2 ** 26
    n = sampler_node(np.zeros((10, 2)), ratio=np.ones((1, 6)), gate_on=[[0.0]])
    assert n.channels == 6                                                    # ImplicitChannels: the one width that is not 1
    n.offset = fix(np.zeros((1, 4)))
    with pytest.raises(ValueError):
        n.channels                                                            # 6 and 4: no single width
    doc = ' '.join(cls.__doc__.split())
    for words in ('q = n / rate', 'e = q - gate_on[v]', 's = e * rate', 'u = s * ratio[v] + offset[v]', 'not (e >= 0)', 'j = min(i + 1, T - 1)',
                  'c = floor((u - loop_start) / L)', 'j = (i + 1 >= loop_end) ? loop_start : i + 1', 'tbl[i, w] + f * (tbl[j, w] - tbl[i, w])',
                  'pure function of the absolute frame', 'RingMod(Sampler, ADSR)', 'Out of scope', 'carried read pointer', 'a frame-rate `ratio`',
                  'above linear', 'anti-aliasing', 'fold it into `ratio`', 'reverse loops and crossfades', 'voice program', 'specialised build',
                  'fused kernels', 'control path', 'table_from_wav'):
        assert words in doc, words


@pytest.mark.parametrize('bad', [np.zeros(4), np.zeros((2, 2, 2)), np.zeros((1, 4)), np.zeros((4, 0)), np.zeros((4, 2), dtype=complex),
                                 [[0.0], [1.0]], None, np.array([['a'], ['b']]), np.zeros((2 ** 13 + 1, 2 ** 13), dtype=np.int8)],
                         ids=['1-D', '3-D', 'T=1', 'W=0', 'complex', 'a list', 'None', 'strings', 'over the cap'])
def test_table_validation_refuses(bad):
    n = ext.Sampler()
    with pytest.raises(BadStateValue):
        n.get_state().table = bad


def test_state_validation_and_the_resident_copy():
    n = ext.Sampler()
    s = n.get_state()
    for good in (np.zeros((2, 1)), np.ones((7, 5)), np.ones((4, 2), dtype=np.float32), np.arange(6, dtype=np.uint8).reshape(3, 2),
                 np.zeros((2 ** 13, 2 ** 13), dtype=np.int8)):                 # the cap itself
        s.table = good
    s.table = np.array([[0, 10], [1, 11], [2, 12]])                           # int64, what a .sigs value arrives as
    got = n.resident_table()
    assert got.dtype.is_floating_point and got.element_size() == 4 and tuple(got.shape) == (2, 3) and got.is_contiguous()
    assert got.tolist() == [[0.0, 1.0, 2.0], [10.0, 11.0, 12.0]]              # the transpose: every recording contiguous
    assert n.resident_table() is got                                          # unchanged: no second upload
    s.table[1, 1] = 5                                                         # an in-place edit is seen at the next render
    assert n.resident_table().tolist() == [[0.0, 1.0, 2.0], [10.0, 5.0, 12.0]]
    s.table = np.array([[1.5], [2.5]])                                        # so is a replaced array
    assert n.resident_table().tolist() == [[1.5, 2.5]]
    # the loop: integers >= 0, loop_start < loop_end where a loop is on; the table's length at render time
    for name in ('loop_start', 'loop_end'):
        for bad in (-1, 1.0, True, None, '3', np.float64(2.0)):
            with pytest.raises(BadStateValue):
                setattr(s, name, bad)
    s.table = np.zeros((10, 1))
    s.loop_start = 4                                                          # no loop yet: any start
    with pytest.raises(BadStateValue):
        s.loop_end = 4
    with pytest.raises(BadStateValue):
        s.loop_end = 3
    s.loop_end = np.int64(10)
    assert n.loop() == (4, 10)
    with pytest.raises(BadStateValue):
        s.loop_start = 10
    s.loop_end = 11                                                           # longer than the table: the state alone cannot tell ...
    with pytest.raises(BadStateValue, match='loop_end <= 10 frames'):
        n.loop()                                                              # ... the render does
    s.table = np.zeros((11, 1))
    assert n.loop() == (4, 11)
    s.table = np.zeros((5, 2))                                                # a replaced, shorter table
    with pytest.raises(BadStateValue):
        n.loop()
    s.loop_end = 0
    assert n.loop() == (4, 0)                                                 # no loop: the start is not looked at


def test_the_eager_node_checks_the_loop_before_it_launches(stubbed):
    from helpers import render
    n = sampler_node(np.zeros((10, 1)), ratio=row(0.5, 2.0), gate_on=[[0.0]], loop=(2, 10))
    out = render(n, 0, 64, V)
    assert out.shape == (64, V) and out.dtype == np.float32
    one = render(n, 4096, 1, V)
    assert one.shape == (1, V) and one.dtype == np.float64                    # a one-frame request: float64
    name, a = stubbed.calls[0]
    assert name == 'sig_sampler_play' and a[:6] == (0, 1, RATE, 64, V, 0) and a[19:23] == (10, 1, 2, 10)
    assert a[6] is not None and a[7:9] == (1, 0) and a[9] is not None and a[10:12] == (0, 0)      # ratio per voice, offset unplugged: zeros((1, 1))
    n.get_state().table = np.zeros((5, 1))
    launched = len(stubbed.calls)
    with pytest.raises(BadStateValue):
        render(n, 128, 64, V)
    assert len(stubbed.calls) == launched


def test_class_resolves_by_qualified_name_and_loads_from_a_patch():
    from signals_amd.chain import discovery, sigs
    from signals_amd.chain.driver import load_signal
    assert load_signal('signals_amd.chain.ext.Sampler') is ext.Sampler
    assert load_signal('signals.chain.ext.Sampler') is ext.Sampler
    assert discovery.load_signal('signals.chain.ext.Sampler') is ext.Sampler
    assert ext.Sampler().cls_name().endswith('chain.ext.Sampler')
    p = sigs.loads('+ 1a signals.chain.fixed.Fixed value=[[1.0,0.5]]\n+ 1b signals.chain.fixed.Fixed value=[[0.25]]\n'
                   '+ 2a signals.chain.ext.Sampler loop_start=1 loop_end=3 table=[[0,3],[1,2],[2,1],[3,0]]\n> 1a 2a.ratio\n> 1b 2a.gate_on')
    node = p['2a']
    assert isinstance(node, ext.Sampler) and node.ratio.sig is p['1a'] and node.gate_on.sig is p['1b'] and node.offset.sig is None
    s = node.get_state()
    assert s.table.shape == (4, 2) and s.table.dtype.kind == 'i' and node.loop() == (1, 3)
    assert node.resident_table().tolist() == [[0.0, 1.0, 2.0, 3.0], [3.0, 2.0, 1.0, 0.0]]
    with pytest.raises(BadStateValue):
        sigs.loads('+ 1a signals.chain.ext.Sampler table=[[1,2,3]]')
    with pytest.raises(BadStateValue):
        sigs.loads('+ 1a signals.chain.ext.Sampler loop_end=2 loop_start=2')


def test_table_from_wav_reads_what_file_writer_wrote(tmp_path):
    rng = np.random.default_rng(8)
    block = rng.uniform(-1, 1, (300, 2)).astype(np.float32)
    for subtype, want in (('FLOAT', block.astype(np.float64)), ('PCM_16', np.rint(block.astype(np.float64) * 32767.0) / 32768.0)):
        w = files.FileWriter()
        w.get_state().path = str(tmp_path / f'{subtype}.wav')
        w.get_state().subtype = subtype
        import torch
        w.write_rows(0, RATE, 2, torch.from_numpy(block[:200]))
        w.write_rows(200, RATE, 2, torch.from_numpy(block[200:]))
        w.destroy()
        table = ext.Sampler.table_from_wav(tmp_path / f'{subtype}.wav')
        assert table.shape == (300, 2) and table.dtype == np.float64 and table.flags['C_CONTIGUOUS']
        assert np.array_equal(table, want)
        n = ext.Sampler()
        n.get_state().table = table                                           # a table the state takes as it is
        assert tuple(n.resident_table().shape) == (2, 300)
    with pytest.raises(ValueError):
        (tmp_path / 'not.wav').write_bytes(b'nothing of the kind')
        ext.Sampler.table_from_wav(str(tmp_path / 'not.wav'))


# ---------------------------------------------------------------------------------------------- C ABI
def test_entry_point_is_exported_and_declared(lib):
    assert 'sig_sampler_play' in _native.EXPORTS
    raw = ctypes.CDLL(str(_native.LIB_PATH))
    assert raw.sig_sampler_play is not None
    assert lib.sig_abi_version() == 7                                         # additive
    header = (ROOT / 'include' / 'signals_amd.h').read_text()
    assert 'int sig_sampler_play(' in header and '#define SIG_ABI_VERSION 7' in header
    assert 'SIG_SAMPLER_MAX_POINTS = 1 << 26' in header
    assert 'sig_sampler_play' in (ROOT / 'INTEGRATION.md').read_text()
    shared = (ROOT / 'signals_amd' / 'csrc' / 'sig_sampler.h').read_text()
    assert '__host__ __device__' in shared and 'hip_runtime' not in shared and 'sig_common' not in shared    # one text for both sides, nothing of HIP in it
    assert '"sig_sampler.h"' in (ROOT / 'signals_amd' / 'csrc' / 'sampler.hip').read_text()


def test_sampler_play_argument_errors_do_not_reach_the_device(lib):
    p = 64                                                                    # (never dereferenced: every call fails its checks)
    args = dict(position=4096, step=1, rate=48000, rows=512, voices=8, rpp=256,
                ratio=p, rs=1, rrs=8, offset=p, os=1, ors=8, gate=p, gs=0, grs=0, select=p, ss=1, srs=8,
                table=p, T=1000, W=4, ls=0, le=0, out=p, odt=0, old=8, stream=None)

    def call(**over):
        a = dict(args, **over)
        return lib.sig_sampler_play(*(a[k] for k in args))
    assert call(table=None) == INV and call(out=None) == INV                  # a null table or out
    assert call(T=1) == INV and call(T=0) == INV and call(T=-5) == INV and call(W=0) == INV and call(W=-1) == INV
    assert call(T=2 ** 26, W=2) == INV and call(T=2 ** 25 + 1, W=2) == INV and call(T=2 ** 30, W=2 ** 30) == INV    # T * W over the cap
    assert call(le=1001) == INV and call(ls=5, le=5) == INV and call(ls=6, le=5) == INV and call(ls=-1, le=5) == INV
    assert call(le=-1) == INV and call(ls=-1) == INV and call(ls=1000, le=1000) == INV
    assert call(old=7) == INV and call(old=0) == INV                          # rows narrower than the voices
    for name in ('rs', 'os', 'gs', 'ss'):
        assert call(**{name: 2}) == INV and call(**{name: -1}) == INV         # strides other than 0 or 1
    for name in ('rrs', 'ors', 'grs', 'srs'):
        assert call(**{name: -1}) == INV
    assert call(rows=-1) == INV and call(voices=-1) == INV and call(rate=0) == INV and call(position=-1) == INV
    assert call(step=0) == INV and call(rpp=-1) == INV and call(odt=2) == INV
    # accepted, nothing to launch: no rows, no voices -- at the cap, with every loop the rule allows, with every port unplugged
    assert call(rows=0) == 0 and call(voices=0, old=0) == 0
    assert call(rows=0, T=2 ** 26, W=1) == 0 and call(rows=0, T=2, W=2 ** 25) == 0 and call(rows=0, T=2, W=1) == 0
    assert call(rows=0, le=1000) == 0 and call(rows=0, ls=999, le=1000) == 0 and call(rows=0, ls=0, le=1) == 0 and call(rows=0, ls=7) == 0
    assert call(rows=0, ratio=None, offset=None, gate=None, select=None) == 0 and call(rows=0, odt=1) == 0
    assert call(rows=0, step=256, rpp=1) == 0


# ---------------------------------------------------------------------------------------------- planning
def test_purity_and_modulation_classification():
    from signals_amd.engine import _KNOWN_TYPES, _audio_ports, _control_ports, _ctl_const, _foreign, _is_pure, _modulated
    assert ext.Sampler in _KNOWN_TYPES
    s = sampler_node(np.zeros((10, 1)), ratio=row(0.5, 2.0), gate_on=[[0.0]])
    assert not _foreign(s)
    assert _control_ports(s) == [s.ratio, s.offset, s.gate_on, s.select] and _audio_ports(s) == []
    assert all(_ctl_const(p) for p in _control_ports(s)) and not _modulated(s)
    assert _is_pure(s, {})                                                    # constant controls: a pure function of the position
    g = fx.Gain(); g.left = s; g.right = fix([[0.5]])
    assert _is_pure(g, {})
    swept = sampler_node(np.zeros((10, 1)), ratio=mkosc(osc.Sine, [[0.5]]), gate_on=[[0.0]])
    assert _modulated(swept) and not _is_pure(swept, {})                      # like an oscillator with an LFO on hertz


def test_a_pure_sampler_needs_no_history_of_its_own_and_renders_a_filters():
    from signals_amd.engine import _Batch
    s = sampler_node(np.zeros((10, 1)), ratio=row(0.5, 2.0), gate_on=[[0.0]])
    lp = fx.LowPass(); lp.input = s; lp.cutoff = fix(row(500, 5000))
    for pos, want in ((0, 0), (37, 37), (4096, 100)):
        batch = _Batch(types.SimpleNamespace(rate=RATE), pos, 256, 2, False)
        batch._require(lp, V, 0)
        assert batch._need[(lp, V)] == 0 and batch._need[(s, V)] == want, pos


class _Recorder:
    """stands in for engine.KernelTimer: the launch labels in order"""
    region = False

    def __init__(self):
        self.names = []

    def launch(self, name, fn, **meta):
        self.names.append(name)
        return fn()


@pytest.fixture
def stubbed(monkeypatch):
    """every entry point of the library answers 0 without touching its arguments: the planner runs on CPU tensors"""
    class Lib:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            def entry(*a):
                self.calls.append((name, a))
                return 0
            return entry
    one = Lib()
    monkeypatch.setattr(_native, 'lib', lambda: one)
    monkeypatch.setattr(_native, '_gpu', lambda *a: None)
    monkeypatch.setattr(_native, '_stream', lambda t: 0)
    return one


FUSED = ('fused', 'latency', 'cascade', 'steady', 'walk', 'biquad_bus', 'biquad_coldstart_env', 'voice_program')
SETTINGS = ({}, {'fuse_program': 'always'}, {'fuse': False})


def voice(shape, modulated=False, loop=None):
    ratio = row(0.5, 2.0)
    if modulated:
        ratio = fx.Mix(); ratio.left = mkosc(osc.Sine, [[0.7]]); ratio.right = fix(row(0.5, 2.0)); ratio.mix = fix([[0.01]])
    s = sampler_node(SR.burst(64, 2), ratio=ratio, gate_on=[[0.001]], select=row(0, 1.9), loop=loop)
    if shape == 'sampler':
        return s, V
    if shape == 'lowpass':
        top = fx.LowPass(); top.input = s; top.cutoff = fix(row(500, 5000))
        return top, V
    rm = fx.RingMod(); rm.left = s; rm.right = envelope(row(0.001, 0.002))
    b = ext.SumBus(); b.input = rm
    return b, 1


@pytest.mark.parametrize('shape', ['sampler', 'enveloped_bus', 'lowpass'])
def test_launch_labels_on_every_renderer_setting(stubbed, shape):
    """one kernel per node whatever the renderer is allowed: the sampler through sig_sampler_play, what surrounds it on the route it
    has without the node -- RingMod(x, ADSR) as the one envelope pass where fusing is on, the LowPass as the cold-start filter"""
    from signals_amd.engine import BatchRenderer
    around = {'sampler': ({}, {}, {}),
              'enveloped_bus': ({'adsr_apply', 'sum_bus'}, {'adsr_apply', 'sum_bus'}, {'adsr', 'elementwise[RingMod]', 'sum_bus'}),
              'lowpass': ({'biquad_coldstart[lp]'},) * 3}[shape]
    launched = 0
    for kw, others in zip(SETTINGS, around):
        for modulated, loop, label in ((False, None, 'sampler_play[OneShot]'), (True, (8, 60), 'sampler_play[Loop,per-block]')):
            top, C = voice(shape, modulated, loop)
            rec = _Recorder()
            r = BatchRenderer(top, C, RATE, timer=rec, **kw)
            r.render(0, 256, 3)
            r.render(768, 256, 2)                                             # continuing
            r.render(8192, 256, 2)                                            # fresh
            assert not any(word in n for n in rec.names for word in FUSED), (kw, rec.names)
            plays = [n for n in rec.names if n.startswith('sampler_play')]
            assert set(plays) == {label} and len(plays) >= 3, (kw, rec.names)
            rest = {n for n in rec.names if not n.startswith('sampler_play') and 'block-rate' not in n and not n.startswith('control_program')}
            assert rest == set(others), (kw, modulated, rec.names)
            launched += len(plays)
            assert [name for name, _ in stubbed.calls].count('sig_sampler_play') == launched


def test_the_voice_program_declines_a_graph_with_the_node():
    from signals_amd.engine import _VoiceProgram
    for shape in ('sampler', 'enveloped_bus', 'lowpass'):
        top, _ = voice(shape)
        assert _VoiceProgram.compile(None, top.input.sig if shape == 'enveloped_bus' else top, V) is None
    assert ext.Sampler not in _VoiceProgram.KERNEL_NODES and not issubclass(ext.Sampler, _VoiceProgram.KERNEL_NODES)


def test_the_launch_carries_the_rows_the_table_and_the_loop(stubbed):
    from signals_amd.engine import BatchRenderer
    top, _ = voice('sampler', modulated=True, loop=(8, 60))
    BatchRenderer(top, V, RATE).render(4096, 256, 3)
    (a,) = [a for name, a in stubbed.calls if name == 'sig_sampler_play']
    position, step, rate, rows, voices, rpp = a[:6]
    assert (position, step, rate, rows, voices, rpp) == (4096, 1, RATE, 768, V, 256)
    ratio, offset, gate, select = (a[6 + 3 * k:9 + 3 * k] for k in range(4))
    assert ratio[0] is not None and ratio[1:] == (1, V)                       # per-block rows of the modulated port: K rows, V apart
    assert gate[0] is not None and gate[1:] == (0, 0) and select[0] is not None and select[1:] == (1, 0)
    assert a[18] == top.resident_table().data_ptr() and a[19:23] == (64, 2, 8, 60)
    assert a[24] == _native.F32 and a[25] >= V
    # constant controls: one launch over history and blocks alike, one control row
    top, _ = voice('lowpass')
    stubbed.calls.clear()
    BatchRenderer(top, V, RATE, fuse=False).render(4096, 256, 2)
    (a,) = [a for name, a in stubbed.calls if name == 'sig_sampler_play']
    assert a[:6] == (4096 - 100, 1, RATE, 100 + 512, V, 0) and a[22] == 0      # the filter's 100 context rows are simply rendered


def test_narrow_controls_and_a_bad_loop_raise_in_the_batch_as_in_the_node(stubbed):
    from signals_amd.engine import BatchRenderer
    BatchRenderer(sampler_node(np.zeros((10, 1)), ratio=[[1.0]], gate_on=[[0.0]]), V, RATE).render(0, 256, 2)     # width 1: its natural width
    a = [a for name, a in stubbed.calls if name == 'sig_sampler_play'][-1]
    assert a[4] == 1
    with pytest.raises(IndexError, match='index 3 is out of bounds for axis 1 with size 3'):
        BatchRenderer(sampler_node(np.zeros((10, 1)), ratio=row(0.5, 2.0, 3), gate_on=[[0.0]]), V, RATE).render(0, 256, 2)
    n = sampler_node(np.zeros((10, 1)), ratio=row(0.5, 2.0), gate_on=[[0.0]], loop=(2, 10))
    n.get_state().table = np.zeros((5, 1))
    with pytest.raises(BadStateValue):
        BatchRenderer(n, V, RATE).render(0, 256, 2)


def test_a_sampler_in_a_control_path_is_refused_with_its_reason():
    from signals_amd.engine import NotBatchable, _Batch, _ControlProgram
    s = sampler_node(SR.burst(64), ratio=[[1.0]], gate_on=[[0.0]])
    with pytest.raises(NotBatchable, match='a sampler has no block-rate program'):
        _ControlProgram((s,), 4, channels=1)
    g = fx.Gain(); g.left = s; g.right = fix([[100.0]])
    with pytest.raises(NotBatchable, match='a sampler has no block-rate program'):
        _ControlProgram((g,), 4, channels=1)
    batch = _Batch(types.SimpleNamespace(rate=RATE), 0, 256, 4, False)
    with pytest.raises(NotBatchable, match=r'Sampler in a control path: a sampler has no block-rate schedule \(the eager node serves one-frame requests\)'):
        batch._control_node(s, 'cutoff')
