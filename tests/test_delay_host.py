"""The short multi-tap delay line without a GPU: the node API of ext.Delay and its state validation, name resolution and the .sigs
loader, sig_delay_taps's export, declaration and argument checks, the tap arithmetic of sig_delay.h compiled for the host
(tests/native/delay_taps.cpp) against the numpy restatement (tests/delay_reference.py) bit for bit, that restatement against a
direct loop, and how the engine's planner classifies and schedules the node: a filter's history, never pure, the refusals, no fused
matcher and no voice program."""
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
from signals_amd.chain import ext, fixed, fx, osc

import delay_reference as DR

ROOT = pathlib.Path(__file__).resolve().parent.parent
INV = 1     # hipErrorInvalidValue
RATE, V = 48000, 8


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


def delay_node(input_, time=None, taps=None):
    n = ext.Delay()
    if taps is not None:
        n.get_state().taps = np.asarray(taps)
    n.input = input_
    if time is not None:
        n.time = time if not isinstance(time, (np.ndarray, list, float)) else fix(time)
    return n


# ---------------------------------------------------------------------------------------------- the restatement
# the delays in frames the cases are built from: 0, integers, the last fraction below 99, 99, beyond, negative, infinities, NaN
D_CASES = [0.0, -0.0, 1.0, 2.0, 37.0, 98.0, 98.999, 99.0, 99.0 - 2.0 ** -46, 99.5, 1e6, 0.5, 2.0 ** -30, 17.25, 63.999999, -1.0, -1e-300,
           math.inf, -math.inf, math.nan]
M_CASES = [1.0, 0.5, 2.0, 0.0, -1.0, 1.0 / 3.0, 7.0]


def test_reference_restatement_against_a_direct_loop():
    rng = np.random.default_rng(5)
    frames, c0, position = 40, 37, 37                                          # c0 < 100: the zero fill is exercised
    x = rng.uniform(-1, 1, (c0 + frames, 1))
    taps = [(1.0, 0.75), (0.5, -0.5), (2.0, 0.25), (0.0, 1.0)]
    time = np.array([[d / RATE for d in D_CASES]])
    got = DR.delay_block(x, c0, frames, time, RATE, taps)
    assert got.shape == (frames, len(D_CASES)) and got.dtype == np.float64
    series = [float(v) for v in x[:, 0]]                                       # entry k is absolute frame k: position == c0
    for v, t in enumerate(time[0]):
        for n in range(frames):
            want = DR.delay_loop(series, position + n, float(t), RATE, taps)
            assert got[n, v] == want or (math.isnan(want) and math.isnan(got[n, v])), (v, n)
    # the NaN voice, and the +-inf voices through the tap with m = 0 (inf * 0 is NaN), every row of them; no other
    assert np.isnan(got[:, -3:]).all() and not np.isnan(got[:, :-3]).any()
    alone = DR.delay_block(x, c0, frames, time, RATE, taps[:3])
    assert np.isnan(alone[:, -1]).all() and not np.isnan(alone[:, :-1]).any()  # without that tap: +inf -> 99, -inf -> 0


def test_reference_identity_shift_and_blocks():
    rng = np.random.default_rng(6)
    x = rng.uniform(-1, 1, (100 + 64, 3))
    assert np.array_equal(DR.delay_block(x, 100, 64, [[0.0]], RATE, [(1.0, 1.0)]), x[100:])                 # the identity
    assert np.array_equal(DR.delay_block(x, 100, 64, [[17 / RATE * 1.0]], 48000, [(1.0, 1.0)]).shape, (64, 3))
    shifted = DR.delay_block(x, 100, 64, [[0.25]], 100, [(1.0, 1.0)])          # t * rate = 25 exactly
    assert np.array_equal(shifted, x[75:75 + 64])
    far = DR.delay_block(x, 100, 64, [[1.0]], RATE, [(1.0, 1.0)])              # beyond 99: clipped
    assert np.array_equal(far, x[1:1 + 64])
    early = DR.delay_block(x[100:], 0, 64, [[0.25]], 100, [(1.0, 1.0)])        # position 0: zeros in front
    assert np.array_equal(early[:25], np.zeros((25, 3))) and np.array_equal(early[25:], x[100:100 + 39])
    two = DR.delay(x, 100, 32, [[0.0, 0.1, 0.2], [0.25, 0.0, 0.05]], 100, [(1.0, 1.0), (0.5, -1.0)], blocks=2)
    want = np.concatenate([DR.delay_block(x, 100, 32, [[0.0, 0.1, 0.2]], 100, [(1.0, 1.0), (0.5, -1.0)]),
                           DR.delay_block(x[32:], 100, 32, [[0.25, 0.0, 0.05]], 100, [(1.0, 1.0), (0.5, -1.0)])])
    assert np.array_equal(two, want)


# ---------------------------------------------------------------------------------------------- the header, compiled for the host
@pytest.fixture(scope='module')
def host_taps(tmp_path_factory):
    """tests/native/delay_taps.cpp built against signals_amd/csrc/sig_delay.h, -O2 -ffp-contract=off as the device code is built"""
    cxx = shutil.which('g++') or shutil.which('c++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = tmp_path_factory.mktemp('delay_taps') / 'delay_taps'
    subprocess.run([cxx, '-std=c++17', '-O2', '-ffp-contract=off', '-I', str(ROOT / 'signals_amd' / 'csrc'),
                    str(ROOT / 'tests' / 'native' / 'delay_taps.cpp'), '-o', str(exe)], check=True, capture_output=True, text=True)

    def run(lines):
        done = subprocess.run([str(exe)], input='\n'.join(lines) + '\n', check=True, capture_output=True, text=True, timeout=60)
        return done.stdout.split('\n')[:-1]
    return run


def hexf(x) -> str:
    x = float(x)
    return 'nan' if math.isnan(x) else ('inf' if x == math.inf else ('-inf' if x == -math.inf else x.hex()))


def test_host_tap_arithmetic_equals_the_reference_bit_for_bit(host_taps):
    cases = [(d / rate, rate, m) for rate in (48000.0, 44100.0, 100.0) for d in D_CASES for m in M_CASES]
    got = host_taps([f'T {hexf(t)} {hexf(rate)} {hexf(m)}' for t, rate, m in cases])
    assert len(got) == len(cases)
    kinds = set()
    for (t, rate, m), line in zip(cases, got):
        ok, i, f = line.split()
        wi, wf, nan = DR.taps_of([[t]], rate, [(m, 1.0)])
        assert (ok == '0') == bool(nan[0]), (t, rate, m)
        assert int(i) == int(wi[0, 0]) and 0 <= int(i) <= 99, (t, rate, m, line)
        assert float.fromhex(f) == wf[0, 0] and math.copysign(1.0, float.fromhex(f)) == math.copysign(1.0, wf[0, 0]) and 0.0 <= wf[0, 0] < 1.0
        kinds.add('nan' if nan[0] else ('zero' if wi[0, 0] == 0 and wf[0, 0] == 0 else ('cap' if wi[0, 0] == 99 else
                  ('whole' if wf[0, 0] == 0 else 'fraction'))))
    assert kinds == {'nan', 'zero', 'cap', 'whole', 'fraction'}               # the list reaches every branch


def test_host_read_and_sum_equal_numpy_bit_for_bit(host_taps):
    rng = np.random.default_rng(7)
    n = 400
    u = rng.integers(0, 3, n)
    acc, g, x0, x1 = (rng.uniform(-2, 2, n) for _ in range(4))
    f = rng.uniform(0, 1, n)
    f[:20] = 0.0
    x0[20:30] = np.float32(x0[20:30]); x1[20:30] = x0[20:30]                   # equal neighbours
    x0[30], x1[31], acc[32] = math.nan, math.inf, -0.0
    got = host_taps([f'S {int(u[k])} {hexf(acc[k])} {hexf(g[k])} {hexf(x0[k])} {hexf(x1[k])} {hexf(f[k])}' for k in range(n)])
    with np.errstate(invalid='ignore'):
        p = g * (x0 + f * (x1 - x0))
        want = np.where(u == 0, p, acc + p)
    have = np.array([float.fromhex(s) if 'nan' not in s else math.nan for s in got])
    both = np.isnan(want)
    assert np.array_equal(np.isnan(have), both)
    assert np.array_equal(have[~both].view(np.uint64), want[~both].view(np.uint64))


# ---------------------------------------------------------------------------------------------- the node
def test_node_api():
    cls = ext.Delay
    assert cls.port_names() == ['input', 'time']
    assert cls.flags() & SignalFlags.EFFECT and not cls.flags() & SignalFlags.GENERATOR
    assert issubclass(cls, BlockCachingEmitter) and not issubclass(cls, fx.CritFilter) and not issubclass(cls, fx.Effect)
    assert 'taps' in cls().state_attrs()
    assert np.array_equal(cls().get_state().taps, [[1.0, 1.0]])               # one tap at `time`
    assert _native.DELAY_MAX_FRAMES == 99 and _native.DELAY_MAX_TAPS == 16 and cls().context_frames() == 100
    n = delay_node(mkosc(osc.Sawtooth, np.full((1, 6), 220.0)), time=[[0.001]])
    assert n.channels == 6                                                    # ImplicitChannels: the one width that is not 1
    n.time = fix(np.zeros((1, 4)))
    with pytest.raises(ValueError):
        n.channels                                                            # 6 and 4: no single width
    doc = ' '.join(cls.__doc__.split())
    for words in ('clip((t * rate) * m_u, 0, 99)', 'floor(d_u)', 'x[n - i_u - 1] - x[n - i_u]', 'ascending u', 'Out of scope', 'beyond 99 frames',
                  'feedback', 'a frame-rate `time`', 'above linear', 'voice program', 'control path', 'bit for bit'):
        assert words in doc, words


@pytest.mark.parametrize('bad', [np.zeros(2), np.zeros((2, 2, 2)), np.zeros((0, 2)), np.zeros((17, 2)), np.zeros((3, 3)), np.zeros((3, 1)),
                                 np.zeros((2, 2), dtype=complex), np.array([[1.0, np.nan]]), np.array([[np.inf, 1.0]]), [[1.0, 1.0]], None,
                                 np.array([['a', 'b']])],
                         ids=['1-D', '3-D', 'U=0', 'U=17', 'three columns', 'one column', 'complex', 'NaN', 'inf', 'a list', 'None', 'strings'])
def test_state_validation_refuses(bad):
    n = ext.Delay()
    with pytest.raises(BadStateValue):
        n.get_state().taps = bad


def test_state_validation_accepts():
    n = ext.Delay()
    for good in (np.zeros((1, 2)), np.ones((16, 2)), np.ones((4, 2), dtype=np.float32), np.array([[-1.0, -2.0]]),
                 np.arange(6, dtype=np.uint8).reshape(3, 2)):
        n.get_state().taps = good
    n.get_state().taps = np.array([[1, 1], [2, -1]])                          # int64, what a .sigs value arrives as
    assert n.get_state().taps.dtype == np.int64
    got = n.host_taps()
    assert got.dtype == np.float64 and got.flags['C_CONTIGUOUS'] and got.tolist() == [[1.0, 1.0], [2.0, -1.0]]
    n.get_state().taps[1, 1] = 3                                              # an in-place edit is seen at the next launch
    assert n.host_taps().tolist() == [[1.0, 1.0], [2.0, 3.0]]
    U, m, g = _native._taps(n.host_taps())
    assert U == 2 and list(m) == [1.0, 2.0] and list(g) == [1.0, 3.0]
    with pytest.raises(_native.NativeError):
        _native._taps(np.zeros((17, 2)))


def test_class_resolves_by_qualified_name_and_loads_from_a_patch():
    from signals_amd.chain import discovery, sigs
    from signals_amd.chain.driver import load_signal
    assert load_signal('signals_amd.chain.ext.Delay') is ext.Delay
    assert load_signal('signals.chain.ext.Delay') is ext.Delay
    assert discovery.load_signal('signals.chain.ext.Delay') is ext.Delay
    assert ext.Delay().cls_name().endswith('chain.ext.Delay')
    p = sigs.loads('+ 1a signals.chain.fixed.Fixed value=[[220.0]]\n+ 1b signals.chain.fixed.Fixed value=[[0.001]]\n'
                   '+ 1c signals.chain.osc.Sawtooth\n'
                   '+ 2a signals.chain.ext.Delay taps=[[1,1],[2,-1]]\n> 1a 1c.hertz\n> 1c 2a.input\n> 1b 2a.time')
    node = p['2a']
    assert isinstance(node, ext.Delay) and node.input.sig is p['1c'] and node.time.sig is p['1b']
    assert node.get_state().taps.shape == (2, 2) and node.get_state().taps.dtype.kind == 'i'
    with pytest.raises(BadStateValue):
        sigs.loads('+ 1a signals.chain.ext.Delay taps=[[1,1,1]]')


# ---------------------------------------------------------------------------------------------- C ABI
def test_entry_point_is_exported_and_declared(lib):
    assert 'sig_delay_taps' in _native.EXPORTS
    raw = ctypes.CDLL(str(_native.LIB_PATH))
    assert raw.sig_delay_taps is not None
    assert lib.sig_abi_version() == 7                                         # additive
    header = (ROOT / 'include' / 'signals_amd.h').read_text()
    assert 'int sig_delay_taps(' in header and '#define SIG_ABI_VERSION 7' in header
    assert 'SIG_DELAY_CONTEXT = 100, SIG_DELAY_MAX_FRAMES = 99, SIG_DELAY_MAX_TAPS = 16' in header
    shared = (ROOT / 'signals_amd' / 'csrc' / 'sig_delay.h').read_text()
    assert '__host__ __device__' in shared and 'hip_runtime' not in shared    # one text for both sides, nothing of HIP in it
    assert '"sig_delay.h"' in (ROOT / 'signals_amd' / 'csrc' / 'delay.hip').read_text()


def test_delay_taps_argument_errors_do_not_reach_the_device(lib):
    p = 64                                                                    # (never dereferenced: every call fails its checks)
    m = (ctypes.c_double * 16)(*([1.0] * 16))
    g = (ctypes.c_double * 16)(*([1.0] * 16))
    args = dict(rate=48000, position=4096, N=256, K=2, c0=100, voices=8, x=p, xdt=0, xld=8, xs=1, time=p, ts=1, trs=8, tb=1,
                U=4, m=m, g=g, out=p, odt=0, old=8, stream=None)

    def call(**over):
        a = dict(args, **over)
        return lib.sig_delay_taps(*(a[k] for k in args))
    assert call(U=0) == INV and call(U=17) == INV and call(U=-1) == INV       # 1 .. 16 taps
    assert call(c0=101) == INV and call(c0=101, position=101) == INV          # more context than the window has
    assert call(c0=99) == INV and call(c0=0) == INV                           # inconsistent with the position: min(100, 4096) = 100
    assert call(position=37, c0=100) == INV and call(position=37, c0=36) == INV and call(position=0, c0=1) == INV
    assert call(c0=-1, position=0) == INV
    assert call(x=None) == INV and call(out=None) == INV and call(m=None) == INV and call(g=None) == INV
    assert call(N=0) == INV and call(N=-5) == INV                             # N >= 1
    assert call(K=-1) == INV and call(voices=-1) == INV and call(rate=0) == INV and call(position=-1) == INV
    assert call(old=4) == INV and call(xld=4) == INV and call(xs=2) == INV    # rows narrower than the voices, strides 0 / 1
    assert call(ts=2) == INV and call(trs=-1) == INV and call(tb=3) == INV    # time rows: strides 0 / 1, one row or one per block
    assert call(odt=2) == INV and call(xdt=2) == INV
    # accepted, nothing to launch: no blocks, no voices -- with every consistent context
    assert call(K=0) == 0 and call(voices=0, old=0) == 0
    assert call(K=0, position=37, c0=37) == 0 and call(K=0, position=0, c0=0) == 0 and call(K=0, position=100, c0=100) == 0
    assert call(K=0, time=None, tb=1) == 0 and call(tb=0) == INV              # time unplugged
    assert call(K=0, U=1) == 0 and call(K=0, U=16) == 0 and call(K=0, xs=0, xld=1) == 0 and call(K=0, xdt=1, odt=1) == 0


# ---------------------------------------------------------------------------------------------- planning
def test_purity_and_modulation_classification():
    from signals_amd.engine import _KNOWN_TYPES, _audio_ports, _control_ports, _ctl_const, _foreign, _is_pure, _modulated
    assert ext.Delay in _KNOWN_TYPES
    d = delay_node(mkosc(osc.Sawtooth, [[440.0]]), time=[[0.001]])
    assert not _foreign(d)
    assert _control_ports(d) == [d.time] and _audio_ports(d) == [d.input]
    assert all(_ctl_const(p) for p in _control_ports(d)) and not _modulated(d)
    assert not _is_pure(d, {})                                                # request-dependent like a filter, whatever drives it
    g = fx.Gain(); g.left = d; g.right = fix([[0.5]])
    assert not _is_pure(g, {})                                                # ... and so is everything downstream
    swept = delay_node(mkosc(osc.Sawtooth, [[440.0]]), time=mkosc(osc.Sine, [[0.5]]))
    assert _modulated(swept) and not _is_pure(swept, {})
    d.get_state().enabled = False
    assert _is_pure(d, {})                                                    # disabled: zeros((1, 1))


def test_the_delay_gets_a_filters_history():
    from signals_amd.engine import _Batch
    src = mkosc(osc.Sawtooth, row(100, 200))
    d = delay_node(src, time=[[0.001]])
    lp = fx.LowPass(); lp.input = d; lp.cutoff = fix(row(500, 5000))
    for pos, want in ((0, 0), (37, 37), (100, 100), (4096, 100)):
        batch = _Batch(types.SimpleNamespace(rate=RATE), pos, 256, 2, False)
        batch._require(lp, V, 0)
        assert batch._need[(lp, V)] == 0 and batch._need[(d, V)] == want and batch._need[(src, V)] == want, pos
    batch = _Batch(types.SimpleNamespace(rate=RATE), 4096, 256, 2, False)      # read by a pure node that needs no history: still 100 upstream
    batch._require(d, V, 0)
    assert batch._need[(d, V)] == 0 and batch._need[(src, V)] == 100


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


def flanger(voices=V):
    dry = mkosc(osc.Sawtooth, row(100, 200, voices))
    lfo = fx.Gain(); lfo.left = mkosc(osc.Sine, [[0.7]]); lfo.right = fix([[0.00075]])
    time = fx.Mix(); time.left = lfo; time.right = fix([[0.0015]]); time.mix = fix([[0.5]])        # 0 .. 1.5 ms
    wet = delay_node(dry, time=time)
    mix = fx.Mix(); mix.left = dry; mix.right = wet; mix.mix = fix([[0.5]])
    return mix, wet


FUSED = ('fused', 'latency', 'cascade', 'steady', 'walk', 'biquad_bus', 'biquad_coldstart_env', 'voice_program')


@pytest.mark.parametrize('shape', ['flanger', 'flanger_bus', 'lowpass_over', 'over_lowpass', 'twice', 'gain_bus'])
def test_no_fused_matcher_and_no_voice_program_takes_a_graph_with_the_node(stubbed, shape):
    """the fused matchers read fx.SingleCritFilter and osc.Osc, the voice program its KERNEL_NODES: a graph with a Delay renders one
    kernel per node whatever the renderer is allowed, the Delay through sig_delay_taps -- neither mistaken for a filter nor dropped"""
    from signals_amd.engine import BatchRenderer, _VoiceProgram

    def build():
        saw = mkosc(osc.Sawtooth, row(100, 200))
        if shape.startswith('flanger'):
            top = flanger()[0]
        elif shape == 'lowpass_over':
            top = fx.LowPass(); top.input = delay_node(saw, time=[[0.0005]]); top.cutoff = fix(row(500, 5000))
        elif shape == 'over_lowpass':
            lp = fx.LowPass(); lp.input = saw; lp.cutoff = fix(row(500, 5000))
            top = delay_node(lp, time=[[0.0005]])
        elif shape == 'twice':
            top = delay_node(delay_node(saw, time=[[0.0005]]), time=row(0, 0.002), taps=[[1, 1], [0.5, -0.5]])
        else:
            top = fx.Gain(); top.left = delay_node(saw, time=[[0.0005]]); top.right = fix(row(0.1, 1.0))
        if shape.endswith('bus'):
            b = ext.SumBus(); b.input = top
            return b, 1
        return top, V
    launched = 0
    for kw in ({}, {'fuse_program': 'always'}, {'fuse_program': 'always', 'mixed_programs': True}, {'fuse': False}):
        top, C = build()
        rec = _Recorder()
        r = BatchRenderer(top, C, RATE, timer=rec, **kw)
        r.render(0, 256, 3)
        r.render(768, 256, 2)                                                 # continuing: the tails
        r.render(8192, 256, 2)                                                # fresh: the own-history block
        inner = ('fused_osc_biquad[Sawtooth,lp]',) if shape == 'over_lowpass' else ()     # the LowPass(Sawtooth) BEHIND the Delay may fuse: the Delay reads its rows
        assert not any(word in n for n in rec.names for word in FUSED if n not in inner), (kw, rec.names)
        delays = [n for n in rec.names if n.startswith('delay_taps[')]
        per_render = 2 if shape == 'twice' else 1
        assert len(delays) >= 3 * per_render, rec.names
        if shape.startswith('flanger'):
            assert all(n == 'delay_taps[1,per-block]' for n in delays), rec.names
        if shape == 'twice':
            assert {'delay_taps[1]', 'delay_taps[2]'} == set(delays), rec.names
        launched += len(delays)
        assert [name for name, _ in stubbed.calls].count('sig_delay_taps') == launched
    top, _ = build()
    assert _VoiceProgram.compile(None, top.input.sig if shape.endswith('bus') else top, V) is None           # the voice program declines the graph
    assert ext.Delay not in _VoiceProgram.KERNEL_NODES and not issubclass(ext.Delay, _VoiceProgram.KERNEL_NODES)


def test_the_launch_carries_the_window_the_time_rows_and_the_taps(stubbed):
    from signals_amd.engine import BatchRenderer
    top, wet = flanger()
    wet.get_state().taps = np.array([[1.0, 0.5], [0.5, -0.25], [2.0, 0.125]])
    BatchRenderer(top, V, RATE).render(4096, 256, 3)
    calls = [a for name, a in stubbed.calls if name == 'sig_delay_taps']
    main = [a for a in calls if a[2:5] == (256, 3, 100)]                      # (the own-history block is not asked for: the top needs none)
    assert len(main) == 1 and len(calls) == 1
    (rate, position, N, K, c0, voices, _, xdt, xld, xs, time, ts, trs, tb, U, m, g, _, odt, old, _), = main
    assert (rate, position, voices, xdt, xs, odt) == (RATE, 4096, V, _native.F32, 1, _native.F32) and xld >= V and old >= V
    assert time is not None and (ts, tb) == (0, 3) and trs == 1                # per-block rows of a one-column LFO
    assert U == 3 and list(m) == [1.0, 0.5, 2.0] and list(g) == [0.5, -0.25, 0.125]


def test_short_blocks_over_an_impure_input_are_refused_like_a_filters(stubbed):
    from signals_amd.engine import BatchRenderer, NotBatchable
    lp = fx.LowPass(); lp.input = mkosc(osc.Sawtooth, row(100, 200)); lp.cutoff = fix(row(500, 5000))
    top = delay_node(lp, time=[[0.0005]])
    with pytest.raises(NotBatchable, match='block size <= 100 depend on the after-window cache'):
        BatchRenderer(top, V, RATE, fuse=False).render(0, 64, 3)
    BatchRenderer(top, V, RATE, fuse=False).render(0, 64, 1)                  # one block, not continuing: nothing cached is involved
    BatchRenderer(delay_node(mkosc(osc.Sawtooth, row(100, 200)), time=[[0.0005]]), V, RATE).render(0, 64, 3)      # a pure input: any N
    chained = delay_node(delay_node(mkosc(osc.Sawtooth, row(100, 200)), time=[[0.0005]]), time=[[0.0005]])
    with pytest.raises(NotBatchable, match='block size <= 100'):
        BatchRenderer(chained, V, RATE).render(0, 100, 2)                     # a Delay is an impure input itself


def test_narrow_ports_broadcast_at_width_one_and_raise_otherwise(stubbed):
    from signals_amd.engine import BatchRenderer
    wide = delay_node(mkosc(osc.Sawtooth, [[220.0]]), time=row(0, 0.001))     # input of width 1 broadcasts
    BatchRenderer(wide, V, RATE).render(0, 256, 2)
    a = [a for name, a in stubbed.calls if name == 'sig_delay_taps'][-1]
    assert a[5] == V and a[9] == 0 and a[11] == 1                             # voices, in_stride 0, time_stride 1
    for top in (delay_node(mkosc(osc.Sawtooth, row(100, 200, 3)), time=[[0.001]]),
                delay_node(mkosc(osc.Sawtooth, row(100, 200)), time=row(0, 0.001, 3))):
        with pytest.raises(IndexError, match='index 3 is out of bounds for axis 1 with size 3'):
            BatchRenderer(top, V, RATE).render(0, 256, 2)


def test_a_delay_in_a_control_path_is_refused_with_its_reason():
    from signals_amd.engine import NotBatchable, _Batch, _ControlProgram
    d = delay_node(mkosc(osc.Sine, [[3.0]]), time=[[0.001]])
    with pytest.raises(NotBatchable, match='delay line has no block-rate program'):
        _ControlProgram((d,), 4, channels=1)
    g = fx.Gain(); g.left = d; g.right = fix([[100.0]])
    with pytest.raises(NotBatchable, match='delay line has no block-rate program'):
        _ControlProgram((g,), 4, channels=1)
    batch = _Batch(types.SimpleNamespace(rate=RATE), 0, 256, 4, False)
    with pytest.raises(NotBatchable, match=r'Delay in a control path: a delay line has no block-rate schedule \(the eager node serves one-frame requests\)'):
        batch._control_node(d, 'cutoff')
