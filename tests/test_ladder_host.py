"""The 4-pole ladder filter without a GPU: the numpy restatement (tests/ladder_reference.py) pinned against things that are not the code
under test -- scipy's one-pole, the DC gain, the saturator's bound -- then the node API of ext.Ladder and its state validation, name
resolution and the .sigs loader, sig_ladder_coldstart's export, declaration and argument checks, and how the engine's planner
classifies and schedules the node: a filter's history, never pure, one ladder_coldstart launch per node on every renderer setting, no
fused matcher and no voice program, the refusal in a control path."""
import ctypes
import math
import pathlib
import types

import numpy as np
import pytest
import scipy.signal

from signals_amd import SignalFlags, _native
from signals_amd.chain import BadStateValue
from signals_amd.chain import ext, fixed, fx, noise, osc
from signals_amd.chain.ext import Ladder                                      # (the feature: without it nothing here runs)

import ladder_reference as LR

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


def ladder_node(input_, cutoff=None, resonance=None, drive=None, poles=None):
    n = Ladder()
    if poles is not None:
        n.get_state().poles = poles
    n.input = input_
    for name, value in (('cutoff', cutoff), ('resonance', resonance), ('drive', drive)):
        if value is not None:
            setattr(n, name, value if not isinstance(value, (np.ndarray, list, float)) else fix(value))
    return n


def run(x, cutoff, k=0.0, d=0.0, poles=4, taps=False):
    """the restatement over one column from zero state"""
    G, H, kk, dd, c, status, nan = LR.design([cutoff], [k], [d], RATE)
    assert status == 0 and not nan.any()
    got = LR.ladder_rows(np.asarray(x, dtype=np.float64).reshape(-1, 1), G, H, kk, dd, c, poles, taps=taps)
    return (got[0][:, 0], got[1][:, 0]) if taps else got[:, 0]


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize('cutoff', [20.0, 200.0, 1000.0, 3000.0, 0.49 * RATE])
def test_without_feedback_and_drive_it_is_four_bilinear_one_poles(cutoff):
    """k = 0, d = 0, poles = p: p passes of scipy's lfilter over the bilinear one-pole low-pass, from zero state, within 1e-12 relative"""
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, 356)
    g = math.tan(math.pi * (cutoff / (RATE / 2)) / 2.0)
    G = g / (1.0 + g)
    want = x
    for p in (1, 2, 3, 4):
        want = scipy.signal.lfilter([G, G], [1.0, (g - 1.0) / (g + 1.0)], want)
        got = run(x, cutoff, poles=p)
        assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), (cutoff, p)


@pytest.mark.parametrize('k', [0.0, 1.0, 3.5])
def test_dc_gain_is_one_over_one_plus_k(k):
    """a constant input over 20000 rows, the restatement run as a stream: every tap settles to 1 / (1 + k)"""
    for p in (1, 2, 3, 4):
        y = run(np.ones(20000), 1000.0, k=k, poles=p)
        assert abs(y[-1] - 1.0 / (1.0 + k)) < 1e-9, (k, p, y[-1])


def test_a_small_drive_is_the_linear_loop_and_a_large_one_bounds_it():
    rng = np.random.default_rng(4)
    x = rng.uniform(-1, 1, 356)
    for k in (0.0, 3.0):
        assert np.max(np.abs(run(x, 1000.0, k=k, d=1e-4) - run(x, 1000.0, k=k, d=0.0))) < 1e-7      # tanh(z) / d = u (1 - (d u)^2 / 3 ...)
    for d in (0.5, 2.0, 8.0, 100.0):
        for k in (0.0, 3.0, 4.0):
            _, u = run(3.0 * x, 3000.0, k=k, d=d, taps=True)
            assert np.max(np.abs(u)) <= 1.0 / d, (d, k)
    _, u = run(3.0 * x, 3000.0, k=0.0, d=100.0, taps=True)
    assert np.max(np.abs(u)) > 0.99 / 100.0                                   # (and reaches it: the bound is not vacuous)
    assert np.array_equal(run(x, 1000.0, k=3.0, d=-1.0), run(x, 1000.0, k=3.0, d=0.0))              # a negative drive is 0
    assert np.array_equal(run(x, 1000.0, k=7.0), run(x, 1000.0, k=4.0))                             # k clips to 4


def test_the_edge_of_self_oscillation_stays_bounded_over_a_window():
    """k = 4 on white input over 356 rows (100 context rows and the largest block of the GPU tests)"""
    x = np.random.default_rng(5).uniform(-1, 1, 356)
    for cutoff in (20.0, 200.0, 1000.0, 3000.0, 0.49 * RATE):
        for p in (1, 2, 3, 4):
            y = run(x, cutoff, k=4.0, poles=p)
            assert np.isfinite(y).all() and np.max(np.abs(y)) < 8.0, (cutoff, p, np.max(np.abs(y)))


def test_design_refusals_and_status_bits():
    nan, inf = math.nan, math.inf
    cut = [1000.0, 0.0, 24000.0, nan, -5.0, 1000.0, 1000.0, 1000.0, 1000.0, 1000.0, 1000.0]
    k = [0.0, 0.0, 0.0, 0.0, 0.0, nan, inf, -inf, -3.0, 2.0, 2.0]
    d = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, nan, inf]
    G, H, kk, dd, c, status, bad = LR.design(cut, k, d, RATE)
    assert bad.tolist() == [False, True, True, True, True, True, True, True, False, True, True]
    assert status == LR.STATUS_BAD_CUTOFF | LR.STATUS_BAD_RESONANCE and np.array_equal(np.isnan(G), bad)
    assert LR.design(cut[:5], None, None, RATE)[5] == LR.STATUS_BAD_CUTOFF
    assert LR.design([1000.0] * 3, k[5:8], None, RATE)[5] == LR.STATUS_BAD_RESONANCE
    assert LR.design([1000.0] * 2, None, d[9:], RATE)[5] == 0                  # a bad drive: NaN rows, no bit
    assert kk[8] == 0.0 and LR.design([1000.0], [0.0], [-inf], RATE)[3][0] == 0.0 and not LR.design([1000.0], [0.0], [-inf], RATE)[6][0]
    x = np.ones((5, len(cut)))
    out = LR.ladder_rows(x, G, H, kk, dd, c, 4)
    assert np.array_equal(np.isnan(out), np.broadcast_to(bad, out.shape))


def test_blocks_are_cold_started_over_their_own_window():
    rng = np.random.default_rng(6)
    x = rng.uniform(-1, 1, (37 + 3 * 16, 3))
    cut, k, d = rng.uniform(200, 8000, (3, 3)), rng.uniform(0, 4, (1, 3)), np.array([[0.0, 1.0, 3.0]])
    got, status = LR.ladder_blocks(x, 37, 16, 3, cut, k, d, 3, RATE)
    assert status == 0 and got.shape == (48, 3)
    for b in range(3):
        c0 = min(100, 37 + 16 * b)
        G, H, kk, dd, c, _, _ = LR.design(cut[b], k[0], d[0], RATE)
        want = LR.ladder_rows(x[37 + 16 * b - c0:37 + 16 * (b + 1)], G, H, kk, dd, c, 3)[c0:]
        assert np.array_equal(got[16 * b:16 * (b + 1)], want)


def test_the_docstrings_figures_are_the_restatements():
    doc = ' '.join(Ladder.__doc__.split())
    figures = [round(100 * LR.impulse_tail_share(hz, 3.5, RATE, rows=60000)) for hz in (1000, 3000)]
    assert figures == [66, 29] and '66 % at 1 kHz' in doc and '29 % at 3 kHz' in doc and '93 % at 200 Hz' in doc


# ---------------------------------------------------------------------------------------------- the node
def test_node_api_and_class_relations():
    assert Ladder.port_names() == ['cutoff', 'drive', 'input', 'resonance']
    assert Ladder.flags() & SignalFlags.EFFECT and not Ladder.flags() & SignalFlags.GENERATOR
    assert issubclass(Ladder, fx.CritFilter)
    assert not issubclass(Ladder, ext.ResonantFilter) and not issubclass(Ladder, fx.SingleCritFilter) and not issubclass(Ladder, fx.DoubleCritFilter)
    n = Ladder()
    assert 'poles' in n.state_attrs() and n.get_state().poles == 4 and n.context_frames() == 100
    assert str(n.type()) == 'ladder' and not n.type().is_band and n.type() not in list(fx.CritFilter.Type)
    assert _native.FILT_TYPES['ladder'] == 12 == max(_native.FILT_TYPES.values()) and len(set(_native.FILT_TYPES.values())) == len(_native.FILT_TYPES)
    n = ladder_node(mkosc(osc.Sawtooth, np.full((1, 6), 220.0)), cutoff=np.full((1, 6), 1000.0), resonance=np.full((1, 6), 3.0))
    assert n.channels == 6                                                    # ImplicitChannels: the one width that is not 1


def test_docstring_holds_the_definition_the_edges_and_what_is_out_of_scope():
    doc = ' '.join(Ladder.__doc__.split())
    for words in ('g = tan(pi * wn / 2)', 'G = g / (1 + g)', 'k = clip(resonance, 0, 4)', 'd = max(drive, 0)', 'c = 1 / (1 + k * ((G*G) * (G*G)))',
                  'S = H * (((s1*G + s2)*G + s3)*G + s4)', 'u = (x - k*S) * c', 'u = tanh(d*u) / d', 'v = (u - s_j)*G', 'out = y_poles',
                  '1 / (1 + k)', 'edge of self-oscillation', 'NaN or +-inf', 'NaN or +inf', 'no status bit', 'the ring IS the sound',
                  'Out of scope', 'the voice program, the specialised build and the fused kernels', 'block-rate control path',
                  'a frame-rate cutoff, k or drive', 'pass-band gain compensation', 'high-pass and band-pass pole mixes', 'oversampling',
                  'carried state'):
        assert words in doc, words


@pytest.mark.parametrize('bad', [0, 5, -1, 2.0, '4', None, True, np.array([4]), [4]],
                         ids=['0', '5', '-1', 'a float', 'a string', 'None', 'a bool', 'an array', 'a list'])
def test_poles_validation_refuses(bad):
    n = Ladder()
    with pytest.raises(BadStateValue):
        n.get_state().poles = bad
    assert n.get_state().poles == 4


def test_poles_validation_accepts():
    n = Ladder()
    for good in (1, 2, 3, 4, np.int64(3), np.int32(1)):
        n.get_state().poles = good
        assert n.get_state().poles == good


def test_class_resolves_by_qualified_name_and_loads_from_a_patch():
    from signals_amd.chain import discovery, sigs
    from signals_amd.chain.driver import load_signal
    assert load_signal('signals_amd.chain.ext.Ladder') is Ladder
    assert load_signal('signals.chain.ext.Ladder') is Ladder
    assert discovery.load_signal('signals.chain.ext.Ladder') is Ladder
    assert Ladder().cls_name().endswith('chain.ext.Ladder')
    p = sigs.loads('+ 1a signals.chain.fixed.Fixed value=[[220.0]]\n+ 1b signals.chain.fixed.Fixed value=[[800.0]]\n'
                   '+ 1c signals.chain.fixed.Fixed value=[[3.0]]\n+ 1d signals.chain.osc.Sawtooth\n'
                   '+ 2a signals.chain.ext.Ladder poles=2\n> 1a 1d.hertz\n> 1d 2a.input\n> 1b 2a.cutoff\n> 1c 2a.resonance\n> 1c 2a.drive')
    node = p['2a']
    assert isinstance(node, Ladder) and node.input.sig is p['1d'] and node.cutoff.sig is p['1b']
    assert node.resonance.sig is p['1c'] and node.drive.sig is p['1c'] and node.get_state().poles == 2
    assert sigs.loads('+ 1a signals.chain.ext.Ladder')['1a'].get_state().poles == 4
    with pytest.raises(BadStateValue):
        sigs.loads('+ 1a signals.chain.ext.Ladder poles=5')


# ---------------------------------------------------------------------------------------------- C ABI
def test_entry_point_is_exported_and_declared(lib):
    assert 'sig_ladder_coldstart' in _native.EXPORTS
    raw = ctypes.CDLL(str(_native.LIB_PATH))
    assert raw.sig_ladder_coldstart is not None
    assert lib.sig_abi_version() == 7 == _native.ABI_VERSION                  # additive
    header = (ROOT / 'include' / 'signals_amd.h').read_text()
    assert 'int sig_ladder_coldstart(' in header and '#define SIG_ABI_VERSION 7' in header and 'SIG_FILT_LADDER = 12' in header
    assert '`sig_ladder_coldstart`' in (ROOT / 'INTEGRATION.md').read_text()
    assert '"sig_coldstart.h"' in (ROOT / 'signals_amd' / 'csrc' / 'ladder.hip').read_text()


def test_ladder_coldstart_argument_errors_do_not_reach_the_device(lib):
    p = 64                                                                    # (never dereferenced: every call fails its checks or has nothing to launch)
    args = dict(rate=48000, position=4096, N=256, K=2, ctx=100, voices=8, cut=p, cs=1, cb=1, res=p, rs=1, rb=1, drv=p, ds=1, db=1, poles=4,
                x=p, xld=8, hist=100, out=p, old=8, dtype=0, status=None, stream=None)

    def call(**over):
        a = dict(args, **over)
        return lib.sig_ladder_coldstart(*(a[k] for k in args))
    assert call(poles=0) == INV and call(poles=5) == INV and call(poles=-1) == INV
    assert call(x=None) == INV and call(out=None) == INV and call(cut=None) == INV
    assert call(rate=0) == INV and call(position=-1) == INV and call(N=-1) == INV and call(K=-1) == INV and call(voices=-1) == INV and call(ctx=-1) == INV
    assert call(xld=4) == INV and call(old=4) == INV and call(hist=99) == INV and call(position=37, hist=36) == INV
    assert call(cs=2) == INV and call(rs=2) == INV and call(ds=-1) == INV     # strides 0 / 1
    assert call(cb=3) == INV and call(rb=3) == INV and call(db=0) == INV      # one row or one per block
    assert call(res=None, rs=2) == INV and call(drv=None, db=3) == INV        # an unplugged row's stride and count are still checked
    assert call(dtype=2) == INV and call(dtype=-1) == INV
    # accepted, nothing to launch
    assert call(K=0) == 0 and call(N=0) == 0 and call(voices=0, xld=0, old=0) == 0
    assert call(K=0, res=None) == 0 and call(K=0, drv=None) == 0 and call(K=0, res=None, drv=None, dtype=1) == 0
    assert call(K=0, position=37, hist=37) == 0 and call(K=0, position=0, hist=0) == 0
    assert call(K=0, cb=0) == 0 and call(K=0, dtype=2) == INV and all(call(K=0, poles=n) == 0 for n in (1, 2, 3, 4))


# ---------------------------------------------------------------------------------------------- planning
def test_purity_and_modulation_classification():
    from signals_amd.engine import _KNOWN_TYPES, _audio_ports, _control_ports, _ctl_const, _foreign, _is_pure, _modulated
    n = ladder_node(mkosc(osc.Sawtooth, row(100, 200)), cutoff=row(500, 5000), resonance=row(0, 4), drive=row(0, 2))
    assert not _foreign(n) and isinstance(n, _KNOWN_TYPES)
    assert _control_ports(n) == [n.cutoff, n.resonance, n.drive] and _audio_ports(n) == [n.input]
    assert all(_ctl_const(p) for p in _control_ports(n)) and not _modulated(n)
    assert not _is_pure(n, {})                                                # request-dependent like every filter
    for name in ('cutoff', 'resonance', 'drive'):
        swept = ladder_node(mkosc(osc.Sawtooth, row(100, 200)), cutoff=row(500, 5000))
        setattr(swept, name, mkosc(osc.Sine, row(0.5, 2.0)))
        assert _modulated(swept), name


def test_the_ladder_gets_a_filters_history():
    from signals_amd.engine import _Batch
    src = mkosc(osc.Sawtooth, row(100, 200))
    n = ladder_node(src, cutoff=row(500, 5000))
    g = fx.Gain(); g.left = n; g.right = fix(row(0.1, 1.0))
    for pos, want in ((0, 0), (37, 37), (100, 100), (4096, 100)):
        batch = _Batch(types.SimpleNamespace(rate=RATE), pos, 256, 2, False)
        batch._require(g, V, 0)
        assert batch._need[(n, V)] == 0 and batch._need[(src, V)] == want, pos


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
SETTINGS = ({}, {'fuse': False}, {'specialise': True}, {'mixed_programs': True}, {'fuse_program': 'always'},
            {'fuse_program': 'always', 'mixed_programs': True})


def lfo_cutoff():
    """cutoffs moved by a block-rate LFO: per-block rows"""
    lfo = fx.Gain(); lfo.left = mkosc(osc.Sine, row(0.5, 2.0)); lfo.right = fix([[200.0]])
    m = fx.Mix(); m.left = lfo; m.right = fix(row(1000, 5000)); m.mix = fix([[0.5]])
    return m


def build(shape):
    """(top, rendered width, ladder nodes per render)"""
    saw = mkosc(osc.Sawtooth, row(100, 200))
    if shape == 'plain':
        return ladder_node(saw, cutoff=row(500, 5000)), V, 1
    if shape == 'driven':
        return ladder_node(saw, cutoff=row(500, 5000), resonance=row(0, 4), drive=row(0.5, 2), poles=2), V, 1
    if shape == 'swept_bus':
        b = ext.SumBus(); b.input = ladder_node(saw, cutoff=lfo_cutoff(), resonance=row(0, 4))
        return b, 1, 1
    if shape == 'twice':
        return ladder_node(ladder_node(saw, cutoff=row(500, 5000), resonance=row(0, 4)), cutoff=row(800, 900), drive=row(1, 2), poles=3), V, 2
    if shape == 'gain_bus':
        g = fx.Gain(); g.left = ladder_node(saw, cutoff=row(500, 5000), resonance=row(0, 4)); g.right = fix(row(0.1, 1.0))
        b = ext.SumBus(); b.input = g
        return b, 1, 1
    if shape == 'over_lowpass':
        lp = fx.LowPass(); lp.input = saw; lp.cutoff = fix(row(500, 5000))
        return ladder_node(lp, cutoff=row(500, 5000), resonance=row(0, 4)), V, 1
    if shape == 'lowpass_over':
        lp = fx.LowPass(); lp.input = ladder_node(saw, cutoff=row(500, 5000), resonance=row(0, 4)); lp.cutoff = fix(row(500, 5000))
        return lp, V, 1
    raise KeyError(shape)


LABELS = {'plain': {'ladder_coldstart[4]'}, 'driven': {'ladder_coldstart[2,drive]'}, 'swept_bus': {'ladder_coldstart[4,blocks]'},
          'twice': {'ladder_coldstart[4]', 'ladder_coldstart[3,drive]'}, 'gain_bus': {'ladder_coldstart[4]'},
          'over_lowpass': {'ladder_coldstart[4]'}, 'lowpass_over': {'ladder_coldstart[4]'}}


@pytest.mark.parametrize('shape', sorted(LABELS))
def test_every_renderer_setting_renders_one_ladder_launch_per_node(stubbed, shape):
    """the fused matchers read fx.SingleCritFilter and osc.Osc, the voice program its KERNEL_NODES: a graph with a Ladder renders the
    Ladder through sig_ladder_coldstart whatever the renderer is allowed -- one launch per node and batch, neither mistaken for a biquad
    nor dropped -- and the nodes around it keep their routes: the oscillator in front its own kernel, a bus behind sum_bus"""
    from signals_amd.engine import BatchRenderer, _VoiceProgram
    launched = 0
    for kw in SETTINGS:
        top, C, per_render = build(shape)
        rec = _Recorder()
        r = BatchRenderer(top, C, RATE, timer=rec, **kw)
        r.render(0, 256, 3)
        r.render(768, 256, 2)                                                 # continuing: the tails
        ladders = [n for n in rec.names if n.startswith('ladder_coldstart[')]
        assert len(ladders) == 2 * per_render and set(ladders) == LABELS[shape], (kw, rec.names)
        inner = ('fused_osc_biquad[Sawtooth,lp]',) if shape == 'over_lowpass' else ()     # the LowPass(Sawtooth) IN FRONT may fuse: the Ladder reads its rows
        assert not any(word in n for n in rec.names for word in FUSED if n not in inner), (kw, rec.names)
        assert not any(n.startswith(('biquad_coldstart_q', 'biquad_coldstart_eq', 'band_coldstart')) for n in rec.names), (kw, rec.names)
        if shape != 'over_lowpass':
            assert sum(n.startswith('osc_bank[Sawtooth') for n in rec.names) == 2, (kw, rec.names)
        if shape.endswith('bus'):
            assert rec.names.count('sum_bus') == 2, (kw, rec.names)
        launched += len(ladders)
        assert [name for name, _ in stubbed.calls].count('sig_ladder_coldstart') == launched
    top, _, _ = build(shape)
    assert _VoiceProgram.compile(None, top.input.sig if shape.endswith('bus') else top, V) is None             # the voice program declines the graph
    assert _VoiceProgram.compile(None, top.input.sig if shape.endswith('bus') else top, V, mixed=True) is None
    assert Ladder not in _VoiceProgram.KERNEL_NODES and not issubclass(Ladder, _VoiceProgram.KERNEL_NODES)


def test_the_launch_carries_the_window_the_three_control_rows_and_the_poles(stubbed):
    from signals_amd.engine import BatchRenderer
    top = ladder_node(mkosc(osc.Sawtooth, row(100, 200)), cutoff=lfo_cutoff(), resonance=row(0, 4), poles=3)
    BatchRenderer(top, V, RATE).render(4096, 256, 3)
    (a,) = [a for name, a in stubbed.calls if name == 'sig_ladder_coldstart']
    rate, position, N, K, ctx, voices, cut, cs, cb, res, rs, rb, drv, ds, db, poles, _, xld, hist, _, old, dtype, status, _ = a
    assert (rate, position, N, K, ctx, voices) == (RATE, 4096, 256, 3, 100, V) and xld >= V and old >= V and hist == 100
    assert cut is not None and (cs, cb) == (1, 3)                             # per-block cutoff rows
    assert res is not None and (rs, rb) == (1, 1) and (drv, ds, db) == (None, 0, 1)       # drive unplugged: a null row
    assert poles == 3 and dtype == _native.F32 and status is not None
    stubbed.calls.clear()
    top = ladder_node(mkosc(osc.Sawtooth, row(100, 200)), cutoff=row(500, 5000), drive=row(0, 0))
    BatchRenderer(top, V, RATE).render(0, 256, 2)
    (a,) = [a for name, a in stubbed.calls if name == 'sig_ladder_coldstart']
    assert a[9] is None and a[12] is not None and a[18] == 0                  # a plugged row of zeros is a row; position 0: no history
    disabled = fix(row(1, 2)); disabled.get_state().enabled = False
    stubbed.calls.clear()
    BatchRenderer(ladder_node(mkosc(osc.Sawtooth, row(100, 200)), cutoff=row(500, 5000), drive=disabled), V, RATE).render(0, 256, 2)
    (a,) = [a for name, a in stubbed.calls if name == 'sig_ladder_coldstart']
    assert a[12] is None                                                      # a disabled source: unplugged


def test_short_blocks_over_an_impure_input_are_refused_like_a_filters(stubbed):
    from signals_amd.engine import BatchRenderer, NotBatchable
    white = noise.White(); white.get_state().channels = V
    lp = fx.LowPass(); lp.input = mkosc(osc.Sawtooth, row(100, 200)); lp.cutoff = fix(row(500, 5000))
    top = ladder_node(lp, cutoff=row(500, 5000))
    with pytest.raises(NotBatchable, match='block size <= 100 depend on the after-window cache'):
        BatchRenderer(top, V, RATE, fuse=False).render(0, 64, 3)
    BatchRenderer(top, V, RATE, fuse=False).render(0, 64, 1)                  # one block, not continuing: nothing cached is involved
    BatchRenderer(ladder_node(mkosc(osc.Sawtooth, row(100, 200)), cutoff=row(500, 5000)), V, RATE).render(0, 64, 3)      # a pure input: any N
    chained = ladder_node(ladder_node(mkosc(osc.Sawtooth, row(100, 200)), cutoff=row(500, 5000)), cutoff=row(500, 5000))
    with pytest.raises(NotBatchable, match='block size <= 100'):
        BatchRenderer(chained, V, RATE).render(0, 100, 2)                     # a Ladder is an impure input itself


def test_narrow_ports(stubbed):
    """an input of width 1 broadcasts where it is pure; a narrow control raises the IndexError of a narrow cutoff"""
    from signals_amd.engine import BatchRenderer, NotBatchable
    wide = ladder_node(mkosc(osc.Sawtooth, [[220.0]]), cutoff=row(500, 5000), resonance=row(0, 4))
    BatchRenderer(wide, V, RATE).render(0, 256, 2)
    a = [a for name, a in stubbed.calls if name == 'sig_ladder_coldstart'][-1]
    assert a[5] == V and a[17] >= V                                           # voices; the input was widened to them
    swept = mkosc(osc.Sawtooth, [[220.0]]); swept.phase = mkosc(osc.Sine, [[0.5]])
    with pytest.raises(NotBatchable, match='request-dependent input of one column'):
        BatchRenderer(ladder_node(swept, cutoff=row(500, 5000)), V, RATE).render(0, 256, 2)
    for top in (ladder_node(mkosc(osc.Sawtooth, row(100, 200, 3)), cutoff=row(500, 5000)),
                ladder_node(mkosc(osc.Sawtooth, row(100, 200)), cutoff=row(500, 5000, 3)),
                ladder_node(mkosc(osc.Sawtooth, row(100, 200)), cutoff=row(500, 5000), resonance=row(0, 4, 3)),
                ladder_node(mkosc(osc.Sawtooth, row(100, 200)), cutoff=row(500, 5000), drive=[[1.0]])):
        with pytest.raises(IndexError, match='is out of bounds for axis 1 with size'):
            BatchRenderer(top, V, RATE).render(0, 256, 2)


def test_a_ladder_in_a_control_path_is_refused_with_its_reason():
    from signals_amd.engine import NotBatchable, _Batch, _ControlProgram
    n = ladder_node(mkosc(osc.Sine, [[3.0]]), cutoff=[[100.0]])
    with pytest.raises(NotBatchable, match='ladder filter has no block-rate program'):
        _ControlProgram((n,), 4, channels=1)
    g = fx.Gain(); g.left = n; g.right = fix([[100.0]])
    with pytest.raises(NotBatchable, match=r'Ladder in a control path: a ladder filter has no block-rate program \(the eager node serves one-frame requests\)'):
        _ControlProgram((g,), 4, channels=1)
    lp = fx.LowPass(); lp.input = n; lp.cutoff = fix([[10.0]])
    with pytest.raises(NotBatchable, match='ladder filter has no block-rate program'):
        _ControlProgram((lp,), 4, channels=1)                                 # inside a control filter's input too
    batch = _Batch(types.SimpleNamespace(rate=RATE), 0, 256, 4, False)
    with pytest.raises(NotBatchable, match=r'Ladder in a control path: a ladder filter has no block-rate schedule \(the eager node serves one-frame requests\)'):
        batch._control_node(n, 'cutoff')
