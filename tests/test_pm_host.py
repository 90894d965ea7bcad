"""Phase-modulation oscillators without a GPU: the node API of ext.PMSine / PMSquare / PMSawtooth / PMTriangle, the OscPM
instruction's encoding and argument checks, sig_osc_bank_pm's export and argument checks, how the engine's planner classifies the
new nodes, the programs it compiles for them, and the specialised build of a program with the new instruction."""
import ctypes
import pathlib
import types

import numpy as np
import pytest
import torch

from signals_amd import SignalFlags, _native, specialise
from signals_amd.chain import BadShape, BlockCachingEmitter, BlockLoc, ExplicitChannelsEmitter, Receiver, Request, Shape, port
from signals_amd.chain import ext, fixed, fx, osc

ROOT = pathlib.Path(__file__).resolve().parent.parent
INV = 1     # hipErrorInvalidValue
PM_CLASSES = {'Sine': ext.PMSine, 'Square': ext.PMSquare, 'Sawtooth': ext.PMSawtooth, 'Triangle': ext.PMTriangle}


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


def sine(hz):
    o = osc.Sine(); o.hertz = fix(hz)
    return o


# ---------------------------------------------------------------------------------------------- the node
def test_node_api():
    for kind, cls in PM_CLASSES.items():
        assert cls.kind() == kind and cls.port_names() == ['hertz', 'index', 'mod', 'phase']
        assert cls.flags() & SignalFlags.GENERATOR
        assert issubclass(cls, ext.PMOsc) and issubclass(cls, BlockCachingEmitter) and not issubclass(cls, osc.Osc)
    n = ext.PMSine(); n.hertz = fix(np.full((1, 6), 220.0)); n.index = fix([[1.5]]); n.mod = sine([[110.0]])
    assert n.channels == 6                                                    # ImplicitChannels: the one width that is not 1
    n.mod = sine(np.full((1, 4), 110.0))
    with pytest.raises(ValueError):
        n.channels                                                            # 6 and 4: no single width


def test_classes_resolve_by_qualified_name():
    from signals_amd.chain import discovery, sigs
    from signals_amd.chain.driver import load_signal
    for kind, cls in PM_CLASSES.items():
        assert load_signal(f'signals_amd.chain.ext.PM{kind}') is cls
        assert load_signal(f'signals.chain.ext.PM{kind}') is cls
        assert discovery.load_signal(f'signals.chain.ext.PM{kind}') is cls
    with pytest.raises(TypeError):
        load_signal('signals_amd.chain.ext.PMOsc')                           # abstract
    p = sigs.loads('+ 1a signals.chain.fixed.Fixed value=[[220.0]]\n+ 1b signals.chain.osc.Sine\n> 1a 1b.hertz\n'
                   '+ 2a signals_amd.chain.ext.PMSine\n> 1a 2a.hertz\n> 1b 2a.mod')
    assert isinstance(p['2a'], ext.PMSine) and p['2a'].mod.sig is p['1b'] and p['2a'].hertz.sig is p['1a']


class Wide(BlockCachingEmitter, ExplicitChannelsEmitter):
    @classmethod
    def flags(cls):
        return SignalFlags.GENERATOR

    def _eval(self, request: Request) -> torch.Tensor:
        return torch.zeros((request.loc.shape.frames, 3), dtype=torch.float32)


class Probe(Receiver):
    input = port('input')
    HOST_ARRAYS = False

    @classmethod
    def flags(cls):
        return SignalFlags(0)


def test_bad_shape_at_the_modulator_port():
    w = Wide(); w.get_state().channels = 3
    n = ext.PMSquare(); n.mod = w
    p = Probe(); p.input = n
    with pytest.raises(BadShape):
        p.input.request(BlockLoc(position=0, rate=48000, shape=Shape(16, 2)))  # a 3-wide reply to a 2-wide request: raised before any kernel


def test_self_feedback_is_a_cycle():
    n = ext.PMSine(); n.mod = n
    with pytest.raises(AssertionError, match='Cycle'):
        n.upstream()


# ---------------------------------------------------------------------------------------------- C ABI
def test_instruction_encoding_and_header():
    assert _native.VP_OPS['OscPM'] == 12
    assert _native.voice_program_words([('Osc', 0, 0, 0, 0), ('OscPM', 0, 1, 0, 0)]) == [0x0, 0x10c]
    assert _native.voice_program_words([('OscPM', 2, 1, 3, 0)]) == [0x314c]
    header = (ROOT / 'include' / 'signals_amd.h').read_text()
    assert 'SIG_VP_OSCPM = 12' in header and 'int sig_osc_bank_pm(' in header and '#define SIG_ABI_VERSION 7' in header
    assert 'OscPM' not in _native.VP_EXT_OPS                                  # neither the extended handlers nor the band variant


def test_entry_point_is_exported(lib):
    assert 'sig_osc_bank_pm' in _native.EXPORTS
    assert ctypes.CDLL(str(_native.LIB_PATH)).sig_osc_bank_pm is not None
    assert lib.sig_abi_version() == 7


def test_osc_bank_pm_argument_errors_do_not_reach_the_device(lib):
    p = 64                                                                    # (never dereferenced: every call fails its checks)
    args = dict(kind=0, position=0, step=1, rate=48000, rows=256, voices=8, rpp=0, hertz=p, hs=1, hrs=0, phase=None, ps=0, prs=0,
                index=p, istr=1, irs=0, mod=p, mdt=0, mld=8, mcs=1, out=p, odt=0, old=8, stream=None)

    def call(**over):
        a = dict(args, **over)
        return lib.sig_osc_bank_pm(*(a[k] for k in args))
    assert call(hertz=None) == INV and call(out=None) == INV
    assert call(istr=2) == INV and call(irs=-1) == INV                        # index rows: strides 0 / 1, row stride >= 0
    assert call(mdt=2) == INV and call(mcs=2) == INV                          # the modulator: float32 | float64, column stride 0 / 1
    assert call(mld=4) == INV                                                 # rows narrower than the voices
    assert call(old=4) == INV and call(rate=0) == INV and call(position=-1) == INV and call(step=0) == INV
    assert call(rows=0) == 0 and call(voices=0, old=0) == 0                   # accepted, nothing to launch


def _program(code, n_oscs=2, n_params=1, types=()):
    P = _native.VoiceProgramT()
    P.n_ins = len(code)
    for k, (op, kind, a, b, c) in enumerate(code):
        P.ins[k] = _native.VpIns(_native.VP_OPS[op], kind, a, b, c)
    row = ctypes.c_double(440.0)
    ptr = ctypes.cast(ctypes.pointer(row), ctypes.c_void_p).value
    P.n_oscs = n_oscs
    for k in range(n_oscs):
        P.hertz[k] = _native.VpRows(ptr, 0, 1)
        P.phase[k] = _native.VpRows(None, 0, 1)
    P.n_params = n_params
    for k in range(n_params):
        P.params[k] = _native.VpRows(ptr, 0, 1)
    P.n_filters = len(types)
    for k, t in enumerate(types):
        P.cutoff[k] = _native.VpRows(ptr, 0, 1)
        P.filter_type[k] = _native.FILT_TYPES[t]
        P.filter_level[k] = 1
    P.depth = 1 if types else 0
    return P, row


def test_voice_program_refuses_oscpm_slots_out_of_range(lib):
    buf = (ctypes.c_float * 64)()

    def run(code, **kw):
        P, keep = _program(code, **kw)
        return lib.sig_voice_program(ctypes.byref(P), 48000, 0, 256, 1, 100, 8, 2, 0, None, 0, None, 0, 0, None,
                                     ctypes.addressof(buf), 8, None, None)
    mod = ('Osc', 0, 0, 0, 0)
    assert run([mod, ('OscPM', 0, 2, 0, 0)]) == INV                           # oscillator slot 2 of 2
    assert run([mod, ('OscPM', 0, 1, 1, 0)]) == INV                           # parameter slot 1 of 1
    assert run([mod, ('OscPM', 0, 1, 0, 0)], n_params=0) == INV               # no parameter at all
    assert run([mod, ('OscPM', 4, 1, 0, 0)]) == INV                           # not a waveform
    assert run([mod, ('OscPM', 0, 1, 0, 0), ('Band', 0, 0, 0, 0)], types=['bp', 'bp']) == INV     # no variant with both
    P, keep = _program([mod, ('OscPM', 0, 1, 0, 0)])
    P.ins[1].op = 13                                                          # past the last instruction
    assert lib.sig_voice_program(ctypes.byref(P), 48000, 0, 256, 1, 100, 8, 2, 0, None, 0, None, 0, 0, None,
                                 ctypes.addressof(buf), 8, None, None) == INV


# ---------------------------------------------------------------------------------------------- planning
def test_purity_and_modulation_classification():
    from signals_amd.engine import _KNOWN_TYPES, _audio_ports, _control_ports, _ctl_const, _foreign, _is_pure, _modulated
    for cls in PM_CLASSES.values():
        assert cls in _KNOWN_TYPES or issubclass(cls, _KNOWN_TYPES)
    c = ext.PMSine(); c.hertz = fix([[440.0]]); c.index = fix([[2.0]]); c.mod = sine([[220.0]])
    assert not _foreign(c)
    assert _control_ports(c) == [c.hertz, c.phase, c.index] and _audio_ports(c) == [c.mod]
    assert all(_ctl_const(p) for p in _control_ports(c)) and not _modulated(c) and _is_pure(c, {})
    lfo = sine([[2.0]])
    swept = ext.PMSawtooth(); swept.hertz = fix([[440.0]]); swept.index = lfo; swept.mod = sine([[220.0]])
    assert _modulated(swept) and not _is_pure(swept, {})                      # index re-read every block: tails
    lp = fx.LowPass(); lp.input = sine([[220.0]]); lp.cutoff = fix([[900.0]])
    filtered = ext.PMTriangle(); filtered.hertz = fix([[440.0]]); filtered.index = fix([[1.0]]); filtered.mod = lp
    assert not _modulated(filtered) and not _is_pure(filtered, {})            # pure only with a pure modulator
    g = fx.Gain(); g.left = c; g.right = fix([[0.5]])
    assert _is_pure(g, {})
    bare = ext.PMSquare(); bare.hertz = fix([[440.0]])
    assert _is_pure(bare, {}) and not _modulated(bare)                        # unplugged mod / index: the plain oscillator
    assert not isinstance(c, osc.Osc)                                         # the fused kernels' matchers never pick a PM carrier


def test_voice_program_words():
    """(_VoiceProgram compiles from the graph alone -- Fixed rows resident on the CPU device here -- so the words are asserted
    on the host)"""
    from signals_amd.engine import _VoiceProgram
    V = 8
    row = lambda lo, hi: np.linspace(lo, hi, V).reshape(1, V)
    m = sine(row(110, 220))
    c = ext.PMSine(); c.hertz = fix(row(220, 440)); c.index = fix(row(0.5, 4.0)); c.mod = m
    g = fx.Gain(); g.left = c; g.right = fix(row(0.1, 0.9))
    bus = ext.SumBus(); bus.input = g
    prog = _VoiceProgram(None, bus.input.sig, V)                              # the per-voice graph under SumBus(Gain(PMSine(mod=Sine)))
    assert prog.code == [('Osc', 0, 0, 0, 0), ('OscPM', 0, 1, 0, 0), ('Gain', 0, 1, 0, 0)]
    assert _native.voice_program_words(prog.code) == [0x0, 0x10c, 0x102]
    assert (len(prog.oscs), len(prog.params), len(prog.filters), prog.n_temps, prog.depth) == (2, 2, 0, 0, 0)
    folded = _VoiceProgram(None, c, V)                                        # ... with the constant Gain folded into the bus weights
    assert _native.voice_program_words(folded.code) == [0x0, 0x10c] and len(folded.params) == 1

    env = ext.ADSR()
    for name in _native.ADSR_PARAMS:
        setattr(env, name, fix(row(0.01, 0.2)))
    rm = fx.RingMod(); rm.left = env; rm.right = sine(row(110, 220))
    saw = ext.PMSawtooth(); saw.hertz = fix(row(220, 440)); saw.index = fix(row(0.5, 4.0)); saw.mod = rm
    lp = fx.LowPass(); lp.input = saw; lp.cutoff = fix(row(500, 5000))
    prog = _VoiceProgram(None, lp, V)
    assert prog.code == [('Adsr', 0, 0, 0, 0), ('Save', 0, 0, 0, 0), ('Osc', 0, 0, 0, 0), ('Mul', 0, 0, 0, 0),
                         ('OscPM', 2, 1, 0, 0), ('Filter', 0, 0, 0, 0)]
    assert _native.voice_program_words(prog.code) == [0x9, 0x5, 0x0, 0x3, 0x14c, 0x1]
    assert (len(prog.oscs), len(prog.params), len(prog.filters), prog.n_temps, prog.depth) == (2, 1, 1, 1, 1)

    # a two-operator voice behind one filter: two oscillator slots, one parameter, no temporary -- the SMALL register file
    two = ext.PMSine(); two.hertz = fix(row(220, 440)); two.index = fix(row(0.5, 4.0)); two.mod = sine(row(110, 220))
    f = fx.LowPass(); f.input = two; f.cutoff = fix(row(500, 5000))
    prog = _VoiceProgram(types.SimpleNamespace(owner=types.SimpleNamespace(specialise=False), N=256, _pure={}), f, V)
    assert (len(prog.oscs), len(prog.params), len(prog.filters), prog.n_temps) == (2, 1, 1, 0) and prog.worthwhile()

    # a band filter and a PM carrier: no interpreter variant has both, the per-node schedule keeps the graph
    bp = fx.BandPass(); bp.input = two; bp.low = fix(row(300, 400)); bp.high = fix(row(900, 1200))
    assert _VoiceProgram.compile(None, bp, V) is None


def test_pm_in_a_control_path_is_refused_with_its_reason():
    from signals_amd.engine import NotBatchable, _Batch, _ControlProgram
    pm = ext.PMSine(); pm.hertz = fix([[3.0]]); pm.index = fix([[1.0]]); pm.mod = sine([[1.0]])
    with pytest.raises(NotBatchable, match='phase-modulation oscillator has no block-rate program'):
        _ControlProgram((pm,), 4)
    g = fx.Gain(); g.left = pm; g.right = fix([[100.0]])
    with pytest.raises(NotBatchable, match='phase-modulation oscillator has no block-rate program'):
        _ControlProgram((g,), 4)
    lp = fx.LowPass(); lp.input = pm; lp.cutoff = fix([[10.0]])
    with pytest.raises(NotBatchable, match='phase-modulation oscillator has no window-rate program'):
        _ControlProgram((lp,), 4, channels=1)
    batch = _Batch(types.SimpleNamespace(rate=48000), 0, 256, 4, False)
    with pytest.raises(NotBatchable, match='phase-modulation oscillator has no block-rate schedule'):
        batch._control_node(pm, 'hertz')


# ---------------------------------------------------------------------------------------------- specialised build
def test_flags_of_a_pm_program():
    code = [('Osc', 0, 0, 0, 0), ('OscPM', 0, 1, 0, 0)]
    f = set(specialise.flags(code, 2, 1, 0, 0, 2, 2))
    assert {'-DSIG_VP_STATIC_CODE={0x0,0x10c}', '-DSIG_VP_S_NO=2', '-DSIG_VP_S_NP=1', '-DSIG_VP_S_EXT=0'} <= f


@pytest.mark.skipif(specialise.hipcc() is None, reason='no hipcc in this environment')
def test_the_specialised_pm_program_builds(tmp_path, monkeypatch):
    monkeypatch.setattr(specialise, 'CACHE', tmp_path)
    code = [('Osc', 0, 0, 0, 0), ('OscPM', 2, 1, 0, 0), ('Filter', 0, 0, 0, 0)]
    image = specialise.build(code, 2, 1, 1, 0, 2, 2)
    assert b'sig_vp_specialised' in image and b'sig_vp_specialised_info' in image
