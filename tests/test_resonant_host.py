"""The resonant low-pass / high-pass without a GPU: the numpy restatement (tests/resonant_reference.py) against the RBJ cookbook form,
against the oracle's Butterworth design at q = 1/sqrt2 and against scipy's sosfilt and the oracle's block semantics; the node API of
ext.ResonantLowPass / ResonantHighPass, name resolution and the .sigs loader; sig_biquad_coldstart_q's export and argument checks; the
FilterQ instruction's encoding, the programs the engine compiles for the node and the combinations it refuses; which launches the
planner picks for a resonant voice (on a stubbed library: no fused kernel may take it); the control-path refusal, sharding, and the
specialised build of a program with the instruction."""
import ctypes
import math
import pathlib
import types

import numpy as np
import pytest
import scipy.signal

from oracle import chain_ref as R
from signals_amd import SignalFlags, _native, specialise
from signals_amd.chain import ext, fixed, fx, osc

import resonant_reference as RR

ROOT = pathlib.Path(__file__).resolve().parent.parent
INV = 1     # hipErrorInvalidValue
RATE = 48000


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


def mkosc(cls, hz):
    o = cls(); o.hertz = fix(hz)
    return o


def resonant(cls, input_, cutoff, q=None):
    f = cls(); f.input = input_; f.cutoff = cutoff if not isinstance(cutoff, np.ndarray) else fix(cutoff)
    if q is not None:
        f.resonance = q if not isinstance(q, np.ndarray) else fix(q)
    return f


V = 8
row = lambda lo, hi: np.linspace(lo, hi, V).reshape(1, V)


# ---------------------------------------------------------------------------------------------- the restatement
def test_coefficients_against_the_rbj_cookbook_form():
    rng = np.random.default_rng(1)
    worst = 0.0
    for _ in range(4000):
        wn, q, btype = rng.uniform(0.001, 0.999), 10.0 ** rng.uniform(-1, 1.5), ('lp', 'hp')[rng.integers(2)]
        mine, rbj = RR.resonant_sos(wn, q, btype)[0], RR.rbj_sos(wn, q, btype)[0]
        worst = max(worst, float(np.max(np.abs(mine - rbj) / np.maximum(np.abs(rbj), 1e-300))))
    assert worst < 1e-10, worst                     # (8e-12 measured: two roundings of tan / sin / cos apart, amplified near wn = 1)


def test_coefficients_against_the_oracles_butterworth_at_q_one_over_sqrt2():
    rng = np.random.default_rng(2)
    for _ in range(4000):
        wn, btype = rng.uniform(0.001, 0.999), ('lp', 'hp')[rng.integers(2)]
        want = R.butter2_sos(wn, btype)
        assert np.array_equal(RR.resonant_sos(wn, None, btype), want)                     # unplugged: the damping is sqrt2 itself
        assert np.max(np.abs(RR.resonant_sos(wn, 1.0 / math.sqrt(2.0), btype) - want)) < 1e-15   # 1 / (1 / sqrt2): an ulp of sqrt2 apart


@pytest.mark.parametrize('bad', [0.0, -1.0, math.nan, math.inf, -math.inf])
def test_a_bad_resonance_and_a_bad_cutoff_raise(bad):
    with pytest.raises(ValueError, match='resonance must be finite and > 0'):
        RR.resonant_sos(0.3, bad, 'lp')
    for wn in (0.0, 1.0, math.nan):
        with pytest.raises(ValueError, match='critical frequencies'):
            RR.resonant_sos(wn, 2.0, 'hp')


def test_stable_for_every_q():
    rng = np.random.default_rng(3)
    for _ in range(4000):
        sos = RR.resonant_sos(rng.uniform(0.001, 0.999), 10.0 ** rng.uniform(-3, 3), 'lp')[0]
        a1, a2 = sos[4], sos[5]
        assert abs(a2) < 1.0 and abs(a1) < 1.0 + a2                            # the stability triangle


def test_filtered_blocks_against_scipy_sosfilt():
    rng = np.random.default_rng(4)
    frames, blocks, voices, history = 32, 5, 3, 50
    x = rng.uniform(-1, 1, (history + frames * blocks, voices))
    cut, q = rng.uniform(100, 15000, (blocks, voices)), rng.uniform(0.5, 8, (1, voices))
    for btype in ('lp', 'hp'):
        got = RR.filter_blocks(btype, x, history, frames, blocks, cut, q, RATE)
        for b in range(blocks):
            start = history + b * frames
            c = min(100, start)
            for v in range(voices):
                sos = RR.resonant_sos(cut[b, v] / (RATE / 2), q[0, v], btype)
                want = scipy.signal.sosfilt(sos, x[start - c:start + frames, v])[c:]
                assert np.array_equal(got[b * frames:(b + 1) * frames, v], want), (btype, b, v)


@pytest.mark.parametrize('pos,N', [(0, 128), (50, 128), (0, 32), (172_800_000, 128)])
def test_block_semantics_against_the_oracle_filter(pos, N):
    """cold start, context rows, the block cache and per-block control rows are chain_ref.Filter's: with q unplugged the oracle node
    renders the very rows of chain_ref.Filter (closed_form: the same arithmetic), with q = 1/sqrt2 plugged rows within rounding"""
    RF = RR.oracle_node()
    hz, cut = row(110, 880), row(300, 9000)
    lfo = lambda: R.Binary('Mix', R.Binary('Gain', R.Osc('Sine', R.Fixed([[40.0]])), R.Fixed(0.5 * cut)), R.Fixed(2.0 * cut), R.Fixed([[0.5]]))
    src = lambda: R.Osc('Sawtooth', R.Fixed(hz))
    for btype in ('lp', 'hp'):
        for sweep in (False, True):
            ctl = lfo if sweep else (lambda: R.Fixed(cut))
            want = R.render_stream(R.Filter(btype, src(), ctl(), closed_form=True), pos, N, 4, V)
            assert np.array_equal(R.render_stream(RF(btype, src(), ctl()), pos, N, 4, V), want)
            plugged = R.render_stream(RF(btype, src(), ctl(), R.Fixed(np.full((1, V), 1.0 / math.sqrt(2.0)))), pos, N, 4, V)
            assert np.max(np.abs(plugged - want)) < 1e-13      # coefficients 4.4e-16 apart, an L1 gain of a few, |x| <= 1
    # a cascade: the inner filter's cached block serves the outer one's context
    inner = lambda F, *a: F('hp', src(), R.Fixed(cut), *a)
    want = R.render_stream(R.Filter('lp', inner(R.Filter), R.Fixed(2 * cut), closed_form=True), pos, N, 4, V)
    if N > 100:
        got = R.render_stream(RF('lp', inner(RF), R.Fixed(2 * cut)), pos, N, 4, V)
        assert np.max(np.abs(got - want)) < 1e-13              # (the inner chain_ref.Filter designs through scipy.butter: 1e-15 apart)


# ---------------------------------------------------------------------------------------------- the node
@pytest.mark.parametrize('cls,btype', [(ext.ResonantLowPass, 'lp'), (ext.ResonantHighPass, 'hp')])
def test_node_api(cls, btype):
    assert cls.port_names() == ['cutoff', 'input', 'resonance']
    assert cls.flags() & SignalFlags.EFFECT and not cls.flags() & SignalFlags.GENERATOR
    assert issubclass(cls, ext.ResonantFilter) and issubclass(cls, fx.CritFilter) and not issubclass(cls, fx.SingleCritFilter)
    assert not issubclass(cls, fx.DoubleCritFilter)
    assert cls.cls_name() == f'signals.chain.ext.{cls.__name__}'
    n = cls()
    assert str(n.type()) == btype and n.context_frames() == 100 and not isinstance(n, fx.SingleCritFilter)
    n.input = mkosc(osc.Sawtooth, row(100, 200)); n.cutoff = fix(row(500, 900)); n.resonance = fix([[4.0]])
    assert n.channels == V
    doc = ext.ResonantFilter.__doc__
    for words in ('q = 1/sqrt2', 'unplugged answers zero', 'finite and > 0', 'IndexError', 'Not an `fx.SingleCritFilter`',
                  'q * rate / (pi * cutoff)', '83 % at 200 Hz', '45 % at 1 kHz', '9 % at 3 kHz', 'Out of scope', 'closed-form, row-walker, cascade',
                  'control path', 'band-pass, notch and peaking', 'frame-rate cutoff or q', 'self-oscillation', 'carried state or a longer context'):
        assert words in doc, words


def test_classes_resolve_by_qualified_name_and_load_from_a_patch():
    from signals_amd.chain import discovery, sigs
    from signals_amd.chain.driver import load_signal
    for cls in (ext.ResonantLowPass, ext.ResonantHighPass):
        assert load_signal(f'signals_amd.chain.ext.{cls.__name__}') is cls
        assert load_signal(f'signals.chain.ext.{cls.__name__}') is cls
        assert discovery.load_signal(f'signals.chain.ext.{cls.__name__}') is cls
    p = sigs.loads('+ 1a signals.chain.fixed.Fixed value=[[220]]\n+ 1b signals.chain.fixed.Fixed value=[[900]]\n'
                   '+ 1c signals.chain.fixed.Fixed value=[[4]]\n+ 1d signals.chain.osc.Sawtooth\n'
                   '+ 2a signals.chain.ext.ResonantLowPass\n> 1a 1d.hertz\n> 1d 2a.input\n> 1b 2a.cutoff\n> 1c 2a.resonance')
    node = p['2a']
    assert isinstance(node, ext.ResonantLowPass) and node.input.sig is p['1d'] and node.cutoff.sig is p['1b']
    assert node.resonance.sig is p['1c'] and p['1c'].get_state().value.dtype.kind == 'i'          # integers arrive as int64


# ---------------------------------------------------------------------------------------------- C ABI
def test_entry_point_is_exported_and_declared(lib):
    assert 'sig_biquad_coldstart_q' in _native.EXPORTS
    raw = ctypes.CDLL(str(_native.LIB_PATH))
    assert raw.sig_biquad_coldstart_q is not None
    assert lib.sig_abi_version() == 7                                         # additive
    header = (ROOT / 'include' / 'signals_amd.h').read_text()
    assert 'int sig_biquad_coldstart_q(' in header and 'SIG_VP_FILTERQ = 15' in header and 'SIG_STATUS_BAD_RESONANCE = 2' in header
    assert 'SIG_FILT_RES_LOWPASS = 4, SIG_FILT_RES_HIGHPASS = 5' in header
    assert _native.STATUS_BAD_RESONANCE == 2 and _native.STATUS_BAD_CUTOFF == 1
    assert _native.FILT_TYPES['rlp'] == 4 and _native.FILT_TYPES['rhp'] == 5


def test_biquad_coldstart_q_argument_errors_do_not_reach_the_device(lib):
    p = 64                                                                    # (never dereferenced: every call fails its checks)
    args = dict(type=0, rate=RATE, pos=0, N=256, K=4, ctx=100, voices=8, cut=p, cs=1, cb=1, res=p, rs=1, rb=1,
                x=p, xld=8, hist=0, out=p, old=8, dt=0, status=None, stream=None)

    def call(**over):
        a = dict(args, **over)
        return lib.sig_biquad_coldstart_q(*(a[k] for k in args))
    assert call(type=2) == INV and call(type=4) == INV and call(type=-1) == INV               # lp / hp only
    assert call(cut=None) == INV and call(x=None) == INV and call(out=None) == INV
    assert call(rs=2) == INV and call(rs=-1) == INV and call(rb=3) == INV and call(rb=0) == INV    # q rows: stride 0 / 1, 1 | nblocks rows
    assert call(res=None, rs=2) == INV and call(res=None, rb=3) == INV                        # (checked for a null row too)
    assert call(cs=2) == INV and call(cb=3) == INV
    assert call(rate=0) == INV and call(pos=-1) == INV and call(N=-1) == INV and call(voices=-1) == INV
    assert call(xld=4) == INV and call(old=4) == INV and call(pos=50, hist=49) == INV and call(dt=2, K=0) == 0
    assert call(dt=2) == INV
    assert call(K=0) == 0 and call(N=0) == 0 and call(voices=0, xld=0, old=0) == 0            # accepted, nothing to launch
    assert call(K=0, res=None) == 0 and call(K=0, rs=0) == 0
    assert call(K=4, N=0, rb=4, cb=4) == 0                                                   # per-block rows of both controls


def test_status_bit_raises_the_resonance_error():
    from signals_amd import runtime
    word = runtime.StatusWord('signals.chain.ext.ResonantLowPass')
    word.tensor[0] = _native.STATUS_BAD_RESONANCE
    with pytest.raises(ValueError, match=r'signals.chain.ext.ResonantLowPass: filter resonance must be finite and > 0'):
        runtime.check_status()
    runtime.check_status()                                                    # (polled: cleared)
    word.tensor[0] = _native.STATUS_BAD_CUTOFF
    with pytest.raises(ValueError, match='critical frequencies'):
        runtime.check_status()


# ---------------------------------------------------------------------------------------------- the instruction
def test_instruction_encoding():
    assert _native.VP_OPS['FilterQ'] == 15 and _native.VP_RES_OPS == ('FilterQ',)
    assert _native.voice_program_words([('FilterQ', 0, 0, 0, -1)]) == [0xf000f]           # q unplugged: slot 15
    assert _native.voice_program_words([('FilterQ', 0, 1, 0, 2)]) == [0x2010f]
    assert 'FilterQ' not in _native.VP_EXT_OPS and 'FilterQ' not in _native.VP_TABLE_OPS


def _program(code, n_oscs=1, n_params=1, types=(), levels=None):
    P = _native.VoiceProgramT()
    P.n_ins = len(code)
    for k, (op, kind, a, b, c) in enumerate(code):
        P.ins[k] = _native.VpIns(_native.VP_OPS[op], kind, a, b, c)
    keep = ctypes.c_double(440.0)
    ptr = ctypes.cast(ctypes.pointer(keep), ctypes.c_void_p).value
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
        P.filter_level[k] = (levels or [1] * len(types))[k]
    P.depth = max(levels or [1]) if types else 0
    return P, keep


def test_voice_program_filterq_argument_checks(lib):
    buf = (ctypes.c_float * 64)()

    def run(code, nblocks=1, tabs=None, **kw):
        P, keep = _program(code, **kw)
        return lib.sig_voice_program_ex(ctypes.byref(P), RATE, 0, 256, nblocks, 100, 8, 2 if nblocks else 1, 0, None, 0, None, 0, 0, None,
                                        ctypes.addressof(buf), 8, None, None, ctypes.byref(tabs) if tabs is not None else None)
    src, fq = ('Osc', 2, 0, 0, 0), ('FilterQ', 0, 0, 0, 0)
    # accepted (no blocks: no launch)
    assert run([src, fq], types=['rlp'], nblocks=0) == 0 and run([src, ('FilterQ', 0, 0, 0, -1)], types=['rhp'], n_params=0, nblocks=0) == 0
    assert run([src, fq], types=['lp']) == INV                                # the word on a Butterworth slot
    assert run([src, ('Filter', 0, 0, 0, 0)], types=['rlp']) == INV           # a Filter word on a resonant slot
    assert run([src], types=['rlp']) == INV                                   # a resonant slot without its word
    assert run([src, fq, fq], types=['rlp']) == INV                           # one word per slot
    assert run([src, ('FilterQ', 0, 1, 0, 0)], types=['rlp']) == INV          # slot 1 of 1
    assert run([src, ('FilterQ', 0, 0, 0, 1)], types=['rlp']) == INV          # q: parameter slot 1 of 1
    assert run([src, ('FilterQ', 0, 0, 0, -2)], types=['rlp']) == INV
    # resonant -> plain in one program; the refusals: no variant has the resonant design with a band, a PM carrier or a table
    assert run([src, fq, ('Filter', 0, 1, 0, 0)], types=['rhp', 'lp'], levels=[1, 2], nblocks=0) == 0
    assert run([src, fq, ('Band', 0, 1, 0, 0)], types=['rlp', 'bp', 'bp'], levels=[1, 2, 2]) == INV
    assert run([src, ('OscPM', 0, 1, 0, 0), fq], n_oscs=2, types=['rlp']) == INV
    t = _native.VpTablesT(); t.n_tables = 1; t.table[0] = _native.VpTable(64, 64, 1)
    assert run([('OscTable', 0, 0, 0, -1), fq], types=['rlp'], tabs=t) == INV
    assert run([src, fq, ('Shape', 0, 0, 0, -1)], types=['rlp'], tabs=t) == INV
    assert run([('OscTable', 0, 0, 0, -1)], tabs=t, nblocks=0) == 0                   # (the table program itself is accepted)


def test_voice_program_words():
    from signals_amd.engine import _VoiceProgram
    SAW = _native.OSC_KINDS['Sawtooth']
    one = resonant(ext.ResonantLowPass, mkosc(osc.Sawtooth, row(100, 200)), row(500, 5000), row(0.5, 8))
    prog = _VoiceProgram(None, one, V)
    assert prog.code == [('Osc', SAW, 0, 0, 0), ('FilterQ', 0, 0, 0, 0)]
    assert _native.voice_program_words(prog.code) == [0x40, 0xf]
    assert [(t, level) for _, t, level, _ in prog.filters] == [('rlp', 1)] and prog.resonant == [(one, 0)]
    assert (len(prog.oscs), len(prog.params), prog.n_temps, prog.depth) == (1, 1, 0, 1)
    assert prog.controls[prog.params[0]][0] is one.resonance and prog.controls[prog.filters[0][0]][0] is one.cutoff
    assert prog.controls[prog.params[0]][2] == prog.controls[prog.filters[0][0]][2] == 0     # both read where the filter is designed
    batch = types.SimpleNamespace(owner=types.SimpleNamespace(specialise=False), N=256, _pure={})
    assert _VoiceProgram(batch, one, V).worthwhile()                          # the SMALL register file

    unplugged = resonant(ext.ResonantHighPass, mkosc(osc.Sawtooth, row(100, 200)), row(500, 5000))
    prog = _VoiceProgram(None, unplugged, V)
    assert prog.code[-1] == ('FilterQ', 0, 0, 0, -1) and prog.params == [] and prog.filters[0][1] == 'rhp'
    off = resonant(ext.ResonantHighPass, mkosc(osc.Sawtooth, row(100, 200)), row(500, 5000), row(1, 2))
    off.resonance.sig.get_state().enabled = False                             # a disabled source: unplugged
    assert _VoiceProgram(None, off, V).code[-1] == ('FilterQ', 0, 0, 0, -1)

    # ResonantHighPass -> LowPass: one program, the plain filter's word beside the resonant one's
    lp = fx.LowPass(); lp.cutoff = fix(row(2000, 9000))
    lp.input = resonant(ext.ResonantHighPass, mkosc(osc.Sawtooth, row(100, 200)), row(100, 900), row(1, 4))
    prog = _VoiceProgram(None, lp, V)
    assert prog.code == [('Osc', SAW, 0, 0, 0), ('FilterQ', 0, 0, 0, 0), ('Filter', 0, 1, 0, 0)]
    assert [(t, level) for _, t, level, _ in prog.filters] == [('rhp', 1), ('lp', 2)] and prog.depth == 2
    assert prog.controls[prog.params[0]][2] == 1                              # q of the inner filter: one filter between it and the sink

    # a resonant pair behind a Mix: two slots, two q registers and the mix
    m = fx.Mix(); m.mix = fix([[0.5]])
    m.left = resonant(ext.ResonantLowPass, mkosc(osc.Sawtooth, row(100, 200)), row(500, 5000), row(0.5, 8))
    m.right = resonant(ext.ResonantHighPass, mkosc(osc.Square, row(100, 200)), row(500, 5000), row(0.5, 8))
    prog = _VoiceProgram(None, m, V)
    assert prog.code == [('Osc', SAW, 0, 0, 0), ('FilterQ', 0, 0, 0, 0), ('Save', 0, 0, 0, 0), ('Osc', _native.OSC_KINDS['Square'], 1, 0, 0),
                         ('FilterQ', 0, 1, 0, 1), ('Mix', 0, 0, 2, 0)]
    assert [t for _, t, _, _ in prog.filters] == ['rlp', 'rhp'] and len(prog.params) == 3

    # ResonantLowPass(Mix(Saw, Square)) -> LowPass
    mix = fx.Mix(); mix.left = mkosc(osc.Sawtooth, row(100, 200)); mix.right = mkosc(osc.Square, row(100, 200)); mix.mix = fix([[0.3]])
    lp = fx.LowPass(); lp.cutoff = fix(row(2000, 9000)); lp.input = resonant(ext.ResonantLowPass, mix, row(500, 5000), row(0.5, 8))
    assert [op for op, *_ in _VoiceProgram(None, lp, V).code] == ['Osc', 'Save', 'Osc', 'Mix', 'FilterQ', 'Filter']


def test_voice_program_refusals_name_their_reason():
    from signals_amd.engine import _NoProgram, _VoiceProgram
    res = lambda src: resonant(ext.ResonantLowPass, src, row(500, 5000), row(0.5, 8))
    bp = fx.BandPass(); bp.input = res(mkosc(osc.Sawtooth, row(100, 200))); bp.low = fix(row(300, 400)); bp.high = fix(row(900, 1200))
    with pytest.raises(_NoProgram, match='a resonant filter and a band filter'):
        _VoiceProgram(None, bp, V)
    pm = ext.PMSine(); pm.hertz = fix(row(220, 440)); pm.index = fix([[1.0]]); pm.mod = mkosc(osc.Sawtooth, row(110, 220))
    with pytest.raises(_NoProgram, match='a resonant filter and a phase-modulation oscillator'):
        _VoiceProgram(None, res(pm), V)
    wt = ext.Wavetable(); wt.hertz = fix(row(220, 440))
    with pytest.raises(_NoProgram, match='a resonant filter and a wavetable oscillator or a waveshaper'):
        _VoiceProgram(None, res(wt), V)
    sh = ext.Shaper(); sh.input = res(mkosc(osc.Sawtooth, row(100, 200)))
    with pytest.raises(_NoProgram, match='a resonant filter and a wavetable oscillator or a waveshaper'):
        _VoiceProgram(None, sh, V)
    for top in (bp, res(pm), res(wt), sh):
        assert _VoiceProgram.compile(None, top, V) is None                    # the graph stays one kernel per node


# ---------------------------------------------------------------------------------------------- planning
def test_purity_and_modulation_classification():
    from signals_amd.engine import _KNOWN_TYPES, _audio_ports, _control_ports, _ctl_const, _foreign, _is_pure, _modulated
    f = resonant(ext.ResonantLowPass, mkosc(osc.Sawtooth, [[440.0]]), np.array([[900.0]]), np.array([[4.0]]))
    assert isinstance(f, _KNOWN_TYPES) and not _foreign(f)
    assert _control_ports(f) == [f.cutoff, f.resonance] and _audio_ports(f) == [f.input]
    assert all(_ctl_const(p) for p in _control_ports(f)) and not _modulated(f) and not _is_pure(f, {})      # a filter: never pure
    swept = resonant(ext.ResonantLowPass, mkosc(osc.Sawtooth, [[440.0]]), np.array([[900.0]]), mkosc(osc.Sine, [[2.0]]))
    assert _modulated(swept)                                                  # q re-read every block


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
        def __getattr__(self, name):
            return lambda *a: 0
    monkeypatch.setattr(_native, 'lib', lambda: Lib())
    monkeypatch.setattr(_native, '_gpu', lambda *a: None)
    monkeypatch.setattr(_native, '_stream', lambda t: 0)


FUSED = ('fused', 'latency', 'cascade', 'steady', 'walk', 'biquad_coldstart[', 'biquad_bus', 'biquad_coldstart_env')


@pytest.mark.parametrize('kind', [osc.Sine, osc.Sawtooth])
@pytest.mark.parametrize('shape', ['plain', 'gain', 'bus', 'gain_bus', 'cascade_bus', 'enveloped'])
def test_no_fused_matcher_takes_a_resonant_voice(stubbed, kind, shape):
    """the closed-form / walker voice chain, the cascade, the enveloped filter and the bus over a filter all match fx.SingleCritFilter:
    with the voice program switched off a resonant voice runs one kernel per node, with it on as a FilterQ program"""
    from signals_amd.engine import BatchRenderer

    def build():
        top = resonant(ext.ResonantLowPass, mkosc(kind, row(100, 200)), row(500, 5000), row(0.5, 8))
        if shape == 'cascade_bus':
            top = resonant(ext.ResonantHighPass, top, row(50, 90), row(0.5, 2))
        if shape == 'enveloped':
            env = ext.ADSR()
            for name in _native.ADSR_PARAMS:
                setattr(env, name, fix([[0.01]]))
            rm = fx.RingMod(); rm.left = top; rm.right = env
            top = rm
        if 'gain' in shape:
            g = fx.Gain(); g.left = top; g.right = fix(row(0.1, 1.0))
            top = g
        if 'bus' in shape or shape == 'enveloped':
            b = ext.SumBus(); b.input = top
            return b, 1
        return top, V
    for kw, programmed in (({'fuse_program': False}, False), ({}, True)):
        top, C = build()
        rec = _Recorder()
        r = BatchRenderer(top, C, RATE, timer=rec, **kw)
        r.render(0, 256, 3)
        r.render(768, 256, 2)
        assert not any(word in n for n in rec.names for word in FUSED), (kw, rec.names)
        if programmed:
            programs = [n for n in rec.names if n.startswith(('voice_program[', 'voice_program_bus['))]
            assert len(programs) == 2 and all('FilterQ' in n for n in programs), rec.names
            # (an envelope is outside the small register file: the default keeps it, its product and the bus per node)
            assert shape == 'enveloped' or programs == rec.names, rec.names
        else:
            assert sum(n.startswith('biquad_coldstart_q[lp]') for n in rec.names) >= 2, rec.names
            assert any(n.startswith('osc_bank[') for n in rec.names), rec.names


def test_swept_controls_launch_the_per_block_form(stubbed):
    from signals_amd.engine import BatchRenderer
    lfo = fx.Gain(); lfo.left = mkosc(osc.Sine, [[3.0]]); lfo.right = fix(row(1.0, 2.0))
    top = resonant(ext.ResonantHighPass, mkosc(osc.Sawtooth, row(100, 200)), row(500, 5000), lfo)
    rec = _Recorder()
    BatchRenderer(top, V, RATE, timer=rec, fuse=False).render(0, 256, 3)
    assert 'biquad_coldstart_q[hp,blocks]' in rec.names, rec.names


def test_a_narrow_resonance_raises_like_a_narrow_cutoff(stubbed):
    from signals_amd.engine import BatchRenderer
    for kw in ({'fuse': False}, {'fuse_program': 'always'}):
        top = resonant(ext.ResonantLowPass, mkosc(osc.Sawtooth, row(100, 200)), row(500, 5000), np.array([[1.0, 2.0, 3.0]]))
        with pytest.raises(IndexError, match='index 3 is out of bounds for axis 1 with size 3'):
            BatchRenderer(top, V, RATE, **kw).render(0, 256, 2)
        top = resonant(ext.ResonantLowPass, mkosc(osc.Sawtooth, row(100, 200)), np.array([[500.0, 600.0, 700.0]]), row(1, 2))
        with pytest.raises(IndexError, match='index 3 is out of bounds for axis 1 with size 3'):
            BatchRenderer(top, V, RATE, **kw).render(0, 256, 2)


def test_a_resonant_filter_in_a_control_path_is_refused_with_its_reason():
    from signals_amd.engine import NotBatchable, _Batch, _ControlProgram
    f = resonant(ext.ResonantLowPass, mkosc(osc.Sine, [[3.0]]), np.array([[10.0]]), np.array([[2.0]]))
    with pytest.raises(NotBatchable, match='resonant filter has no block-rate program'):
        _ControlProgram((f,), 4, channels=1)
    g = fx.Gain(); g.left = f; g.right = fix([[100.0]])
    with pytest.raises(NotBatchable, match='resonant filter has no block-rate program'):
        _ControlProgram((g,), 4, channels=1)
    batch = _Batch(types.SimpleNamespace(rate=RATE), 0, 256, 4, False)
    with pytest.raises(NotBatchable, match='resonant filter has no block-rate schedule'):
        batch._control_node(f, 'right')


def test_sharded_renderer_hands_every_rank_its_slice_of_resonance(monkeypatch):
    from signals_amd import parallel
    from signals_amd.engine import BatchRenderer, _VoiceProgram
    voices, world = 12, 3
    hertz, cut, q = np.linspace(100, 200, voices)[None, :], np.linspace(300, 3000, voices)[None, :], np.linspace(0.5, 8, voices)[None, :]
    built = {}

    def build(lo, hi):
        f = resonant(ext.ResonantLowPass, mkosc(osc.Sawtooth, hertz[:, lo:hi]), cut[:, lo:hi], q[:, lo:hi])
        bus = ext.SumBus(); bus.input = f
        built[(lo, hi)] = f
        return bus
    monkeypatch.setattr(parallel.dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(parallel.dist, 'get_world_size', lambda: world)
    covered = []
    for rank in range(world):
        monkeypatch.setattr(parallel.dist, 'get_rank', lambda rank=rank: rank)
        r = parallel.ShardedRenderer(build, voices, 1, fuse_program='always')
        assert (r.rank, r.world) == (rank, world) and (r.lo, r.hi) == parallel.shard_voices(voices, world, rank)
        assert isinstance(r.renderer, BatchRenderer)
        f = built[(r.lo, r.hi)]
        assert r.renderer.node.input.sig is f and f.channels == r.hi - r.lo
        assert np.array_equal(f.resonance.sig.get_state().value, q[:, r.lo:r.hi])       # scattered like cutoff and hertz
        assert np.array_equal(f.cutoff.sig.get_state().value, cut[:, r.lo:r.hi])
        prog = _VoiceProgram(None, f, r.hi - r.lo)
        assert prog.code[-1] == ('FilterQ', 0, 0, 0, 0) and prog.controls[prog.params[0]][0] is f.resonance
        covered += list(range(r.lo, r.hi))
    assert covered == list(range(voices))


# ---------------------------------------------------------------------------------------------- specialised build
def test_flags_of_a_resonant_program():
    code = [('Osc', 2, 0, 0, 0), ('FilterQ', 0, 0, 0, 0)]
    f = set(specialise.flags(code, 1, 1, 1, 0, 2, 2))
    assert {'-DSIG_VP_STATIC_CODE={0x40,0xf}', '-DSIG_VP_S_RES=1', '-DSIG_VP_S_NF=1', '-DSIG_VP_S_NP=1', '-DSIG_VP_S_EXT=0'} <= f
    assert not any('SIG_VP_S_TAB' in x for x in f)
    plain = specialise.flags([('Osc', 2, 0, 0, 0), ('Filter', 0, 0, 0, 0)], 1, 0, 1, 0, 2, 2)
    assert not any('SIG_VP_S_RES' in x for x in plain)                        # programs without the word keep their flags


@pytest.mark.skipif(specialise.hipcc() is None, reason='no hipcc in this environment')
def test_the_specialised_resonant_program_builds(tmp_path, monkeypatch):
    monkeypatch.setattr(specialise, 'CACHE', tmp_path)
    code = [('Osc', 2, 0, 0, 0), ('FilterQ', 0, 0, 0, 0), ('Filter', 0, 1, 0, 0), ('Gain', 0, 1, 0, 0)]
    image = specialise.build(code, 1, 2, 2, 0, 2, 2)
    assert b'sig_vp_specialised' in image and b'sig_vp_specialised_info' in image
