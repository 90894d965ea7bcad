"""The RBJ equaliser biquads without a GPU: the numpy restatement (tests/eq_reference.py) against the cookbook's trigonometric forms, its
identities (Peaking at 0 dB, the denominators shared with the resonant low-pass) and scipy's sosfilt; the node API of ext.EqFilter's six
classes; sig_biquad_coldstart_eq's export and argument checks; the FilterEq instruction's encoding (b = -1 included), the programs the
engine compiles for the nodes, the variant the library names and the entries that refuse the word; which launches the planner picks (on
a stubbed library); the specialised build's flags and the image of one equaliser program."""
import ctypes
import math
import pathlib

import numpy as np
import pytest
import scipy.signal

from signals_amd import SignalFlags, _native, specialise
from signals_amd.chain import BadStateValue, ext, fixed, fx, osc

import eq_reference as EQ
import resonant_reference as RR

ROOT = pathlib.Path(__file__).resolve().parent.parent
INV = 1     # hipErrorInvalidValue
RATE = 48000
CLASSES = {'bp': ext.ResonantBandPass, 'notch': ext.Notch, 'ap': ext.AllPass, 'peak': ext.Peaking, 'ls': ext.LowShelf, 'hs': ext.HighShelf}
QS, GAINS, WNS = (0.5, 1.0 / math.sqrt(2.0), 4.0), (-12.0, 0.0, 12.0), (0.01, 0.3, 0.9)


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


def eq(cls, input_, cutoff, q=None, gain=None):
    f = cls(); f.input = input_; f.cutoff = cutoff if not isinstance(cutoff, np.ndarray) else fix(cutoff)
    if q is not None:
        f.resonance = q if not isinstance(q, np.ndarray) else fix(q)
    if gain is not None:
        f.gain = gain if not isinstance(gain, np.ndarray) else fix(gain)
    return f


V = 8
row = lambda lo, hi: np.linspace(lo, hi, V).reshape(1, V)


# ---------------------------------------------------------------------------------------------- the restatement
def _cookbook(wn, q, gain, kind):
    """the cookbook's tables, written here on their own: w0 = pi wn, alpha = sin w0 / (2 q), A = 10^(dB / 40); normalised by a0"""
    w0 = math.pi * wn
    c, al, A = math.cos(w0), math.sin(w0) / (2.0 * q), 10.0 ** (gain / 40.0)
    rA = 2.0 * math.sqrt(A) * al
    b, a = {
        'bp': ([al, 0.0, -al], [1 + al, -2 * c, 1 - al]),
        'notch': ([1.0, -2 * c, 1.0], [1 + al, -2 * c, 1 - al]),
        'ap': ([1 - al, -2 * c, 1 + al], [1 + al, -2 * c, 1 - al]),
        'peak': ([1 + al * A, -2 * c, 1 - al * A], [1 + al / A, -2 * c, 1 - al / A]),
        'ls': ([A * ((A + 1) - (A - 1) * c + rA), 2 * A * ((A - 1) - (A + 1) * c), A * ((A + 1) - (A - 1) * c - rA)],
               [(A + 1) + (A - 1) * c + rA, -2 * ((A - 1) + (A + 1) * c), (A + 1) + (A - 1) * c - rA]),
        'hs': ([A * ((A + 1) + (A - 1) * c + rA), -2 * A * ((A - 1) + (A + 1) * c), A * ((A + 1) + (A - 1) * c - rA)],
               [(A + 1) - (A - 1) * c + rA, 2 * ((A - 1) - (A + 1) * c), (A + 1) - (A - 1) * c - rA]),
    }[kind]
    return np.array(b) / a[0], np.array(a) / a[0]


@pytest.mark.parametrize('kind', EQ.KINDS)
def test_coefficients_against_the_cookbooks_trigonometric_forms(kind):
    """1e-12 relative, coefficient by coefficient (the band-pass's middle tap is 0 in both forms)"""
    worst = 0.0
    for q in QS:
        for gain in GAINS:
            for wn in WNS:
                sos = EQ.eq_sos(wn, q, gain, kind)[0]
                b, a = _cookbook(wn, q, gain, kind)
                want = np.concatenate([b, a])
                zero = want == 0.0
                assert np.array_equal(sos[zero], want[zero]), (kind, q, gain, wn)
                err = float(np.max(np.abs(sos[~zero] - want[~zero]) / np.abs(want[~zero])))
                print(f'{kind} q={q:.3f} gain={gain:+.0f} wn={wn}: {err:.2e}')
                worst = max(worst, err)
                assert np.allclose(EQ.rbj_sos(wn, q, gain, kind)[0], want, rtol=1e-13, atol=1e-15)
    assert worst < 1e-12, worst


def test_peaking_at_zero_db_is_the_identity_section():
    for q in QS + (None,):
        for wn in WNS:
            for gain in (0.0, None, -0.0):
                sos = EQ.eq_sos(wn, q, gain, 'peak')[0]
                assert np.array_equal(sos[:3], sos[3:]), (q, wn, sos)
    x = np.random.default_rng(0).uniform(-1, 1, 300)
    assert np.max(np.abs(scipy.signal.sosfilt(EQ.eq_sos(0.3, 4.0, 0.0, 'peak'), x) - x)) < 1e-13


def test_notch_and_allpass_denominators_are_the_resonant_lowpass_bits():
    rng = np.random.default_rng(5)
    for _ in range(2000):
        wn, q = rng.uniform(0.001, 0.999), 10.0 ** rng.uniform(-1, 1.5)
        want = RR.resonant_sos(wn, q, 'lp')[0, 3:]
        for kind in ('notch', 'ap', 'bp'):
            assert np.array_equal(EQ.eq_sos(wn, q, None, kind)[0, 3:], want), (kind, wn, q)
        assert np.array_equal(EQ.eq_sos(wn, None, None, 'notch')[0, 3:], RR.resonant_sos(wn, None, 'lp')[0, 3:])     # unplugged: sqrt2 itself


def test_responses_are_what_their_names_say():
    w = np.array([0.3 * math.pi])
    for q in QS:
        mag = lambda kind, g=0.0, at=w: np.abs(scipy.signal.sosfreqz(EQ.eq_sos(0.3, q, g, kind), worN=at)[1])
        assert abs(mag('bp')[0] - 1.0) < 1e-12 and mag('notch')[0] < 1e-12            # constant 0 dB peak; the null
        assert np.max(np.abs(mag('ap', at=np.linspace(0.01, 3.1, 50)) - 1.0)) < 1e-12
        for g in (-12.0, 12.0):
            assert abs(20 * math.log10(mag('peak', g)[0]) - g) < 1e-9
            assert abs(20 * math.log10(mag('ls', g, np.array([1e-6]))[0]) - g) < 1e-6
            assert abs(20 * math.log10(mag('hs', g, np.array([math.pi]))[0]) - g) < 1e-6
            assert abs(20 * math.log10(mag('ls', g)[0]) - g / 2) < 1e-9                # the cutoff is the shelf's midpoint


@pytest.mark.parametrize('bad', [math.nan, math.inf, -math.inf])
def test_bad_controls_raise(bad):
    for kind in EQ.GAIN_KINDS:
        with pytest.raises(ValueError, match='gain must be finite'):
            EQ.eq_sos(0.3, 2.0, bad, kind)
    EQ.eq_sos(0.3, 2.0, bad, 'notch')                                          # (no gain port: not read)
    for kind in EQ.KINDS:
        with pytest.raises(ValueError, match='resonance must be finite and > 0'):
            EQ.eq_sos(0.3, bad, 0.0, kind)
        with pytest.raises(ValueError, match='resonance must be finite and > 0'):
            EQ.eq_sos(0.3, 0.0, 0.0, kind)
        for wn in (0.0, 1.0, math.nan):
            with pytest.raises(ValueError, match='critical frequencies'):
                EQ.eq_sos(wn, 2.0, 0.0, kind)


def test_filtered_blocks_against_scipy_sosfilt():
    rng = np.random.default_rng(4)
    frames, blocks, voices, history = 32, 5, 3, 50
    x = rng.uniform(-1, 1, (history + frames * blocks, voices))
    cut, q, gain = rng.uniform(100, 15000, (blocks, voices)), rng.uniform(0.5, 8, (1, voices)), rng.uniform(-12, 12, (blocks, 1))
    for kind in EQ.KINDS:
        got = EQ.filter_blocks(kind, x, history, frames, blocks, cut, q, gain, RATE)
        for b in range(blocks):
            start = history + b * frames
            c = min(100, start)
            for v in range(voices):
                sos = EQ.eq_sos(cut[b, v] / (RATE / 2), q[0, v], gain[b, 0], kind)
                want = scipy.signal.sosfilt(sos, x[start - c:start + frames, v])[c:]
                assert np.array_equal(got[b * frames:(b + 1) * frames, v], want), (kind, b, v)
    bad = EQ.filter_blocks('peak', x, history, frames, blocks, cut, q, np.array([[math.inf, 0.0, 0.0]]), RATE, lenient=True)
    assert np.isnan(bad[:, 0]).all() and np.isfinite(bad[:, 1:]).all()


def test_block_semantics_against_the_oracle_filter():
    """the oracle node shares chain_ref.Filter's cache and context semantics: a Peaking at 0 dB in front of a LowPass renders the
    LowPass's rows of the bare source (to rounding: the identity section's recurrence cancels to an ulp)"""
    from oracle import chain_ref as R
    EF = EQ.oracle_node()
    hz, cut = row(110, 880), row(300, 9000)
    src = lambda: R.Osc('Sawtooth', R.Fixed(hz))
    for pos, N in ((0, 128), (50, 128), (0, 32)):
        want = R.render_stream(R.Filter('lp', src(), R.Fixed(cut), closed_form=True), pos, N, 4, V)
        got = R.render_stream(R.Filter('lp', EF('peak', src(), R.Fixed(2 * cut), R.Fixed(row(0.5, 4))), R.Fixed(cut), closed_form=True), pos, N, 4, V)
        assert np.max(np.abs(got - want)) < 1e-12, (pos, N)


# ---------------------------------------------------------------------------------------------- the nodes
@pytest.mark.parametrize('kind', EQ.KINDS)
def test_node_api(kind):
    cls = CLASSES[kind]
    gained = kind in EQ.GAIN_KINDS
    assert cls.port_names() == (['cutoff', 'gain', 'input', 'resonance'] if gained else ['cutoff', 'input', 'resonance'])
    assert cls.flags() & SignalFlags.EFFECT and not cls.flags() & SignalFlags.GENERATOR
    assert issubclass(cls, ext.EqFilter) and issubclass(cls, ext.ResonantFilter) and issubclass(cls, fx.CritFilter)
    assert not issubclass(cls, fx.SingleCritFilter) and not issubclass(cls, fx.DoubleCritFilter)
    assert cls.cls_name() == f'signals.chain.ext.{cls.__name__}'
    n = cls()
    assert str(n.type()) == 'eq' + kind and _native.FILT_TYPES[str(n.type())] == 6 + EQ.KINDS.index(kind)
    assert n.type().has_gain == gained and not n.type().is_band and n.context_frames() == 100
    assert (n.gain_port() is not None) == gained
    assert n.resonance.sig is None and (not gained or n.gain.sig is None)      # defaults: unplugged = 1/sqrt2 and 0 dB
    n.input = mkosc(osc.Sawtooth, row(100, 200)); n.cutoff = fix(row(500, 900)); n.resonance = fix([[4.0]])
    assert n.channels == V


def test_docstring_states_the_formulae_the_truncation_and_the_scope():
    doc = ext.EqFilter.__doc__
    for words in ('A = exp(gain * ln(10) / 40)', 'g = sqrt(A) * d', 'b = (d*k, 0, -d*k)', 'b = (1 + k*k, 2*(k*k - 1), 1 + k*k)',
                  'b = (1 - d*k + k*k, 2*(k*k - 1), 1 + d*k + k*k)', '1 - (d/A)*k + k*k', '1/nrm = A + g*k + k*k', '1/nrm = 1 + g*k + A*k*k',
                  'y = b0 x + z0', 'means 0 dB', 'filter gain must be finite', 'IndexError', '100-frame cold start',
                  'high-q `Notch` and `ResonantBandPass` at low cutoffs', 'Out of scope', 'frame-rate cutoff, q or gain',
                  'closed-form, row-walker, cascade', 'control path', 'constant-skirt band-pass', 'shelf-slope S', 'b = a'):
        assert words in doc, words


def test_classes_resolve_by_qualified_name_and_load_from_a_patch():
    from signals_amd.chain import discovery, sigs
    from signals_amd.chain.driver import load_signal
    for cls in CLASSES.values():
        assert load_signal(f'signals_amd.chain.ext.{cls.__name__}') is cls
        assert load_signal(f'signals.chain.ext.{cls.__name__}') is cls
        assert discovery.load_signal(f'signals.chain.ext.{cls.__name__}') is cls
    p = sigs.loads('+ 1a signals.chain.fixed.Fixed value=[[220]]\n+ 1b signals.chain.fixed.Fixed value=[[900]]\n'
                   '+ 1c signals.chain.fixed.Fixed value=[[4]]\n+ 1d signals.chain.osc.Sawtooth\n+ 1e signals.chain.fixed.Fixed value=[[-6]]\n'
                   '+ 2a signals.chain.ext.Peaking\n> 1a 1d.hertz\n> 1d 2a.input\n> 1b 2a.cutoff\n> 1c 2a.resonance\n> 1e 2a.gain')
    node = p['2a']
    assert isinstance(node, ext.Peaking) and node.input.sig is p['1d'] and node.gain.sig is p['1e'] and node.resonance.sig is p['1c']


def test_bad_state_is_refused_as_on_every_filter_node():
    """the nodes keep no state of their own (their controls are ports, like ResonantFilter's): a bad value is the plugged Fixed's
    BadStateValue"""
    for cls in CLASSES.values():
        n = cls()
        assert type(n.get_state()) is type(ext.ResonantLowPass().get_state())
        n.resonance = fix([[2.0]])
        with pytest.raises(BadStateValue, match='must be a 2D array'):
            n.resonance.sig.get_state().value = np.array([1.0, 2.0])
        if n.gain_port() is not None:
            n.gain = fix([[6.0]])
            with pytest.raises(BadStateValue, match='must be a 2D array'):
                n.gain.sig.get_state().value = 6.0


# ---------------------------------------------------------------------------------------------- C ABI
def test_entry_point_is_exported_and_declared(lib):
    assert 'sig_biquad_coldstart_eq' in _native.EXPORTS
    raw = ctypes.CDLL(str(_native.LIB_PATH))
    assert raw.sig_biquad_coldstart_eq is not None
    assert lib.sig_abi_version() == 7                                         # additive
    header = (ROOT / 'include' / 'signals_amd.h').read_text()
    assert 'int sig_biquad_coldstart_eq(' in header and 'SIG_VP_FILTEREQ = 18' in header and 'SIG_STATUS_BAD_GAIN = 4' in header
    assert ('SIG_FILT_EQ_BANDPASS = 6, SIG_FILT_EQ_NOTCH = 7, SIG_FILT_EQ_ALLPASS = 8, SIG_FILT_EQ_PEAKING = 9, SIG_FILT_EQ_LOWSHELF = 10,\n'
            '       SIG_FILT_EQ_HIGHSHELF = 11') in header
    assert _native.STATUS_BAD_GAIN == 4 and _native.STATUS_BAD_RESONANCE == 2 and _native.STATUS_BAD_CUTOFF == 1
    assert [_native.FILT_TYPES['eq' + k] for k in EQ.KINDS] == [6, 7, 8, 9, 10, 11]
    assert _native.EQ_GAIN_TYPES == ('eqpeak', 'eqls', 'eqhs')


def test_biquad_coldstart_eq_argument_errors_do_not_reach_the_device(lib):
    p = 64                                                                    # (never dereferenced: every call fails its checks)
    args = dict(type=9, rate=RATE, pos=0, N=256, K=4, ctx=100, voices=8, cut=p, cs=1, cb=1, res=p, rs=1, rb=1, gain=p, gs=1, gb=1,
                x=p, xld=8, hist=0, out=p, old=8, dt=0, status=None, stream=None)

    def call(**over):
        a = dict(args, **over)
        return lib.sig_biquad_coldstart_eq(*(a[k] for k in args))
    assert call(type=0) == INV and call(type=5) == INV and call(type=12) == INV and call(type=-1) == INV     # the six equaliser types only
    assert call(cut=None) == INV and call(x=None) == INV and call(out=None) == INV
    assert call(rs=2) == INV and call(rb=3) == INV and call(gs=2) == INV and call(gs=-1) == INV and call(gb=3) == INV and call(gb=0) == INV
    assert call(gain=None, gs=2) == INV and call(res=None, rb=3) == INV       # (checked for a null row too)
    assert call(cs=2) == INV and call(cb=3) == INV and call(rate=0) == INV and call(pos=-1) == INV and call(N=-1) == INV
    assert call(xld=4) == INV and call(old=4) == INV and call(pos=50, hist=49) == INV and call(dt=2) == INV
    for t in range(6, 12):
        assert call(type=t, K=0) == 0                                         # accepted, nothing to launch
    assert call(N=0) == 0 and call(voices=0, xld=0, old=0) == 0 and call(K=0, res=None, gain=None) == 0
    assert call(K=4, N=0, rb=4, cb=4, gb=4) == 0                              # per-block rows of all three controls
    assert lib.sig_biquad_coldstart_q(9, RATE, 0, 256, 0, 100, 8, p, 1, 1, p, 1, 1, p, 8, 0, p, 8, 0, None, None) == INV   # not the q entry's type


def test_status_bit_raises_the_gain_error():
    from signals_amd import runtime
    word = runtime.StatusWord('signals.chain.ext.Peaking')
    word.tensor[0] = _native.STATUS_BAD_GAIN
    with pytest.raises(ValueError, match=r'signals.chain.ext.Peaking: filter gain must be finite'):
        runtime.check_status()
    runtime.check_status()                                                    # (polled: cleared)
    word.tensor[0] = _native.STATUS_BAD_GAIN | _native.STATUS_BAD_RESONANCE
    with pytest.raises(ValueError, match='resonance must be finite and > 0'):
        runtime.check_status()


# ---------------------------------------------------------------------------------------------- the instruction
def test_instruction_encoding():
    assert _native.VP_OPS['FilterEq'] == 18 and _native.VP_EQ_OPS == ('FilterEq',)
    assert _native.voice_program_words([('FilterEq', 0, 0, -1, -1)]) == [0xff012]         # gain and q unplugged: slot 15 each
    assert _native.voice_program_words([('FilterEq', 0, 1, 3, 2)]) == [0x23112]
    assert _native.voice_program_words([('FilterEq', 0, 1, -1, 2)]) == [0x2f112]
    assert 'FilterEq' not in _native.VP_EXT_OPS and 'FilterEq' not in _native.VP_TABLE_OPS
    # a word of the resonant family: the family arithmetic is FilterQ's
    assert _native.vp_families([('Osc', 2, 0, 0, 0), ('FilterEq', 0, 0, -1, -1)]) == ('resonant',)
    assert _native.vp_families([('OscUni', 2, 0, 0, -1), ('FilterEq', 0, 0, -1, -1)]) == ('resonant', 'unison')
    assert _native.vp_families([('FilterQ', 0, 0, 0, -1), ('FilterEq', 0, 1, -1, -1)]) == ('resonant',)


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


SRC, FE = ('Osc', 2, 0, 0, 0), ('FilterEq', 0, 0, 0, 0)


def _entries(lib):
    """every entry that takes a program: name -> call(P, nblocks, tables, unison)"""
    buf = (ctypes.c_float * 64)()

    def head(P, nblocks):
        return (ctypes.byref(P), RATE, 0, 256, nblocks, 100, 8, 2 if nblocks else 1, 0, None, 0, None, 0, 0, None, ctypes.addressof(buf), 8, None, None)
    ref = lambda x: ctypes.byref(x) if x is not None else None
    return {'sig_voice_program': lambda P, nb, t, u: lib.sig_voice_program(*head(P, nb)),
            'sig_voice_program_ex': lambda P, nb, t, u: lib.sig_voice_program_ex(*head(P, nb), ref(t)),
            'sig_voice_program_unison': lambda P, nb, t, u: lib.sig_voice_program_unison(*head(P, nb), ref(t), ref(u)),
            'sig_voice_program_mixed': lambda P, nb, t, u: lib.sig_voice_program_mixed(*head(P, nb), ref(t), ref(u))}


def test_voice_program_filtereq_argument_checks(lib):
    ex = _entries(lib)['sig_voice_program_ex']

    def run(code, nblocks=1, **kw):
        P, keep = _program(code, **kw)
        return ex(P, nblocks, None, None)
    # accepted (no blocks: nothing is launched), gain and q plugged or not, every type
    for t in ('eqbp', 'eqnotch', 'eqap', 'eqpeak', 'eqls', 'eqhs'):
        assert run([SRC, FE], types=[t], nblocks=0) == 0
        assert run([SRC, ('FilterEq', 0, 0, -1, -1)], types=[t], n_params=0, nblocks=0) == 0
        assert run([SRC, ('FilterEq', 0, 0, 1, 0)], types=[t], n_params=2, nblocks=0) == 0
    assert run([SRC, FE], types=['lp']) == INV and run([SRC, FE], types=['rlp']) == INV          # the word on another slot's type
    assert run([SRC, ('Filter', 0, 0, 0, 0)], types=['eqpeak']) == INV                           # another word on an equaliser slot
    assert run([SRC, ('FilterQ', 0, 0, 0, 0)], types=['eqpeak']) == INV
    assert run([SRC], types=['eqap']) == INV                                                     # a slot without its word
    assert run([SRC, FE, FE], types=['eqap']) == INV                                             # one word per slot
    assert run([SRC, ('FilterEq', 0, 1, 0, 0)], types=['eqap']) == INV                           # slot 1 of 1
    assert run([SRC, ('FilterEq', 0, 0, 0, 1)], types=['eqpeak']) == INV                         # q: parameter slot 1 of 1
    assert run([SRC, ('FilterEq', 0, 0, 1, 0)], types=['eqpeak']) == INV                         # gain: parameter slot 1 of 1
    assert run([SRC, ('FilterEq', 0, 0, -2, 0)], types=['eqpeak']) == INV and run([SRC, ('FilterEq', 0, 0, 0, -2)], types=['eqpeak']) == INV
    assert run([SRC, ('Filter', 0, 0, -1, 0)], types=['lp']) == INV                              # b = -1 is FilterEq's alone
    assert run([SRC, ('FilterQ', 0, 0, -1, 0)], types=['rlp']) == INV
    # an equaliser, a resonant and a plain slot in one program
    assert run([SRC, FE, ('FilterQ', 0, 1, 0, 0), ('Filter', 0, 2, 0, 0)], types=['eqhs', 'rlp', 'hp'], levels=[1, 2, 3], nblocks=0) == 0


def test_every_entry_refuses_the_word_where_it_refuses_filterq(lib):
    """sig_voice_program, _ex and _unison take FilterEq alone and refuse it together with a band, a PM carrier, a table word or a
    unison oscillator -- FilterQ's rules word for word; sig_voice_program_mixed lifts them.  An accepted program with zero blocks
    launches nothing (every call here returns before any device work: no GPU)."""
    tabs = _native.VpTablesT(); tabs.n_tables = 1; tabs.table[0] = _native.VpTable(64, 64, 1)
    uni = _native.VpUnisonT(); uni.copies = 2
    combos = {
        'band': dict(code=[SRC, FE, ('Band', 0, 1, 0, 0)], types=['eqpeak', 'bp', 'bp'], levels=[1, 2, 2]),
        'pm': dict(code=[SRC, ('OscPM', 0, 1, 0, 0), FE], n_oscs=2, types=['eqnotch']),
        'table': dict(code=[('OscTable', 0, 0, 0, -1), FE], types=['eqap']),
        'shape': dict(code=[SRC, FE, ('Shape', 0, 0, 0, -1)], types=['eqls']),
        'unison': dict(code=[('OscUni', 2, 0, 0, -1), FE], types=['eqpeak']),
        'blep': dict(code=[('OscBlep', 2, 0, 0, -1), FE], types=['eqhs']),
    }
    for name, call in _entries(lib).items():
        P, keep = _program([SRC, FE], types=['eqpeak'])
        assert call(P, 0, None, None) == 0, name                                           # alone: every entry
        for what, kw in combos.items():
            P, keep = _program(kw['code'], **{k: v for k, v in kw.items() if k != 'code'})
            if name == 'sig_voice_program_mixed':
                assert call(P, 0, tabs, uni) == 0, (name, what)                            # lifted (a block would launch: not asked here)
            else:
                assert call(P, 1, tabs, uni) == INV, (name, what)                          # (refused before any device work)
        if name != 'sig_voice_program_mixed':                                              # (... as it refuses FilterQ)
            P, keep = _program([SRC, ('FilterQ', 0, 0, 0, 0), ('Band', 0, 1, 0, 0)], types=['rlp', 'bp', 'bp'], levels=[1, 2, 2])
            assert call(P, 1, tabs, uni) == INV, name


def test_variant_names_stay_resonant_and_mixed(lib):
    assert _native.VP_VARIANTS == ('plain', 'band', 'pm', 'table', 'shape', 'resonant', 'unison', 'blep', 'mixed')
    assert _native.voice_program_variant([SRC, ('FilterEq', 0, 0, 1, 0)], 1, 2, 1, 0) == ('resonant', True)
    assert _native.voice_program_variant([('OscUni', 2, 0, 0, -1), ('FilterEq', 0, 0, -1, -1)], 1, 0, 1, 0) == ('mixed', True)
    four = [SRC, ('Save', 0, 0, 0, 0)] + [('FilterEq', 0, k, -1, 0) for k in range(4)] + [('Mix', 0, 0, 1, 0)]
    assert _native.voice_program_variant(four, 1, 2, 4, 1) == ('resonant', False)               # four filter slots: the full register file


def test_voice_program_words():
    from signals_amd.engine import _NoProgram, _VoiceProgram
    SAW = _native.OSC_KINDS['Sawtooth']
    saw = lambda: mkosc(osc.Sawtooth, row(100, 200))
    one = eq(ext.Peaking, saw(), row(500, 5000), row(0.5, 8), row(-12, 12))
    prog = _VoiceProgram(None, one, V)
    assert prog.code == [('Osc', SAW, 0, 0, 0), ('FilterEq', 0, 0, 1, 0)]
    assert _native.voice_program_words(prog.code) == [0x40, 0x01012]
    assert [(t, level) for _, t, level, _ in prog.filters] == [('eqpeak', 1)] and prog.resonant == [(one, 0)] and prog.gains == [(one, 1)]
    assert (len(prog.oscs), len(prog.params), prog.n_temps, prog.depth) == (1, 2, 0, 1) and prog.families == ('resonant',)
    assert prog.controls[prog.params[0]][0] is one.resonance and prog.controls[prog.params[1]][0] is one.gain
    assert prog.controls[prog.filters[0][0]][0] is one.cutoff

    bare = eq(ext.Peaking, saw(), row(500, 5000))                             # q and gain unplugged
    assert _VoiceProgram(None, bare, V).code[-1] == ('FilterEq', 0, 0, -1, -1) and _VoiceProgram(None, bare, V).params == []
    off = eq(ext.LowShelf, saw(), row(500, 5000), row(1, 2), row(-3, 3))
    off.gain.sig.get_state().enabled = False                                  # a disabled source: unplugged
    assert _VoiceProgram(None, off, V).code[-1] == ('FilterEq', 0, 0, -1, 0)
    notch = eq(ext.Notch, saw(), row(500, 5000), row(1, 2))                   # no gain port: b = -1
    prog = _VoiceProgram(None, notch, V)
    assert prog.code[-1] == ('FilterEq', 0, 0, -1, 0) and prog.filters[0][1] == 'eqnotch' and prog.gains == [(notch, -1)]

    # the phaser: Saw -> AllPass x 4 -> Mix with the dry voice; four filter slots, the full register file
    dry = saw()
    wet = dry
    for _ in range(4):
        wet = eq(ext.AllPass, wet, row(300, 3000), np.full((1, V), 0.7))
    mix = fx.Mix(); mix.left = wet; mix.right = dry; mix.mix = fix([[0.5]])
    prog = _VoiceProgram(None, mix, V)
    assert prog.code == [('Osc', SAW, 0, 0, 0), ('Save', 0, 0, 0, 0)] + [('FilterEq', 0, k, -1, k) for k in range(4)] + [('Mix', 0, 0, 4, 1)]
    assert [(t, level) for _, t, level, _ in prog.filters] == [('eqap', k + 1) for k in range(4)] and prog.depth == 4
    assert len(prog.params) == 5 and prog.n_temps == 1 and prog.families == ('resonant',)

    # behind a unison oscillator: a program only with mixed_programs
    uni = ext.UnisonSawtooth(); uni.hertz = fix(row(100, 200))
    top = eq(ext.HighShelf, uni, row(500, 5000), row(0.5, 2), row(-6, 6))
    with pytest.raises(_NoProgram, match='a unison oscillator with'):
        _VoiceProgram(None, top, V)
    assert _VoiceProgram.compile(None, top, V) is None
    prog = _VoiceProgram(None, top, V, mixed=True)
    assert [op for op, *_ in prog.code] == ['OscUni', 'FilterEq'] and prog.families == ('resonant', 'unison')
    bp = fx.BandPass(); bp.input = eq(ext.Notch, saw(), row(500, 900)); bp.low = fix(row(300, 400)); bp.high = fix(row(900, 1200))
    with pytest.raises(_NoProgram, match='a resonant filter and a band filter'):
        _VoiceProgram(None, bp, V)


# ---------------------------------------------------------------------------------------------- planning
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


FUSED = ('fused', 'latency', 'cascade', 'steady', 'walk', 'biquad_coldstart[', 'biquad_bus', 'biquad_coldstart_env', 'biquad_coldstart_q[')


@pytest.mark.parametrize('kind', ['peak', 'ap'])
def test_planner_routes(stubbed, kind):
    """alone, an equaliser voice is a FilterEq program by default and one kernel per node with the program off; never a
    Butterworth-only fused kernel, never the resonant low-pass / high-pass entry"""
    from signals_amd.engine import BatchRenderer
    from signals_amd.engine import _control_ports
    for kw, programmed in (({'fuse_program': False}, False), ({}, True)):
        top = eq(CLASSES[kind], mkosc(osc.Sawtooth, row(100, 200)), row(500, 5000), row(0.5, 8), row(-6, 6) if kind == 'peak' else None)
        assert _control_ports(top) == ([top.cutoff, top.resonance, top.gain] if kind == 'peak' else [top.cutoff, top.resonance])
        bus = ext.SumBus(); bus.input = top
        rec = _Recorder()
        r = BatchRenderer(bus, 1, RATE, timer=rec, **kw)
        r.render(0, 256, 3)
        r.render(768, 256, 2)
        assert not any(word in n for n in rec.names for word in FUSED), (kw, rec.names)
        if programmed:
            assert len(rec.names) == 2 and all(n.startswith('voice_program_bus[') and 'FilterEq' in n for n in rec.names), rec.names
        else:
            assert sum(n.startswith(f'biquad_coldstart_eq[eq{kind}]') for n in rec.names) == 2, rec.names
            assert any(n.startswith('osc_bank[') for n in rec.names), rec.names


def test_the_phaser_and_the_unison_voice_compile_as_stated(stubbed):
    from signals_amd.engine import BatchRenderer

    def phaser():
        dry = mkosc(osc.Sawtooth, row(100, 200))
        wet = dry
        for _ in range(4):
            wet = eq(ext.AllPass, wet, row(300, 3000), np.full((1, V), 0.7))
        mix = fx.Mix(); mix.left = wet; mix.right = dry; mix.mix = fix([[0.5]])
        return mix
    rec = _Recorder()
    BatchRenderer(phaser(), V, RATE, timer=rec).render(0, 256, 2)                # the full register file: per node by default
    assert sum(n.startswith('biquad_coldstart_eq[eqap]') for n in rec.names) == 4 and not any('voice_program' in n for n in rec.names), rec.names
    rec = _Recorder()
    BatchRenderer(phaser(), V, RATE, timer=rec, fuse_program='always').render(0, 256, 2)
    assert len(rec.names) == 1 and rec.names[0].startswith('voice_program[') and rec.names[0].count('FilterEq') == 4, rec.names

    def voice():
        uni = ext.UnisonSawtooth(); uni.hertz = fix(row(100, 200))
        return eq(ext.Peaking, uni, row(500, 5000), row(0.5, 2), row(-6, 6))
    rec = _Recorder()
    BatchRenderer(voice(), V, RATE, timer=rec).render(0, 256, 2)                 # two families: per node unless asked
    assert any(n.startswith('biquad_coldstart_eq[eqpeak]') for n in rec.names) and not any('voice_program' in n for n in rec.names), rec.names
    rec = _Recorder()
    BatchRenderer(voice(), V, RATE, timer=rec, mixed_programs=True).render(0, 256, 2)
    assert len(rec.names) == 1 and 'OscUni,FilterEq' in rec.names[0], rec.names


def test_narrow_controls_raise_like_a_narrow_cutoff(stubbed):
    from signals_amd.engine import BatchRenderer
    narrow, saw = np.array([[1.0, 2.0, 3.0]]), lambda: mkosc(osc.Sawtooth, row(100, 200))
    for kw in ({'fuse': False}, {'fuse_program': 'always'}):
        for top in (eq(ext.Peaking, saw(), row(500, 5000), row(1, 2), narrow), eq(ext.Peaking, saw(), row(500, 5000), narrow, row(-3, 3)),
                    eq(ext.Notch, saw(), 500.0 * narrow, row(1, 2))):
            with pytest.raises(IndexError, match='index 3 is out of bounds for axis 1 with size 3'):
                BatchRenderer(top, V, RATE, **kw).render(0, 256, 2)


def test_an_equaliser_in_a_control_path_is_refused_with_its_reason():
    from signals_amd.engine import NotBatchable, _ControlProgram
    f = eq(ext.Peaking, mkosc(osc.Sine, [[3.0]]), np.array([[10.0]]), np.array([[2.0]]), np.array([[6.0]]))
    with pytest.raises(NotBatchable, match='resonant filter has no block-rate program'):
        _ControlProgram((f,), 4, channels=1)


# ---------------------------------------------------------------------------------------------- specialised build
def test_flags_of_an_equaliser_program():
    code = [('Osc', 2, 0, 0, 0), ('FilterEq', 0, 0, 1, 0)]
    f = specialise.flags(code, 1, 2, 1, 0, 2, 2)
    assert {'-DSIG_VP_STATIC_CODE={0x40,0x1012}', '-DSIG_VP_S_RES=1', '-DSIG_VP_S_EQ=1', '-DSIG_VP_S_NF=1', '-DSIG_VP_S_NP=2'} <= set(f)
    assert not any('SIG_VP_S_TAB' in x or 'SIG_VP_S_MIXED' in x for x in f)
    for other in ([('Osc', 2, 0, 0, 0), ('Filter', 0, 0, 0, 0)], [('Osc', 2, 0, 0, 0), ('FilterQ', 0, 0, 0, 0)],
                  [('OscUni', 2, 0, 0, -1), ('FilterQ', 0, 0, 0, -1)], [('OscTable', 0, 0, 0, -1), ('Shape', 0, 0, 0, -1)]):
        assert not any('SIG_VP_S_EQ' in x for x in specialise.flags(other, 1, 1, 1, 0, 2, 2))     # only with the word
    assert specialise.flags([('Osc', 2, 0, 0, 0), ('FilterQ', 0, 0, 0, 0)], 1, 1, 1, 0, 2, 2)[-1] == '-DSIG_VP_S_RES=1'   # (the list it always had)
    mixed = specialise.flags([('OscUni', 2, 0, 0, -1), ('FilterEq', 0, 0, -1, -1)], 1, 0, 1, 0, 2, 2)
    assert {'-DSIG_VP_S_RES=1', '-DSIG_VP_S_EQ=1', '-DSIG_VP_S_UNI=1', '-DSIG_VP_S_MIXED=1'} <= set(mixed)


@pytest.mark.skipif(specialise.hipcc() is None, reason='no hipcc in this environment')
def test_the_specialised_equaliser_program_builds(tmp_path, monkeypatch):
    monkeypatch.setattr(specialise, 'CACHE', tmp_path)
    code = [('Osc', 2, 0, 0, 0), ('FilterEq', 0, 0, 1, 0), ('FilterEq', 0, 1, -1, -1), ('Filter', 0, 2, 0, 0)]
    image = specialise.build(code, 1, 2, 3, 0, 2, 2)
    assert b'sig_vp_specialised' in image and b'sig_vp_specialised_info' in image
