"""The hard-sync oscillators without a GPU: the node API of ext.SyncOsc (a BlepOsc with a `ratio` port), name resolution and the
.sigs loader, the exports and argument checks of sig_osc_bank_sync and the OscSync word, the programs the engine compiles for the
node, the specialised build of such a program, and the numpy restatement (tests/sync_reference.py): against a direct loop, against
tests/blep_reference.py at ratio <= 1, against the naive hard-synced waveform outside the windows, its special values, its
continuity, and the aliasing it removes."""
import ctypes
import math
import pathlib
import types

import numpy as np
import pytest

from signals_amd import SignalFlags, _native, specialise
from signals_amd.chain import ext, fixed, fx

import blep_reference as BR
import sync_reference as SR

ROOT = pathlib.Path(__file__).resolve().parent.parent
INV = 1     # hipErrorInvalidValue
KINDS = ('Sawtooth', 'Square')
NODES = {kind: getattr(ext, 'Sync' + kind) for kind in KINDS}                  # (the module needs the feature: nothing here passes without it)
SAW, SQUARE = 2, 1
CLEAR_RATIOS = (1.5, 2.0, 2.75, 3.25)                                          # at d = 1 / 64 no interior edge's window is cut by the reset


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


def sync_node(hertz, ratio=None, copies=None, spread=None, kind='Sawtooth'):
    n = NODES[kind]()
    if copies is not None:
        n.get_state().copies = copies
    n.hertz = fix(hertz)
    if ratio is not None:
        n.ratio = ratio if not isinstance(ratio, (list, np.ndarray)) else fix(ratio)
    if spread is not None:
        n.spread = fix(spread)
    return n


# ---------------------------------------------------------------------------------------------- the node
def test_class_hierarchy_and_ports():
    assert issubclass(ext.SyncOsc, ext.BlepOsc) and issubclass(ext.SyncOsc, ext.UnisonOsc)
    assert not hasattr(ext, 'SyncSine') and not hasattr(ext, 'SyncTriangle')
    for kind in KINDS:
        cls = NODES[kind]
        assert issubclass(cls, ext.SyncOsc) and cls.kind() == kind and cls.bandlimited() is True
        assert cls.port_names() == ['hertz', 'phase', 'ratio', 'spread']
        assert cls.flags() & SignalFlags.GENERATOR
        assert 'copies' in cls().state_attrs()
        c = cls().get_state().copies
        assert c.shape == (1, 2) and not c.any()                              # BlepOsc's default: one clean copy
    for kind in ('Square', 'Sawtooth', 'Triangle'):                           # the parents keep their ports and their route
        assert getattr(ext, 'Blep' + kind).port_names() == ['hertz', 'phase', 'spread']
        assert not issubclass(getattr(ext, 'Blep' + kind), ext.SyncOsc)
    with pytest.raises(TypeError):
        ext.SyncOsc()                                                         # abstract: a kind is a subclass
    assert sync_node(np.full((1, 6), 220.0), [[2.5]]).channels == 6
    doc = ext.SyncOsc.__doc__
    for line in ('R  = max(ratio[v], 1.0)', 'm  = mod(t, 1);  s = m * R;  k = floor(s);  f = s - k', 'ds = min(d * R, 0.5)',
                 'g  = R - (ceil(R) - 1)', 'Sawtooth: w = (2f - 1) - estep(f, k >= 1, k + 1 < R) - g * step(m)',
                 'estep(fb, kb >= 1, kb + 0.5 < R)', "trailing window is cut at", 'The formula is the definition there too',
                 'no longer band-limits', '-5 dB', 'Out of scope'):
        assert line in doc, line
    for line in ('s = m * R;  k = floor(s);  f = s - k', 'ds = min(d * R, 0.5)', 'g  = R - (ceil(R) - 1)',
                 'Sawtooth: w = (2f - 1) - estep(f, k >= 1, k + 1 < R) - g * step(m, d)', 'sb = s + 0.5;  kb = floor(sb);  fb = sb - kb'):
        assert line in SR.__doc__, line                                       # the restatement states the same definition


def test_class_resolves_by_qualified_name_and_loads_from_a_patch():
    from signals_amd.chain import discovery, sigs
    from signals_amd.chain.driver import load_signal
    assert load_signal('signals_amd.chain.ext.SyncSawtooth') is ext.SyncSawtooth
    assert load_signal('signals.chain.ext.SyncSquare') is ext.SyncSquare
    assert discovery.load_signal('signals.chain.ext.SyncSawtooth') is ext.SyncSawtooth
    p = sigs.loads('+ 1a signals.chain.fixed.Fixed value=[[220.0]]\n+ 1b signals.chain.fixed.Fixed value=[[2.5]]\n'
                   '+ 2a signals.chain.ext.SyncSawtooth copies=[[0,0],[1,0],[-1,0]]\n+ 2b signals.chain.ext.SyncSquare\n'
                   '> 1a 2a.hertz\n> 1b 2a.ratio\n> 1a 2b.hertz')
    node = p['2a']
    assert isinstance(node, ext.SyncSawtooth) and node.hertz.sig is p['1a'] and node.ratio.sig is p['1b']
    assert node.get_state().copies.shape == (3, 2) and p['2b'].get_state().copies.shape == (1, 2) and p['2b'].ratio.sig is None


# ---------------------------------------------------------------------------------------------- C ABI
def test_entry_point_and_word_are_declared(lib):
    assert 'sig_osc_bank_sync' in _native.EXPORTS
    raw = ctypes.CDLL(str(_native.LIB_PATH))
    assert raw.sig_osc_bank_sync is not None
    header = (ROOT / 'include' / 'signals_amd.h').read_text()
    assert 'int sig_osc_bank_sync(' in header and 'SIG_VP_OSCSYNC = 19' in header and '   OSCSYNC acc =' in header
    assert _native.VP_OPS['OscSync'] == 19 and _native.VP_SYNC_OPS == ('OscSync',) and 'OscSync' not in _native.VP_EXT_OPS
    assert _native.VP_BLEP_OPS == ('OscBlep',) and _native.VP_UNI_OPS == ('OscUni',)       # the earlier words' lists stay
    assert _native.voice_program_words([('OscSync', SAW, 0, -1, -1)]) == [0xff053]         # no ratio, no spread: slot 15 each
    assert _native.voice_program_words([('OscSync', SQUARE, 1, 2, 0)]) == [0x02133]
    assert _native.vp_families([('OscSync', SAW, 0, 0, -1), ('Filter', 0, 0, 0, 0)]) == ('unison',)
    assert _native.vp_families([('OscSync', SAW, 0, 0, -1), ('FilterQ', 0, 0, 0, -1)]) == ('resonant', 'unison')


def test_osc_bank_sync_argument_errors_do_not_reach_the_device(lib):
    p = 64                                                                    # (never dereferenced: every call fails its checks)
    host = (ctypes.c_double * 16)()
    args = dict(kind=2, position=0, step=1, rate=48000, rows=256, voices=8, rpp=0, hertz=p, hs=1, hrs=0, phase=None, ps=0, prs=0,
                spread=p, ss=1, srs=0, ratio=p, rs=1, rrs=0, copies=7, detune=host, offsets=host, out=p, odt=0, old=8, stream=None)

    def call(**over):
        a = dict(args, **over)
        return lib.sig_osc_bank_sync(*(a[k] for k in args))
    assert call(kind=0) == INV and call(kind=3) == INV                        # Sine, Triangle: their reset changes the slope
    assert call(kind=4) == INV and call(kind=-1) == INV
    assert call(rs=2) == INV and call(rs=-1) == INV and call(rrs=-1) == INV   # the ratio's strides, checked like the spread's
    assert call(ss=2) == INV and call(srs=-1) == INV and call(hs=2) == INV and call(prs=-1) == INV
    assert call(detune=None) == INV and call(offsets=None) == INV
    assert call(copies=17) == INV and call(copies=0) == INV and call(copies=-1) == INV
    assert call(old=4) == INV and call(hertz=None) == INV and call(out=None) == INV
    assert call(odt=2) == INV and call(rate=0) == INV and call(position=-1) == INV and call(step=0) == INV and call(rpp=-1) == INV
    for kind in (1, 2):
        assert call(kind=kind, rows=0) == 0                                   # accepted, nothing to launch
    assert call(voices=0, old=0) == 0 and call(rows=0, copies=1) == 0 and call(rows=0, copies=16) == 0
    assert call(rows=0, ratio=None) == 0 and call(rows=0, spread=None, phase=None) == 0    # unplugged
    assert call(rows=0, rs=0) == 0


def _program(code, n_oscs=1, n_params=1, types=()):
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


def test_voice_program_refuses_bad_sync_programs(lib):
    buf = (ctypes.c_float * 64)()

    def copies(n):
        u = _native.VpUnisonT()
        u.copies = n
        return u

    def run(code, uni, nblocks=1, control_rows=2, entry='sig_voice_program_unison', **kw):
        P, keep = _program(code, **kw)
        return getattr(lib, entry)(ctypes.byref(P), 48000, 0, 256, nblocks, 100, 8, control_rows, 0, None, 0, None, 0, 0, None,
                                   ctypes.addressof(buf), 8, None, None, None, ctypes.byref(uni) if uni is not None else None)
    one = copies(1)
    word = ('OscSync', SAW, 0, 0, -1)
    assert run([('OscSync', 0, 0, 0, -1)], one) == INV                        # Sine
    assert run([('OscSync', 3, 0, 0, -1)], one) == INV                        # Triangle
    assert run([('OscSync', 4, 0, 0, -1)], one) == INV
    assert run([('OscSync', SAW, 0, 1, -1)], one) == INV                      # ratio: parameter slot 1 of 1
    assert run([('OscSync', SAW, 0, -2, -1)], one) == INV and run([('OscSync', SAW, 0, 16, -1)], one) == INV
    assert run([('OscSync', SAW, 0, -1, 1)], one) == INV                      # spread: parameter slot 1 of 1
    assert run([('OscSync', SAW, 1, 0, -1)], one) == INV                      # oscillator slot 1 of 1
    assert run([word], None) == INV                                           # the word without its copies
    assert run([word], copies(17)) == INV and run([word], copies(0)) == INV
    assert run([('OscBlep', SAW, 0, -1, -1)], one) == INV                     # only OscSync's b may be -1
    # the unison family's exclusions, and the one of its own: never with FilterEq, through any entry
    assert run([word, ('FilterQ', 0, 0, 0, -1)], one, types=['rlp']) == INV
    assert run([word, ('Band', 0, 0, 0, 0)], one, types=['bp', 'bp']) == INV
    assert run([word, ('FilterEq', 0, 0, -1, -1)], one, types=['eqpeak'], entry='sig_voice_program_mixed') == INV
    assert run([('OscBlep', SAW, 0, 0, -1), ('FilterEq', 0, 0, -1, -1)], one, types=['eqpeak'], nblocks=0, control_rows=1,
               entry='sig_voice_program_mixed') == 0                          # (what the equaliser word keeps taking)
    # accepted, nothing to launch: no blocks
    for kind in (SQUARE, SAW):
        for b in (-1, 0):
            assert run([('OscSync', kind, 0, b, -1)], one, nblocks=0, control_rows=1) == 0
    assert run([word, ('Filter', 0, 0, 0, 0)], copies(7), nblocks=0, control_rows=1, types=['lp']) == 0
    assert run([word, ('Save', 0, 0, 0, 0), ('OscBlep', 3, 1, 0, -1), ('Mul', 0, 0, 0, 0)], one, nblocks=0, control_rows=1, n_oscs=2) == 0
    assert run([word, ('FilterQ', 0, 0, 0, -1)], one, nblocks=0, control_rows=1, types=['rlp'], entry='sig_voice_program_mixed') == 0
    assert run([('OscSync', 3, 0, 0, -1), ('FilterQ', 0, 0, 0, -1)], one, types=['rlp'], entry='sig_voice_program_mixed') == INV


def test_the_variant_of_a_program_with_the_word(lib):
    """sig_voice_program_variant answers for the word: the band-limited family, or mixed with a resonant filter (the launch then picks
    the sync kernel set of that variant)"""
    fam, small = ctypes.c_int32(-1), ctypes.c_int32(-1)
    for code, kw, want in (([('OscSync', SAW, 0, 0, -1)], {}, 7), ([('OscSync', SQUARE, 0, -1, -1), ('Filter', 0, 0, 0, 0)], dict(types=['lp']), 7),
                           ([('OscSync', SAW, 0, 0, -1), ('FilterQ', 0, 0, 0, -1)], dict(types=['rlp']), 8),
                           ([('OscBlep', SAW, 0, 0, -1)], {}, 7), ([('OscUni', SAW, 0, 0, -1)], {}, 6)):
        P, keep = _program(code, **kw)
        assert lib.sig_voice_program_variant(ctypes.byref(P), ctypes.byref(fam), ctypes.byref(small)) == 0
        assert (fam.value, small.value) == (want, 1), code


# ---------------------------------------------------------------------------------------------- planning
def test_voice_programs():
    from signals_amd.engine import _KNOWN_TYPES, _VoiceProgram, _control_ports, _is_pure
    V = 8
    row = lambda lo, hi: np.linspace(lo, hi, V).reshape(1, V)
    bare = sync_node(row(220, 440))
    assert any(issubclass(ext.SyncOsc, t) for t in _KNOWN_TYPES if isinstance(t, type))
    assert _control_ports(bare) == [bare.hertz, bare.phase, bare.spread, bare.ratio] and _is_pure(bare, {})
    prog = _VoiceProgram.compile(None, bare, V, min_nodes=1)
    assert prog.describe() == 'OscSync' and prog.code == [('OscSync', SAW, 0, -1, -1)] and prog.unison is bare      # ratio unplugged: b = -1
    swept = sync_node(row(220, 440), row(1.0, 4.0), spread=[[0.5]])
    lp = fx.LowPass(); lp.input = swept; lp.cutoff = fix(row(500, 5000))
    bus = ext.SumBus(); bus.input = lp
    prog = _VoiceProgram.compile(None, lp, V)
    word = prog.code[0]
    assert prog.code == [('OscSync', SAW, 0, word[3], word[4]), ('Filter', 0, 0, 0, 0)] and prog.depth == 1 and prog.families == ('unison',)
    assert {word[3], word[4]} == {0, 1} and len(prog.params) == 2             # the ratio and the spread: a parameter register each
    assert prog.controls[prog.params[word[3]]][0] is swept.ratio and prog.controls[prog.params[word[4]]][0] is swept.spread
    small = types.SimpleNamespace(owner=types.SimpleNamespace(specialise=False), N=256, _pure={})
    assert _VoiceProgram(small, lp, V).worthwhile()                           # the small-file rule, as for OscUni
    # the parents keep their words
    b = ext.BlepSawtooth(); b.hertz = fix(row(220, 440))
    assert _VoiceProgram.compile(None, b, V, min_nodes=1).code == [('OscBlep', SAW, 0, 0, -1)]
    # behind a resonant filter: refused unless mixed, with or without a trailing Shaper
    rl = ext.ResonantLowPass(); rl.input = sync_node(row(220, 440), [[2.5]]); rl.cutoff = fix(row(500, 5000)); rl.resonance = fix([[2.0]])
    assert _VoiceProgram.compile(None, rl, V) is None
    with pytest.raises(Exception, match='no interpreter variant has both'):
        _VoiceProgram(None, rl, V)
    prog = _VoiceProgram(None, rl, V, mixed=True)
    assert [op for op, *_ in prog.code] == ['OscSync', 'FilterQ'] and prog.families == ('resonant', 'unison')
    sh = ext.Shaper(); sh.input = rl
    assert [op for op, *_ in _VoiceProgram(None, sh, V, mixed=True).code] == ['OscSync', 'FilterQ', 'Shape']
    # with an equaliser biquad: one kernel per node, mixed or not, with the reason
    pk = ext.Peaking(); pk.input = sync_node(row(220, 440), [[2.5]]); pk.cutoff = fix(row(500, 5000))
    for mixed in (False, True):
        with pytest.raises(Exception, match='a hard-sync oscillator and an equaliser filter'):
            _VoiceProgram(None, pk, V, mixed=mixed)
        assert _VoiceProgram.compile(None, pk, V, mixed=mixed) is None


def test_the_node_in_a_control_path_is_refused_with_its_reason():
    from signals_amd.engine import NotBatchable, _ControlProgram
    with pytest.raises(NotBatchable, match='SyncSquare in a control path: a unison oscillator has no block-rate program'):
        _ControlProgram((sync_node([[3.0]], [[2.0]], kind='Square'),), 4)


# ---------------------------------------------------------------------------------------------- specialised build
def test_flags_of_a_program_with_the_word():
    code = [('OscSync', SAW, 0, 0, -1), ('Filter', 0, 0, 0, 0)]
    f = specialise.flags(code, 1, 1, 1, 0, 2, 2)
    assert f[-2:] == ['-DSIG_VP_S_UNI=1', '-DSIG_VP_S_SYNC=1']                # the copies parameter, and the handler
    assert {'-DSIG_VP_STATIC_CODE={0xf0053,0x1}', '-DSIG_VP_S_NO=1', '-DSIG_VP_S_NF=1', '-DSIG_VP_S_EXT=0'} <= set(f)
    assert not any(x in ' '.join(f) for x in ('S_TAB', 'S_RES', 'S_MIXED', 'S_BLEP', 'S_EQ'))
    for other in ([('OscBlep', SAW, 0, 0, -1), ('Filter', 0, 0, 0, 0)], [('OscUni', SAW, 0, 0, -1)], [('Osc', 2, 0, 0, 0), ('Filter', 0, 0, 0, 0)],
                  [('Osc', 0, 0, 0, 0), ('FilterEq', 0, 0, -1, -1)]):
        assert not any('SYNC' in x for x in specialise.flags(other, 1, 0, 1, 0, 2, 2)), other       # programs without the word: the list they had
    mixed = specialise.flags([('OscSync', SAW, 0, 0, -1), ('FilterQ', 0, 0, 0, -1)], 1, 1, 1, 0, 2, 2)
    assert mixed[-4:] == ['-DSIG_VP_S_RES=1', '-DSIG_VP_S_UNI=1', '-DSIG_VP_S_SYNC=1', '-DSIG_VP_S_MIXED=1']
    names = specialise.flags.__code__.co_varnames
    assert 'copies' not in names and 'ratio' not in names                     # one image serves every copies array and every ratio


@pytest.mark.skipif(specialise.hipcc() is None, reason='no hipcc in this environment')
def test_the_specialised_sync_program_builds(tmp_path, monkeypatch):
    monkeypatch.setattr(specialise, 'CACHE', tmp_path)
    image = specialise.build([('OscSync', SAW, 0, 0, 1), ('Filter', 0, 0, 0, 0), ('Gain', 0, 1, 0, 0)], 1, 2, 1, 0, 2, 2)
    assert b'sig_vp_specialised' in image and b'sig_vp_specialised_info' in image
    image = specialise.build([('OscSync', SQUARE, 0, 0, -1), ('FilterQ', 0, 0, 0, 1), ('Shape', 0, 0, 0, -1)], 1, 2, 1, 0, 2, 2)
    assert b'sig_vp_specialised' in image                                     # the mixed patch: sync -> resonant -> shaper


# ---------------------------------------------------------------------------------------------- the restatement
def _step(m, d):
    if m < d:
        x = m / d
        return 2.0 * x - x * x - 1.0
    if m > 1.0 - d:
        y = (m - 1.0) / d
        return y * y + 2.0 * y + 1.0
    return 0.0


def _estep(p, ds, lo_ok, hi_ok):
    if p < ds and lo_ok:
        x = p / ds
        return 2.0 * x - x * x - 1.0
    if p > 1.0 - ds and hi_ok:
        y = (p - 1.0) / ds
        return y * y + 2.0 * y + 1.0
    return 0.0


def _direct(kind, t, d, ratio):
    """the definition for one sample, branch by branch in Python floats"""
    R = max(ratio, 1.0)
    m = float(np.mod(np.float64(t), 1.0))
    s = m * R
    k = math.floor(s)
    f = s - k
    ds = min(d * R, 0.5)
    g = R - (math.ceil(R) - 1.0)
    if kind == 'Sawtooth':
        return (2.0 * f - 1.0) - _estep(f, ds, k >= 1, k + 1 < R) - g * _step(m, d)
    sb = s + 0.5
    kb = math.floor(sb)
    fb = sb - kb
    return (1.0 if f < 0.5 else -1.0) + _estep(f, ds, k >= 1, k + 1 < R) - _estep(fb, ds, kb >= 1, kb + 0.5 < R) + (0.0 if g <= 0.5 else 1.0) * _step(m, d)


@pytest.mark.parametrize('kind', KINDS)
def test_reference_restatement_against_a_direct_loop(kind):
    rng = np.random.default_rng(4)
    copies = np.stack([rng.uniform(-0.12, 0.12, 5), rng.uniform(0, 1, 5)], axis=1)
    hz = np.array([[440.0, -2000.0, 13000.0, 30000.0, 0.0, 1e-3, 750.0, 440.0, 1234.5]])     # 750 = rate / 64: exact edges at phase 0
    ph, sp = np.array([[0.3, 0.7, 0.1, 0.9, 0.25, 0.5, 0.0, 0.0, 0.6]]), rng.uniform(0, 1, (1, 9))
    ra = np.array([[1.5, 2.75, 3.25, 7.77, 2.0, 5.5, 2.0, 0.25, 4.0]])
    got = SR.sync(kind, copies, 50, 70, hz, ph, sp, ra)
    assert got.shape == (70, 9) and got.dtype == np.float64 and np.isfinite(got).all()
    worst = 0.0
    for r in range(70):
        for v in range(9):
            s = None
            for d, p in copies.tolist():
                h = hz[0, v] * (1.0 + sp[0, v] * d)
                t = float(np.float64(50 + r) / 48000 * h + (ph[0, v] + p))
                w = _direct(kind, t, min(abs(h) / 48000, 0.5), ra[0, v])
                s = w if s is None else s + w
            worst = max(worst, abs(got[r, v] - s / 5))
    assert worst == 0.0, worst                                                # (the same operations in the same order)
    for ratio in CLEAR_RATIOS:                                                # one copy at rate / 64, phase 0: the reset and every edge are hit exactly
        one = SR.sync(kind, [[0, 0]], 0, 256, [[750.0]], ratio=[[ratio]])
        for r in range(256):
            assert one[r, 0] == _direct(kind, float(np.float64(r) / 48000 * 750.0 + 0.0), 750.0 / 48000, ratio), (ratio, r)
    # landmarks at 1 kHz and ratio 2: zero at the reset and at the slave's interior edge, the Sawtooth's ramp between them
    at = [float(SR.sync_wave(kind, np.float64(t), np.float64(1000 / 48000), 2.0)) for t in (0.0, 0.125, 0.25, 0.5, 0.75)]
    assert at[0] == 0.0 and at[3] == 0.0, at
    assert (at[1], at[2], at[4]) == ((-0.5, 0.0, 0.0) if kind == 'Sawtooth' else (1.0, 0.0, 0.0)), at


@pytest.mark.parametrize('ratio', [0.0, 1.0, 0.5, -3.0])
def test_at_ratio_up_to_one_it_is_the_band_limited_oscillator(ratio):
    """Square directly, Sawtooth at phase + 0.5, within 1e-12: the phases differ by a rounding of t, which 1 / d amplifies"""
    rng = np.random.default_rng(6)
    hz, ph = rng.uniform(55, 12000, (1, 64)), rng.uniform(0, 1, (1, 64))
    hz[0, :3] = (750.0, -440.0, 20000.0)
    copies = np.array([[0.0, 0.0], [0.01, 0.3], [-0.02, 0.7]])
    for pos in (0, 100000):
        sq = SR.sync('Square', copies, pos, 512, hz, ph, [[0.5]], [[ratio]])
        assert np.abs(sq - BR.blep('Square', copies, pos, 512, hz, ph, [[0.5]])).max() <= 1e-12
        saw = SR.sync('Sawtooth', copies, pos, 512, hz, ph, [[0.5]], [[ratio]])
        assert np.abs(saw - BR.blep('Sawtooth', copies, pos, 512, hz, ph + 0.5, [[0.5]])).max() <= 1e-12
    assert np.array_equal(SR.sync('Sawtooth', copies, 0, 256, hz, ph, ratio=[[ratio]]), SR.sync('Sawtooth', copies, 0, 256, hz, ph))   # unplugged: zeros


@pytest.mark.parametrize('kind', KINDS)
def test_rows_outside_every_window_are_the_naive_waveform(kind):
    rng = np.random.default_rng(5)
    hz, ph, ra = rng.uniform(55, 3000, (1, 64)), rng.uniform(0, 1, (1, 64)), rng.uniform(1.0, 6.0, (1, 64))
    from oracle import chain_ref as R
    for pos in (0, 48000 * 3600):
        n = R.frame_range(pos, 512)
        got = SR.sync(kind, [[0, 0]], pos, 512, hz, ph, ratio=ra)
        naive = SR.sync(kind, [[0, 0]], pos, 512, hz, ph, ratio=ra, naive=True)
        t = n / 48000 * hz + ph
        inside = SR.in_window(kind, t, BR.increment(hz, 48000), ra)
        assert 0.01 < inside.mean() < 0.8                                     # both sides are exercised
        assert np.array_equal(got[~inside], naive[~inside])                   # bit for bit
        assert not np.array_equal(got[inside], naive[inside])
        # ... and the naive waveform is osc.py's closed form of the slave's phase: 2 f - 1, sign(0.5 - f) without the isolated zero
        f = np.mod(t, 1.0) * ra
        f = f - np.floor(f)
        assert np.array_equal(naive, 2.0 * f - 1.0 if kind == 'Sawtooth' else np.where(f < 0.5, 1.0, -1.0))


@pytest.mark.parametrize('kind', KINDS)
def test_special_values(kind):
    t = np.linspace(-1, 1, 4001)
    for bad in (np.nan, np.inf, -np.inf):
        assert np.isnan(SR.sync_wave(kind, t, 0.01, bad)).all(), bad          # a ratio that is not finite: NaN (not R = 1, not R = inf)
    rows = SR.sync(kind, [[0, 0]], 0, 64, [[440.0, 440.0, 440.0]], ratio=[[2.0, np.nan, np.inf]])
    assert np.isfinite(rows[:, 0]).all() and np.isnan(rows[:, 1:]).all()      # per voice
    assert np.isnan(SR.sync_wave(kind, np.array([np.nan, np.inf, -np.inf]), 0.01, 2.5)).all()       # a non-finite t
    zero = SR.sync_wave(kind, t, 0.0, 2.5)                                    # d = 0: ds = 0, no window, the naive value
    assert np.isfinite(zero).all() and np.array_equal(zero, SR.sync_wave(kind, t, 0.0, 2.5, naive=True))
    assert np.array_equal(SR.sync(kind, [[0, 0]], 0, 64, [[0.0]], [[0.3]], ratio=[[2.5]]), SR.sync(kind, [[0, 0]], 5, 64, [[0.0]], [[0.3]], ratio=[[2.5]]))   # 0 Hz: a constant
    from oracle import chain_ref as R
    hz = np.array([[440.0, 2000.0, 13000.0]])
    assert np.array_equal(SR.sync(kind, [[0, 0]], 0, 256, -hz, [[0.2]], ratio=[[2.5]]),
                          SR.sync_wave(kind, R.frame_range(0, 256) / 48000 * -hz + 0.2, hz / 48000, 2.5))     # hertz < 0: |h|
    for ratio in (0.0, 0.5, 1.0, -7.0):                                       # ratio < 1: R = 1
        assert np.array_equal(SR.sync_wave(kind, t, 0.01, ratio), SR.sync_wave(kind, t, 0.01, 1.0)), ratio
    assert np.abs(SR.sync_wave(kind, t, 0.01, 3.3)).max() <= 1.0 + 1e-12


@pytest.mark.parametrize('ratio', CLEAR_RATIOS)
@pytest.mark.parametrize('kind', KINDS)
def test_the_restatement_is_continuous(kind, ratio):
    """d = 1 / 64 and the ratios whose last interior edge keeps clear of the reset.  Phases one ulp apart across every interior edge
    and across the reset, taken in [1, 2) where an ulp of t is 2^-52 and m = t - 1 is exact: the slave's phase f moves by R ulp and by
    one rounding of s = m R (at most ulp(R) <= R 2^-52), and the waveform's slope in f is at most 2 + 2 / ds (the naive slope plus the
    residual's); the evaluation's own roundings add a few ulp of a value <= 2.  So a move is bounded by (2 + 2 / ds) R 2^-51 + 2^-50,
    where a discontinuity would move it by its height.  Then a fine sweep over two cycles under the same slope."""
    d = 1.0 / 64.0
    ds = min(d * ratio, 0.5)
    slope = (2.0 + 2.0 / ds) * ratio
    edges = [1.0] + [1.0 + j / ratio for j in range(1, math.ceil(ratio))] + [2.0]
    if kind == 'Square':
        edges += [1.0 + (j + 0.5) / ratio for j in range(0, math.ceil(ratio)) if (j + 0.5) / ratio < 1.0]
    for e in edges:
        ts = [np.float64(e)]
        for _ in range(3):
            ts.insert(0, np.nextafter(ts[0], -np.inf)); ts.append(np.nextafter(ts[-1], np.inf))
        w = SR.sync_wave(kind, np.array(ts), d, ratio)
        move = float(np.abs(np.diff(w)).max())
        assert move <= slope * 2.0 ** -51 + 2.0 ** -50, (kind, ratio, e, move)
    t = np.linspace(-1.0, 1.0, 1_000_001)
    w = SR.sync_wave(kind, t, d, ratio)
    assert np.isfinite(w).all() and np.abs(w).max() <= 1.0 + 1e-12
    jump = float(np.abs(np.diff(w)).max())
    assert jump < slope * (t[1] - t[0]) * (1.0 + 1e-6), (kind, ratio, jump)
    assert float(np.abs(np.diff(SR.sync_wave(kind, t, d, ratio, naive=True))).max()) > 0.4       # (the naive edges do jump)


def test_the_cut_window_is_the_one_discontinuity():
    """ratio 2.02 at d = 1 / 64: g = 0.02 < ds = 0.0316, the last interior edge's trailing window is cut at the reset -- the formula is
    the definition there too, and the jump is what the window had left, under the residual's height of 1"""
    d, ratio = 1.0 / 64.0, 2.02
    t = np.linspace(0.0, 1.0, 1_000_001)
    w = SR.sync_wave('Sawtooth', t, d, ratio)
    jump = np.abs(np.diff(w))
    at = int(np.argmax(jump))
    assert 0.05 < jump[at] < 1.0 and (at <= 1 or at >= t.shape[0] - 3), (jump[at], at)    # at the reset, nowhere else
    rest = np.delete(jump, at)
    assert rest.max() < (2.0 + 2.0 / (d * ratio)) * ratio * (t[1] - t[0]) * (1.0 + 1e-6)


# required margin below the naive hard-synced waveform's alias / harmonic ratio, naive ratio, band-limited ratio (dB): the ratios are
# what the definition gives in numpy's float64 (recorded to one decimal, re-derived by the test); the margin is the requirement
ALIAS = {('Sawtooth', 1.5): (-12.6, -28.0), ('Sawtooth', 2.0): (-9.9, -24.1), ('Sawtooth', 2.7): (-8.8, -23.6), ('Sawtooth', 3.3): (-8.7, -25.7),
         ('Square', 1.5): (-15.6, -30.8), ('Square', 2.0): (-11.4, -24.6), ('Square', 2.7): (-10.1, -25.0), ('Square', 3.3): (-10.0, -25.6)}
MARGIN_DB = 12.0


@pytest.mark.parametrize('kind,ratio', sorted(ALIAS))
def test_the_aliasing_it_removes(kind, ratio):
    """the point of the feature: 4096 frames at hertz = 48000 * 37 / 1024 and phase 0.1234 (148 whole master cycles: the master sets
    the period, so every harmonic and every alias falls on a bin of its own), an unwindowed rfft"""
    hz, ph = np.array([[48000 * 37 / 1024]]), np.array([[0.1234]])
    x = SR.sync(kind, [[0, 0]], 0, 4096, hz, ph, ratio=[[ratio]])[:, 0]
    naive = SR.sync(kind, [[0, 0]], 0, 4096, hz, ph, ratio=[[ratio]], naive=True)[:, 0]
    naive_db, clean_db = ALIAS[kind, ratio]
    got_naive, got_clean = SR.alias_ratio_db(naive), SR.alias_ratio_db(x)
    print('alias / harmonic', kind, ratio, 'naive', got_naive, 'band-limited', got_clean)
    assert got_clean <= got_naive - MARGIN_DB, (kind, ratio, got_naive, got_clean)
    assert abs(got_naive - naive_db) < 0.06 and abs(got_clean - clean_db) < 0.06, (kind, ratio, got_naive, got_clean)   # the recorded figures
    assert np.abs(x).max() <= 1.0 + 1e-12


def test_reference_renders_blocks_with_per_block_rows_and_as_an_oracle_node():
    from oracle import chain_ref as R
    copies = np.array([[0.0, 0.0], [0.01, 0.5]])
    hertz = np.array([[100.0, 200.0], [3000.0, 4000.0]])
    ratio = np.array([[1.5, 2.5], [3.5, 1.0]])
    got = SR.sync('Sawtooth', copies, 50, 4, hertz, phase=[[0.25]], spread=[[0.5]], ratio=ratio, blocks=2)
    n = R.frame_range(50, 8)
    want = np.concatenate([SR.sync_sum('Sawtooth', n[:4], 48000, hertz[:1], 0.25, 0.5, ratio[:1], copies),
                           SR.sync_sum('Sawtooth', n[4:], 48000, hertz[1:], 0.25, 0.5, ratio[1:], copies)])
    assert np.array_equal(got, want) and abs(got).max() <= 1.0
    node = SR.SyncOsc('Sawtooth', copies, R.Fixed(hertz[:1]), R.Fixed([[0.25]]), R.Fixed([[0.5]]), R.Fixed(ratio[:1]))
    assert np.array_equal(R.render(node, 50, 4, 2), want[:4])
    bare = SR.SyncOsc('Square', copies, R.Fixed(hertz[:1]))                   # unplugged ratio: zeros, the band-limited Square
    assert np.abs(R.render(bare, 50, 64, 2) - BR.blep('Square', copies, 50, 64, hertz[:1])).max() <= 1e-12
