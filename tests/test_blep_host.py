"""The band-limited oscillators without a GPU: the node API of ext.BlepOsc (a UnisonOsc: its ports, state and validator), name
resolution and the .sigs loader, the exports and argument checks of sig_osc_bank_blep and the OscBlep word, the programs the
engine compiles for the node, the specialised build of such a program, and the numpy restatement (tests/blep_reference.py): against
a direct loop, its continuity, its agreement with the naive waveform outside the correction windows, and the aliasing it removes."""
import ctypes
import math
import pathlib
import types

import numpy as np
import pytest

from signals_amd import SignalFlags, _native, specialise
from signals_amd.chain import BadStateValue
from signals_amd.chain import ext, fixed, fx

import blep_reference as BR
import unison_reference as UR

ROOT = pathlib.Path(__file__).resolve().parent.parent
INV = 1     # hipErrorInvalidValue
KINDS = ('Square', 'Sawtooth', 'Triangle')
NODES = {kind: getattr(ext, 'Blep' + kind) for kind in KINDS}                  # (the module needs the feature: nothing here passes without it)
SAW = 2
SWEEP_HERTZ = (2000.0, -2000.0, 13000.0, 30000.0, 1e-3)


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


def blep_node(hertz, copies=None, spread=None, kind='Sawtooth'):
    n = NODES[kind]()
    if copies is not None:
        n.get_state().copies = copies
    n.hertz = fix(hertz)
    if spread is not None:
        n.spread = fix(spread)
    return n


# ---------------------------------------------------------------------------------------------- the node
def test_class_hierarchy_and_ports():
    assert issubclass(ext.BlepOsc, ext.UnisonOsc) and not hasattr(ext, 'BlepSine')
    assert ext.BlepOsc.bandlimited() is True and ext.UnisonOsc.bandlimited() is False
    for kind in KINDS:
        cls = NODES[kind]
        assert issubclass(cls, ext.BlepOsc) and cls.kind() == kind and cls.bandlimited() is True
        assert cls.port_names() == ['hertz', 'phase', 'spread']
        assert cls.flags() & SignalFlags.GENERATOR
        assert 'copies' in cls().state_attrs()
    for kind in ('Sine',) + KINDS:                                             # the existing classes keep their route
        assert getattr(ext, 'Unison' + kind).bandlimited() is False and not issubclass(getattr(ext, 'Unison' + kind), ext.BlepOsc)
    with pytest.raises(TypeError):
        ext.BlepOsc()                                                         # abstract: a kind is a subclass
    n = blep_node(np.full((1, 6), 220.0), spread=[[0.5]])
    assert n.channels == 6
    doc = ext.BlepOsc.__doc__
    for line in ('d = min(|h_u| / rate, 0.5)', 'Sawtooth: m = mod(t - 0.5, 1);  w = (2m - 1) - step(m)',
                 'Square:   m = mod(t, 1);        w = (m < 0.5 ? 1 : -1) + step(m) - step(mod(t + 0.5, 1))',
                 'Triangle: m = mod(t - 0.25, 1); w = tri(t - 0.25) + (4/3) d (corner(mod(t + 0.25, 1)) - corner(m))',
                 'tri(u) = (4 mod(u, 0.5) - 1) * (m < 0.5 ? -1 : 1)',
                 'rate / 4', 'no longer band-limits', 'Out of scope'):
        assert line in doc, line
    for line in doc.splitlines():                                             # the restatement states the same definition
        if line.strip().startswith(('step(m)', 'corner(m)', '= y*y', '= 0 ', '= ((m - 1)', 'Sawtooth:', 'Square:', 'Triangle:')):
            assert ' '.join(line.split()) in ' '.join(BR.__doc__.split()), line
    assert 'tri(u) = (4 mod(u, 0.5) - 1) * (m < 0.5 ? -1 : 1)' in BR.__doc__


def test_default_copies_and_the_shared_validator():
    c = ext.BlepSawtooth().get_state().copies
    assert c.shape == (1, 2) and c.dtype == np.float64 and not c.any()        # one clean oscillator
    assert np.array_equal(c, BR.default_copies())
    assert ext.BlepSquare().get_state().copies is not c                       # a factory: every node its own array
    assert ext.UnisonSawtooth().get_state().copies.shape == (7, 2)            # the parent's default stays
    n = ext.BlepTriangle()
    for bad in (np.zeros(2), np.zeros((0, 2)), np.zeros((17, 2)), np.zeros((3, 3)), np.array([[0.0, np.nan]]), [[0.0, 0.0]], None):
        with pytest.raises(BadStateValue):
            n.get_state().copies = bad
    n.get_state().copies = UR.default_copies()                                # the JP-8000 array: the anti-aliased supersaw
    assert n.host_copies().shape == (7, 2)
    n.get_state().copies = np.array([[0, 0], [1, 0], [-1, 0]])                # int64, what a .sigs value arrives as
    assert n.host_copies().dtype == np.float64 and n.host_copies().tolist() == [[0.0, 0.0], [1.0, 0.0], [-1.0, 0.0]]
    n.get_state().copies[1, 0] = 2                                            # an in-place edit is what the next launch takes
    assert n.host_copies().tolist() == [[0.0, 0.0], [2.0, 0.0], [-1.0, 0.0]]


def test_class_resolves_by_qualified_name_and_loads_from_a_patch():
    from signals_amd.chain import discovery, sigs
    from signals_amd.chain.driver import load_signal
    assert load_signal('signals_amd.chain.ext.BlepSawtooth') is ext.BlepSawtooth
    assert load_signal('signals.chain.ext.BlepSquare') is ext.BlepSquare
    assert discovery.load_signal('signals.chain.ext.BlepTriangle') is ext.BlepTriangle
    p = sigs.loads('+ 1a signals.chain.fixed.Fixed value=[[220.0]]\n+ 1b signals.chain.fixed.Fixed value=[[1]]\n'
                   '+ 2a signals.chain.ext.BlepSawtooth copies=[[0,0],[1,0],[-1,0]]\n+ 2b signals.chain.ext.BlepSquare\n'
                   '> 1a 2a.hertz\n> 1b 2a.spread\n> 1a 2b.hertz')
    node = p['2a']
    assert isinstance(node, ext.BlepSawtooth) and node.hertz.sig is p['1a'] and node.spread.sig is p['1b']
    assert node.get_state().copies.shape == (3, 2) and p['2b'].get_state().copies.shape == (1, 2)
    with pytest.raises(BadStateValue):
        sigs.loads('+ 1a signals.chain.ext.BlepSawtooth copies=[[0,0,0]]')


# ---------------------------------------------------------------------------------------------- C ABI
def test_entry_point_and_word_are_declared(lib):
    assert 'sig_osc_bank_blep' in _native.EXPORTS
    raw = ctypes.CDLL(str(_native.LIB_PATH))
    assert raw.sig_osc_bank_blep is not None
    header = (ROOT / 'include' / 'signals_amd.h').read_text()
    assert 'int sig_osc_bank_blep(' in header and 'SIG_VP_OSCBLEP = 17' in header and '   OSCBLEP acc =' in header
    assert 'OSCUNI, OSCBLEP: c may be -1' in header
    assert _native.VP_OPS['OscBlep'] == 17 and _native.VP_OPS['OscUni'] == 16
    assert _native.VP_BLEP_OPS == ('OscBlep',) and 'OscBlep' not in _native.VP_EXT_OPS
    assert _native.voice_program_words([('OscBlep', 2, 0, 0, -1)]) == [0xf0051]            # Sawtooth, no spread: slot 15
    assert _native.voice_program_words([('OscBlep', 3, 1, 0, 2)]) == [0x20171]
    assert _native.vp_families([('OscBlep', 2, 0, 0, -1), ('Filter', 0, 0, 0, 0)]) == ('unison',)
    assert _native.vp_families([('OscBlep', 2, 0, 0, -1), ('OscUni', 2, 1, 0, -1)]) == ('unison',)       # one family, two words
    assert _native.vp_families([('OscBlep', 2, 0, 0, -1), ('FilterQ', 0, 0, 0, -1)]) == ('resonant', 'unison')


def test_osc_bank_blep_argument_errors_do_not_reach_the_device(lib):
    p = 64                                                                    # (never dereferenced: every call fails its checks)
    host = (ctypes.c_double * 16)()
    args = dict(kind=2, position=0, step=1, rate=48000, rows=256, voices=8, rpp=0, hertz=p, hs=1, hrs=0, phase=None, ps=0, prs=0,
                spread=p, ss=1, srs=0, copies=7, detune=host, offsets=host, out=p, odt=0, old=8, stream=None)

    def call(**over):
        a = dict(args, **over)
        return lib.sig_osc_bank_blep(*(a[k] for k in args))
    assert call(kind=0) == INV                                                # Sine has no edge
    assert call(kind=4) == INV and call(kind=-1) == INV
    assert call(detune=None) == INV and call(offsets=None) == INV             # a null copies pointer
    assert call(copies=17) == INV and call(copies=0) == INV and call(copies=-1) == INV
    assert call(old=4) == INV and call(hertz=None) == INV and call(out=None) == INV
    assert call(ss=2) == INV and call(srs=-1) == INV
    assert call(odt=2) == INV and call(rate=0) == INV and call(position=-1) == INV and call(step=0) == INV
    for kind in (1, 2, 3):
        assert call(kind=kind, rows=0) == 0                                   # accepted, nothing to launch
    assert call(voices=0, old=0) == 0 and call(rows=0, copies=1) == 0 and call(rows=0, copies=16) == 0
    assert call(rows=0, spread=None) == 0 and call(rows=0, phase=None) == 0   # unplugged
    # the unison entry keeps refusing kind 4 and keeps taking Sine
    assert lib.sig_osc_bank_unison(*(dict(args, kind=4)[k] for k in args)) == INV
    assert lib.sig_osc_bank_unison(*(dict(args, kind=0, rows=0)[k] for k in args)) == 0


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


def test_voice_program_refuses_bad_blep_programs(lib):
    buf = (ctypes.c_float * 64)()

    def copies(n):
        u = _native.VpUnisonT()
        u.copies = n
        return u

    def tables(*geometry):
        t = _native.VpTablesT()
        t.n_tables = len(geometry)
        for k, (ptr, points, waves) in enumerate(geometry):
            t.table[k] = _native.VpTable(ptr, points, waves)
        return t

    def run(code, uni, tabs=None, nblocks=1, control_rows=2, entry='sig_voice_program_unison', **kw):
        P, keep = _program(code, **kw)
        return getattr(lib, entry)(ctypes.byref(P), 48000, 0, 256, nblocks, 100, 8, control_rows, 0, None, 0, None, 0, 0, None,
                                   ctypes.addressof(buf), 8, None, None, ctypes.byref(tabs) if tabs is not None else None,
                                   ctypes.byref(uni) if uni is not None else None)
    seven = copies(7)
    word = ('OscBlep', SAW, 0, 0, -1)
    assert run([('OscBlep', 0, 0, 0, -1)], seven) == INV                      # Sine
    assert run([('OscBlep', 4, 0, 0, -1)], seven) == INV                      # a kind above Triangle
    assert run([('OscUni', 4, 0, 0, -1)], seven) == INV                       # ... which OscUni keeps refusing too
    assert run([word], None) == INV                                           # the word without its copies
    assert run([word], copies(17)) == INV and run([word], copies(0)) == INV
    assert run([('OscBlep', SAW, 0, 1, -1)], seven) == INV                    # unison slot 1: only slot 0 exists
    assert run([('OscBlep', SAW, 1, 0, -1)], seven) == INV                    # oscillator slot 1 of 1
    assert run([('OscBlep', SAW, 0, 0, 1)], seven) == INV                     # spread: parameter slot 1 of 1
    # the unison family's exclusions
    assert run([word, ('Band', 0, 0, 0, 0)], seven, types=['bp', 'bp']) == INV
    assert run([word, ('OscPM', 0, 1, 0, 0)], seven, n_oscs=2) == INV
    assert run([word, ('Save', 0, 0, 0, 0), ('OscTable', 0, 1, 0, -1), ('Mul', 0, 0, 0, 0)], seven, tabs=tables((64, 64, 3)), n_oscs=2) == INV
    assert run([word, ('Shape', 0, 0, 0, -1)], seven, tabs=tables((64, 64, 3))) == INV
    assert run([word, ('FilterQ', 0, 0, 0, -1)], seven, types=['rlp']) == INV
    P, keep = _program([word])
    assert lib.sig_voice_program_ex(ctypes.byref(P), 48000, 0, 256, 1, 100, 8, 2, 0, None, 0, None, 0, 0, None,
                                    ctypes.addressof(buf), 8, None, None, None) == INV
    # accepted, nothing to launch: no blocks -- alone, behind a filter, beside an OscUni word, and combined through the mixed entry
    for kind in (1, 2, 3):
        assert run([('OscBlep', kind, 0, 0, -1)], seven, nblocks=0, control_rows=1) == 0
    assert run([word], copies(1), nblocks=0, control_rows=1) == 0 and run([word], copies(16), nblocks=0, control_rows=1) == 0
    assert run([word, ('Filter', 0, 0, 0, 0)], seven, nblocks=0, control_rows=1, types=['lp']) == 0
    assert run([word, ('Save', 0, 0, 0, 0), ('OscUni', 0, 1, 0, -1), ('Mul', 0, 0, 0, 0)], seven, nblocks=0, control_rows=1, n_oscs=2) == 0
    assert run([word, ('FilterQ', 0, 0, 0, -1)], seven, nblocks=0, control_rows=1, types=['rlp'], entry='sig_voice_program_mixed') == 0
    assert run([('OscBlep', 0, 0, 0, -1), ('FilterQ', 0, 0, 0, -1)], seven, types=['rlp'], entry='sig_voice_program_mixed') == INV      # Sine there too


# ---------------------------------------------------------------------------------------------- planning
def test_voice_programs():
    from signals_amd.engine import _KNOWN_TYPES, _VoiceProgram, _control_ports, _is_pure
    V = 8
    row = lambda lo, hi: np.linspace(lo, hi, V).reshape(1, V)
    bare = blep_node(row(220, 440))
    assert any(issubclass(ext.BlepOsc, t) for t in _KNOWN_TYPES if isinstance(t, type))
    assert _control_ports(bare) == [bare.hertz, bare.phase, bare.spread] and _is_pure(bare, {})
    prog = _VoiceProgram.compile(None, bare, V, min_nodes=1)
    assert prog.describe() == 'OscBlep' and prog.code == [('OscBlep', SAW, 0, 0, -1)] and prog.unison is bare
    lp = fx.LowPass(); lp.input = bare; lp.cutoff = fix(row(500, 5000))
    prog = _VoiceProgram.compile(None, lp, V)
    assert prog.code == [('OscBlep', SAW, 0, 0, -1), ('Filter', 0, 0, 0, 0)] and prog.depth == 1 and prog.families == ('unison',)
    assert _native.voice_program_words(prog.code) == [0xf0051, 0x1]
    small = types.SimpleNamespace(owner=types.SimpleNamespace(specialise=False), N=256, _pure={})
    assert _VoiceProgram(small, lp, V).worthwhile()                           # the small-file rule, as for OscUni
    # the parent's classes keep their word
    u = ext.UnisonSawtooth(); u.hertz = fix(row(220, 440))
    assert _VoiceProgram.compile(None, u, V, min_nodes=1).code == [('OscUni', SAW, 0, 0, -1)]
    # a band-limited and a plain unison oscillator on one copies array: one program, one unison slot
    shared = np.array([[0.0, 0.0], [0.01, 0.5]])
    a = blep_node(row(220, 440), shared, kind='Square'); b = ext.UnisonSine(); b.hertz = fix(row(110, 220)); b.get_state().copies = shared
    m = fx.Mix(); m.left = a; m.right = b; m.mix = fix([[0.25]])
    prog = _VoiceProgram.compile(None, m, V)
    assert prog.code == [('OscBlep', 1, 0, 0, -1), ('Save', 0, 0, 0, 0), ('OscUni', 0, 1, 0, -1), ('Mix', 0, 0, 0, 0)]
    b.get_state().copies = shared.copy()
    with pytest.raises(Exception, match='distinct copies arrays'):
        _VoiceProgram(None, m, V)
    # with a Shaper: refused unless mixed
    sh = ext.Shaper(); sh.input = blep_node(row(220, 440))
    assert _VoiceProgram.compile(None, sh, V) is None
    with pytest.raises(Exception, match='no interpreter variant has both'):
        _VoiceProgram(None, sh, V)
    prog = _VoiceProgram(None, sh, V, mixed=True)
    assert [op for op, *_ in prog.code] == ['OscBlep', 'Shape'] and prog.families == ('table', 'unison')
    rl = ext.ResonantLowPass(); rl.input = blep_node(row(220, 440)); rl.cutoff = fix(row(500, 5000)); rl.resonance = fix([[2.0]])
    assert _VoiceProgram.compile(None, rl, V) is None
    assert [op for op, *_ in _VoiceProgram(None, rl, V, mixed=True).code] == ['OscBlep', 'FilterQ']


def test_the_node_in_a_control_path_is_refused_with_its_reason():
    from signals_amd.engine import NotBatchable, _ControlProgram
    with pytest.raises(NotBatchable, match='unison oscillator has no block-rate program'):
        _ControlProgram((blep_node([[3.0]]),), 4)


# ---------------------------------------------------------------------------------------------- specialised build
def test_flags_of_a_program_with_the_word():
    code = [('OscBlep', SAW, 0, 0, -1), ('Filter', 0, 0, 0, 0)]
    f = specialise.flags(code, 1, 0, 1, 0, 2, 2)
    assert f[-2:] == ['-DSIG_VP_S_UNI=1', '-DSIG_VP_S_BLEP=1']                # the copies parameter, and the handler
    assert {'-DSIG_VP_STATIC_CODE={0xf0051,0x1}', '-DSIG_VP_S_NO=1', '-DSIG_VP_S_NF=1', '-DSIG_VP_S_EXT=0'} <= set(f)
    assert not any(x in ' '.join(f) for x in ('S_TAB', 'S_RES', 'S_MIXED'))
    uni = specialise.flags([('OscUni', SAW, 0, 0, -1), ('Filter', 0, 0, 0, 0)], 1, 0, 1, 0, 2, 2)
    assert '-DSIG_VP_S_UNI=1' in uni and not any('BLEP' in x for x in uni)    # programs without the word: the list they had
    for other in ([('Osc', 2, 0, 0, 0), ('Filter', 0, 0, 0, 0)], [('OscTable', 0, 0, 0, -1)], [('Osc', 0, 0, 0, 0), ('FilterQ', 0, 0, 0, -1)]):
        assert not any('BLEP' in x or 'S_UNI' in x for x in specialise.flags(other, 2, 1, 1, 0, 2, 2)), other
    mixed = specialise.flags([('OscBlep', SAW, 0, 0, -1), ('FilterQ', 0, 0, 0, -1)], 1, 0, 1, 0, 2, 2)
    assert mixed[-4:] == ['-DSIG_VP_S_RES=1', '-DSIG_VP_S_UNI=1', '-DSIG_VP_S_BLEP=1', '-DSIG_VP_S_MIXED=1']
    assert 'copies' not in specialise.flags.__code__.co_varnames              # one image serves every copies array


@pytest.mark.skipif(specialise.hipcc() is None, reason='no hipcc in this environment')
def test_the_specialised_blep_program_builds(tmp_path, monkeypatch):
    monkeypatch.setattr(specialise, 'CACHE', tmp_path)
    image = specialise.build([('OscBlep', SAW, 0, 0, 0), ('Filter', 0, 0, 0, 0), ('Gain', 0, 1, 0, 0)], 1, 2, 1, 0, 2, 2)
    assert b'sig_vp_specialised' in image and b'sig_vp_specialised_info' in image


# ---------------------------------------------------------------------------------------------- the restatement
def _step(m, d):
    if m < d:
        x = m / d
        return 2.0 * x - x * x - 1.0
    if m > 1.0 - d:
        y = (m - 1.0) / d
        return y * y + 2.0 * y + 1.0
    return 0.0


def _corner(m, d):
    if m < d:
        return (1.0 - m / d) ** 3
    if m > 1.0 - d:
        return ((m - 1.0) / d + 1.0) ** 3
    return 0.0


def _direct(kind, t, d):
    """the definition for one sample, branch by branch in Python floats (the Triangle's naive part as 4 |m - 1/2| - 1)"""
    mod = lambda x: float(np.mod(np.float64(x), 1.0))
    if kind == 'Sawtooth':
        m = mod(t - 0.5)
        return (2.0 * m - 1.0) - _step(m, d)
    if kind == 'Square':
        m = mod(t)
        return (1.0 if m < 0.5 else -1.0) + _step(m, d) - _step(mod(t + 0.5), d)
    m = mod(t - 0.25)
    tri = 4.0 * abs(m - 0.5) - 1.0                                            # the textbook form: within an ulp of tri(u) in osc.py's order
    return tri + 4.0 / 3.0 * d * (_corner(mod(t + 0.25), d) - _corner(m, d))


@pytest.mark.parametrize('kind', KINDS)
def test_reference_restatement_against_a_direct_loop(kind):
    rng = np.random.default_rng(4)
    copies = np.stack([rng.uniform(-0.12, 0.12, 5), rng.uniform(0, 1, 5)], axis=1)
    hz = np.array([[440.0, -2000.0, 13000.0, 30000.0, 0.0, 1e-3, 750.0]])     # 750 = rate / 64: exact edges at phase 0
    ph, sp = np.array([[0.3, 0.7, 0.1, 0.9, 0.25, 0.5, 0.0]]), rng.uniform(0, 1, (1, 7))
    got = BR.blep(kind, copies, 50, 70, hz, ph, sp)
    assert got.shape == (70, 7) and got.dtype == np.float64 and np.isfinite(got).all()
    worst = 0.0
    for r in range(70):
        for v in range(7):
            s = None
            for d, p in copies.tolist():
                h = hz[0, v] * (1.0 + sp[0, v] * d)
                t = float(np.float64(50 + r) / 48000 * h + (ph[0, v] + p))
                w = _direct(kind, t, min(abs(h) / 48000, 0.5))
                s = w if s is None else s + w
            worst = max(worst, abs(got[r, v] - s / 5))
    assert worst <= 4e-16, worst                                              # (a ** 3 against a * a * a, |m - 0.5| against mod(u, 0.5): an ulp of a value <= 1 each)
    one = BR.blep(kind, [[0, 0]], 0, 256, [[750.0]])                          # one copy at rate / 64, phase 0: m = 0 and m = 1/2 are hit
    for r in range(256):
        assert abs(one[r, 0] - _direct(kind, float(np.float64(r) / 48000 * 750.0 + 0.0), 750.0 / 48000)) <= 4e-16, r
    # the waveforms' landmarks at 1 kHz: zero at the edges t = 0 and 1/2, the peaks at 1/4 and 3/4 (the Triangle's rounded off: 35/36)
    at = [float(BR.blep_wave(kind, np.float64(t), np.float64(1000 / 48000))) for t in (0.0, 0.25, 0.5, 0.75)]
    peak = {'Sawtooth': 0.5, 'Square': 1.0, 'Triangle': 0.9722222222222222}[kind]
    assert at[0] == 0.0 and at[2] == 0.0 and math.isclose(at[1], peak, rel_tol=1e-15) and math.isclose(at[3], -peak, rel_tol=1e-15), at


@pytest.mark.parametrize('kind', KINDS)
def test_special_values(kind):
    zero = BR.blep_wave(kind, np.linspace(-1, 1, 4001), 0.0)                  # d = 0: no window, the naive value
    assert np.isfinite(zero).all()                                            # (m / 0 is an inf or a NaN in the branch no select takes)
    from oracle import chain_ref as R
    t = np.linspace(-1, 1, 4001)
    naive = R.osc_wave(kind, t)
    edge = np.abs(naive) == 0.0 if kind != 'Sawtooth' else np.zeros_like(t, dtype=bool)   # np.sign's isolated zero, dropped on purpose
    assert np.array_equal(zero[~edge], naive[~edge])
    bad = BR.blep_wave(kind, np.array([np.nan, np.inf, -np.inf]), 0.01)
    assert np.isnan(bad).all()                                                # a non-finite t gives NaN
    assert np.isnan(BR.blep_wave(kind, np.array([np.nan]), 0.0)).all()
    assert np.array_equal(BR.blep(kind, [[0, 0]], 0, 64, [[0.0]], [[0.3]]), BR.blep(kind, [[0, 0]], 5, 64, [[0.0]], [[0.3]]))   # 0 Hz: a constant
    hz = np.array([[440.0, 2000.0, 13000.0]])
    assert np.array_equal(BR.blep(kind, [[0, 0]], 0, 256, -hz, [[0.2]]), BR.blep_wave(kind, R.frame_range(0, 256) / 48000 * -hz + 0.2, hz / 48000))   # |h|


@pytest.mark.parametrize('hertz', SWEEP_HERTZ)
@pytest.mark.parametrize('kind', KINDS)
def test_the_restatement_is_continuous(kind, hertz):
    """a fine sweep of t over two cycles: no step larger than (2 + 2 / d) grid steps (the naive slope plus the residual's)"""
    d = float(BR.increment(np.float64(hertz), 48000))
    t = np.linspace(-1.0, 1.0, 2_000_001)
    w = BR.blep_wave(kind, t, d)
    assert np.isfinite(w).all() and np.abs(w).max() <= 1.0 + 1e-12
    jump = float(np.abs(np.diff(w)).max())
    assert jump < (2.0 + 2.0 / d) * (t[1] - t[0]), (kind, hertz, jump)
    from oracle import chain_ref as R
    assert float(np.abs(np.diff(R.osc_wave(kind, t))).max()) > (0.5 if kind != 'Triangle' else 0.0)      # (the naive edge does jump)


@pytest.mark.parametrize('kind', KINDS)
def test_rows_outside_every_window_are_the_naive_waveform(kind):
    from oracle import chain_ref as R
    rng = np.random.default_rng(5)
    hz, ph = rng.uniform(55, 7000, (1, 64)), rng.uniform(0, 1, (1, 64))
    for pos in (0, 48000 * 3600):
        n = R.frame_range(pos, 512)
        got = BR.blep(kind, [[0, 0]], pos, 512, hz, ph)
        inside = BR.in_window(kind, n / 48000 * hz + ph, BR.increment(hz, 48000))
        assert 0.01 < inside.mean() < 0.6                                     # both sides are exercised
        assert np.array_equal(got[~inside], R.osc(kind, pos, 512, 48000, hz, ph)[~inside])
        assert not np.array_equal(got[inside], R.osc(kind, pos, 512, 48000, hz, ph)[inside])


# required margin below the naive waveform's alias / harmonic ratio, naive ratio, band-limited ratio (dB).
# The two ratios are what this definition gives in numpy's float64 (recorded here to two decimals and re-derived by the test); the
# margins are the requirement: a two-sample polynomial step removes about 15 dB of a saw's and a square's fold-back at this pitch and
# 13 dB of a triangle's, and 12 / 12 / 10 dB leave room for nothing but rounding
ALIAS = {'Sawtooth': (12.0, -13.3, -28.6), 'Square': (12.0, -15.3, -31.6), 'Triangle': (10.0, -42.3, -55.0)}


@pytest.mark.parametrize('kind', KINDS)
def test_the_aliasing_it_removes(kind):
    """the point of the feature: 4096 frames from position 1000 at hertz = 48000 * 37 / 1024 and phase 0.1234 (148 whole cycles: every
    harmonic and every alias falls on a bin of its own), an unwindowed rfft"""
    from oracle import chain_ref as R
    hz, ph = np.array([[48000 * 37 / 1024]]), np.array([[0.1234]])
    x = BR.blep(kind, [[0, 0]], 1000, 4096, hz, ph)[:, 0]
    naive = R.osc(kind, 1000, 4096, 48000, hz, ph)[:, 0]
    margin, naive_db, clean_db = ALIAS[kind]
    got_naive, got_clean = BR.alias_ratio_db(naive), BR.alias_ratio_db(x)
    print('alias / harmonic', kind, 'naive', got_naive, 'band-limited', got_clean)
    assert got_clean <= got_naive - margin, (kind, got_naive, got_clean)
    assert abs(got_naive - naive_db) < 0.05 and abs(got_clean - clean_db) < 0.05, (kind, got_naive, got_clean)   # the recorded figures
    assert abs(x.mean()) < 1e-12 and np.abs(x).max() <= 1.0


def test_reference_renders_blocks_with_per_block_rows_and_as_an_oracle_node():
    from oracle import chain_ref as R
    copies = UR.default_copies()
    hertz = np.array([[100.0, 200.0], [3000.0, 4000.0]])
    got = BR.blep('Sawtooth', copies, 50, 4, hertz, phase=[[0.25]], spread=[[0.5]], blocks=2)
    n = R.frame_range(50, 8)
    want = np.concatenate([BR.blep_sum('Sawtooth', n[:4], 48000, hertz[:1], 0.25, 0.5, copies),
                           BR.blep_sum('Sawtooth', n[4:], 48000, hertz[1:], 0.25, 0.5, copies)])
    assert np.array_equal(got, want) and abs(got).max() <= 1.0
    node = BR.BlepOsc('Sawtooth', copies, R.Fixed(hertz[:1]), R.Fixed([[0.25]]), R.Fixed([[0.5]]))
    assert np.array_equal(R.render(node, 50, 4, 2), want[:4])
