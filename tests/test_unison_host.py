"""The unison oscillators without a GPU: the node API of ext.UnisonOsc and its state validation, name resolution and the .sigs
loader, the exports and argument checks of sig_osc_bank_unison and sig_voice_program_unison, the OscUni instruction's encoding, how
the engine's planner classifies the node and the programs it compiles for it, the specialised build of a program with the
instruction, and the numpy restatement (tests/unison_reference.py) against a direct loop."""
import ctypes
import math
import pathlib
import types

import numpy as np
import pytest

from signals_amd import SignalFlags, _native, specialise
from signals_amd.chain import BadStateValue, BlockCachingEmitter
from signals_amd.chain import ext, fixed, fx, osc

import unison_reference as UR

ROOT = pathlib.Path(__file__).resolve().parent.parent
INV = 1     # hipErrorInvalidValue
KINDS = ('Sine', 'Square', 'Sawtooth', 'Triangle')
NODES = {kind: getattr(ext, 'Unison' + kind) for kind in KINDS}                # (the module needs the feature: nothing here passes without it)


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


def unison_node(hertz, copies=None, spread=None, kind='Sawtooth'):
    n = getattr(ext, 'Unison' + kind)()
    if copies is not None:
        n.get_state().copies = copies
    n.hertz = fix(hertz)
    if spread is not None:
        n.spread = fix(spread)
    return n


# ---------------------------------------------------------------------------------------------- the node
def test_node_api():
    assert issubclass(ext.UnisonOsc, BlockCachingEmitter) and not issubclass(ext.UnisonOsc, osc.Osc)
    for kind in KINDS:
        cls = getattr(ext, 'Unison' + kind)
        assert issubclass(cls, ext.UnisonOsc) and cls.kind() == kind
        assert cls.port_names() == ['hertz', 'phase', 'spread']
        assert cls.flags() & SignalFlags.GENERATOR
        assert 'copies' in cls().state_attrs()
    with pytest.raises(TypeError):
        ext.UnisonOsc()                                                       # abstract: a kind is a subclass
    n = unison_node(np.full((1, 6), 220.0), spread=[[0.5]])
    assert n.channels == 6                                                    # ImplicitChannels: the one width that is not 1
    assert ext.UnisonOsc.__doc__ and 'r_u = 1.0 + spread[v] * d[u]' in ext.UnisonOsc.__doc__ and 'Out of scope' in ext.UnisonOsc.__doc__


def test_default_copies():
    c = ext.UnisonSawtooth().get_state().copies
    assert c.shape == (7, 2) and c.dtype == np.float64
    assert c[:, 0].tolist() == [-0.11002313, -0.06288439, -0.01952356, 0.0, 0.01991221, 0.06216538, 0.10745242]
    assert np.array_equal(c[:, 1], np.mod(np.arange(7) * 0.6180339887498949, 1.0))
    assert np.array_equal(c, UR.default_copies())
    assert ext.UnisonSine().get_state().copies is not c                       # a factory: every node its own array
    assert _native.UNISON_MAX_COPIES == 16 and _native.VP_MAX_UNISON == 1


@pytest.mark.parametrize('bad', [np.zeros(2), np.zeros((0, 2)), np.zeros((17, 2)), np.zeros((3, 3)), np.array([[0.0, np.nan]]),
                                 np.array([[np.inf, 0.0]]), np.array([[0.0, -np.inf]]), [[0.0, 0.0]], None, np.zeros((2, 2, 2)),
                                 np.array([['a', 'b']])],
                         ids=['1-D', '0 rows', '17 rows', '3 columns', 'NaN', 'inf', '-inf', 'a list', 'None', '3-D', 'strings'])
def test_state_validation_refuses(bad):
    n = ext.UnisonSawtooth()
    with pytest.raises(BadStateValue):
        n.get_state().copies = bad


def test_state_validation_accepts():
    n = ext.UnisonSquare()
    for good in (np.zeros((1, 2)), np.zeros((16, 2)), np.zeros((7, 2), dtype=np.float32), np.array([[0, 0], [1, 0]]),
                 np.arange(8, dtype=np.uint8).reshape(4, 2)):
        n.get_state().copies = good
    n.get_state().copies = np.array([[0, 0], [1, 0], [-1, 0]])                 # int64, what a .sigs value arrives as
    assert n.get_state().copies.dtype == np.int64
    got = n.host_copies()
    assert got.dtype == np.float64 and got.tolist() == [[0.0, 0.0], [1.0, 0.0], [-1.0, 0.0]]
    n.get_state().copies[1, 0] = 2                                            # an in-place edit is what the next launch takes
    assert n.host_copies().tolist() == [[0.0, 0.0], [2.0, 0.0], [-1.0, 0.0]]


def test_class_resolves_by_qualified_name_and_loads_from_a_patch():
    from signals_amd.chain import discovery, sigs
    from signals_amd.chain.driver import load_signal
    assert load_signal('signals_amd.chain.ext.UnisonSawtooth') is ext.UnisonSawtooth
    assert load_signal('signals.chain.ext.UnisonSine') is ext.UnisonSine
    assert discovery.load_signal('signals.chain.ext.UnisonTriangle') is ext.UnisonTriangle
    p = sigs.loads('+ 1a signals.chain.fixed.Fixed value=[[220.0]]\n+ 1b signals.chain.fixed.Fixed value=[[1]]\n'
                   '+ 2a signals.chain.ext.UnisonSawtooth copies=[[0,0],[1,0],[-1,0]]\n> 1a 2a.hertz\n> 1b 2a.spread')
    node = p['2a']
    assert isinstance(node, ext.UnisonSawtooth) and node.hertz.sig is p['1a'] and node.spread.sig is p['1b']
    assert node.get_state().copies.shape == (3, 2) and node.get_state().copies.dtype.kind == 'i'
    with pytest.raises(BadStateValue):
        sigs.loads('+ 1a signals.chain.ext.UnisonSawtooth copies=[[0,0,0]]')


# ---------------------------------------------------------------------------------------------- C ABI
def test_entry_points_are_exported_and_declared(lib):
    assert 'sig_osc_bank_unison' in _native.EXPORTS and 'sig_voice_program_unison' in _native.EXPORTS
    raw = ctypes.CDLL(str(_native.LIB_PATH))
    assert raw.sig_osc_bank_unison is not None and raw.sig_voice_program_unison is not None
    assert lib.sig_abi_version() == 7
    header = (ROOT / 'include' / 'signals_amd.h').read_text()
    assert 'int sig_osc_bank_unison(' in header and 'int sig_voice_program_unison(' in header
    assert 'SIG_VP_OSCUNI = 16' in header and 'SIG_VP_MAX_UNISON = 1' in header and 'SIG_UNISON_MAX_COPIES = 16' in header
    assert 'sig_vp_unison_t' in header and '   OSCUNI acc =' in header
    assert ctypes.sizeof(_native.VpUnisonT) == 8 + 2 * 16 * 8                 # int32 + padding, two arrays of 16 doubles


def test_osc_bank_unison_argument_errors_do_not_reach_the_device(lib):
    p = 64                                                                    # (never dereferenced: every call fails its checks)
    host = (ctypes.c_double * 16)()
    args = dict(kind=2, position=0, step=1, rate=48000, rows=256, voices=8, rpp=0, hertz=p, hs=1, hrs=0, phase=None, ps=0, prs=0,
                spread=p, ss=1, srs=0, copies=7, detune=host, offsets=host, out=p, odt=0, old=8, stream=None)

    def call(**over):
        a = dict(args, **over)
        return lib.sig_osc_bank_unison(*(a[k] for k in args))
    assert call(copies=0) == INV and call(copies=17) == INV and call(copies=-1) == INV
    assert call(detune=None) == INV and call(offsets=None) == INV
    assert call(kind=4) == INV and call(kind=-1) == INV
    assert call(old=4) == INV                                                 # rows narrower than the voices
    assert call(hertz=None) == INV and call(out=None) == INV
    assert call(ss=2) == INV and call(srs=-1) == INV                          # spread rows: strides 0 / 1, row stride >= 0
    assert call(odt=2) == INV and call(rate=0) == INV and call(position=-1) == INV and call(step=0) == INV
    assert call(rows=0) == 0 and call(voices=0, old=0) == 0                   # accepted, nothing to launch
    assert call(rows=0, copies=1) == 0 and call(rows=0, copies=16) == 0       # the limits themselves are inside
    assert call(rows=0, spread=None) == 0 and call(rows=0, phase=None) == 0   # unplugged


def test_instruction_encoding():
    assert _native.VP_OPS['OscUni'] == 16
    assert _native.voice_program_words([('OscUni', 2, 0, 0, -1)]) == [0xf0050]            # Sawtooth, no spread: slot 15
    assert _native.voice_program_words([('OscUni', 3, 1, 0, 2)]) == [0x20170]
    assert 'OscUni' not in _native.VP_EXT_OPS and _native.VP_UNI_OPS == ('OscUni',)


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


def test_voice_program_refuses_bad_unison_programs(lib):
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

    def run(code, uni, tabs=None, nblocks=1, control_rows=2, **kw):
        P, keep = _program(code, **kw)
        return lib.sig_voice_program_unison(ctypes.byref(P), 48000, 0, 256, nblocks, 100, 8, control_rows, 0, None, 0, None, 0, 0, None,
                                            ctypes.addressof(buf), 8, None, None, ctypes.byref(tabs) if tabs is not None else None,
                                            ctypes.byref(uni) if uni is not None else None)
    seven = copies(7)
    word = ('OscUni', 2, 0, 0, -1)
    assert run([word], copies(0)) == INV and run([word], copies(17)) == INV and run([word], copies(-3)) == INV      # copies outside 1..16
    assert run([('Osc', 0, 0, 0, 0)], copies(17), nblocks=0, control_rows=1) == INV   # ... even where no word reads them
    assert run([word], None) == INV                                           # the word without its argument
    assert run([('OscUni', 2, 0, 1, -1)], seven) == INV                       # unison slot 1: only slot 0 exists
    assert run([('OscUni', 2, 1, 0, -1)], seven) == INV                       # oscillator slot 1 of 1
    assert run([('OscUni', 2, 0, 0, 1)], seven) == INV                        # spread: parameter slot 1 of 1
    assert run([('OscUni', 2, 0, 0, 0)], seven, n_params=0) == INV
    assert run([('OscUni', 4, 0, 0, -1)], seven) == INV                       # a kind above Triangle
    # no interpreter variant has the word together with any of these
    assert run([word, ('Band', 0, 0, 0, 0)], seven, types=['bp', 'bp']) == INV
    assert run([word, ('OscPM', 0, 1, 0, 0)], seven, n_oscs=2) == INV
    assert run([word, ('Save', 0, 0, 0, 0), ('OscTable', 0, 1, 0, -1), ('Mul', 0, 0, 0, 0)], seven, tabs=tables((64, 64, 3)), n_oscs=2) == INV
    assert run([word, ('Shape', 0, 0, 0, -1)], seven, tabs=tables((64, 64, 3))) == INV
    assert run([word, ('FilterQ', 0, 0, 0, -1)], seven, types=['rlp']) == INV
    # sig_voice_program_ex and sig_voice_program are the same call without the copies
    P, keep = _program([word])
    assert lib.sig_voice_program_ex(ctypes.byref(P), 48000, 0, 256, 1, 100, 8, 2, 0, None, 0, None, 0, 0, None,
                                    ctypes.addressof(buf), 8, None, None, None) == INV
    assert lib.sig_voice_program(ctypes.byref(P), 48000, 0, 256, 1, 100, 8, 2, 0, None, 0, None, 0, 0, None,
                                 ctypes.addressof(buf), 8, None, None) == INV
    # accepted, nothing to launch: no blocks
    assert run([word], seven, nblocks=0, control_rows=1) == 0 and run([word], copies(1), nblocks=0, control_rows=1) == 0
    assert run([word], copies(16), nblocks=0, control_rows=1) == 0
    assert run([word, ('Filter', 0, 0, 0, 0)], seven, nblocks=0, control_rows=1, types=['lp']) == 0
    assert run([('Osc', 0, 0, 0, 0)], seven, nblocks=0, control_rows=1) == 0  # copies nobody reads


# ---------------------------------------------------------------------------------------------- planning
def test_purity_and_modulation_classification():
    from signals_amd.engine import _KNOWN_TYPES, _audio_ports, _control_ports, _ctl_const, _foreign, _is_pure, _modulated
    assert ext.UnisonOsc in _KNOWN_TYPES
    u = unison_node([[440.0]], spread=[[1.0]])
    assert not _foreign(u)
    assert _control_ports(u) == [u.hertz, u.phase, u.spread] and _audio_ports(u) == []       # a leaf
    assert all(_ctl_const(p) for p in _control_ports(u)) and not _modulated(u) and _is_pure(u, {})
    swept = unison_node([[440.0]]); swept.spread = sine([[2.0]])
    assert _modulated(swept) and not _is_pure(swept, {})                      # spread re-read every block: tails
    g = fx.Gain(); g.left = u; g.right = fix([[0.5]])
    assert _is_pure(g, {})


def test_voice_programs():
    from signals_amd.engine import _VoiceProgram
    V = 8
    row = lambda lo, hi: np.linspace(lo, hi, V).reshape(1, V)
    bare = unison_node(row(220, 440))
    prog = _VoiceProgram.compile(None, bare, V, min_nodes=1)
    assert prog.describe() == 'OscUni' and prog.code == [('OscUni', 2, 0, 0, -1)]         # Sawtooth, spread unplugged
    assert prog.unison is bare and (len(prog.oscs), len(prog.params), len(prog.filters), prog.n_temps, prog.depth) == (1, 0, 0, 0, 0)
    assert _VoiceProgram.compile(None, bare, V) is None                       # a single node stays its own kernel (under a bus it does not)

    spread = unison_node(row(220, 440), spread=row(0, 1), kind='Triangle')
    lp = fx.LowPass(); lp.input = spread; lp.cutoff = fix(row(500, 5000))
    prog = _VoiceProgram.compile(None, lp, V)
    assert prog.describe() == 'OscUni,Filter' and prog.code == [('OscUni', 3, 0, 0, 0), ('Filter', 0, 0, 0, 0)] and prog.depth == 1
    assert _native.voice_program_words(prog.code) == [0x00070, 0x1]
    small = types.SimpleNamespace(owner=types.SimpleNamespace(specialise=False), N=256, _pure={})
    assert _VoiceProgram(small, lp, V).worthwhile()                           # the SMALL register file: the existing rule

    # two nodes that share one copies array: one unison slot
    shared = np.array([[0.0, 0.0], [0.01, 0.5]])
    a, b = unison_node(row(220, 440), shared), unison_node(row(110, 220), shared, kind='Square')
    m = fx.Mix(); m.left = a; m.right = b; m.mix = fix([[0.25]])
    prog = _VoiceProgram.compile(None, m, V)
    assert prog.code == [('OscUni', 2, 0, 0, -1), ('Save', 0, 0, 0, 0), ('OscUni', 1, 1, 0, -1), ('Mix', 0, 0, 0, 0)]
    assert prog.unison is a and prog.unison.get_state().copies is shared
    # two distinct arrays, even of equal values: the launch carries one
    b.get_state().copies = shared.copy()
    assert _VoiceProgram.compile(None, m, V) is None
    with pytest.raises(Exception, match='distinct copies arrays'):
        _VoiceProgram(None, m, V)

    # with a band filter, a PM carrier, a Wavetable, a Shaper or a resonant filter: no interpreter variant has both
    def none_with(top):
        assert _VoiceProgram.compile(None, top, V) is None
        with pytest.raises(Exception, match='no interpreter variant has both'):
            _VoiceProgram(None, top, V)
    bp = fx.BandPass(); bp.input = unison_node(row(220, 440)); bp.low = fix(row(300, 400)); bp.high = fix(row(900, 1200))
    none_with(bp)
    pm = ext.PMSine(); pm.hertz = fix(row(220, 440)); pm.index = fix([[1.0]]); pm.mod = unison_node(row(110, 220))
    none_with(pm)
    w = ext.Wavetable(); w.hertz = fix(row(220, 440))
    mw = fx.Mix(); mw.left = unison_node(row(220, 440)); mw.right = w; mw.mix = fix([[0.5]])
    none_with(mw)
    sh = ext.Shaper(); sh.input = unison_node(row(220, 440))
    none_with(sh)
    rl = ext.ResonantLowPass(); rl.input = unison_node(row(220, 440)); rl.cutoff = fix(row(500, 5000)); rl.resonance = fix([[2.0]])
    none_with(rl)


def test_unison_in_a_control_path_is_refused_with_its_reason():
    from signals_amd.engine import NotBatchable, _Batch, _ControlProgram
    u = unison_node([[3.0]])
    with pytest.raises(NotBatchable, match='unison oscillator has no block-rate program'):
        _ControlProgram((u,), 4)
    g = fx.Gain(); g.left = u; g.right = fix([[100.0]])
    with pytest.raises(NotBatchable, match='unison oscillator has no block-rate program'):
        _ControlProgram((g,), 4)
    lp = fx.LowPass(); lp.input = u; lp.cutoff = fix([[10.0]])
    with pytest.raises(NotBatchable, match='unison oscillator has no block-rate program'):
        _ControlProgram((lp,), 4, channels=1)
    batch = _Batch(types.SimpleNamespace(rate=48000), 0, 256, 4, False)
    with pytest.raises(NotBatchable, match='unison oscillator has no block-rate schedule'):
        batch._control_node(u, 'hertz')


# ---------------------------------------------------------------------------------------------- specialised build
def test_flags_name_the_unison_variant_exactly_for_programs_with_the_word():
    uni = [('OscUni', 2, 0, 0, -1), ('Filter', 0, 0, 0, 0)]
    f = specialise.flags(uni, 1, 0, 1, 0, 2, 2)
    assert '-DSIG_VP_S_UNI=1' in f and '-DSIG_VP_S_TAB=1' not in f and '-DSIG_VP_S_RES=1' not in f
    assert {'-DSIG_VP_STATIC_CODE={0xf0050,0x1}', '-DSIG_VP_S_NO=1', '-DSIG_VP_S_NF=1', '-DSIG_VP_S_EXT=0'} <= set(f)
    for other in ([('Osc', 2, 0, 0, 0), ('Filter', 0, 0, 0, 0)], [('OscTable', 0, 0, 0, -1)], [('Osc', 0, 0, 0, 0), ('FilterQ', 0, 0, 0, -1)],
                  [('Osc', 0, 0, 0, 0), ('OscPM', 0, 1, 0, 0)]):
        assert not any('SIG_VP_S_UNI' in x for x in specialise.flags(other, 2, 1, 1, 0, 2, 2)), other
    # the image does not depend on the copies: they are no part of what it is built from
    assert 'copies' not in specialise.flags.__code__.co_varnames and 'unison' not in specialise.flags.__code__.co_varnames


@pytest.mark.skipif(specialise.hipcc() is None, reason='no hipcc in this environment')
def test_the_specialised_unison_program_builds(tmp_path, monkeypatch):
    monkeypatch.setattr(specialise, 'CACHE', tmp_path)
    code = [('OscUni', 2, 0, 0, 0), ('Filter', 0, 0, 0, 0), ('Gain', 0, 1, 0, 0)]
    image = specialise.build(code, 1, 2, 1, 0, 2, 2)
    assert b'sig_vp_specialised' in image and b'sig_vp_specialised_info' in image


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize('kind', KINDS)
def test_reference_restatement_against_a_direct_loop(kind):
    from oracle import chain_ref as R
    rng = np.random.default_rng(4)
    copies = np.stack([rng.uniform(-0.12, 0.12, 5), rng.uniform(0, 1, 5)], axis=1)
    # the restatement and the node state the same definition: the node's docstring carries the loop below line by line, the
    # restatement's defaults are the node's, and the node takes the layout the loop runs
    doc = ext.UnisonOsc.__doc__
    for line in ('r_u = 1.0 + spread[v] * d[u]', 'h_u = hertz[v] * r_u', 'q_u = phase[v] + p[u]', 't_u = frame_range / rate * h_u + q_u',
                 's   = ((w(t_0) + w(t_1)) + w(t_2)) + ...', 'out = s / U'):
        assert line in doc, line
    n = NODES[kind]()
    assert n.kind() == kind and np.array_equal(n.get_state().copies, UR.default_copies()) and ext.UNISON_DETUNE == UR.DETUNE
    n.get_state().copies = copies
    assert np.array_equal(n.host_copies(), copies)
    hz, ph, sp = rng.uniform(55, 1760, (1, 3)), rng.uniform(0, 1, (1, 3)), rng.uniform(0, 1, (1, 3))
    got = UR.unison(kind, copies, 50, 6, hz, ph, sp)
    assert got.shape == (6, 3) and got.dtype == np.float64
    for r in range(6):
        for v in range(3):
            s = None
            for d, p in copies.tolist():
                t = np.float64(50 + r) / 48000 * (hz[0, v] * (1.0 + sp[0, v] * d)) + (ph[0, v] + p)
                w = float(R.osc_wave(kind, np.float64(t)))
                s = w if s is None else s + w
            assert got[r, v] == s / 5, (r, v)
    one = UR.unison(kind, np.array([[0, 0]]), 50, 6, hz, ph, sp)              # one copy without detune: the plain oscillator's bits
    assert np.array_equal(one, R.osc(kind, 50, 6, 48000, hz, ph))


def test_reference_renders_blocks_with_per_block_rows_and_as_an_oracle_node():
    from oracle import chain_ref as R
    copies = NODES['Sawtooth']().get_state().copies                           # the node's own default layout
    assert np.array_equal(copies, UR.default_copies())
    hertz = np.array([[100.0, 200.0], [300.0, 400.0]])
    got = UR.unison('Sawtooth', copies, 50, 4, hertz, phase=[[0.25]], spread=[[0.5]], blocks=2)
    n = R.frame_range(50, 8)
    want = np.concatenate([UR.unison_sum('Sawtooth', n[:4], 48000, hertz[:1], 0.25, 0.5, copies),
                           UR.unison_sum('Sawtooth', n[4:], 48000, hertz[1:], 0.25, 0.5, copies)])
    assert np.array_equal(got, want) and abs(got).max() <= 1.0
    node = UR.UnisonOsc('Sawtooth', copies, R.Fixed(hertz[:1]), R.Fixed([[0.25]]), R.Fixed([[0.5]]))
    assert np.array_equal(R.render(node, 50, 4, 2), want[:4])
    silent = UR.UnisonOsc('Sine', copies, R.Fixed(hertz[:1]))                 # spread unplugged: every copy at hertz, offsets apart
    assert np.array_equal(R.render(silent, 0, 4, 2), UR.unison('Sine', copies, 0, 4, hertz[:1]))
    assert math.isclose(float(np.mod(np.arange(7) * 0.6180339887498949, 1.0)[1]), 0.6180339887498949)
