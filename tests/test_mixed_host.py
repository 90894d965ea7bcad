"""Mixed voice programs without a GPU: the `mixed` keyword of _VoiceProgram on the seven patches of tests/mixed_patches.py (exact
words, slot counts, what the program carries), the refusals that stay without it, the family helper of _native, the flag list of
the specialised build (SIG_VP_S_MIXED for combined programs only; every other list what it was), the C entry
sig_voice_program_mixed -- what it still refuses, and that sig_voice_program_unison refuses combined programs as before; its accepting
calls carry no blocks, return before the program is looked at and show the symbol and its signature only (tests/test_gpu_mixed.py shows
that combined programs pass the checks and run) -- the engine's policy for such programs, and the specialised image of one of them."""
import ctypes
import types

import numpy as np
import pytest

from signals_amd import _native, specialise

import mixed_patches as MP

INV = 1     # hipErrorInvalidValue
V = 8
SAW, SINE = MP.SAW, MP.SINE


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


def voice(which, **kw):
    """the per-voice graph of a patch: under a SumBus the bus's input"""
    top, _, C = MP.patch(which, MP.draw(V), **kw)
    return top.input.sig if C == 2 else top


#          patch: (words, (oscs, params, filters, temps, depth), families, unison?, tables, resonant slots)
EXPECTED = {
    'supersaw': ([('OscUni', SAW, 0, 0, 0), ('FilterQ', 0, 0, 0, 1)], (1, 2, 1, 0, 1), ('resonant', 'unison'), True, 0, 1),
    'supersaw_bus': ([('OscUni', SAW, 0, 0, 0), ('FilterQ', 0, 0, 0, 1), ('Save', 0, 0, 0, 0), ('Adsr', 0, 0, 0, 0), ('Mul', 0, 0, 0, 0)],
                     (1, 2, 1, 1, 1), ('resonant', 'unison'), True, 0, 1),
    'overdrive': ([('Osc', SAW, 0, 0, 0), ('FilterQ', 0, 0, 0, 0), ('Shape', 0, 0, 0, -1)], (1, 1, 1, 0, 1), ('table', 'resonant'), False, 1, 1),
    'pad': ([('OscTable', 0, 0, 0, 0), ('FilterQ', 0, 0, 0, 1)], (1, 2, 1, 0, 1), ('table', 'resonant'), False, 1, 1),
    'bell': ([('Osc', SINE, 0, 0, 0), ('OscPM', SINE, 1, 0, 0), ('FilterQ', 0, 0, 0, 1)], (2, 2, 1, 0, 1), ('pm', 'resonant'), False, 0, 1),
    'wah': ([('OscTable', 0, 0, 0, 0), ('Band', 0, 0, 0, 0)], (1, 1, 2, 0, 1), ('band', 'table'), False, 1, 0),
    'three': ([('OscUni', SAW, 0, 0, 0), ('FilterQ', 0, 0, 0, 1), ('Shape', 0, 0, 0, -1)], (1, 2, 1, 0, 1), ('table', 'resonant', 'unison'), True, 1, 1),
}


@pytest.mark.parametrize('which', MP.PATCHES)
def test_the_patches_compile_with_mixed_and_only_with_it(which):
    from signals_amd.engine import _VoiceProgram
    code, counts, families, unison, tables, resonant = EXPECTED[which]
    prog = _VoiceProgram(None, voice(which), V, mixed=True)
    assert prog.code == code
    assert (len(prog.oscs), len(prog.params), len(prog.filters), prog.n_temps, prog.depth) == counts
    assert prog.families == families and _native.vp_families(prog.code) == families
    assert (prog.unison is not None) == unison and len(prog.tables) == tables and len(prog.resonant) == resonant
    assert (len(prog.bands) == 1) == ('band' in families) and prog.mixed
    same = _VoiceProgram.compile(None, voice(which), V, mixed=True)
    assert same is not None and same.code == code
    # the guard: without the keyword the graph is no program, as before
    assert _VoiceProgram.compile(None, voice(which), V) is None
    with pytest.raises(Exception, match='no interpreter variant has both'):
        _VoiceProgram(None, voice(which), V)
    with pytest.raises(Exception, match='no interpreter variant has both'):
        _VoiceProgram(None, voice(which), V, mixed=False)


def test_three_copies_and_a_program_of_one_family():
    from signals_amd.engine import _VoiceProgram
    copies = MP.draw(V)['copies3']
    prog = _VoiceProgram(None, voice('supersaw', copies=copies), V, mixed=True)
    assert prog.unison.get_state().copies is copies and prog.unison.host_copies().shape == (3, 2)
    # a program of one family is the same program with the keyword and without it
    from helpers import fix
    from signals_amd.chain import ext
    rl = ext.ResonantLowPass(); rl.input = MP.mkosc('Sawtooth', np.full((1, V), 220.0)); rl.cutoff = fix(np.full((1, V), 900.0))
    a, b = _VoiceProgram(None, rl, V), _VoiceProgram(None, rl, V, mixed=True)
    assert a.code == b.code == [('Osc', SAW, 0, 0, 0), ('FilterQ', 0, 0, 0, -1)] and a.families == b.families == ('resonant',)


def test_families_and_words():
    assert set(_native.VP_FAMILIES) == {'band', 'pm', 'table', 'resonant', 'unison'}
    assert _native.VP_FAMILIES['table'] is _native.VP_TABLE_OPS and _native.VP_FAMILIES['resonant'] is _native.VP_RES_OPS
    assert _native.VP_FAMILIES['unison'] is _native.VP_UNI_OPS
    assert _native.vp_families([('Osc', 0, 0, 0, 0), ('Filter', 0, 0, 0, 0), ('Gain', 0, 0, 0, 0)]) == ()
    assert _native.vp_families([('OscTable', 0, 0, 0, -1), ('Shape', 0, 0, 1, -1)]) == ('table',)      # one family, two words
    assert _native.vp_families([('Osc', 0, 0, 0, 0), ('OscPM', 0, 1, 0, 0), ('Band', 0, 0, 0, 0)]) == ('band', 'pm')
    # words: op | kind << 5 | a << 8 | b << 12 | c << 16, c = -1 as 15
    words = _native.voice_program_words(EXPECTED['three'][0])
    assert words == [0x00050, 0x1000f, 0xf000e]
    back = [(w & 31, (w >> 5) & 7, (w >> 8) & 15, (w >> 12) & 15, (w >> 16) & 15) for w in words]
    assert back == [(_native.VP_OPS[op], kind, a, b, c & 15) for op, kind, a, b, c in EXPECTED['three'][0]]
    assert _native.voice_program_words(EXPECTED['wah'][0]) == [0x0000d, 0x0000b]
    assert 'sig_voice_program_mixed' in _native.EXPORTS
    header = (_native.LIB_PATH.parent.parent.parent / 'include' / 'signals_amd.h').read_text()
    assert 'int sig_voice_program_mixed(' in header and '#define SIG_ABI_VERSION 7' in header


def test_flags_name_the_mixed_build_for_combined_programs_only():
    for which in MP.PATCHES:
        code, (no, np_, nf, nt, _), *_ = EXPECTED[which]
        f = specialise.flags(code, no, np_, nf, nt, 1, 0)
        assert f[-1] == '-DSIG_VP_S_MIXED=1' and f.count('-DSIG_VP_S_MIXED=1') == 1, which
    f = specialise.flags(EXPECTED['supersaw'][0], 1, 2, 1, 0, 1, 0)
    assert f == ['-DSIG_VP_STATIC_CODE={0x50,0x1000f}', '-DSIG_VP_S_NF=1', '-DSIG_VP_S_NO=1', '-DSIG_VP_S_NP=2', '-DSIG_VP_S_NT=0',
                 '-DSIG_VP_S_EXT=0', '-DSIG_VP_STATIC_VPT=1', '-DSIG_VP_STATIC_C=0', '-DSIG_VP_STATIC_WAVES=3', '-DSIG_VP_S_RES=1',
                 '-DSIG_VP_S_UNI=1', '-DSIG_VP_S_MIXED=1']
    # every other program: the list of the commit before this option existed, literally (so cache keys and images stay)
    plain = [('Osc', 2, 0, 0, 0), ('Filter', 0, 0, 0, 0), ('Gain', 0, 0, 0, 0)]
    assert specialise.flags(plain, 1, 1, 1, 0, 2, 2) == [
        '-DSIG_VP_STATIC_CODE={0x40,0x1,0x2}', '-DSIG_VP_S_NF=1', '-DSIG_VP_S_NO=1', '-DSIG_VP_S_NP=1', '-DSIG_VP_S_NT=0', '-DSIG_VP_S_EXT=0',
        '-DSIG_VP_STATIC_VPT=2', '-DSIG_VP_STATIC_C=2', '-DSIG_VP_STATIC_WAVES=2']
    uni = [('OscUni', 2, 0, 0, 0), ('Filter', 0, 0, 0, 0)]
    assert specialise.flags(uni, 1, 1, 1, 0, 1, 0) == [
        '-DSIG_VP_STATIC_CODE={0x50,0x1}', '-DSIG_VP_S_NF=1', '-DSIG_VP_S_NO=1', '-DSIG_VP_S_NP=1', '-DSIG_VP_S_NT=0', '-DSIG_VP_S_EXT=0',
        '-DSIG_VP_STATIC_VPT=1', '-DSIG_VP_STATIC_C=0', '-DSIG_VP_STATIC_WAVES=3', '-DSIG_VP_S_UNI=1']
    tab = [('OscTable', 0, 0, 0, -1), ('Shape', 0, 0, 1, 0)]
    assert specialise.flags(tab, 1, 1, 0, 0, 2, 1) == [
        '-DSIG_VP_STATIC_CODE={0xf000d,0x100e}', '-DSIG_VP_S_NF=1', '-DSIG_VP_S_NO=1', '-DSIG_VP_S_NP=1', '-DSIG_VP_S_NT=0', '-DSIG_VP_S_EXT=0',
        '-DSIG_VP_STATIC_VPT=2', '-DSIG_VP_STATIC_C=1', '-DSIG_VP_STATIC_WAVES=2', '-DSIG_VP_S_TAB=1']


# ---------------------------------------------------------------------------------------------- the C entry
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


def test_the_mixed_entry_accepts_combined_programs_and_keeps_every_other_check(lib):
    buf = (ctypes.c_float * 64)()
    seven = _native.VpUnisonT(); seven.copies = 7

    def tables(*geometry):
        t = _native.VpTablesT()
        t.n_tables = len(geometry)
        for k, (ptr, points, waves) in enumerate(geometry):
            t.table[k] = _native.VpTable(ptr, points, waves)
        return t

    def run(entry, code, uni=seven, tabs=None, nblocks=0, **kw):
        """nblocks 0: the arguments of the call itself are checked, then it returns 0 without looking at the program (no launch
        without a GPU); nblocks > 0: the program's checks run too, and what they refuse returns before any device work"""
        P, keep = _program(code, **kw)
        control_rows = 1 + nblocks
        return getattr(lib, entry)(ctypes.byref(P), 48000, 0, 256, nblocks, 100, 8, control_rows, 0, None, 0, None, 0, 0, None,
                                   ctypes.addressof(buf), 8, None, None, ctypes.byref(tabs) if tabs is not None else None,
                                   ctypes.byref(uni) if uni is not None else None)
    uni, fq = ('OscUni', 2, 0, 0, -1), ('FilterQ', 0, 0, 0, -1)
    t64 = tables((64, 64, 2))
    combined = [
        dict(code=[uni, fq], types=['rlp']),
        dict(code=[('OscTable', 0, 0, 0, -1), fq], types=['rlp'], tabs=t64),
        dict(code=[('Osc', 2, 0, 0, 0), fq, ('Shape', 0, 0, 0, -1)], types=['rlp'], tabs=t64),
        dict(code=[('Osc', 0, 0, 0, 0), ('OscPM', 0, 1, 0, 0), fq], types=['rlp'], n_oscs=2),
        dict(code=[uni, ('Band', 0, 0, 0, 0)], types=['bp', 'bp']),
    ]
    for case in combined:
        assert run('sig_voice_program_mixed', **case) == 0, case['code']                      # (the symbol and its signature: see the docstring)
        assert run('sig_voice_program_unison', nblocks=256, **case) == INV, case['code']      # the old entries: as before
    # what the mixed entry still refuses (a launch's worth of blocks, so that the program is looked at)
    mixed = lambda **case: run('sig_voice_program_mixed', nblocks=256, **case)
    assert mixed(code=[uni, fq], types=['lp']) == INV                         # a FilterQ word on a Butterworth slot
    assert mixed(code=[uni, ('Filter', 0, 0, 0, 0)], types=['rlp']) == INV    # a resonant slot without its word
    assert mixed(code=[uni, ('Band', 0, 0, 0, 0), ('Filter', 0, 2, 0, 0)], types=['bp', 'bp', 'rlp']) == INV
    assert mixed(code=[uni, fq], types=['rlp'], uni=None) == INV              # OscUni without the copies
    assert mixed(code=[('OscTable', 0, 0, 0, -1), fq], types=['rlp'], tabs=tables((64, 48, 2))) == INV      # not a power of two
    assert mixed(code=[('OscTable', 0, 0, 0, -1), fq], types=['rlp']) == INV  # the word without its tables
    assert mixed(code=[('OscTable', 0, 0, 0, -1), fq], types=['rlp'], tabs=tables((64, 16384, 2))) == INV   # past the table cap
    assert mixed(code=[uni, ('Band', 0, 0, 0, 0)], types=['bp', 'bs']) == INV  # a band pair of two types
    bad = _native.VpUnisonT(); bad.copies = 17
    assert run('sig_voice_program_mixed', code=[uni, fq], types=['rlp'], uni=bad) == INV


# ---------------------------------------------------------------------------------------------- policy
def test_worthwhile_treats_mixed_programs_like_any_other():
    """the measured policy (tools/time_mixed.py): the small-file rule extends to mixed programs"""
    from signals_amd.engine import _VoiceProgram
    batch = lambda special, N: types.SimpleNamespace(owner=types.SimpleNamespace(specialise=special), N=N, _pure={})
    prog = lambda which, b: _VoiceProgram(b, voice(which), V, mixed=True)
    for which in ('supersaw', 'overdrive', 'pad', 'bell', 'wah', 'three'):   # each fits the interpreter's small register file
        assert prog(which, batch(False, 256)).worthwhile(), which
    full = 'supersaw_bus'                                                     # an ADSR: the full register file, one wave per SIMD
    assert not prog(full, batch(False, 256)).worthwhile()                     # interpreted: loses to the per-node schedule
    assert prog(full, batch(False, 64)).worthwhile()                          # blocks shorter than the context behind a filter: nothing else batches
    assert not prog(full, batch('background', 256)).worthwhile()              # (the interpreter renders meanwhile: its policy)
    if specialise.hipcc() is not None:
        assert prog(full, batch(True, 256)).worthwhile()                      # the kernel built for the program
    from signals_amd.engine import BatchRenderer
    assert BatchRenderer(voice('supersaw'), V).mixed_programs is False        # opt-in
    assert BatchRenderer(voice('supersaw'), V, mixed_programs=True).mixed_programs is True


@pytest.mark.skipif(specialise.hipcc() is None, reason='no hipcc in this environment')
def test_the_specialised_mixed_program_builds(tmp_path, monkeypatch):
    monkeypatch.setattr(specialise, 'CACHE', tmp_path)
    code, (no, np_, nf, nt, _), *_ = EXPECTED['three']                        # three families: tables and copies in one parameter
    image = specialise.build(code, no, np_, nf, nt, 2, 2)
    assert len(image) > 0 and b'sig_vp_specialised' in image and b'sig_vp_specialised_info' in image
