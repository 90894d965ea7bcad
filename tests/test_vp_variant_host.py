"""Which interpreter kernel a voice program gets, without a GPU: sig_voice_program_variant answers with the selection function the
launch itself calls (voice_program.hip vp_variant / fits_small), so the family and the register file of a program can be pinned on
the host.  The programs are those of the families' host tests (test_specialise_build.py, test_band_program_host.py, test_pm_host.py,
test_shaper_host.py, test_resonant_host.py, test_unison_host.py, test_blep_host.py, test_mixed_host.py).

The last part keeps the cell table of tests/test_gpu_vp_variants.py complete: its family list against the VpLaunch instantiations
declared in sig_vp_launch.h, and the voices it renders for the second kernel sets (resonant_eq, mixed_eq, sync, mixed_sync) -- their
programs, variants, register files and the oracle's own distance to the cells' tolerance."""
import itertools

import pytest

from signals_amd import _native

from test_mixed_host import EXPECTED as MIXED_PATCHES

SAW = 2

#   family: (words, (oscs, params, filters, temps))
PROGRAMS = {
    'plain': ([('Osc', 2, 0, 0, 0), ('Filter', 0, 0, 0, 0), ('Save', 0, 0, 0, 0), ('Osc', 3, 1, 0, 0), ('Filter', 0, 1, 0, 0), ('Mul', 0, 0, 0, 0)],
              (2, 0, 2, 1)),
    'band': ([('Osc', 2, 0, 0, 0), ('Band', 0, 0, 0, 0)], (1, 0, 2, 0)),
    'pm': ([('Osc', 0, 0, 0, 0), ('OscPM', 2, 1, 0, 0), ('Filter', 0, 0, 0, 0)], (2, 1, 1, 0)),
    'table': ([('OscTable', 0, 0, 0, -1), ('Filter', 0, 0, 0, 0)], (1, 0, 1, 0)),
    'shape': ([('Osc', 2, 0, 0, 0), ('Shape', 0, 0, 0, 0), ('Gain', 0, 1, 0, 0)], (1, 2, 0, 0)),
    'resonant': ([('Osc', 2, 0, 0, 0), ('FilterQ', 0, 0, 0, 0), ('Filter', 0, 1, 0, 0), ('Gain', 0, 1, 0, 0)], (1, 2, 2, 0)),
    'unison': ([('OscUni', 2, 0, 0, 0), ('Filter', 0, 0, 0, 0), ('Gain', 0, 1, 0, 0)], (1, 2, 1, 0)),
    'blep': ([('OscBlep', SAW, 0, 0, -1), ('Filter', 0, 0, 0, 0)], (1, 0, 1, 0)),
    'mixed': (MIXED_PATCHES['supersaw'][0], MIXED_PATCHES['supersaw'][1][:4]),
}
# one word of each family of which a single-family variant has at most one (slots inside the small register file)
FAMILY_WORD = {'band': ('Band', 0, 0, 0, 0), 'pm': ('OscPM', 0, 1, 0, 0), 'table': ('OscTable', 0, 0, 0, -1),
               'resonant': ('FilterQ', 0, 0, 0, -1), 'unison': ('OscUni', SAW, 0, 0, -1)}


@pytest.fixture(scope='module')
def lib():
    if not _native.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return _native.lib()


def variant(code, counts):
    """(family, small register file?) of a program -- and, for every program this file asks about, the agreement with the Python table:
    words of two or more of VP_FAMILIES <=> the MIXED variant"""
    oscs, params, filters, temps = counts
    family, small = _native.voice_program_variant(list(code), oscs, params, filters, temps)
    assert (len(_native.vp_families(list(code))) >= 2) == (family == 'mixed'), code
    return family, small


def test_the_names_mirror_the_header():
    header = (_native.LIB_PATH.parent.parent.parent / 'include' / 'signals_amd.h').read_text()
    for value, name in enumerate(_native.VP_VARIANTS):
        assert f'SIG_VP_FAMILY_{name.upper()} = {value}' in header, name
    assert 'int sig_voice_program_variant(' in header and 'sig_voice_program_variant' in _native.EXPORTS
    assert tuple(PROGRAMS) == _native.VP_VARIANTS


@pytest.mark.parametrize('family', list(PROGRAMS))
def test_family_per_program(lib, family):
    code, counts = PROGRAMS[family]
    assert variant(code, counts) == (family, True)


def test_small_file(lib):
    """inside VpLimits<true> (two filter slots, three oscillators, four parameters, one temporary, no Amp / ADSR / White): the small
    register file; one Amp word, or a second temporary, and the same program takes the full one"""
    code, (oscs, params, filters, temps) = PROGRAMS['plain']
    assert variant(code, (oscs, params, filters, temps)) == ('plain', True)
    assert variant(code + [('Amp', 0, 0, 0, 0)], (oscs, params + 1, filters, temps)) == ('plain', False)
    assert variant(code, (oscs, params, filters, 2)) == ('plain', False)
    for word in ('Adsr', 'Noise'):                                            # the other two extended handlers
        assert variant(code + [(word, 0, 0, 0, 0)], (oscs, params, filters, temps)) == ('plain', False)
    # each slot count at the limit and one past it
    assert variant(code, (3, 4, 2, 1)) == ('plain', True)
    for past in ((4, 4, 2, 1), (3, 5, 2, 1), (3, 4, 3, 1)):
        assert variant(code, past) == ('plain', False), past
    # the register file does not depend on the family
    for family, (code, counts) in PROGRAMS.items():
        assert variant(code + [('Amp', 0, 0, 0, 0)], counts) == (family, False), family


def test_blep_with_unison_is_blep(lib):
    code = [('OscUni', SAW, 0, 0, -1), ('Save', 0, 0, 0, 0), ('OscBlep', SAW, 1, 0, -1), ('Mul', 0, 0, 0, 0)]
    assert variant(code, (2, 0, 0, 1)) == ('blep', True)
    assert variant(code[:1], (1, 0, 0, 0)) == ('unison', True)


def test_shape_with_table_is_shape(lib):
    code = [('OscTable', 0, 0, 0, -1), ('Shape', 0, 0, 1, 0)]               # (test_mixed_host.py: one family, two words)
    assert variant(code, (1, 1, 0, 0)) == ('shape', True)
    assert variant(code[:1], (1, 0, 0, 0)) == ('table', True)


@pytest.mark.parametrize('pair', list(itertools.combinations(FAMILY_WORD, 2)), ids='+'.join)
def test_any_two_families_are_mixed(lib, pair):
    code = [('Osc', 0, 0, 0, 0)] + [FAMILY_WORD[name] for name in pair]
    assert variant(code, (2, 1, 2, 0)) == ('mixed', True)
    assert variant(list(reversed(code)), (2, 1, 2, 0)) == ('mixed', True)     # (the order of the words does not matter)
    for name in pair:                                                         # ... and either alone is its own family
        assert variant([('Osc', 0, 0, 0, 0), FAMILY_WORD[name]], (2, 1, 2, 0)) == (name, True)


@pytest.mark.parametrize('which', list(MIXED_PATCHES))
def test_the_mixed_patches_are_mixed(lib, which):
    code, counts = MIXED_PATCHES[which][0], MIXED_PATCHES[which][1][:4]
    small = not any(op in _native.VP_EXT_OPS for op, *_ in code)
    assert variant(code, counts) == ('mixed', small)


def test_shape_and_blep_on_top_of_another_family_are_mixed(lib):
    assert variant([('Osc', 0, 0, 0, 0), ('Shape', 0, 0, 0, -1), ('FilterQ', 0, 0, 0, -1)], (1, 0, 1, 0)) == ('mixed', True)
    assert variant([('OscBlep', SAW, 0, 0, -1), ('Band', 0, 0, 0, 0)], (1, 0, 2, 0)) == ('mixed', True)


# ---------------------------------------------------------------------------------------------- the cell table of test_gpu_vp_variants.py
@pytest.fixture
def cpu_device():
    from signals_amd import runtime
    old = runtime._device
    runtime.set_device('cpu')
    yield
    runtime._device = old


def test_the_cell_table_has_every_instantiated_family():
    """a family added to sig_vp_launch.h without its 12 cells (and its short-block cells) fails here, on every machine"""
    import re
    import test_gpu_vp_variants as CELLS
    header = (_native.LIB_PATH.parent / 'sig_vp_launch.h').read_text()
    names = re.findall(r'^extern template struct VpLaunch<vp_family::(\w+)>;', header, flags=re.M)
    assert len(names) == len(set(names)) == 13, names
    assert set(names) == set(CELLS.FAMILIES) and len(CELLS.FAMILIES) == len(names), (names, CELLS.FAMILIES)
    assert CELLS.FAMILIES[:len(_native.VP_VARIANTS)] == _native.VP_VARIANTS                 # the nine the C ABI names, in its order
    rest = CELLS.FAMILIES[len(_native.VP_VARIANTS):]
    assert set(rest) == set(CELLS.BASE) == set(CELLS.WORDS) and set(CELLS.BASE.values()) <= set(_native.VP_VARIANTS)


#                family: (words of the small-file voice, (oscs, params, filters, temps))
SECOND_SETS = {
    'resonant_eq': ([('Osc', SAW, 0, 0, 0), ('Gain', 0, 0, 0, 0), ('FilterEq', 0, 0, 2, 1)], (1, 3, 1, 0)),
    'mixed_eq': ([('OscUni', SAW, 0, 0, 0), ('Gain', 0, 1, 0, 0), ('FilterEq', 0, 0, 3, 2)], (1, 4, 1, 0)),
    'sync': ([('OscSync', SAW, 0, 1, 0), ('Filter', 0, 0, 0, 0)], (1, 2, 1, 0)),
    'mixed_sync': ([('OscSync', SAW, 0, 1, 0), ('FilterQ', 0, 0, 0, 2)], (1, 3, 1, 0)),
}


@pytest.mark.parametrize('full', [False, True], ids=['small', 'full'])
@pytest.mark.parametrize('family', list(SECOND_SETS))
def test_the_second_sets_voices(lib, cpu_device, family, full):
    """the eight voices the cell table adds for the _eq and _sync kernel sets: each compiles as a mixed-enabled program with the
    word that selects its set, lands in the base variant and the register file its cell claims, has a filter in series (the
    short-block cells need depth > 0), and its oracle alone stays inside the cells' tolerance at both block lengths: finite, below
    4 in magnitude (0.25 into +12 dB is 1; a resonance of 2 and the shelf's overshoot stay well under 4 times that), and the
    float32 rounding of the oracle -- half an ulp, 2^-24 |x| < 2.4e-7 for |x| < 4 -- is below 1e-6 max(1, max|oracle|)"""
    import numpy as np
    import test_gpu_vp_variants as CELLS
    from helpers import f32
    code, counts, depth = CELLS.program(family, full)
    if not full:
        assert (code, counts) == SECOND_SETS[family], (code, counts)
    else:
        assert code[:len(SECOND_SETS[family][0])] == SECOND_SETS[family][0] and 'Adsr' in [op for op, *_ in code], code
    assert depth == 1
    assert variant(code, counts) == (CELLS.BASE[family], not full)
    words = [op for op, *_ in code]
    have, have_not = CELLS.WORDS[family]
    assert all(w in words for w in have) and not any(w in words for w in have_not), words
    for frames in (CELLS.N, CELLS.SHORT_N):
        want = CELLS.wanted(family, full, frames)
        assert want.shape == (CELLS.K * frames, CELLS.V) and np.isfinite(want).all()
        peak, tol = float(np.abs(want).max()), CELLS.tolerance(want)
        rounding = float(np.abs(f32(want).astype(np.float64) - want).max())
        print('second set oracle', family, 'full' if full else 'small', frames, 'max|oracle|', peak, 'float32 rounding', rounding, 'tol', tol)
        assert peak < 4.0 and rounding < tol, (family, full, frames, peak, rounding, tol)


def test_bad_calls_are_refused(lib):
    with pytest.raises(_native.NativeError):
        _native.voice_program_variant([], 0, 0, 0, 0)                         # no words
    P = _native._program_struct(PROGRAMS['plain'][0])
    import ctypes
    out = ctypes.c_int32(0)
    assert lib.sig_voice_program_variant(None, ctypes.byref(out), ctypes.byref(out)) != 0
    assert lib.sig_voice_program_variant(ctypes.byref(P), None, ctypes.byref(out)) != 0
    assert lib.sig_voice_program_variant(ctypes.byref(P), ctypes.byref(out), None) != 0
