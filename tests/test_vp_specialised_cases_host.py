"""The cases of tests/test_gpu_vp_specialised.py (tests/vp_specialised_cases.py), checked without a GPU: that the table is complete,
that every voice is the program, the image and the geometry the GPU test says it renders, that the images build, and that the new
inputs can tell a wrong kernel from a right one.

    - census: every family in every group it is listed for, the image count inside the cap;
    - programs: every voice compiles to its family's interpreter variant (what the twin render of the GPU test runs);
    - flags: specialise.flags of every image has exactly its family's switches, SIG_VP_S_EXT=1 for the `full` voices, and the forced
      voices per lane and sink;
    - the four-per-lane voices have no filter and no temporary, to the store and under a bus;
    - geometry: under set_voice_program_tuning sig_voice_program_geometry answers every cell's (voices per lane, span), four voices per
      lane included where the store is 16-byte aligned, and refuses four where it is not;
    - builds: one image per family is cross-compiled for gfx950 into a temporary cache;
    - sensitivity of the four-per-lane voices: the oracle of voice v + 1's parameter rows in voice v's column -- a lane that mixed up
      its four voices -- and the oracle one frame late differ from the true one by at least 10 x the GPU test's tolerance in every
      block.  For the voices shared with the span cases tests/test_vp_span_cases_host.py shows the same of a chain started one row
      late and of a control row not reloaded.

The factor 10 is a condition on the inputs, not a measurement of any kernel.  Each check prints the ratios it measured."""
import concurrent.futures
import re
import time

import numpy as np
import pytest

import vp_span_cases as C
import vp_specialised_cases as S
from test_gpu_mixed import tolerance
from test_gpu_vp_variants import FAMILIES, WORDS, scale

FACTOR = 10.0


def test_the_table_is_complete():
    cases = S.voices()
    assert len(cases) == len(set(cases)) == 13 + 13 + 5 + 7 and len(FAMILIES) == 13
    for kind in ('full', 'swept'):
        assert [f for k, f in cases if k == kind] == list(FAMILIES), kind
    assert [f for k, f in cases if k == 'deep'] == list(C.DEEP) and len(C.DEEP) == 5
    assert [f for k, f in cases if k == 'four'] == list(S.FOUR) == ['plain', 'pm', 'table', 'shape', 'unison', 'blep', 'sync']
    assert set(S.SWITCHES) == set(FAMILIES) and set(S.CELLS) == set(S.KINDS) == {k for k, _ in cases}
    assert S.CELLS['swept'] == S.CELLS['deep'] and len(S.CELLS['full']) == 2 and len(S.CELLS['four']) == 2
    assert all(vpl == 4 for vpl, _, _ in S.CELLS['four']) and not any(vpl == 4 for kind in ('full', 'swept', 'deep') for vpl, _, _ in S.CELLS[kind])
    assert all(span > 1 for kind in S.KINDS for _, span, _ in S.CELLS[kind])
    assert all({sink for _, _, sink in S.CELLS[kind]} == {'store', 'bus2'} for kind in S.KINDS)
    images = S.images()
    assert len(images) == S.IMAGES == 26 + 52 + 20 + 14 <= S.MAX_IMAGES == 120
    assert len(S.cells()) == S.IMAGES                                         # (no two long cells of a voice share an image)
    # the fresh and the short render run on images the deep voices already have
    have = {(vpl, sink) for vpl, _, sink in S.CELLS['deep']}
    assert {(C.FRESH[2][0], sink) for sink in S.SINKS} <= have and set(C.SHORT_CELLS) <= have
    assert S.V4 % 4 == 0 and S.V4 > 64 and S.V4 % 64 != 0 and -(-S.V4 // 4) == 17


@pytest.mark.parametrize('kind,family', S.voices())
def test_every_voice_compiles_to_its_familys_variant(kind, family):
    from signals_amd import _native
    from signals_amd.engine import _VoiceProgram
    prog = _VoiceProgram.compile(None, S.build(kind, family)[0], S.width(kind), mixed=True)
    assert prog is not None, (kind, family)
    counts = (len(prog.oscs), len(prog.params), len(prog.filters), prog.n_temps)
    assert _native.voice_program_variant(prog.code, *counts) == S.variant(kind, family), (kind, family, prog.code, counts)
    assert S.launched(kind, family, 'store').code == prog.code
    words = [op for op, *_ in prog.code]
    if family in WORDS:
        have, have_not = WORDS[family]
        assert all(w in words for w in have) and not any(w in words for w in have_not), (kind, family, words)
    if kind == 'deep':
        assert prog.depth == 2, (family, prog.depth)


@pytest.mark.parametrize('family', S.FOUR)
def test_the_four_per_lane_voices_keep_no_filter_state_and_no_temporaries(family):
    """what engine/voice_program.py asks before it asks for the four-per-lane image; under a bus the Gain is the bus's"""
    store, bus = S.launched('four', family, 'store'), S.launched('four', family, 'bus2')
    for prog in (store, bus):
        assert not prog.filters and prog.n_temps == 0 and prog.depth == 0, (family, prog.code)
    assert store.code[-1][0] == 'Gain' and store.code[:-1] == bus.code, (family, store.code, bus.code)
    assert len(store.params) == len(bus.params) + 1


@pytest.mark.parametrize('kind,family,vpl,sink', S.images())
def test_every_image_is_built_with_its_familys_switches(kind, family, vpl, sink):
    from signals_amd import specialise
    flags = specialise.flags(*S.image_args(kind, family, vpl, sink))
    on = {m.group(1): m.group(2) for f in flags if (m := re.fullmatch(r'-DSIG_VP_S_([A-Z]+)=(\d+)', f))}
    switches = {name for name in S.ALL_SWITCHES if name in on}
    assert all(on[name] == '1' for name in switches)
    assert switches == set(S.SWITCHES[family]), (kind, family, flags)
    words = {op for op, *_ in S.image_args(kind, family, vpl, sink)[0]}
    extended = bool(words & {'Amp', 'Adsr', 'Noise'})
    assert on['EXT'] == str(int(extended)) and (kind != 'full' or on['EXT'] == '1'), (kind, family, flags)
    assert f'-DSIG_VP_STATIC_VPT={vpl}' in flags and f'-DSIG_VP_STATIC_C={S.SINKS[sink]}' in flags
    assert f'-DSIG_VP_STATIC_WAVES={ {1: 3, 2: 2, 4: 1}[vpl] }' in flags
    assert sum(f.startswith('-DSIG_VP_STATIC_CODE={') for f in flags) == 1


def test_the_geometry_answers_every_cell():
    from signals_amd import _native
    geometry = _native.voice_program_geometry
    try:
        for kind, family, vpl, span, sink in S.cells():
            depth = S.launched(kind, family, sink).depth
            _native.set_voice_program_tuning(vpl, span)
            for K in C.KS:
                got = geometry(S.width(kind), C.N, K, C.CONTEXT, depth, S.SINKS[sink], S.aligned(kind), specialised=(vpl == 4))
                assert got == (vpl, span), (kind, family, sink, K, got)
            if vpl == 4:
                # not without the image at hand; to the store not on an 8-byte aligned one (a bus takes four either way)
                assert geometry(S.V4, C.N, C.KS[0], C.CONTEXT, depth, S.SINKS[sink], 4, specialised=False)[0] != 4
                if sink == 'store':
                    assert geometry(S.V4, C.N, C.KS[0], C.CONTEXT, depth, 0, 2, specialised=True)[0] != 4
                    assert geometry(S.V4 - 2, C.N, C.KS[0], C.CONTEXT, depth, 0, 2, specialised=True)[0] != 4
                # the interpreter's twin of the cell runs at two per lane
                _native.set_voice_program_tuning(2, span)
                assert geometry(S.V4, C.N, C.KS[0], C.CONTEXT, depth, S.SINKS[sink], 4)[0] == 2
        for family in C.DEEP:
            position, K, (vpl, span) = C.FRESH
            _native.set_voice_program_tuning(vpl, span)
            for sink in S.SINKS:
                assert geometry(C.V, C.N, K, C.CONTEXT, 2, S.SINKS[sink], 2) == (vpl, span), (family, sink)
        for family in C.SHORT_DEEP:
            for vpl, sink in C.SHORT_CELLS:
                _native.set_voice_program_tuning(vpl, 0)                       # (short blocks: the span is 1 whatever is asked)
                assert geometry(C.V, C.SHORT_N, C.SHORT_K, C.CONTEXT, 2, S.SINKS[sink], 2) == (vpl, 1), (family, vpl, sink)
    finally:
        _native.set_voice_program_tuning(0, 0)


def test_one_image_per_family_builds(tmp_path, monkeypatch):
    """the `full` voice of every family at two voices per lane under the bus: extended handlers, lane pairs and bus flush in one
    image.  Cross-compiled for gfx950 into an empty cache, at most 8 at a time"""
    from signals_amd import specialise
    if specialise.hipcc() is None:
        pytest.skip('no hipcc on this machine: nothing to specialise with')
    monkeypatch.setattr(specialise, 'CACHE', tmp_path)
    jobs = [S.image_args('full', family, 2, 'bus2') for family in FAMILIES]
    t0 = time.perf_counter()
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
        built = list(pool.map(lambda args: specialise.build(*args), jobs))
    print('vp specialised host:', len(built), 'images built in', round(time.perf_counter() - t0, 1), 's')
    # (hipcc --genco writes an offload bundle around the gfx950 code object)
    assert len(built) == 13 and all(b'\x7fELF' in image and b'gfx950' in image[:4096] for image in built)
    assert len(set(built)) == 13 and len(list(tmp_path.glob('vp_*.hsaco'))) == 13 and not list(tmp_path.glob('*.tmp'))


def block_ratios(a, b, tol):
    """max |a - b| / tol per block of the long render"""
    return np.abs(a - b).reshape(-1, C.N, a.shape[1]).max(axis=(1, 2)) / tol


@pytest.mark.parametrize('family', S.FOUR)
def test_a_neighbours_rows_or_a_late_frame_show_in_every_block(family):
    want = S.oracle(S.four(family)[1], 'four', 'long')
    assert want.shape == (sum(C.KS) * C.N, S.V4) and np.isfinite(want).all()
    bus = want @ S.pan('four').T
    tol, bus_tol = tolerance(want) * scale(family), tolerance(bus) * scale(family)
    wrong = {'the next voice\'s rows': S.oracle(S.four(family, shift=1)[1], 'four', 'long'),
             'one frame late': S.oracle(S.four(family)[1], 'four', 'long', position=C.POSITION + 1)}
    assert np.array_equal(wrong['the next voice\'s rows'], np.roll(want, -1, axis=1))      # (a voice is a function of its own column)
    for what, rows in wrong.items():
        ratio, bus_ratio = block_ratios(rows, want, tol), block_ratios(rows @ S.pan('four').T, bus, bus_tol)
        print('vp specialised four', family, what, 'err/tol per block', np.round(ratio, 1), 'under the bus', np.round(bus_ratio, 1))
        assert ratio.size == sum(C.KS) and (ratio >= FACTOR).all() and (bus_ratio >= FACTOR).all(), (family, what, ratio, bus_ratio)
