"""The SPECIALISED builds of the voice program (signals_amd/specialise.py: voice_program.hip compiled with one program's words, its exact
register file, the voices per lane and the sink as macros -- the code object BatchRenderer(specialise=True) launches) at what the
interpreter is held to by tests/test_gpu_vp_spans.py: more than one block per lane, for all 13 kernel families, at one, two and FOUR
voices per lane, to the store and under a 2-channel bus.  The source is the interpreter's, the code object is not: the dispatch loop is
unrolled, every switch folded, the registers allocated for one program at one to three waves per SIMD, and the four-per-lane form
exists as a specialised image only.  The cases are tests/vp_specialised_cases.py's; tests/test_vp_specialised_cases_host.py and
tests/test_vp_span_cases_host.py show on the CPU that the inputs tell a wrong kernel from a right one tenfold in every block.

Shapes.  As tests/test_gpu_vp_spans.py: 66 voices, 48 kHz, blocks of N = 130 frames ((130 - 100) % 4 = 2, (130 - 100) % 8 = 6: the
first warm row of the next block's chains falls inside a row group; every block ends in single-row groups), one BatchRenderer
rendering two consecutive batches of 3 and 4 blocks from position 0.  The four-per-lane voices are 68 wide: a 16-byte aligned store,
two voice tiles at one voice per lane and 17 live lanes at four.

Table (voices per lane, blocks per lane) and sink, by kind of voice:

    full   (the family's voice x ADSR), 13 families        (1, 2) store | (2, 3) bus
    swept  (every family control on an LFO), 13            (1, 2) store | (1, 2) bus | (2, 3) bus | (2, 16) store
    deep   (two filters in series), 5                      the same four; `fresh`: 5 blocks from position 1000 at (1, 2), both
                                                           sinks; `short` (band, resonant_eq, mixed): blocks of 32 frames at two
                                                           voices per lane under the bus and one to the store
    four   (oscillator [-> Shaper] -> Gain), 7             (4, 2) store | (4, 3) bus

112 + 10 + 6 = 128 cells on 112 images (an image is keyed by program, voices per lane and sink; the span is a run-time argument).
A module fixture builds them all up front through specialise.build, 8 at a time, into the package's ordinary cache: 112
images (110 distinct files: two pairs of voices share a program) in 14.7 s of compile time on a cold cache with 16 CPUs, 34 s with 8
(no GPU time; 0.7 s to read them back on a warm one).  A render then must not add
an image to the cache: the table's programs are the ones the engine asks for.  (The label is the engine's: it marks a launch
*specialised once the image is attached for the voices per lane IT computed, and the library finds the image by the same key for the
voices per lane the launch computes -- the geometry check in front of the render holds the two together.)

Before a render sig_voice_program_variant must name the voice's variant and sig_voice_program_geometry must answer the cell's
(voices per lane, span) for each batch size.  After it each batch must have been exactly one voice_program[ | voice_program_bus[
launch whose label ends in *specialised, with the words that select the _eq and _sync families -- and, for a swept voice, the one
control_program launch in front of it.  A missing image or the interpreter in its place fails the cell.

Three assertions on the rows.

1. Against the oracle: the float32 output within 1e-6 max(1, max|oracle|) of float32(oracle) (tests/test_gpu_mixed.py `tolerance`),
   times max(1, L) behind the Shaper (test_gpu_vp_variants.scale).  No sample is excluded.  Both sinks.

2. Against the interpreter: the same cell at the same tuning with the attached images switched off (for four voices per lane, which
   the interpreter has not, at two) -- within 2.5e-7 max(1, max|interpreter|) on the finite samples, NaN positions identical.  The
   bound is the one tests/test_gpu_specialise.py holds the plain family to: both run the same float64 operations on the same rows
   and round once to float32 (one ulp of a float32 below 2 is 1.2e-7; the compiler may order a sum or contract differently).

3. Store sink: the span render is bit for bit the render of the SAME image at (voices per lane, 1), NaN positions included.  The
   argument is assertion 2 of tests/test_gpu_vp_spans.py -- whichever lane owns a block, its chains are cold-started on the same
   row, designed from the same control row and advanced by the same per-row operations in the same order, the phase is the exact
   n / rate of each row -- and it is stronger here: both renders launch the same code object, so not even the compiler's choices
   differ.  The bus sink adds voice tiles in another order per geometry and is held to assertions 1 and 2.

Measured on an MI355X, the largest max|err| / tol over a family's cells (tol = 1e-6 max(1, max|oracle|), shape: times L): plain
2.9e-5, band 2.2e-7, pm 0.18 (the four-per-lane voice to the store: 1.79e-7 against 1e-6), table 0, shape 0, resonant 4.7e-5,
unison 0.0075, blep 0, mixed 0.00047, resonant_eq 1.1e-5, mixed_eq 0, sync 0, mixed_sync 0 -- 0: every cell of the family equals
float32(oracle) bit for bit; 102 of the 128 cells do.  Assertion 2: the largest max|specialised - interpreter| is 0 in every family
-- all 128 cells, the 14 at four voices per lane against the interpreter's two included, equal the interpreter's render bit for
bit.  Every store cell with a span above 1 was bit-equal to its span-1 render.  No cell found a fault in the kernels."""
import concurrent.futures
import functools
import time

import numpy as np
import pytest

from helpers import RATE, f32, maxerr
import vp_span_cases as C
import vp_specialised_cases as S
from test_gpu_mixed import tolerance
from test_gpu_vp_variants import check_label, scale

pytestmark = pytest.mark.gpu

WORKERS = 8                                                                   # compilers at a time (a command may use 16 CPUs)
INTERPRETER_BOUND = 2.5e-7                                                    # assertion 2, of max(1, max|interpreter|)
SUFFIX = '*specialised'


def cached():
    """the voice-program images in the package's cache"""
    from signals_amd import specialise
    return {path.name for path in specialise.CACHE.glob('vp_*.hsaco')}


@pytest.fixture(scope='module', autouse=True)
def _images():
    import torch
    from gpu_helpers import gpu_ready
    from signals_amd import _native, specialise
    gpu_ready()
    if specialise.hipcc() is None:
        pytest.skip('no hipcc on this machine: nothing to specialise with')
    jobs = [S.image_args(*image) for image in S.images()]
    assert len(jobs) <= S.MAX_IMAGES
    before, t0 = cached(), time.perf_counter()
    with concurrent.futures.ThreadPoolExecutor(max_workers=WORKERS) as pool:
        built = list(pool.map(lambda args: specialise.build(*args), jobs))
    print('vp specialised:', len(built), 'images,', len(cached() - before), 'built now, in', round(time.perf_counter() - t0, 1), 's')
    yield
    torch.cuda.synchronize()
    specialise.forget()
    _native.voice_program_use_attached(True)
    _native.set_voice_program_tuning(0, 0)


@functools.lru_cache(maxsize=None)
def wanted(kind, family, render):
    """the oracle's voice rows of one voice and render, float64: computed once, shared by its geometries and sinks"""
    want = S.oracle(S.build(kind, family)[1], kind, render)
    want.setflags(write=False)
    return want


def check_program(kind, family, frames, ks, sink, vpl, span):
    """no silent collapse: the voice compiles to a program of its family's variant, and every batch gets the geometry the cell is
    about -- four voices per lane only with the image at hand; -> the filters in series"""
    from signals_amd import _native
    from signals_amd.engine import _VoiceProgram
    prog = _VoiceProgram.compile(None, S.build(kind, family)[0], S.width(kind), mixed=True)
    assert prog is not None, (kind, family)
    counts = (len(prog.oscs), len(prog.params), len(prog.filters), prog.n_temps)
    assert _native.voice_program_variant(prog.code, *counts) == S.variant(kind, family), (kind, family, prog.code, counts)
    for K in ks:
        got = _native.voice_program_geometry(S.width(kind), frames, K, C.CONTEXT, prog.depth, S.SINKS[sink], S.aligned(kind), specialised=(vpl == 4))
        assert got == (vpl, span), (kind, family, K, got)
    return prog.depth


def run(kind, family, render, sink, vpl, span, specialised=True):
    """the batches of one render at one geometry, through the specialised image or (`specialised` False) the interpreter:
    (rows, the launch labels per batch, the filters in series)"""
    import torch
    from signals_amd import _native, runtime
    from signals_amd.chain import ext
    from signals_amd.engine import BatchRenderer, KernelTimer
    position, frames, ks = C.RENDERS[render]
    node, _ = S.build(kind, family)
    if sink == 'store':
        top, width = node, S.width(kind)
    else:
        top = ext.SumBus(); top.input = node
        top.get_state().gains = np.ascontiguousarray(S.pan(kind))
        width = S.SINKS[sink]
    _native.set_voice_program_tuning(vpl, 0 if frames < C.CONTEXT else span)  # (short blocks: the span is 1 whatever is asked)
    _native.voice_program_use_attached(specialised)
    try:
        depth = check_program(kind, family, frames, ks, sink, vpl, span)
        images, timer = cached(), KernelTimer()
        r = BatchRenderer(top, width, RATE, timer=timer, fuse_program='always', mixed_programs=True, specialise=specialised)
        parts, labels, pos = [], [], position
        for K in ks:
            before = len(timer.records)
            parts.append(r.render(pos, frames, K).cpu().numpy())
            labels.append([rec[0] for rec in timer.records[before:]])
            pos += frames * K
        torch.cuda.synchronize()
        runtime.check_status()
        assert cached() == images, (kind, family, sink, vpl, sorted(cached() - images))      # the fixture built what the engine asks for
    finally:
        _native.set_voice_program_tuning(0, 0)
        _native.voice_program_use_attached(True)
    for names in labels:
        # a swept voice's LFO rows are rendered by the control program in front of the launch; nothing else may run, and the voices
        # themselves in exactly one launch: of the image, or of the interpreter for the twin
        rows = [n for n in names if n.startswith('control_program[')]
        assert len(rows) == (1 if kind == 'swept' else 0), (kind, family, names)
        voice = [n for n in names if n not in rows]
        if specialised:
            assert len(voice) == 1 and voice[0].endswith(SUFFIX), (kind, family, sink, vpl, names)
            voice = [voice[0][:-len(SUFFIX)]]
        check_label(family, sink, voice)
    return np.concatenate(parts), labels, depth


@functools.lru_cache(maxsize=None)
def interpreted(kind, family, render, sink, vpl, span):
    """the interpreter's render of a cell: what assertion 2 compares with; four voices per lane run at two"""
    got, _, _ = run(kind, family, render, sink, min(vpl, 2), span, specialised=False)
    got.setflags(write=False)
    return got


@functools.lru_cache(maxsize=None)
def one_block_per_lane(kind, family, render, vpl):
    """the same image's store render at span 1: what assertion 3 compares a span with"""
    got, _, _ = run(kind, family, render, 'store', vpl, 1)
    got.setflags(write=False)
    return got


def cell(what, kind, family, render, sink, vpl, span):
    rows = wanted(kind, family, render)
    want = rows if sink == 'store' else rows @ S.pan(kind).T                  # (oracle.chain_ref.sum_bus)
    tol = tolerance(want) * scale(family)
    got, labels, depth = run(kind, family, render, sink, vpl, span)
    err = maxerr(got, f32(want))
    twin = interpreted(kind, family, render, sink, vpl, span)
    ok = np.isfinite(twin)
    bound = INTERPRETER_BOUND * max(1.0, float(np.abs(twin[ok]).max()) if ok.any() else 0.0)
    same_nan = got.shape == twin.shape and np.array_equal(np.isfinite(got), ok)
    diff = float(np.abs(got[ok].astype(np.float64) - twin[ok]).max()) if same_nan and ok.any() else 0.0
    print(what, family, kind, (vpl, span), sink, 'max|err|', err, 'tol', tol, 'max|interpreter diff|', diff, 'bound', bound,
          'equals float32(oracle)', bool(np.array_equal(got, f32(want))), 'equals the interpreter', bool(np.array_equal(got, twin, equal_nan=True)),
          labels)
    assert got.shape == want.shape and err <= tol, (kind, family, render, sink, vpl, span, err, tol)
    assert same_nan and diff <= bound, (kind, family, render, sink, vpl, span, diff, bound)
    if sink == 'store' and span > 1:
        base = one_block_per_lane(kind, family, render, vpl)
        same = np.array_equal(got, base, equal_nan=True)
        if not same:
            rows_off = np.flatnonzero((got != base).any(axis=1))
            print(what, family, kind, (vpl, span), 'differs from span 1 in', rows_off.size, 'rows, first', rows_off[:8],
                  'max|diff|', float(np.nanmax(np.abs(got - base))))
        assert same, (kind, family, render, vpl, span)
    return depth


@pytest.mark.parametrize('kind,family,vpl,span,sink', S.cells())
def test_specialised_cell(kind, family, vpl, span, sink):
    cell('vp specialised', kind, family, 'long', sink, vpl, span)


@pytest.mark.parametrize('sink', list(S.SINKS))
@pytest.mark.parametrize('family', C.DEEP)
def test_fresh_specialised_cell(family, sink):
    """two filters in series from position 1000 on a fresh renderer: the lane of blocks 0 and 1 re-walks a virtual history block"""
    assert C.FRESH[0] % C.N != 0
    assert cell('vp specialised fresh', 'deep', family, 'fresh', sink, *C.FRESH[2]) == 2


@pytest.mark.parametrize('vpl,sink', C.SHORT_CELLS)
@pytest.mark.parametrize('family', C.SHORT_DEEP)
def test_short_specialised_cell(family, vpl, sink):
    """blocks of 32 frames behind two filters in series: the four-step short-block walk of the same source"""
    assert C.SHORT_N < C.CONTEXT
    assert cell('vp specialised short', 'deep', family, 'short', sink, vpl, 1) == 2
