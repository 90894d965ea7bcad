"""Every family of the voice-program interpreter (signals_amd/csrc/sig_vp_machine.h, the 13 of tests/test_gpu_vp_variants.py) with
MORE THAN ONE BLOCK PER LANE: what happens at a block boundary inside a lane's span -- the next block's chains starting in the middle
of a row group, their design from inside a block and the redesign of the current chains on entry, the reload of the per-block
parameter rows for blocks 2 .. span, ragged and oversized spans, the re-walk of the block in front of a span for two filters in
series, the bus sink over a span -- is otherwise run by the plain family alone (tests/test_gpu_voice_program.py), the other
families' tests leaving the span at 1.  The cases are tests/vp_span_cases.py's; tests/test_vp_span_cases_host.py shows on the CPU
that a chain started one row late, or a control row not reloaded, misses the tolerance here at least tenfold in every block.

Shapes.  66 voices (two voice tiles at one voice per lane, the second ragged; one at two per lane), 48 kHz, blocks of N = 130 frames:
(130 - 100) % 4 = 2 and (130 - 100) % 8 = 6, so the first warm row of the next block's chains (row N - 100 of a block) falls inside a
row group in the full register file (4 rows) and in the small one (8 rows) -- at the suite's other block lengths, 128 and 256,
(N - 100) % 4 == 0 and the full-file kernels never saw a straddling group; and 130 % 4 = 130 % 8 = 2, so every block ends in
single-row groups.  One BatchRenderer renders two consecutive batches of 3 and 4 blocks from position 0 (the second continues from
the first one's history), through the interpreter alone (fuse_program='always', mixed_programs=True, specialise=False, attached
images off).

Geometries (voices per lane, blocks per lane), forced with set_voice_program_tuning, and the blocks each lane owns:

    (1, 2)     K = 3: [0 1] [2]    (a ragged last span)         K = 4: [0 1] [2 3]
    (2, 3)     K = 3: [0 1 2]                                   K = 4: [0 1 2] [3]    (a lone last block)
    (2, 16)    K = 3: [0 1 2]      (the span exceeds the batch: one lane walks it all)    K = 4: [0 1 2 3]

Voices: per family the small-file and the full-file voice of tests/test_gpu_vp_variants.py, one voice whose every family-specific
control follows a block-rate LFO, and for plain, band, resonant, resonant_eq and mixed a voice with two filters in series:
13 x 3 + 5 = 44, each at every geometry to the store and under a 2-channel bus: 264 cells.  The deep voices also start fresh in
mid-stream, 5 blocks from position 1000 at (1, 2) (lanes own [0 1] [2 3] [4]; 1000 is no block multiple: the history is virtual
blocks): 10 cells.  Blocks of 32 frames, shorter than the context, for the deep voices of band, resonant_eq and mixed, two voices
per lane under the bus and one to the store: steps 1 and 2 of the short-block walk start the next chains of level 1 and of level 2
apart, so `design` has to skip the slots below that level in its band, resonant and equaliser branches: 6 cells.

Before a render sig_voice_program_variant must name the voice's variant and register file and sig_voice_program_geometry must
answer (voices per lane, span) for each batch size: no cell falls back to span 1 unnoticed.  After it each batch must have been
exactly one interpreter launch (voice_program[ | voice_program_bus[, not *specialised, with the words that select the _eq and
_sync kernel sets) -- and, for a swept voice, the one control_program launch that renders its LFO rows in front of it.

Two assertions on the rows.

1. Against the oracle: the float32 output within 1e-6 max(1, max|oracle|) of float32(oracle) (tests/test_gpu_mixed.py `tolerance`),
   times max(1, L) behind the Shaper (test_gpu_vp_variants.scale).  No sample is excluded.  Both sinks.

2. Store sink: the span render is bit for bit the render of the same cell at (voices per lane, 1), NaN positions included.  This
   follows from the code: whichever lane owns a block, its chains are cold-started on the same row (start_next zeroes them where the
   walk reaches row s - min(100, s)), designed from the same control row, and advanced by the same per-row operations in the same
   order; the oscillators' phase is the exact n / rate of each row, not an accumulated one; the parameter registers hold the block's
   own rows; the envelope's segment is a function of the voice's rows and the time alone.  Only the grouping of the rows into
   dispatches differs (a span walks a block's last 100 rows as that block's groups, span 1 as a step of their own that starts at
   row s - 100), and no operation reaches across the rows of a group.  The bus sink adds voice tiles in another order per geometry
   and is held to the oracle only.

Measured on an MI355X, the largest max|err| / tol over a family's cells (tol = 1e-6 max(1, max|oracle|), shape: times L): plain
0.0017, band 2.2e-7, pm 0.16 (the swept voice to the store: 1.79e-7 against 1.13e-6), table 0, shape 0, resonant 4.7e-5, unison 0.0075,
blep 0, mixed 0.00047, resonant_eq 1.1e-5, mixed_eq 0, sync 0, mixed_sync 0 -- 0: every cell of the family equals float32(oracle)
bit for bit; 229 of the 280 cells do.  Every store cell with a span above 1 was bit-equal to its span-1 render: assertion 2 holds
as derived, the envelope's re-seeding at each step start included.  No cell found a fault in the kernels."""
import functools

import numpy as np
import pytest

from helpers import RATE, f32, maxerr
import mixed_patches as MP
import vp_span_cases as C
from test_gpu_mixed import tolerance
from test_gpu_vp_variants import check_label, scale

pytestmark = pytest.mark.gpu

ALIGNED = 2                                                                   # (rows, 66) float32 from the allocator: 8-byte aligned, even


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    from gpu_helpers import gpu_ready
    from signals_amd import _native
    gpu_ready()
    yield
    _native.set_voice_program_tuning(0, 0)
    _native.voice_program_use_attached(True)


@functools.lru_cache(maxsize=None)
def wanted(kind, family, render):
    """the oracle's voice rows of one voice and render, float64: computed once, shared by its geometries and sinks"""
    want = C.oracle(C.build(kind, family)[1], render)
    want.setflags(write=False)
    return want


def check_program(kind, family, frames, ks, sink, vpl, span):
    """no silent collapse: the voice compiles to a program of its family's variant and register file, and every batch gets the
    geometry the cell is about; -> the filters in series"""
    from signals_amd import _native
    from signals_amd.engine import _VoiceProgram
    prog = _VoiceProgram.compile(None, C.build(kind, family)[0], C.V, mixed=True)
    assert prog is not None, (kind, family)
    counts = (len(prog.oscs), len(prog.params), len(prog.filters), prog.n_temps)
    assert _native.voice_program_variant(prog.code, *counts) == C.variant(kind, family), (kind, family, prog.code, counts)
    for K in ks:
        assert _native.voice_program_geometry(C.V, frames, K, C.CONTEXT, prog.depth, C.SINKS[sink], ALIGNED) == (vpl, span), (kind, family, K)
    return prog.depth


def run(kind, family, render, sink, vpl, span):
    """the batches of one render at one geometry: (rows, the launch labels per batch)"""
    import torch
    from signals_amd import _native, runtime
    from signals_amd.chain import ext
    from signals_amd.engine import BatchRenderer, KernelTimer
    position, frames, ks = C.RENDERS[render]
    node, _ = C.build(kind, family)
    if sink == 'store':
        top, width = node, C.V
    else:
        top = ext.SumBus(); top.input = node
        top.get_state().gains = np.ascontiguousarray(MP.draw(C.V)['pan'])
        width = C.SINKS[sink]
    _native.set_voice_program_tuning(vpl, 0 if frames < C.CONTEXT else span)  # (short blocks: the span is 1 whatever is asked)
    _native.voice_program_use_attached(False)                                # the interpreter, whatever image another test attached
    try:
        depth = check_program(kind, family, frames, ks, sink, vpl, span)
        timer = KernelTimer()
        r = BatchRenderer(top, width, RATE, timer=timer, fuse_program='always', mixed_programs=True, specialise=False)
        parts, labels, pos = [], [], position
        for K in ks:
            before = len(timer.records)
            parts.append(r.render(pos, frames, K).cpu().numpy())
            labels.append([rec[0] for rec in timer.records[before:]])
            pos += frames * K
        torch.cuda.synchronize()
        runtime.check_status()
    finally:
        _native.set_voice_program_tuning(0, 0)
        _native.voice_program_use_attached(True)
    for names in labels:
        # a swept voice's LFO rows are rendered by the control program in front of the launch; nothing else may run, and the
        # voices themselves in exactly one interpreter launch
        rows = [n for n in names if n.startswith('control_program[')]
        assert len(rows) <= (1 if kind == 'swept' else 0), (kind, family, names)
        check_label(family, sink, [n for n in names if n not in rows])
    return np.concatenate(parts), labels, depth


@functools.lru_cache(maxsize=None)
def one_block_per_lane(kind, family, render, vpl):
    """the store render at span 1: what assertion 2 compares a span with, shared by the geometries of one `vpl`"""
    got, _, _ = run(kind, family, render, 'store', vpl, 1)
    got.setflags(write=False)
    return got


def cell(what, kind, family, render, sink, vpl, span):
    rows = wanted(kind, family, render)
    want = rows if sink == 'store' else rows @ MP.draw(C.V)['pan'].T          # (oracle.chain_ref.sum_bus)
    tol = tolerance(want) * scale(family)
    got, labels, depth = run(kind, family, render, sink, vpl, span)
    err = maxerr(got, f32(want))
    print(what, family, kind, (vpl, span), sink, 'max|err|', err, 'tol', tol, labels)
    assert got.shape == want.shape and err <= tol, (kind, family, render, sink, vpl, span, err, tol)
    if sink == 'store' and span > 1:
        base = one_block_per_lane(kind, family, render, vpl)
        same = np.array_equal(got, base, equal_nan=True)
        if not same:
            rows_off = np.flatnonzero((got != base).any(axis=1))
            print(what, family, kind, (vpl, span), 'differs from span 1 in', rows_off.size, 'rows, first', rows_off[:8],
                  'max|diff|', float(np.nanmax(np.abs(got - base))))
        assert same, (kind, family, render, vpl, span)
    return depth


@pytest.mark.parametrize('sink', list(C.SINKS))
@pytest.mark.parametrize('geometry', C.GEOMETRIES, ids=lambda g: '%dx%d' % g)
@pytest.mark.parametrize('kind,family', C.voices())
def test_span_cell(kind, family, geometry, sink):
    cell('vp span', kind, family, 'long', sink, *geometry)


@pytest.mark.parametrize('sink', list(C.SINKS))
@pytest.mark.parametrize('family', C.DEEP)
def test_fresh_span_cell(family, sink):
    """two filters in series from position 1000 on a fresh renderer: the lane of blocks 0 and 1 re-walks a virtual history block"""
    assert C.FRESH[0] % C.N != 0
    assert cell('vp span fresh', 'deep', family, 'fresh', sink, *C.FRESH[2]) == 2


@pytest.mark.parametrize('vpl,sink', C.SHORT_CELLS)
@pytest.mark.parametrize('family', C.SHORT_DEEP)
def test_short_deep_cell(family, vpl, sink):
    """blocks of 32 frames behind two filters in series: the four-step short-block walk, whose steps 1 and 2 start the next chains
    of level 1 and level 2 apart.  Fixed controls and depth 2: the engine batches these (a NotBatchable fails the test)"""
    assert C.SHORT_N < C.CONTEXT
    assert cell('vp span short', 'deep', family, 'short', sink, vpl, 1) == 2
