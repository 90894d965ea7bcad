"""Differential test on random graphs over the WHOLE node set (tests/random_ext_graphs.py: the ten extension families beside the
original nodes, every family shared between a history reader and a plain one, modulated, and one column wide under a wide reader):
what is under test is the composition in signals_amd/engine/batch.py -- history rows, the memo per (node, channels), tails, widths and
the choice of route -- not the kernels, which the families' own tests pin.

Renders per seed at 48 kHz, (position, N, batches): (0, 128, (1, 2)), continuing batches: the tails; (1000, 256, (2, 1)), a fresh
mid-stream start on the own-history path; (37, 128, (2,)), a fresh start with fewer than 100 context rows.  Four legs:

    1. eager     helpers.stream within tol of float32(oracle), no sample excluded
    2. per node  BatchRenderer(fuse=False) equals the eager rows bit for bit (the same NaN positions, the same bits): the same kernels
                 over the same stored float32 rows, as every family's own GPU test states; no family documents an exception for this
                 route, so none is made.  No NotBatchable at N >= 128
    3. default   BatchRenderer() within tol of the oracle, and bit-equal to eager when the launch names show no fused kernel and no
                 voice program (tests/test_gpu_delay.py: check_routes)
    4. program   BatchRenderer(fuse_program='always', mixed_programs=True) within tol of the oracle, the launch geometry cycled through
                 (0, 0), (2, 2), (1, 3) by seed % 3; and the short-block render (0, 64, (3, 2, 1)), where NotBatchable is allowed and
                 must carry a reason

tol = 1e-6 * G * max(1, max |oracle|) with the graph's gain bound G from the generator (derived from the description on the CPU, never
from a GPU result; random_ext_graphs.py's docstring).  The closing test prints how much of it each leg used.

Measured on an MI355X, the largest error / tol over the 32 seeds per leg: eager 0.144, per node 0 (bit-equal on every seed), default
0.144, program 0.144 -- all three at seed 21, position 1000, the same 7.15e-7 against a tol of 4.98e-6 (max |oracle| 3.23, G 1.54);
54 of the 96 default-route renders ran without a fused kernel or a voice program and were bit-equal to eager, 69 of the 96
program-route renders launched a voice program, 66 of them with a word of an extension family, 10 of the 32 short-block renders
stayed batched (the others: 'cascaded filters with block size <= 100 depend on the after-window cache entries').

What the seeds found (17 of the 32 before the fix, seed 0 the first): a Delay over a request-dependent input that answers ONE column
-- signals_amd/engine/batch.py: _delay_uncached; pinned by tests/test_gpu_delay.py:
test_a_one_column_swept_input_is_evaluated_afresh_for_every_context_request."""
import functools

import numpy as np
import pytest

from gpu_helpers import gpu_ready, render_batches
from helpers import f32, maxerr, stream
import random_ext_graphs as G

pytestmark = pytest.mark.gpu

TUNING = ((0, 0), (2, 2), (1, 3))
FUSED = ('fused', 'latency', 'cascade', 'steady', 'walk', 'biquad_bus', 'biquad_coldstart_env', 'adsr_apply', 'voice_program')
USED = {'eager': 0.0, 'per node': 0.0, 'default': 0.0, 'program': 0.0}
WORST = {}
RUNS = {'seeds': 0, 'program_renders': 0, 'with_program': 0, 'with_extension_word': 0, 'short_renders': 0, 'short_batched': 0,
        'default_bit_equal': 0, 'default_renders': 0}


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    from signals_amd import _native
    gpu_ready()
    yield
    _native.set_voice_program_tuning(0, 0)


@functools.lru_cache(maxsize=None)
def wanted(seed, pos, N, K):
    """(the oracle's rows, tol) of one render of one seed, computed once on the CPU and shared by the legs"""
    graph = G.Builder(seed).build(gpu=False)
    want = G.oracle_rows(graph, pos, N, K)
    want.setflags(write=False)
    return want, G.tolerance(graph, want)


def within(leg, got, want, tol, what):
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape)
    err = maxerr(got, f32(want))
    if err / tol > USED[leg]:
        USED[leg], WORST[leg] = err / tol, what
    print(f'random ext graph {what} {leg}: max|err| {err:.3g} tol {tol:.3g} used {err / tol:.3f} max|oracle| {float(np.abs(want).max()):.3g}')
    assert err <= tol, (what, leg, err, tol)


def extension_words(names):
    from signals_amd import _native
    for n in names:
        if n.startswith('voice_program') and '[' in n:
            words = n[n.index('[') + 1:n.index(']')].split(',')
            if _native.vp_families([(op, 0, 0, 0, 0) for op in words if op in _native.VP_OPS]):
                return True
    return False


@pytest.mark.parametrize('seed', G.SEEDS)
def test_random_ext_graph_on_every_route(seed):
    from signals_amd import _native
    from signals_amd.engine import NotBatchable
    b = G.Builder(seed)
    _native.set_voice_program_tuning(*TUNING[seed % 3])
    try:
        for pos, N, ks in G.RENDERS:
            K, what = sum(ks), (seed, pos, N)
            want, tol = wanted(seed, pos, N, K)
            graph = b.build()
            eager = stream(graph.node, pos, N, K, graph.channels)
            within('eager', eager, want, tol, what)                                            # 1
            graph = b.build()
            plain, names, _ = render_batches(graph.node, graph.channels, pos, N, ks, names=True, fuse=False)        # 2 (NotBatchable here fails the test)
            assert not any(w in n for n in names for w in FUSED), names
            assert plain.dtype == np.float32 and np.array_equal(plain, eager, equal_nan=True), (what, maxerr(plain, eager))
            graph = b.build()
            default, names, _ = render_batches(graph.node, graph.channels, pos, N, ks, names=True)                  # 3
            within('default', default, want, tol, what)
            RUNS['default_renders'] += 1
            if not any(w in n for n in names for w in FUSED):
                RUNS['default_bit_equal'] += 1
                assert np.array_equal(default, eager, equal_nan=True), (what, sorted(names), maxerr(default, eager))
            graph = b.build()
            program, names, _ = render_batches(graph.node, graph.channels, pos, N, ks, names=True, fuse_program='always', mixed_programs=True)   # 4
            within('program', program, want, tol, what)
            RUNS['program_renders'] += 1
            RUNS['with_program'] += any(n.startswith('voice_program') for n in names)
            RUNS['with_extension_word'] += extension_words(names)
        pos, N, ks = G.SHORT
        want, tol = wanted(seed, pos, N, sum(ks))
        graph = b.build()
        RUNS['short_renders'] += 1
        try:
            short, names, _ = render_batches(graph.node, graph.channels, pos, N, ks, names=True, fuse_program='always', mixed_programs=True)
        except NotBatchable as e:
            assert str(e).strip(), 'a refusal without a reason'
            print(f'random ext graph {(seed, pos, N)} program: NOT BATCHABLE: {e}')
        else:
            RUNS['short_batched'] += 1
            within('program', short, want, tol, (seed, pos, N))
        RUNS['seeds'] += 1
    finally:
        _native.set_voice_program_tuning(0, 0)


def test_the_random_ext_graphs_did_exercise_the_routes():
    """(runs after the 32 seeds above) at least half of the program-route renders launched a voice program, at least one of those
    carried a word of an extension family, some short-block renders stayed batched; prints how much of the tolerance each leg used"""
    if RUNS['seeds'] == 0:
        pytest.skip('the seeds did not run in this session')
    print('random ext graphs', RUNS)
    print('random ext graphs, largest error / tol per leg:', {k: round(v, 4) for k, v in USED.items()}, 'at', WORST)
    assert RUNS['with_program'] >= RUNS['program_renders'] // 2, RUNS
    assert RUNS['with_extension_word'] >= 1, RUNS
    assert RUNS['short_batched'] >= 1, RUNS
