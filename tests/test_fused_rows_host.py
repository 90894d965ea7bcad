"""The case table of tests/fused_rows_cases.py, checked without a GPU: the restatement against chain_ref.render_stream of the equivalent
oracle graph (parameter tables as a node that answers row floor((position - start) / N), the row in front of the launch at -1) and
against the oracle of test_gpu_engine.py's test_block_rate_fm_runs_in_the_fused_chain with the tables filled from its LFOs; the census
of the axes, edges and launch counts; the numpy model of the walker's schedule against the restatement, and seven deliberately wrong
kernels of that model, each of which has to miss the outer bar by 100x in every leg its fault is reached in; and the condition on the
inputs that makes a K-row table count: rolled by one row it moves the restatement by 1e-3 of full scale at least."""
import numpy as np
import pytest

import fused_rows_cases as F
from oracle import chain_ref as R


# ------------------------------------------------------------------------------------------------ the restatement against the graph
class Table(R.Node):
    """per-block parameter rows as an oracle node: row floor((position - start) / N); -1 (a context request in front of the launch) is
    the row in front, where the table has one; past the last row (the `after` window of the last block, which no kept sample depends
    on) the last row"""
    cached = False

    def __init__(self, rows, front, start, N):
        super().__init__()
        self.rows, self.front, self.start, self.N = rows, front, start, N

    def eval(self, position, frames, channels, rate):
        b = (position - self.start) // self.N
        if b < 0 and self.front is not None:
            return self.front
        if self.rows.shape[0] == 1:
            return self.rows
        assert b >= 0, 'a K-row table was asked for the row in front of the launch and has none'
        return self.rows[min(b, self.rows.shape[0] - 1)][None, :]


def graph(c: F.Case, I: F.Inputs) -> R.Node:
    table = lambda rows, front=None: Table(rows, front, c.position, c.N)
    node = R.Osc(c.kind, table(I.hertz, I.hertz_hist), table(I.phase, I.phase_hist))
    if F.is_pair(c):
        node = R.Binary(c.source[0], node, R.Osc(c.source[1], R.Fixed(I.hertz2), R.Fixed(I.phase2)), None if I.mix is None else R.Fixed(I.mix))
    node = R.Filter(c.btype, node, table(np.broadcast_to(I.cutoff, (I.cutoff.shape[0], c.V))))      # (the reference raises on a one-column cutoff)
    if I.gain is not None:
        node = R.Binary('Gain', node, table(I.gain))
    return node


GRAPH_CASES = ('fm_sine_lp_store', 'fm_saw_lp_store_phase_rows', 'fm_square_hp_mono_columns', 'fm_tri_lp_store_from_zero', 'fm_sine_hp_bus2_qualify',
               'fm_saw_hp_store_one_block', 'fm_sine_lp_bus2_k9', 'swept_sine_lp_store', 'swept_tri_hp_store_v130_columns', 'swept_sine_hp_store_all_tail',
               'swept_square_lp_store_short', 'swept_saw_lp_bus2_k9', 'pair_mix_saw_square', 'pair_ring_tri_square_swept', 'pair_ring_sine_saw_short',
               'pair_ring_square_tri')


@pytest.mark.parametrize('name', GRAPH_CASES)
def test_restatement_equals_the_oracle_graph(name):
    """Gain(Filter(Osc | Mix | RingMod)) over table nodes, rendered block by block by chain_ref.render_stream: the oracle's cached
    oscillator answers a block's context from the previous block, made with the previous block's rows"""
    b = F.build(name)
    c, I = b.case, b.inputs
    want = R.render_stream(graph(c, I), c.position, c.N, c.K, c.V)
    assert want.shape == b.per_voice.shape and np.isfinite(want).all()
    assert float(np.abs(want - b.per_voice).max()) <= 1e-12, (name, float(np.abs(want - b.per_voice).max()))


def test_graph_cases_are_representative():
    cs = [F.BY_NAME[n] for n in GRAPH_CASES]
    assert any(F.is_fm(c) and c.position == 37 for c in cs) and any(F.is_fm(c) and c.N == 100 for c in cs) and any(F.is_fm(c) and c.position == 0 for c in cs)
    assert any(c.source == 'swept' and c.N == 100 for c in cs) and any(c.source == 'swept' and c.N < F.CTX for c in cs)
    assert {c.source[0] for c in cs if F.is_pair(c)} == {F.MIX, F.RING} and any(F.is_pair(c) and c.cutoff == 'KV' for c in cs)
    assert any(F.is_fm(c) and c.K == 1 for c in cs) and any(c.K == 9 for c in cs) and any(c.hertz == 'K1' for c in cs)


@pytest.mark.parametrize('kind,phase_mod,sweep,start', [('Sawtooth', False, False, 4096), ('Sine', False, False, 0), ('Triangle', True, True, 4096),
                                                       ('Square', True, False, 0), ('Sine', False, True, 4096)])
def test_restatement_reproduces_the_engine_oracle(golden, kind, phase_mod, sweep, start):
    """the oracle graph of test_block_rate_fm_runs_in_the_fused_chain (a vibrato on hertz, a wobble on phase, a swept cutoff): the
    tables hold its LFOs' block-rate values -- row b what the LFO answers at the block's position, the row in front what it answers at
    the first context row, where a fresh graph evaluates its oscillator for the context"""
    g = golden('c2')
    V, N, K = 32, 256, 9
    hz, ph, cut = g['c2/hertz'][:, :V], g['c2/phase'][:, :V], g['c2/cutoff'][:, :V]
    fm = lambda: R.Binary('Mix', R.Binary('Gain', R.Osc('Sine', R.Fixed([[5.3]])), R.Fixed([[9.0]])), R.Fixed(hz * 2.0), R.Fixed([[0.5]]))
    pm = lambda: R.Binary('Mix', R.Binary('Gain', R.Osc('Triangle', R.Fixed([[2.1]])), R.Fixed([[0.05]])), R.Fixed(ph * 2.0), R.Fixed([[0.5]]))
    sw = lambda: R.Binary('RingMod', R.Binary('Mix', R.Osc('Sine', R.Fixed([[1.7]])), R.Fixed([[1.0]]), R.Fixed([[0.4]])), R.Fixed(cut))
    oracle = R.Filter('lp', R.Osc(kind, fm(), pm() if phase_mod else R.Fixed(ph)), sw() if sweep else R.Fixed(cut))
    want = R.render_stream(oracle, start, N, K, V)

    def rows(make, positions):
        return np.concatenate([np.broadcast_to(R.render(make(), p, 1, V), (1, V)) for p in positions])
    blocks, front = [start + b * N for b in range(K)], [start - min(start, F.CTX)]
    c = F.case('engine', kind, 'lp', V, N, K, start, 'store', 'fm', 'KV' if sweep else '1V', None, 'KV', 'KV' if phase_mod else '1V')
    I = F.Inputs(rows(fm, blocks), rows(fm, front), rows(pm, blocks) if phase_mod else ph, rows(pm, front) if phase_mod else None,
                 rows(sw, blocks) if sweep else cut, None, None, None, None, None)
    got = F.restate(c, I)
    assert float(np.abs(got - want).max()) <= 1e-12, float(np.abs(got - want).max())


# ------------------------------------------------------------------------------------------------------------------- the census
def test_every_axis_value_is_met():
    for axis, values in F.AXES.items():
        met = {getattr(c, axis) for c in F.CASES}
        assert met == set(values), (axis, set(values) ^ met)
    assert all(c.V <= 200 and c.N <= 356 and c.K <= 9 for c in F.CASES)


def test_the_edges_the_table_is_there_for():
    some = lambda pred: [c.name for c in F.CASES if pred(c)]
    sources = {'swept': lambda c: c.source == 'swept', 'fm': F.is_fm, 'pair': F.is_pair}
    for what, mine in sources.items():                                          # block sizes per source; FM never below the context
        assert {c.N for c in F.CASES if mine(c)} == ({100, 101, 256, 356} if what == 'fm' else {64, 100, 101, 256, 356}), what
        assert {c.sink for c in F.CASES if mine(c)} == {'store', 1, 2}, what
    assert {c.position for c in F.CASES if F.is_fm(c)} == set(F.AXES['position'])
    # geometries: spans against K = 5, ragged voice tiles at 1, 2 and 4 voices per lane, the store sink's fall-backs, dead lanes on the bus
    assert {span for _, span in F.GEOMETRIES} == {1, 2, 3, 4, 8} and {vpt for vpt, _ in F.GEOMETRIES} == {1, 2, 4} and len(F.GEOMETRIES) == 8
    assert all(200 % (64 * vpt) for vpt in (1, 2, 4))
    for what, mine in sources.items():
        assert some(lambda c: mine(c) and c.V == 200 and c.K == 5 and c.sink == 'store') and some(lambda c: mine(c) and c.V == 200 and c.sink == 2), what
    assert {F.store_vpt(c, 4) for c in F.CASES if c.sink == 'store' and c.V == 67} == {1} and some(lambda c: c.sink != 'store' and c.V == 67)
    assert {F.store_vpt(c, 4) for c in F.CASES if c.sink == 'store' and c.V == 130} == {2}
    assert {(c.offset, F.store_vpt(c, 4)) for c in F.CASES if c.sink == 'store' and c.V % 4 == 0} == {(0, 4), (1, 1), (2, 2)}
    assert some(lambda c: c.V == 64 and c.sink == 'store' and c.offset == 0) and some(lambda c: c.V == 64 and c.sink != 'store')
    assert some(lambda c: c.N < F.CTX and F.effective(c, (4, 8)) == (4, 1))
    # table shapes
    shapes = {(c.cutoff, c.gain) for c in F.CASES}
    assert shapes >= {('KV', '1V'), ('1V', 'KV'), ('KV', 'KV'), ('KV', None), ('K1', 'K1'), ('1V', '1V'), ('1V', None)}
    fm_shapes = {(c.hertz, c.phase) for c in F.CASES if F.is_fm(c)}
    assert fm_shapes >= {('KV', '1V'), ('1V', 'KV'), ('KV', 'KV'), ('K1', '1V')}
    for c in F.CASES:
        I = F.build(c.name).inputs
        assert (I.hertz_hist is not None) == (F.is_fm(c) and c.hertz[0] == 'K') and (I.phase_hist is not None) == (F.is_fm(c) and c.phase[0] == 'K'), c.name
        assert F.is_fm(c) or (c.hertz, c.phase) == ('1V', '1V'), c.name
    # waveforms, filters, sinks
    for what, mine in sources.items():
        assert {c.kind for c in F.CASES if mine(c)} == set(F.KINDS) and {c.btype for c in F.CASES if mine(c)} == {'lp', 'hp'}, what
    assert {(c.kind, c.sink == 'store') for c in F.CASES} == {(k, s) for k in F.KINDS for s in (True, False)}
    assert all((F.build(c.name).inputs.pan is None) == (c.sink != 2) for c in F.CASES)
    # the Sine recurrence: taken, left past 2^26 cycles, left by one block's row and by the row in front alone
    fast = {c.name: F.all_fast(c, F.build(c.name).inputs) for c in F.CASES if c.kind == 'Sine'}
    assert all(fast[c.name] == (c.special is None) for c in F.CASES if c.kind == 'Sine'), fast
    for name in some(lambda c: c.special == 'far'):
        c, I = F.BY_NAME[name], F.build(name).inputs
        assert (c.position / F.RATE * I.hertz[:, :64]).min() > F.SINE_FAST_MAX_CYCLES and (c.position + c.K * c.N) / F.RATE * I.hertz[:, 64:].max() < F.SINE_FAST_MAX_CYCLES
    assert {c.source for c in F.CASES if c.special == 'far'} >= {'swept', 'fm'} and some(lambda c: c.special == 'far' and F.is_pair(c) and c.kind == 'Sine')
    for name in some(lambda c: c.special == 'qualify'):
        c, I = F.BY_NAME[name], F.build(name).inputs
        over, front = np.abs(I.hertz) > F.RATE / 4, np.abs(I.hertz_hist) > F.RATE / 4
        assert over.sum() == 1 and over[c.K // 2, F.QUALIFY_MIDDLE] and 0 < c.K // 2 < c.K - 1
        assert front.sum() == 1 and front[0, F.QUALIFY_FRONT] and not over[:, F.QUALIFY_FRONT].any()
        assert F.QUALIFY_MIDDLE // 64 != F.QUALIFY_FRONT // 64 and c.V > 128 + 64 and c.position > 0       # ordinary voices in other waves
    assert {c.sink for c in F.CASES if c.special == 'qualify'} == {'store', 2}
    # paired sources: both operations with every second waveform; a Sine first oscillator on the recurrence and past it; with cutoff rows; no mix row
    pairs = [c for c in F.CASES if F.is_pair(c)]
    assert {(c.source[0], c.source[1]) for c in pairs} == {(op, k) for op in (F.MIX, F.RING) for k in F.KINDS}
    assert any(c.kind == 'Sine' and c.special is None for c in pairs) and any(c.kind == 'Sine' and c.special == 'far' for c in pairs)
    assert any(c.cutoff == 'KV' for c in pairs) and any(not c.source[2] for c in pairs) and all(c.source[2] for c in pairs if c.source[0] == F.MIX)
    # the bad cutoff
    c = F.BY_NAME[F.STATUS_CASE]
    b = F.build(c.name)
    assert c.sink == 'store' and c.special == 'bad_cutoff' and (b.inputs.cutoff == 0).sum() == 1 and b.inputs.cutoff[F.BAD_AT] == 0 and F.BAD_AT[0] + 1 < c.K
    nan = np.isnan(b.ref)
    assert nan[F.BAD_AT[0] * c.N:(F.BAD_AT[0] + 1) * c.N, F.BAD_AT[1]].all() and nan.sum() == c.N


def test_the_launch_cap():
    counts = F.launches()
    print('fused rows: launches per test', counts)
    assert max(counts.values()) <= F.LAUNCH_CAP, counts
    for n in F.BATCHING + F.ONE_ROW + F.STEADY + (F.STATUS_CASE,):
        assert n in F.BY_NAME, n
    cs = [F.BY_NAME[n] for n in F.BATCHING]
    assert {c.source if not F.is_pair(c) else 'pair' for c in cs} == {'swept', 'fm', 'pair'} and {c.sink == 'store' for c in cs} == {True, False}
    assert any(c.kind == 'Sine' for c in cs) and any(c.kind != 'Sine' and c.sink == 'store' for c in cs) and any(c.position == 0 for c in cs)
    for c in (F.BY_NAME[n] for n in F.ONE_ROW):
        assert c.source == 'swept' and not F.k_row_tables(c)
    assert {F.BY_NAME[n].sink for n in F.ONE_ROW} == {'store', 1, 2}
    for c in (F.BY_NAME[n] for n in F.STEADY):
        assert c.kind == 'Sine' and c.sink != 'store' and c.source == 'swept' and F.k_row_tables(c)
    assert {F.k_row_tables(F.BY_NAME[n]) for n in F.STEADY} == {('gain',), ('cutoff',), ('cutoff', 'gain')} and {F.BY_NAME[n].sink for n in F.STEADY} == {1, 2}


# ------------------------------------------------------------------------------------------------- the reference and its inputs
@pytest.mark.parametrize('name', [c.name for c in F.CASES])
def test_reference_is_worth_comparing_with(name):
    """the tables are what the docstring says; the reference is finite but for the bad cutoff and of a full scale the 1e-6 bar means
    something at; the model of the schedule with nothing wrong, under the geometry with the most boundaries inside spans, is the
    restatement to rounding; and every K-row table counts: rolled by one row it moves the reference by 1e-3 of full scale at least"""
    b = F.build(name)
    c, I = b.case, b.inputs
    for k in F.TABLES:
        t = getattr(I, k)
        assert (t is None) == (getattr(c, k) is None) and (t is None or t.shape == F.table_shape(getattr(c, k), c.K, c.V)), (name, k)
    ok = I.cutoff > 0
    assert I.cutoff[ok].min() >= 60.0 and I.cutoff.max() <= 9000.0 and (I.gain is None or (0.25 <= np.abs(I.gain).min() and np.abs(I.gain).max() <= 1.0))
    assert I.gain is None or I.gain.shape[0] == 1 or ((I.gain > 0).any() and (I.gain < 0).any())
    assert 0.0 <= I.phase.min() and I.phase.max() < 1.0 and I.hertz.min() >= 55.0
    assert b.ref.shape == (c.K * c.N, F.channels_of(c)) and np.isfinite(b.ref).all() == (c.special != 'bad_cutoff')
    peak = float(np.nanmax(np.abs(b.ref)))
    assert peak > 0.3, (name, peak)
    finite = np.isfinite(b.ref)
    same = F.model(c, I, (4, 8))
    assert float(np.abs(same - b.ref)[finite].max()) <= 1e-11 * max(1.0, peak), (name, float(np.abs(same - b.ref)[finite].max()))
    for k in F.k_row_tables(c):
        rolled = F.model(c, I._replace(**{k: np.roll(getattr(I, k), 1, axis=0)}), (1, 1))
        both = finite & np.isfinite(rolled)
        moved = float(np.abs(rolled - b.ref)[both].max())
        print(f'fused rows: {name}: max|ref| {peak:.4g}, {k} rows rolled by one: moved by {moved:.3g}')
        assert moved >= F.DISCRIMINATION * peak, (name, k, moved, peak)


def test_inputs_are_deterministic():
    for name in ('fm_sine_hp_bus2_qualify', 'pair_mix_sine_tri_far'):
        first, again = F.build(name), F.build.__wrapped__(name)
        assert all(a is None and b is None or np.array_equal(a, b) for a, b in zip(first.inputs, again.inputs)) and np.array_equal(first.ref, again.ref)


# ------------------------------------------------------------------------------------------------------------ the wrong kernels
# cases each wrong kernel fails (under every geometry that reaches its fault), as counted by test_wrong_kernels_are_caught
CAUGHT = {'warm_up_design': 19, 'weights_late': 23, 'front_row': 11, 'row_in_span': 12, 'no_reseed': 4, 'dead_lane': 20, 'column_stride': 3}


@pytest.mark.parametrize('wrong', F.WRONG)
def test_wrong_kernels_are_caught(wrong):
    """each wrong kernel (fused_rows_cases.model) misses the outer bar by 100x at least in EVERY leg that reaches its fault
    (fused_rows_cases.applies), a non-empty set of cases whose size is stated in CAUGHT; none is run on a GPU"""
    caught, passed = set(), []
    for c in F.CASES:
        b = F.build(c.name)
        seen = set()
        for geometry in F.GEOMETRIES:
            key = F.effective(c, geometry) if wrong == 'dead_lane' else F.effective(c, geometry)[1]
            if not F.applies(wrong, c, geometry) or key in seen:                # (the schedule depends on the span alone, a dead lane on the voices per lane)
                continue
            seen.add(key)
            if F.misses(F.model(c, b.inputs, geometry, wrong), b.ref):
                caught.add(c.name)
            else:
                passed.append((c.name, geometry))
    print(f'fused rows: {wrong} fails {len(caught)} cases: {sorted(caught)}')
    assert not passed, (wrong, passed)
    assert len(caught) == CAUGHT[wrong] > 0, (wrong, len(caught))
