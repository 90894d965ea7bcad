"""The case table of tests/bus_pass_cases.py, checked without a GPU: the census (every axis value, every kernel instantiation of
biquad_bus.hip, the row-group and window edges the table is there for, the launch cap), the restatement against
chain_ref.render_stream of the equivalent oracle graph, the conditions that keep a dropped voice from hiding under the bound, the
hand-placed envelope boundaries, and the float64-versus-longdouble distance the bound is built on."""
import numpy as np
import pytest

import bus_pass_cases as B
import envelopes as E
from oracle import chain_ref as R


def test_longdouble_is_longer_than_float64():
    """the recurrence term of the bound is a float64-versus-longdouble distance: on a build whose longdouble is float64 it would be
    zero and the bound quietly another one"""
    assert np.finfo(np.longdouble).nmant >= 63, np.finfo(np.longdouble)


def test_every_axis_value_is_met():
    for axis, values in B.AXES.items():
        met = {getattr(c, axis) for c in B.CASES}
        assert met == set(values), (axis, set(values) ^ met)


def test_every_instantiation_is_reached():
    """biquad_bus_kernel<VPT, kRing, ENV, C>: voices per lane 4 | 1 x envelope x C in 1, 2, 4, all twelve"""
    reached = {(v.vpt, v.env, v.C) for v in map(B.expected_variant, B.CASES)}
    assert reached == set(B.INSTANTIATIONS) and len(B.INSTANTIATIONS) == 12, set(B.INSTANTIATIONS) - reached
    for c in B.CASES:
        v = B.expected_variant(c)
        assert v.chunk == (8 if v.env and v.vpt == 4 and v.C >= 2 else 16) and v.chunk % v.group == 0 and v.chunk % v.ring == 0, c.name


def test_the_edges_the_table_is_there_for():
    variants = {c.name: B.expected_variant(c) for c in B.CASES}
    some = lambda pred: [n for n, v in variants.items() if pred(B.BY_NAME[n], v)]
    # the one-voice kernel through each clause of the 16-byte predicate, and with two to seventeen voice tiles
    assert some(lambda c, v: v.vpt == 1 and c.V % 4) and some(lambda c, v: v.vpt == 1 and c.V % 4 == 0 and c.layout == 'pad1')
    assert some(lambda c, v: v.vpt == 1 and c.V % 4 == 0 and c.layout == 'ld1')
    assert {v.voice_tiles for v in variants.values() if v.vpt == 1} >= {1, 2, 4, 5, 17}
    assert {v.voice_tiles for v in variants.values() if v.vpt == 4} >= {1, 2, 5}
    assert some(lambda c, v: v.vpt == 4 and c.V % 256 and c.V > 4) and some(lambda c, v: v.vpt == 1 and c.V % 64 and c.V > 64)     # dead lanes
    assert some(lambda c, v: v.idle_waves and v.voice_tiles > 1 and c.K > 1)
    # the flush: a ragged front at every group size (C = 4 needs context 6), a ragged end, blocks shorter than a group
    for C in (1, 2, 4):
        for env in (False, True):
            mine = lambda c, v: v.C == C and v.env == env
            assert some(lambda c, v: mine(c, v) and v.ragged_front), (C, env)
            assert some(lambda c, v: mine(c, v) and v.ragged_end), (C, env)
    assert some(lambda c, v: v.C == 4 and v.ragged_front and c.context == 6)
    assert some(lambda c, v: v.short_of_group and v.C == 1) and some(lambda c, v: v.short_of_group and v.C == 2)
    assert some(lambda c, v: c.N == 1 and c.K > 1)
    # window geometry: block 0 inside the context, blocks that reach back into the history, the ring's repeated last row
    assert some(lambda c, v: 0 < c.position < c.context and c.K > 1) and some(lambda c, v: c.position == 0 and c.context and c.K > 2)
    assert some(lambda c, v: v.into_history and v.vpt == 4) and some(lambda c, v: v.into_history and v.vpt == 1)
    assert some(lambda c, v: v.repeats_last_row and c.N + c.context < v.ring)
    # other paths
    assert some(lambda c, v: c.C == 'mono' and v.env) and some(lambda c, v: c.gains_extra and v.vpt == 4) and some(lambda c, v: c.gains_extra and v.vpt == 1)
    assert some(lambda c, v: c.out_extra and v.C == 1) and some(lambda c, v: c.out_extra and v.C == 4)
    for cutoff in B.AXES['cutoff']:
        assert some(lambda c, v: c.cutoff == cutoff and (c.K > 1 or not cutoff.startswith('blocks'))), cutoff
    assert some(lambda c, v: v.env and c.position == B.FAR) and some(lambda c, v: v.env and c.position == B.HOUR)


def test_the_launch_cap():
    counts = B.launches()
    print('bus pass: launches', counts, 'in all', sum(counts.values()))
    assert sum(counts.values()) <= B.LAUNCH_CAP, counts
    for name in B.BATCHING + B.CUTOFF_ROWS + B.LANES + (B.STATUS_CASE, B.DEAD_VOICES_ACROSS[0]) + B.BUS_WIDTH + tuple(d[0] for d in B.DEAD_VOICES):
        assert name in B.BY_NAME, name
    for name, live, layout in B.DEAD_VOICES + (B.DEAD_VOICES_ACROSS,):           # which kernel the two renders of a pair take
        c = B.BY_NAME[name]
        kernels = {4 if live % 4 == 0 and B.expected_variant(c._replace(layout=layout)).vec_ok else 1, B.expected_variant(c._replace(layout=layout)).vpt}
        assert (len(kernels) == 2) == ((name, live, layout) == B.DEAD_VOICES_ACROSS), (name, live, layout, kernels)
    assert all(B.channels_of(B.BY_NAME[n]) >= 2 for n in B.BUS_WIDTH) and B.BY_NAME[B.STATUS_CASE].cutoff == 'blocks'
    assert all(B.BY_NAME[n].K > 1 for n in B.BATCHING + B.CUTOFF_ROWS) and all(B.BY_NAME[n].layout == 'contig' or B.BY_NAME[n].layout == 'pad4' for n in B.LANES)
    assert all(B.expected_variant(B.BY_NAME[n]).vpt == 4 for n in B.LANES) and {B.BY_NAME[n].env is None for n in B.LANES} == {True, False}
    assert {B.BY_NAME[n].env is None for n in B.BATCHING} == {True, False} and {B.expected_variant(B.BY_NAME[n]).vpt for n in B.BATCHING} == {1, 4}


@pytest.mark.parametrize('name', [c.name for c in B.CASES])
def test_reference_is_worth_comparing_with(name):
    """float32-exact inputs in +-0.25, cutoffs in 200 .. 8000 Hz, max|ref| above FULL_SCALE, every voice heard in some channel; and the
    figures of the bound: the float64-versus-longdouble distance of the recurrence, per case"""
    b = B.build(name)
    c = b.case
    x = b.x.array
    assert x.dtype == np.float32 and x.shape == (B.history_of(c) + c.N * c.K, c.V) and np.abs(x).max() <= 0.25
    assert b.cutoff.min() >= 200.0 and b.cutoff.max() <= 8000.0
    if b.cutoff.shape[0] > 1:
        assert all(not np.array_equal(b.cutoff[i], b.cutoff[i + 1]) for i in range(b.cutoff.shape[0] - 1)), name
    if b.gains is not None:
        assert (b.gains.array > 0).all()                                        # cos / sin of (0, pi / 2): every voice carries weight
    assert b.ref.shape == (c.N * c.K, B.channels_of(c)) and np.isfinite(b.ref).all()
    peak = float(np.abs(b.ref).max())
    share = B.contributions(b.y64, b.level, b.weight, b.ref)
    half, summation, recurrence = B.bound_terms(b)
    distance = float(np.abs(b.y64.astype(np.longdouble) - b.y80).max())
    print(f'bus pass: {name}: max|ref| {peak:.4g}, least voice share {share.min():.3g}, max|y64 - y80| {distance:.3g}, '
          f'bound terms: half ulp {half.max():.3g}, summation {summation.max():.3g}, recurrence {recurrence.max():.3g}')
    assert peak > B.FULL_SCALE, (name, peak)
    assert share.min() >= B.CONTRIBUTION, (name, int(share.argmin()), float(share.min()))
    assert 0.0 < distance < 1e-12, (name, distance)                            # longer than float64, and the same recurrence
    assert float((half + summation + recurrence).max()) < 1e-6 * max(1.0, peak)  # the bound is the tighter of the two bars


ENVELOPED = [c.name for c in B.CASES if c.env is not None]


@pytest.mark.parametrize('name', ENVELOPED)
def test_placed_boundaries_are_in_the_rendered_rows(name):
    """every hand-placed voice that was kept has its stage end exactly on the row it was placed for (envelopes.boundary_rows; a
    gate_off is compared directly by the definition, so it is its own value), and the strides are the case's"""
    b = B.build(name)
    c = b.case
    rows = c.N * c.K
    hit = E.boundary_rows(b.env, c.position, rows) if all(v.shape[1] == c.V for v in b.env.values()) else \
        E.boundary_rows({k: np.broadcast_to(v, (1, c.V)) for k, v in b.env.items()}, c.position, rows)
    for k in B.PARAMS:
        assert b.env[k].shape == ((1, 1) if k in B.COMMON[c.env] else (1, c.V)), (name, k)
    assert hit.any(), name
    for v, p in b.placed:
        assert c.position <= p.frame < c.position + rows, (name, p)
        if p.stage == 'gate_off':
            assert b.env['gate_off'][0, v if b.env['gate_off'].shape[1] > 1 else 0] == p.frame / B.RATE, (name, v, p)
        else:
            assert hit[p.frame - c.position, v], (name, v, p)
    assert 0.0 <= b.level.min() and b.level.max() <= 1.0 and np.ptp(b.level) > 0.5, name


def test_placed_boundaries_cover_every_target_and_stage():
    """over the table: each stage end on each target row -- a block's first output row, the first and last row of a chunk of 8 and of
    16 window rows, window rows 63, 64 and 65 -- under four voices per lane and under one"""
    met = {4: set(), 1: set()}
    for name in ENVELOPED:
        b = B.build(name)
        vpt = B.expected_variant(b.case).vpt
        met[vpt] |= {(p.target, p.stage) for _, p in b.placed}
        if b.case.K > 1:
            met[vpt] |= {('later block', p.stage) for _, p in b.placed if p.block and p.target == 'first'}
    want = {(t, s) for t in B.TARGETS + ('later block',) for s in B.STAGES}
    for vpt in (4, 1):
        assert met[vpt] >= want, (vpt, sorted(want - met[vpt]))


# --------------------------------------------------------------------------------------- the restatement against the oracle's graph
class Rows(R.Node):
    """the materialised input as an oracle node: row r of `x` is frame `first` + r, frames outside it are zeros (only the `after`
    window of the last block reads there, which no kept sample depends on)"""
    cached = False

    def __init__(self, x, first):
        super().__init__()
        self.x, self.first = x, first

    def eval(self, position, frames, channels, rate):
        out = np.zeros((frames, self.x.shape[1]))
        lo, hi = max(position, self.first), min(position + frames, self.first + self.x.shape[0])
        if hi > lo:
            out[lo - position:hi - position] = self.x[lo - self.first:hi - self.first]
        return out


class BlockRows(R.Node):
    """per-block control rows: row b for the block that starts at position + b N"""
    cached = False

    def __init__(self, rows, position, N):
        super().__init__()
        self.rows, self.position, self.N = rows, position, N

    def eval(self, position, frames, channels, rate):
        b = (position - self.position) // self.N if self.rows.shape[0] > 1 else 0
        return self.rows[b][None, :]


@pytest.mark.parametrize('name', ['v4_dead_lane_c4', 'v4_growing_context', 'e4_c1', 'e1_c4'])
def test_restatement_equals_the_oracle_graph(name):
    """SumBus(Filter(x)) / SumBus(RingMod(Filter(x), ADSR)) rendered block by block by chain_ref.render_stream (context 100: the
    oracle's own), with per-block cutoff rows and from position 0 among them"""
    b = B.build(name)
    c = b.case
    assert c.context == R.CONTEXT_FRAMES
    cutoff = np.broadcast_to(b.cutoff, (b.cutoff.shape[0], c.V))
    node = R.Filter(c.btype, Rows(b.x.array.astype(np.float64), c.position - B.history_of(c)), BlockRows(cutoff, c.position, c.N))
    if b.env is not None:
        node = R.Binary('RingMod', node, R.Adsr(**b.env))
    per_voice = R.render_stream(node, c.position, c.N, c.K, c.V)
    want = R.sum_bus(per_voice, None if b.gains is None else b.gains.array)
    assert np.array_equal(want, b.ref), (name, float(np.abs(want - b.ref).max()))


def test_inputs_are_deterministic():
    for name in ('v1_one_voice', 'e4_c4_short'):
        first, again = B.build(name), B.build.__wrapped__(name)
        assert np.array_equal(first.x.array, again.x.array) and np.array_equal(first.ref, again.ref) and np.array_equal(first.cutoff, again.cutoff)
        assert all(np.array_equal(first.env[k], again.env[k]) for k in (first.env or {}))
