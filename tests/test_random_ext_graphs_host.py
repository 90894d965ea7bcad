"""The generator of tests/random_ext_graphs.py, without a GPU: the 32 seeds build the same graph twice, draw from every family in every
situation the engine's rules distinguish (the census), and give an oracle the GPU test can be held to -- finite rows that sound, and a
gain bound G <= 64 -- at every (position, N, K) the GPU test renders.  Nothing is rendered on a GPU here: the description and the
oracle graph (numpy and scipy) alone."""
import collections
import functools

import numpy as np
import pytest

import random_ext_graphs as G

SEEDS = G.SEEDS


@functools.lru_cache(maxsize=None)
def described(seed):
    """(entries, G, channels) of a seed, built once with both sides (the GPU node classes are plain Python until they render)"""
    graph = G.Builder(seed).build()
    assert graph.node is not None
    return graph.entries, graph.G, graph.channels


@pytest.mark.parametrize('seed', SEEDS)
def test_two_builds_of_a_seed_are_the_same_graph(seed):
    b = G.Builder(seed)
    one, two = b.build(), b.build()
    assert one.node is not two.node and one.ref is not two.ref                # fresh objects
    assert one.entries == two.entries and one.G == two.G and one.channels == two.channels
    assert G.Builder(seed).build(gpu=False).entries == one.entries            # (with or without the GPU side: the same draws)
    pos, N, batches = G.RENDERS[1]
    a, c = G.oracle_rows(one, pos, N, sum(batches)), G.oracle_rows(two, pos, N, sum(batches))
    assert a.dtype == np.float64 and np.array_equal(a, c, equal_nan=True)


@pytest.mark.parametrize('seed', SEEDS)
def test_the_oracle_is_usable(seed):
    """finite rows, max |oracle| > 0.01 and G <= 64 at every render of the GPU test (an unusable draw is drawn again inside the
    generator, as part of the seed's definition: Builder.attempt); the GPU node graph infers the width the oracle is asked for"""
    b = G.Builder(seed)
    graph = b.build()
    assert 1.0 <= graph.G <= G.G_MAX, graph.G
    assert graph.node.channels == graph.channels, (graph.node.channels, graph.channels)
    for pos, N, batches in G.RENDERS + (G.SHORT,):
        rows = G.oracle_rows(b.build(gpu=False), pos, N, sum(batches))
        assert rows.shape == (N * sum(batches), graph.channels)
        assert np.isfinite(rows).all(), (seed, pos)
        assert np.abs(rows).max() > 0.01, (seed, pos)
        assert G.tolerance(graph, rows) < 1e-3


def readers_in_series(entries):
    """(some history reader has another one below it, a Delay is among such a pair)"""
    def below(i):
        out = set()
        for j in entries[i].inputs:
            out |= {j} | below(j)
        return out
    series = delay = False
    for i, e in enumerate(entries):
        if e.family in G.READERS:
            under = [entries[j] for j in below(i) if entries[j].family in G.READERS]
            series |= bool(under)
            delay |= bool(under) and (e.family == 'Delay' or any(u.family == 'Delay' for u in under))
    return series, delay


def test_census():
    """every family in at least 3 seeds; per family, where it can: read with history, with a modulated port, one column wide under a
    reader V wide, shared between a reader that asks for history rows and one that asks for none; two history readers in series in at
    least 8 seeds, a Delay among them in at least 3"""
    seeds_of = collections.defaultdict(set)
    seen = collections.defaultdict(set)
    taps, kinds = set(), set()
    series = delays = 0
    for seed in SEEDS:
        entries, _, _ = described(seed)
        for e in entries:
            seeds_of[e.family].add(seed)
            kinds.add(e.kind)
            for what in ('reads_history', 'modulated', 'narrow_under_wide', 'shared_mixed'):
                if getattr(e, what):
                    seen[what].add(e.family)
            assert e.width in (1, G.V) or e.family == 'SumBus'
            assert e.width == G.V or e.family not in G.ALWAYS_WIDE
        s, d = readers_in_series(entries)
        series += s
        delays += d
    table = {f: (len(seeds_of[f]), *(f in seen[w] for w in ('reads_history', 'modulated', 'narrow_under_wide', 'shared_mixed'))) for f in G.FAMILIES}
    print('family: seeds, read with history, modulated, narrow under wide, shared by a history reader and a plain one')
    for f, row in table.items():
        print(f'  {f:18s}', *row)
    print('series', series, 'with a Delay', delays, 'kinds', sorted(kinds))
    missing = []
    for f in G.FAMILIES:
        if len(seeds_of[f]) < 3:
            missing.append((f, 'seeds', len(seeds_of[f])))
        if f == 'SumBus':
            continue                                                          # (the sink: nothing reads it, no control port, as wide as its gains)
        if f not in seen['reads_history']:
            missing.append((f, 'reads_history'))
        if f not in seen['shared_mixed']:
            missing.append((f, 'shared_mixed'))
        if f not in G.NO_CONTROL and f not in seen['modulated']:
            missing.append((f, 'modulated'))
        if f not in G.ALWAYS_WIDE and f not in seen['narrow_under_wide']:
            missing.append((f, 'narrow_under_wide'))
    assert not missing, missing
    assert series >= 8 and delays >= 3, (series, delays)
    for kind in ('Delay,1', 'Delay,3', 'Delay,16', 'Sampler,loop', 'Sampler,one-shot', 'PMSine', 'PMSawtooth', 'LowShelf', 'HighShelf',
                 'BlepSquare', 'BlepSawtooth', 'SyncSawtooth', 'SyncSquare', 'ResonantLowPass', 'ResonantHighPass', 'LowPass', 'HighPass',
                 'BandPass', 'BandStop', 'Sine', 'Square', 'Sawtooth', 'Triangle'):
        assert kind in kinds, kind
    assert any(described(seed)[2] == 1 for seed in SEEDS) and any(described(seed)[2] == 2 for seed in SEEDS)      # a bus without and with gains
    assert sum(described(seed)[2] == G.V for seed in SEEDS) >= 8              # and graphs without one


def test_the_gain_bound_is_the_worst_path():
    """G from the description: the product of the nodes' bounds along the worst path, computed by hand for one seed's entries"""
    for seed in list(SEEDS)[:8]:
        b = G.Builder(seed)
        graph = b.build(gpu=False)
        gains = [n['g'] for n in b.nodes]

        def path(i):
            return gains[i] * max([1.0] + [path(j) for j in graph.entries[i].inputs])
        assert graph.G == path(len(gains) - 1)
        assert all(1.0 <= g <= 2.0 + 1e-9 for g in gains), gains              # every family's bound inside its range's: q <= 2, +6 dB, L <= 2


def test_control_positions_cover_every_block_of_every_render():
    for pos, N, batches in G.RENDERS + (G.SHORT,):
        for b in range(sum(batches)):
            assert pos + b * N in G.CONTROL_POSITIONS
        assert max(pos - G.CONTEXT, 0) in G.CONTROL_POSITIONS
