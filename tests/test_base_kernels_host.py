"""The case tables of tests/base_kernel_cases.py, checked without a GPU: every kernel variant the dispatchers can choose is meant
to be reached, the inputs are the same on every build, the exact-arithmetic inputs are exact, and the tables stay within their
caps."""
import numpy as np
import pytest

import base_kernel_cases as K


def same(a: K.Built, b: K.Built) -> bool:
    views = lambda built: [v for v in list(built.operands.values()) + [built.out] if v is not None]
    return (all(x.pad == y.pad and x.ld_extra == y.ld_extra and x.array.dtype == y.array.dtype and np.array_equal(x.array, y.array)
                for x, y in zip(views(a), views(b))) and np.array_equal(a.ref, b.ref, equal_nan=True))


@pytest.mark.parametrize('kernel', list(K.VARIANTS))
def test_every_variant_is_reached(kernel):
    reached = set()
    for case in K.CASES[kernel]:
        got = K.expected_variant(kernel, case)
        reached.update(got if isinstance(got, tuple) else (got,))
    assert reached == set(K.VARIANTS[kernel]), (kernel, sorted(set(K.VARIANTS[kernel]) - reached))


def test_the_edges_the_tables_are_there_for():
    fast = [c for c in K.EW_CASES if K.expected_variant('elementwise', c) == 'fast']
    for op in ('Gain', 'Mix', 'RingMod', 'Amp'):
        mine = [c for c in fast if c[0] == op]
        assert {3, 4, 15, 16, 17, 67} <= {c[1] for c in mine} and {4, 252, 256, 260} <= {c[2] for c in mine}, op
        if op != 'RingMod':
            assert {'s11', 'row', 'blk4', 'blk8'} <= {c[4] for c in mine}, op
    generic = [c for c in K.EW_CASES if K.expected_variant('elementwise', c) == 'generic']
    assert any(c[4] == 'blk6' and c[5] == 'f32' and c[3] in ('contig', 'pad4', 'ld4') and c[2] % 4 == 0 for c in generic)
    assert K.EW_GRID_STRIDE in generic and K.EW_GRID_STRIDE[1] * K.EW_GRID_STRIDE[2] > 16384 * 256
    # sum_bus: every fast kernel with a ragged row group, C = 4, the wrapper's splits, the cap
    for chunks in (1, 2, 3, 4):
        rows = {c[1] for c in K.BUS_CASES if f'fast-{chunks}' in K.expected_variant('sum_bus', c)}
        assert any(r % 4 for r in rows) and any(r > 4 and r % 4 for r in rows), chunks
    assert {K.bus_widths(C) for C in (3, 5, 7)} == {(2, 1), (4, 1), (4, 2, 1)}
    assert {'mono', 1, 2, 3, 4, 5, 7} <= {c[2] for c in K.BUS_CASES}
    V, rows = K.BUS_CAP[:2]
    assert K.expected_variant('sum_bus', K.BUS_CAP) == ('fast-1',) and ((rows + 3) // 4 + 3) // 4 > 2048 and rows % 4
    assert any(c[0] == 256 and c[5] == 'pad1' and K.expected_variant('sum_bus', c) == ('generic-scalar',) for c in K.BUS_CASES)
    # mix_matrix: more items than the 2048 wave slots of the default launch, with a ragged last tile
    items = [((rows + 31) // 32) * (V // 64) for rows, V, _, _ in K.MIX_CASES]
    assert sorted(items)[-2:] == [2049, 2112] and all(rows % 32 for rows, _, _, _ in K.MIX_CASES)
    # adsr / osc: a second voice tile with one live lane under both tilings, both ends of the row tiles
    for kernel in ('adsr', 'adsr_apply', 'osc'):
        met = {(K.expected_variant(kernel, c), c[1]) for c in K.CASES[kernel]}
        assert {('VEC4', 260), ('VEC4', 256), ('VEC4', 4), ('VEC1', 65), ('VEC1', 3), ('VEC1', 1), ('VEC1', 260)} <= met, kernel
        assert {1, 15, 16, 17, 64, 65} <= {c[2] for c in K.CASES[kernel]}, kernel
    assert {c[3] for c in K.ADSR_CASES} == {0, 2 ** 31 + 5} and {c[3] for c in K.OSC_CASES} == {0, K.HOUR + 7}


def test_case_counts_and_no_duplicates():
    tables = {'elementwise': K.EW_CASES, 'sum_bus': K.BUS_CASES, 'mix_matrix': K.MIX_CASES, 'adsr': K.ADSR_CASES, 'osc': K.OSC_CASES}
    for name, table in tables.items():
        assert len(set(table)) == len(table), name
        assert len(table) <= K.CAPS[name], (name, len(table))
    assert K.CAPS['elementwise'] <= 150


def test_inputs_are_deterministic():
    for case in K.EW_CASES:
        assert same(K.ew_build(case), K.ew_build(case)), case
    for case in K.BUS_CASES[:-1]:
        for leg in ('exact', 'random'):
            assert same(K.bus_build(case, leg), K.bus_build(case, leg)), case
    for case in K.MIX_CASES[:5]:
        for leg in ('exact', 'random'):
            assert same(K.mix_build(case, leg), K.mix_build(case, leg)), case
    for case in K.ADSR_CASES:
        assert same(K.adsr_build(case), K.adsr_build(case)), case
    for case in K.OSC_CASES:
        assert same(K.osc_build(case), K.osc_build(case)), case


def exact(x: np.ndarray, weights: np.ndarray, ref: np.ndarray):
    """integers times multiples of 1/8 whose sums of magnitudes stay below 2^24 eighths: exact in float32 in any order"""
    assert np.array_equal(x, np.rint(x)) and np.abs(x).max() <= 8
    assert np.array_equal(weights * 8, np.rint(weights * 8)) and np.abs(weights).max() <= 2
    assert float((np.abs(x) @ np.abs(weights)).max()) * 8 < 2 ** 24
    assert np.array_equal(ref, ref.astype(np.float32).astype(np.float64))


def test_exact_inputs_are_exact():
    for case in K.BUS_CASES:
        b = K.bus_build(case, 'exact')
        x = b.operands['x'].array.astype(np.float64)
        g = np.ones((1, x.shape[1])) if b.operands['gains'] is None else b.operands['gains'].array
        exact(x, g.T, b.ref)
    m = K.mix_matrix_of('exact').astype(np.float64)
    assert not np.array_equal(m, m.T)
    for case in K.MIX_CASES:
        b = K.mix_build(case, 'exact')
        x = b.operands['x'].array.astype(np.float64)
        exact(x.reshape(-1, 64), m, b.ref.reshape(-1, 64))


def test_references_are_worth_comparing_with():
    """no reference is trivially constant: Amp has NaNs and numbers, envelopes move, far positions are live"""
    negative = 0
    for case in K.EW_CASES:
        ref = K.ew_build(case).ref
        if case[0] == 'Amp' and case[2] >= 64 and case[4] != 's11':         # (one exponent for all: NaNs or numbers)
            assert np.isnan(ref).any() and np.isfinite(ref).any(), case
        negative += int(case[0] == 'Amp' and bool((ref[np.isfinite(ref)] < 0).any()))     # a negative base under a whole exponent
    assert negative >= 20
    live = 0
    for case in K.ADSR_CASES:
        b = K.adsr_build(case)
        assert b.ref.min() >= -1.0 and b.ref.max() <= 1.0
        live += int(case[1] >= 65 and np.ptp(np.abs(b.ref)) > 0.1)
        if case[1] >= 65:
            assert len(np.unique(b.ref)) > case[1] // 2, case
    assert live >= 15
