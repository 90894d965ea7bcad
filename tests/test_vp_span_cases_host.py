"""The cases of tests/test_gpu_vp_spans.py (tests/vp_span_cases.py), checked on the CPU with the oracle alone: that the inputs can tell
a wrong kernel from a right one, and that the arithmetic the shapes rest on still holds.  No GPU call is made here.

    - the block length puts the first warm row inside a row group and leaves single-row groups at the end of every block, for both
      register files; the geometries give the lanes the blocks the GPU test's docstring says they own;
    - the case lists: all 13 families as small, full and swept voices, the five deep ones;
    - every swept control matters in every block: the oracle with ONE control held at the row of a batch's first block -- what a
      lane that did not reload, or redesign from, the rows of the later blocks of its span would compute -- differs from the true
      oracle by at least 10 x the GPU test's tolerance in every later block of that batch;
    - the context matters in every block: the oracle with every filter cold-started on 99 rows instead of 100 -- a chain started one
      row late -- differs from the true one by at least 10 x the tolerance in every block after the first of the render (the first
      block at position 0 has no context; at the fresh start every block has).

The factor 10 is a condition on the inputs (LFO depths and rates, cutoffs), not a measurement of any kernel.  Each check prints the
ratios it measured."""
import functools

import numpy as np
import pytest

import vp_span_cases as C
from test_gpu_mixed import tolerance
from test_gpu_vp_variants import FAMILIES, scale

FACTOR = 10.0


@functools.lru_cache(maxsize=None)
def wanted(kind, family, render):
    want = C.oracle(C.build(kind, family)[1], render)
    want.setflags(write=False)
    return want


def block_errors(a, b, frames):
    """max |a - b| per block"""
    return np.abs(a - b).reshape(-1, frames, a.shape[1]).max(axis=(1, 2))


def test_the_block_length_splits_row_groups():
    assert C.CONTEXT == 100 and C.N > C.CONTEXT > C.SHORT_N
    from oracle import chain_ref as R
    assert R.CONTEXT_FRAMES == C.CONTEXT
    import re
    from signals_amd import _native
    header = (_native.LIB_PATH.parent / 'sig_vp_machine.h').read_text()
    rows = int(re.search(r'^#define SIG_VP_ROWS (\d+)$', header, flags=re.M).group(1))
    assert 'constexpr int kRowGroup = SIG_VP_ROWS;' in header and 'constexpr int RG = SMALL ? kRowGroup : kRowGroup / 2;' in header
    assert C.ROW_GROUPS == (rows // 2, rows)                                  # the full and the small register file
    for rg in C.ROW_GROUPS:
        assert (C.N - C.CONTEXT) % rg != 0, rg                                # the next block's chains start inside a group
        assert C.N % rg != 0, rg                                              # every block ends in single-row groups
    assert (C.N - C.CONTEXT) % 4 == 2 and (C.N - C.CONTEXT) % 8 == 6


def test_the_lanes_own_the_blocks_the_table_claims():
    spans = {span for _, span in C.GEOMETRIES}
    assert {(span, K) for span in spans for K in C.KS} | {(C.FRESH[2][1], C.FRESH[1])} == set(C.OWNED)
    for (span, K), blocks in C.OWNED.items():
        assert C.owned(span, K) == blocks, (span, K)
        assert sorted(b for lane in blocks for b in lane) == list(range(K))
    assert any(len(lane) > 1 for (span, K), blocks in C.OWNED.items() for lane in blocks)
    assert [len(lane) for lane in C.OWNED[2, 3]] == [2, 1] and [len(lane) for lane in C.OWNED[3, 4]] == [3, 1]     # ragged last spans
    assert all(len(C.OWNED[16, K]) == 1 for K in C.KS)                        # a span longer than the batch: one lane


def test_the_case_lists_are_complete():
    cases = C.voices()
    assert len(cases) == len(set(cases)) == 13 * 3 + 5
    for kind in C.KINDS:
        assert [f for k, f in cases if k == kind] == list(FAMILIES), kind
    assert len(FAMILIES) == 13 and set(C.SWEPT) == set(FAMILIES)
    assert sorted(f for k, f in cases if k == 'deep') == sorted(('plain', 'band', 'resonant', 'resonant_eq', 'mixed')) == sorted(C.DEEP)
    assert set(C.SHORT_DEEP) <= set(C.DEEP)
    assert {key for key in C.VARIANT} == {('swept', f) for f in FAMILIES} | {('deep', f) for f in C.DEEP}


@pytest.mark.parametrize('family', FAMILIES)
def test_every_swept_control_matters_in_every_block(family):
    want = wanted('swept', family, 'long')
    assert np.isfinite(want).all()
    tol = tolerance(want) * scale(family)
    _, _, handles = C.swept(family)
    assert tuple(handles) == C.SWEPT[family]
    first = 0
    for K in C.KS:                                                            # the batches: blocks [first, first + K)
        for control in handles:
            _, ref, h = C.swept(family)
            C.freeze(h, control, C.POSITION + first * C.N)
            ratio = block_errors(C.oracle(ref, 'long'), want, C.N)[first:first + K] / tol
            print('vp span frozen', family, control, 'batch from block', first, 'err/tol per block', np.round(ratio, 1))
            assert ratio[0] == 0.0 or first > 0                               # (block 0 reads the very row it was frozen at)
            assert (ratio[1:] >= FACTOR).all(), (family, control, first, ratio)
        first += K


CONTEXT_CASES = [(kind, family, 'long') for kind, family in C.voices() if kind != 'swept'] + [('deep', family, 'fresh') for family in C.DEEP]


@pytest.mark.parametrize('kind,family,render', CONTEXT_CASES)
def test_one_row_less_context_shows_in_every_block(kind, family, render):
    want = wanted(kind, family, render)
    assert np.isfinite(want).all()
    tol = tolerance(want) * scale(family)
    with C.context_rows(C.CONTEXT - 1):
        short = C.oracle(C.build(kind, family)[1], render)
    again = C.oracle(C.build(kind, family)[1], render)                        # (the context is back)
    assert np.array_equal(again, want)
    position, frames, _ = C.RENDERS[render]
    ratio = block_errors(short, want, frames) / tol
    print('vp span 99 rows', kind, family, render, 'err/tol per block', np.round(ratio, 1))
    assert (ratio[(0 if position >= C.CONTEXT else 1):] >= FACTOR).all(), (kind, family, render, ratio)
    if position == 0:
        assert ratio[0] == 0.0                                                # no context in front of position 0
