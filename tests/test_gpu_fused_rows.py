"""The per-block-row span walker, fused_walk_kernel<KIND, VPT, GAIN, C, ROWS = true> (signals_amd/csrc/sig_fused_walk.h), called directly
through `_native.fused_rows` -- sig_fused_osc_biquad_rows / sig_fused_voice_bus_rows, *_fm, sig_fused_osc_pair_biquad /
sig_fused_voice_pair_bus -- at its launch edges: tests/fused_rows_cases.py has the cases, the float64 restatement and the bounds,
tests/test_fused_rows_host.py the census and the wrong kernels the cases have to catch.  `out` is a view inside an allocation filled
with SENTINEL (a padded leading dimension, a row in front and behind, 0, 1 or 2 columns into a 16-byte row: the store sink then takes
4, 1 or 2 voices per lane); every parameter table is a contiguous row slice of an allocation with a NaN row in front and behind, so a
read of row -1 or row K poisons the result.

  1. every case against the restatement under each of the eight forced geometries (set_fused_tuning(vpt, span, 0, 0)): every sample
     finite (but the bad cutoff's), within 1e-6 max(1, max|ref|), on the unpaired store sink within 2e-7 (3e-7 where a Sine voice
     leaves the recurrence); the status word clean; exact-phase waveforms on the store sink bit for bit the same under every geometry,
     a Sine on the recurrence within 1.2e-7.
  2. K blocks in one call against K calls of one block, each with its own rows and the right row in front; one-row tables against K
     identical rows, bit for bit, and against the plain entries sig_fused_osc_biquad / sig_fused_voice_bus.
  3. Sine on a bus with cutoff and / or gain rows under closed_form = 1 (fused_steady_bus_kernel<.., GROWS / CROWS> takes the waves
     that qualify), geometries (0, 0), (8, 4), (8, 1), (2, 3).
  4. the status word; 5. the refusals `_native.fused_rows` documents.

sig_fused_voice_bus_rows and its kin take buses of one and two channels; a bus of four with per-block parameters is refused by the
C entry (the engine renders it per node), so C = 4 is a leg of 5., not of 1.

Measured on an MI355X, max|got - float32(ref)| per leg over all cases and geometries of 1.:
    store sink, exact phase 7.3e-12; store sink, fast Sine 2.3e-10; store sink, Sine on the exact phase 1.19e-07 (swept, past 2^26
    cycles) and 1.19e-07 under FM (past 2^26 cycles, and the waves a row above rate / 4 takes off the recurrence); store sink, paired
    1.19e-07; bus C = 1 0; bus C = 2 9.5e-07 at max|ref| 8.9 (fm_sine_hp_bus2_qualify: one float32 unit of a bus in [8, 16)); closed_form = 1 legs 0.
So the ROWS instantiation holds the figures of tests/test_gpu_fused_walker.py (2e-7, 3e-7) as they stand.  One-row tables through the
rows entry against the plain entry: 0 in every sample (store and bus, geometries (1, 1), (4, 2), (2, 3)).  The file runs in 6.5 s.
Wrong kernels modelled in numpy (tests/test_fused_rows_host.py, none run on a GPU), cases each fails at 100x the outer bar: the next
block's warm-up designed with the current cutoff 19; weights swapped one block late 23; row 0 for the row in front 11; the FM row
indexed within the span 12; no new Sine seed at a block boundary 4; a dead lane with its voice's bus weight 20; a one-column table read
with stride `voices` 3.
"""
import numpy as np
import pytest
import torch

import fused_rows_cases as F
from gpu_helpers import gpu_ready
from helpers import RATE, f32, maxerr
from signals_amd import _native
from signals_amd.engine import CONTEXT as CTX

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENTINEL = F.SENTINEL
WORST = {}                                         # leg -> the largest max|got - float32(ref)| seen
LAUNCHES = [0]


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    gpu_ready()
    assert CTX == F.CTX and RATE == F.RATE
    yield
    _native.set_fused_tuning()                     # back to the launch heuristics


@pytest.fixture(autouse=True)
def _launch_cap():
    LAUNCHES[0] = 0
    yield
    assert LAUNCHES[0] <= F.LAUNCH_CAP, LAUNCHES[0]


def geometry(vpt, span, closed_form=0):
    """force voices per lane and blocks per lane, the walker (or, with closed_form, the closed form for the waves that qualify)"""
    _native.set_fused_tuning(vpt, span, closed_form, 0)


def guarded(array):
    """(allocation, rows): a float64 table as rows [1, 1 + rows) of an allocation whose first and last row are NaN; None stays None"""
    if array is None:
        return None, None
    rows, cols = array.shape
    wide = torch.full((rows + 2, cols), float('nan'), dtype=torch.float64, device=DEV)
    sub = wide[1:1 + rows]
    sub.copy_(torch.from_numpy(np.array(array)))                               # (a copy: the cases' arrays are read-only)
    assert sub.is_contiguous()
    return wide, sub


def place_out(rows, cols, offset):
    """(allocation, view): float32 (rows, cols) at `offset` columns of rows [1, 1 + rows) of a SENTINEL-filled allocation whose leading
    dimension is a multiple of 4 with columns to spare"""
    ld = (offset + cols + 3) // 4 * 4 + 4
    wide = torch.full((rows + 2, ld), SENTINEL, dtype=torch.float32, device=DEV)
    sub = wide[1:1 + rows, offset:offset + cols]
    assert wide.data_ptr() % 256 == 0 and sub.stride(0) == ld and ld % 4 == 0
    return wide, sub


def around(wide, sub, offset) -> bool:
    """everything of `wide` outside `sub` still holds SENTINEL"""
    host = wide.cpu().numpy().copy()
    host[1:1 + sub.shape[0], offset:offset + sub.shape[1]] = SENTINEL
    return bool((host == SENTINEL).all())


def run(c: F.Case, I: F.Inputs, position=None, K=None, status=0, **changes):
    """one launch of `_native.fused_rows`: (out as float32 numpy, the status word, whether every sentinel is intact)"""
    position, K = c.position if position is None else position, c.K if K is None else K
    t = {k: guarded(getattr(I, k))[1] for k in F.Inputs._fields}
    pair = (c.source[0], c.source[1], t['hertz2'], t['phase2'], t['mix']) if F.is_pair(c) else None
    bus = c.sink != 'store'
    offset = 0 if bus else c.offset
    wide, out = place_out(K * c.N, F.channels_of(c), offset)
    word = torch.full((1,), status, dtype=torch.int32, device=DEV)
    args = dict(hertz=t['hertz'], phase=t['phase'], cutoff=t['cutoff'], gain=t['gain'], out=out, bus_gains=t['pan'], bus=bus, status=word,
                pair=pair, hertz_hist=t['hertz_hist'], phase_hist=t['phase_hist'])
    args.update(changes)
    _native.fused_rows(c.kind, c.btype, RATE, position, c.N, K, CTX, c.V, **args)
    torch.cuda.synchronize()
    LAUNCHES[0] += 1
    return out.cpu().numpy().copy(), int(word.item()), around(wide, out, offset)


def run_plain(c: F.Case, I: F.Inputs):
    """the same launch through the entries without per-block rows: sig_fused_osc_biquad / sig_fused_voice_bus"""
    t = {k: guarded(getattr(I, k))[1] for k in F.Inputs._fields}
    offset = 0 if c.sink != 'store' else c.offset
    wide, out = place_out(c.K * c.N, F.channels_of(c), offset)
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    if c.sink == 'store':
        _native.fused_osc_biquad(c.kind, c.btype, RATE, c.position, c.N, c.K, CTX, t['hertz'], t['phase'], t['cutoff'], t['gain'], out, status=word)
    else:
        _native.fused_voice_bus(c.kind, c.btype, RATE, c.position, c.N, c.K, CTX, c.V, t['hertz'], t['phase'], t['cutoff'], t['gain'], t['pan'], out,
                                status=word)
    torch.cuda.synchronize()
    LAUNCHES[0] += 1
    return out.cpu().numpy().copy(), int(word.item()), around(wide, out, offset)


def held_to(got, b: F.Built, what, tight=True):
    """a float32 result against the case's restatement: written, finite where the reference is (helpers.maxerr: the same NaN pattern),
    within the outer bar and, with `tight`, the case's tighter bound; returns max|got - float32(ref)|"""
    assert got.dtype == np.float32 and not (got == SENTINEL).any(), what
    err = maxerr(got, f32(b.ref))
    bound = F.tight_bound(b.case, b.inputs) if tight else None
    print(f'fused rows: {what}: max|got - f32(ref)| {err:.3g}, outer bar {F.outer_bar(b.ref):.3g}, tighter bound {bound}')
    assert err <= F.outer_bar(b.ref), (what, err, F.outer_bar(b.ref))
    assert bound is None or err < bound, (what, err, bound)
    return err


# ------------------------------------------------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize('name', [c.name for c in F.CASES])
def test_case_against_the_restatement_under_every_geometry(name):
    b = F.build(name)
    c, I = b.case, b.inputs
    flagged = F.BAD_CUTOFF if c.special == 'bad_cutoff' else 0
    first = None
    for vpt, span in F.GEOMETRIES:
        geometry(vpt, span)
        got, status, intact = run(c, I)
        what = (name, vpt, span)
        assert intact, what
        assert status == flagged, (what, status)
        err = held_to(got, b, what)
        leg = F.leg_of(c, I)
        WORST[leg] = max(WORST.get(leg, 0.0), err)
        if first is None:
            first = got
        elif c.sink == 'store' and c.kind != 'Sine':
            assert np.array_equal(got, first, equal_nan=True), (what, maxerr(got, first))      # exact phase: bit for bit
        elif c.sink == 'store' and c.special is None:
            assert maxerr(got, first) < 1.2e-7, (what, maxerr(got, first))                    # the recurrence, seeded per span or block
    print(f'fused rows: largest so far by leg: {WORST}')


# ------------------------------------------------------------------------------------------------ 2. the same rows another way
def one_ulp(ref) -> float:
    """a float32 unit in the last place at the bus's full scale: float64 sums of the same terms in another order round apart by it"""
    return float(np.spacing(np.float32(max(1.0, np.nanmax(np.abs(ref))))))


@pytest.mark.parametrize('name', F.BATCHING)
def test_blocks_in_one_call_equal_one_block_calls(name):
    """K blocks under (4, 8) -- every boundary inside a span where N >= CTX -- against K launches of one block with rows b of the
    tables and, under FM, row b - 1 in front (the launch's own row in front for b = 0).  Store sink: exact-phase waveforms bit for
    bit, Sine (seeded per span there, per block here) within 1.2e-7; a bus: within one float32 unit of its full scale"""
    b = F.build(name)
    c, I = b.case, b.inputs
    geometry(4, 8)
    whole, status, intact = run(c, I)
    assert status == 0 and intact
    held_to(whole, b, (name, 'whole'))
    for k in range(c.K):
        rows = {}
        for t in F.TABLES:
            a = getattr(I, t)
            rows[t] = a if a is None or a.shape[0] == 1 else a[k:k + 1]
        for t in ('hertz', 'phase'):
            front = getattr(I, t + '_hist')
            rows[t + '_hist'] = front if front is None or k == 0 else getattr(I, t)[k - 1:k]
        alone, status, intact = run(c, I._replace(**rows), position=c.position + k * c.N, K=1)
        assert status == 0 and intact, (name, k)
        part = whole[k * c.N:(k + 1) * c.N]
        if c.sink != 'store':
            assert maxerr(alone, part) <= one_ulp(b.ref), (name, k, maxerr(alone, part))
        elif c.kind == 'Sine':
            assert maxerr(alone, part) < 1.2e-7, (name, k, maxerr(alone, part))
        else:
            assert np.array_equal(alone, part), (name, k, maxerr(alone, part))


@pytest.mark.parametrize('name', F.ONE_ROW)
def test_one_row_tables(name):
    """(1, V) cutoff and gain through the rows entry = K identical rows, bit for bit (the walker designs each block again from the
    same numbers), and = the plain entry within the outer bar (there the Sine seed and the gain are folded another way)"""
    b = F.build(name)
    c, I = b.case, b.inputs
    repeated = I._replace(cutoff=np.repeat(I.cutoff, c.K, axis=0), gain=None if I.gain is None else np.repeat(I.gain, c.K, axis=0))
    for vpt, span in ((1, 1), (4, 2), (2, 3)):
        geometry(vpt, span)
        one, status, intact = run(c, I)
        assert status == 0 and intact
        held_to(one, b, (name, vpt, span))
        rows, status, intact = run(c, repeated)
        assert status == 0 and intact and np.array_equal(rows, one), (name, vpt, span, maxerr(rows, one))
        plain, status, intact = run_plain(c, I)
        assert status == 0 and intact
        diff = maxerr(plain, one)
        print(f'fused rows: {name} ({vpt}, {span}): rows entry against the plain entry: {diff:.3g}')
        WORST['rows entry against the plain entry'] = max(WORST.get('rows entry against the plain entry', 0.0), diff)
        assert diff <= F.outer_bar(b.ref), (name, vpt, span, diff)
    print(f'fused rows: largest so far by leg: {WORST}')


# --------------------------------------------------------------------------------------------------------- 3. the closed form
@pytest.mark.parametrize('name', F.STEADY)
def test_closed_form_with_per_block_rows(name):
    b = F.build(name)
    c, I = b.case, b.inputs
    for vpt, span in F.STEADY_GEOMETRIES:
        geometry(vpt, span, closed_form=1)
        got, status, intact = run(c, I)
        assert status == 0 and intact, (name, vpt, span)
        err = held_to(got, b, (name, vpt, span, 'closed form'))
        WORST['closed_form = 1'] = max(WORST.get('closed_form = 1', 0.0), err)
    print(f'fused rows: largest so far by leg: {WORST}')


# ------------------------------------------------------------------------------------------------------- 4. the status word
def test_bad_cutoff_is_flagged_and_stays_in_its_block():
    """cutoff[2, 40] = 0: exactly voice 40's rows of block 2 are NaN (helpers.maxerr compares the NaN pattern), every other sample --
    block 3 of voice 40, whose warm-up chain ran beside the poisoned one, included -- meets the bounds; SIG_STATUS_BAD_CUTOFF joins a
    bit that was set before; the same launch with that cutoff mended leaves the word alone"""
    b = F.build(F.STATUS_CASE)
    c, I = b.case, b.inputs
    blk, v = F.BAD_AT
    for vpt, span in ((1, 1), (4, 2)):
        geometry(vpt, span)
        got, status, intact = run(c, I, status=4)
        assert status == (4 | F.BAD_CUTOFF) and intact, (vpt, span, status)
        held_to(got, b, ('bad cutoff', vpt, span))
        assert np.isnan(got[blk * c.N:(blk + 1) * c.N, v]).all() and np.isnan(got).sum() == c.N
        got, status, intact = run(c, I, status=0)
        assert status == F.BAD_CUTOFF and intact and np.isnan(got).sum() == c.N
    mended = I.cutoff.copy()
    mended[blk, v] = 1000.0
    got, status, intact = run(c, I._replace(cutoff=mended), status=4)
    assert status == 4 and intact and np.isfinite(got).all()
    keep = np.isfinite(b.ref)
    assert maxerr(got[keep], f32(b.ref)[keep]) < 2e-7


# ---------------------------------------------------------------------------------------------------------- 5. the refusals
def test_refusals():
    """what `_native.fused_rows` and the C entries behind it refuse, in front of any launch: NativeError and `out` untouched"""
    b = F.build('fm_sine_lp_store')
    c, I = b.case, b.inputs
    swept = F.build('swept_square_hp_bus2')
    pair = F.build('pair_mix_saw_square')
    short = F.build('swept_square_lp_store_short')
    wide, out = place_out(c.K * c.N, c.V, 0)
    dev = lambda a: guarded(a)[1]
    refused = {
        'FM and a second oscillator': (c, I, dict(pair=(F.MIX, 'Sine', dev(I.hertz[:1]), dev(I.phase[:1]), dev(I.phase[:1])))),
        'cutoff rows neither 1 nor K': (swept.case, swept.inputs, dict(cutoff=dev(swept.inputs.cutoff[:3]))),
        'gain rows neither 1 nor K': (swept.case, swept.inputs, dict(gain=dev(swept.inputs.gain[:3]))),
        'hertz_hist of the wrong width': (c, I, dict(hertz_hist=dev(I.hertz_hist[:, :c.V - 1]))),
        'phase rows without phase_hist': (c, I, dict(phase_hist=None)),
        'FM below the context': (short.case._replace(source='fm'), short.inputs._replace(hertz_hist=short.inputs.hertz), {}),
        'Mix without a mix row': (pair.case, pair.inputs._replace(mix=None), {}),
        'a bus of four channels': (swept.case._replace(sink=4), swept.inputs._replace(pan=np.concatenate([swept.inputs.pan] * 2)), {}),
    }
    assert tuple(refused) == F.REFUSALS
    for what, (rc, rI, changes) in refused.items():
        if rc.sink == 'store' and rc.V == c.V and rc.N == c.N:
            changes = dict(changes, out=out)                                   # the guarded `out`: a refusal writes nothing
        with pytest.raises(_native.NativeError):
            run(rc, rI, **changes)
        LAUNCHES[0] = 0
    torch.cuda.synchronize()
    assert bool((wide == SENTINEL).all())
    geometry(4, 2)
    got, status, intact = run(c, I)                                             # the same arguments unchanged: a launch
    assert status == 0 and intact
    held_to(got, b, 'accepted')


def test_figures():
    """the figures of the module docstring, as measured by the tests above (when the whole file ran)"""
    print('fused rows: max|got - float32(ref)| by leg:', ', '.join(f'{k} {v:.3g}' for k, v in sorted(WORST.items())))
