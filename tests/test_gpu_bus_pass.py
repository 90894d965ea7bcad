"""The filter-and-bus pass, sig_biquad_coldstart_bus (signals_amd/csrc/biquad_bus.hip), called directly through
`_native.biquad_coldstart_bus` at its group, tile and envelope edges: tests/bus_pass_cases.py has the cases, the float64 restatement
and the bound, tests/test_bus_pass_host.py the census of what they reach.  Every buffer is a view into an allocation whose other
elements hold a sentinel: NaN around the input and the gains (a read outside a view poisons the sums), SENTINEL around and under `out`.

  1. every case against the restatement, every sample: |got - ref| <= half a float32 unit in the last place of ref + the summation
     term V 2^-53 (|y env| @ |w|^T) + the recurrence term (4 |y64 - y80|) @ |w|^T; against float32(ref) the same, but for samples
     whose ref lies within the last two terms of a float32 rounding midpoint, where float32(ref) itself may fall either side: one unit
     more.  The project's 1e-6 max(1, max|ref|) as an outer bar.
  2. bit for bit: K blocks in one call against K calls of one block; dead voices against live ones with gain 0; a bus of four
     channels against two against one; K identical cutoff rows against one.
  3. four voices per lane against one voice per lane: within twice the summation term (the order of the sums differs).
  4. the status word; 5. the refusals and the empty launches of the C entry; 6. the engine's default route into the kernel.

Measured on an MI355X over the cases of 1. (the largest of each over all samples of all cases): |got - ref| 1.98e-07 under a half
unit of 2.38e-07, a summation term of 8.76e-12 and a recurrence term of 2.3e-13; |got - ref| exceeded the half unit alone in no sample
(the largest |got - ref| - half unit: -8.0e-25), |got - float32(ref)| was 0 in every sample of every case, and the two kernels of 3.
differed in no sample.  The engine routes of 6.: 4.8e-07 to 9.5e-07 at max|oracle| 7.9 to 11.4 (Delay, Mix), 6.0e-08 at 1 to 1.5 (Ladder).

Three deliberately wrong kernels, modelled in numpy against the case table (not run): the flush's k_lo one too large (a block's first
output row left unstored) fails 1. in the 32 cases whose blocks have a ragged front group, v4_ragged_front_c4 (C = 4, context 6) among
them; q_lane refreshed from the block's row instead of the window's (the envelope c rows late) fails 1. in 14 of the 17 envelope cases,
every one whose blocks have context rows and a moving envelope; a dead lane with weight 1 fails 1. in the 37 cases whose last voice
tile has dead lanes, and test_dead_voices.
"""
import numpy as np
import pytest
import torch

import bus_pass_cases as B
import envelopes as E
from gpu_helpers import gpu_ready, tolerance
from helpers import RATE, f32, fix, maxerr, mkosc
from signals_amd import _native

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENTINEL = B.SENTINEL
INVALID_VALUE = 1                                  # hipErrorInvalidValue
TORCH_DTYPE = {np.float32: torch.float32, np.float64: torch.float64}
LAUNCHES = {}                                      # test -> launches made, against bus_pass_cases.launches()


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    gpu_ready()


def place(array: np.ndarray, pad: int, ld_extra: int, fill: float, copy: bool = True):
    """(buffer, view): `array` as the columns [pad, pad + V) of rows [1, 1 + rows) of a buffer pad + V + ld_extra columns wide with a row
    in front and a row behind, everything else (without `copy`: everything) `fill`"""
    rows, V = array.shape
    wide = torch.full((rows + 2, pad + V + ld_extra), fill, dtype=TORCH_DTYPE[array.dtype.type], device=DEV)
    sub = wide[1:1 + rows, pad:pad + V]
    assert wide.data_ptr() % 256 == 0 and sub.stride(0) == pad + V + ld_extra
    if copy:
        sub.copy_(torch.from_numpy(np.array(array)))                           # (a copy: the cases' arrays are read-only)
    return wide, sub


def around(wide: torch.Tensor, sub: torch.Tensor, fill: float) -> bool:
    """everything of `wide` outside `sub` (rows [1, 1 + rows), the view's columns) still holds `fill`"""
    host = wide.cpu().numpy().copy()
    pad = (sub.data_ptr() - wide.data_ptr()) // wide.element_size() % wide.stride(0)
    host[1:1 + sub.shape[0], pad:pad + sub.shape[1]] = fill
    return bool(np.isnan(host).all()) if np.isnan(fill) else bool((host == fill).all())


class Stage:
    """the operands of a launch on the device.  From a case's Built, with `live` the first voices of its buffers only, `layout` another
    layout of x, `gains` other gain rows (None: mono), `cutoff` other cutoff rows"""

    def __init__(self, b: B.Built, layout=None, gains='own', cutoff=None, env='own'):
        c = self.case = b.case
        pad, extra = B.LAYOUT[layout or c.layout]
        self.x_wide, self.x = place(b.x.array, pad, extra, float('nan'))
        g = (None if b.gains is None else b.gains.array) if isinstance(gains, str) else gains
        self.g_wide, self.g = (None, None) if g is None else place(g, 0, c.gains_extra, float('nan'))
        self.C = 1 if g is None else g.shape[0]
        self.cutoff = torch.from_numpy(np.array(b.cutoff if cutoff is None else cutoff)).to(DEV)
        rows = b.env if isinstance(env, str) else env
        self.env = None if rows is None else {k: torch.from_numpy(np.array(v)).to(DEV) for k, v in rows.items()}
        self.hist = B.history_of(c)

    def out(self, rows, C=None, extra=None):
        C = C or self.C
        return place(np.zeros((rows, C), dtype=np.float32), 0, self.case.out_extra if extra is None else extra, SENTINEL, copy=False)

    def run(self, test, live=None, block=None, status=0, cutoff=None):
        """one launch: the whole case, or its block `block` alone (reading its history from the same buffer); `live`: the first voices
        only.  Returns (out rows as float32 numpy, status word, whether every sentinel is intact)"""
        c = self.case
        V = live or c.V
        position, K, hist, first = c.position, c.K, self.hist, 0
        if block is not None:
            position, K = c.position + block * c.N, 1
            hist = min(c.context, position)
            first = self.hist + block * c.N - hist
        buf = self.x[first:first + hist + c.N * K, :V]
        gains = None if self.g is None else self.g[:, :V]
        cut = self.cutoff if cutoff is None else cutoff
        if cut.shape[1] > 1 and V != c.V:
            cut = cut[:, :V].contiguous()
        env = None if self.env is None else {k: (v if v.shape[1] == 1 or V == c.V else v[:, :V].contiguous()) for k, v in self.env.items()}
        wide, out = self.out(c.N * K)
        word = torch.full((1,), status, dtype=torch.int32, device=DEV)
        workspace = _native._bus_workspace(None, V, c.N * K, self.C, DEV)
        _native.biquad_coldstart_bus(c.btype, RATE, position, c.N, K, c.context, cut, buf, hist, gains, out, envelope=env,
                                     workspace=workspace, status=word)
        torch.cuda.synchronize()
        LAUNCHES[test] = LAUNCHES.get(test, 0) + 1
        intact = around(wide, out, SENTINEL) and around(self.x_wide, self.x, float('nan')) and \
            (self.g is None or around(self.g_wide, self.g, float('nan')))
        return out.cpu().numpy().copy(), int(word.item()), intact


def near_midpoint(ref, half, slack):
    """samples whose float64 reference lies within `slack` of the midpoint of two float32 values: float32(ref) may fall either side"""
    return np.abs(np.abs(ref - f32(ref).astype(np.float64)) - half) <= slack


def held_to(got, b: B.Built, terms=None):
    """(failures, figures) of a float32 result against the case's restatement under the three-term bound; `terms`: (half ulp,
    summation, recurrence, reference) of another selection of the case's voices"""
    half, summation, recurrence, ref = terms or (*B.bound_terms(b), b.ref)
    got = got.astype(np.float64)
    err = np.abs(got - ref)
    err32 = np.abs(got - f32(ref).astype(np.float64))
    bound = half + summation + recurrence
    bound32 = bound + np.where(near_midpoint(ref, half, summation + recurrence), 2 * half, 0.0)
    bar = tolerance(ref)
    failures = []
    if not np.isfinite(got).all() or (got == SENTINEL).any():
        failures.append('not finite, or not written')
    if not (err <= bound).all():
        n = np.unravel_index(np.argmax(err - bound), err.shape)
        failures.append(f'|got - ref| {err[n]:.3g} > {bound[n]:.3g} at {n}')
    if not (err32 <= bound32).all():
        n = np.unravel_index(np.argmax(err32 - bound32), err.shape)
        failures.append(f'|got - f32(ref)| {err32[n]:.3g} > {bound32[n]:.3g} at {n}')
    if not err32.max() <= bar:
        failures.append(f'outer bar: {err32.max():.3g} > {bar:.3g}')
    figures = {'|got - ref|': float(err.max()), '|got - f32(ref)|': float(err32.max()), '|got - ref| - half ulp': float((err - half).max()),
               'half ulp': float(half.max()), 'summation': float(summation.max()), 'recurrence': float(recurrence.max()),
               'least bound / error': float((bound / np.maximum(err, 1e-300)).min())}
    return failures, figures


# ------------------------------------------------------------------------------------------------------- 1. the restatement
def test_every_case_against_the_restatement():
    failed, worst = [], {}
    for c in B.CASES:
        b = B.build(c.name)
        got, status, intact = Stage(b).run('cases')
        failures, figures = held_to(got, b)
        if status != 0:
            failures.append(f'status {status}')
        if not intact:
            failures.append('a sentinel was overwritten')
        print(f'bus pass: {c.name}:', ', '.join(f'{k} {v:.3g}' for k, v in figures.items()), '| FAILED: ' + '; '.join(failures) if failures else '')
        for k, v in figures.items():
            worst[k] = min(worst.get(k, v), v) if k.startswith('least') else max(worst.get(k, v), v)
        failed += [(c.name, f) for f in failures]
    print('bus pass: largest over the cases:', ', '.join(f'{k} {v:.3g}' for k, v in worst.items()))
    assert not failed, (len(failed), failed[:12])
    assert LAUNCHES['cases'] == B.launches()['cases']


# ---------------------------------------------------------------------------------------------------- 2. bit-for-bit invariants
def same(a, b):
    return a.dtype == np.float32 and a.shape == b.shape and bool(np.isfinite(a).all()) and np.array_equal(a, b)


@pytest.mark.parametrize('name', B.BATCHING)
def test_batching(name):
    """K blocks in one call = the K single-block calls at position + b N over the same buffer, under row 0 of the cutoffs"""
    b = B.build(name)
    stage = Stage(b, cutoff=b.cutoff[:1])
    whole, status, intact = stage.run('batching')
    assert status == 0 and intact
    N = b.case.N
    for k in range(b.case.K):
        alone, status, intact = stage.run('batching', block=k)
        assert status == 0 and intact and same(alone, whole[k * N:(k + 1) * N]), (name, k, maxerr(alone, whole[k * N:(k + 1) * N]))


@pytest.mark.parametrize('name,live,layout', B.DEAD_VOICES)
def test_dead_voices(name, live, layout):
    """the first `live` voices of the buffers = all voices with the other gains at 0 (a zero may carry either sign: ==)"""
    b = B.build(name)
    gains = b.gains.array.copy()
    some, status, intact = Stage(b, layout=layout).run('dead voices', live=live)
    assert status == 0 and intact
    gains[:, live:] = 0.0
    every, status, intact = Stage(b, layout=layout, gains=gains).run('dead voices')
    assert status == 0 and intact and np.isfinite(some).all() and float(np.abs(some).max()) > B.FULL_SCALE
    assert bool((some == every).all()), (name, live, maxerr(some, every))


def test_dead_voices_across_the_two_kernels():
    """61 of 64 voices from 16-byte rows: one voice per lane against four, so the sums differ in order and the two agree within twice
    the summation term, one float32 unit more where the reference lies that close to a rounding midpoint"""
    name, live, layout = B.DEAD_VOICES_ACROSS
    b = B.build(name)
    gains = b.gains.array.copy()
    gains[:, live:] = 0.0
    some = Stage(b, layout=layout).run('dead voices', live=live)[0].astype(np.float64)
    every = Stage(b, layout=layout, gains=gains).run('dead voices')[0].astype(np.float64)
    ref = R_sum(b.y64 * b.level, gains)
    half, slack = B.half_ulp32(ref), B.summation_term(b.y64, b.level, gains) + B.recurrence_term(b.y64, b.y80, gains)
    bound = 2 * B.summation_term(b.y64, b.level, gains) + np.where(near_midpoint(ref, half, slack), 2 * half, 0.0)
    assert (np.abs(some - every) <= bound).all(), float(np.abs(some - every).max())
    assert (np.abs(some - ref) <= half + slack).all()


def R_sum(per_voice, gains):
    from oracle import chain_ref as R
    return R.sum_bus(per_voice, gains)


@pytest.mark.parametrize('name', B.BUS_WIDTH)
def test_bus_width(name):
    """C = 4 under [g0, g1, g0, g1] = C = 2 under [g0, g1] = two C = 1 calls: the tile reduction adds the same 64 values in the same
    order whatever C is"""
    b = B.build(name)
    g = b.gains.array[:2]
    four = Stage(b, gains=np.concatenate([g, g])).run('bus width')
    two = Stage(b, gains=g).run('bus width')
    ones = [Stage(b, gains=g[k:k + 1]).run('bus width') for k in (0, 1)]
    assert all(status == 0 and intact for _, status, intact in [four, two] + ones)
    assert four[0].shape[1] == 4 and float(np.abs(two[0]).max()) > B.FULL_SCALE
    for k in (0, 1):
        assert same(four[0][:, k], two[0][:, k]) and same(four[0][:, k + 2], two[0][:, k]) and same(ones[k][0][:, 0], two[0][:, k]), (name, k)


@pytest.mark.parametrize('name', B.CUTOFF_ROWS)
def test_identical_cutoff_rows(name):
    b = B.build(name)
    assert b.cutoff.shape[0] == 1
    one, status, intact = Stage(b).run('cutoff rows')
    assert status == 0 and intact
    rows, status, intact = Stage(b, cutoff=np.repeat(b.cutoff, b.case.K, axis=0)).run('cutoff rows')
    assert status == 0 and intact and same(rows, one), (name, maxerr(rows, one))


# ------------------------------------------------------------------------------------------------------- 3. voices per lane
@pytest.mark.parametrize('name', B.LANES)
def test_four_voices_per_lane_against_one(name):
    """the same data from 16-byte rows and from a buffer viewed from column 1: the lanes' sums are taken in another order, so the
    float64 sums differ by at most twice the summation term; the float32 results by that, or by one unit where the reference lies
    within the bound of a rounding midpoint"""
    b = B.build(name)
    assert B.expected_variant(b.case).vpt == 4 and B.expected_variant(b.case._replace(layout='pad1')).vpt == 1
    four, status, intact = Stage(b).run('lanes')
    assert status == 0 and intact
    one, status, intact = Stage(b, layout='pad1').run('lanes')
    assert status == 0 and intact
    half, summation, recurrence = B.bound_terms(b)
    bound = 2 * summation + np.where(near_midpoint(b.ref, half, summation + recurrence), 2 * half, 0.0)
    diff = np.abs(four.astype(np.float64) - one.astype(np.float64))
    print(f'bus pass: {name}: four against one voice per lane: {int((diff > 0).sum())} of {diff.size} samples differ, max {diff.max():.3g}')
    assert (diff <= bound).all(), (name, float(diff.max()))
    assert not held_to(one, b)[0], held_to(one, b)[0]


# ------------------------------------------------------------------------------------------------------------- 4. the status word
@pytest.mark.parametrize('value', B.STATUS_VALUES)
def test_bad_cutoff(value):
    """a cutoff of 0, rate / 2 or NaN in the last voice of block 1's row: SIG_STATUS_BAD_CUTOFF beside a bit that was set before, the
    bit alone in a fresh word (once per launch, whatever the number of lanes that report), block 1 NaN in every channel and block 0
    untouched by it; the render without that voice finite, with a clean status word"""
    b = B.build(B.STATUS_CASE)
    c = b.case
    assert c.K == 2 and b.cutoff.shape == (2, c.V) and B.channels_of(c) == 2
    good, status, intact = Stage(b).run('status')
    assert status == 0 and intact
    cutoff = b.cutoff.copy()
    cutoff[1, c.V - 1] = value
    stage = Stage(b, cutoff=cutoff)
    got, status, intact = stage.run('status', status=4)
    assert status == (4 | B.BAD_CUTOFF) and intact
    assert np.isnan(got[c.N:]).all() and same(got[:c.N], good[:c.N])
    got, status, intact = stage.run('status', status=0)
    assert status == B.BAD_CUTOFF and intact and np.isnan(got[c.N:]).all()
    # the control: one channel, without that voice
    live = c.V - 1
    mono = Stage(b, cutoff=cutoff, gains=b.gains.array[:1])
    got, status, intact = mono.run('status', live=live)
    assert status == 0 and intact and np.isfinite(got).all()
    w = b.gains.array[:1, :live]
    ref = R_sum(b.y64[:, :live], w)
    terms = (B.half_ulp32(ref), B.summation_term(b.y64[:, :live], 1.0, w), B.recurrence_term(b.y64[:, :live], b.y80[:, :live], w), ref)
    assert not held_to(got, b, terms)[0], held_to(got, b, terms)[0]


def test_bad_values_in_the_padding_of_the_gains_are_not_read():
    """what lies in the columns between `voices` and the gains' leading dimension -- NaN, 0, a number -- changes neither a bit of the
    result nor the status word"""
    b = B.build(B.STATUS_CASE)
    assert b.case.gains_extra == 3
    results = []
    for fill in (float('nan'), 0.0, 7.0):
        stage = Stage(b)
        stage.g_wide[1:1 + stage.g.shape[0], stage.g.shape[1]:] = fill
        out_wide, out = stage.out(b.case.N * b.case.K)
        word = torch.zeros(1, dtype=torch.int32, device=DEV)
        _native.biquad_coldstart_bus(b.case.btype, RATE, b.case.position, b.case.N, b.case.K, b.case.context, stage.cutoff, stage.x, stage.hist,
                                     stage.g, out, status=word)
        torch.cuda.synchronize()
        LAUNCHES['status'] = LAUNCHES.get('status', 0) + 1
        assert int(word.item()) == 0 and around(out_wide, out, SENTINEL)
        results.append(out.cpu().numpy().copy())
    assert same(results[1], results[0]) and same(results[2], results[0]) and not held_to(results[0], b)[0]


# --------------------------------------------------------------------------------------------------------- 5. the C entry's refusals
def entry_args(stage: Stage, out: torch.Tensor, status: torch.Tensor, workspace: torch.Tensor, **changes):
    c = stage.case
    a = dict(type=_native.FILT_TYPES[c.btype], rate=RATE, position=c.position, N=c.N, K=c.K, context=c.context, V=c.V,
             cutoff=stage.cutoff.data_ptr(), cutoff_stride=0 if stage.cutoff.shape[1] == 1 else 1, cutoff_blocks=stage.cutoff.shape[0],
             adsr_params=None, adsr_strides=None, x=stage.x.data_ptr() + stage.hist * stage.x.stride(0) * 4, in_ld=stage.x.stride(0),
             in_history=stage.hist, gains=stage.g.data_ptr(), gains_ld=stage.g.stride(0), C=stage.C, workspace=workspace.data_ptr(),
             out=out.data_ptr(), out_ld=out.stride(0), status=status.data_ptr(), stream=_native.current_stream_handle(0))
    a.update(changes)
    return tuple(a.values())


REFUSED = {'C = 3': dict(C=3), 'C = 2 without gains': dict(gains=None, gains_ld=0), 'type bp': dict(type=_native.FILT_TYPES['bp']),
           'in_history one short': dict(in_history=5), 'out_ld < C': dict(out_ld=1), 'cutoff blocks neither 1 nor K': dict(cutoff_blocks=3)}


def test_refusals_and_empty_launches():
    """argument checks of sig_biquad_coldstart_bus, in front of any launch: hipErrorInvalidValue and `out` untouched; a launch with
    nothing to render (N, K or V = 0) returns 0 and writes nothing"""
    assert tuple(REFUSED) == B.REFUSALS
    b = B.build(B.STATUS_CASE)
    c = b.case
    stage = Stage(b)
    assert stage.hist == 6 and stage.C == 2 and c.K == 2 and stage.cutoff.shape[0] == 2
    wide, out = stage.out(c.N * c.K)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    workspace = _native._bus_workspace(None, c.V, c.N * c.K, 4, DEV)
    entry = _native.lib().sig_biquad_coldstart_bus
    for what, changes in REFUSED.items():
        assert entry(*entry_args(stage, out, status, workspace, **changes)) == INVALID_VALUE, what
    for what in B.EMPTY:                                                        # (no block: the cutoff rows can only be the one row for all)
        assert entry(*entry_args(stage, out, status, workspace, **{what: 0, 'cutoff_blocks': 1 if what == 'K' else 2})) == 0, what
    torch.cuda.synchronize()
    assert bool((wide == SENTINEL).all()) and int(status.item()) == 0
    assert entry(*entry_args(stage, out, status, workspace)) == 0                  # the same arguments unchanged: a launch
    torch.cuda.synchronize()
    LAUNCHES['refusals'] = 1
    assert not held_to(out.cpu().numpy(), b)[0]


def test_launch_census():
    """what ran above is what tests/test_bus_pass_host.py counted against the cap (when the whole file ran)"""
    want = B.launches()
    if set(LAUNCHES) == set(want):
        assert LAUNCHES == want, (LAUNCHES, want)
    assert sum(LAUNCHES.values()) <= B.LAUNCH_CAP


# ------------------------------------------------------------------------------------------------------- 6. the engine's default route
GV = 66
START = 37


def graph_rows():
    rng = np.random.default_rng(29)
    th = rng.uniform(0.3, np.pi / 2 - 0.3, (4, GV))
    return dict(hertz=rng.uniform(55, 1760, (1, GV)), phase=rng.uniform(0, 1, (1, GV)), cut=rng.uniform(200, 8000, (1, GV)),
                cut2=rng.uniform(2000, 8000, (1, GV)), time=rng.uniform(0, 0.002, (1, GV)), k=rng.uniform(0, 3, (1, GV)),
                mix=rng.uniform(0.2, 0.8, (1, GV)), pan=np.where(np.arange(4)[:, None] % 2 == 0, np.cos(th), np.sin(th)))


def graph(which, p, N):
    """(GPU bus node, oracle per-voice node, gains | None, launch label)"""
    import delay_reference as DR
    import ladder_reference as LR
    from oracle import chain_ref as R
    from signals_amd.chain import ext, fx
    saw = lambda: mkosc('Sawtooth', p['hertz'], p['phase'])
    rsaw = lambda: R.Osc('Sawtooth', R.Fixed(p['hertz']), R.Fixed(p['phase']))
    bus = ext.SumBus()
    if which == 'delay':
        d = ext.Delay(); d.input = saw(); d.time = fix(p['time'])
        f = fx.LowPass(); f.input = d; f.cutoff = fix(p['cut'])
        bus.input, gains = f, p['pan'][:2]
        ref, label = R.Filter('lp', DR.oracle_node()(rsaw(), R.Fixed(p['time'])), R.Fixed(p['cut'])), 'biquad_bus[lp]'
    elif which == 'ladder':
        lad = ext.Ladder(); lad.get_state().poles = 4; lad.input = saw(); lad.cutoff = fix(p['cut2']); lad.resonance = fix(p['k'])
        f = fx.HighPass(); f.input = lad; f.cutoff = fix(p['cut'])
        env = E.aligned_draws(GV, START - 16, 4 * N, seed=N)
        a = ext.ADSR()
        for k in E.PARAMS:
            setattr(a, k, fix(env[k]))
        rm = fx.RingMod(); rm.left = f; rm.right = a
        bus.input, gains = rm, None
        ref = R.Binary('RingMod', R.Filter('hp', LR.oracle_node()(rsaw(), R.Fixed(p['cut2']), R.Fixed(p['k'])), R.Fixed(p['cut'])), R.Adsr(**env))
        label = 'biquad_bus[hp,env]'
        assert E.boundary_rows(env, START, 4 * N).any(axis=0).sum() >= GV // 2
    else:
        m = fx.Mix(); m.left = saw(); m.right = mkosc('Triangle', p['hertz'], p['phase']); m.mix = fix(p['mix'])
        f = fx.LowPass(); f.input = m; f.cutoff = fix(p['cut'])
        bus.input, gains = f, p['pan']
        ref = R.Filter('lp', R.Binary('Mix', rsaw(), R.Osc('Triangle', R.Fixed(p['hertz']), R.Fixed(p['phase'])), R.Fixed(p['mix'])), R.Fixed(p['cut']))
        label = 'biquad_bus[lp]'
    if gains is not None:
        bus.get_state().gains = np.ascontiguousarray(gains)
    return bus, ref, gains, label


# N = 64 and 130 for the bus over LowPass(Mix).  A filter over a Delay or a Ladder is a filter over an input that is not
# position-pure: with blocks of at most 100 frames the batch refuses it (NotBatchable: the reference serves the next block from its
# after-window cache there), so those two graphs never reach the kernel at N = 64; they run at N = 101 -- the nearest size the batch
# takes, with ragged row groups at every C -- and 130
ROUTES = [('delay', 101), ('delay', 130), ('ladder', 101), ('ladder', 130), ('mix', 64), ('mix', 130)]


@pytest.mark.parametrize('which,N', ROUTES)
def test_the_default_engine_route(which, N):
    """SumBus(LowPass(ext.Delay(Sawtooth))) stereo, SumBus(RingMod(HighPass(ext.Ladder(Sawtooth)), ADSR)) mono and
    SumBus(LowPass(Mix(Sawtooth, Triangle))) on four channels, 66 voices, two continuing batches of two blocks from position 37 through
    a default BatchRenderer: the bus is the biquad_bus launch, no sum_bus launch, within 1e-6 max(1, max|oracle|)"""
    from oracle import chain_ref as R
    from signals_amd.engine import BatchRenderer, KernelTimer
    p = graph_rows()
    bus, ref_node, gains, label = graph(which, p, N)
    want = R.sum_bus(R.render_stream(ref_node, START, N, 4, GV), gains)
    timer = KernelTimer()
    r = BatchRenderer(bus, 1 if gains is None else gains.shape[0], RATE, timer=timer)
    got = np.concatenate([r.render(START, N, 2).cpu().numpy(), r.render(START + 2 * N, N, 2).cpu().numpy()])
    torch.cuda.synchronize()
    launched = set(timer.summary())
    assert label in launched and not any(n.startswith('sum_bus') for n in launched), launched
    err, scale = maxerr(got, f32(want)), max(1.0, float(np.abs(want).max()))
    print(f'bus pass: engine {which} N = {N}: {sorted(launched)}, max|err| {err:.3g}, max|oracle| {scale:.3g}')
    assert float(np.abs(want).max()) > B.FULL_SCALE and err <= 1e-6 * scale, (which, N, err, scale)
