"""The control-program kernels (signals_amd/csrc/control_program.hip) called directly through `_native.control_program` and
`_native.control_program_attached`, over the hand-written programs of tests/control_program_cases.py: at the chunk edges of the
interpreter (128 columns) and of the specialised build (256), every window length h = 0 .. 100 on the one-column and the wide
filter path, per-block ROWs in both stride forms, programs of 1, 2 and 48 instructions, and the launch arguments the engine never
produces.  Every program passes `validate` before it is uploaded.

What is asserted:
  variants     the variant a program's ops require and the wider ones (a plain program also through _windowed and _envelope) give
               the same bits, NaN positions included.
  specialised  the ten structures of K.SPECIALISED, built by specialise.ensure_control, give the interpreter's bits.
  reference    outputs made only of ROW, Square / Sawtooth / Triangle, Gain / Mix / RingMod, Noise and ADSR equal the float64
               restatement exactly; a float64 Sine without a Filter or an Amp behind it is within one unit in the last place at full
               scale (2^-52) per Sine, scaled by the case's own rows; everything with a Filter, an Amp or a window-rate Sine is within
               1e-6 max(1, max|reference|), NaNs where the reference has them.
  guards       the 64 cells behind every output and front row keep their pattern; a NULL front is skipped; with n_outs = 0 or a
               refused argument nothing is written at all.
  status       a cutoff above Nyquist in column 200 of 300 sets SIG_STATUS_BAD_CUTOFF (and NaN in that column alone); valid
               cutoffs leave the word 0.
  per node     one program per op family against the per-node kernels the header names as the same bits: the osc bank's float64
               store, elementwise, adsr (rows = 1, float64), white_noise, biquad_coldstart over the window rows.

Measured on an MI355X, the largest error as a fraction of its bound, per group of the table (test_report prints them under -s):
  sine (of the 2^-52-per-Sine bound):  size 0, operands 0 -- the float64 Sine met the oracle's bits in every case of the table.
  bar (of 1e-6 max(1, max|reference|)):  columns 6.9e-9, window length 3.1e-10, window contents 0.045, launch 2.0e-9, operands 1.2e-10,
      status 3.4e-9, size 0 (the 48-word chains, Amp and Filter included, came out equal).  Window contents is the one group with a
      window-rate Sine: its history rows are the float32 v_sin path (within 1.3e-7 of the float64 one, include/signals_amd.h) where the
      restatement rounds the float64 sine, and a low-pass passes a part of that difference on.  No group uses half of the bar.
No case of the table exposed a defect in the kernels or the marshalling."""
import numpy as np
import pytest
import torch

import control_program_cases as K
from gpu_helpers import gpu_ready
from signals_amd import _native

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
BAR = 1e-6                          # tests/test_gpu_filtered_control.py: close
MEASURED = {}                       # (kind, group) -> largest error / bound, filled by the run and printed by test_report


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    gpu_ready(DEV)


class Outcome:
    """what one launch left: per output the (nblocks, cols) rows and the front row (None: no front position, or a NULL front),
    the status words, and whether every guard cell kept its pattern"""

    def __init__(self, case, up, n_outs):
        torch.cuda.synchronize()
        L = case.launch
        self.rows, self.fronts, self.guards, self.raw = [], [], True, []
        for (reg, cols, has_front), buf, front in zip(case.outs, up.buffers, up.fronts):
            host = buf.cpu().numpy()
            self.raw.append(host)
            self.guards &= bool((host[L.nblocks * cols:].view(np.uint64) == K.guard_bits()).all())
            self.rows.append(host[:L.nblocks * cols].reshape(L.nblocks, cols).copy())
            if front is None:
                self.fronts.append(None)
                continue
            fhost = front.cpu().numpy()
            self.raw.append(fhost)
            self.guards &= bool((fhost[cols:].view(np.uint64) == K.guard_bits()).all())
            written = L.front_position >= 0 and n_outs > 0
            if not written:
                self.guards &= bool((fhost.view(np.uint64) == K.guard_bits()).all())
            self.fronts.append(fhost[:cols].reshape(1, cols).copy() if written else None)
        self.status = {k: int(t[0].item()) for k, t in up.status.items()}
        self.status_guard = all(int(t[1].item()) == 0 for t in up.status.values())

    def untouched(self) -> bool:
        return all(bool((h.view(np.uint64) == K.guard_bits()).all()) for h in self.raw)


_handles, _outcomes = {}, {}


def handle_of(case, up):
    """the handle of the specialised build for the case's structure (built once per structure)"""
    from signals_amd import specialise
    if case.structure not in _handles:
        _handles[case.structure] = specialise.ensure_control(_native.control_program_description(up.ins_list, up.outs_list))
        assert _handles[case.structure], f'specialised build of {case.structure} failed'
    return _handles[case.structure]


def run(case, route, n_outs=None, **override) -> Outcome:
    """launch `case` through `route` ('plain' | 'windowed' | 'envelope' | 'specialised'); `override`: launch arguments replaced
    (the refusals), which returns the error code instead"""
    key = (case.name, route)
    if n_outs is None and not override and key in _outcomes:
        return _outcomes[key]
    up = K.to_ctl(case, DEV)                                       # (validates first)
    L = case.launch._replace(**{k: v for k, v in override.items() if k != 'n_ins'})
    n_ins = override.get('n_ins', len(case.ins))
    count = len(case.outs) if n_outs is None else n_outs
    args = (L.rate, L.position, L.step, L.nblocks, L.cols, up.program, n_ins, up.outs, count)
    try:
        if route == 'specialised':
            _native.control_program_attached(handle_of(case, up), *args, front_position=L.front_position, min_position=L.min_position)
        else:
            _native.control_program(*args, front_position=L.front_position, min_position=L.min_position,
                                    windowed=route == 'windowed', envelope=route == 'envelope')
    except _native.NativeError as e:
        if not override:
            raise
        return Outcome(case, up, 0), str(e)
    out = Outcome(case, up, count)
    if override:
        return out, None
    if n_outs is None:
        _outcomes[key] = out
    return out


def same_bits(a, b) -> bool:
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def agree(x: Outcome, y: Outcome) -> bool:
    return all(same_bits(a, b) for a, b in zip(x.rows, y.rows)) and all(same_bits(a, b) for a, b in zip(x.fronts, y.fronts)) \
        and x.status == y.status


# ---------------------------------------------------------------------------------------------------------------- the variants
@pytest.mark.parametrize('case', K.CASES, ids=lambda c: c.name)
def test_variants_agree_bit_for_bit(case):
    routes = K.variants_of(case)
    first = run(case, routes[0])
    assert first.guards and first.status_guard, case.name
    for route in routes[1:]:
        other = run(case, route)
        assert other.guards and other.status_guard, (case.name, route)
        assert agree(first, other), (case.name, route)


@pytest.mark.parametrize('structure', K.SPECIALISED)
def test_specialised_build_agrees_bit_for_bit(structure):
    from signals_amd import specialise
    if specialise.hipcc() is None:
        pytest.skip('no hipcc: the specialised kernels cannot be built')
    cases = [c for c in K.CASES if c.structure == structure]
    assert cases
    for case in cases:
        got = run(case, 'specialised')
        assert got.guards and got.status_guard, case.name
        assert agree(run(case, K.variant_of(case)), got), case.name


# -------------------------------------------------------------------------------------------------------------- the reference
def note(kind, group, ratio):
    MEASURED[(kind, group)] = max(MEASURED.get((kind, group), 0.0), float(ratio))


def held(case, got, want, bound, kind, what):
    """one output array against its reference under the rule of its kind"""
    assert got.shape == want.shape, what
    if got.size == 0:
        return
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    if kind == 'exact':
        assert same_bits(got, want), what
        return
    live = ~np.isnan(want)
    err = np.abs(got - want)[live]
    if kind == 'sine':
        ratio = float(np.max(err / bound[live])) if err.size else 0.0
    else:
        ratio = float(err.max() / (BAR * max(1.0, float(np.abs(want[live]).max())))) if err.size else 0.0
    note(kind, case.group, ratio)
    print(f'{case.name} {what[1:]} {kind}: {ratio:.3g} of its bound')
    assert ratio <= 1.0, (what, ratio)


@pytest.mark.parametrize('case', K.CASES, ids=lambda c: c.name)
def test_against_the_float64_restatement(case):
    got = run(case, K.variant_of(case))
    ref = K.reference(case)
    bounds = K.sine_bounds(case) if any(K.holds_to(case, reg) == 'sine' for reg, _, _ in case.outs) else [None] * len(case.outs)
    for k, (reg, cols, has_front) in enumerate(case.outs):
        kind = K.holds_to(case, reg)
        held(case, got.rows[k], ref[k][0], bounds[k][0] if bounds[k] else None, kind, (case.name, reg, 'rows'))
        assert (got.fronts[k] is None) == (ref[k][1] is None), (case.name, reg)
        if ref[k][1] is not None:
            held(case, got.fronts[k], ref[k][1], bounds[k][1] if bounds[k] else None, kind, (case.name, reg, 'front'))


def test_exact_outputs_are_most_of_the_table():
    kinds = [K.holds_to(c, reg) for c in K.CASES for reg, _, _ in c.outs]
    assert kinds.count('exact') >= 60 and kinds.count('sine') >= 8 and kinds.count('bar') >= 60


# ------------------------------------------------------------------------------------------------- status, refusals, no outputs
@pytest.mark.parametrize('route', ['windowed', 'envelope', 'specialised'])
def test_bad_cutoff_sets_the_status_word(route):
    from signals_amd import specialise
    if route == 'specialised' and specialise.hipcc() is None:
        pytest.skip('no hipcc: the specialised kernels cannot be built')
    bad, good = run(K.BY_NAME['status_bad'], route), run(K.BY_NAME['status_good'], route)
    assert list(bad.status.values()) == [_native.STATUS_BAD_CUTOFF] and list(good.status.values()) == [0]
    assert bad.status_guard and good.status_guard
    for rows in bad.rows + bad.fronts:
        assert np.isnan(rows[:, 200]).all() and np.isfinite(np.delete(rows, 200, axis=1)).all()
    assert all(np.isfinite(rows).all() for rows in good.rows + good.fronts)


@pytest.mark.parametrize('route', ['plain', 'windowed', 'envelope', 'specialised'])
def test_refusals_and_no_outputs_touch_nothing(route):
    from signals_amd import specialise
    if route == 'specialised' and specialise.hipcc() is None:
        pytest.skip('no hipcc: the specialised kernels cannot be built')
    for what, name, override in K.REFUSALS:
        out, error = run(K.BY_NAME[name], route, **override)
        assert error is not None and error.endswith(f'hipError_t {K.INVALID_VALUE}'), (what, error)
        assert out.untouched(), what
    out = run(K.BY_NAME[K.NO_OUTPUTS], route, n_outs=0)
    assert out.untouched()


# -------------------------------------------------------------------------------------------------------- the per-node kernels
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)


def row_of(case, reg):
    return dev(case.ins[reg].data)


def test_osc_registers_equal_the_osc_bank():
    """Sine (float64 store) and Sawtooth at one row per block"""
    case = K.BY_NAME['leading_3']
    L, got = case.launch, run(case, 'plain')
    sine = case.ins[case.outs[1][0]]
    out = torch.empty((L.nblocks, 1), dtype=torch.float64, device=DEV)
    _native.osc_bank('Sine', L.position, L.rate, dev(got.rows[0][:1]), None, out, step=L.step)
    assert sine.op == K.OSC and sine.kind == K.SINE and same_bits(out.cpu().numpy(), got.rows[1])
    case = K.BY_NAME['plain_129']
    L, got = case.launch, run(case, 'plain')
    lfo = case.ins[case.outs[0][0]]
    out = torch.empty((L.nblocks, 1), dtype=torch.float64, device=DEV)
    _native.osc_bank('Sawtooth', L.position, L.rate, row_of(case, lfo.a), row_of(case, lfo.b), out, step=L.step)
    assert same_bits(out.cpu().numpy(), got.rows[0])


def test_elementwise_and_noise_registers_equal_their_kernels():
    case = K.BY_NAME['noise_129']
    L, got = case.launch, run(case, 'windowed')
    mix, gain = case.ins[case.outs[0][0]], case.ins[case.ins[case.outs[0][0]].a]
    noise = case.ins[case.outs[1][0]]
    for b, p in enumerate(K.frames_of(case)):
        out = torch.empty((1, L.cols), dtype=torch.float64, device=DEV)
        _native.white_noise(noise.data, p, out)
        assert same_bits(out.cpu().numpy(), got.rows[1][b:b + 1]), b
    g = _native.elementwise('Gain', dev(got.rows[1]), row_of(case, gain.b), None, torch.empty((L.nblocks, L.cols), dtype=torch.float64, device=DEV))
    m = _native.elementwise('Mix', g, row_of(case, mix.b), row_of(case, mix.c), torch.empty_like(g))
    assert same_bits(m.cpu().numpy(), got.rows[0])
    case = K.BY_NAME['operands_300']                                          # Amp: the same pow, NaNs included
    L, got = case.launch, run(case, 'plain')
    amp = case.ins[case.outs[-1][0]]
    a = _native.elementwise('Amp', row_of(case, amp.a), row_of(case, amp.b), None, torch.empty((1, L.cols), dtype=torch.float64, device=DEV))
    assert same_bits(np.repeat(a.cpu().numpy(), L.nblocks, axis=0), got.rows[-1])


def test_adsr_registers_equal_the_adsr_kernel():
    case = K.BY_NAME['adsr_129']
    L, got = case.launch, run(case, 'envelope')
    e = case.ins[case.outs[1][0]]
    g = case.ins[e.dst - 1]
    rows = dict(zip(_native.ADSR_PARAMS, (row_of(case, r) for r in (e.a, e.b, e.c, g.a, g.b, g.c))))
    for b, p in enumerate(K.frames_of(case)):
        out = torch.empty((1, L.cols), dtype=torch.float64, device=DEV)
        _native.adsr(p, L.rate, rows, out)
        assert same_bits(out.cpu().numpy(), got.rows[1][b:b + 1]), b


@pytest.mark.parametrize('name', ['position_narrow_101', 'position_wide_2', 'clamp_filter_37'])
def test_filter_registers_equal_the_coldstart_biquad(name):
    """the window rows (Square / Sawtooth and a product: the restatement's rows are the kernel's, bit for bit) through
    sig_biquad_coldstart: h context rows, one block of one row"""
    case = K.BY_NAME[name]
    L, got = case.launch, run(case, 'windowed')
    f = case.ins[case.outs[1][0]]
    assert f.op == K.FILTER
    for b, p in enumerate(K.frames_of(case)):
        window = K.window_rows(case, f.dst, K.evaluate(case, p, b), p, b)
        h = window.shape[0] - 1
        out = torch.empty((1, f.cols), dtype=torch.float64, device=DEV)
        _native.biquad_coldstart(K.FILT_NAMES[f.kind], L.rate, p, 1, 1, h, row_of(case, f.b), dev(window), h, out)
        assert same_bits(out.cpu().numpy(), got.rows[1][b:b + 1]), (name, b)


def test_report():
    """the figures the docstring quotes (run with -s to see them)"""
    for (kind, group), ratio in sorted(MEASURED.items()):
        print(f'MEASURED {kind:5s} {group:16s} {ratio:.3g}')
    assert all(r <= 1.0 for r in MEASURED.values())
