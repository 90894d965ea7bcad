"""The base per-node kernels -- elementwise.hip, sum_bus.hip, mix_matrix.hip, adsr.hip and the plain osc_bank_kernel -- called
directly through their `_native` wrappers and held against the float64 restatements of oracle/chain_ref.py, at their tile edges
and under padded, column-offset and mixed layouts (tests/base_kernel_cases.py lists the cases and says which kernel variant each
is meant to reach).  Every buffer is a torch view into one allocation whose other elements hold a sentinel: NaN around the inputs,
so that a read outside a view poisons the result, and SENTINEL around (and under) the outputs, which must come back unchanged
around the view and overwritten everywhere inside it.

What is asserted, per kernel:
  elementwise  Gain, RingMod, Mix: the kernel evaluates the reference's expression in float64 (the library is built with
               -ffp-contract=off), so a float32 out equals float32(reference) and a float64 out equals the reference, bit for bit.
               Amp: NaNs where numpy has them; float32 out within the 4e-7 of test_effects_golden; float64 out within
               AMP_F64_BOUND relative, 4 x the largest error measured over these cases (below).
  sum_bus      exact leg (integers times multiples of 1/8: exact in any order): equal.  random leg: float64 out within
               V 2^-53 (|x| @ |g|^T), float32 out within that plus half a float32 unit in the last place of the reference.
  mix_matrix   exact leg: equal.  random leg: within 1e-6 max(1, max|reference|), the bound of the existing test.
  adsr         equal to float32(reference), float64 out to the reference; adsr_apply: equal to float32(reference * float64(x)).
  osc_bank     Square, Sawtooth, Triangle equal in both types; Sine float32 within 1.5e-7, float64 below 1e-15 (test_gpu_eager.py).

Measured on an MI355X over these cases: Amp float64 out, largest relative error against numpy 2.22e-16 (one unit
in the last place; AMP_F64_MEASURED), so 8.88e-16 is asserted."""
import numpy as np
import pytest
import torch

import base_kernel_cases as K
from gpu_helpers import gpu_ready
from signals_amd import _native

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENTINEL = -777.0
SINE_TOL = 1.5e-7                   # tests/test_gpu_eager.py
AMP_F32_TOL = 4e-7                  # tests/test_gpu_eager.py test_effects_golden
AMP_F64_MEASURED = 2.22e-16        # largest relative error of a float64 Amp out against numpy over EW_CASES
AMP_F64_BOUND = 4 * AMP_F64_MEASURED      # 8.88e-16: other inputs of the same ranges


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    gpu_ready()


def materialise(v: K.View, fill: float, copy: bool = True):
    """(buffer, view): `v` inside a buffer of its layout with one further row, everything else (without `copy`: everything) `fill`"""
    rows, V = v.array.shape
    wide = torch.full((rows + 1, v.pad + V + v.ld_extra), fill, dtype=torch.from_numpy(v.array[:0]).dtype, device=DEV)
    sub = wide[:rows, v.pad:v.pad + V]
    assert sub.data_ptr() % 256 == (v.pad * v.array.itemsize) % 256 and (rows == 1 or sub.stride(0) == K.ld(v))
    if copy:
        sub.copy_(torch.from_numpy(v.array))
    return wide, sub


def inputs(built: K.Built) -> dict:
    """name -> view tensor | None of the operands, NaN around each"""
    return {name: None if v is None else materialise(v, float('nan'))[1] for name, v in built.operands.items()}


def outcome(wide: torch.Tensor, v: K.View):
    """(what the view holds, whether everything around it still holds SENTINEL)"""
    rows, V = v.array.shape
    host = wide.cpu().numpy()
    got = host[:rows, v.pad:v.pad + V].copy()
    host[:rows, v.pad:v.pad + V] = SENTINEL
    return got, bool((host == SENTINEL).all())


def as_out(ref: np.ndarray, got: np.ndarray) -> np.ndarray:
    """the float64 reference as the type of `got` stores it"""
    return ref.astype(got.dtype)


def same_bits(got: np.ndarray, want: np.ndarray) -> bool:
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


class Tally:
    """failures and the worst figure per bound of one kernel's cases"""

    def __init__(self, kernel):
        self.kernel, self.failed, self.worst, self.launches = kernel, [], {}, 0

    def figure(self, name, value, bound, case):
        if value >= self.worst.get(name, (-1.0,))[0]:
            self.worst[name] = (float(value), float(bound), case)

    def check(self, ok, case, what):
        if not ok:
            self.failed.append((case, what))

    def done(self):
        print(f'base kernels: {self.kernel}: {self.launches} launches, {len(self.failed)} failed')
        for name, (value, bound, case) in sorted(self.worst.items()):
            print(f'base kernels: {self.kernel}: worst {name} = {value:.4g} (bound {bound:.4g}) at {case}')
        assert not self.failed, (self.kernel, len(self.failed), self.failed[:12])


def test_elementwise():
    tally = Tally('elementwise')
    for case in K.EW_CASES:
        built = K.ew_build(case)
        ins = inputs(built)
        wide, out = materialise(built.out, SENTINEL, copy=False)
        _native.elementwise(case[0], ins['a'], ins['b'], ins['c'], out)
        tally.launches += 1
        got, untouched = outcome(wide, built.out)
        tally.check(untouched, case, 'wrote outside the view')
        if case[0] != 'Amp':
            tally.check(same_bits(got, as_out(built.ref, got)), case, 'differs from the reference')
            continue
        nans = np.isnan(built.ref)
        tally.check(np.array_equal(np.isnan(got), nans), case, 'NaN pattern')
        if nans.all() or not np.array_equal(np.isnan(got), nans):
            continue
        if got.dtype == np.float32:
            err = float(np.abs(got.astype(np.float64) - as_out(built.ref, got).astype(np.float64))[~nans].max())
            tally.figure('Amp float32 |err|', err, AMP_F32_TOL, case)
            tally.check(err < AMP_F32_TOL, case, f'Amp float32 error {err}')
        else:
            rel = float((np.abs(got - built.ref)[~nans] / np.abs(built.ref[~nans])).max())
            tally.figure('Amp float64 relative error', rel, AMP_F64_BOUND, case)
            tally.check(rel <= AMP_F64_BOUND, case, f'Amp float64 relative error {rel}')
    tally.done()


def test_sum_bus():
    tally = Tally('sum_bus')
    for case in K.BUS_CASES:
        for leg in ('exact', 'random'):
            built = K.bus_build(case, leg)
            ins = inputs(built)
            wide, out = materialise(built.out, SENTINEL, copy=False)
            _native.sum_bus(ins['x'], ins['gains'], out)
            tally.launches += len(K.bus_widths(case[2]))
            got, untouched = outcome(wide, built.out)
            tally.check(untouched, case, f'{leg}: wrote outside the view')
            if leg == 'exact':
                tally.check(same_bits(got, as_out(built.ref, got)), case, 'exact leg differs from the reference')
                continue
            err, bound = np.abs(got.astype(np.float64) - built.ref), K.bus_bound(built)
            tally.check(bool(np.isfinite(got).all()) and bool((err <= bound).all()), case, f'random leg: error {err.max()}')
            if np.isfinite(err).all():
                at = np.unravel_index(np.argmax(err / bound), err.shape)
                tally.figure(f'{got.dtype} out, error / bound', err[at] / bound[at], 1.0, case)
    tally.done()


def test_mix_matrix():
    tally = Tally('mix_matrix')
    for case in K.MIX_CASES:
        for leg in ('exact', 'random'):
            built = K.mix_build(case, leg)
            ins = inputs(built)
            wide, out = materialise(built.out, SENTINEL, copy=False)
            _native.mix_matrix(ins['x'], ins['m'], out)
            tally.launches += 1
            got, untouched = outcome(wide, built.out)
            tally.check(untouched, case, f'{leg}: wrote outside the view')
            if leg == 'exact':
                tally.check(same_bits(got, as_out(built.ref, got)), case, 'exact leg differs from the reference')
                continue
            bound = 1e-6 * max(1.0, float(np.abs(built.ref).max()))
            err = float(np.abs(got.astype(np.float64) - built.ref).max())
            tally.figure('random leg |err|', err, bound, case)
            tally.check(err < bound, case, f'random leg: error {err}')
    # a view one float off a 16-byte boundary is refused by the entry's alignment check, and nothing is written
    built = K.mix_build(K.MIX_REFUSED, 'exact')
    ins = inputs(built)
    wide, out = materialise(built.out, SENTINEL, copy=False)
    assert ins['x'].data_ptr() % 16 == 4 and ins['x'].stride(0) % 4 == 0
    with pytest.raises(_native.NativeError):
        _native.mix_matrix(ins['x'], ins['m'], out)
    torch.cuda.synchronize()
    assert bool((wide == SENTINEL).all())
    tally.done()


def test_adsr():
    tally = Tally('adsr')
    for case in K.ADSR_CASES:
        built = K.adsr_build(case)
        ins = inputs(built)
        rows = {name: ins[name] for name in K.ADSR_PARAMS}
        wide, out = materialise(built.out, SENTINEL, copy=False)
        if case[0] == 'apply':
            _native.adsr_apply(case[3], K.RATE, rows, ins['x'], out)
        else:
            _native.adsr(case[3], K.RATE, rows, out)
        tally.launches += 1
        got, untouched = outcome(wide, built.out)
        tally.check(untouched, case, 'wrote outside the view')
        tally.check(same_bits(got, as_out(built.ref, got)), case, 'differs from the reference')
    tally.done()


def test_osc_bank():
    tally = Tally('osc_bank')
    for case in K.OSC_CASES:
        built = K.osc_build(case)
        ins = inputs(built)
        wide, out = materialise(built.out, SENTINEL, copy=False)
        _native.osc_bank(case[0], case[3], K.RATE, ins['hertz'], ins['phase'], out)
        tally.launches += 1
        got, untouched = outcome(wide, built.out)
        tally.check(untouched, case, 'wrote outside the view')
        if case[0] != 'Sine':
            tally.check(same_bits(got, as_out(built.ref, got)), case, 'differs from the reference')
            continue
        err = float(np.abs(got.astype(np.float64) - as_out(built.ref, got).astype(np.float64)).max())
        if got.dtype == np.float32:
            tally.figure('Sine float32 |err|', err, SINE_TOL, case)
            tally.check(err <= SINE_TOL, case, f'Sine float32 error {err}')
        else:
            tally.figure('Sine float64 |err|', err, 1e-15, case)
            tally.check(err < 1e-15, case, f'Sine float64 error {err}')
    tally.done()


@pytest.mark.parametrize('x_dtype,channels,with_gains', [(torch.float32, 1, False), (torch.float32, 1, True), (torch.float32, 2, True),
                                                         (torch.float32, 4, True), (torch.float64, 1, True)])
@pytest.mark.parametrize('out_dtype', [torch.float32, torch.float64])
def test_sum_bus_without_voices_writes_zeros(x_dtype, channels, with_gains, out_dtype):
    """rows = 5, voices = 0 straight through the C entry, with pointers to real tensors: the sum over no voices is 0.0 on every
    path (the float32 fast path used to take the launch and start no kernel), and rows = 0 touches nothing"""
    lib = _native.lib()
    code = {torch.float32: _native.F32, torch.float64: _native.F64}
    x = torch.full((6, 4), float('nan'), dtype=x_dtype, device=DEV)
    gains = torch.full((channels, 4), float('nan'), dtype=torch.float64, device=DEV)
    out = torch.full((6, channels + 1), SENTINEL, dtype=out_dtype, device=DEV)
    args = lambda rows: (rows, 0, x.data_ptr(), 4, code[x_dtype], gains.data_ptr() if with_gains else None, 4 if with_gains else 0,
                         channels, out.data_ptr(), channels + 1, code[out_dtype], None)
    assert lib.sig_sum_bus(*args(0)) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert lib.sig_sum_bus(*args(5)) == 0
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert np.array_equal(host[:5, :channels], np.zeros((5, channels), dtype=host.dtype)), host
    assert bool((host[5] == SENTINEL).all()) and bool((host[:, channels] == SENTINEL).all())
