"""GPU parity, eager pull path: every golden case of tests/golden/ rendered through signals_amd's
node API (one HIP kernel per node per block, through the C ABI) against the reference's outputs.

Tolerances (BASELINE.json north_star: 1e-6 in float32, integer positions bit-exact):
  * Square/Sawtooth/Triangle: BIT-EXACT against float32(reference float64) -- their f64 arithmetic is
    reproduced operation for operation;
  * Sine, float32 store: <= 1.5e-7 (exact f64 phase reduction, then the hardware v_sin_f32);
    float64 (block-rate) store: 1e-15 (f64 polynomial);
  * block-rate (float64) replies: 1e-15;
  * filters/effects on float32 buffers: 1e-6 bar, 3e-7 asserted.
"""
import numpy as np
import pytest
import torch

from gpu_helpers import gpu_ready
from helpers import HOUR, OSC, RATE, f32, fix, loc, maxerr, mkosc, render, stream, Probe

pytestmark = pytest.mark.gpu

ULP1 = 1.2e-7
SINE_TOL = 1.5e-7      # f32 Sine: exact phase reduction + v_sin_f32 (measured max error 1.07e-7)


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    gpu_ready()


@pytest.mark.parametrize('kind', list(OSC))
def test_osc_golden(golden, kind):
    g = golden('osc')
    exact = kind != 'Sine'
    cases = [(f'osc/{kind}/p{int(p)}', int(p), 256, g['osc/hertz'], g['osc/phase']) for p in g['osc/positions']]
    cases += [(f'osc/{kind}/nophase/p256', 256, 256, g['osc/hertz'], None),
              (f'osc/edge/{kind}', 0, 64, g['osc/edge/hertz'], g['osc/edge/phase']),
              (f'osc/neg/{kind}', 1000, 128, g['osc/neg/hertz'], g['osc/neg/phase'])]
    for key, pos, n, hz, ph in cases:
        got = render(mkosc(kind, hz, ph), pos, n, hz.shape[1])
        assert got.dtype == np.float32
        ref = f32(g[key])
        if exact:
            assert np.array_equal(got, ref), (key, maxerr(got, ref))
        else:
            assert maxerr(got, ref) <= SINE_TOL, key


def test_osc_int_hertz_and_block_rate(golden):
    g = golden('osc')
    got = render(mkosc('Sine', np.array([[220]])), 0, 256, 1)
    assert maxerr(got, f32(g['osc/int_hertz/Sine'])) <= SINE_TOL
    ctrl = render(mkosc('Sine', g['osc/hertz'], g['osc/phase']), 512, 1, 16)
    assert ctrl.dtype == np.float64 and ctrl.shape == (1, 16)
    assert maxerr(ctrl, g['osc/ctrl/Sine/p512']) < 1e-15


@pytest.mark.parametrize('kind', list(OSC))
def test_osc_block_rate_f64_bit_exact_nonsine(golden, kind):
    """float64 store path: the discontinuous waveforms are bit-exact in f64"""
    if kind == 'Sine':
        pytest.skip('Sine is within 1 ulp(f64), covered above')
    from oracle import chain_ref as R
    g = golden('osc')
    for pos in (0, 123, HOUR + 7):
        got = render(mkosc(kind, g['osc/hertz'], g['osc/phase']), pos, 1, 16)
        assert np.array_equal(got, R.osc(kind, pos, 1, RATE, g['osc/hertz'], g['osc/phase']))


@pytest.mark.parametrize('fname', ('LowPass', 'HighPass'))
@pytest.mark.parametrize('oname', ('Sine', 'Sawtooth'))
def test_single_filter_golden(golden, fname, oname):
    from signals_amd.chain import fx
    g = golden('filter')
    worst = 0.0
    for pos in g['filt/positions']:
        f = getattr(fx, fname)()
        f.input = mkosc(oname, g['filt/hertz'], g['filt/phase'])
        f.cutoff = fix(g['filt/cutoff'])
        got = render(f, int(pos), 256, 16)
        worst = max(worst, maxerr(got, f32(g[f'filt/{fname}/{oname}/p{int(pos)}'])))
    assert worst < 3e-7, worst


def test_filter_ragged_and_short_context(golden):
    from signals_amd.chain import fx
    g = golden('filter')
    for pos, n in ((7, 33), (99, 101), (100, 64), (101, 1000)):
        f = fx.LowPass()
        f.input = mkosc('Triangle', g['filt/hertz'], g['filt/phase'])
        f.cutoff = fix(g['filt/cutoff'])
        got = render(f, pos, n, 16)
        assert got.shape == (n, 16)
        assert maxerr(got, f32(g[f'filt/ragged/p{pos}_n{n}'])) < 3e-7, (pos, n)


def test_sequential_and_cascade(golden):
    from signals_amd.chain import fx
    g = golden('filter')
    f = fx.LowPass()
    f.input = mkosc('Sine', g['filt/hertz'], g['filt/phase'])
    f.cutoff = fix(g['filt/seq/cutoff'])
    assert maxerr(stream(f, 0, 256, 4, 16), f32(g['filt/seq/LowPass'])) < 3e-7
    c = golden('cascade')
    for N in (256, 1024):
        f1 = fx.LowPass()
        f1.input = mkosc('Sawtooth', c['casc/hertz'], c['casc/phase'])
        f1.cutoff = fix(c['casc/cut1'])
        f2 = fx.LowPass()
        f2.input = f1
        f2.cutoff = fix(c['casc/cut2'])
        assert maxerr(stream(f2, 0, N, 4, 8), f32(c[f'casc/seq_n{N}'])) < 3e-7, N
    f1 = fx.LowPass()
    f1.input = mkosc('Sawtooth', c['casc/hertz'], c['casc/phase'])
    f1.cutoff = fix(c['casc/cut1'])
    f2 = fx.HighPass()
    f2.input = f1
    f2.cutoff = fix(c['casc/cut2'])
    assert maxerr(render(f2, 768, 256, 8), f32(c['casc/fresh_p768'])) < 3e-7


def test_effects_golden(golden):
    from signals_amd.chain import fx, shape
    g = golden('effects')
    V, N, pos = 8, 128, 300
    hz, ph = g['fxs/hertz'], g['fxs/phase']

    def check(node, key, channels=V, tol=2e-7):
        got = render(node, pos, N, channels)
        assert maxerr(got, f32(g[key])) < tol, key

    n = fx.Gain(); n.left = mkosc('Sine', hz, ph); n.right = fix(g['fxs/gain']); check(n, 'fxs/Gain')
    n = fx.Gain(); n.left = mkosc('Sine', hz, ph); n.right = fix([[0.2]]); check(n, 'fxs/Gain_scalar')
    n = fx.Mix(); n.left = mkosc('Sine', hz, ph); n.right = mkosc('Sawtooth', hz * 0.5, ph)
    n.mix = fix(g['fxs/gain']); check(n, 'fxs/Mix')
    n = fx.RingMod(); n.left = mkosc('Sine', hz, ph); n.right = mkosc('Triangle', hz * 0.25, ph)
    check(n, 'fxs/RingMod')
    e = g['fxs/amp_exp']
    n = fx.Amp(); n.left = mkosc('Sawtooth', hz, ph); n.right = fix(np.round(e)); check(n, 'fxs/Amp_int', tol=4e-7)
    n = fx.Amp(); n.left = mkosc('Sawtooth', hz, ph); n.right = fix(e); check(n, 'fxs/Amp_frac', tol=4e-7)
    n = shape.Merge(); n.left = mkosc('Sine', hz, ph); n.right = mkosc('Square', hz * 0.5, ph)
    check(n, 'fxs/Merge', channels=2 * V)


def test_protocol_corners(golden):
    from signals_amd.chain import fx
    g = golden('effects')
    V, N, pos = 8, 128, 300
    o = mkosc('Sine', g['fxs/hertz'], g['fxs/phase'])
    o.get_state().enabled = False
    d = render(o, pos, N, V)
    assert d.shape == (1, 1) and d[0, 0] == 0 and np.array_equal(d, g['fxs/disabled'])
    n = fx.Gain()
    n.right = fix(g['fxs/gain'])
    u = render(n, pos, N, V)
    assert u.shape == g['fxs/unplugged_left'].shape and np.array_equal(u, g['fxs/unplugged_left'])
    b = render(mkosc('Sine', [[440.0]]), 0, N, 2)
    assert b.shape == (N, 1) and maxerr(b, f32(g['fxs/broadcast_1to2'])) <= SINE_TOL


def test_sigs_topologies(golden):
    from signals_amd.chain import fx, shape
    g = golden('sigs')
    assert maxerr(stream(mkosc('Sine', np.array([[220]])), 0, 256, 3, 1), f32(g['sigs/vis_test'])) <= SINE_TOL
    tri = mkosc('Triangle', np.array([[440]]))
    gn = fx.Gain(); gn.left = tri; gn.right = fix(np.array([[0.2]]))
    lp = fx.LowPass(); lp.input = gn; lp.cutoff = fix(np.array([[600]]))
    m = shape.Merge(); m.left = lp; m.right = gn
    assert maxerr(stream(m, 0, 256, 3, 2), f32(g['sigs/lowpass_test'])) < 2e-7


@pytest.mark.parametrize('tag,pos0', (('p0', 0), ('p1h', HOUR)))
def test_c2_reduced(golden, tag, pos0):
    from signals_amd.chain import fx
    g = golden('c2')
    f = fx.LowPass(); f.input = mkosc('Sine', g['c2/hertz'], g['c2/phase']); f.cutoff = fix(g['c2/cutoff'])
    n = fx.Gain(); n.left = f; n.right = fix(g['c2/gain'])
    assert maxerr(stream(n, pos0, 256, 4, 32), f32(g[f'c2/{tag}'])) < 2e-8     # gains are ~1/32


def test_sum_bus_vs_oracle():
    from oracle import chain_ref as R
    from signals_amd.chain.ext import SumBus
    rng = np.random.default_rng(7)
    for V in (3, 64, 1000, 1024):
        hz, ph = rng.uniform(55, 1760, (1, V)), rng.uniform(0, 1, (1, V))
        ref_x = f32(R.osc('Sawtooth', 512, 96, RATE, hz, ph)).astype(np.float64)
        bus = SumBus(); bus.input = mkosc('Sawtooth', hz, ph)
        assert maxerr(render(bus, 512, 96, 1), f32(R.sum_bus(ref_x))) < 1e-5 * max(1, V / 64)
        pan = rng.uniform(0, np.pi / 2, V)
        gains = np.stack([np.cos(pan), np.sin(pan)]) / V
        bus = SumBus(); bus.input = mkosc('Sawtooth', hz, ph); bus.get_state().gains = gains
        got = render(bus, 512, 96, 2)
        assert got.shape == (96, 2)
        assert maxerr(got, f32(R.sum_bus(ref_x, gains))) < 1e-7


def test_bad_cutoff_raises_like_scipy():
    from signals_amd import runtime
    from signals_amd.chain import fx
    f = fx.LowPass(); f.input = mkosc('Sine', [[440.0, 220.0]]); f.cutoff = fix([[1000.0, 24000.0]])
    out = render(f, 0, 64, 2)
    assert np.isfinite(out[:, 0]).all() and np.isnan(out[:, 1]).all()
    with pytest.raises(ValueError):
        runtime.check_status()
    runtime.check_status()      # cleared
    f = fx.LowPass(); f.input = mkosc('Sine', [[440.0, 220.0]]); f.cutoff = fix([[1000.0]])
    with pytest.raises(IndexError):
        render(f, 0, 64, 2)
    bp = fx.BandPass(); bp.input = mkosc('Sine', [[440.0, 440.0]]); bp.low = fix([[1000.0, 100.0]]); bp.high = fix([[100.0, 1000.0]])
    out = render(bp, 0, 64, 2)          # voice 0: low >= high -> scipy's ValueError, surfaced at the sink edge
    assert np.isnan(out[:, 0]).all() and np.isfinite(out[:, 1]).all()
    with pytest.raises(ValueError):
        runtime.check_status()


@pytest.mark.parametrize('cls,btype', (('BandPass', 'bp'), ('BandStop', 'bs')))
def test_band_filters_vs_scipy(cls, btype):
    """the reference's band filters crash; pinned against scipy butter(2,[lo,hi]) + sosfilt"""
    from oracle import chain_ref as R
    from signals_amd.chain import fx
    from helpers import stream
    rng = np.random.default_rng(17)
    V = 16
    hz, ph = rng.uniform(55, 1760, (1, V)), rng.uniform(0, 1, (1, V))
    lo = np.geomspace(40, 6000, V).reshape(1, V)
    hi = lo * rng.uniform(1.2, 4.0, (1, V))

    def build():
        f = getattr(fx, cls)(); f.input = mkosc('Sawtooth', hz, ph); f.low = fix(lo); f.high = fix(hi)
        return f
    for pos, n in ((0, 256), (50, 100), (HOUR, 512)):
        got = render(build(), pos, n, V)
        ref = R.render(R.BandFilter(btype, R.Osc('Sawtooth', R.Fixed(hz), R.Fixed(ph)), R.Fixed(lo), R.Fixed(hi)), pos, n, V)
        assert maxerr(got, f32(ref)) < 5e-7, (cls, pos, n)
    from signals_amd.engine import BatchRenderer
    batch = BatchRenderer(build(), V, RATE).render(0, 256, 4).cpu().numpy()
    assert np.array_equal(batch, stream(build(), 0, 256, 4, V))


def test_extreme_block_sizes_vs_oracle():
    """ragged and maximum sizes: 1-frame-short context, a one-second block (48000 frames), 3 voices (not a multiple
    of the 4-wide vector path), a position near 2^40, and empty launches through the C ABI"""
    import ctypes
    from oracle import chain_ref as R
    from signals_amd import _native
    from signals_amd.chain import fx
    rng = np.random.default_rng(41)
    V = 3
    hz, ph, cut = rng.uniform(55, 1760, (1, V)), rng.uniform(0, 1, (1, V)), rng.uniform(200, 8000, (1, V))
    for pos, n in ((99, 48000), (1, 2), (2 ** 40 - 17, 257)):
        f = fx.LowPass(); f.input = mkosc('Sawtooth', hz, ph); f.cutoff = fix(cut)
        got = render(f, pos, n, V)
        ref = R.filter_block('lp', lambda p, k: R.osc('Sawtooth', p, k, RATE, hz, ph), pos, n, RATE, cut)
        assert got.shape == (n, V) and maxerr(got, f32(ref)) < 3e-7, (pos, n)
    # zero rows / zero voices: accepted, nothing launched, nothing touched
    out = torch.full((4, 4), 7.0, device='cuda')
    row = torch.ones((1, 4), dtype=torch.float64, device='cuda')
    lib = _native.lib()
    assert lib.sig_osc_bank(0, 0, RATE, 0, 4, row.data_ptr(), 1, None, 0, out.data_ptr(), 0, 4, None) == 0
    assert lib.sig_osc_bank(0, 0, RATE, 4, 0, row.data_ptr(), 1, None, 0, out.data_ptr(), 0, 4, None) == 0
    assert lib.sig_sum_bus(0, 4, out.data_ptr(), 4, 0, None, 0, 1, out.data_ptr(), 1, 0, None) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
