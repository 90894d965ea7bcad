"""Swept band filters in the batched engine: BandPass / BandStop whose `low` / `high` ports follow block-rate LFOs.  The per-node
schedule (band_coldstart with one band per block) is bit-identical to the eager pull path; the voice program (its Band
instruction: two filter slots, designed per block in the kernel) is within 1e-6 of it, for long blocks, for blocks shorter than
the filter context, alone and behind a LowPass, and against the CPU oracle.  A sweep that crosses low >= high poisons exactly the
blocks it crosses in, as eager does."""
import numpy as np
import pytest
import torch

from gpu_helpers import close, gpu_ready, lfo, render_batches
from helpers import RATE, f32, fix, maxerr, mkosc, stream

pytestmark = pytest.mark.gpu

CLASSES = (('BandPass', 'bp'), ('BandStop', 'bs'))


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    gpu_ready()


def draw(V, seed=5):
    rng = np.random.default_rng(seed)
    lo = rng.uniform(150, 2500, (1, V))
    return dict(hertz=rng.uniform(55, 1760, (1, V)), phase=rng.uniform(0, 1, (1, V)), lo=lo, hi=lo * rng.uniform(2.5, 4.0, (1, V)),
                cut=rng.uniform(2000, 9000, (1, V)), gain=rng.uniform(0.2, 1.0, (1, V)))


def swept(cls, p, behind_lowpass=False, low_depth=0.4, high_depth=0.3):
    """Band(Sawtooth) [Band(LowPass(Sawtooth))] with low = LFO around lo, high = LFO around hi: (GPU node, oracle node)"""
    from oracle import chain_ref as R
    from signals_amd.chain import fx
    btype = dict(CLASSES)[cls]
    src = mkosc('Sawtooth', p['hertz'], p['phase'])
    ref_src = R.Osc('Sawtooth', R.Fixed(p['hertz']), R.Fixed(p['phase']))
    if behind_lowpass:
        lp = fx.LowPass(); lp.input = src; lp.cutoff = fix(p['cut'])
        src, ref_src = lp, R.Filter('lp', ref_src, R.Fixed(p['cut']))
    low, ref_low = lfo(37.0, low_depth * p['lo'], p['lo'])
    high, ref_high = lfo(23.0, high_depth * p['hi'], p['hi'])
    f = getattr(fx, cls)(); f.input = src; f.low = low; f.high = high
    return f, R.BandFilter(btype, ref_src, ref_low, ref_high)


@pytest.mark.parametrize('pos', [0, 1000])
@pytest.mark.parametrize('cls', [c for c, _ in CLASSES])
def test_per_node_schedule_is_bit_identical_to_eager(cls, pos):
    from signals_amd.engine import KernelTimer
    V, N = 96, 256
    p = draw(V)
    timer = KernelTimer()
    got = render_batches(swept(cls, p)[0], V, pos, N, (4, 3), timer=timer, fuse=False).rows
    torch.cuda.synchronize()
    assert any(k.startswith('band_coldstart[') and k.endswith(',blocks]') for k in timer.summary()), set(timer.summary())
    want = stream(swept(cls, p)[0], pos, N, 7, V)
    assert np.array_equal(got, want, equal_nan=True)


@pytest.mark.parametrize('mode', ['default', 'always', 'specialise'])
@pytest.mark.parametrize('pos', [0, 1000])
@pytest.mark.parametrize('cls', [c for c, _ in CLASSES])
def test_voice_program_matches_eager(cls, pos, mode):
    from signals_amd import specialise
    if mode == 'specialise' and specialise.hipcc() is None:
        pytest.skip('no hipcc: the specialised kernel cannot be built')
    kw = {'default': {}, 'always': {'fuse_program': 'always'}, 'specialise': {'specialise': True}}[mode]
    V, N = 96, 256
    p = draw(V)
    got = render_batches(swept(cls, p)[0], V, pos, N, (4, 3), **kw).rows
    close(got, stream(swept(cls, p)[0], pos, N, 7, V), (cls, pos, mode))


@pytest.mark.parametrize('mode', ['default', 'specialise'])
def test_bus_over_a_swept_band_is_one_voice_program_launch(mode):
    from signals_amd import specialise
    from signals_amd.chain import ext, fx
    from signals_amd.engine import KernelTimer
    if mode == 'specialise' and specialise.hipcc() is None:
        pytest.skip('no hipcc: the specialised kernel cannot be built')
    V, N = 128, 256
    p = draw(V, seed=9)
    th = np.random.default_rng(3).uniform(0, np.pi / 2, V)
    pan = np.stack([np.cos(th), np.sin(th)])

    def build():
        g = fx.Gain(); g.left = swept('BandPass', p)[0]; g.right = fix(p['gain'])
        b = ext.SumBus(); b.input = g; b.get_state().gains = np.ascontiguousarray(pan)
        return b
    timer = KernelTimer()
    got = render_batches(build(), 2, 0, N, (4, 4), timer=timer, specialise=(mode == 'specialise')).rows
    names = set(timer.summary())
    assert any(k.startswith('voice_program_bus[') for k in names), names
    assert not any(k.startswith('band_coldstart') for k in names), names
    assert not any(k.startswith('osc_bank') and 'block-rate' not in k for k in names), names
    if mode == 'specialise':
        assert any('*specialised' in k for k in names), names
    close(got, stream(build(), 0, N, 8, 2), mode)


@pytest.mark.parametrize('behind_lowpass', [False, True])
@pytest.mark.parametrize('N', [16, 32, 64, 99])
@pytest.mark.parametrize('cls', [c for c, _ in CLASSES])
def test_short_blocks(cls, N, behind_lowpass):
    """blocks shorter than the filter context, continuing batches: alone (depth 1) and behind a LowPass (depth 2, which the
    per-node schedule cannot batch)"""
    from signals_amd.engine import KernelTimer
    V = 64
    p = draw(V, seed=11)
    timer = KernelTimer()
    got = render_batches(swept(cls, p, behind_lowpass)[0], V, 0, N, (5, 6), timer=timer).rows
    torch.cuda.synchronize()
    assert any(k.startswith('voice_program[') for k in timer.summary()), set(timer.summary())
    close(got, stream(swept(cls, p, behind_lowpass)[0], 0, N, 11, V), (cls, N, behind_lowpass))


@pytest.mark.parametrize('cls,btype', CLASSES)
def test_against_the_oracle(cls, btype):
    from oracle import chain_ref as R
    V, N, K = 1024, 256, 16
    p = draw(V, seed=21)
    node, ref = swept(cls, p)
    got = render_batches(node, V, 0, N, (K,)).rows
    want = R.render_stream(ref, 0, N, K, V)
    assert maxerr(got, f32(want)) < 5e-7, cls


@pytest.mark.parametrize('kw', [{'fuse': False}, {}, {'fuse_program': 'always'}])
def test_a_sweep_that_crosses_low_and_high_poisons_only_those_blocks(kw):
    from signals_amd import runtime
    try:
        runtime.check_status()                   # (nothing pending from earlier tests)
    except ValueError:
        pass
    V, N, K = 64, 256, 12
    p = draw(V, seed=4)
    p['hi'] = p['lo'] * 1.3                       # low swings +-90 %, high +-10 %: some blocks have low >= high
    from signals_amd.engine import BatchRenderer
    node = swept('BandPass', p, low_depth=0.9, high_depth=0.1)[0]
    r = BatchRenderer(node, V, RATE, **kw)                                    # (kept: its status words live as long as it does)
    got = r.render(0, N, K).cpu().numpy()
    with pytest.raises(ValueError):
        runtime.check_status()
    eager_node = swept('BandPass', p, low_depth=0.9, high_depth=0.1)[0]
    want = stream(eager_node, 0, N, K, V)
    with pytest.raises(ValueError):
        runtime.check_status()
    bad = np.isnan(want).reshape(K, N, V)
    assert bad.any() and not bad.all()
    assert (bad.all(axis=1) | ~bad.any(axis=1)).all()                        # whole blocks of one voice
    assert np.array_equal(np.isnan(got), np.isnan(want))
    if kw.get('fuse') is False:
        assert np.array_equal(got, want, equal_nan=True)
    else:
        close(got, want, kw)
