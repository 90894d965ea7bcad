"""LowPass / HighPass and White inside block-rate control paths (an LFO softened by a LowPass on a cutoff, smoothed random drift
on `hertz`): the control program evaluates the filter's input per window row and cold-starts the biquad in the launch.  The
per-block rows equal eager one-frame requests bit for bit; whole graphs are bit-identical to eager under fuse=False and within
1e-6 of full scale under the default schedule, the voice program and the specialised kernels; the shapes the batch cannot
reproduce raise NotBatchable."""
import numpy as np
import pytest
import torch

from gpu_helpers import close, gpu_ready, render_batches
from helpers import HOUR, RATE, fix, loc, mkosc, stream, Probe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    gpu_ready()


def smoothed(V, kind='Square', lfo_hz=3.0, cut=4.0, ftype='LowPass', lo=300.0, hi=3000.0):
    """lo + (hi - lo) * Filter(LFO) as Mix(Gain(Filter(LFO), 2 (hi - lo)), 2 lo, 0.5), V columns: (GPU node, oracle node)"""
    from oracle import chain_ref as R
    from signals_amd.chain import fx
    lfo = mkosc(kind, [[lfo_hz] * V])
    f = getattr(fx, ftype)(); f.input = lfo; f.cutoff = fix([[cut] * V])
    g = fx.Gain(); g.left = f; g.right = fix([[2.0 * (hi - lo)]])
    m = fx.Mix(); m.left = g; m.right = fix([[2.0 * lo]]); m.mix = fix([[0.5]])
    btype = {'LowPass': 'lp', 'HighPass': 'hp'}[ftype]
    ref = R.Binary('Mix', R.Binary('Gain', R.Filter(btype, R.Osc(kind, R.Fixed([[lfo_hz] * V])), R.Fixed([[cut] * V])),
                                   R.Fixed([[2.0 * (hi - lo)]])), R.Fixed([[2.0 * lo]]), R.Fixed([[0.5]]))
    return m, ref


def drift(V, base, seed=3):
    """base * (1 + 0.02 * (LowPass(White, 1 Hz) - 0.5)): +-1 % smoothed random drift, V columns"""
    from signals_amd.chain import fx, noise
    w = noise.White(); w.get_state().channels = V; w.get_state().seed = seed
    f = fx.LowPass(); f.input = w; f.cutoff = fix([[1.0] * V])
    g = fx.Gain(); g.left = f; g.right = fix(0.02 * base)
    m = fx.Mix(); m.left = g; m.right = fix(base * 0.99 * 2.0); m.mix = fix([[0.5]])        # 0.5 (0.02 b f) + 0.5 (1.98 b)
    return m


def eager_rows(node, positions, channels):
    p = Probe()
    p.input = node
    rows = [p.input.request(loc(q, 1, channels)).double().cpu().numpy() for q in positions]
    del p.input
    return np.concatenate(rows)


def engine_rows(renderer, node, pos, N, K, channels, continuing=False):
    from signals_amd.engine import _Batch
    b = _Batch(renderer, pos, N, K, continuing)
    b._widths.append(channels)
    return b._control_node(node, 'ctl').cpu().numpy()


# ---------------------------------------------------------------- control rows, bit for bit
@pytest.mark.parametrize('pos', [0, 1, 37, 100, 101, HOUR])
@pytest.mark.parametrize('ftype', ['LowPass', 'HighPass'])
def test_control_rows_equal_eager_one_frame_requests(pos, ftype):
    from signals_amd.engine import BatchRenderer
    V, N, K = 3, 256, 9
    node, _ = smoothed(V, kind='Sawtooth', lfo_hz=41.0, cut=300.0, ftype=ftype)
    r = BatchRenderer(node, V, RATE)
    got = engine_rows(r, node, pos, N, K, V)
    want = eager_rows(smoothed(V, kind='Sawtooth', lfo_hz=41.0, cut=300.0, ftype=ftype)[0], [pos + b * N for b in range(K)], V)
    assert got.shape == (K, V)
    assert np.array_equal(got, want)


def test_noise_control_rows_and_a_batch_continued_across_two_calls():
    from signals_amd.engine import BatchRenderer
    V, N = 8, 160
    base = np.linspace(100.0, 800.0, V)[None, :]
    node = drift(V, base)
    r = BatchRenderer(node, V, RATE)
    got = np.concatenate([engine_rows(r, node, 0, N, 5, V), engine_rows(r, node, 5 * N, N, 4, V, continuing=True)])
    want = eager_rows(drift(V, base), [b * N for b in range(9)], V)
    assert np.array_equal(got, want)


def test_front_row_of_a_control_program():
    from signals_amd.chain import fx
    from signals_amd.engine import BatchRenderer, _Batch
    V, N, K, pos = 4, 300, 5, 9000
    node, _ = smoothed(V)
    g = fx.Gain(); g.left = mkosc('Sine', [[440.0] * V]); g.right = node
    r = BatchRenderer(g, V, RATE)
    rows, fronts = _Batch(r, pos, N, K, False)._control_many([g.right], pos - N, channels=V)
    want = eager_rows(smoothed(V)[0], [pos - N] + [pos + b * N for b in range(K)], V)
    assert np.array_equal(fronts[0].cpu().numpy(), want[:1])
    assert np.array_equal(rows[0].cpu().numpy(), want[1:])


# ---------------------------------------------------------------- whole graphs
def graph_a(V, p):
    """Sine -> LowPass -> Gain, the cutoff a Square LFO through LowPass(4 Hz), 300-3000 Hz"""
    from oracle import chain_ref as R
    from signals_amd.chain import fx
    ctl, ref_ctl = smoothed(V)
    s = mkosc('Sine', p['hertz'], p['phase'])
    f = fx.LowPass(); f.input = s; f.cutoff = ctl
    g = fx.Gain(); g.left = f; g.right = fix(p['gain'])
    ref = R.Binary('Gain', R.Filter('lp', R.Osc('Sine', R.Fixed(p['hertz']), R.Fixed(p['phase'])), ref_ctl), R.Fixed(p['gain']))
    return g, ref


def graph_b(V, p, bus=False):
    """the C2 voice (Sine -> LowPass -> Gain [-> SumBus]) with LowPass(White, 1 Hz) as +-1 % drift on hertz"""
    from signals_amd.chain import ext, fx
    s = mkosc('Sine', p['hertz'], p['phase'])
    s.hertz = drift(V, p['hertz'])
    f = fx.LowPass(); f.input = s; f.cutoff = fix(p['cut'])
    g = fx.Gain(); g.left = f; g.right = fix(p['gain'])
    if not bus:
        return g
    b = ext.SumBus(); b.input = g; b.get_state().gains = np.ascontiguousarray(p['pan'])
    return b


def graph_ring(V, p):
    """RingMod(LowPass(LowPass(Sawtooth)), Sine) with the inner cutoff a smoothed LFO: the voice program's shape"""
    from signals_amd.chain import fx
    ctl, _ = smoothed(V, kind='Triangle', lfo_hz=2.0, cut=6.0, lo=500.0, hi=4000.0)
    s = mkosc('Sawtooth', p['hertz'], p['phase'])
    f1 = fx.LowPass(); f1.input = s; f1.cutoff = ctl
    f2 = fx.LowPass(); f2.input = f1; f2.cutoff = fix(p['cut'])
    r = fx.RingMod(); r.left = f2; r.right = mkosc('Sine', [[5.0] * V])
    return r


def graph_band(V, p):
    """BandPass(Sawtooth) with `low` a smoothed LFO"""
    from signals_amd.chain import fx
    low, _ = smoothed(V, kind='Sine', lfo_hz=1.5, cut=3.0, lo=200.0, hi=600.0)
    s = mkosc('Sawtooth', p['hertz'], p['phase'])
    f = fx.BandPass(); f.input = s; f.low = low; f.high = fix(p['hi'])
    return f


def draw(V, seed=5):
    rng = np.random.default_rng(seed)
    th = rng.uniform(0, np.pi / 2, V)
    return dict(hertz=rng.uniform(55, 1760, (1, V)), phase=rng.uniform(0, 1, (1, V)), cut=rng.uniform(2000, 9000, (1, V)),
                gain=rng.uniform(0.2, 1.0, (1, V)), hi=rng.uniform(2000, 6000, (1, V)), pan=np.stack([np.cos(th), np.sin(th)]))


GRAPHS = {'a': lambda V, p: graph_a(V, p)[0], 'b': lambda V, p: graph_b(V, p), 'b_bus': lambda V, p: graph_b(V, p, bus=True),
          'ring': graph_ring, 'band': graph_band}


@pytest.mark.parametrize('name', list(GRAPHS))
def test_per_node_schedule_is_bit_identical_to_eager(name):
    from signals_amd.engine import KernelTimer
    V, N = 64, 256
    p = draw(V)
    C = 2 if name == 'b_bus' else V
    timer = KernelTimer()
    got = render_batches(GRAPHS[name](V, p), C, 0, N, (4, 3), timer=timer, fuse=False).rows
    torch.cuda.synchronize()
    assert any(k.startswith('control_program[') for k in timer.summary()), set(timer.summary())
    want = stream(GRAPHS[name](V, p), 0, N, 7, C)
    assert np.array_equal(got, want, equal_nan=True)


@pytest.mark.parametrize('mode', ['default', 'always', 'specialise'])
@pytest.mark.parametrize('name', list(GRAPHS))
def test_fused_schedules_match_eager(name, mode):
    from signals_amd import specialise
    if mode == 'specialise' and specialise.hipcc() is None:
        pytest.skip('no hipcc: the specialised kernels cannot be built')
    kw = {'default': {}, 'always': {'fuse_program': 'always'}, 'specialise': {'specialise': True}}[mode]
    V, N = 64, 256
    p = draw(V, seed=11)
    C = 2 if name == 'b_bus' else V
    got = render_batches(GRAPHS[name](V, p), C, 0, N, (4, 3), **kw).rows
    close(got, stream(GRAPHS[name](V, p), 0, N, 7, C), (name, mode))


def test_fm_path_takes_the_fused_walker():
    from signals_amd.engine import KernelTimer
    V, N = 64, 256
    p = draw(V, seed=2)
    timer = KernelTimer()
    got = render_batches(graph_b(V, p, bus=True), 2, 0, N, (3, 3), timer=timer).rows
    torch.cuda.synchronize()
    names = set(timer.summary())
    assert any('fm' in k or 'fused' in k for k in names), names
    close(got, stream(graph_b(V, p, bus=True), 0, N, 6, 2), 'fm')


@pytest.mark.parametrize('pos', [0, 4800])
def test_smoothed_lfo_cutoff_against_the_oracle(pos):
    from oracle import chain_ref as R
    V, N, K = 16, 256, 5
    p = draw(V, seed=4)
    node, ref = graph_a(V, p)
    got = render_batches(node, V, pos, N, (K,)).rows
    want = R.render_stream(ref, pos, N, K, V)
    close(got, want, ('oracle', pos))


# ---------------------------------------------------------------- errors and the shapes left to the eager path
def test_bad_cutoff_raises_the_eager_error():
    from signals_amd import runtime
    V, N = 4, 256
    p = draw(V)
    node = graph_a(V, p)[0]
    ctl_filter(node).cutoff = fix([[30000.0] * V])            # the control filter's Wn > 1
    with pytest.raises(ValueError):
        stream(node, 0, N, 1, V)
        runtime.check_status()
    node = graph_a(V, p)[0]
    ctl_filter(node).cutoff = fix([[30000.0] * V])
    with pytest.raises(ValueError):
        render_batches(node, V, 0, N, (3,), fuse=False).rows
        runtime.check_status()
    for _ in range(8):                                               # (check_status raises at the first word it finds set)
        try:
            runtime.check_status()
            break
        except ValueError:
            pass


def ctl_filter(g):
    """the LowPass inside graph (a)'s cutoff path"""
    return g.left.sig.cutoff.sig.left.sig.left.sig


def out_of_scope():
    from signals_amd.chain import fx
    V = 4
    p = draw(V)
    cases = {}
    g = graph_a(V, p)[0]                                             # N <= 100
    cases['short blocks'] = (g, 64)
    g = graph_a(V, p)[0]                                             # a filter of a filter
    lp = ctl_filter(g)
    inner = fx.LowPass(); inner.input = lp.input.sig; inner.cutoff = fix([[50.0] * V]); lp.input = inner
    cases['filter of a filter'] = (g, 256)
    g = graph_a(V, p)[0]                                             # a modulated oscillator inside the window
    lfo = ctl_filter(g).input.sig
    lfo.hertz = mkosc('Sine', [[0.5] * V])
    cases['modulated oscillator'] = (g, 256)
    g = graph_a(V, p)[0]                                             # a shared input node
    lfo = ctl_filter(g).input.sig
    r = fx.RingMod(); r.left = g; r.right = lfo
    cases['shared input'] = (r, 256)
    return cases


@pytest.mark.parametrize('case', ['short blocks', 'filter of a filter', 'modulated oscillator', 'shared input'])
def test_out_of_scope_shapes_raise_not_batchable(case):
    from signals_amd.engine import BatchRenderer, NotBatchable
    node, N = out_of_scope()[case]
    r = BatchRenderer(node, 4, RATE, fuse=False)
    with pytest.raises(NotBatchable):
        r.render(0, N, 3)
    r = BatchRenderer(node, 4, RATE)
    with pytest.raises(NotBatchable):
        r.render(0, N, 3)


@pytest.mark.parametrize('case', ['short blocks', 'filter of a filter'])
def test_block_driver_over_an_out_of_scope_graph_equals_eager(case):
    from signals_amd.chain.driver import BlockDriver
    node, N = out_of_scope()[case]
    want = stream(out_of_scope()[case][0], 0, N, 4, 4)
    d = BlockDriver(blocksize=N); d.get_state().channels = 4; d.input = node
    got = d.render(4)
    assert np.array_equal(np.asarray(got), want)


def test_fresh_start_with_history_in_front_is_left_to_eager():
    from signals_amd.engine import BatchRenderer, NotBatchable
    V = 8
    p = draw(V)
    r = BatchRenderer(graph_b(V, p), V, RATE, fuse=False)
    with pytest.raises(NotBatchable):
        r.render(4800, 256, 2)
