"""ext.ADSR inside block-rate control paths (a filter envelope on a cutoff, a pitch envelope on `hertz`): the control program's
AdsrArgs / Adsr pair.  The per-block rows equal eager one-frame requests and the definition (oracle/chain_ref.py:adsr) bit for
bit, through the interpreter, the specialised kernel and the multi-port launch with its front row, and at window rate under a
LowPass; whole graphs are within 1e-6 max(1, |ref|) of the oracle graph on every route and bit-identical to eager under fuse=False.

Parameter set: tests/adsr_control_cases.py.  Whole graphs: 70 voices (they cross a wave), two batches of 5 and 4 blocks, blocks of
64 (shorter than the filters' context) and 256 frames, positions 0 and one hour; cutoffs from 300 to 6000 Hz, inside (0, rate / 2).
References are rendered once per (graph, block size, position) and shared by the routes."""
import functools

import numpy as np
import pytest
import torch

import adsr_control_cases as A
from gpu_helpers import gpu_ready, render_batches
from helpers import HOUR, RATE, fix, loc, maxerr, mkosc, stream, Probe

pytestmark = pytest.mark.gpu

N_ROWS, K_ROWS = 256, 9


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    gpu_ready()


def eager_rows(node, positions, channels):
    p = Probe()
    p.input = node
    rows = [p.input.request(loc(q, 1, channels)).double().cpu().numpy() for q in positions]
    del p.input
    return np.concatenate(rows)


def engine_rows(renderer, node, pos, N, K, channels):
    from signals_amd.engine import _Batch
    b = _Batch(renderer, pos, N, K, False)
    b._widths.append(channels)
    return b._control_node(node, 'ctl').cpu().numpy()


def specialised(mode):
    from signals_amd import specialise
    if mode == 'specialise' and specialise.hipcc() is None:
        pytest.skip('no hipcc: the specialised kernels cannot be built')
    return {'specialise': True} if mode == 'specialise' else {}


def launched(timer):
    torch.cuda.synchronize()
    names = set(timer.summary())
    assert any(k.startswith('control_program[block-rate]') for k in names), names
    return names


# ---------------------------------------------------------------- control rows, bit for bit
@pytest.mark.parametrize('pos', A.POSITIONS)
@pytest.mark.parametrize('mode', ['interpreter', 'specialise'])
def test_rows_equal_eager_and_the_definition(pos, mode):
    from signals_amd.engine import BatchRenderer, KernelTimer
    N, K, V = N_ROWS, K_ROWS, A.V
    p = A.rows(N, pos)
    positions = [pos + b * N for b in range(K)]
    want = A.oracle(p, positions)
    node, timer = A.node(p), KernelTimer()
    got = engine_rows(BatchRenderer(node, V, RATE, timer=timer, **specialised(mode)), node, pos, N, K, V)
    names = launched(timer)
    assert mode != 'specialise' or 'control_program[block-rate]*specialised' in names, names
    assert got.shape == (K, V) and got.dtype == np.float64
    assert np.array_equal(got, want)
    assert np.array_equal(eager_rows(A.node(p), positions, V), want)


@pytest.mark.parametrize('pos', A.POSITIONS)
@pytest.mark.parametrize('mode', ['interpreter', 'specialise'])
def test_rows_and_front_row_of_a_multi_port_launch(pos, mode):
    """`_control_many` over two ports -- the envelope itself and a cutoff swept by a second reader of it -- from the batch's second
    block on, the first block's position as the front position one block in front"""
    from signals_amd.chain import fx
    from signals_amd.engine import BatchRenderer, _Batch
    N, K, V = N_ROWS, K_ROWS, A.V
    p = A.rows(N, pos)
    positions = [pos + b * N for b in range(K)]
    want = A.oracle(p, positions)
    env = A.node(p)
    g = fx.Gain(); g.left = mkosc('Sine', [[440.0] * V]); g.right = env
    m = fx.Mix(); m.left = fix([[6000.0]]); m.right = fix([[300.0]]); m.mix = env
    f = fx.LowPass(); f.input = g; f.cutoff = m
    r = BatchRenderer(f, V, RATE, **specialised(mode))
    rows, fronts = _Batch(r, pos + N, N, K - 1, False)._control_many([g.right, f.cutoff], pos, channels=V)
    assert np.array_equal(fronts[0].cpu().numpy(), want[:1]) and np.array_equal(rows[0].cpu().numpy(), want[1:])
    cut = want * 6000.0 + (1.0 - want) * 300.0                      # fx.py:40, one rounding per operation
    assert np.array_equal(fronts[1].cpu().numpy(), cut[:1]) and np.array_equal(rows[1].cpu().numpy(), cut[1:])


def test_a_disabled_envelope_answers_zeros():
    from signals_amd.engine import BatchRenderer
    node = A.node(A.rows())
    node.get_state().enabled = False
    got = engine_rows(BatchRenderer(node, A.V, RATE), node, 0, N_ROWS, K_ROWS, A.V)
    assert got.shape == (1, 1) and not got.any()


# ---------------------------------------------------------------- window rate: a slewed envelope
def slewed(p, V):
    from signals_amd.chain import fx
    f = fx.LowPass(); f.input = A.node(p); f.cutoff = fix([[30.0] * V])
    return f


@pytest.mark.parametrize('pos', [0, 37, 101, HOUR])
@pytest.mark.parametrize('mode', ['interpreter', 'specialise'])
def test_window_rate_rows_equal_eager(pos, mode):
    from signals_amd.engine import BatchRenderer
    N, K, V = N_ROWS, K_ROWS, A.V
    p = A.rows(N, pos)
    node = slewed(p, V)
    got = engine_rows(BatchRenderer(node, V, RATE, **specialised(mode)), node, pos, N, K, V)
    want = eager_rows(slewed(p, V), [pos + b * N for b in range(K)], V)
    assert got.shape == (K, V)
    assert np.ptp(want, axis=0).min() > 1e-3                        # (every column moves)
    assert np.array_equal(got, want)


# ---------------------------------------------------------------- whole graphs
VOICES, BATCHES = 70, (5, 4)
BASE, PEAK = 300.0, 6000.0


def draw(V, seed=9):
    rng = np.random.default_rng(seed)
    th = rng.uniform(0, np.pi / 2, V)
    return dict(hertz=rng.uniform(55, 1760, (1, V)), phase=rng.uniform(0, 1, (1, V)), gain=rng.uniform(0.2, 1.0, (1, V)),
                q=rng.choice([0.7, 2.0, 4.0], (1, V)), pan=np.stack([np.cos(th), np.sin(th)]))


def sweep(env, ref_env, peak=PEAK, base=BASE):
    """base + (peak - base) * envelope as Mix(peak, base, mix=envelope): (GPU node, oracle node)"""
    from oracle import chain_ref as R
    from signals_amd.chain import fx
    m = fx.Mix(); m.left = fix([[peak]]); m.right = fix([[base]]); m.mix = env
    return m, R.Binary('Mix', R.Fixed([[peak]]), R.Fixed([[base]]), ref_env)


def second(e):
    """the amplitude envelope of graph (b): the cutoff's, slower"""
    return {**e, 'decay': e['decay'] * 1.5, 'sustain': np.array([[0.4]]), 'release': e['release'] * 0.5 + 1e-4}


def graph(which, N, pos):
    """(GPU node, oracle node) under a stereo bus"""
    from oracle import chain_ref as R
    from signals_amd.chain import ext, fx
    import resonant_reference as RR
    V = VOICES
    p, e = draw(V), A.rows(N, pos, V)
    env, ref_env = A.node(e), R.Adsr(**e)
    if which == 'a':                                                  # Sine -> LowPass(cutoff envelope) -> Gain
        cut, ref_cut = sweep(env, ref_env)
        f = fx.LowPass(); f.input = mkosc('Sine', p['hertz'], p['phase']); f.cutoff = cut
        top = fx.Gain(); top.left = f; top.right = fix(p['gain'])
        ref = R.Binary('Gain', R.Filter('lp', R.Osc('Sine', R.Fixed(p['hertz']), R.Fixed(p['phase'])), ref_cut), R.Fixed(p['gain']))
    elif which in ('b', 'd'):                                         # Sawtooth -> ResonantLowPass(cutoff envelope) -> RingMod(., ADSR)
        cut, ref_cut = sweep(env, ref_env)
        f = ext.ResonantLowPass(); f.input = mkosc('Sawtooth', p['hertz'], p['phase']); f.cutoff = cut; f.resonance = fix(p['q'])
        amp, ref_amp = (env, ref_env) if which == 'd' else (A.node(second(e)), R.Adsr(**second(e)))       # (d): ONE envelope for both
        top = fx.RingMod(); top.left = f; top.right = amp
        ref = R.Binary('RingMod', RR.oracle_node()('lp', R.Osc('Sawtooth', R.Fixed(p['hertz']), R.Fixed(p['phase'])), ref_cut,
                                                   R.Fixed(p['q'])), ref_amp)
    else:                                                             # (c) a kick: Sine with hertz on an envelope -> Gain
        hz, ref_hz = sweep(env, ref_env, 200.0, 50.0)
        s = mkosc('Sine', p['hertz'], p['phase']); s.hertz = hz
        top = fx.Gain(); top.left = s; top.right = fix(p['gain'])
        ref = R.Binary('Gain', R.Osc('Sine', ref_hz, R.Fixed(p['phase'])), R.Fixed(p['gain']))
    bus = ext.SumBus(); bus.input = top; bus.get_state().gains = np.ascontiguousarray(p['pan'])
    return bus, R.SumBus(ref, p['pan'])


@functools.lru_cache(maxsize=None)
def references(which, N, pos):
    """(oracle, eager) rows of the nine blocks, read-only"""
    from oracle import chain_ref as R
    node, ref = graph(which, N, pos)
    want = R.render_stream(ref, pos, N, sum(BATCHES), 2)
    eager = stream(node, pos, N, sum(BATCHES), 2)
    want.setflags(write=False); eager.setflags(write=False)
    return want, eager


def batches(which, N, pos, **kw):
    from signals_amd.engine import KernelTimer
    timer = KernelTimer()
    got = render_batches(graph(which, N, pos)[0], 2, pos, N, BATCHES, timer=timer, **kw).rows           # (NotBatchable would surface here)
    return got, launched(timer)


def close(got, ref, what):
    tol = 1e-6 * np.maximum(1.0, np.abs(ref))
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    print(what, 'max|err|', float(err.max()), 'max|ref|', float(np.abs(ref).max()))
    assert got.shape == ref.shape and not np.isnan(got).any()
    assert (err <= tol).all(), (what, float((err / tol).max()))


ROUTES = [('a', 'default'), ('b', 'default'), ('b', 'specialise'), ('c', 'default'), ('d', 'default')]


@pytest.mark.parametrize('pos', [0, HOUR])
@pytest.mark.parametrize('N', [64, 256])
@pytest.mark.parametrize('which,mode', ROUTES)
def test_graph_against_the_oracle(which, mode, N, pos):
    want, _ = references(which, N, pos)
    got, names = batches(which, N, pos, **specialised(mode))
    assert np.abs(want).max() > 0.5                                  # (the voices sound)
    close(got, want, (which, mode, N, pos, sorted(names)))


@pytest.mark.parametrize('pos', [0, HOUR])
@pytest.mark.parametrize('N', [64, 256])
@pytest.mark.parametrize('which', ['a', 'b', 'c', 'd'])
def test_per_node_schedule_is_bit_identical_to_eager(which, N, pos):
    want, eager = references(which, N, pos)
    got, _ = batches(which, N, pos, fuse=False)
    close(got, want, (which, 'fuse=False', N, pos))
    assert np.array_equal(got, eager)
