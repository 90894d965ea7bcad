"""ADSR envelopes whose stage boundaries land exactly on sample rows (tests/envelopes.py: round numbers, whole frame counts,
hand-placed edges, hours into the stream) through every route that renders an envelope, against the oracle:

  * the routes that follow the envelope as a line per stage (sig_adsr.h: segment_at) -- the fused cascade
    (fused_cascade_bus, BASELINE config 3's default schedule), the filter + envelope + bus pass (biquad_bus), the
    voice-program interpreter and its specialised images -- within 1e-6 of full scale;
  * the routes that evaluate the definition at every row -- the ADSR node (bit-exact) and the filter's envelope epilogue.

Every test asserts that the rows it renders hold exact stage boundaries (envelopes.boundary_rows), so that it keeps its point."""
import numpy as np
import pytest
import torch

import envelopes as E
from gpu_helpers import render_batches, tolerance
from helpers import RATE, f32, fix, maxerr, mkosc

pytestmark = pytest.mark.gpu
CASCADE = 'fused_cascade_bus[Sawtooth,lp,lp,env]'


@pytest.fixture(scope='module', autouse=True)
def _device():
    assert torch.cuda.is_available()
    from signals_amd import _native, runtime
    runtime.set_device('cuda:0')
    yield
    torch.cuda.synchronize()
    _native.set_fused_cascade_tuning()
    _native.set_voice_program_tuning()
    _native.voice_program_use_attached(True)


def names(timer):
    torch.cuda.synchronize()
    return set(timer.summary())


def voices(env, seed):
    """oscillator and filter rows for the voices of an envelope table"""
    V = env['attack'].shape[1]
    rng = np.random.default_rng(seed)
    th = rng.uniform(0, np.pi / 2, V)
    return dict(hertz=rng.uniform(55, 1760, (1, V)), phase=rng.uniform(0, 1, (1, V)), cut1=rng.uniform(200, 8000, (1, V)),
                cut2=rng.uniform(200, 8000, (1, V)), env=env, pan=np.stack([np.cos(th), np.sin(th)]))


def mk_adsr(env):
    from signals_amd.chain import ext
    a = ext.ADSR()
    for k in E.PARAMS:
        setattr(a, k, fix(env[k]))
    return a


def c3(p, pan=None):
    """Saw -> LowPass -> LowPass -> x ADSR -> SumBus (BASELINE config 3), and its oracle"""
    from oracle import chain_ref as R
    from signals_amd.chain import ext, fx
    f1 = fx.LowPass(); f1.input = mkosc('Sawtooth', p['hertz'], p['phase']); f1.cutoff = fix(p['cut1'])
    f2 = fx.LowPass(); f2.input = f1; f2.cutoff = fix(p['cut2'])
    rm = fx.RingMod(); rm.left = f2; rm.right = mk_adsr(p['env'])
    bus = ext.SumBus(); bus.input = rm
    if pan is not None:
        bus.get_state().gains = np.ascontiguousarray(pan)
    o = R.Filter('lp', R.Filter('lp', R.Osc('Sawtooth', R.Fixed(p['hertz']), R.Fixed(p['phase'])), R.Fixed(p['cut1'])),
                 R.Fixed(p['cut2']))
    return bus, R.Binary('RingMod', o, R.Adsr(**p['env']))


def ringmod(p, side):
    """RingMod(LowPass(Saw), ADSR) with the envelope on the given side, and its oracle"""
    from oracle import chain_ref as R
    from signals_amd.chain import fx
    f = fx.LowPass(); f.input = mkosc('Sawtooth', p['hertz'], p['phase']); f.cutoff = fix(p['cut1'])
    rm = fx.RingMod()
    rf = R.Filter('lp', R.Osc('Sawtooth', R.Fixed(p['hertz']), R.Fixed(p['phase'])), R.Fixed(p['cut1']))
    if side == 'left':
        rm.left, rm.right = mk_adsr(p['env']), f
        return rm, R.Binary('RingMod', R.Adsr(**p['env']), rf)
    rm.left, rm.right = f, mk_adsr(p['env'])
    return rm, R.Binary('RingMod', rf, R.Adsr(**p['env']))


def assert_boundaries(env, position, frames, at_least):
    """the window's rows hold exact stage boundaries of at least `at_least` envelopes"""
    hit = E.boundary_rows(env, position, frames).any(axis=0)
    assert hit.sum() >= at_least, (position, frames, int(hit.sum()))


# --------------------------------------------------------------------------------------------------- the fused cascade
POSITIONS = [0, 24_000, E.HOUR, 10 * E.HOUR]


@pytest.mark.parametrize('N', [1024, 256])
@pytest.mark.parametrize('position', POSITIONS)
def test_fused_cascade_vs_oracle(position, N):
    """C3 over the whole table, a fresh graph at `position`: mono and stereo, one batch of 9 blocks, batches of 5 + 3 + 1
    (the later ones continue the stream) and forced launch geometries, against the oracle's sequential render"""
    from oracle import chain_ref as R
    from signals_amd import _native
    from signals_amd.engine import KernelTimer
    K = 9
    env, kinds = E.table(position, N, K, seed=position % 997 + N)
    p = voices(env, 7)
    V = env['attack'].shape[1]
    assert_boundaries(env, position, K * N, 100)
    _, node = c3(p)
    per_voice = R.render_stream(node, position, N, K, V)
    try:
        for pan in (None, p['pan']):
            ref = R.sum_bus(per_voice, pan)
            scale = max(1.0, float(np.abs(ref).max()))
            C = 1 if pan is None else 2
            for geometry, batches in (((0, 0), (K,)), ((0, 0), (5, 3, 1)), ((1, 1), (K,)), ((4, 4), (5, 3, 1)), ((2, 8), (K,))):
                _native.set_fused_cascade_tuning(*geometry)
                timer = KernelTimer()
                got = render_batches(c3(p, pan)[0], C, position, N, batches, timer=timer).rows
                assert names(timer) == {CASCADE}, names(timer)
                err = maxerr(got, f32(ref))
                assert err < 1e-6 * scale, (position, N, C, geometry, batches, err, scale)
    finally:
        _native.set_fused_cascade_tuning()


def test_fused_cascade_grid_vs_the_per_node_schedule_over_many_blocks():
    """1024 round-number envelopes from the grid of the issue that set these tests (gate_on 0 / 0.5 s, stages of 0 to
    200 ms, gates of 5 ms to 1 s) over 64 blocks of 1024 (1.4 s), the cascade against fuse=False (one kernel per node:
    the ADSR node evaluates the definition at every row), each within 1e-6 of full scale of the oracle, so within 2e-6
    of each other; continuing batches of 24 + 40"""
    from signals_amd.engine import KernelTimer
    N, K = 1024, 64
    grid = E.round_grid([0.0, 0.5], [0, 1, 5, 10, 20, 50, 100], [0, 10, 50, 100, 200], [0, 10, 100, 200, 500], [5, 50, 300, 1000])
    pick = np.sort(np.random.default_rng(3).permutation(grid['attack'].shape[1])[:1024])
    env = {k: np.ascontiguousarray(v[:, pick]) for k, v in grid.items()}
    p = voices(env, 11)
    assert_boundaries(env, 0, K * N, 600)
    timer = KernelTimer()
    got = render_batches(c3(p)[0], 1, 0, N, (24, 40), timer=timer).rows
    assert names(timer) == {CASCADE}, names(timer)
    timer = KernelTimer()
    plain = render_batches(c3(p)[0], 1, 0, N, (24, 40), timer=timer, fuse=False).rows
    assert not any('cascade' in n or 'bus[' in n or n.startswith('voice_program') for n in names(timer)), names(timer)
    scale = max(1.0, float(np.abs(plain).max()))
    assert maxerr(got, plain) < 2e-6 * scale, (maxerr(got, plain), scale)


@pytest.mark.parametrize('position', [0, E.HOUR])
def test_filter_envelope_bus_pass_vs_oracle(position):
    """the schedule behind fuse_program=False without the cascade kernel: the outer filter, the envelope and the bus in one
    pass (sig_biquad_coldstart_bus, which tracks the envelope like the cascade), continuing batches"""
    from oracle import chain_ref as R
    from signals_amd.engine import BatchRenderer, KernelTimer
    N, K = 1024, 9
    env, _ = E.table(position, N, K, seed=5)
    p = voices(env, 13)
    V = env['attack'].shape[1]
    assert_boundaries(env, position, K * N, 100)
    _, node = c3(p)
    per_voice = R.render_stream(node, position, N, K, V)
    for pan in (None, p['pan']):
        ref = R.sum_bus(per_voice, pan)
        timer = KernelTimer()
        r = BatchRenderer(c3(p, pan)[0], 1 if pan is None else 2, RATE, timer=timer, fuse_program=False)
        r.fuse_cascade = False
        got = np.concatenate([r.render(position, N, 5).cpu().numpy(), r.render(position + 5 * N, N, 4).cpu().numpy()])
        assert 'biquad_bus[lp,env]' in names(timer), names(timer)
        assert maxerr(got, f32(ref)) < tolerance(ref), position


# ------------------------------------------------------------------------------------------ voice programs
def program_case(position, N, side, seed):
    K = 1536 // N                                                           # 32 ms whatever the block size
    env, _ = E.table(position, N, K, seed=seed + N)
    p = voices(env, seed)
    return K, env, p


@pytest.mark.parametrize('side', ['left', 'right'])
@pytest.mark.parametrize('position', [0, E.HOUR])
def test_voice_program_interpreter_vs_oracle(position, side):
    """RingMod(LowPass(Saw), ADSR), the envelope either side, as one interpreted launch (fuse_program='always'): stored per
    voice and under a stereo bus, one and two voices per lane, N = 256, 64 and 32, batches continuing the stream"""
    from oracle import chain_ref as R
    from signals_amd import _native
    from signals_amd.chain import ext
    from signals_amd.engine import KernelTimer
    _native.voice_program_use_attached(False)
    try:
        for N in (256, 64, 32):
            K, env, p = program_case(position, N, side, 17)
            V = env['attack'].shape[1]
            assert_boundaries(env, position, K * N, 100)
            ref = R.render_stream(ringmod(p, side)[1], position, N, K, V)
            ref_bus = R.sum_bus(ref, p['pan'])
            batches = (K // 2, K // 3, K - K // 2 - K // 3)
            for vpl in (1, 2):
                _native.set_voice_program_tuning(vpl, 1)
                timer = KernelTimer()
                got = render_batches(ringmod(p, side)[0], V, position, N, batches, timer=timer, fuse_program='always',
                                     specialise=False).rows
                launched = names(timer)
                assert any(n.startswith('voice_program') for n in launched) and not any('specialised' in n for n in launched), launched
                assert maxerr(got, f32(ref)) < tolerance(ref), (position, side, N, vpl)
                bus = ext.SumBus(); bus.input = ringmod(p, side)[0]
                bus.get_state().gains = np.ascontiguousarray(p['pan'])
                timer = KernelTimer()
                got = render_batches(bus, 2, position, N, batches, timer=timer, fuse_program='always', specialise=False).rows
                launched = names(timer)
                assert any(n.startswith('voice_program_bus') for n in launched), launched
                assert maxerr(got, f32(ref_bus)) < tolerance(ref_bus), (position, side, N, vpl, 'bus')
    finally:
        _native.set_voice_program_tuning()
        _native.voice_program_use_attached(True)


@pytest.mark.parametrize('bus', [False, True])
@pytest.mark.parametrize('side', ['left', 'right'])
def test_specialised_image_vs_oracle(side, bus):
    """the same graphs through the kernel built for their program (specialise=True: the extended handlers), one and two
    voices per lane, N = 256, 64 and 32, deep in the stream"""
    from oracle import chain_ref as R
    from signals_amd import _native, specialise
    from signals_amd.chain import ext
    from signals_amd.engine import KernelTimer
    if specialise.hipcc() is None:
        pytest.skip('no hipcc on this machine: nothing to specialise with')
    position = E.HOUR
    try:
        for N in (256, 64, 32):
            K, env, p = program_case(position, N, side, 23)
            V = env['attack'].shape[1]
            assert_boundaries(env, position, K * N, 100)
            ref = R.render_stream(ringmod(p, side)[1], position, N, K, V)
            C = V
            if bus:
                ref, C = R.sum_bus(ref, p['pan']), 2
            for vpl in (1, 2):
                _native.set_voice_program_tuning(vpl, 1)
                node = ringmod(p, side)[0]
                if bus:
                    top = ext.SumBus(); top.input = node
                    top.get_state().gains = np.ascontiguousarray(p['pan'])
                    node = top
                timer = KernelTimer()
                got = render_batches(node, C, position, N, (K // 2, K - K // 2), timer=timer, fuse_program='always', specialise=True).rows
                assert any(n.endswith('*specialised') for n in names(timer)), names(timer)
                assert maxerr(got, f32(ref)) < tolerance(ref), (side, bus, N, vpl)
    finally:
        _native.set_voice_program_tuning()


# ----------------------------------------------------------------------- control legs: the definition at every row
@pytest.mark.parametrize('position', [0, 24_000, E.HOUR, int(2.3 * E.HOUR), 10 * E.HOUR])
def test_adsr_node_bit_exact_on_the_table(position):
    from oracle import chain_ref as R
    N, K = 1024, 9
    env, _ = E.table(position, N, K, seed=29)
    V = env['attack'].shape[1]
    assert_boundaries(env, position, K * N, 100)
    got = render_batches(mk_adsr(env), V, position, N, (4, 5)).rows
    assert np.array_equal(got, f32(R.adsr(position, K * N, RATE, **env))), position


@pytest.mark.parametrize('position', [0, E.HOUR])
def test_filter_envelope_epilogue_on_the_table(position):
    """RingMod(Filter, ADSR) as the sink of the per-node schedule: the envelope in the outer filter's epilogue
    (sig_biquad_coldstart_env) behind two filters, and behind one"""
    from oracle import chain_ref as R
    from signals_amd.engine import KernelTimer
    N, K = 256, 6
    env, _ = E.table(position, N, K, seed=31)
    p = voices(env, 37)
    V = env['attack'].shape[1]
    assert_boundaries(env, position, K * N, 100)
    for graph, ref_node in ((c3(p)[0].input.sig, c3(p)[1]), ringmod(p, 'right')):
        timer = KernelTimer()
        got = render_batches(graph, V, position, N, (2, 4), timer=timer, fuse_program=False).rows
        launched = names(timer)
        assert 'biquad_coldstart[lp,env]' in launched or 'adsr_apply' in launched, launched
        assert not any('bus[' in n or n.startswith('voice_program') for n in launched), launched
        ref = R.render_stream(ref_node, position, N, K, V)
        assert maxerr(got, f32(ref)) < tolerance(ref), (position, launched)
