"""White noise on every route that generates it, against the CPU definition (oracle/chain_ref.py: white): sig_white_noise
(noise.hip), the SIG_CTL_NOISE instruction of the control programs (control_program.hip, interpreter and specialised) and the
SIG_VP_NOISE instruction of the voice programs (voice_program.hip, interpreter and specialised).  A noise sample -- and a
noise sample times a float64 gain, rounded once to float32 -- is exact, so the bar there is array_equal; where a filter
follows it is the project's own, maxerr <= 1e-6 * max(1, max |ref|).  The reference draws np.random.rand from the global
unseeded generator (noise.py:22-23): against it the parity stays statistical (tests/test_gpu_engine.py)."""
import functools

import numpy as np
import pytest
import torch

from helpers import HOUR, RATE, Probe, f32, fix, loc, maxerr, mkosc
import gpu_helpers as GH
from gpu_helpers import render_batches
import test_gpu_filtered_control as FC
import test_gpu_voice_program as VP

pytestmark = pytest.mark.gpu

SEEDS = (0, 1, 12345, 2 ** 32, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1)
CHANNELS = (1, 2, 3, 63, 64, 65, 1000)
POSITIONS = (0, 1, 2 ** 31 - 40, 2 ** 32 - 40, HOUR, 2 ** 40 - 17)


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    from signals_amd import _native, specialise
    GH.gpu_ready()
    yield
    torch.cuda.synchronize()
    specialise.forget()                                                       # (attached kernels and the tuning are process-wide)
    _native.voice_program_use_attached(True)
    _native.set_voice_program_tuning()


def need_hipcc():
    from signals_amd import specialise
    if specialise.hipcc() is None:
        pytest.skip('no hipcc: the specialised kernels cannot be built')


def close(got, ref, what):
    """the `close` of tests/gpu_helpers.py; returns max |ref|"""
    GH.close(got, ref, what)
    return float(np.max(np.abs(ref)))


def names(timer):
    torch.cuda.synchronize()
    return set(timer.summary())


def white_node(V, seed):
    from signals_amd.chain import noise
    w = noise.White()
    w.get_state().channels = V
    w.get_state().seed = seed
    return w


def dev(a):
    return VP.dev(a)


# ================================================================ sig_white_noise
def native_white(seed, pos, rows, C, dtype):
    from signals_amd import _native
    out = torch.full((rows, C), float('nan'), dtype=dtype, device='cuda')
    _native.white_noise(seed, pos, out)
    return out.cpu().numpy()


@pytest.mark.parametrize('shift', [(0, 0), (3, 2), (5, 4)])
def test_white_noise_kernel_bit_for_bit(shift):
    """every seed with a channel count and a position (three pairings of the lists), 96 rows -- so the blocks at 2^31 - 40 and
    2^32 - 40 straddle those frames --, float32 and float64 stores"""
    from oracle import chain_ref as R
    for i, seed in enumerate(SEEDS):
        C, pos = CHANNELS[(i + shift[0]) % len(CHANNELS)], POSITIONS[(i + shift[1]) % len(POSITIONS)]
        want = R.white(seed, pos, 96, C)
        for dtype in (torch.float32, torch.float64):
            got = native_white(seed, pos, 96, C, dtype)
            assert got.dtype == (np.float32 if dtype == torch.float32 else np.float64)
            assert np.array_equal(got, want), (seed, pos, C, dtype)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('C', [1, 65])
def test_white_noise_into_a_padded_output(dtype, C):
    """a column slice of a wider tensor (out_ld > channels): the slice is the oracle's block, the padding keeps its sentinel"""
    from oracle import chain_ref as R
    from signals_amd import _native
    rows, ld, at, seed, pos = 200, 80, 5, 2 ** 63 + 11, 2 ** 32 - 100
    wide = torch.full((rows, ld), -7.0, dtype=dtype, device='cuda')
    view = wide[:, at:at + C]
    assert view.stride(0) == ld
    _native.white_noise(seed, pos, view)
    got = wide.cpu().numpy()
    assert np.array_equal(got[:, at:at + C], R.white(seed, pos, rows, C))
    assert np.all(got[:, :at] == -7.0) and np.all(got[:, at + C:] == -7.0)


@pytest.mark.parametrize('rows,C,seed,pos', [(4100, 4096, 12345, 2 ** 31 - 1000), (2050, 4097, 2 ** 64 - 1, 2 ** 32 - 1000)])
def test_white_noise_launch_beyond_one_trip_of_the_grid_stride_loop(rows, C, seed, pos):
    """more than 2048 * 16 * 256 = 8 388 608 elements: the kernel's loop iterates (16.8 M and 8.4 M samples, an even and an odd
    channel count)"""
    from oracle import chain_ref as R
    assert rows * C > 2048 * 16 * 256
    got = native_white(seed, pos, rows, C, torch.float32)
    assert np.array_equal(got, R.white(seed, pos, rows, C).astype(np.float32))


@pytest.mark.parametrize('V,seed', [(1, 2 ** 63), (3, 2 ** 64 - 1), (64, 12345), (65, 2 ** 32)])
def test_white_node_eager_replies(V, seed):
    """the node through the pull protocol: float32 blocks and float64 one-frame (block-rate) replies, both the oracle's values"""
    from oracle import chain_ref as R
    p = Probe()
    p.input = white_node(V, seed)
    for q in POSITIONS:
        one = p.input.request(loc(q, 1, V))
        assert one.dtype == torch.float64 and tuple(one.shape) == (1, V)
        assert np.array_equal(one.cpu().numpy(), R.white(seed, q, 1, V)), (V, q)
        block = p.input.request(loc(q + 7, 80, V))
        assert block.dtype == torch.float32 and np.array_equal(block.cpu().numpy(), R.white(seed, q + 7, 80, V)), (V, q)
    del p.input


# ================================================================ control programs: SIG_CTL_NOISE
def control_renderers(node, V, timer=None):
    """the interpreter's renderer and, where hipcc is there, the specialised one"""
    from signals_amd import specialise
    from signals_amd.engine import BatchRenderer
    out = {'interpreter': BatchRenderer(node, V, RATE)}
    if specialise.hipcc() is not None:
        out['specialised'] = BatchRenderer(node, V, RATE, specialise=True, timer=timer)
    return out


@pytest.mark.parametrize('V,seed', [(1, 2 ** 63), (3, 2 ** 64 - 1), (8, 12345)])
def test_control_rows_of_a_bare_white(V, seed):
    """White as a control input: K rows at pos + b N, the front row, a batch continued across two calls -- the seed travels in
    the instruction's pointer field"""
    from oracle import chain_ref as R
    from signals_amd.chain import fx
    from signals_amd.engine import KernelTimer, _Batch
    N = 160
    row = lambda q: R.white(seed, q, 1, V)
    timer = KernelTimer()
    g = fx.Gain(); g.left = mkosc('Sine', [[440.0] * V]); g.right = white_node(V, seed)
    renderers = control_renderers(g, V, timer)
    for mode, r in renderers.items():
        for pos in (0, 1, 2 ** 31 - 2 * N, 2 ** 32 - 2 * N - 3, HOUR, 2 ** 40 - 17):
            got = np.concatenate([FC.engine_rows(r, g.right.sig, pos, N, 5, V),
                                  FC.engine_rows(r, g.right.sig, pos + 5 * N, N, 4, V, continuing=True)])
            want = np.concatenate([row(pos + b * N) for b in range(9)])
            assert got.dtype == np.float64 and np.array_equal(got, want), (mode, pos)
            if pos >= N:
                rows, fronts = _Batch(r, pos, N, 5, False)._control_many([g.right], pos - N, channels=V)
                assert np.array_equal(fronts[0].cpu().numpy(), row(pos - N)), (mode, pos)
                assert np.array_equal(rows[0].cpu().numpy(), want[:5]), (mode, pos)
    if 'specialised' in renderers:
        assert 'control_program[block-rate]*specialised' in names(timer), names(timer)


def drift_oracle(V, base, seed=3, cut=1.0):
    from oracle import chain_ref as R
    f = R.Filter('lp', R.White(seed, V), R.Fixed([[cut] * V]))
    return R.Binary('Mix', R.Binary('Gain', f, R.Fixed(0.02 * base)), R.Fixed(base * 0.99 * 2.0), R.Fixed([[0.5]]))


@pytest.mark.parametrize('pos', [0, 37, 100, 101, HOUR])
def test_drift_control_rows_against_the_oracle(pos):
    """drift(V, base) = Mix(Gain(LowPass(White, 1 Hz), 0.02 base), 1.98 base, 0.5) at block rate, a batch continued across two
    calls, against the same graph of oracle nodes within 1e-6 * max |ref|.  max |ref| is the Mix output, 792.0004 at every
    position here (base runs from 100 to 800), while the cold-started 1 Hz filter over at most 101 rows stays below 5.1e-5 and
    moves the Mix output by less than 4.1e-4: this bar, 7.9e-4, says little about the noise itself.  So the same rows are
    read from LowPass(White, 2 kHz) alone as well, max |ref| 0.70 to 0.80, within 1e-6.
    The interpreter and the specialised control program give the same rows bit for bit."""
    from oracle import chain_ref as R
    V, N = 8, 160
    base = np.linspace(100.0, 800.0, V)[None, :]
    positions = [pos + b * N for b in range(9)]
    for what, build, ref in (('drift', lambda: FC.drift(V, base), drift_oracle(V, base)),
                             ('lowpass', lambda: lowpass_white(V, 5, 2000.0)[0], lowpass_white(V, 5, 2000.0)[1])):
        want = np.concatenate([R.render(ref, q, 1, V) for q in positions])
        got = {}
        node = build()
        for mode, r in control_renderers(node, V).items():
            got[mode] = np.concatenate([FC.engine_rows(r, node, pos, N, 5, V), FC.engine_rows(r, node, pos + 5 * N, N, 4, V, continuing=True)])
            scale = close(got[mode], want, (what, mode, pos))
            print(f'{what} at {pos} ({mode}): max |ref| = {scale:.6g}, max err = {maxerr(got[mode], want):.3g}')
        if 'specialised' in got:
            assert np.array_equal(got['interpreter'], got['specialised']), (what, pos)


def lowpass_white(V, seed, cut, ftype='LowPass'):
    """Filter(White) with one cutoff for every column: (GPU node, oracle node)"""
    from oracle import chain_ref as R
    from signals_amd.chain import fx
    f = getattr(fx, ftype)(); f.input = white_node(V, seed); f.cutoff = fix([[cut] * V])
    return f, R.Filter({'LowPass': 'lp', 'HighPass': 'hp'}[ftype], R.White(seed, V), R.Fixed([[cut] * V]))


# ================================================================ voice programs: SIG_VP_NOISE
NOISE_GAIN = [('Noise', 0, 0, 0, 0), ('Gain', 0, 0, 0, 0)]


@pytest.mark.parametrize('V', [2, 3, 5, 64, 66])
def test_noise_gain_through_the_c_abi(V):
    """Noise -> Gain through sig_voice_program at forced one and two voices per lane (two: even voice counts when stored, any
    under a bus) and several blocks per lane: float32(white * gain) exactly; the second seed slot; under a bus whose two
    channels each pick one voice (an exact sum) so that odd voice counts run at two voices per lane too"""
    from oracle import chain_ref as R
    from signals_amd import _native
    N, K = 128, 3
    gain = np.random.default_rng(V).uniform(0.2, 1.0, (1, V))
    pick = np.zeros((2, V)); pick[0, V - 1] = 1.0; pick[1, V // 2] = 1.0
    try:
        for (vpt, span), seed, pos in (((1, 1), 12345, 777), ((2, 1), 2 ** 64 - 1, 2 ** 32 - 200), ((1, 4), 2 ** 63, 2 ** 31 - 100),
                                       ((2, 2), 2 ** 32, HOUR)):
            _native.set_voice_program_tuning(vpt, span)
            want = R.white(seed, pos, K * N, V)
            got = VP.launch(NOISE_GAIN, [], [dev(gain)], [], 0, 0, pos, N, K, V, seeds=(seed, seed ^ 1))
            assert np.array_equal(got, f32(want * gain)), (V, vpt, span)
            slot1 = VP.launch([('Noise', 0, 1, 0, 0), ('Gain', 0, 0, 0, 0)], [], [dev(gain)], [], 0, 0, pos, N, K, V, seeds=(seed ^ 1, seed))
            assert np.array_equal(slot1, f32(want * gain)), (V, vpt, span)
            bus = VP.launch([('Noise', 0, 0, 0, 0)], [], [], [], 0, 0, pos, N, K, V, bus=pick, seeds=(seed, 0))
            assert np.array_equal(bus, f32(want[:, [V - 1, V // 2]])), (V, vpt, span)
    finally:
        _native.set_voice_program_tuning()


def gained_white(V, seed, gain):
    from oracle import chain_ref as R
    from signals_amd.chain import fx
    g = fx.Gain(); g.left = white_node(V, seed); g.right = fix(gain)
    return g, R.Binary('Gain', R.White(seed, V), R.Fixed(gain))


@pytest.mark.parametrize('V', [2, 3, 5, 64, 66])
def test_noise_gain_through_the_engine(V):
    """Gain(White) as a voice program of the batched engine: the interpreter at forced one and two voices per lane, the
    specialised kernel at the geometry's own choice and at four voices per lane where the geometry offers it (a voice count
    that is a multiple of four): float32(white * gain) exactly"""
    from oracle import chain_ref as R
    from signals_amd import _native, specialise
    from signals_amd.engine import BatchRenderer, KernelTimer
    N, K, seed, pos = 128, 4, 2 ** 63 + 5, 2 ** 32 - 2 * 128 - 1
    gain = np.random.default_rng(V).uniform(0.2, 1.0, (1, V))
    want = f32(R.white(seed, pos, K * N, V) * gain)
    try:
        for vpl in (1, 2):
            _native.set_voice_program_tuning(vpl, 1)
            timer = KernelTimer()
            got = BatchRenderer(gained_white(V, seed, gain)[0], V, RATE, fuse_program='always', timer=timer).render(pos, N, K).cpu().numpy()
            assert any(n.startswith('voice_program[Noise,Gain]') for n in names(timer)), names(timer)
            assert np.array_equal(got, want), (V, vpl)
        if specialise.hipcc() is not None:
            for vpl in (0, 4):
                _native.set_voice_program_tuning(vpl, 0)
                timer = KernelTimer()
                r = BatchRenderer(gained_white(V, seed, gain)[0], V, RATE, fuse_program='always', specialise=True, timer=timer)
                got = r.render(pos, N, K).cpu().numpy()
                assert 'voice_program[Noise,Gain]*specialised' in names(timer), names(timer)
                assert np.array_equal(got, want), (V, vpl)
            if V % 4 == 0:
                assert _native.voice_program_geometry(V, N, K, 100, 0, 0, 4, specialised=True)[0] == 4      # (still forced to four)
    finally:
        _native.set_voice_program_tuning()


def two_whites(V, s0, s1, m):
    from oracle import chain_ref as R
    from signals_amd.chain import fx
    x = fx.Mix(); x.left = white_node(V, s0); x.right = white_node(V, s1); x.mix = fix(m)
    return x, R.Binary('Mix', R.White(s0, V), R.White(s1, V), R.Fixed(m))


@pytest.mark.parametrize('mode', ['per-node', 'always', 'specialise'])
def test_two_whites_in_one_voice_read_both_seed_slots(mode):
    """Mix(White(s0), White(s1), m) with m in [0.1, 0.4]: a swapped or ignored second seed is off by more than 0.1"""
    from oracle import chain_ref as R
    from signals_amd.engine import BatchRenderer, KernelTimer
    if mode == 'specialise':
        need_hipcc()
    kw = {'per-node': {'fuse': False}, 'always': {'fuse_program': 'always'}, 'specialise': {'fuse_program': 'always', 'specialise': True}}[mode]
    V, N, K, pos, s0, s1 = 6, 128, 3, 4800, 2 ** 64 - 1, 2 ** 63
    m = np.linspace(0.1, 0.4, V)[None, :]
    node, ref = two_whites(V, s0, s1, m)
    want = R.render_stream(ref, pos, N, K, V)
    for wrong in (two_whites(V, s1, s0, m)[1], two_whites(V, s0, s0, m)[1], two_whites(V, s1, s1, m)[1]):
        assert maxerr(R.render_stream(wrong, pos, N, K, V), want) > 0.1
    timer = KernelTimer()
    got = BatchRenderer(node, V, RATE, timer=timer, **kw).render(pos, N, K).cpu().numpy()
    launched = names(timer)
    if mode == 'per-node':
        assert not any(n.startswith('voice_program') for n in launched), launched
    else:
        assert any(n.startswith('voice_program[Noise,Save,Noise,Mix]') for n in launched), launched
        assert mode != 'specialise' or any(n.endswith('*specialised') for n in launched), launched
    close(got, want, mode)


def test_a_third_white_leaves_the_program_route():
    """two seed slots: a voice with three White nodes is no voice program (_NoProgram); the engine renders it through the
    per-node schedule, and that equals the oracle"""
    from oracle import chain_ref as R
    from signals_amd.chain import fx
    from signals_amd.engine import BatchRenderer, KernelTimer, _Batch, _NoProgram, _VoiceProgram
    V, N, K, pos = 6, 128, 3, 4800
    m = np.linspace(0.1, 0.4, V)[None, :]
    pair, ref_pair = two_whites(V, 11, 12, m)
    top = fx.RingMod(); top.left = pair; top.right = white_node(V, 13)
    ref = R.Binary('RingMod', ref_pair, R.White(13, V))
    timer = KernelTimer()
    r = BatchRenderer(top, V, RATE, fuse_program='always', timer=timer)
    with pytest.raises(_NoProgram):
        _VoiceProgram(_Batch(r, pos, N, K, False), top, V)
    got = r.render(pos, N, K).cpu().numpy()
    assert not any(n.count('Noise') > 2 for n in names(timer)), names(timer)
    assert 'white_noise' in names(timer), names(timer)
    close(got, R.render_stream(ref, pos, N, K, V), 'three whites')


@pytest.mark.parametrize('N', [256, 300, 16, 64, 100])
@pytest.mark.parametrize('ftype', ['LowPass', 'HighPass'])
def test_filtered_white_in_the_voice_program(ftype, N):
    """LowPass / HighPass(White): blocks longer than the filter context and no longer than it (the virtual-block layout, whose
    context rows are noise frames in front of the block), a fresh graph at position 0 continued by a second batch, a fresh
    graph deep in the stream continued likewise -- interpreter and specialised kernel against the oracle's sequential blocks"""
    from oracle import chain_ref as R
    from signals_amd import specialise
    from signals_amd.engine import KernelTimer
    V, seed = 6, 2 ** 63 + 9
    cut = np.array([[40.0, 300.0, 1000.0, 3000.0, 9000.0, 15000.0]])

    def build():
        from signals_amd.chain import fx
        f = getattr(fx, ftype)(); f.input = white_node(V, seed); f.cutoff = fix(cut)
        return f, R.Filter({'LowPass': 'lp', 'HighPass': 'hp'}[ftype], R.White(seed, V), R.Fixed(cut))
    modes = [{'fuse_program': 'always'}] + ([{'fuse_program': 'always', 'specialise': True}] if specialise.hipcc() is not None else [])
    for pos in (0, 2 ** 32 - 2 * N - 5):
        want = R.render_stream(build()[1], pos, N, 5, V)
        for kw in modes:
            timer = KernelTimer()
            got = render_batches(build()[0], V, pos, N, (3, 2), timer=timer, **kw).rows
            assert any(n.startswith('voice_program[Noise,Filter]') for n in names(timer)), names(timer)
            assert 'specialise' not in kw or any(n.endswith('*specialised') for n in names(timer)), names(timer)
            close(got, want, (ftype, N, pos, kw))


def test_two_filters_over_white():
    """LowPass(LowPass(White)): depth 2, the inner filter's cached history between batches"""
    from oracle import chain_ref as R
    from signals_amd import specialise
    from signals_amd.chain import fx
    V, N, seed = 5, 256, 77
    c1, c2 = np.array([[30.0, 90.0, 400.0, 2000.0, 8000.0]]), np.array([[5000.0, 60.0, 700.0, 150.0, 12000.0]])

    def build():
        inner = fx.LowPass(); inner.input = white_node(V, seed); inner.cutoff = fix(c1)
        outer = fx.LowPass(); outer.input = inner; outer.cutoff = fix(c2)
        return outer
    want = R.render_stream(R.Filter('lp', R.Filter('lp', R.White(seed, V), R.Fixed(c1)), R.Fixed(c2)), 0, N, 6, V)
    for kw in [{'fuse_program': 'always'}] + ([{'fuse_program': 'always', 'specialise': True}] if specialise.hipcc() is not None else []):
        close(render_batches(build(), V, 0, N, (3, 1, 2), **kw).rows, want, kw)


@pytest.mark.parametrize('mode', ['per-node', 'default', 'always', 'specialise'])
@pytest.mark.parametrize('V', [64, 3])
def test_subtractive_voice_under_a_bus(V, mode):
    """SumBus(RingMod(LowPass(White), ADSR)), mono and stereo with pan gains, on every schedule"""
    from oracle import chain_ref as R
    from signals_amd.chain import ext, fx
    if mode == 'specialise':
        need_hipcc()
    kw = SCHEDULES[mode]
    N, seed = 256, 2 ** 64 - 3
    rng = np.random.default_rng(V)
    cut = rng.uniform(200.0, 8000.0, (1, V))
    env = dict(attack=rng.uniform(0.001, 0.004, (1, V)), decay=rng.uniform(0.002, 0.006, (1, V)), sustain=rng.uniform(0.2, 0.9, (1, V)),
               release=rng.uniform(0.002, 0.01, (1, V)), gate_on=rng.uniform(0.0, 0.003, (1, V)), gate_off=rng.uniform(0.015, 0.03, (1, V)))
    th = rng.uniform(0, np.pi / 2, V)
    pan = np.stack([np.cos(th), np.sin(th)])

    def build(gains):
        f = fx.LowPass(); f.input = white_node(V, seed); f.cutoff = fix(cut)
        a = ext.ADSR()
        for k, v in env.items():
            setattr(a, k, fix(v))
        m = fx.RingMod(); m.left = f; m.right = a
        b = ext.SumBus(); b.input = m
        if gains is not None:
            b.get_state().gains = np.ascontiguousarray(gains)
        return b
    voice = R.render_stream(R.Binary('RingMod', R.Filter('lp', R.White(seed, V), R.Fixed(cut)), R.Adsr(**env)), 0, N, 7, V)
    for gains in (None, pan):
        want = R.sum_bus(voice, gains)
        got = render_batches(build(gains), want.shape[1], 0, N, (4, 3), **kw).rows
        close(got, want, (V, mode, gains is None))


# ================================================================ whole graphs across schedules
SCHEDULES = {'per-node': {'fuse': False}, 'default': {}, 'always': {'fuse_program': 'always'}, 'specialise': {'specialise': True}}


def graph_b_oracle(V, p, bus=False):
    """the oracle twin of tests/test_gpu_filtered_control.py: graph_b"""
    from oracle import chain_ref as R
    s = R.Osc('Sine', drift_oracle(V, p['hertz']), R.Fixed(p['phase']))
    g = R.Binary('Gain', R.Filter('lp', s, R.Fixed(p['cut'])), R.Fixed(p['gain']))
    return R.SumBus(g, p['pan']) if bus else g


def noise_gate(V, P):
    """the noise_gate graph of tests/test_gpu_specialise.py, Gain(RingMod(HighPass(Sawtooth), White), g): (GPU node, oracle node)"""
    from oracle import chain_ref as R
    from signals_amd.chain import fx
    f = fx.HighPass(); f.input = mkosc('Sawtooth', P['hertz']); f.cutoff = fix(P['cut'])
    m = fx.RingMod(); m.left = f; m.right = white_node(V, 2 ** 63 + 1)
    g = fx.Gain(); g.left = m; g.right = fix(P['gain'])
    ref = R.Binary('Gain', R.Binary('RingMod', R.Filter('hp', R.Osc('Sawtooth', R.Fixed(P['hertz'])), R.Fixed(P['cut'])),
                                    R.White(2 ** 63 + 1, V)), R.Fixed(P['gain']))
    return g, ref


@functools.lru_cache(maxsize=None)
def whole_graph(name, V):
    """(builder of the GPU graph, request channels, the oracle's (4 + 3) blocks of 256)"""
    from oracle import chain_ref as R
    p = FC.draw(V, seed=11)
    if name == 'noise_gate':
        build, ref, C = (lambda: noise_gate(V, p)[0]), noise_gate(V, p)[1], V
    else:
        bus = name == 'b_bus'
        build, ref, C = (lambda: FC.graph_b(V, p, bus=bus)), graph_b_oracle(V, p, bus=bus), 2 if bus else V
    return build, C, R.render_stream(ref, 0, 256, 7, C)


@pytest.mark.parametrize('mode', list(SCHEDULES))
@pytest.mark.parametrize('V', [64, 3])
@pytest.mark.parametrize('name', ['b', 'b_bus', 'noise_gate'])
def test_whole_graphs_against_the_oracle(name, V, mode):
    """graph_b, graph_b under a bus (smoothed random drift on `hertz`: White inside a control path) and the noise gate (White
    at frame rate), one kernel per node, the default schedule, the voice program and the specialised kernels, (4, 3) blocks of
    256 -- against oracle nodes, where the existing tests compare them with the eager GPU render"""
    if mode == 'specialise':
        need_hipcc()
    build, C, want = whole_graph(name, V)
    got = render_batches(build(), C, 0, 256, (4, 3), **SCHEDULES[mode]).rows
    close(got, want, (name, V, mode))
