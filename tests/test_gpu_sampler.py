"""The sample-playback node on the GPU: sig_sampler_play against tests/sampler_reference.py bit for bit, the eager node (BlockDriver,
eager pulls) against the batched engine (BatchRenderer) bit for bit, and every route against a float64 chain of oracle.chain_ref plus
sampler_reference.

Bars.  The formula has no transcendental and the library is built with contraction off, so the kernel's float64 output equals the
reference bit for bit (NaN where the reference has NaN) and its float32 output equals float32(reference) bit for bit: no tolerance.
Under fuse=False the batched engine launches the same kernels on the same stored float32 rows as the eager path, so the two are
bit-equal.  Against the float64 oracle chain every route is held to the project's bound, max|float32 - oracle| <= 1e-6 * max(1,
max|oracle|): the tables stay within +-1, so the sampler's own float32 rounding is at most 2^-25 = 3e-8, and what follows it (an
envelope <= 1, a Butterworth low-pass, a bus with gains that sum to <= 1) is what the other nodes' tests already hold to that bound;
the oracle's own float32 rounding is asserted to stay under it on the host.

Shapes.  V crosses a wave (1, 3, 64, 70, 130); N in {16, 128}, K in {1, 3}: 384 rows cross the kernel's 32-row waves and 128-row
workgroups and every block boundary falls inside a wave or on its edge; positions 0, 37 and one hour; tables (2, 1), (5, 3) and
(1000, 2).  The per-voice controls put a trigger inside a block, the recording's end inside a block, one voice in the future, one NaN
ratio, and cycle through ratios 0, 0.5, 1, 1.5, 2.75, -1.  The references are computed once per shape and shared by the dtypes."""
import functools

import numpy as np
import pytest
import torch

from gpu_helpers import dev, gpu_ready, render_batches, tolerance
from helpers import HOUR, RATE, f32, fix, maxerr, render
import sampler_reference as SR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    gpu_ready()


def table_dev(table):
    """the device layout: float32 (W, T), every recording contiguous"""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(table, dtype=np.float32).T)).to('cuda:0')


def same(got, want):
    """bit for bit: the same NaN positions, the same bit patterns elsewhere"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    nan = np.isnan(want)
    bits = np.uint64 if got.dtype == np.float64 else np.uint32
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(bits), want[~nan].view(bits)))


RATIOS = [1.0, 0.5, 2.0, 1.5, 2.75, 0.0, -1.0]
TABLES = [(2, 1), (5, 3), (1000, 2)]


def controls(rng, blocks, V, pos, N, K, T, W):
    """(ratio, offset, gate_on, select) rows (blocks, V): voice v takes the next case of each list, so V = 1 takes the first and V >= 7
    all of them; per block the lists are shifted"""
    rows = N * K
    # the trigger, in frames after `pos`: so that the recording ends in the middle of the launch at ratio 1 (voice 0 of block 0 has that
    # ratio), inside block 0, just before the launch, far in the future, at the launch's first frame, in the last block, long ago
    gates = [-(T - 1) + rows / 2 + 0.5, 5.25, -3.0, 10.0 * rows + 7, 0.0, rows - 3.0, -50.0 * T]
    offsets = [0.0, 0.5, 1.25, T - 2.0, -1.0, T - 1.0, 0.75]
    r = np.array([[RATIOS[(v + 2 * b) % 7] for v in range(V)] for b in range(blocks)])
    g = np.array([[(pos + gates[(v + 3 * b) % 7]) / RATE for v in range(V)] for b in range(blocks)])
    o = np.array([[offsets[(v // 7 + b) % 7] for v in range(V)] for b in range(blocks)])
    s = rng.uniform(-0.5, W + 0.5, (blocks, V))
    r[:, 1::5] += rng.uniform(0, 0.3, r[:, 1::5].shape)                        # fractions on some voices
    if V > 1:
        r[:, V // 2] = np.nan                                                  # the NaN ratio: ONE voice
        g[:, V // 2] = (pos - 3.0) / RATE                                      # ... that has been triggered
    if V > 3:
        g[:, 3] = (pos + 10.0 * rows + 7) / RATE                               # one voice gated in the future, in every block
    return r, o, g, s


@functools.lru_cache(maxsize=None)
def kernel_case(V, N, K, pos, T, W, loop, per_block):
    """(table, (ratio, offset, gate_on, select), (loop_start, loop_end), float64 reference): computed once, read-only"""
    rng = np.random.default_rng(V * 1000 + N * 10 + K + pos % 1000 + T)
    table = rng.uniform(-1, 1, (T, W)).astype(np.float32).astype(np.float64)
    rows = controls(rng, K if per_block else 1, V, pos, N, K, T, W)
    bounds = ((0, T) if T < 5 else (1, T - 1)) if loop else (0, 0)
    want = SR.sampler(table, pos, N, *rows, *bounds, rate=RATE, blocks=K)
    for a in (table, want) + rows:
        a.setflags(write=False)
    return table, rows, bounds, want


@pytest.mark.parametrize('pos', [0, 37, HOUR])
@pytest.mark.parametrize('V', [1, 3, 64, 70, 130])
def test_sampler_play_matches_the_reference_bit_for_bit(V, pos):
    """every N, K, table, loop, control form and out dtype at one (V, position); outputs are padded and the padding must stay untouched"""
    from signals_amd import _native
    for N in (16, 128):
        for K in (1, 3):
            for T, W in TABLES:
                tab = None
                for loop in (False, True):
                    for per_block in (False, True):
                        table, rows, bounds, want = kernel_case(V, N, K, pos, T, W, loop, per_block)
                        tab = table_dev(table) if tab is None else tab        # (one table per (V, N, K, pos, T): the seed has no more in it)
                        if V > 1:
                            assert np.isnan(want[:, V // 2]).all() and not np.isnan(np.delete(want, V // 2, axis=1)).any()   # that voice alone
                        if V > 3:
                            assert not want[:, 3].any()                        # gated in the future
                        ctl = [dev(r) for r in rows]
                        for t_out, cast in ((torch.float64, lambda a: a), (torch.float32, f32)):
                            obuf = torch.full((N * K, V + 3), 7.0, dtype=t_out, device='cuda:0')
                            _native.sampler_play(pos, RATE, *ctl, tab, *bounds, obuf[:, :V], rows_per_param=N if per_block else 0)
                            assert bool((obuf[:, V:] == 7.0).all()), (V, pos, N, K, T)
                            assert same(obuf[:, :V].cpu().numpy(), cast(want)), (V, pos, N, K, T, W, loop, per_block, t_out)


def test_the_trigger_and_the_end_fall_inside_a_block():
    """what the shared cases rely on, looked at directly: voice 1 starts 5.25 frames into block 0 and voice 0's recording ends in the
    middle of the launch, both inside a block of 128"""
    table, rows, bounds, want = kernel_case(70, 128, 3, 37, 1000, 2, False, False)
    assert not want[:6, 1].any() and want[6:40, 1].all()                       # silent up to the trigger, then sound
    last = np.flatnonzero(want[:, 0])[-1]
    assert want[:last, 0].all() and 128 < last < 255 and not want[last + 1:, 0].any()      # the end inside block 1


def test_block_rate_reads_unplugged_ports_and_broadcast_rows():
    from signals_amd import _native
    rng = np.random.default_rng(31)
    T, W, V, N, K = 1000, 2, 70, 128, 9
    table = rng.uniform(-1, 1, (T, W))
    tab = table_dev(table)
    r, o, g, s = controls(rng, K, V, 4096, N, K, T, W)
    # step = N, one output row per block, its own control row: what a control port would see
    out = torch.empty((K, V), dtype=torch.float64, device='cuda:0')
    _native.sampler_play(4096, RATE, dev(r), dev(o), dev(g), dev(s), tab, 0, 0, out, step=N, rows_per_param=1)
    assert same(out.cpu().numpy(), SR.sampler(table, 4096, 1, r, o, g, s, rate=RATE, blocks=K, step=N))
    _native.sampler_play(4096, RATE, dev(r), dev(o), dev(g), dev(s), tab, 100, 900, out, step=N, rows_per_param=1)
    assert same(out.cpu().numpy(), SR.sampler(table, 4096, 1, r, o, g, s, 100, 900, rate=RATE, blocks=K, step=N))
    # every port unplugged: u = 0 for ever, the first frame of column 0 held; ratio alone: the recording from frame 0
    out = torch.empty((N * 3, V), dtype=torch.float32, device='cuda:0')
    _native.sampler_play(0, RATE, None, None, None, None, tab, 0, 0, out)
    assert same(out.cpu().numpy(), np.full((N * 3, V), np.float32(table[0, 0])))
    _native.sampler_play(0, RATE, dev([[1.0]]), None, None, None, tab, 0, 0, out[:, :1])
    assert same(out[:, :1].cpu().numpy(), f32(SR.sampler(table, 0, N * 3, [[1.0]], rate=RATE)))
    # one-column rows broadcast over the voices beside per-voice rows; the identity in float32
    _native.sampler_play(0, RATE, dev([[1.0]]), None, dev([[0.0]]), dev(s[:1]), tab, 0, 0, out)
    held = table.astype(np.float32)
    w = SR.column(s[:1], W)[0]
    assert same(out.cpu().numpy(), held[:N * 3][:, w])


def test_wrapper_refusals():
    from signals_amd import _native
    out = torch.zeros((256, 8), dtype=torch.float32, device='cuda:0')
    tab = table_dev(np.zeros((10, 2)))
    with pytest.raises(_native.NativeError, match='hipError_t 1'):
        _native.sampler_play(0, RATE, dev([[1.0]]), None, None, None, tab, 5, 11, out)       # a loop past the table
    with pytest.raises(_native.NativeError, match='hipError_t 1'):
        _native.sampler_play(0, RATE, dev([[1.0]]), None, None, None, tab, 5, 5, out)
    with pytest.raises(_native.NativeError, match='sampler table'):
        _native.sampler_play(0, RATE, dev([[1.0]]), None, None, None, tab.T, 0, 0, out)      # not contiguous
    with pytest.raises(_native.NativeError, match='sampler table'):
        _native.sampler_play(0, RATE, dev([[1.0]]), None, None, None, tab[:, :1].contiguous(), 0, 0, out)
    with pytest.raises(_native.NativeError, match='ratio has 3 channels'):
        _native.sampler_play(0, RATE, dev(np.ones((1, 3))), None, None, None, tab, 0, 0, out)
    assert not out.any()


# ---------------------------------------------------------------------------------------------- graphs: eager against batched against the oracle
GV = 70
TABLE = SR.burst(1000, 4, seed=4)
LOOP = (200, 900)


def draw():
    rng = np.random.default_rng(23)
    th = rng.uniform(0, np.pi / 2, GV)
    gate = np.where(np.arange(GV) % 2 == 0, rng.uniform(0, 0.004, GV), rng.uniform(0.168, 0.172, GV))[None, :]   # inside the first batch; inside the fresh one at 8192
    gate[0, 5] = 10.0                                                          # one voice gated in the future
    return dict(ratio=rng.uniform(0.5, 2.0, (1, GV)), offset=rng.uniform(0, 50, (1, GV)), gate=gate, select=rng.uniform(0, 4, (1, GV)),
                cut=rng.uniform(200, 8000, (1, GV)), pan=np.stack([np.cos(th), np.sin(th)]) / GV)


def sampler_node(p, loop):
    from signals_amd.chain import ext
    s = ext.Sampler()
    s.get_state().table = TABLE
    if loop:
        s.get_state().loop_end, s.get_state().loop_start = LOOP[1], LOOP[0]
    s.ratio, s.offset, s.gate_on, s.select = fix(p['ratio']), fix(p['offset']), fix(p['gate']), fix(p['select'])
    return s


def graph(which, p):
    """(GPU node, oracle node, rendered width) of one voice shape"""
    from oracle import chain_ref as R
    from signals_amd.chain import ext, fx
    RS = SR.oracle_node()
    loop = which in ('enveloped', 'enveloped_bus')

    def ref_sampler():
        return RS(TABLE, R.Fixed(p['ratio']), R.Fixed(p['offset']), R.Fixed(p['gate']), R.Fixed(p['select']), *(LOOP if loop else (0, 0)))
    env = dict(attack=[[0.001]], decay=[[0.01]], sustain=[[0.6]], release=[[0.02]], gate_on=p['gate'], gate_off=p['gate'] + 0.05)

    def enveloped():
        e = ext.ADSR()
        for name, value in env.items():
            setattr(e, name, fix(value))
        rm = fx.RingMod(); rm.left = sampler_node(p, loop); rm.right = e
        return rm, R.Binary('RingMod', ref_sampler(), R.Adsr(**env))
    if which == 'sampler':
        return sampler_node(p, loop), ref_sampler(), GV
    if which == 'enveloped':
        return (*enveloped(), GV)
    if which == 'lowpass':
        f = fx.LowPass(); f.input = sampler_node(p, loop); f.cutoff = fix(p['cut'])
        return f, R.Filter('lp', ref_sampler(), R.Fixed(p['cut'])), GV
    if which == 'enveloped_bus':
        top, ref = enveloped()
        b = ext.SumBus(); b.input = top; b.get_state().gains = np.ascontiguousarray(p['pan'])
        return b, R.SumBus(ref, p['pan']), 2
    raise KeyError(which)


FUSED = ('fused', 'latency', 'cascade', 'steady', 'walk', 'biquad_bus', 'biquad_coldstart_env', 'voice_program')
CASES = [('sampler', 128), ('enveloped', 128), ('lowpass', 128), ('lowpass', 64), ('enveloped_bus', 128)]


def eager_rows(top, C, pos, N, blocks):
    """sequential eager pulls through a BlockDriver: the reference-shaped path"""
    from signals_amd.chain.driver import BlockDriver
    d = BlockDriver(RATE, N)
    d.get_state().channels = C
    d.input = top
    d.frame_position = pos
    rows = np.concatenate([d.pull(eager=True) for _ in range(blocks)])
    del d.input
    return rows


def batched_rows(top, C, pos, N, ks, **kw):
    return render_batches(top, C, pos, N, ks, names=True, **kw)[:2]


def bound(want):
    return tolerance(want)


def check_routes(which, p, want, pos, N, ks):
    """the eager path and the batched engine under fuse=False: bit-equal; those two, the default route and fuse_program='always':
    within the bound of the oracle; the sampler itself one sig_sampler_play launch per batch on each, no fused kernel, no voice program"""
    assert np.abs(TABLE).max() <= 1.0
    assert maxerr(f32(want), want) <= bound(want)                              # the oracle's own float32 rounding stays under the bound
    C = want.shape[1]
    eager = eager_rows(graph(which, p)[0], C, pos, N, sum(ks))
    assert eager.dtype == np.float32 and maxerr(eager, want) <= bound(want), (which, N, maxerr(eager, want))
    for kw in ({'fuse': False}, {}, {'fuse_program': 'always'}):
        got, names = batched_rows(graph(which, p)[0], C, pos, N, ks, **kw)
        label = 'sampler_play[Loop]' if which.startswith('enveloped') else 'sampler_play[OneShot]'
        assert {n for n in names if n.startswith('sampler_play')} == {label}, names
        assert not {n for n in names if any(w in n for w in FUSED)}, (kw, names)
        assert got.dtype == np.float32 and maxerr(got, want) <= bound(want), (which, N, kw, maxerr(got, want))
        if kw == {'fuse': False}:
            assert same(got, eager), (which, N, maxerr(got, eager))


@pytest.mark.parametrize('which,N', CASES)
def test_batched_equals_eager_and_every_route_meets_the_oracle(which, N):
    """from position 0, batches of 3 + 2 blocks: the second continues the first"""
    from oracle import chain_ref as R
    p = draw()
    top, ref, C = graph(which, p)
    want = R.render_stream(ref, 0, N, 5, C)
    check_routes(which, p, want, 0, N, (3, 2))
    assert np.abs(want).max() > (0.003 if which == 'enveloped_bus' else 0.2)   # (the graphs sound)


@pytest.mark.parametrize('which,N', CASES)
def test_a_fresh_batch_at_position_8192(which, N):
    """a fresh renderer and a fresh graph at 8192: a pure function of the position, so nothing in front is needed but a filter's
    100 context rows, which are simply rendered; the odd voices trigger inside this batch"""
    from oracle import chain_ref as R
    p, pos = draw(), 8192
    top, ref, C = graph(which, p)
    want = R.render_stream(ref, pos, N, 3, C)
    check_routes(which, p, want, pos, N, (3,))
    assert np.abs(want).max() > (0.003 if which == 'enveloped_bus' else 0.2)


@pytest.mark.parametrize('pos', [0, 37, 8192])
def test_one_frame_requests_are_answered_in_float64(pos):
    p = draw()
    for loop in (False, True):
        got = render(sampler_node(p, loop), pos, 1, GV)
        assert got.shape == (1, GV) and got.dtype == np.float64
        want = SR.sampler(TABLE, pos, 1, p['ratio'], p['offset'], p['gate'], p['select'], *(LOOP if loop else (0, 0)), rate=RATE)
        assert same(got, want)


def test_a_sampler_in_a_control_path_renders_eagerly():
    """the batch refuses with the reason; the eager path serves the one-frame requests and meets the oracle"""
    from oracle import chain_ref as R
    from signals_amd.chain import fx
    from signals_amd.engine import BatchRenderer, NotBatchable
    from helpers import mkosc
    p = draw()
    RS = SR.oracle_node()

    def voice():
        hz = fx.Mix(); hz.left = sampler_node(p, True); hz.right = fix(p['cut']); hz.mix = fix([[0.05]])      # the cutoffs, moved by the recording
        f = fx.LowPass(); f.input = mkosc('Sawtooth', p['cut'] / 4); f.cutoff = hz
        return f
    with pytest.raises(NotBatchable, match='Sampler in a control path: a sampler has no block-rate'):
        BatchRenderer(voice(), GV, RATE).render(0, 256, 2)
    ref = R.Filter('lp', R.Osc('Sawtooth', R.Fixed(p['cut'] / 4)),
                   R.Binary('Mix', RS(TABLE, R.Fixed(p['ratio']), R.Fixed(p['offset']), R.Fixed(p['gate']), R.Fixed(p['select']), *LOOP),
                            R.Fixed(p['cut']), R.Fixed([[0.05]])))
    eager = eager_rows(voice(), GV, 0, 256, 2)
    assert maxerr(eager, R.render_stream(ref, 0, 256, 2, GV)) < 1e-6
