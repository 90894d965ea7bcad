"""The modal resonator bank on the GPU: sig_modal_bank against the numpy restatement (tests/modal_reference.py) over the shared case
table, the entry's refusals, launch-geometry independence, the eager node against the kernel and against the batched engine bit for
bit, one-frame requests, and a table edited or replaced between renders.

Tolerance.  Because of exp and sin the kernel is held to a bound, not to bits: every sample -- none is left out -- within
1e-6 * max(1, A) of the float64 restatement, A the largest set's sum of |a|.  NaN placement is compared exactly, the rows before a
strike and the voices with every mode dropped to exactly 0.0.  The largest error seen is printed per case.  The restatement's rows
are rendered once per case and shared."""
import functools

import numpy as np
import pytest
import torch

from gpu_helpers import dev, gpu_ready, render_batches, tolerance
from helpers import RATE, f32, fix, maxerr, mkosc, render, stream
import modal_reference as MR

pytestmark = pytest.mark.gpu

CASES = MR.cases()
INV = 1     # hipErrorInvalidValue


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    gpu_ready()


@functools.lru_cache(maxsize=None)
def wanted(index):
    want = MR.render_case(CASES[index])
    want.setflags(write=False)
    return want


def launch(c, dtype, pad=0):
    from signals_amd import _native
    rows, voices = c['N'] * c['K'], c['voices']
    buf = torch.full((rows, voices + pad), 7.0, dtype=dtype, device='cuda:0')
    _native.modal_bank(c['position'], RATE, dev(c['hertz']), dev(c['gate_on']), dev(c['damp']), dev(c['select']), dev(MR.table(c['modes'])),
                       buf[:, :voices], step=c['step'], rows_per_param=c['N'] if c['K'] > 1 else 0)
    got = buf.cpu().numpy()
    assert (got[:, voices:] == 7.0).all(), (c['name'], 'the padding is not written')
    return got[:, :voices]


def check(c, got, want, what):
    """NaN placement exactly, the restatement's exact zeros (before a strike, every mode dropped) exactly 0.0, everything else within
    the bound; returns the largest error"""
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, 'NaN placement')
    gate = np.zeros((1, 1)) if c['gate_on'] is None else c['gate_on']
    n = c['position'] + np.arange(c['N'] * c['K']) * c['step']
    e = n[:, None] / RATE - np.repeat(gate, c['N'], axis=0) if gate.shape[0] > 1 else n[:, None] / RATE - gate
    silent = np.broadcast_to(~(e >= 0), want.shape)
    assert (got[silent] == 0.0).all() and (want[silent] == 0.0).all(), (what, 'rows before the strike are exactly 0.0')
    tab = MR.table(c['modes'])
    hz = np.broadcast_to(c['hertz'], (c['hertz'].shape[0], c['voices']))
    with np.errstate(invalid='ignore'):
        dropped = np.abs(hz) * tab[..., 0].min() >= 0.5 * RATE               # every mode of every set at or above half the rate
    dropped = np.repeat(dropped, c['N'], axis=0) if dropped.shape[0] > 1 else np.broadcast_to(dropped, want.shape)
    assert (got[dropped] == 0.0).all(), (what, 'every mode dropped is exactly 0.0')
    err, tol = maxerr(got, want), MR.tolerance(c['modes'])
    print('modal kernel', what, 'max|err|', err, 'tol', tol)
    assert err <= tol, (what, err, tol)
    return err


# ---------------------------------------------------------------------------------------------- C ABI
@pytest.mark.parametrize('index', range(len(CASES)), ids=[c['name'] for c in CASES])
def test_kernel_against_the_restatement(index):
    c, want = CASES[index], wanted(index)
    worst32 = check(c, launch(c, torch.float32, pad=0 if index % 2 else 3), want, (c['name'], 'float32'))
    worst64 = check(c, launch(c, torch.float64, pad=5 if index % 2 else 0), want, (c['name'], 'float64'))
    print('modal worst', c['name'], 'float32', worst32, 'float64', worst64, 'A', MR.gain_bound(c['modes']))


def test_the_refusals_leave_the_output_untouched():
    from signals_amd import _native
    lib = _native.lib()
    V, rows = 8, 128
    out = torch.full((rows, V), 7.0, dtype=torch.float32, device='cuda:0')
    hz, modes = dev(np.full((1, V), 440.0)), dev(MR.table(MR.mode_table(4, 2)))
    args = dict(position=64, step=1, rate=RATE, rows=rows, voices=V, rpp=0,
                hertz=hz.data_ptr(), hs=1, hrs=0, gate=None, gs=0, grs=0, damp=None, ds=0, drs=0, select=None, ss=0, srs=0,
                modes=modes.data_ptr(), W=2, M=4, out=out.data_ptr(), odt=_native.F32, old=V, stream=None)

    def call(**over):
        a = dict(args, **over)
        return lib.sig_modal_bank(*(a[k] for k in args))
    refused = [dict(modes=None), dict(hertz=None), dict(out=None), dict(M=0), dict(M=65), dict(W=0), dict(W=513, M=4), dict(old=V - 1),
               dict(position=-1), dict(hs=2), dict(gs=-1), dict(ds=3), dict(ss=2), dict(hrs=-1), dict(step=0), dict(rate=0), dict(odt=2)]
    for over in refused:
        assert call(**over) == INV, over
    assert call(rows=0) == 0 and call(voices=0) == 0                          # accepted, nothing launched
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7.0).all()                                   # the canary stands after every one of them
    assert call() == 0
    torch.cuda.synchronize()
    assert maxerr(out.cpu().numpy(), MR.modal(MR.mode_table(4, 2), 64, rows, np.full((1, V), 440.0))) <= MR.tolerance(MR.mode_table(4, 2))


def test_a_stretch_of_frames_has_the_same_bits_however_it_is_launched():
    """4 blocks of 64 frames in one launch with per-block rows, in four launches, and as one launch of constant rows cut differently:
    bit-equal, from a position that is a multiple of the run and from one that is not"""
    from signals_amd import _native
    V, N, K = 70, 64, 4
    modes = dev(MR.table(MR.mode_table(24, 3)))
    for pos in (0, 1000):
        c = next(c for c in CASES if c['name'] == f'per block[pos={pos}]')
        rows = [dev(np.ascontiguousarray(np.repeat(c[k], 1, axis=0)[:, :V])) for k in ('hertz', 'gate_on', 'damp', 'select')]
        whole = torch.empty((N * K, V), dtype=torch.float32, device='cuda:0')
        _native.modal_bank(pos, RATE, *rows, modes, whole, rows_per_param=N)
        parts = []
        for b in range(K):
            part = torch.empty((N, V), dtype=torch.float32, device='cuda:0')
            _native.modal_bank(pos + b * N, RATE, *(r[b:b + 1].contiguous() for r in rows), modes, part)
            parts.append(part)
        assert torch.equal(whole.view(torch.int32), torch.cat(parts).view(torch.int32)), pos
        first = [r[:1].contiguous() for r in rows]                            # constant rows: any cut of the stretch
        one = torch.empty((N * K, V), dtype=torch.float64, device='cuda:0')
        _native.modal_bank(pos, RATE, *first, modes, one)
        cut = [torch.empty((n, V), dtype=torch.float64, device='cuda:0') for n in (1, 99, 29, 127)]
        at = pos
        for part in cut:
            _native.modal_bank(at, RATE, *first, modes, part)
            at += part.shape[0]
        assert torch.equal(one.view(torch.int64), torch.cat(cut).view(torch.int64)), pos


# ---------------------------------------------------------------------------------------------- the node, eager and batched
V = 8
MODES = np.stack([MR.mode_table(12, 1)[0], np.concatenate([MR.string64()[:8], np.tile([0.0, 0.0, 1.0], (4, 1))])])    # (2, 12, 3)


def draw(seed=3):
    rng = np.random.default_rng(seed)
    th = rng.uniform(0, np.pi / 2, V)
    return dict(hertz=rng.uniform(110, 1760, (1, V)), gate_on=rng.uniform(-0.002, 0.006, (1, V)), damp=rng.uniform(0, 4, (1, V)),
                select=rng.uniform(-1, 3, (1, V)), cut=rng.uniform(200, 8000, (1, V)), pan=np.stack([np.cos(th), np.sin(th)]))


def node(modes, hertz, gate_on=None, damp=None, select=None):
    from signals_amd.chain import ext
    m = ext.Modal()
    m.get_state().modes = modes
    for name, value in (('hertz', hertz), ('gate_on', gate_on), ('damp', damp), ('select', select)):
        if value is not None:
            setattr(m, name, fix(value) if isinstance(value, np.ndarray) else value)
    return m


def sweep(p):
    """hertz on a slow Sine around each voice's pitch: (GPU node, oracle node)"""
    from oracle import chain_ref as R
    from signals_amd.chain import fx
    s = mkosc('Sine', [[3.1]])
    g = fx.Gain(); g.left = s; g.right = fix(0.2 * p['hertz'])
    m = fx.Mix(); m.left = g; m.right = fix(2.0 * p['hertz']); m.mix = fix([[0.5]])
    rm = R.Binary('Mix', R.Binary('Gain', R.Osc('Sine', R.Fixed([[3.1]])), R.Fixed(0.2 * p['hertz'])), R.Fixed(2.0 * p['hertz']), R.Fixed([[0.5]]))
    return m, rm


def graph(which, p, pos, swept=True):
    """(GPU node, oracle node, rendered width): the voice under a bus, alone or through a low-pass; struck around `pos`; `swept`:
    hertz on a slow Sine, else on Fixed rows like gate_on"""
    from oracle import chain_ref as R
    from signals_amd.chain import ext, fx
    RM = MR.oracle_node()
    gate = p['gate_on'] + pos / RATE
    hz, rhz = sweep(p) if swept else (p['hertz'], R.Fixed(p['hertz']))
    m = node(MODES, hz, gate, p['damp'], p['select'])
    rm = RM(MODES, rhz, R.Fixed(gate), R.Fixed(p['damp']), R.Fixed(p['select']))
    if which == 'lowpass_bus':
        lp = fx.LowPass(); lp.input = m; lp.cutoff = fix(p['cut'])
        m, rm = lp, R.Filter('lp', rm, R.Fixed(p['cut']))
    b = ext.SumBus(); b.input = m; b.get_state().gains = np.ascontiguousarray(p['pan'])
    return b, R.SumBus(rm, p['pan']), 2


def test_the_eager_block_equals_the_kernel_call_bit_for_bit():
    from signals_amd import _native
    p = draw()
    for pos, frames in ((0, 64), (1000, 100)):
        got = render(node(MODES, p['hertz'], p['gate_on'] + pos / RATE, p['damp'], p['select']), pos, frames, V)
        out = torch.empty((frames, V), dtype=torch.float32, device='cuda:0')
        _native.modal_bank(pos, RATE, dev(p['hertz']), dev(p['gate_on'] + pos / RATE), dev(p['damp']), dev(p['select']), dev(MR.table(MODES)), out)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), out.cpu().numpy().view(np.int32))


@pytest.mark.parametrize('pos', [0, 37, 2 ** 24 + 5])
def test_one_frame_requests_are_float64_and_within_the_bound(pos):
    p = draw()
    gate = p['gate_on'] + pos / RATE - 0.003
    for frames in (1, 70):
        got = render(node(MODES, p['hertz'], gate, p['damp'], p['select']), pos, frames, V)
        want = MR.modal(MODES, pos, frames, p['hertz'], gate, p['damp'], p['select'])
        assert got.shape == (frames, V) and got.dtype == (np.float64 if frames == 1 else np.float32)
        err = maxerr(got, want)
        print('modal eager', pos, frames, 'max|err|', err)
        assert err <= MR.tolerance(MODES)
    plain = render(node(MODES, p['hertz']), pos, 1, V)                        # unplugged gate_on, damp, select: zeros
    assert np.array_equal(plain, render(node(MODES, p['hertz'], np.zeros((1, 1)), np.zeros((1, 1)), np.zeros((1, 1))), pos, 1, V))


def test_a_narrow_control_raises_index_error():
    """the node's own check, reached where the port does not refuse the reply first: in the batched engine, as a narrow `cutoff` is"""
    from signals_amd.engine import BatchRenderer
    p = draw()
    with pytest.raises(IndexError, match='index 3 is out of bounds for axis 1 with size 3'):
        BatchRenderer(node(MODES, p['hertz'][:, :3]), V, RATE).render(0, 64, 2)
    with pytest.raises(IndexError, match='index 5 is out of bounds for axis 1 with size 5'):
        BatchRenderer(node(MODES, p['hertz'], damp=p['damp'][:, :5]), V, RATE).render(0, 64, 2)
    m = node(MODES, p['hertz'])
    with pytest.raises(IndexError, match='index 3 is out of bounds for axis 1 with size 3'):
        m.control_rows(lambda bound: dev(p['hertz'][:, :3]), V)


@functools.lru_cache(maxsize=None)
def oracle_rows(which, pos, N, blocks, swept):
    from oracle import chain_ref as R
    _, ref, C = graph(which, draw(), pos, swept)
    want = R.render_stream(ref, pos, N, blocks, C)
    want.setflags(write=False)
    return want


ROUTES = {'per_node': {'fuse': False}, 'default': {}, 'specialise=False': {'specialise': False},
          'mixed_programs': {'fuse_program': 'always', 'mixed_programs': True}}
# 8 voices, 5 blocks as batches of 2 and 3, gate_on on Fixed rows.  The issue's shape is 64 frames with hertz on a slow Sine.  Behind a
# filter the engine renders no modulated source at blocks of 100 frames or fewer, whatever the source is (it answers NotBatchable
# and the graph keeps the eager path): that leg is pinned as the refusal it is, and the low-pass graph is compared at 64 frames with
# hertz on Fixed rows and at 128 frames with the sweep
SHAPES = {'bus,64,swept': ('bus', 64, True), 'lowpass_bus,64,fixed': ('lowpass_bus', 64, False), 'lowpass_bus,128,swept': ('lowpass_bus', 128, True)}


@pytest.mark.parametrize('pos', [0, 1000])
@pytest.mark.parametrize('route', list(ROUTES))
@pytest.mark.parametrize('shape', list(SHAPES))
def test_batched_rows_equal_eager_rows_bit_for_bit_and_the_oracle_within_the_bound(shape, route, pos):
    which, N, swept = SHAPES[shape]
    ks = (2, 3)
    p = draw()
    eager = stream(graph(which, p, pos, swept)[0], pos, N, sum(ks), 2)
    got, names, _ = render_batches(graph(which, p, pos, swept)[0], 2, pos, N, ks, names=True, **ROUTES[route])
    what = (shape, route, pos)
    banks = sorted(n for n in names if n.startswith('modal_bank'))
    assert banks == ['modal_bank[Modal12,per-block]' if swept else 'modal_bank[Modal12]'], (what, names)     # one kernel per batch, one label
    assert not any(word in n for n in names for word in ('voice_program', 'fused', 'cascade', 'walk', 'steady', 'latency')), (what, names)
    assert got.dtype == np.float32
    # the node's rows are the same bits on both paths; so is everything behind them where the engine runs one kernel per node, which
    # it does for the bare bus on every route.  With fusing on, LowPass -> SumBus is the filter-and-bus pass (biquad_bus[lp]), whose
    # sums differ from the eager bus's in the last bit for any source: those legs are held to the bound against the eager rows too
    if which == 'bus' or route == 'per_node':
        assert np.array_equal(got.view(np.int32), eager.view(np.int32)), what
    else:
        assert 'biquad_bus[lp]' in names and maxerr(got, eager) <= tolerance(eager), (what, names)
    want = oracle_rows(which, pos, N, sum(ks), swept)
    err, tol = maxerr(got, f32(want)), tolerance(want) * max(1.0, MR.gain_bound(MODES))
    print('modal route', what, 'max|err|', err, 'tol', tol, sorted(names))
    assert err <= tol, (what, err, tol)


@pytest.mark.parametrize('pos', [0, 1000])
def test_a_swept_voice_behind_a_filter_at_64_frames_keeps_the_eager_path(pos):
    """the engine's rule for every modulated source in front of a filter at blocks of 100 frames or fewer; the eager rows are the
    oracle's within the bound"""
    from signals_amd.engine import BatchRenderer, NotBatchable
    p = draw()
    with pytest.raises(NotBatchable, match='block size <= 100'):
        BatchRenderer(graph('lowpass_bus', p, pos)[0], 2, RATE).render(pos, 64, 5)
    eager = stream(graph('lowpass_bus', p, pos)[0], pos, 64, 5, 2)
    want = oracle_rows('lowpass_bus', pos, 64, 5, True)
    err, tol = maxerr(eager, f32(want)), tolerance(want) * max(1.0, MR.gain_bound(MODES))
    print('modal eager behind a filter', pos, 'max|err|', err, 'tol', tol)
    assert err <= tol


def test_a_table_edited_in_place_and_a_table_replaced_are_heard_at_the_next_render():
    p = draw()
    modes = MR.string64()[:6].copy()
    m = node(modes, p['hertz'])
    tol = MR.tolerance(modes)
    assert maxerr(render(m, 0, 64, V), MR.modal(modes, 0, 64, p['hertz'])) <= tol
    modes[1] = (2.37, -0.8, 0.3)                                              # edited in place: an inharmonic second mode
    after = render(m, 64, 64, V)
    assert maxerr(after, MR.modal(modes, 64, 64, p['hertz'])) <= tol
    assert maxerr(after, MR.modal(MR.string64()[:6], 64, 64, p['hertz'])) > 100 * tol
    bar = np.array([[1, 1, 2], [3, 1, 1]])                                    # replaced, by an integer array
    m.get_state().modes = bar
    assert maxerr(render(m, 128, 64, V), MR.modal(bar, 128, 64, p['hertz'])) <= MR.tolerance(bar)
