"""The 4-pole ladder filter on the GPU: sig_ladder_coldstart through _native.ladder_coldstart against tests/ladder_reference.py at the
smallest shapes that reach each edge of the kernel, then the eager node (BlockDriver, eager pulls) against the batched engine
(BatchRenderer, fuse=False and the default route) bit for bit, and all of them against a float64 chain of oracle.chain_ref plus the
restatement.

The bar is the project's own (README: every output within 1e-6 of the reference): |got - ref| <= 1e-6 * max(1, max|ref|) on every
element of every output, float32 outputs against the float64 restatement too; NaN exactly where the definition says NaN and nowhere
else.  What the bar has to absorb: the device's tan and tanh against numpy's (an ulp or two of float64, carried through a loop whose
gain stays of order 1 over <= 356 rows), the kernel's rounded 1 / d, and for float32 outputs the store's rounding, 2^-24 max|ref| =
6e-8 max|ref| -- every kernel case asserts that this floor, computed from the reference alone, is under a quarter of the bar.  Input
amplitudes <= 1 and k <= 4 keep max|ref| of order 1.

Shapes.  voices 1 (a lone lane), 3 (no vector access), 64 (a full wave), 65 (one lane over), 68 (4 voices per lane, a ragged tile);
block_frames 16 (shorter than the context: blocks reach into the history), 100, 101, 256; nblocks 1 and 3; positions 0, 37, 1000
(history 0, 37, 100); poles 1 .. 4; float32 and float64 buffers; contiguous, padded (an odd leading dimension) and offset (a base pointer
one and two elements into a row) layouts, which take the kernel from 4 voices per lane to 1 and 2.  The references are computed once
per case and shared by the dtypes and layouts."""
import functools
import math

import numpy as np
import pytest
import torch

from gpu_helpers import dev, gpu_ready, render_batches
from helpers import RATE, fix, maxerr, mkosc
import ladder_reference as LR

pytestmark = pytest.mark.gpu

BAR = 1e-6


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    gpu_ready()


def same(got, want):
    """bit for bit: the same NaN positions, the same bit patterns elsewhere"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    nan = np.isnan(want)
    bits = np.uint64 if got.dtype == np.float64 else np.uint32
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(bits), want[~nan].view(bits)))


def within_bar(got, want):
    """(ok, error over the bar's scale): every element, NaN exactly where `want` has NaN"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False, math.inf
    live = ~np.isnan(want)
    if not live.any():
        return True, 0.0
    err = float(np.max(np.abs(got[live] - want[live]))) / max(1.0, float(np.max(np.abs(want[live]))))
    return err <= BAR, err


# ---------------------------------------------------------------------------------------------- the kernel
# every voice takes the next value, moved on by three per block: V = 1 takes the first ones, V >= 8 all of them
CUTS = [20.0, 0.49 * RATE, 200.0, 1000.0, 3000.0, 8000.0, 12000.0, 55.0]
KS = [0.0, 3.99, 4.0, 7.0, 1.0, 2.5, -2.0, 3.5]                              # 7 clips to 4, -2 to 0
DS = [0.0, 0.5, 8.0, -1.0, 2.0, 0.0, 1.0, 30.0]                              # -1 clips to 0
# (cutoff rows, k rows and columns, d rows and columns): 'K' one row per block, 1 one row; 'V' one column per voice, 1 one column; None: a null row
FORMS = {'rows': ('K', ('K', 'V'), ('K', 'V')), 'one': (1, (1, 'V'), (1, 'V')), 'columns': ('K', ('K', 1), (1, 1)),
         'linear': (1, (1, 'V'), None), 'driven': ('K', None, (1, 'V')), 'bare': (1, None, None), 'zeros': (1, (1, 1), 'zeros')}


def control(values, rows, cols, K, V, shift=0):
    r, c = (K if rows == 'K' else 1), (V if cols == 'V' else 1)
    return np.array([[values[(v + 3 * b + shift) % len(values)] for v in range(c)] for b in range(r)], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def kernel_case(V, N, K, pos, poles, form):
    """(window float32-representable float64, cutoff, k | None, d | None, float64 reference): computed once, read-only"""
    rng = np.random.default_rng(V * 1000 + N * 10 + K + pos + poles)
    c0 = min(100, pos)
    x = rng.uniform(-1.0, 1.0, (c0 + N * K, V)).astype(np.float32).astype(np.float64)
    cut_rows, k_form, d_form = FORMS[form]
    cut = control(CUTS, cut_rows, 'V', K, V)
    k = None if k_form is None else control(KS, *k_form, K, V, shift=1)
    d = None if d_form is None else (np.zeros((1, V)) if d_form == 'zeros' else control(DS, *d_form, K, V, shift=2))
    want, status = LR.ladder_blocks(x, c0, N, K, cut, k, d, poles, RATE)
    assert status == 0 and not np.isnan(want).any()
    for a in (x, cut, k, d, want):
        if a is not None:
            a.setflags(write=False)
    return x, cut, k, d, want


def laid_out(a, dtype, layout):
    """(the buffer, the (rows, V) view of it that holds `a`): 'contig', 'padded' (leading
    dimension V + 3), 'off1' / 'off2' (leading dimension V + 4, the view one / two elements into the row)"""
    rows, V = a.shape
    pad, off = {'contig': (0, 0), 'padded': (3, 0), 'off1': (4, 1), 'off2': (4, 2)}[layout]
    buf = torch.zeros((rows, V + pad), dtype=dtype, device='cuda:0')
    view = buf[:, off:off + V]
    view.copy_(torch.from_numpy(np.array(a)).to('cuda:0', dtype))
    return buf, view


SEEN = {(kind, dt): 0.0 for kind in ('linear', 'driven') for dt in ('float32', 'float64')}


@pytest.mark.parametrize('pos', [0, 37, 1000])
@pytest.mark.parametrize('V', [1, 3, 64, 65, 68])
def test_ladder_coldstart_meets_the_restatement(V, pos):
    """every N and K at one (V, position), the poles and the control forms taking turns so that each (V, position) sees all of them;
    both dtypes, four layouts; outputs are padded and the padding must stay untouched"""
    from signals_amd import _native
    c0 = min(100, pos)
    forms = sorted(FORMS)
    turn = 0
    for N in (16, 100, 101, 256):
        for K in (1, 3):
            for form in (forms[turn % len(forms)], forms[(turn + 3) % len(forms)]):
                poles = 1 + turn % 4
                turn += 1
                x, cut, k, d, want = kernel_case(V, N, K, pos, poles, form)
                scale = max(1.0, float(np.max(np.abs(want))))
                floor = float(np.max(np.abs(want.astype(np.float32).astype(np.float64) - want)))
                assert floor <= 0.25 * BAR * scale and scale < 16.0, (floor, scale)      # the float32 floor of the reference alone; max|ref| of order 1
                status = torch.zeros(1, dtype=torch.int32, device='cuda:0')
                for dtype in (torch.float32, torch.float64):
                    for layout in ('contig', 'padded', 'off1', 'off2'):
                        _, xin = laid_out(x, dtype, layout)
                        obuf, out = laid_out(np.zeros((N * K, V)), dtype, layout)
                        _native.ladder_coldstart(RATE, pos, N, K, 100, dev(cut), dev(k), dev(d), poles, xin, c0, out, status=status)
                        got = obuf.cpu().numpy()
                        off = {'contig': 0, 'padded': 0, 'off1': 1, 'off2': 2}[layout]
                        ok, err = within_bar(got[:, off:off + V], want)
                        kind = 'driven' if d is not None and (d > 0).any() else 'linear'
                        key = (kind, str(dtype).split('.')[-1])
                        SEEN[key] = max(SEEN[key], err)
                        assert ok, (V, pos, N, K, poles, form, dtype, layout, err)
                        assert not got[:, :off].any() and not got[:, off + V:].any(), (V, pos, N, K, form, layout)
                assert int(status.item()) == 0, (V, pos, N, K, form)
    print(f'ladder kernel V={V} pos={pos}: max error over the bar\'s scale so far: ' + ', '.join(f'{k} {dt} {e:.3e}' for (k, dt), e in sorted(SEEN.items())))


def test_an_unplugged_drive_a_row_of_zeros_and_a_negative_drive_are_the_same_filter():
    """three ways to a linear loop: the kernel without tanh (a null row), and the `d > 0` branch not taken per lane"""
    from signals_amd import _native
    V, N, K, pos = 68, 101, 3, 1000
    x, cut, k, _, want = kernel_case(V, N, K, pos, 4, 'linear')
    outs = []
    for d in (None, np.zeros((1, V)), np.full((1, 1), -1.0), np.full((K, V), -math.inf)):
        out = torch.zeros((N * K, V), dtype=torch.float64, device='cuda:0')
        _native.ladder_coldstart(RATE, pos, N, K, 100, dev(cut), dev(k), dev(d), 4, dev(x), 100, out)
        outs.append(out.cpu().numpy())
    assert within_bar(outs[0], want)[0] and all(same(o, outs[0]) for o in outs[1:])


def test_bad_controls_give_nan_rows_and_exactly_their_status_bits():
    """a bad cutoff, k or drive in a live voice: NaN rows for that voice in that block alone; SIG_STATUS_BAD_CUTOFF and
    SIG_STATUS_BAD_RESONANCE exactly as the definition says, no bit for the drive, none from the padding lanes"""
    from signals_amd import _native
    nan, inf = math.nan, math.inf
    V, N, K, pos = 68, 16, 3, 37
    rng = np.random.default_rng(9)
    x = rng.uniform(-1, 1, (37 + N * K, V)).astype(np.float32).astype(np.float64)

    def rows(base):
        return np.tile(np.array(base, dtype=np.float64), (K, 1))
    good = dict(cut=rows([1000.0 + 50 * v for v in range(V)]), k=rows([KS[v % 8] for v in range(V)]), d=rows([DS[v % 8] for v in range(V)]))
    cases = [('cut', [(0, 5, nan), (1, 0, 0.0), (2, 67, RATE / 2.0), (1, 33, -10.0), (0, 64, 1e9)], _native.STATUS_BAD_CUTOFF),
             ('k', [(0, 1, nan), (1, 66, inf), (2, 3, -inf)], _native.STATUS_BAD_RESONANCE),
             ('d', [(0, 2, nan), (2, 65, inf)], 0),
             ('all', [], _native.STATUS_BAD_CUTOFF | _native.STATUS_BAD_RESONANCE)]
    for name, edits, bits in cases:
        ctl = {key: value.copy() for key, value in good.items()}
        if name == 'all':
            ctl['cut'][1, 7] = nan; ctl['k'][1, 7] = nan; ctl['k'][2, 40] = inf; ctl['d'][0, 9] = nan
            edits = [(1, 7, nan), (2, 40, inf), (0, 9, nan)]
        else:
            for b, v, value in edits:
                ctl[name][b, v] = value
        want, status = LR.ladder_blocks(x, 37, N, K, ctl['cut'], ctl['k'], ctl['d'], 4, RATE)
        mask = np.zeros((N * K, V), dtype=bool)
        for b, v, _ in edits:
            mask[b * N:(b + 1) * N, v] = True
        assert status == bits and np.array_equal(np.isnan(want), mask), name
        for dtype in (torch.float32, torch.float64):
            word = torch.zeros(1, dtype=torch.int32, device='cuda:0')
            out = torch.zeros((N * K, V), dtype=dtype, device='cuda:0')
            _native.ladder_coldstart(RATE, 37, N, K, 100, dev(ctl['cut']), dev(ctl['k']), dev(ctl['d']), 4, dev(x, dtype), 37, out, status=word)
            ok, err = within_bar(out.cpu().numpy(), want)                     # (NaN exactly on `mask`, the other voices untouched by it)
            assert ok and int(word.item()) == bits, (name, dtype, err, int(word.item()))
    # the padding lanes shadow voice 0: a bad voice 0 is reported once, by its live lane, and a good one by nobody
    for V in (3, 65):
        word = torch.zeros(1, dtype=torch.int32, device='cuda:0')
        out = torch.zeros((N, V), dtype=torch.float32, device='cuda:0')
        _native.ladder_coldstart(RATE, 0, N, 1, 100, dev(np.full((1, V), 1000.0)), None, None, 4, dev(x[:N, :V], torch.float32), 0, out, status=word)
        assert int(word.item()) == 0 and not torch.isnan(out).any()


def test_wrapper_refusals():
    from signals_amd import _native
    x = torch.zeros((100 + 256, 8), dtype=torch.float32, device='cuda:0')
    out = torch.zeros((256, 8), dtype=torch.float32, device='cuda:0')
    cut = dev(np.full((1, 8), 1000.0))
    with pytest.raises(_native.NativeError, match='ladder shapes'):
        _native.ladder_coldstart(RATE, 4096, 256, 1, 100, cut, None, None, 4, x[:300], 100, out)
    with pytest.raises(_native.NativeError, match='hipError_t 1'):
        _native.ladder_coldstart(RATE, 4096, 256, 1, 100, cut, None, None, 5, x, 100, out)                  # poles
    with pytest.raises(IndexError):
        _native.ladder_coldstart(RATE, 4096, 256, 1, 100, dev(np.full((1, 1), 1000.0)), None, None, 4, x, 100, out)
    assert not out.any()                                                      # (a launch with nothing to render: tests/test_ladder_host.py, at the C entry)


# ---------------------------------------------------------------------------------------------- graphs: eager against batched against the oracle
GV = 5
LFO_HZ = 2.3
FUSED = ('fused', 'latency', 'cascade', 'steady', 'walk', 'biquad_bus', 'biquad_coldstart_env', 'voice_program')


def ladder_node(input_, cutoff, resonance=None, drive=None, poles=4):
    from signals_amd.chain import ext
    n = ext.Ladder()
    n.get_state().poles = poles
    n.input = input_
    for name, value in (('cutoff', cutoff), ('resonance', resonance), ('drive', drive)):
        if value is not None:
            setattr(n, name, fix(value) if isinstance(value, np.ndarray) else value)
    return n


def draw():
    rng = np.random.default_rng(23)
    th = rng.uniform(0, np.pi / 2, GV)
    return dict(hertz=rng.uniform(55, 1760, (1, GV)), phase=rng.uniform(0, 1, (1, GV)), cut=rng.uniform(200, 8000, (1, GV)),
                cut2=rng.uniform(200, 8000, (1, GV)), k=np.array([[0.0, 3.99, 4.0, 3.0, 7.0]]), k2=rng.uniform(0, 3, (1, GV)),
                d=np.array([[2.0, 0.0, 0.5, 8.0, -1.0]]), pan=np.stack([np.cos(th), np.sin(th)]) / GV)


def graph(which, p):
    """(GPU node, oracle node, rendered width, the launch labels of its ladders)"""
    from oracle import chain_ref as R
    from signals_amd.chain import ext, fx, noise
    RL = LR.oracle_node()
    saw = lambda: mkosc('Sawtooth', p['hertz'], p['phase'])
    rsaw = lambda: R.Osc('Sawtooth', R.Fixed(p['hertz']), R.Fixed(p['phase']))
    if which == 'saw':
        return (ladder_node(saw(), p['cut'], p['k'], p['d']), RL(rsaw(), R.Fixed(p['cut']), R.Fixed(p['k']), R.Fixed(p['d'])), GV,
                {'ladder_coldstart[4,drive]'})
    if which == 'swept_bus':
        # cutoff = 0.5 * (800 * sine LFO, a phase per voice) + 0.5 * cutoffs: per-block rows; k Fixed per voice; a stereo bus behind
        lfo = fx.Gain(); lfo.left = mkosc('Sine', [[LFO_HZ]], p['phase']); lfo.right = fix([[800.0]])
        cut = fx.Mix(); cut.left = lfo; cut.right = fix(2.0 * p['cut'] + 1000.0); cut.mix = fix([[0.5]])
        b = ext.SumBus(); b.input = ladder_node(saw(), cut, p['k'], poles=3); b.get_state().gains = np.ascontiguousarray(p['pan'])
        rcut = R.Binary('Mix', R.Binary('Gain', R.Osc('Sine', R.Fixed([[LFO_HZ]]), R.Fixed(p['phase'])), R.Fixed([[800.0]])),
                        R.Fixed(2.0 * p['cut'] + 1000.0), R.Fixed([[0.5]]))
        return b, R.SumBus(RL(rsaw(), rcut, R.Fixed(p['k']), poles=3), p['pan']), 2, {'ladder_coldstart[3,blocks]'}
    if which == 'twice':
        return (ladder_node(ladder_node(saw(), p['cut'], p['k2'], poles=2), p['cut2'], p['k2'], p['d']),
                RL(RL(rsaw(), R.Fixed(p['cut']), R.Fixed(p['k2']), poles=2), R.Fixed(p['cut2']), R.Fixed(p['k2']), R.Fixed(p['d'])), GV,
                {'ladder_coldstart[2]', 'ladder_coldstart[4,drive]'})
    if which == 'white':
        w = noise.White(); w.get_state().channels = GV; w.get_state().seed = 11
        return (ladder_node(w, p['cut'], p['k'], p['d'], poles=1), RL(R.White(11, GV), R.Fixed(p['cut']), R.Fixed(p['k']), R.Fixed(p['d']), poles=1),
                GV, {'ladder_coldstart[1,drive]'})
    if which == 'narrow':
        # ONE column in: a Sawtooth with one hertz for all, under cutoff, k and drive rows as wide as the request
        return (ladder_node(mkosc('Sawtooth', [[220.0]]), p['cut'], p['k'], p['d']),
                RL(R.Osc('Sawtooth', R.Fixed([[220.0]])), R.Fixed(p['cut']), R.Fixed(p['k']), R.Fixed(p['d'])), GV, {'ladder_coldstart[4,drive]'})
    raise KeyError(which)


GRAPHS = ('saw', 'swept_bus', 'twice', 'white', 'narrow')


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


@functools.lru_cache(maxsize=None)
def oracle_rows(which, pos, N, blocks):
    from oracle import chain_ref as R
    _, ref, C, _ = graph(which, draw())
    want = R.render_stream(ref, pos, N, blocks, C)
    want.setflags(write=False)
    return want


@pytest.mark.parametrize('pos', [0, 1000])
@pytest.mark.parametrize('N', [64, 256])
@pytest.mark.parametrize('which', GRAPHS)
def test_batched_equals_eager_and_both_meet_the_oracle(which, N, pos):
    """three batches of four blocks: the second and third continue the first (the tails), the first at 1000 starts mid-stream (the
    own-history block).  One kernel per node (fuse=False): bit-equal to the eager path.  The default route: bit-equal where no fused
    kernel took a node around the ladder, else the bar.  Ladder(Ladder) at N = 64 is an impure input under short blocks: the batch
    refuses like a filter's, the driver falls back to the eager path and that is what is compared"""
    from signals_amd import runtime
    from signals_amd.chain.driver import BlockDriver
    from signals_amd.engine import BatchRenderer, NotBatchable
    p, ks = draw(), (4, 4, 4)
    _, _, C, labels = graph(which, p)
    want = oracle_rows(which, pos, N, sum(ks))
    eager = eager_rows(graph(which, p)[0], C, pos, N, sum(ks))
    ok, err = within_bar(eager, want)
    print(f'ladder graph {which} N={N} pos={pos}: eager error over the bar\'s scale {err:.3e}, max|ref| {np.max(np.abs(want)):.3f}')
    assert eager.dtype == np.float32 and ok, (which, N, pos, err)
    for kw in ({'fuse': False}, {}):
        if which == 'twice' and N <= 100:
            with pytest.raises(NotBatchable, match='block size <= 100'):
                BatchRenderer(graph(which, p)[0], C, RATE, **kw).render(pos, N, ks[0])
            d = BlockDriver(RATE, N)
            d.get_state().channels = C
            d.engine_options = dict(kw)
            d.input = graph(which, p)[0]
            d.frame_position = pos
            got = np.concatenate([d.render(k) for k in ks])
            del d.input
            assert d._engine_ok is False and same(got, eager), (which, N, pos, kw)
            continue
        got, names = batched_rows(graph(which, p)[0], C, pos, N, ks, **kw)
        assert {n for n in names if n.startswith('ladder_coldstart[')} == labels, (kw, names)
        fused = {n for n in names if any(w in n for w in FUSED)}
        assert not fused, (kw, names)                                          # nothing around the ladder fuses on these graphs: the same launches
        ok, err = within_bar(got, want)
        assert got.dtype == np.float32 and ok, (which, N, pos, kw, err)
        assert same(got, eager), (which, N, pos, kw, maxerr(got, eager))
    runtime.check_status()                                                    # no status bit was set on any route


@pytest.mark.parametrize('pos', [0, 37, 1000])
def test_one_frame_requests(pos):
    """frames == 1: float64 from the same kernel; in a control path the batch refuses with the reason and the eager path serves it"""
    from helpers import render
    from oracle import chain_ref as R
    from signals_amd.chain import fx
    from signals_amd.engine import BatchRenderer, NotBatchable
    p = draw()
    top, ref, C, _ = graph('saw', p)
    got = render(top, pos, 1, GV)
    want = R.render(ref, pos, 1, GV)
    assert got.shape == (1, GV) and got.dtype == np.float64
    assert within_bar(got, want)[0]                                           # (the context rows are the oscillator's stored float32 blocks)

    def voice():
        lfo = ladder_node(mkosc('Sine', [[3.0]]), np.full((1, GV), 100.0), np.full((1, GV), 2.0))      # (one column in, controls as wide as the request)
        hz = fx.Mix(); hz.left = lfo; hz.right = fix(p['cut']); hz.mix = fix([[0.001]])           # the cutoffs, moved by the filtered LFO
        f = fx.LowPass(); f.input = mkosc('Sawtooth', p['hertz'], p['phase']); f.cutoff = hz
        return f
    with pytest.raises(NotBatchable, match='Ladder in a control path: a ladder filter has no block-rate'):
        BatchRenderer(voice(), GV, RATE).render(pos, 256, 2)
    RL = LR.oracle_node()
    lfo_ref = RL(R.Osc('Sine', R.Fixed([[3.0]])), R.Fixed(np.full((1, GV), 100.0)), R.Fixed(np.full((1, GV), 2.0)))
    vref = R.Filter('lp', R.Osc('Sawtooth', R.Fixed(p['hertz']), R.Fixed(p['phase'])),
                    R.Binary('Mix', lfo_ref, R.Fixed(p['cut']), R.Fixed([[0.001]])))
    eager = eager_rows(voice(), GV, pos, 256, 2)
    assert maxerr(eager, R.render_stream(vref, pos, 256, 2, GV)) < 1e-6


def test_bad_controls_raise_at_the_sink_edge():
    """a NaN k in one voice: that voice's rows are NaN on the eager path and check_status() raises; the other voices render"""
    from signals_amd import runtime
    p = draw()
    k = p['k'].copy(); k[0, 2] = math.nan
    top = ladder_node(mkosc('Sawtooth', p['hertz'], p['phase']), p['cut'], k, p['d'])
    from helpers import render
    rows = render(top, 0, 64, GV)                                             # (a probe, not the driver: that one checks the status itself)
    assert np.isnan(rows[:, 2]).all() and not np.isnan(np.delete(rows, 2, axis=1)).any()
    with pytest.raises(ValueError, match='filter resonance'):
        runtime.check_status()
    runtime.check_status()                                                    # (polled: the word is clear again)
