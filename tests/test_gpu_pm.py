"""Phase-modulation oscillators on the GPU: sig_osc_bank_pm against the numpy formula, the eager node against
tests/pm_reference.py, and the engine's routes (fuse=False, default, fuse_program='always', specialise=True) on two-operator
voices, carriers behind filters, enveloped and filtered modulators and short blocks, from position 0 and from one hour, over two
consecutive batches.

Tolerances.  The bar is 1e-6 per node output.  A PM carrier turns a modulator deviation e_m into S I e_m, S the
waveform's largest slope per cycle (Sine 2 pi, Triangle 4, Sawtooth 2, Square 0): float32(GPU) is compared with float32(reference)
within 1e-6 (1 + S I_max); behind filters the same factor applies to the neighbouring tests' filter tolerance, 1e-6 max(1, |ref|)
(test_gpu_program_engine.py, test_gpu_swept_band.py).  Square and Sawtooth jump by 2: on the routes whose
modulator differs from the reference's in the last float32 bit (the voice program computes it in float64 with the hardware sine) a
sample whose reference phase lies within 1e-5 >= 2 I_max e_m of a jump may land on the other side, so those samples are excluded,
at most 1e-3 of all.  Behind a filter a crossed jump reaches exactly the rows the reference's block structure lets it reach: every
block is filtered from zero state over [<= 100 context rows | block] (fx.py:85-106), so a sample at row r touches the rows from r
to the end of each block b with start_b - 100 <= r < end_b, at most N + 100 rows, and only those are excluded.  Their share
cannot stay below 1e-3 (2e-5 per jump of the samples are near one, each reaching up to N + 100 rows), so it is bounded by what the
count of near samples allows: with lambda = 2e-5 jumps rows voices expected, at most (lambda + 3 sqrt(lambda)) (N + 100) rows
(1.9 % at N = 256, 1.2 % at N = 64), while the near samples themselves stay below 1e-3.  fuse=False is bit-equal to the eager
path everywhere; both are compared WITHOUT a mask against the reference fed the float32 modulator the route itself materialises
(bit-exact for the non-sine carriers, the plain 1e-6 max(1, |ref|) behind filters and under the bus: no modulator deviation)."""
import numpy as np
import pytest
import torch

from gpu_helpers import ROUTES_WITH_DEFAULT as ROUTES, dev, gpu_ready, lfo, render_batches, tolerance
from helpers import HOUR, RATE, f32, fix, maxerr, mkosc, render, stream
from signals_amd.engine import CONTEXT
import pm_reference as PR

pytestmark = pytest.mark.gpu

KINDS = ('Sine', 'Square', 'Sawtooth', 'Triangle')
I_MAX = 4.0


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    gpu_ready()


# ---------------------------------------------------------------------------------------------- C ABI
def abi_case(kind, pos, V, rows, mod_dtype, wide_mod, pad, blocks, one_row_mod, out_dtype):
    """`blocks` > 1: that many parameter rows, rows / blocks output rows each; `one_row_mod`: a (1, .) modulator for every row"""
    from oracle import chain_ref as R
    from signals_amd import _native
    rng = np.random.default_rng(0)
    hz, ph, ix = rng.uniform(55, 1760, (blocks, V)), rng.uniform(0, 1, (blocks, V)), rng.uniform(0, I_MAX, (blocks, V))
    m = rng.uniform(-1, 1, (1 if one_row_mod else rows, V if wide_mod else 1)).astype(mod_dtype)
    mbuf = torch.zeros((m.shape[0], m.shape[1] + pad), dtype=torch.float32 if mod_dtype == np.float32 else torch.float64, device='cuda:0')
    mbuf[:, :m.shape[1]] = torch.from_numpy(m).to('cuda:0')
    obuf = torch.zeros((rows, V + pad), dtype=out_dtype, device='cuda:0')
    rpp = rows // blocks
    _native.osc_bank_pm(kind, pos, RATE, dev(hz), dev(ph), dev(ix), mbuf[:, :m.shape[1]], obuf[:, :V], rows_per_param=rpp if blocks > 1 else 0)
    got = obuf[:, :V].cpu().numpy()
    assert not obuf[:, V:].any()                                              # the padding is not written
    rep = lambda a: np.repeat(a, rpp, axis=0) if blocks > 1 else a
    t = (R.frame_range(pos, rows) / RATE * rep(hz) + rep(ph)) + rep(ix) * m.astype(np.float64)
    return got, R.osc_wave(kind, t)


@pytest.mark.parametrize('pos', [0, 50, HOUR])
@pytest.mark.parametrize('kind', KINDS)
def test_osc_bank_pm_matches_the_formula(kind, pos):
    # (voices, modulator dtype, (N, V) modulator, padding of both leading dimensions, parameter rows, rows, one-row modulator);
    # 500 rows in 5 blocks of 100: the parameter row changes inside a wave's 16 rows, and the last wave is ragged
    for V, mod_dtype, wide_mod, pad, blocks, rows, one_row in ((256, np.float32, True, 0, 1, 512, False), (256, np.float32, True, 4, 4, 512, False),
                                                              (256, np.float64, True, 0, 1, 512, False), (256, np.float32, False, 0, 4, 512, False),
                                                              (97, np.float32, True, 3, 1, 512, False), (97, np.float64, False, 0, 4, 512, False),
                                                              (256, np.float32, True, 0, 5, 500, False), (97, np.float64, True, 3, 5, 500, False),
                                                              (256, np.float32, True, 0, 1, 512, True), (97, np.float64, False, 0, 5, 500, True)):
        what = (kind, pos, V, mod_dtype.__name__, wide_mod, pad, blocks, rows, one_row)
        got64, want = abi_case(kind, pos, V, rows, mod_dtype, wide_mod, pad, blocks, one_row, torch.float64)
        got32, _ = abi_case(kind, pos, V, rows, mod_dtype, wide_mod, pad, blocks, one_row, torch.float32)
        if kind == 'Sine':
            e64, e32 = maxerr(got64, want), maxerr(got32, want)
            print('sig_osc_bank_pm Sine', what, 'f64 store', e64, 'f32 store', e32)
            assert e64 < 1e-15, what                                          # the f64 polynomial (test_gpu_eager.py's bound for the f64 store)
            assert e32 <= 1.3e-7, what
        else:
            assert np.array_equal(got64, want), what                          # bit-exact in f64 before the store
            assert np.array_equal(got32, f32(want)), what


@pytest.mark.parametrize('kind', KINDS)
def test_unplugged_index_or_modulator_gives_sig_osc_bank_bits(kind):
    from signals_amd import _native
    rng = np.random.default_rng(1)
    V, rows = 256, 384
    hz, ph = dev(rng.uniform(55, 1760, (1, V))), dev(rng.uniform(0, 1, (1, V)))
    m = dev(rng.uniform(-1, 1, (rows, V)), torch.float32)
    for pos in (0, 50, HOUR):
        for dt in (torch.float32, torch.float64):
            plain = _native.osc_bank(kind, pos, RATE, hz, ph, torch.empty((rows, V), dtype=dt, device='cuda:0'))
            no_index = _native.osc_bank_pm(kind, pos, RATE, hz, ph, None, m, torch.empty((rows, V), dtype=dt, device='cuda:0'))
            no_mod = _native.osc_bank_pm(kind, pos, RATE, hz, ph, dev(np.full((1, V), 2.0)), None,
                                         torch.empty((rows, V), dtype=dt, device='cuda:0'))
            assert torch.equal(plain, no_index) and torch.equal(plain, no_mod), (kind, pos, dt)


# ---------------------------------------------------------------------------------------------- graphs
def draw(V, seed=3):
    rng = np.random.default_rng(seed)
    th = rng.uniform(0, np.pi / 2, V)
    return dict(hertz=rng.uniform(55, 1760, (1, V)), phase=rng.uniform(0, 1, (1, V)), mphase=rng.uniform(0, 1, (1, V)),
                index=rng.uniform(0, I_MAX, (1, V)), cut1=rng.uniform(200, 8000, (1, V)), cut2=rng.uniform(200, 8000, (1, V)),
                gain=rng.uniform(0.2, 1.0, (1, V)), pan=np.stack([np.cos(th), np.sin(th)]),
                env=dict(attack=rng.uniform(0.002, 0.02, (1, V)), decay=rng.uniform(0.01, 0.05, (1, V)), sustain=rng.uniform(0.3, 0.9, (1, V)),
                         release=rng.uniform(0.01, 0.05, (1, V)), gate_on=rng.uniform(0.0, 0.01, (1, V)), gate_off=rng.uniform(0.04, 0.07, (1, V))))


def carrier(kind, p, mod, rmod, index=None, rindex=None):
    from oracle import chain_ref as R
    from signals_amd.chain import ext
    c = getattr(ext, 'PM' + kind)(); c.hertz = fix(p['hertz']); c.phase = fix(p['phase']); c.mod = mod
    c.index = index if index is not None else fix(p['index'])
    ref = PR.PMOsc(kind, R.Fixed(p['hertz']), R.Fixed(p['phase']), rindex if rindex is not None else R.Fixed(p['index']), rmod)
    return c, ref


def graph(which, p, kind='Sine', ratio=1.0, given=None):
    """(GPU node, oracle node, the oracle's PM carrier, rendered width, filtered, the GPU modulator node) of one voice shape;
    `given`: an oracle node that answers the modulator's rows instead of the oracle's own modulator"""
    from oracle import chain_ref as R
    from signals_amd.chain import ext, fx
    V = p['hertz'].shape[1]
    mhz = p['hertz'] * ratio
    m, rm = mkosc('Sine', mhz, p['mphase']), given or R.Osc('Sine', R.Fixed(mhz), R.Fixed(p['mphase']))
    if which == 'bus':                                                        # (a) SumBus(Gain(PMSine(mod=Sine))), stereo pan
        c, rc = carrier('Sine', p, m, rm)
        g = fx.Gain(); g.left = c; g.right = fix(p['gain'])
        b = ext.SumBus(); b.input = g; b.get_state().gains = np.ascontiguousarray(p['pan'])
        rb = R.SumBus(R.Binary('Gain', rc, R.Fixed(p['gain'])), p['pan'])
        return b, rb, rc, 2, False, m
    if which == 'ratio':                                                      # (b) every carrier kind, a Sine modulator at a ratio
        c, rc = carrier(kind, p, m, rm)
        return c, rc, rc, V, False, m
    if which == 'lowpass':                                                    # (c) LowPass(PMSawtooth(mod=Sine))
        c, rc = carrier('Sawtooth', p, m, rm)
        f = fx.LowPass(); f.input = c; f.cutoff = fix(p['cut1'])
        return f, R.Filter('lp', rc, R.Fixed(p['cut1'])), rc, V, True, m
    if which == 'cascade':                                                    # (c) two filters behind a PM carrier
        c, rc = carrier('Sine', p, m, rm)
        f1 = fx.LowPass(); f1.input = c; f1.cutoff = fix(p['cut1'])
        f2 = fx.HighPass(); f2.input = f1; f2.cutoff = fix(p['cut2'])
        return f2, R.Filter('hp', R.Filter('lp', rc, R.Fixed(p['cut1'])), R.Fixed(p['cut2'])), rc, V, True, m
    if which == 'enveloped':                                                  # (d) mod = RingMod(ADSR, Sine), index on a block-rate LFO
        env = ext.ADSR()
        for name, row in p['env'].items():
            setattr(env, name, fix(row))
        x = fx.RingMod(); x.left = env; x.right = m
        ix, rix = lfo(3.1, 0.4 * p['index'], 0.6 * p['index'])                # 0.2 .. 1.0 of the row: below I_MAX
        c, rc = carrier('Sine', p, x, given or R.Binary('RingMod', R.Adsr(**p['env']), rm), ix, rix)
        return c, rc, rc, V, False, x
    if which == 'filtered_mod':                                               # (e) a modulator that is itself filtered
        f = fx.LowPass(); f.input = mkosc('Sawtooth', mhz, p['mphase']); f.cutoff = fix(p['cut2'])
        rf = R.Filter('lp', R.Osc('Sawtooth', R.Fixed(mhz), R.Fixed(p['mphase'])), R.Fixed(p['cut2']))
        c, rc = carrier('Sine', p, f, rf)
        return c, rc, rc, V, True, f
    raise KeyError(which)


def reach_of_jumps(near, pos, N, K):
    """the rows a crossed jump at a near-jump sample can reach behind ONE filter: from its row to the end of every block whose
    [<= 100 context rows | block] window holds it (each block is filtered from zero state, fx.py:85-106)"""
    mask = np.zeros(near.shape, dtype=bool)
    for r, v in zip(*np.nonzero(near)):
        for b in range(K):
            if b * N - CONTEXT <= r < (b + 1) * N:
                mask[max(r, b * N):(b + 1) * N, v] = True
    return mask


def check_route(route, which, pos, N, ks, V=96, **gkw):
    """one route on one graph against eager (fuse=False: bit-equal) and against the oracle within the derived tolerance"""
    from oracle import chain_ref as R
    from signals_amd import specialise
    if route == 'specialise':
        assert specialise.hipcc() is not None
    p = draw(V)
    K = sum(ks)
    node, _, _, C, filtered, _ = graph(which, p, **gkw)
    got = render_batches(node, C, pos, N, ks, **ROUTES[route]).rows
    what = (route, which, pos, N, gkw)
    kind = {'ratio': gkw.get('kind', 'Sine'), 'lowpass': 'Sawtooth'}.get(which, 'Sine')
    scaled = filtered or which == 'bus'
    if route == 'per_node':
        eager = stream(graph(which, p, **gkw)[0], pos, N, K, C)
        assert np.array_equal(got, eager, equal_nan=True), what                # as the docstring of fuse=False promises
    if route == 'per_node' and which != 'filtered_mod':
        # the reference fed the float32 modulator the route itself materialises (position-pure here, so rendered eagerly on its
        # own: block by block, or -- behind filters, whose context requests reach 100 rows per filter either side -- as one range): no
        # modulator deviation, so no mask and no PM factor on the tolerance
        mnode = graph(which, p, **gkw)[5]
        reach = 2 * CONTEXT                                                   # (two filters in series ask for the context of a context)
        lo, hi = (max(pos - reach, 0), pos + K * N + reach) if filtered else (pos, pos + K * N)
        rows = render(mnode, lo, hi - lo, V) if filtered else stream(mnode, pos, N, K, V)
        _, ref, _, _, _, _ = graph(which, p, given=PR.Given(rows, lo), **gkw)
        want = R.render_stream(ref, pos, N, K, C)
        if which == 'ratio' and kind != 'Sine':
            assert np.array_equal(got, f32(want)), what                       # bit-exact
            return
        tol = 1.3e-7 if which == 'ratio' else tolerance(want)
        err = maxerr(got, want if which == 'ratio' else f32(want))
        print('pm route', what, 'max|err|', err, 'tol', tol, 'own modulator, no mask')
        assert err <= tol, (what, err, tol)
        return
    _, ref, rc, _, _, _ = graph(which, p, **gkw)
    want = R.render_stream(ref, pos, N, K, C)
    near = PR.near_jump(kind, np.broadcast_to(rc.cycles(pos, N, K), (K * N, V)))
    assert near.mean() <= 1e-3, (what, near.mean())
    if which == 'bus':
        mask = np.zeros(want.shape, dtype=bool)                               # (a Sine carrier: no jumps)
    elif filtered:
        mask = reach_of_jumps(near, pos, N, K)
        lam = 2e-5 * len(PR.JUMPS[kind]) * near.size
        assert mask.mean() <= (lam + 3.0 * np.sqrt(lam)) * (N + CONTEXT) / near.size, (what, mask.mean(), int(near.sum()))
    else:
        mask = near
    tol = 1e-6 * (1.0 + PR.SLOPE[kind] * I_MAX) * (max(1.0, float(np.abs(want).max())) if scaled else 1.0)
    err = np.abs(got.astype(np.float64) - f32(want).astype(np.float64))
    err[mask] = 0.0
    print('pm route', what, 'max|err|', float(err.max()), 'tol', tol, 'near', float(near.mean()), 'excluded', float(mask.mean()))
    assert float(err.max()) <= tol, (what, float(err.max()), tol)


@pytest.mark.parametrize('pos', [0, HOUR])
@pytest.mark.parametrize('route', list(ROUTES))
def test_two_operator_voice_under_a_stereo_bus(route, pos):
    check_route(route, 'bus', pos, 256, (4, 3))


@pytest.mark.parametrize('pos', [0, HOUR])
@pytest.mark.parametrize('route', list(ROUTES))
@pytest.mark.parametrize('kind', KINDS)
def test_carrier_kinds_and_ratios(kind, route, pos):
    for ratio in (0.5, 1, 2, 3, 3.5, 7):
        check_route(route, 'ratio', pos, 256, (4, 3), kind=kind, ratio=ratio)


@pytest.mark.parametrize('pos', [0, HOUR])
@pytest.mark.parametrize('route', list(ROUTES))
@pytest.mark.parametrize('which', ['lowpass', 'cascade'])
def test_carriers_behind_filters(which, route, pos):
    check_route(route, which, pos, 256, (4, 3), ratio=2)


@pytest.mark.parametrize('pos', [0, HOUR])
@pytest.mark.parametrize('route', list(ROUTES))
def test_enveloped_modulator_with_a_swept_index(route, pos):
    check_route(route, 'enveloped', pos, 256, (4, 3), ratio=2)


@pytest.mark.parametrize('pos', [0, HOUR])
@pytest.mark.parametrize('route', list(ROUTES))
def test_filtered_modulator(route, pos):
    check_route(route, 'filtered_mod', pos, 256, (4, 3), ratio=0.5)


@pytest.mark.parametrize('pos', [0, HOUR])
@pytest.mark.parametrize('route', list(ROUTES))
@pytest.mark.parametrize('which', ['bus', 'lowpass', 'cascade'])
def test_short_blocks(which, route, pos):
    if which == 'cascade' and route == 'per_node':
        # two filters in series with blocks shorter than the context: the per-node schedule cannot batch them (the inner filter's
        # rows come from the reference's after-window cache entries) and says so; the eager path answers, checked against the oracle
        from oracle import chain_ref as R
        from signals_amd.engine import NotBatchable
        p = draw(96)
        with pytest.raises(NotBatchable, match='cascaded filters with block size <= 100'):
            render_batches(graph(which, p, ratio=2)[0], 96, pos, 64, (5, 6), fuse=False)
        node, ref, _, _, _, _ = graph(which, p, ratio=2)
        want = R.render_stream(ref, pos, 64, 11, 96)
        tol = 1e-6 * (1.0 + PR.SLOPE['Sine'] * I_MAX) * max(1.0, float(np.abs(want).max()))
        assert maxerr(stream(node, pos, 64, 11, 96), f32(want)) <= tol
        return
    check_route(route, which, pos, 64, (5, 6), ratio=2)


# ---------------------------------------------------------------------------------------------- the eager node, and what ran
@pytest.mark.parametrize('pos', [0, 50, HOUR])
@pytest.mark.parametrize('kind', KINDS)
def test_eager_node_against_the_reference(kind, pos):
    from oracle import chain_ref as R
    V, N = 200, 256
    p = draw(V, seed=8)
    mhz = p['hertz'] * 2
    for frames in (N, 1):                                                     # a block (float32) and a one-frame request (float64, one row)
        got = render(graph('ratio', p, kind=kind, ratio=2)[0], pos, frames, V)
        assert got.shape == (frames, V) and got.dtype == (np.float32 if frames > 1 else np.float64)
        rows = render(mkosc('Sine', mhz, p['mphase']), pos, frames, V)        # the modulator block the node is handed
        ref = PR.PMOsc(kind, R.Fixed(p['hertz']), R.Fixed(p['phase']), R.Fixed(p['index']), PR.Given(rows, pos))
        want = R.render(ref, pos, frames, V)
        if kind == 'Sine':
            assert maxerr(got, want) <= (1.3e-7 if frames > 1 else 1e-15), (kind, pos, frames)
        else:
            assert np.array_equal(got, f32(want) if frames > 1 else want), (kind, pos, frames)


@pytest.mark.parametrize('kind', KINDS)
def test_unplugged_modulator_or_index_is_the_plain_oscillator_bit_for_bit(kind):
    from signals_amd.chain import ext
    V, N = 64, 256
    p = draw(V, seed=9)
    for pos in (0, HOUR):
        plain = render(mkosc(kind, p['hertz'], p['phase']), pos, N, V)
        a = getattr(ext, 'PM' + kind)(); a.hertz = fix(p['hertz']); a.phase = fix(p['phase']); a.index = fix(p['index'])
        b = getattr(ext, 'PM' + kind)(); b.hertz = fix(p['hertz']); b.phase = fix(p['phase']); b.mod = mkosc('Sine', p['hertz'])
        assert np.array_equal(render(a, pos, N, V), plain) and np.array_equal(render(b, pos, N, V), plain), (kind, pos)


def test_launches_of_each_route():
    p = draw(128)
    for route, kw in ROUTES.items():
        _, names, r = render_batches(graph('bus', p)[0], 2, 0, 256, (4,), names=True, **kw)
        if route == 'per_node':
            assert any(n.startswith('osc_bank_pm[Sine]') for n in names) and not any(n.startswith('voice_program') for n in names), names
        else:
            assert any(n.startswith('voice_program_bus[Osc,OscPM') for n in names), (route, names)
            assert not any(n.startswith(('osc_bank', 'sum_bus')) for n in names), (route, names)
            assert any('*specialised' in n for n in names) == bool(r.specialise), (route, names)      # (SIG_SPECIALISE=1 turns it on for every route)
    names = render_batches(graph('enveloped', p)[0], 128, 0, 256, (4,), names=True, fuse=False).names      # a swept index: per-block rows on the per-node schedule
    assert any(n.startswith('osc_bank_pm[Sine,per-block]') for n in names), names


def test_a_pm_oscillator_in_a_control_path_keeps_the_eager_path():
    from signals_amd.chain import ext, fx
    from signals_amd.engine import BatchRenderer, NotBatchable
    V = 32
    p = draw(V, seed=5)
    pm = ext.PMSine(); pm.hertz = fix([[3.0]]); pm.index = fix([[1.0]]); pm.mod = mkosc('Sine', [[1.0]])
    g = fx.Gain(); g.left = mkosc('Sawtooth', p['hertz'], p['phase']); g.right = pm
    with pytest.raises(NotBatchable, match='phase-modulation oscillator'):
        BatchRenderer(g, V, RATE).render(0, 256, 2)
    assert stream(g, 0, 256, 2, V).shape == (512, V)
