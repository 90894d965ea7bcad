"""The additive oscillator without a GPU: the node API of ext.Additive with its state validation and spectrum helpers, the numpy
restatement (tests/additive_reference.py) at the band limit's edges, the census of the kernel cases the GPU test runs,
sig_osc_bank_additive's export, declaration and argument checks, and how the engine's planner schedules the node: one
sig_osc_bank_additive launch per batch, no OscTable word and no fused kernel on any renderer setting, a plain Wavetable planned as
before, the inherited refusal in a control path."""
import ctypes
import pathlib
import types

import numpy as np
import pytest

from signals_amd import SignalFlags, _native
from signals_amd.chain import BadStateValue
from signals_amd.chain import ext, fixed, fx, osc

import additive_reference as AR

ROOT = pathlib.Path(__file__).resolve().parent.parent
INV = 1     # hipErrorInvalidValue
RATE, V = 48000, 8


@pytest.fixture(autouse=True)
def _cpu_device():
    from signals_amd import runtime
    old = runtime._device
    runtime.set_device('cpu')
    yield
    runtime._device = old


@pytest.fixture(scope='module')
def lib():
    if not _native.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return _native.lib()


def fix(v):
    f = fixed.Fixed()
    f.get_state().value = np.array(v, ndmin=2, dtype=float)
    return f


def row(lo, hi, n=V):
    return np.linspace(lo, hi, n).reshape(1, n)


def additive_node(table=None, hertz=None, phase=None, select=None):
    a = ext.Additive()
    if table is not None:
        a.get_state().table = table
    a.hertz = fix(row(110, 880)) if hertz is None else (hertz if not isinstance(hertz, (list, np.ndarray)) else fix(hertz))
    if phase is not None:
        a.phase = fix(phase)
    if select is not None:
        a.select = fix(select)
    return a


# ---------------------------------------------------------------------------------------------- the node
def test_the_node_is_a_wavetable_with_a_validator_and_a_default_of_its_own():
    assert issubclass(ext.Additive, ext.Wavetable)
    a = ext.Additive()
    assert a.flags() & SignalFlags.GENERATOR
    assert np.array_equal(a.get_state().table, [[1.0]])                       # one column, H = 1, amplitude 1: a sine
    assert np.array_equal(ext.Wavetable().get_state().table, [[0.0], [1.0], [0.0], [-1.0]])     # the parent keeps its own
    assert {p for p in ('hertz', 'phase', 'select')} <= set(dir(a))
    st = a.get_state()
    for good in (np.ones((1, 1)), np.ones((64, 256)), np.ones((1, 16384)), np.ones((3, 5)), -np.ones((7, 2)),
                 np.arange(6).reshape(3, 2), np.ones((64, 1), dtype=np.float32)):
        st.table = good
        assert st.table is good
    for bad in (np.ones((0, 1)), np.ones((65, 1)), np.ones((64, 257)), np.ones((1, 16385)), np.ones(8), np.ones((2, 2, 2)),
                np.ones((4, 1), dtype=complex), [[1.0]], None, np.ones((4, 0)), np.array([[np.nan]]), np.array([[np.inf], [1.0]])):
        with pytest.raises(BadStateValue):
            st.table = bad
    with pytest.raises(BadStateValue):
        ext.Wavetable().get_state().table = np.ones((3, 1))                   # the parent's power-of-two rule is the parent's still
    st.table = np.arange(6).reshape(3, 2)                                     # integers convert as they do for Wavetable
    assert a.resident_table().dtype.is_floating_point and tuple(a.resident_table().shape) == (3, 2)
    assert a.resident_table().tolist() == [[0.0, 1.0], [2.0, 3.0], [4.0, 5.0]]


def test_select_clips_and_a_nan_is_column_zero():
    assert AR.column([[-3.0, -0.5, 0.0, 0.99, 1.0, 1.5, 2.0, 2.9, 3.0, 1e9, np.nan, -np.inf, np.inf]], 3).tolist() == \
        [[0, 0, 0, 0, 1, 1, 2, 2, 2, 2, 0, 0, 2]]
    table = np.array([[1.0, 0.0, 0.5]])                                       # H = 1: column w plays a sine of amplitude table[0, w]
    t = np.array([[0.25]])
    for sel, amp in ((-1.0, 1.0), (0.7, 1.0), (1.2, 0.0), (2.0, 0.5), (17.0, 0.5), (np.nan, 1.0)):
        assert AR.spectrum_sum(table, t, [[100.0]], [[sel]])[0, 0] == pytest.approx(amp, abs=1e-15)


# ---------------------------------------------------------------------------------------------- the band limit, on the restatement
def test_k_and_g_at_the_edges():
    H = 12
    hz = lambda nf: (0.5 * RATE) / nf
    nf, k, g = AR.band_limit(hz(10.3), H)
    assert k == 10 and g == nf - 10 and abs(g - 0.3) < 1e-12
    nf, k, g = AR.band_limit(2400.0, H)                                       # nf exactly 10.0: partial 10 sits AT rate / 2 and is gone
    assert nf == 10.0 and k == 9 and g == 1.0
    nf, k, g = AR.band_limit(hz(0.7), H)                                      # above rate / 2: nothing
    assert k == 0
    nf, k, g = AR.band_limit(0.0, H)
    assert np.isinf(nf) and k == H and g == 1.0
    nf, k, g = AR.band_limit(hz(12.4), H)                                     # H < nf < H + 1: every partial, the top one fading in
    assert k == H and g == nf - H and 0.39 < g < 0.41
    nf, k, g = AR.band_limit(hz(13.0), H)
    assert k == H and g == 1.0
    assert AR.band_limit(np.inf, H)[1] == 0 and AR.band_limit(-np.inf, H)[1] == 0 and AR.band_limit(RATE / 2.0, H)[1] == 0
    assert np.isnan(AR.band_limit(np.nan, H)[1])
    assert AR.band_limit(-hz(10.3), H)[1] == 10                               # |hertz|


def test_silence_nan_and_the_sign_of_hertz():
    table = AR.spectra(8, 1)
    t = np.linspace(0.0, 3.0, 50)[:, None]
    assert np.array_equal(AR.spectrum_sum(table, t, [[30000.0]]), np.zeros((50, 1)))                 # k = 0: exactly 0.0 ...
    assert np.array_equal(AR.spectrum_sum(table, t * np.nan, [[np.inf]]), np.zeros((50, 1)))         # ... whatever the phase
    assert not np.signbit(AR.spectrum_sum(table, t, [[30000.0]])).any()
    assert np.isnan(AR.spectrum_sum(table, t, [[np.nan]])).all()
    assert np.isnan(AR.spectrum_sum(table, t + np.inf, [[440.0]])).all()      # k >= 1 and a non-finite phase
    # hertz < 0 mirrors: the same k and g, and sin is odd in t
    up = AR.additive(table, 100, 64, [[3100.0]], [[0.0]])
    down = AR.additive(table, 100, 64, [[-3100.0]], [[0.0]])
    assert np.max(np.abs(up + down)) < 1e-12 and np.max(np.abs(up)) > 0.1


def test_the_output_is_continuous_in_hertz_where_a_partial_drops_out():
    """hertz one float64 ulp either side of an integer nf: the partial that leaves has weight g = O(ulp) on one side and is absent on
    the other, and the one below it goes from g = 1 - O(ulp) to 1: the two outputs differ by a few ulps of nf times |a_k| (plus the
    phase's own move, hertz * ulp, times the slope -- taken out by holding t fixed)"""
    H = 16
    table = np.ones((H, 1))
    t = np.linspace(0.01, 0.99, 197)[:, None]
    for n in (3, 7, 10, 16):
        centre = (0.5 * RATE) / n
        lo, hi = np.nextafter(centre, 0.0), np.nextafter(centre, np.inf)
        klo, khi = AR.band_limit(lo, H)[1], AR.band_limit(hi, H)[1]
        assert klo == n and khi == n - 1, (n, klo, khi)                       # the cut-off lies between the two
        a, b = AR.spectrum_sum(table, t, [[lo]]), AR.spectrum_sum(table, t, [[hi]])
        assert np.max(np.abs(a - b)) <= 8 * np.spacing(float(n)) * 1.0, (n, np.max(np.abs(a - b)))


# ---------------------------------------------------------------------------------------------- spectra
@pytest.mark.parametrize('kind', ['Sawtooth', 'Square', 'Triangle'])
def test_the_spectra_converge_to_the_oscillators_at_the_same_phase(kind):
    from oracle import chain_ref as R
    helper = {'Sawtooth': ext.Additive.sawtooth, 'Square': ext.Additive.square, 'Triangle': ext.Additive.triangle}[kind]
    t = np.linspace(0.0, 2.0, 801)[:, None]
    # 0.05 cycles clear of the edges: the jumps at multiples of 1/2, the Triangle's corners at 1/4 and 3/4 (where np.sign's zero also
    # leaves the oscillator an isolated 0.0 at exactly 3/4)
    d = np.abs(np.mod(t, 0.5) - 0.25)[:, 0]
    away = d > 0.05 if kind == 'Triangle' else d < 0.2
    want = R.osc_wave(kind, t)
    errs = []
    for H in (8, 64):
        col = helper(H)
        assert col.shape == (H, 1) and col.dtype == np.float64
        got = np.sin(2.0 * np.pi * t * np.arange(1, H + 1)[None, :]) @ col
        errs.append(np.max(np.abs(got - want)[away]))
    # away from an edge the tail of a 1 / h series is bounded by ~ 1 / (pi H sin(pi d)) at distance d, of a 1 / h^2 series by 1 / H
    assert errs[1] < errs[0] and errs[1] < (0.004 if kind == 'Triangle' else 0.08), (kind, errs)
    assert errs[0] < 0.5
    for bad in (0, 65, 2.5, True):
        with pytest.raises(ValueError):
            helper(bad)


def test_cycle_inverts_a_column_through_the_fft():
    rng = np.random.default_rng(3)
    for H, T in ((1, 4), (7, 64), (64, 256), (64, 2048)):
        col = rng.uniform(-1, 1, (H, 1))
        cyc = ext.Additive.cycle(col, T)
        assert cyc.shape == (T, 1)
        spec = np.fft.rfft(cyc[:, 0]) / (T / 2.0)                             # sin(2 pi h i / T) has the coefficient -j a_h
        assert np.max(np.abs(-spec.imag[1:H + 1] - col[:, 0])) < 1e-12 and np.max(np.abs(spec.real)) < 1e-12
        assert np.max(np.abs(spec.imag[H + 1:])) < 1e-12
    wt = ext.Wavetable()
    wt.get_state().table = ext.Additive.cycle(ext.Additive.sawtooth(16), 2048)       # what a Wavetable takes
    with pytest.raises(ValueError):
        ext.Additive.cycle(np.ones(4), 1)


def test_the_fold_back_of_an_additive_saw_is_the_float32_noise_floor():
    """tests/test_blep_host.py's measurement -- 4096 frames from position 1000 at hertz = 48000 * 37 / 1024 (1734 Hz) and phase 0.1234,
    an unwindowed rfft, power between the harmonics over power in them -- on Additive.sawtooth(64): 13 partials are kept (g = 0.84 on
    the 13th) and nothing folds.  -262.5 dB on the restatement's float64 rows (the transform's own rounding), -151.7 dB once the rows
    are rounded to the float32 the node stores; osc.Sawtooth has -13.3 dB there and BlepSawtooth -28.6 dB"""
    import blep_reference as BR
    hz, ph = np.array([[48000 * 37 / 1024]]), np.array([[0.1234]])
    assert AR.band_limit(hz, 64)[1] == 13
    x = AR.additive(ext.Additive.sawtooth(64), 1000, 4096, hz, ph)[:, 0]
    exact, stored = BR.alias_ratio_db(x), BR.alias_ratio_db(x.astype(np.float32))
    print('alias / harmonic, Additive.sawtooth(64): float64 rows', exact, 'float32 rows', stored)
    assert exact < -240.0 and abs(stored - -151.7) < 1.0, (exact, stored)


# ---------------------------------------------------------------------------------------------- the case table
def test_census_of_the_kernel_cases():
    cases = AR.cases()
    assert len({c['name'] for c in cases}) == len(cases)
    ks = lambda c: AR.band_limit(c['hertz'], c['H'])[1]
    lanes_per_wave = lambda c: 64 * (4 if c['voices'] % 4 == 0 else 1)
    three = [c for c in cases if any(len(set(ks(c)[0, w:w + lanes_per_wave(c)][~np.isnan(ks(c)[0, w:w + lanes_per_wave(c)])])) >= 3
                                     for w in range(0, c['voices'], lanes_per_wave(c)))]
    assert three, 'a wave whose lanes hold at least three different k'
    assert any((ks(c) == 0).any() and (ks(c) == c['H']).any() for c in cases), 'k = 0 and k = H lanes in one launch'
    assert any(c['K'] > 1 and c['hertz'].shape[0] == c['K'] and (np.ptp(ks(c), axis=0) >= 2).any() for c in cases), \
        'a per-block sweep that crosses two cut-offs inside a batch'
    assert any((np.abs(c['hertz']) > 0).any() and (np.abs(c['hertz'][np.abs(c['hertz']) > 0]) < 1.0).any() for c in cases), 'a sub-audio hertz'
    assert any(c['position'] >= AR.HOUR for c in cases), 'a position >= one hour'
    assert any(np.isnan(c['hertz']).any() for c in cases) and any(np.isnan(c['select']).any() for c in cases)
    assert any((c['select'][~np.isnan(c['select'])] >= c['W']).any() and (c['select'][~np.isnan(c['select'])] < 0).any() for c in cases)
    assert {c['voices'] for c in cases} >= {1, 3, 64, 65, 70, 260}
    assert {(c['N'], c['K']) for c in cases} >= {(n, k) for n in (17, 64, 100) for k in (1, 3)}
    assert {c['position'] for c in cases} >= {0, 37, AR.HOUR}
    assert {c['H'] for c in cases} >= {1, 2, 63, 64} and {c['W'] for c in cases} >= {1, 3}
    assert any((c['N'] * c['K']) % 2 for c in cases), 'a row count that is no multiple of the rows a lane carries together'
    for c in cases:
        assert c['table'].shape == (c['H'], c['W']) and c['hertz'].shape[1] == c['voices']
        assert all(x.shape[0] in (1, c['K']) for x in (c['hertz'], c['phase'], c['select']))
    # the pitches of the mix: both sides of rate / (2 H), both sides of rate / 2
    c = next(c for c in cases if c['H'] == 64 and c['voices'] >= 16)
    k = ks(c)[0]
    assert {0.0, 63.0, 64.0} <= set(k[~np.isnan(k)])
    g = AR.band_limit(c['hertz'], 64)[2][0]
    assert ((k == 64) & (g < 1e-6)).any() and ((k == 63) & (g > 1 - 1e-6) & (g < 1)).any()       # the top partial just in, just out


def test_the_restatement_renders_the_cases_inside_the_gain_bound():
    for c in AR.cases()[:4]:
        want = AR.render_case(c)
        assert want.shape == (c['N'] * c['K'], c['voices']) and want.dtype == np.float64
        finite = want[~np.isnan(want)]
        assert np.max(np.abs(finite), initial=0.0) <= AR.gain_bound(c['table']) + 1e-12
        nan_voice = np.isnan(np.broadcast_to(c['hertz'], (c['hertz'].shape[0], c['voices']))).any(axis=0)
        assert np.array_equal(np.isnan(want).any(axis=0), nan_voice)


# ---------------------------------------------------------------------------------------------- C ABI
def test_entry_point_is_exported_and_declared(lib):
    assert 'sig_osc_bank_additive' in _native.EXPORTS
    raw = ctypes.CDLL(str(_native.LIB_PATH))
    assert raw.sig_osc_bank_additive is not None
    assert lib.sig_abi_version() == 7 and _native.ABI_VERSION == 7           # additive
    header = (ROOT / 'include' / 'signals_amd.h').read_text()
    assert 'int sig_osc_bank_additive(' in header and '#define SIG_ABI_VERSION 7' in header
    assert 'SIG_ADDITIVE_MAX_PARTIALS = 64' in header and _native.ADDITIVE_MAX_PARTIALS == 64
    assert 'sig_osc_bank_additive' in (ROOT / 'INTEGRATION.md').read_text()
    assert _native._ARGTYPES['sig_osc_bank_additive'] == _native._ARGTYPES['sig_osc_bank_table']


def test_additive_argument_errors_do_not_reach_the_device(lib):
    p = 64                                                                    # (never dereferenced: every call fails its checks)
    args = dict(position=4096, step=1, rate=48000, rows=512, voices=8, rpp=256,
                hertz=p, hs=1, hrs=8, phase=p, ps=1, prs=8, select=p, ss=1, srs=8,
                table=p, H=16, W=4, out=p, odt=0, old=8, stream=None)

    def call(**over):
        a = dict(args, **over)
        return lib.sig_osc_bank_additive(*(a[k] for k in args))
    assert call(table=None) == INV and call(out=None) == INV and call(hertz=None) == INV      # null pointers
    assert call(H=0) == INV and call(H=65) == INV and call(H=-1) == INV and call(W=0) == INV and call(W=-1) == INV
    assert call(H=64, W=257) == INV and call(H=1, W=16385) == INV and call(H=64, W=2 ** 30) == INV     # H * W over the cap
    assert call(old=7) == INV and call(old=0) == INV                          # rows narrower than the voices
    for name in ('hs', 'ps', 'ss'):
        assert call(**{name: 2}) == INV and call(**{name: -1}) == INV         # strides other than 0 or 1
    for name in ('hrs', 'prs', 'srs'):
        assert call(**{name: -1}) == INV
    assert call(rows=-1) == INV and call(voices=-1) == INV and call(rate=0) == INV and call(position=-1) == INV
    assert call(step=0) == INV and call(rpp=-1) == INV and call(odt=2) == INV
    # accepted, nothing to launch: no rows, no voices -- at every limit, with the optional ports unplugged
    assert call(rows=0) == 0 and call(voices=0, old=0) == 0
    assert call(rows=0, H=64, W=256) == 0 and call(rows=0, H=1, W=16384) == 0 and call(rows=0, H=1, W=1) == 0 and call(rows=0, H=63, W=3) == 0
    assert call(rows=0, phase=None, select=None) == 0 and call(rows=0, odt=1) == 0 and call(rows=0, step=256, rpp=1) == 0


def test_the_wrapper_checks_the_table():
    import torch
    hz, out = torch.zeros((1, 4), dtype=torch.float64), torch.zeros((8, 4))
    for bad in (torch.zeros((65, 1)), torch.zeros((0, 1)), torch.zeros((64, 257)), torch.zeros((4, 2), dtype=torch.float64),
                torch.zeros(4), None, torch.zeros((4, 4)).t()):
        with pytest.raises(_native.NativeError):
            _native.osc_bank_additive(0, RATE, hz, None, None, bad, out)


# ---------------------------------------------------------------------------------------------- planning
class _Recorder:
    """stands in for engine.KernelTimer: the launch labels in order"""
    region = False

    def __init__(self):
        self.names = []

    def launch(self, name, fn, **meta):
        self.names.append(name)
        return fn()


@pytest.fixture
def stubbed(monkeypatch):
    """every entry point of the library answers 0 without touching its arguments: the planner runs on CPU tensors"""
    class Lib:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            def entry(*a):
                self.calls.append((name, a))
                return 0
            return entry
    one = Lib()
    monkeypatch.setattr(_native, 'lib', lambda: one)
    monkeypatch.setattr(_native, '_gpu', lambda *a: None)
    monkeypatch.setattr(_native, '_stream', lambda t: 0)
    return one


# the launches that would hold the oscillator itself: the fused voice kernels and the voice program.  (The filter-and-bus pass,
# biquad_bus, reads the oscillator's stored rows like the cold-start filter does: the nodes around the oscillator keep their routes.)
FUSED = ('fused', 'latency', 'cascade', 'steady', 'walk', 'voice_program')
SETTINGS = ({}, {'fuse_program': 'always'}, {'fuse': False}, {'mixed_programs': True}, {'fuse_program': 'always', 'mixed_programs': True},
            {'fuse_program': 'always', 'specialise': True}, {'fuse_program': 'always', 'mixed_programs': True, 'specialise': True})
TABLE = AR.spectra(12, 3)


def sweep():
    """a block-rate pitch envelope: Mix of an LFO and a constant"""
    o = osc.Sine(); o.hertz = fix([[0.7]])
    m = fx.Mix(); m.left = o; m.right = fix(row(110, 880)); m.mix = fix([[0.01]])
    return m


def voice(shape, modulated=False, cls=None):
    a = additive_node(TABLE, hertz=sweep() if modulated else None, phase=row(0, 0.9), select=row(0, 2.9))
    if cls is ext.Wavetable:
        a = ext.Wavetable(); a.get_state().table = np.zeros((8, 3)); a.hertz = fix(row(110, 880)); a.select = fix(row(0, 2.9))
    if shape == 'alone':
        return a, V
    lp = fx.LowPass(); lp.input = a; lp.cutoff = fix(row(500, 5000))
    if shape == 'lowpass':
        return lp, V
    b = ext.SumBus(); b.input = lp
    return b, 1


@pytest.mark.parametrize('shape', ['alone', 'lowpass', 'lowpass_bus'])
def test_one_additive_launch_per_batch_on_every_renderer_setting(stubbed, shape):
    """Additive [-> LowPass [-> SumBus]]: exactly one sig_osc_bank_additive call per batch and no sig_osc_bank_table call; no voice
    program and no fused kernel, whatever `fuse_program`, `mixed_programs` or `specialise` is"""
    from signals_amd.engine import BatchRenderer
    others = {'alone': (set(),), 'lowpass': ({'biquad_coldstart[lp]'},),
              'lowpass_bus': ({'biquad_coldstart[lp]', 'sum_bus'}, {'biquad_bus[lp]'})}[shape]
    for kw in SETTINGS:
        for modulated, label in ((False, 'osc_bank_additive[Additive12]'), (True, 'osc_bank_additive[Additive12,per-block]')):
            top, C = voice(shape, modulated)
            rec = _Recorder()
            stubbed.calls.clear()
            r = BatchRenderer(top, C, RATE, timer=rec, **kw)
            r.render(0, 256, 3)
            r.render(768, 256, 2)                                             # continuing
            r.render(8192, 256, 2)                                            # fresh
            assert not any(word in n for n in rec.names for word in FUSED), (kw, rec.names)
            banks = [n for n in rec.names if n.startswith('osc_bank') and 'block-rate' not in n]      # (not the sweep's own LFO)
            called = [name for name, _ in stubbed.calls]
            if shape == 'alone' or not modulated:
                assert banks == [label] * 3, (kw, rec.names)                  # one per batch
                assert called.count('sig_osc_bank_additive') == 3
            else:                                                             # (a swept node behind a filter also renders its own history block)
                assert set(banks) == {label} and len(banks) >= 3, (kw, rec.names)
                assert called.count('sig_osc_bank_additive') == len(banks)
            assert 'sig_osc_bank_table' not in called and not any(n.startswith('sig_voice_program') for n in called), (kw, called)
            rest = {n for n in rec.names if not n.startswith('osc_bank') and 'block-rate' not in n and not n.startswith('control_program')}
            assert rest in others, (kw, modulated, rec.names)


def test_the_launch_carries_the_rows_and_the_table(stubbed):
    from signals_amd.engine import BatchRenderer
    top, _ = voice('alone', modulated=True)
    BatchRenderer(top, V, RATE).render(4096, 256, 3)
    (a,) = [a for name, a in stubbed.calls if name == 'sig_osc_bank_additive']
    assert a[:6] == (4096, 1, RATE, 768, V, 256)
    hertz, phase, select = (a[6 + 3 * k:9 + 3 * k] for k in range(3))
    assert hertz[0] is not None and hertz[1:] == (1, V)                       # per-block rows of the modulated port: K rows, V apart
    assert phase[0] is not None and phase[1:] == (1, 0) and select[0] is not None and select[1:] == (1, 0)
    assert a[15] == top.resident_table().data_ptr() and a[16:18] == (12, 3)
    assert a[19] == _native.F32 and a[20] >= V
    # constant controls behind a filter: one launch over history and blocks alike, one parameter row
    top, _ = voice('lowpass')
    stubbed.calls.clear()
    BatchRenderer(top, V, RATE, fuse=False).render(4096, 256, 2)
    (a,) = [a for name, a in stubbed.calls if name == 'sig_osc_bank_additive']
    assert a[:6] == (4096 - 100, 1, RATE, 100 + 512, V, 0)                     # the filter's 100 context rows are simply rendered
    # the eager node: the same entry, float64 for a one-frame request
    stubbed.calls.clear()
    import helpers
    node = additive_node(TABLE, phase=row(0, 0.9))
    assert helpers.render(node, 50, 1, V).dtype == np.float64 and helpers.render(node, 50, 64, V).dtype == np.float32
    assert [name for name, _ in stubbed.calls] == ['sig_osc_bank_additive'] * 2
    assert stubbed.calls[0][1][:6] == (50, 1, RATE, 1, V, 0) and stubbed.calls[0][1][19] == _native.F64


def test_the_voice_program_declines_a_graph_with_the_node():
    from signals_amd.engine import _NoProgram, _VoiceProgram
    for shape in ('alone', 'lowpass', 'lowpass_bus'):
        top, _ = voice(shape)
        inner = top.input.sig if shape == 'lowpass_bus' else top
        for mixed in (False, True):
            assert _VoiceProgram.compile(None, inner, V, min_nodes=1, mixed=mixed) is None
            with pytest.raises(_NoProgram, match='an additive oscillator has no voice-program word'):
                _VoiceProgram(None, inner, V, mixed=mixed)


def test_a_plain_wavetable_still_emits_its_word_and_plans_as_before(stubbed):
    from signals_amd.engine import BatchRenderer, _VoiceProgram
    top, _ = voice('lowpass', cls=ext.Wavetable)
    prog = _VoiceProgram.compile(None, top, V)
    assert prog is not None and [op for op, *_ in prog.code] == ['OscTable', 'Filter']
    rec = _Recorder()
    BatchRenderer(top, V, RATE, timer=rec, fuse_program='always').render(0, 256, 3)
    assert any(n.startswith('voice_program[OscTable,Filter]') for n in rec.names), rec.names
    rec = _Recorder()
    stubbed.calls.clear()
    BatchRenderer(top, V, RATE, timer=rec, fuse=False).render(0, 256, 3)
    assert [n for n in rec.names if n.startswith('osc_bank')] == ['osc_bank_table[Table]'], rec.names
    called = [name for name, _ in stubbed.calls]
    assert called.count('sig_osc_bank_table') == 1 and 'sig_osc_bank_additive' not in called


def test_the_fused_matchers_take_an_osc_only():
    """the closed-form, row-walker and cascade kernels match `osc.Osc`: an Additive in the oscillator's place leaves the graph one
    kernel per node where the same graph over osc.Sawtooth fuses"""
    assert not issubclass(ext.Additive, osc.Osc)
    from signals_amd.engine import _KNOWN_TYPES, _audio_ports, _control_ports, _foreign, _is_pure, _modulated
    a = additive_node(TABLE)
    assert not _foreign(a) and any(issubclass(ext.Additive, k) for k in _KNOWN_TYPES)
    assert _control_ports(a) == [a.hertz, a.phase, a.select] and _audio_ports(a) == []
    assert not _modulated(a) and _is_pure(a, {}) and _modulated(additive_node(TABLE, hertz=sweep()))


def test_the_fused_kernels_run_for_an_osc_and_not_for_the_node(stubbed):
    """LowPass(x) and SumBus(LowPass(x)): over osc.Sawtooth the fused voice kernels take them, over the node never"""
    from signals_amd.engine import BatchRenderer

    def build(source, bus):
        lp = fx.LowPass(); lp.input = source; lp.cutoff = fix(row(500, 5000))
        if not bus:
            return lp, V
        b = ext.SumBus(); b.input = lp; b.get_state().gains = np.ones((2, V))
        return b, 2
    for bus in (False, True):
        saw = osc.Sawtooth(); saw.hertz = fix(row(110, 880))
        rec = _Recorder()
        BatchRenderer(*build(saw, bus), RATE, timer=rec).render(0, 256, 4)
        assert any(n.startswith('fused') for n in rec.names), rec.names                   # the plain oscillator fuses ...
        rec = _Recorder()
        BatchRenderer(*build(additive_node(TABLE), bus), RATE, timer=rec).render(0, 256, 4)
        assert not any(word in n for n in rec.names for word in FUSED), rec.names        # ... the additive one never
        assert [n for n in rec.names if n.startswith('osc_bank')] == ['osc_bank_additive[Additive12]'], rec.names


def test_an_additive_in_a_control_path_is_refused_with_the_inherited_reason():
    from signals_amd.engine import BatchRenderer, NotBatchable, _Batch, _ControlProgram
    a = additive_node(TABLE, hertz=[[3.0]])
    with pytest.raises(NotBatchable, match=r'Additive in a control path: a wavetable oscillator has no block-rate program \(the eager node serves '
                                           r'one-frame requests\)'):
        _ControlProgram((a,), 4, channels=1)
    batch = _Batch(types.SimpleNamespace(rate=RATE), 0, 256, 4, False)
    with pytest.raises(NotBatchable, match=r'Additive in a control path: a wavetable oscillator has no block-rate schedule'):
        batch._control_node(a, 'cutoff')
    saw = osc.Sawtooth(); saw.hertz = fix(row(110, 880))
    lp = fx.LowPass(); lp.input = saw; lp.cutoff = a
    with pytest.raises(NotBatchable, match='a wavetable oscillator has no block-rate'):
        BatchRenderer(lp, V, RATE).render(0, 256, 2)
