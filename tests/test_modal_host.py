"""The modal resonator bank without a GPU: the state's validator and the mode-set presets, the numpy restatement against its
np.longdouble twin on every kernel case, the C entry's export, constants and refusals (no call reaches a device), and the batched
engine's planning -- one sig_modal_bank launch per batch on every renderer setting, no voice program, NotBatchable inside a control
path.

The restatement against its twin: every sample within 1e-6 * max(1, A), A the largest set's sum of |a| -- the kernel's own bar.  The
difference grows with the position, because the rounding of n / rate enters the phase (it is part of the definition); the worst figure
per case is printed."""
import ctypes
import pathlib
import types

import numpy as np
import pytest
import torch

from signals_amd import SignalFlags, _native
from signals_amd.chain import BadStateValue, BlockCachingEmitter
from signals_amd.chain import ext, fixed, fx, osc

import modal_reference as MR

ROOT = pathlib.Path(__file__).resolve().parent.parent
INV = 1     # hipErrorInvalidValue
RATE, V = 48000, 8
CASES = MR.cases()


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


def modal_node(modes=None, hertz=440.0, gate_on=None, damp=None, select=None):
    n = ext.Modal()
    if modes is not None:
        n.get_state().modes = np.asarray(modes)
    for name, value in (('hertz', hertz), ('gate_on', gate_on), ('damp', damp), ('select', select)):
        if value is not None:
            setattr(n, name, value if not isinstance(value, (np.ndarray, list, float, int)) else fix(value))
    return n


# ---------------------------------------------------------------------------------------------- the node's state and presets
def test_node_api():
    n = ext.Modal()
    assert isinstance(n, BlockCachingEmitter) and SignalFlags.GENERATOR in n.flags()
    assert [p for p in ('hertz', 'gate_on', 'damp', 'select') if hasattr(ext.Modal, p)] == ['hertz', 'gate_on', 'damp', 'select']
    assert np.array_equal(n.get_state().modes, [[1.0, 1.0, 1.0]])             # a one-second sine ping
    for phrase in ('voice-program word', 'control path', 'frame-rate ports', 'cosine term', 'strike velocity', 'input signal',
                   'more than 64 modes', 'ELAPSED TIME', 'negative damp', 'silences the voice'):
        assert phrase in ext.Modal.__doc__, phrase


BAD = {'(M, 2)': np.ones((4, 2)), 'M = 65': np.ones((65, 3)), 'W * M = 2049': np.ones((2049, 1, 3)),
       'a negative ratio': np.array([[1.0, 1.0, 1.0], [-0.5, 1.0, 1.0]]), 't60 = 0': np.array([[1.0, 1.0, 0.0]]),
       'a NaN amplitude': np.array([[1.0, np.nan, 1.0]]), 'an infinite ratio': np.array([[np.inf, 1.0, 1.0]]),
       'a NaN t60': np.array([[1.0, 1.0, np.nan]]), 'a negative t60': np.array([[1.0, 1.0, -1.0]]), '1-D': np.ones(3),
       '4-D': np.ones((1, 1, 1, 3)), 'no modes': np.ones((0, 3)), 'a list': [[1.0, 1.0, 1.0]], 'complex': np.ones((2, 3), dtype=complex)}


@pytest.mark.parametrize('bad', list(BAD))
def test_modes_validation_refuses(bad):
    n = ext.Modal()
    with pytest.raises(BadStateValue, match=r'ratio >= 0, amplitude, t60 > 0'):
        n.get_state().modes = BAD[bad]
    assert np.array_equal(n.get_state().modes, [[1.0, 1.0, 1.0]])


def test_modes_validation_accepts_and_the_resident_copy(monkeypatch):
    from signals_amd.chain import nodes
    uploads = []
    monkeypatch.setattr(nodes, 'upload', lambda a: uploads.append(a) or torch.from_numpy(a))
    n = ext.Modal()
    for good in (np.ones((5, 3)), np.array([[2.0, -1.0, np.inf]]), np.array([[1, 1, 1], [2, 0, 3]]), np.ones((2048, 1, 3)), np.ones((32, 64, 3)),
                 np.array([[0.0, 1.0, 1e-9]])):
        n.get_state().modes = good
    modes = np.array([[1, 1, 1], [3, -2, 4]])                                  # int64: what a .sigs value arrives as
    n.get_state().modes = modes
    got = n.resident_modes()
    assert got.dtype == torch.float64 and tuple(got.shape) == (1, 2, 3) and got.is_contiguous()
    want = np.array([[[1.0, 1.0, np.log(1000.0)], [3.0, -2.0, np.log(1000.0) / 4.0]]])
    assert np.array_equal(got.numpy(), want) and np.array_equal(got.numpy(), MR.table(modes))
    assert n.resident_modes() is got and len(uploads) == 1                    # untouched: not uploaded again
    modes[1, 2] = 8                                                           # edited in place: seen
    assert n.resident_modes().numpy()[0, 1, 2] == np.log(1000.0) / 8.0 and len(uploads) == 2
    n.get_state().modes = np.array([[[1.0, 1.0, np.inf]], [[2.0, 1.0, 1.0]]])  # replaced; an undamped mode has lambda 0
    assert np.array_equal(n.resident_modes().numpy()[:, 0, 2], [0.0, np.log(1000.0)]) and len(uploads) == 3


def test_presets():
    s = ext.Modal.string(5, 2.0)
    assert s.shape == (5, 3) and np.array_equal(s[:, 0], [1, 2, 3, 4, 5]) and np.allclose(s[:, 1], 1 / s[:, 0]) and np.allclose(s[:, 2], 2 / s[:, 0])
    assert np.array_equal(s, MR.string64()[:5])
    b = ext.Modal.bar(6, 1.5)
    assert b.shape == (6, 3) and np.abs(b[:4, 0] - [1.0, 2.756, 5.404, 8.933]).max() < 1e-3 and b[0, 0] == 1.0
    assert np.allclose(b[:, 1], 1 / np.arange(1, 7)) and np.allclose(b[:, 2] * b[:, 0], 1.5)
    bell = ext.Modal.bell(6.0)
    assert bell.shape == (12, 3) and np.array_equal(bell[:5, 0], [0.5, 1.0, 1.2, 1.5, 2.0]) and (np.diff(bell[:, 0]) > 0).all()
    assert bell[0, 2] == 6.0 and (bell[:, 2] > 0).all() and 'Fletcher' in ext.Modal.bell.__doc__
    stacked = ext.Modal.stack([s, b, bell])
    assert stacked.shape == (3, 12, 3) and np.array_equal(stacked[0, :5], s) and np.array_equal(stacked[2], bell)
    assert np.array_equal(stacked[0, 5:], np.tile([0.0, 0.0, 1.0], (7, 1))) and (stacked[1, 6:, 1] == 0.0).all()     # zero-amplitude rows
    n = ext.Modal()
    for preset in (s, b, bell, stacked, ext.Modal.string(64, 0.5), ext.Modal.bar(64, 9.0)):
        n.get_state().modes = preset                                          # every preset passes the validator
    for bad in (lambda: ext.Modal.string(0), lambda: ext.Modal.string(65), lambda: ext.Modal.bar(True), lambda: ext.Modal.bar(3, 0.0),
                lambda: ext.Modal.bell(np.inf), lambda: ext.Modal.stack([]), lambda: ext.Modal.stack([np.ones((2, 2))])):
        with pytest.raises(ValueError):
            bad()


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize('index', range(len(CASES)), ids=[c['name'] for c in CASES])
def test_restatement_against_its_longdouble_twin(index):
    c = CASES[index]
    want, twin = MR.render_case(c), MR.render_case(c, dtype=np.longdouble)
    assert want.dtype == np.float64 and twin.dtype == np.longdouble and want.shape == (c['N'] * c['K'], c['voices'])
    assert np.array_equal(np.isnan(want), np.isnan(twin))
    err = float(np.nanmax(np.abs(want - twin))) if not np.isnan(want).all() else 0.0
    print('modal restatement', c['name'], 'max|f64 - longdouble|', err, 'bar', MR.tolerance(c['modes']))
    assert err <= MR.tolerance(c['modes'])


def test_restatement_against_a_direct_loop_and_its_exact_cases():
    """the vectorised restatement equals the definition written sample by sample, bit for bit; and the cases the definition fixes
    exactly: silence before the strike, a NaN gate, a dropped mode, every mode dropped, a NaN pitch, the fade strictly inside (0, 1)"""
    modes = MR.mode_table(5, 2)
    tab = MR.table(modes)
    hz, gate, damp, sel = np.array([[300.0, -2000.0, 0.0]]), np.array([[0.001, 0.0, 0.0005]]), np.array([[0.0, 2.0, 1.0]]), np.array([[0.0, 1.7, np.nan]])
    got = MR.modal(modes, 40, 30, hz, gate, damp, sel)
    for n in range(30):
        for v in range(3):
            q = np.float64(40 + n) / np.float64(RATE)
            e = q - gate[0, v]
            want = np.float64(0.0)
            if e >= 0:
                for r, a, lam in tab[[0, 1, 0][v]]:
                    F = hz[0, v] * r
                    with np.errstate(divide='ignore'):
                        g = np.clip(((0.5 * RATE) - abs(F)) / np.abs(hz[0, v]), 0.0, 1.0)
                    want = want + (a * g) * np.exp(-((lam + damp[0, v]) * e)) * np.sin(2.0 * np.pi * np.mod(e * F, 1.0))
            assert got[n, v] == want, (n, v)
    one = np.array([[1.0, 1.0, 1.0], [3.0, 0.5, 1.0]])
    out = MR.modal(one, 0, 64, np.array([[1000.0, 7900.0, 8000.0, 24000.0, np.nan, 1000.0, 1000.0]]),
                   np.array([[0.0, 0.0, 0.0, 0.0, 0.0005, np.nan, 1e6]]))
    assert (out[:, 3] == 0.0).all() and (out[:, 5:] == 0.0).all()            # every mode dropped; a NaN gate; a far-future gate
    assert (out[:24, 4] == 0.0).all() and np.isnan(out[24:, 4]).all()         # a NaN pitch: 0.0 before the strike, NaN after
    assert np.array_equal(out[:, 2:3], MR.modal(one[:1], 0, 64, [[8000.0]]))  # 3 * 8000 = rate / 2: the mode adds exactly 0
    faded = MR.modal(one, 0, 64, [[7900.0]]) - MR.modal(one[:1], 0, 64, [[7900.0]])         # 23700 Hz: g = 300 / 7900
    e = np.arange(64)[:, None] / RATE
    full = 0.5 * np.exp(-np.log(1000.0) * e) * np.sin(2 * np.pi * 23700.0 * e)
    assert np.abs(full).max() > 0.4 and np.abs(faded - 300.0 / 7900.0 * full).max() < 1e-12


def test_the_case_table_covers_what_the_kernel_test_asks_for():
    voices, frames, positions = ({c[k] for c in CASES} for k in ('voices', 'N', 'position'))
    Ms, Ws = ({MR.table(c['modes']).shape[axis] for c in CASES} for axis in (1, 0))
    assert voices >= {1, 2, 63, 65, 130} and frames >= {1, 2, MR.RUN - 1, MR.RUN, MR.RUN + 1, 255, 256, 257}
    assert Ms >= {1, 2, 63, 64} and Ws >= {1, 3} and positions >= {0, 37, 1000, 2 ** 24 + 5, 2 ** 31 + 3}
    c = next(c for c in CASES if c['voices'] == 130 and c['N'] == MR.RUN + 1)
    hz, gate = c['hertz'][0], c['gate_on'][0]
    rows, pos = c['N'] * c['K'], c['position']
    assert {0.0, 55.0, 440.3, -440.3} <= set(hz[~np.isnan(hz)]) and np.isnan(hz).any()
    tab = MR.table(c['modes'])[0]
    g = np.clip((0.5 * RATE - np.abs(hz[4] * tab[:, 0])) / abs(hz[4]), 0, 1)
    assert ((g > 0) & (g < 1)).any()                                          # a mode inside the fade
    assert (np.abs(hz[5]) * MR.table(c['modes'])[..., 0].min() >= 0.5 * RATE)  # a pitch that drops every mode
    e = (pos + np.arange(rows))[:, None] / RATE - gate[None, :]
    first = np.where((e >= 0).any(axis=0), (e >= 0).argmax(axis=0), rows)
    assert {0.0, -0.5, 1e6} <= set(gate[~np.isnan(gate)]) and np.isnan(gate).any()
    assert ((first > 0) & (first < rows)).any() and (first == rows).sum() >= 3 and len(set(gate[~np.isnan(gate)])) > 20
    assert any(((pos + (rows // 3) + 0.25) / RATE) == x for x in gate) and any(((pos + rows) / RATE) == x for x in gate)
    assert np.isinf(c['modes'][..., 2]).any() and (c['damp'] == 0).any() and (c['damp'] > 0).any()
    sel = next(c for c in CASES if c['select'] is not None and c['voices'] == 130)['select'][0]
    assert {-1.0, 0.5, 2.0, 7.0} <= set(sel[~np.isnan(sel)]) and np.isnan(sel).any()
    assert any(c['step'] > 1 for c in CASES) and any(c['K'] > 1 and all(c[k].shape[0] == c['K'] for k in ('hertz', 'gate_on', 'damp', 'select'))
                                                    for c in CASES)


# ---------------------------------------------------------------------------------------------- C ABI
def test_entry_point_is_exported_and_declared(lib):
    assert 'sig_modal_bank' in _native.EXPORTS
    raw = ctypes.CDLL(str(_native.LIB_PATH))
    assert raw.sig_modal_bank is not None
    assert lib.sig_abi_version() == 7                                         # additive
    header = (ROOT / 'include' / 'signals_amd.h').read_text()
    assert 'int sig_modal_bank(' in header and '#define SIG_ABI_VERSION 7' in header
    assert f'SIG_MODAL_MAX_MODES = {_native.MODAL_MAX_MODES}' in header and f'SIG_MODAL_MAX_POINTS = {_native.MODAL_MAX_POINTS}' in header
    assert (_native.MODAL_MAX_MODES, _native.MODAL_MAX_POINTS) == (64, 2048)
    assert 'sig_modal_bank' in (ROOT / 'INTEGRATION.md').read_text()
    kernel = (ROOT / 'signals_amd' / 'csrc' / 'modal.hip').read_text()
    assert '"sig_modal.h"' in kernel and 'fma(' not in kernel                 # the definition has no fused operation, nor has the recurrence


def test_modal_bank_argument_errors_do_not_reach_the_device(lib):
    p = 64                                                                    # (never dereferenced: every call fails its checks)
    args = dict(position=4096, step=1, rate=48000, rows=512, voices=8, rpp=256,
                hertz=p, hs=1, hrs=8, gate=p, gs=0, grs=0, damp=p, ds=1, drs=8, select=p, ss=1, srs=8,
                modes=p, W=4, M=16, out=p, odt=0, old=8, stream=None)

    def call(**over):
        a = dict(args, **over)
        return lib.sig_modal_bank(*(a[k] for k in args))
    assert call(modes=None) == INV and call(hertz=None) == INV and call(out=None) == INV
    assert call(M=0) == INV and call(M=65) == INV and call(M=-1) == INV and call(W=0) == INV and call(W=-1) == INV
    assert call(W=33, M=64) == INV and call(W=2049, M=1) == INV and call(W=2 ** 30, M=64) == INV      # W * M over the cap
    assert call(old=7) == INV and call(old=0) == INV                          # rows narrower than the voices
    for name in ('hs', 'gs', 'ds', 'ss'):
        assert call(**{name: 2}) == INV and call(**{name: -1}) == INV         # strides other than 0 or 1
    for name in ('hrs', 'grs', 'drs', 'srs'):
        assert call(**{name: -1}) == INV
    assert call(rows=-1) == INV and call(voices=-1) == INV and call(rate=0) == INV and call(position=-1) == INV
    assert call(step=0) == INV and call(rpp=-1) == INV and call(odt=2) == INV
    # accepted, nothing to launch: no rows, no voices -- at the caps, with the optional ports unplugged
    assert call(rows=0) == 0 and call(voices=0, old=0) == 0
    assert call(rows=0, W=32, M=64) == 0 and call(rows=0, W=2048, M=1) == 0 and call(rows=0, W=1, M=1) == 0
    assert call(rows=0, gate=None, damp=None, select=None) == 0 and call(rows=0, odt=1) == 0 and call(rows=0, step=256, rpp=1) == 0


# ---------------------------------------------------------------------------------------------- planning
def test_purity_and_modulation_classification():
    from signals_amd.engine import _audio_ports, _control_ports, _ctl_const, _foreign, _is_pure, _modulated
    m = modal_node(ext.Modal.bar(4), hertz=row(100, 900), gate_on=[[0.0]])
    assert not _foreign(m)
    assert _control_ports(m) == [m.hertz, m.gate_on, m.damp, m.select] and _audio_ports(m) == []
    assert all(_ctl_const(p) for p in _control_ports(m)) and not _modulated(m)
    assert _is_pure(m, {})                                                    # constant controls: a pure function of the position
    swept = modal_node(ext.Modal.bar(4), hertz=row(100, 900), damp=mkosc(osc.Sine, [[0.5]]))
    assert _modulated(swept) and not _is_pure(swept, {})


def mkosc(cls, hz):
    o = cls(); o.hertz = fix(hz)
    return o


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


FUSED = ('fused', 'latency', 'cascade', 'steady', 'walk', 'biquad_coldstart_env', 'voice_program')
SETTINGS = ({}, {'fuse_program': 'always'}, {'fuse': False}, {'specialise': False}, {'fuse_program': 'always', 'mixed_programs': True})


def voice(shape, modulated=False):
    hertz = row(100, 900)
    if modulated:
        hertz = fx.Mix(); hertz.left = mkosc(osc.Sine, [[0.7]]); hertz.right = fix(row(100, 900)); hertz.mix = fix([[0.01]])
    m = modal_node(ext.Modal.stack([ext.Modal.bar(6), ext.Modal.bell()]), hertz=hertz, gate_on=row(0.0, 0.01), select=row(0, 1.9))
    if shape == 'modal':
        return m, V
    if shape == 'lowpass':
        top = fx.LowPass(); top.input = m; top.cutoff = fix(row(500, 5000))
        return top, V
    b = ext.SumBus(); b.input = m
    return b, 1


@pytest.mark.parametrize('shape', ['modal', 'bus', 'lowpass'])
def test_one_launch_per_batch_on_every_renderer_setting_and_no_voice_program(stubbed, shape):
    from signals_amd.engine import BatchRenderer, _VoiceProgram
    launched = 0
    for kw in SETTINGS:
        for modulated, label in ((False, 'modal_bank[Modal12]'), (True, 'modal_bank[Modal12,per-block]')):
            top, C = voice(shape, modulated)
            rec = _Recorder()
            r = BatchRenderer(top, C, RATE, timer=rec, **kw)
            r.render(0, 256, 3)
            r.render(768, 256, 2)                                             # continuing
            r.render(8192, 256, 2)                                            # fresh
            assert not any(word in n for n in rec.names for word in FUSED), (kw, rec.names)
            banks = [n for n in rec.names if n.startswith('modal_bank')]
            assert set(banks) == {label} and len(banks) >= 3, (kw, rec.names)  # (a fresh batch re-renders a modulated node's history block)
            launched += len(banks)
            assert [name for name, _ in stubbed.calls].count('sig_modal_bank') == launched
    top, _ = voice(shape)
    assert _VoiceProgram.compile(None, top, V) is None                        # the voice program declines ...
    with pytest.raises(Exception, match='Modal: a modal bank has no voice-program word'):           # ... with its reason
        _VoiceProgram._count(types.SimpleNamespace(uses={}), voice('modal')[0])
    assert ext.Modal not in _VoiceProgram.KERNEL_NODES and not issubclass(ext.Modal, _VoiceProgram.KERNEL_NODES)


def test_the_launch_carries_the_rows_and_the_table(stubbed):
    from signals_amd.engine import BatchRenderer
    top, _ = voice('modal', modulated=True)
    BatchRenderer(top, V, RATE).render(4096, 256, 3)
    (a,) = [a for name, a in stubbed.calls if name == 'sig_modal_bank']
    assert a[:6] == (4096, 1, RATE, 768, V, 256)
    hertz, gate, damp, select = (a[6 + 3 * k:9 + 3 * k] for k in range(4))
    assert hertz[0] is not None and hertz[1:] == (1, V)                       # per-block rows of the modulated port: K rows, V apart
    assert gate[0] is not None and gate[1:] == (1, 0) and damp[0] is not None and damp[1:] == (0, 0) and select[1:] == (1, 0)
    assert a[18] == top.resident_modes().data_ptr() and a[19:21] == (2, 12)
    assert a[22] == _native.F32 and a[23] >= V
    top, _ = voice('lowpass')                                                 # constant controls: history and blocks in one launch
    stubbed.calls.clear()
    BatchRenderer(top, V, RATE, fuse=False).render(4096, 256, 2)
    (a,) = [a for name, a in stubbed.calls if name == 'sig_modal_bank']
    assert a[:6] == (4096 - 100, 1, RATE, 100 + 512, V, 0)                    # the filter's 100 context rows are simply rendered


def test_narrow_controls_raise_in_the_batch_as_in_the_node(stubbed):
    from signals_amd.engine import BatchRenderer
    BatchRenderer(modal_node(hertz=[[440.0]]), V, RATE).render(0, 256, 2)      # width 1: its natural width
    assert [a for name, a in stubbed.calls if name == 'sig_modal_bank'][-1][4] == 1
    with pytest.raises(IndexError, match='index 3 is out of bounds for axis 1 with size 3'):
        BatchRenderer(modal_node(hertz=row(100, 900, 3)), V, RATE).render(0, 256, 2)
    with pytest.raises(_native.NativeError, match=r'contiguous float64 \(sets, modes, 3\)'):
        _native.modal_bank(0, RATE, torch.zeros((1, 1), dtype=torch.float64), None, None, None, torch.zeros((2, 3), dtype=torch.float64),
                           torch.zeros((4, 1)))
    with pytest.raises(_native.NativeError, match='1 <= modes <= 64, sets \\* modes <= 2048'):
        _native.modal_bank(0, RATE, torch.zeros((1, 1), dtype=torch.float64), None, None, None, torch.zeros((1, 65, 3), dtype=torch.float64),
                           torch.zeros((4, 1)))


def test_the_node_in_a_control_path_is_refused_with_its_reason():
    from signals_amd.engine import BatchRenderer, NotBatchable, _Batch, _ControlProgram
    m = modal_node(ext.Modal.bar(3), hertz=[[2.0]])
    reason = r'ext\.Modal in a control path: a modal bank has no block-rate {} \(the eager node serves one-frame requests\)'
    with pytest.raises(NotBatchable, match=reason.format('program')):
        _ControlProgram((m,), 4, channels=1)
    g = fx.Gain(); g.left = m; g.right = fix([[100.0]])
    with pytest.raises(NotBatchable, match=reason.format('program')):
        _ControlProgram((g,), 4, channels=1)
    batch = _Batch(types.SimpleNamespace(rate=RATE), 0, 256, 4, False)
    with pytest.raises(NotBatchable, match='cutoff: signals.chain.' + reason.format('schedule')):
        batch._control_node(m, 'cutoff')
    lp = fx.LowPass(); lp.input = mkosc(osc.Sawtooth, row(100, 900)); lp.cutoff = g
    with pytest.raises(NotBatchable, match='a modal bank has no block-rate'):
        BatchRenderer(lp, V, RATE).render(0, 256, 2)
