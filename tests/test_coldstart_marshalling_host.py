"""What the cold-start filter wrappers of `_native` hand to the library, without a GPU: for biquad_coldstart (plain, with an
envelope, float64), biquad_coldstart_q, biquad_coldstart_eq, biquad_coldstart_bus, band_coldstart and band_coldstart_blocks the
entry called and its whole argument tuple, pointers as offsets from the tensors' data_ptr(); every refusal by type and exact
message, and which of two that could both fire comes first.  The library is a stub that records (entry name, arguments); `_gpu`
and `_stream` are patched out and the tensors are CPU tensors."""
import ctypes

import pytest
import torch

from signals_amd import _native
from signals_amd._native import NativeError

RATE = 48000
N, K, CTX, POS, HIST = 4, 3, 5, 7, 2            # block frames, blocks, context, position, history rows in front of the input
ROWS = N * K
F32, F64 = 0, 1
REAL_GPU = _native._gpu


@pytest.fixture
def calls(monkeypatch):
    """the stub library: every entry answers 0 and is recorded as (name, arguments), ctypes arrays as lists; `peek`, if set, is
    called with the raw arguments while the call is in flight"""
    seen = []

    class Lib:
        peek = None

        def __getattr__(self, name):
            def entry(*a):
                if self.peek:
                    self.peek(name, a)
                seen.append((name, tuple(list(x) if isinstance(x, ctypes.Array) else x for x in a)))
                return 0
            return entry
    stub = Lib()
    stub.seen = seen
    monkeypatch.setattr(_native, 'lib', lambda: stub)
    monkeypatch.setattr(_native, '_gpu', lambda *a: None)
    monkeypatch.setattr(_native, '_stream', lambda t: 0)
    return stub


def audio(V, dtype=torch.float32, pad=0, col=0, hist=HIST):
    """(buf, out): `hist` + ROWS and ROWS rows of V channels, viewed from column `col` of buffers `pad` channels wider"""
    buf = torch.zeros((hist + ROWS, V + pad), dtype=dtype)[:, col:col + V]
    out = torch.zeros((ROWS, V + pad), dtype=dtype)[:, col:col + V]
    return buf, out


def rows(r, c, fill=1000.0):
    return torch.full((r, c), fill, dtype=torch.float64)


def row_args(t):
    """(ptr, stride, blocks) of a control-row tensor, (None, 0, 1) of an unplugged one"""
    return (None, 0, 1) if t is None else (t.data_ptr(), int(t.shape[1] > 1), t.shape[0])


def window_args(buf, hist=HIST):
    return (buf.data_ptr() + hist * buf.stride(0) * buf.element_size(), buf.stride(0), hist)


def envelope(V, wide=('attack', 'sustain', 'gate_off')):
    return {name: rows(1, V if name in wide else 1, 0.01) for name in _native.ADSR_PARAMS}


def envelope_args(env):
    return ([env[n].data_ptr() for n in _native.ADSR_PARAMS], [int(env[n].shape[1] > 1) for n in _native.ADSR_PARAMS])


HEAD = (RATE, POS, N, K, CTX)

# (voices, cutoff rows, cutoff columns | 0 for `voices`, channels of padding, first column of the view)
LAYOUTS = [(1, 1, 1, 0, 0), (3, 1, 0, 0, 0), (3, K, 0, 2, 1), (8, 1, 0, 0, 0), (8, K, 0, 4, 4), (1, K, 1, 1, 1)]


@pytest.mark.parametrize('V,crows,ccols,pad,col', LAYOUTS)
@pytest.mark.parametrize('form', ['f32', 'f64', 'env'])
def test_biquad_coldstart_arguments(calls, V, crows, ccols, pad, col, form):
    dtype = torch.float64 if form == 'f64' else torch.float32
    buf, out = audio(V, dtype, pad, col)
    cutoff = rows(crows, ccols or V)
    status = torch.zeros(1, dtype=torch.int32) if V == 3 else None
    env = envelope(V) if form == 'env' else None
    assert _native.biquad_coldstart('hp', RATE, POS, N, K, CTX, cutoff, buf, HIST, out, status=status, envelope=env) is out
    st = None if status is None else status.data_ptr()
    head = (1,) + HEAD + (V,) + row_args(cutoff)
    if form == 'env':
        want = ('sig_biquad_coldstart_env', head + envelope_args(env) + window_args(buf) + (out.data_ptr(), V + pad, st, 0))
    else:
        want = ('sig_biquad_coldstart', head + window_args(buf) + (out.data_ptr(), V + pad, F64 if form == 'f64' else F32, st, 0))
    assert calls.seen == [want]
    assert out.data_ptr() == out._base.data_ptr() + col * out.element_size()


# resonance / gain: unplugged, one value, one row, per-block one column, per-block rows
CONTROLS = [None, (1, 1), (1, 0), (K, 1), (K, 0)]


@pytest.mark.parametrize('V,crows,ccols,pad,col', LAYOUTS)
@pytest.mark.parametrize('qshape', CONTROLS)
def test_biquad_coldstart_q_arguments(calls, V, crows, ccols, pad, col, qshape):
    dtype = torch.float64 if pad == 2 else torch.float32
    buf, out = audio(V, dtype, pad, col)
    cutoff = rows(crows, ccols or V)
    q = None if qshape is None else rows(qshape[0], qshape[1] or V, 0.9)
    status = torch.zeros(1, dtype=torch.int32)
    assert _native.biquad_coldstart_q('lp', RATE, POS, N, K, CTX, cutoff, q, buf, HIST, out, status=status) is out
    assert calls.seen == [('sig_biquad_coldstart_q', (0,) + HEAD + (V,) + row_args(cutoff) + row_args(q) + window_args(buf)
                           + (out.data_ptr(), V + pad, F64 if pad == 2 else F32, status.data_ptr(), 0))]


@pytest.mark.parametrize('V,crows,ccols,pad,col', LAYOUTS)
@pytest.mark.parametrize('qshape,gshape', [(None, None), ((1, 1), (K, 0)), ((K, 0), None), (None, (1, 0)), ((K, 1), (1, 1)), ((1, 0), (K, 1))])
def test_biquad_coldstart_eq_arguments(calls, V, crows, ccols, pad, col, qshape, gshape):
    dtype = torch.float64 if pad == 2 else torch.float32
    buf, out = audio(V, dtype, pad, col)
    cutoff = rows(crows, ccols or V)
    q = None if qshape is None else rows(qshape[0], qshape[1] or V, 0.9)
    g = None if gshape is None else rows(gshape[0], gshape[1] or V, 3.0)
    assert _native.biquad_coldstart_eq('eqpeak', RATE, POS, N, K, CTX, cutoff, q, g, buf, HIST, out) is out
    assert calls.seen == [('sig_biquad_coldstart_eq', (_native.FILT_TYPES['eqpeak'],) + HEAD + (V,) + row_args(cutoff) + row_args(q)
                           + row_args(g) + window_args(buf) + (out.data_ptr(), V + pad, F64 if pad == 2 else F32, None, 0))]


@pytest.mark.parametrize('V,crows,ccols,pad,col', LAYOUTS)
@pytest.mark.parametrize('bus,env', [(1, False), (2, True), (4, False), (0, True)])        # bus 0: mono without gains
def test_biquad_coldstart_bus_arguments(calls, V, crows, ccols, pad, col, bus, env):
    buf, _ = audio(V, torch.float32, pad, col)
    out = torch.zeros((ROWS, max(bus, 1) + 3), dtype=torch.float32)[:, 1:1 + max(bus, 1)]
    cutoff = rows(crows, ccols or V)
    gains = (torch.ones((bus, V + 1), dtype=torch.float64)[:, :V] if bus > 1 else rows(1, V)) if bus else None
    envs = envelope(V) if env else None
    workspace = torch.zeros(16, dtype=torch.float64)
    status = torch.zeros(1, dtype=torch.int32)
    assert _native.biquad_coldstart_bus('lp', RATE, POS, N, K, CTX, cutoff, buf, HIST, gains, out, envelope=envs, workspace=workspace,
                                        status=status) is out
    bus = max(bus, 1)
    assert calls.seen == [
        ('sig_fused_voice_bus_workspace', (V, ROWS, bus)),
        ('sig_biquad_coldstart_bus', (0,) + HEAD + (V,) + row_args(cutoff) + (envelope_args(envs) if env else (None, None))
         + window_args(buf) + ((None, 0) if gains is None else (gains.data_ptr(), gains.stride(0))) + (bus, workspace.data_ptr())
         + (out.data_ptr(), bus + 3, status.data_ptr(), 0))]


@pytest.mark.parametrize('V,pad,col', [(1, 0, 0), (3, 2, 1), (8, 4, 4)])
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_band_coldstart_arguments(calls, V, pad, col, dtype):
    buf, out = audio(V, dtype, pad, col)
    low, high = rows(1, V, 300.0), rows(1, V, 3000.0)
    assert _native.band_coldstart('bs', RATE, POS, N, K, CTX, low, high, buf, HIST, out) is out
    assert calls.seen == [('sig_band_coldstart', (3,) + HEAD + (V,) + row_args(low)[:2] + row_args(high)[:2] + window_args(buf)
                           + (out.data_ptr(), V + pad, F64 if dtype == torch.float64 else F32, None, 0))]


@pytest.mark.parametrize('V,pad,col', [(1, 0, 0), (3, 2, 1), (8, 4, 4)])
@pytest.mark.parametrize('lrows,hrows', [(1, 1), (K, K), (1, K), (K, 1)])
def test_band_coldstart_blocks_arguments(calls, V, pad, col, lrows, hrows):
    """a single-row edge beside a per-block one reaches the library as K equal rows of a copy that lives until the call returns"""
    buf, out = audio(V, torch.float32, pad, col)
    low = torch.arange(lrows * V, dtype=torch.float64).reshape(lrows, V) + 300.0
    high = torch.arange(hrows * V, dtype=torch.float64).reshape(hrows, V) + 3000.0
    status = torch.zeros(1, dtype=torch.int32)
    held = {}

    def peek(name, a):                                     # the edges as the library would read them
        blocks = a[11]
        for key, ptr in (('low', a[7]), ('high', a[9])):
            held[key] = list((ctypes.c_double * (blocks * V)).from_address(ptr))
    calls.peek = peek
    assert _native.band_coldstart_blocks('bp', RATE, POS, N, K, CTX, low, high, buf, HIST, out, status=status) is out
    blocks = max(lrows, hrows)
    (name, a), = calls.seen
    assert name == 'sig_band_coldstart_blocks'
    assert a[:7] == (2,) + HEAD + (V,)
    assert (a[8], a[10], a[11]) == (int(V > 1), int(V > 1), blocks)
    assert a[12:] == window_args(buf) + (out.data_ptr(), V + pad, F32, status.data_ptr(), 0)
    for t, r, ptr, key in ((low, lrows, a[7], 'low'), (high, hrows, a[9], 'high')):
        assert (ptr == t.data_ptr()) == (r == blocks)                               # expanded: a copy, else the tensor itself
        assert held[key] == t.expand(blocks, V).reshape(-1).tolist()


# ---------------------------------------------------------------------------------------------------------------- refusals

def refuse(kind, message, fn, *a, **kw):
    with pytest.raises(kind) as e:
        fn(*a, **kw)
    assert type(e.value) is kind
    assert (e.value.args[0] if kind is KeyError else str(e.value)) == message


V3 = 3
WINDOW_ENTRIES = [
    ('biquad', lambda buf, hist, out, **kw: _native.biquad_coldstart('lp', RATE, POS, N, K, CTX, kw.get('cutoff', rows(1, V3)), buf, hist, out)),
    ('biquad', lambda buf, hist, out, **kw: _native.biquad_coldstart_q('lp', RATE, POS, N, K, CTX, kw.get('cutoff', rows(1, V3)), None, buf, hist, out)),
    ('biquad', lambda buf, hist, out, **kw: _native.biquad_coldstart_eq('eqls', RATE, POS, N, K, CTX, kw.get('cutoff', rows(1, V3)), None, None, buf, hist, out)),
    ('biquad bus', lambda buf, hist, out, **kw: _native.biquad_coldstart_bus('lp', RATE, POS, N, K, CTX, kw.get('cutoff', rows(1, V3)), buf, hist, None, out[:, :1])),
    ('band', lambda buf, hist, out, **kw: _native.band_coldstart('bp', RATE, POS, N, K, CTX, rows(1, V3), rows(1, V3), buf, hist, out)),
    ('band', lambda buf, hist, out, **kw: _native.band_coldstart_blocks('bp', RATE, POS, N, K, CTX, rows(K, V3), rows(1, V3), buf, hist, out)),
]


@pytest.mark.parametrize('what,call', WINDOW_ENTRIES)
def test_refusals_common_to_every_entry(calls, monkeypatch, what, call):
    """the buffers: layout, then shapes and dtypes against history and blocks, then (where the entry takes one) the buffer dtype"""
    bus = what == 'biquad bus'
    buf, out = audio(V3)
    crossed = torch.zeros((V3, HIST + ROWS))
    refuse(NativeError, f'{what} in: audio buffers are 2-D with contiguous channels, got strides (1, {HIST + ROWS})', call, crossed.t(), HIST, out)
    if not bus:
        refuse(NativeError, f'{what} out: audio buffers are 2-D with contiguous channels, got strides (1, {ROWS})', call, buf, HIST,
               torch.zeros((V3, ROWS)).t())
    # a layout refusal comes before a shape refusal
    refuse(NativeError, f'{what} in: audio buffers are 2-D with contiguous channels, got strides (1, {HIST + ROWS})', call, crossed.t(), HIST + 1, out)
    ov = 1 if bus else V3
    shapes = lambda b, h, o: (f'{what} shapes: in {tuple(b.shape)} {b.dtype} history {h} out {tuple(o.shape)} {o.dtype} blocks {K}x{N}')
    assert shapes(buf, 1, out[:, :ov]) == f'{what} shapes: in (14, 3) torch.float32 history 1 out (12, {ov}) torch.float32 blocks 3x4'
    refuse(NativeError, shapes(buf, 1, out[:, :ov]), call, buf, 1, out)                                   # history + rows != rows of buf
    refuse(NativeError, shapes(buf, HIST, out[:-1, :ov]), call, buf, HIST, out[:-1])                       # rows != blocks x frames
    if bus:
        refuse(NativeError, 'biquad bus out must be float32, got torch.float64', call, buf, HIST, out.double())
        refuse(NativeError, 'biquad bus out must be float32, got torch.float64', call, buf, 1, out.double())       # before the shapes
    else:
        refuse(NativeError, shapes(buf, HIST, out.double()), call, buf, HIST, out.double())                # dtypes differ
        refuse(NativeError, shapes(buf[:, :2], HIST, out), call, buf[:, :2], HIST, out)                    # channels differ
        half = lambda t: t.to(torch.float16)
        refuse(NativeError, 'unsupported buffer dtype torch.float16', call, half(buf), HIST, half(out))
        if what == 'biquad':                                                                               # the control rows come first
            refuse(NativeError, 'cutoff must be a contiguous float64 2-D tensor', call, half(buf), HIST, half(out), cutoff=rows(1, V3).float())
    # the tensors must be on the GPU: the first thing asked
    monkeypatch.setattr(_native, '_gpu', REAL_GPU)
    refuse(NativeError, 'HIP kernels need tensors resident on an MI355X (got a CPU tensor); no CPU fallback', call, crossed.t(), 1, out)
    assert calls.seen == [] or all(name == 'sig_fused_voice_bus_workspace' for name, _ in calls.seen)


def test_refusals_biquad_coldstart(calls):
    buf, out = audio(V3)
    go = lambda cutoff, btype='lp', out=out, buf=buf, **kw: _native.biquad_coldstart(btype, RATE, POS, N, K, CTX, cutoff, buf, HIST, out, **kw)
    refuse(NativeError, 'cutoff must be a contiguous float64 2-D tensor', go, rows(1, V3).float())
    refuse(NativeError, 'cutoff must be a contiguous float64 2-D tensor', go, rows(1, V3)[0])
    refuse(NativeError, 'cutoff must be a contiguous float64 2-D tensor', go, rows(1, 2 * V3)[:, ::2])
    refuse(NativeError, 'cutoff shape (2, 3) vs blocks 3 voices 3', go, rows(2, V3))
    refuse(NativeError, 'cutoff shape (1, 2) vs blocks 3 voices 3', go, rows(1, 2))
    refuse(IndexError, 'index 1 is out of bounds for axis 1 with size 1', go, rows(1, 1))
    refuse(IndexError, 'index 1 is out of bounds for axis 1 with size 1', go, rows(K, 1))
    refuse(NativeError, 'cutoff shape (2, 1) vs blocks 3 voices 3', go, rows(2, 1))                        # the shape before the IndexError
    refuse(KeyError, 'nope', go, rows(1, V3), btype='nope')
    refuse(NativeError, 'cutoff shape (2, 3) vs blocks 3 voices 3', go, rows(2, V3), btype='nope')        # the cutoff before the type
    refuse(NativeError, 'cutoff must be a contiguous float64 2-D tensor', go, rows(1, V3).float(), buf=buf.double(), out=out.double(),
           envelope=envelope(V3))
    # the envelope: float32 buffers, then its six rows
    refuse(NativeError, 'the envelope epilogue is float32 only', go, rows(1, V3), buf=buf.double(), out=out.double(), envelope=envelope(V3))
    refuse(KeyError, 'nope', go, rows(1, V3), btype='nope', buf=buf.double(), out=out.double(), envelope=envelope(V3))
    env = envelope(V3); env['decay'] = rows(1, 2)
    refuse(NativeError, 'decay has 2 channels for 3 voices', go, rows(1, V3), envelope=env)
    refuse(NativeError, 'the envelope epilogue is float32 only', go, rows(1, V3), buf=buf.double(), out=out.double(), envelope=env)
    env = envelope(V3); env['release'] = rows(2, V3)
    refuse(NativeError, 'release: control rows are contiguous float64 (1,V) or (1,1), got (2, 3) torch.float64', go, rows(1, V3), envelope=env)
    env = envelope(V3); del env['gate_on']
    refuse(KeyError, 'gate_on', go, rows(1, V3), envelope=env)
    assert calls.seen == []


@pytest.mark.parametrize('entry', ['q', 'eq'])
def test_refusals_resonant_and_equaliser(calls, entry):
    buf, out = audio(V3)
    if entry == 'q':
        go = lambda cutoff, q=None, g=None, btype='hp': _native.biquad_coldstart_q(btype, RATE, POS, N, K, CTX, cutoff, q, buf, HIST, out)
        controls = ['resonance']
    else:
        go = lambda cutoff, q=None, g=None, btype='eqhs': _native.biquad_coldstart_eq(btype, RATE, POS, N, K, CTX, cutoff, q, g, buf, HIST, out)
        controls = ['resonance', 'gain']
    good = rows(1, V3)
    refuse(NativeError, 'cutoff must be a contiguous float64 2-D tensor', go, good.float())
    refuse(NativeError, 'cutoff must be a contiguous float64 2-D tensor', go, rows(K, 2 * V3)[:, :V3])
    refuse(NativeError, 'cutoff shape (2, 3) vs blocks 3 voices 3', go, rows(2, V3))
    refuse(NativeError, 'cutoff shape (1, 4) vs blocks 3 voices 3', go, rows(1, 4))
    refuse(IndexError, 'index 1 is out of bounds for axis 1 with size 1', go, rows(K, 1))
    refuse(KeyError, 'nope', go, good, btype='nope')
    refuse(KeyError, 'nope', go, rows(2, V3), btype='nope')                                                # the type before the cutoff
    for name in controls:
        kw = lambda t: {'q' if name == 'resonance' else 'g': t}
        refuse(NativeError, f'{name} must be a contiguous float64 2-D tensor', go, good, **kw(good.float()))
        refuse(NativeError, f'{name} must be a contiguous float64 2-D tensor', go, good, **kw(rows(V3, K).t()))
        refuse(NativeError, f'{name} shape (2, 1) vs blocks 3 voices 3', go, good, **kw(rows(2, 1)))
        refuse(NativeError, f'{name} shape (1, 2) vs blocks 3 voices 3', go, good, **kw(rows(1, 2)))
        refuse(NativeError, f'{name} shape (1, 2) vs blocks 3 voices 3', go, rows(2, V3), **kw(rows(1, 2)))     # before the cutoff
        refuse(NativeError, f'{name} shape (1, 2) vs blocks 3 voices 3', go, good, btype='nope', **kw(rows(1, 2)))   # and the type
    if entry == 'eq':
        refuse(NativeError, 'resonance shape (1, 2) vs blocks 3 voices 3', go, good, q=rows(1, 2), g=rows(1, 2))    # resonance, then gain
    assert calls.seen == []


def test_refusals_biquad_coldstart_bus(calls):
    buf, _ = audio(V3)
    out = torch.zeros((ROWS, 2))
    gains = torch.ones((2, V3), dtype=torch.float64)
    go = lambda cutoff, btype='lp', gains=gains, out=out, **kw: _native.biquad_coldstart_bus(btype, RATE, POS, N, K, CTX, cutoff, buf, HIST,
                                                                                              gains, out, **kw)
    cutoff_message = lambda t: f'cutoff must be contiguous float64 (1|3, 1|3), got {tuple(t.shape)} {t.dtype}'
    for bad in (rows(1, V3).float(), rows(1, 2), rows(2, V3), rows(K, 2 * V3)[:, :V3]):
        refuse(NativeError, cutoff_message(bad), go, bad)
    assert cutoff_message(rows(2, V3)) == 'cutoff must be contiguous float64 (1|3, 1|3), got (2, 3) torch.float64'
    assert calls.seen == []
    refuse(KeyError, 'nope', go, rows(1, 1), btype='nope')                                  # one cutoff column for all voices: no refusal
    refuse(NativeError, cutoff_message(rows(2, V3)), go, rows(2, V3), btype='nope')
    env = envelope(V3); env['attack'] = rows(1, 2)
    refuse(NativeError, 'attack has 2 channels for 3 voices', go, rows(1, V3), envelope=env)
    refuse(KeyError, 'nope', go, rows(1, V3), btype='nope', envelope=env)                   # the type, the envelope, the gains
    refuse(NativeError, 'attack has 2 channels for 3 voices', go, rows(1, V3), envelope=env, gains=None)
    refuse(NativeError, 'a bus without gains is mono', go, rows(1, V3), gains=None)
    for bad in (gains.float(), gains[:1], torch.ones((2, 2 * V3), dtype=torch.float64)[:, ::2]):
        refuse(NativeError, f'bus gains must be float64 (2,3), got {tuple(bad.shape)} {bad.dtype}', go, rows(1, V3), gains=bad)
    # the workspace is asked for before any of these, and a new one made where none is given
    assert calls.seen and all(name == 'sig_fused_voice_bus_workspace' for name, _ in calls.seen)


@pytest.mark.parametrize('per_block', [False, True])
def test_refusals_band(calls, per_block):
    buf, out = audio(V3)
    fn = _native.band_coldstart_blocks if per_block else _native.band_coldstart
    go = lambda low, high, btype='bp': fn(btype, RATE, POS, N, K, CTX, low, high, buf, HIST, out)
    good = rows(1, V3)
    index = lambda n: f'index {n} is out of bounds for axis 1 with size {n}'
    refuse(IndexError, index(1), go, rows(1, 1), good)
    refuse(IndexError, index(1), go, good, rows(1, 1))
    refuse(IndexError, index(2), go, rows(1, 2), rows(1, 1))                                               # low, then high
    refuse(IndexError, index(4), go, good, rows(1, 4).float())                                             # the width before the dtype
    refuse(KeyError, 'nope', go, good, good, btype='nope')
    if per_block:
        refuse(NativeError, 'low must be a contiguous float64 2-D tensor', go, good.float(), good)
        refuse(NativeError, 'high must be a contiguous float64 2-D tensor', go, good, rows(K, 2 * V3)[:, ::2])
        refuse(NativeError, 'low has 2 rows for 3 blocks', go, rows(2, V3), good)
        refuse(NativeError, 'high has 2 rows for 3 blocks', go, rows(K, V3), rows(2, V3))
        refuse(NativeError, 'low has 2 rows for 3 blocks', go, rows(2, V3), good.float())                  # low, then high
        refuse(NativeError, 'low has 2 rows for 3 blocks', go, rows(2, V3), good, btype='nope')
    else:
        row = lambda name, t: f'{name}: control rows are contiguous float64 (1,V) or (1,1), got {tuple(t.shape)} {t.dtype}'
        refuse(NativeError, row('low', good.float()), go, good.float(), good)
        refuse(NativeError, row('high', rows(K, V3)), go, good, rows(K, V3))
        refuse(NativeError, row('high', rows(1, 2 * V3)[:, ::2]), go, good, rows(1, 2 * V3)[:, ::2])
        refuse(NativeError, row('low', rows(K, V3)), go, rows(K, V3), good.float())                        # low, then high
        refuse(NativeError, row('low', rows(K, V3)), go, rows(K, V3), good, btype='nope')
    assert calls.seen == []


def test_one_voice_takes_any_one_column_row(calls):
    """at one voice the one-column rows are the voice's own: no IndexError, stride 0"""
    buf, out = audio(1)
    _native.biquad_coldstart('lp', RATE, POS, N, K, CTX, rows(K, 1), buf, HIST, out)
    _native.band_coldstart_blocks('bs', RATE, POS, N, K, CTX, rows(K, 1), rows(K, 1), buf, HIST, out)
    (biquad, a), (band, b) = calls.seen
    assert (biquad, a[8:10]) == ('sig_biquad_coldstart', (0, K))
    assert (band, b[8], b[10:12]) == ('sig_band_coldstart_blocks', 0, (0, K))
