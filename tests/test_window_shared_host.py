"""What the window nodes' refactoring states once, without a GPU: the resident-copy holder of chain/nodes.py (one upload per
change of the host array, checked with a counting stand-in for the upload), `_native`'s by-value (U, 2) arrays and device-table
checks with the refusals and messages they had when each caller spelled them out, and that sig_window_tile.h is what delay.hip and
fir.hip take their argument checks, grid and dtype dispatch from."""
import pathlib
import re

import numpy as np
import pytest
import torch

from signals_amd import _native
from signals_amd.chain import ResidentCopy, ext, nodes

ROOT = pathlib.Path(__file__).resolve().parent.parent


@pytest.fixture(autouse=True)
def _cpu_device():
    from signals_amd import runtime
    old = runtime._device
    runtime.set_device('cpu')
    yield
    runtime._device = old


@pytest.fixture
def uploads(monkeypatch):
    """counts the uploads and keeps what was handed over"""
    seen = []
    real = nodes.upload

    def counting(host):
        seen.append(host)
        return real(host)
    monkeypatch.setattr(nodes, 'upload', counting)
    return seen


# ---------------------------------------------------------------------------------------------- the resident copy
def test_resident_copy_uploads_once_per_change(uploads):
    held = ResidentCopy(np.float32)
    a = np.arange(6.0).reshape(3, 2)
    first = held.of(a)
    assert len(uploads) == 1 and first.dtype == torch.float32 and first.tolist() == a.tolist()
    assert held.of(a) is first and held.of(a) is first and len(uploads) == 1                         # the same array: no new upload
    assert uploads[0].flags['C_CONTIGUOUS'] and not np.shares_memory(uploads[0], a)                 # a copy of its own
    a[1, 1] = 9.0                                                                                   # an in-place edit
    second = held.of(a)
    assert second is not first and len(uploads) == 2 and second.tolist() == a.tolist() and first.tolist()[1][1] == 3.0
    assert held.of(a) is second and len(uploads) == 2
    b = a.copy()                                                                                    # a replaced array, equal bytes
    third = held.of(b)
    assert third is not second and len(uploads) == 3 and third.tolist() == b.tolist()
    assert held.of(b) is third and len(uploads) == 3
    assert held.of(a) is not third and len(uploads) == 4                                            # ... and back


def test_resident_copy_converts_and_lays_out(uploads):
    ints = np.array([[1, 2, 3], [4, 5, 6]])                                                         # what a .sigs value arrives as
    got = ResidentCopy(np.float64).of(ints)
    assert got.dtype == torch.float64 and got.tolist() == [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]
    turned = ResidentCopy(np.float32, layout=np.transpose).of(ints)
    assert turned.shape == (3, 2) and turned.is_contiguous() and turned.tolist() == [[1.0, 4.0], [2.0, 5.0], [3.0, 6.0]]
    strided = np.arange(24.0).reshape(4, 6)[::2, ::3]                                               # not contiguous on the host
    got = ResidentCopy(np.float32).of(strided)
    assert got.is_contiguous() and got.tolist() == strided.tolist()
    assert len(uploads) == 3 and all(h.flags['C_CONTIGUOUS'] for h in uploads)


def _nodes():
    bus = ext.SumBus(); bus.get_state().gains = np.ones((2, 5))
    wt = ext.Wavetable(); wt.get_state().table = np.arange(8.0).reshape(4, 2)
    sh = ext.Shaper(); sh.get_state().table = np.arange(6.0).reshape(3, 2)
    fir = ext.FIR(); fir.get_state().taps = np.arange(6.0).reshape(3, 2)
    sam = ext.Sampler(); sam.get_state().table = np.arange(10.0).reshape(5, 2)
    mm = ext.MixMatrix()
    return [(bus, 'gains', bus.resident_gains, torch.float64, False), (wt, 'table', wt.resident_table, torch.float32, False),
            (sh, 'table', sh.resident_table, torch.float32, False), (fir, 'taps', fir.resident_table, torch.float64, False),
            (sam, 'table', sam.resident_table, torch.float32, True), (mm, 'matrix', mm.resident_matrix, torch.float32, False)]


def test_every_node_with_a_resident_copy_follows_its_state(uploads):
    for node, attr, resident, dtype, transposed in _nodes():
        before = len(uploads)
        array = getattr(node.get_state(), attr)
        want = (lambda a: a.T) if transposed else (lambda a: a)
        first = resident()
        assert first.dtype == dtype and first.is_contiguous() and np.array_equal(first.numpy(), want(array)), type(node)
        assert resident() is first and len(uploads) == before + 1, type(node)                      # untouched: not uploaded again
        array[0, 0] = 77.0                                                                          # edited in place
        second = resident()
        assert second is not first and len(uploads) == before + 2 and np.array_equal(second.numpy(), want(array)), type(node)
        setattr(node.get_state(), attr, array.copy())                                               # replaced
        third = resident()
        assert third is not second and len(uploads) == before + 3 and resident() is third, type(node)


def test_the_samplers_copy_is_the_transpose(uploads):
    sam = ext.Sampler()
    table = np.arange(12.0).reshape(6, 2)                                                           # (frames, recordings)
    sam.get_state().table = table
    got = sam.resident_table()
    assert got.shape == (2, 6) and got.dtype == torch.float32 and got.is_contiguous()               # every recording contiguous
    assert np.array_equal(got.numpy(), table.T) and uploads[-1].flags['C_CONTIGUOUS']
    assert ext.SumBus().resident_gains() is None and len(uploads) == 1                              # no gains: nothing to hold


# ---------------------------------------------------------------------------------------------- (U, 2) arrays by value
PAIRS = [np.zeros(2), np.zeros((2, 3)), np.zeros((2, 2, 2)), np.zeros((0, 2)), np.array([[1.0, np.nan]]), np.array([[np.inf, 1.0]])]


@pytest.mark.parametrize('check, cap, what, columns', [(_native._copies, _native.UNISON_MAX_COPIES, 'unison copies', '(detune, phase offset)'),
                                                       (_native._taps, _native.DELAY_MAX_TAPS, 'delay taps', '(multiplier, gain)')])
def test_by_value_arrays_refuse_what_they_refused(check, cap, what, columns):
    for bad in PAIRS + [np.zeros((cap + 1, 2))]:
        shape = np.asarray(bad).shape
        with pytest.raises(_native.NativeError) as info:
            check(bad)
        assert str(info.value) == f'{what} must be a finite (1..{cap}, 2) array of {columns} rows, got shape {shape}'
    U, first, second = check([[1, 2], [3, 4]])                                                      # a list of integers converts
    assert U == 2 and list(first) == [1.0, 3.0] and list(second) == [2.0, 4.0]
    U, first, second = check(np.ones((cap, 2)))                                                     # the cap itself
    assert U == cap and len(first) == len(second) == cap
    assert (_native.UNISON_MAX_COPIES, _native.DELAY_MAX_TAPS) == (16, 16)
    assert str(pytest.raises(_native.NativeError, _native._taps, np.zeros((17, 2))).value) == \
        'delay taps must be a finite (1..16, 2) array of (multiplier, gain) rows, got shape (17, 2)'


# ---------------------------------------------------------------------------------------------- device tables
def _refusal(call) -> str:
    with pytest.raises(_native.NativeError) as info:
        call()
    return str(info.value)


def test_wavetable_and_shaper_tables_refuse_what_they_refused():
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32)
    kind = 'a wavetable is a contiguous float32 (points, waves) tensor'
    for bad in (None, torch.zeros((4, 2), dtype=torch.float64), f32(4), f32(4, 2, 2), f32(2, 4).T):
        assert _refusal(lambda: _native._table(bad)) == kind and _refusal(lambda: _native._table(bad, pow2=False)) == kind
    for shape in ((1, 2), (3, 2), (48, 1), (4, 0), (16384, 2), (32768, 1)):
        assert _refusal(lambda: _native._table(f32(*shape))) == f'table {shape}: points a power of two >= 2, points * waves <= 16384'
    for shape in ((1, 2), (4, 0), (16385, 1), (3, 5462)):
        assert _refusal(lambda: _native._table(f32(*shape), pow2=False)) == f'table {shape}: points >= 2, points * waves <= 16384'
    t = f32(4, 2)
    assert _native._table(t) == (t.data_ptr(), 4, 2) and _native._table(f32(16384, 1))[1:] == (16384, 1)
    t = f32(3, 5461)                                                                                # 16383 points, any T for a shaper
    assert _native._table(t, pow2=False) == (t.data_ptr(), 3, 5461)
    assert _native.TABLE_MAX_POINTS == 16384


def test_fir_tables_refuse_what_they_refused():
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64)
    kind = 'a FIR table is a contiguous float64 (taps, columns) tensor'
    for bad in (None, torch.zeros((4, 2), dtype=torch.float32), f64(4), f64(4, 2, 2), f64(2, 4).T):
        assert _refusal(lambda: _native._fir_table(bad)) == kind
    for shape in ((0, 1), (102, 1), (3, 0), (17, 241), (1, 4097), (64, 65)):
        assert _refusal(lambda: _native._fir_table(f64(*shape))) == f'FIR table {shape}: 1 <= taps <= 101, columns >= 1, taps * columns <= 4096'
    for shape in ((1, 1), (101, 40), (64, 64), (1, 4096)):
        t = f64(*shape)
        assert _native._fir_table(t) == (t.data_ptr(), *shape)


def test_sampler_tables_refuse_what_they_refused(monkeypatch):
    calls = []

    class Lib:
        def sig_sampler_play(self, *a):
            calls.append(a)
            return 0
    monkeypatch.setattr(_native, 'lib', lambda: Lib())
    monkeypatch.setattr(_native, '_gpu', lambda *a: None)
    monkeypatch.setattr(_native, '_stream', lambda t: 0)
    out = torch.zeros((8, 3), dtype=torch.float32)
    ratio = torch.ones((1, 3), dtype=torch.float64)
    play = lambda table: _native.sampler_play(0, 48000, ratio, None, None, None, table, 0, 0, out)
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32)
    kind = 'a sampler table is a contiguous float32 (recordings, frames) tensor'
    for bad in (None, torch.zeros((2, 10), dtype=torch.float64), f32(10), f32(2, 10, 1), f32(10, 2).T):
        assert _refusal(lambda: play(bad)) == kind
    for waves, frames in ((2, 1), (0, 10), (1, (1 << 26) + 1)):
        table = torch.empty((waves, frames), dtype=torch.float32)                                   # (never touched: 256 MiB of address space at most)
        assert _refusal(lambda: play(table)) == (f'sampler table of {frames} frames x {waves} recordings: frames >= 2, '
                                                 f'frames * recordings <= {1 << 26}')
    assert not calls
    table = f32(2, 10)
    play(table)
    (a,), position = calls, 18                                                                      # head 6, four rows of 3: the table follows
    assert a[position:position + 5] == (table.data_ptr(), 10, 2, 0, 0)                              # ptr, frames, recordings, loop


# ---------------------------------------------------------------------------------------------- the kernels' shared header
def test_delay_and_fir_take_the_shared_parts_from_the_header():
    csrc = ROOT / 'signals_amd' / 'csrc'
    header = (csrc / 'sig_window_tile.h').read_text()
    for text in ('struct Frame', 'struct Input', 'struct Rows', 'struct Tile', 'tile_at(', 'column(', 'args_ok(', 'workgroups(', 'dispatch(',
                 '0x7fffffffLL', 'context_rows == (position < kHalo ? position'):
        assert text in header, text
    for name in ('delay.hip', 'fir.hip'):
        text = (csrc / name).read_text()
        assert '"sig_window_tile.h"' in text and 'sig_window::args_ok(' in text and 'sig_window::workgroups(' in text
        assert 'sig_window::dispatch(' in text and 'sig_window::tile_at<kTileRows>(' in text and 'sig_window::column<IN>(' in text
        assert 'dispatch_out' not in text and '0x7fffffff' not in text and 'SIG_F32' not in text   # no dispatch, grid or dtype check of its own
        assert len(re.findall(r'SIG_CHECK_ARG', text)) == 2                                         # the shared checks, and the entry's own
        assert 'delay.hip does' not in text and 'fir.hip does' not in text
