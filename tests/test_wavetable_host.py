"""The wavetable oscillator without a GPU: the node API of ext.Wavetable and its state validation, name resolution and the .sigs
loader, sig_osc_bank_table's export and argument checks, the OscTable instruction's encoding and argument checks, how the engine's
planner classifies the node and the programs it compiles for it, the specialised build of a program with the instruction, and the
numpy restatement (tests/wavetable_reference.py) against a direct loop."""
import ctypes
import pathlib
import types

import numpy as np
import pytest

from signals_amd import SignalFlags, _native, specialise
from signals_amd.chain import BadStateValue, BlockCachingEmitter
from signals_amd.chain import ext, fixed, fx, osc

from wavetable_reference import band_limited_saw, lookup, wavetable, wavetable_loop

ROOT = pathlib.Path(__file__).resolve().parent.parent
INV = 1     # hipErrorInvalidValue


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


def sine(hz):
    o = osc.Sine(); o.hertz = fix(hz)
    return o


def table_node(table, hertz, select=None):
    n = ext.Wavetable()
    n.get_state().table = table
    n.hertz = fix(hertz)
    if select is not None:
        n.select = fix(select)
    return n


# ---------------------------------------------------------------------------------------------- the node
def test_node_api():
    cls = ext.Wavetable
    assert cls.port_names() == ['hertz', 'phase', 'select']
    assert cls.flags() & SignalFlags.GENERATOR
    assert issubclass(cls, BlockCachingEmitter) and not issubclass(cls, osc.Osc)
    assert 'table' in cls().state_attrs()
    n = table_node(np.zeros((8, 3)), np.full((1, 6), 220.0), select=[[1.0]])
    assert n.channels == 6                                                    # ImplicitChannels: the one width that is not 1
    n.select = fix(np.zeros((1, 4)))
    with pytest.raises(ValueError):
        n.channels                                                            # 6 and 4: no single width


@pytest.mark.parametrize('bad', [np.zeros(8), np.zeros((2, 2, 2)), np.zeros((3, 1)), np.zeros((1, 4)), np.zeros((16385, 1)),
                                 np.zeros((8192, 3)), np.zeros((4, 0)), [[0.0], [1.0]], None,
                                 np.array([['a'], ['b']])],
                         ids=['1-D', '3-D', 'T=3', 'T=1', 'T*W=16385', 'T*W=24576', 'W=0', 'a list', 'None', 'strings'])
def test_state_validation_refuses(bad):
    n = ext.Wavetable()
    with pytest.raises(BadStateValue):
        n.get_state().table = bad


def test_state_validation_accepts():
    n = ext.Wavetable()
    for good in (np.zeros((2, 1)), np.zeros((2048, 8)), np.zeros((16384, 1)), np.zeros((2, 8192)), np.zeros((64, 3), dtype=np.float32),
                 np.array([[0], [1], [0], [-1]]), np.arange(8, dtype=np.uint8).reshape(4, 2)):
        n.get_state().table = good
    n.get_state().table = np.array([[0], [3], [0], [-3]])                      # int64, what a .sigs value arrives as
    assert n.get_state().table.dtype == np.int64
    got = n.resident_table()                                                  # (the CPU device here) converted to float32
    assert got.dtype.is_floating_point and got.element_size() == 4 and got.tolist() == [[0.0], [3.0], [0.0], [-3.0]]
    n.get_state().table[1, 0] = 5                                             # an in-place edit is seen at the next reply
    assert n.resident_table().tolist() == [[0.0], [5.0], [0.0], [-3.0]]


def test_class_resolves_by_qualified_name_and_loads_from_a_patch():
    from signals_amd.chain import discovery, sigs
    from signals_amd.chain.driver import load_signal
    assert load_signal('signals_amd.chain.ext.Wavetable') is ext.Wavetable
    assert load_signal('signals.chain.ext.Wavetable') is ext.Wavetable
    assert discovery.load_signal('signals.chain.ext.Wavetable') is ext.Wavetable
    p = sigs.loads('+ 1a signals.chain.fixed.Fixed value=[[220.0]]\n+ 1b signals.chain.fixed.Fixed value=[[1]]\n'
                   '+ 2a signals.chain.ext.Wavetable table=[[0,0],[1,2],[0,0],[-1,-2]]\n> 1a 2a.hertz\n> 1b 2a.select')
    node = p['2a']
    assert isinstance(node, ext.Wavetable) and node.hertz.sig is p['1a'] and node.select.sig is p['1b']
    assert node.get_state().table.shape == (4, 2) and node.get_state().table.dtype.kind == 'i'
    with pytest.raises(BadStateValue):
        sigs.loads('+ 1a signals.chain.ext.Wavetable table=[[0],[1],[0]]')


# ---------------------------------------------------------------------------------------------- C ABI
def test_entry_points_are_exported_and_declared(lib):
    assert 'sig_osc_bank_table' in _native.EXPORTS and 'sig_voice_program_ex' in _native.EXPORTS
    raw = ctypes.CDLL(str(_native.LIB_PATH))
    assert raw.sig_osc_bank_table is not None and raw.sig_voice_program_ex is not None
    assert lib.sig_abi_version() == 7
    header = (ROOT / 'include' / 'signals_amd.h').read_text()
    assert 'SIG_VP_OSCTABLE = 13' in header and 'int sig_osc_bank_table(' in header and 'int sig_voice_program_ex(' in header
    assert '#define SIG_ABI_VERSION 7' in header and 'SIG_TABLE_MAX_POINTS = 16384' in header
    assert _native.TABLE_MAX_POINTS == 16384 and _native.VP_MAX_TABLES == 2


def test_osc_bank_table_argument_errors_do_not_reach_the_device(lib):
    p = 64                                                                    # (never dereferenced: every call fails its checks)
    args = dict(position=0, step=1, rate=48000, rows=256, voices=8, rpp=0, hertz=p, hs=1, hrs=0, phase=None, ps=0, prs=0,
                select=p, ss=1, srs=0, table=p, T=64, W=3, out=p, odt=0, old=8, stream=None)

    def call(**over):
        a = dict(args, **over)
        return lib.sig_osc_bank_table(*(a[k] for k in args))
    assert call(table=None) == INV                                            # null table
    assert call(T=3) == INV and call(T=48) == INV and call(T=1) == INV and call(T=0) == INV      # not a power of two >= 2
    assert call(T=2048, W=9) == INV and call(T=16384, W=2) == INV and call(T=2, W=8193) == INV   # over the cap
    assert call(W=0) == INV
    assert call(old=4) == INV                                                 # rows narrower than the voices
    assert call(hertz=None) == INV and call(out=None) == INV
    assert call(ss=2) == INV and call(srs=-1) == INV                          # select rows: strides 0 / 1, row stride >= 0
    assert call(odt=2) == INV and call(rate=0) == INV and call(position=-1) == INV and call(step=0) == INV
    assert call(rows=0) == 0 and call(voices=0, old=0) == 0                   # accepted, nothing to launch
    assert call(rows=0, T=2048, W=8) == 0 and call(rows=0, T=2, W=8192) == 0  # the cap itself is inside


def test_instruction_encoding():
    assert _native.VP_OPS['OscTable'] == 13
    assert _native.voice_program_words([('OscTable', 0, 0, 0, -1)]) == [0xf000d]          # no select: slot 15
    assert _native.voice_program_words([('OscTable', 0, 1, 1, 2)]) == [0x2110d]
    assert 'OscTable' not in _native.VP_EXT_OPS


def _program(code, n_oscs=1, n_params=1, types=()):
    P = _native.VoiceProgramT()
    P.n_ins = len(code)
    for k, (op, kind, a, b, c) in enumerate(code):
        P.ins[k] = _native.VpIns(_native.VP_OPS[op], kind, a, b, c)
    row = ctypes.c_double(440.0)
    ptr = ctypes.cast(ctypes.pointer(row), ctypes.c_void_p).value
    P.n_oscs = n_oscs
    for k in range(n_oscs):
        P.hertz[k] = _native.VpRows(ptr, 0, 1)
        P.phase[k] = _native.VpRows(None, 0, 1)
    P.n_params = n_params
    for k in range(n_params):
        P.params[k] = _native.VpRows(ptr, 0, 1)
    P.n_filters = len(types)
    for k, t in enumerate(types):
        P.cutoff[k] = _native.VpRows(ptr, 0, 1)
        P.filter_type[k] = _native.FILT_TYPES[t]
        P.filter_level[k] = 1
    P.depth = 1 if types else 0
    return P, row


def test_voice_program_refuses_bad_table_programs(lib):
    buf = (ctypes.c_float * 64)()

    def tables(*geometry):
        t = _native.VpTablesT()
        t.n_tables = len(geometry)
        for k, (ptr, points, waves) in enumerate(geometry):
            t.table[k] = _native.VpTable(ptr, points, waves)
        return t

    def run(code, tabs, **kw):
        P, keep = _program(code, **kw)
        return lib.sig_voice_program_ex(ctypes.byref(P), 48000, 0, 256, 1, 100, 8, 2, 0, None, 0, None, 0, 0, None,
                                        ctypes.addressof(buf), 8, None, None, ctypes.byref(tabs) if tabs is not None else None)
    one = tables((64, 64, 3))
    look = ('OscTable', 0, 0, 0, -1)
    assert run([look], None) == INV                                           # the instruction without its tables
    assert run([look], tables()) == INV
    assert run([('OscTable', 0, 0, 1, -1)], one) == INV                       # table slot 1 of 1
    assert run([('OscTable', 0, 1, 0, -1)], one) == INV                       # oscillator slot 1 of 1
    assert run([('OscTable', 0, 0, 0, 1)], one) == INV                        # select: parameter slot 1 of 1
    assert run([('OscTable', 0, 0, 0, 0)], one, n_params=0) == INV
    assert run([look], tables((None, 64, 3))) == INV                          # null table
    assert run([look], tables((64, 48, 1))) == INV and run([look], tables((64, 1, 4))) == INV     # not a power of two >= 2
    assert run([look], tables((64, 2048, 9))) == INV                          # over the cap
    assert run([look], tables((64, 2048, 4), (64, 2048, 5))) == INV           # the cap is shared
    P, keep = _program([look])
    bad = tables((64, 64, 3))
    bad.n_tables = 3
    assert run([look], bad) == INV
    assert run([look, ('Band', 0, 0, 0, 0)], one, types=['bp', 'bp']) == INV  # no variant with a band ...
    assert run([look, ('OscPM', 0, 1, 0, 0)], one, n_oscs=2) == INV   # ... or a PM carrier
    # sig_voice_program is the same call without tables
    P, keep = _program([look])
    assert lib.sig_voice_program(ctypes.byref(P), 48000, 0, 256, 1, 100, 8, 2, 0, None, 0, None, 0, 0, None,
                                 ctypes.addressof(buf), 8, None, None) == INV
    P, keep = _program([look])
    assert lib.sig_voice_program_ex(ctypes.byref(P), 48000, 0, 256, 0, 100, 8, 1, 0, None, 0, None, 0, 0, None,
                                    ctypes.addressof(buf), 8, None, None, ctypes.byref(one)) == 0       # no blocks: no launch


# ---------------------------------------------------------------------------------------------- planning
def test_purity_and_modulation_classification():
    from signals_amd.engine import _KNOWN_TYPES, _audio_ports, _control_ports, _ctl_const, _foreign, _is_pure, _modulated
    assert ext.Wavetable in _KNOWN_TYPES
    w = table_node(np.zeros((8, 2)), [[440.0]], select=[[1.0]])
    assert not _foreign(w)
    assert _control_ports(w) == [w.hertz, w.phase, w.select] and _audio_ports(w) == []       # a leaf
    assert all(_ctl_const(p) for p in _control_ports(w)) and not _modulated(w) and _is_pure(w, {})
    swept = table_node(np.zeros((8, 2)), [[440.0]]); swept.select = sine([[2.0]])
    assert _modulated(swept) and not _is_pure(swept, {})                      # select re-read every block: tails
    vib = ext.Wavetable(); vib.hertz = sine([[5.0]])
    assert _modulated(vib)
    g = fx.Gain(); g.left = w; g.right = fix([[0.5]])
    assert _is_pure(g, {})


def test_voice_program_words():
    from signals_amd.engine import _VoiceProgram
    V = 8
    row = lambda lo, hi: np.linspace(lo, hi, V).reshape(1, V)
    table = np.zeros((64, 3))
    w = table_node(table, row(220, 440), select=row(0, 2))
    g = fx.Gain(); g.left = w; g.right = sine([[3.0]])                        # (a modulated gain stays an instruction)
    prog = _VoiceProgram(None, g, V)
    assert prog.code == [('OscTable', 0, 0, 0, 0), ('Gain', 0, 1, 0, 0)]      # oscillator slot 0, table slot 0, select = parameter 0
    assert _native.voice_program_words(prog.code) == [0x0000d, 0x102]
    assert (len(prog.oscs), len(prog.params), len(prog.filters), prog.n_temps, prog.depth) == (1, 2, 0, 0, 0)
    assert prog.tables == [w]

    bare = table_node(table, row(220, 440))                                   # select unplugged: c = -1
    assert _VoiceProgram(None, bare, V).code == [('OscTable', 0, 0, 0, -1)]

    # Mix of two Wavetables on different columns of ONE table (the same state array): one table slot
    a = table_node(table, row(220, 440), select=[[0.0]])
    b = table_node(table, row(220, 440), select=[[2.0]])
    m = fx.Mix(); m.left = a; m.right = b; m.mix = fix([[0.25]])
    prog = _VoiceProgram(types.SimpleNamespace(owner=types.SimpleNamespace(specialise=False), N=256, _pure={}), m, V)
    assert prog.code == [('OscTable', 0, 0, 0, 0), ('Save', 0, 0, 0, 0), ('OscTable', 0, 1, 0, 1), ('Mix', 0, 0, 2, 0)]
    assert len(prog.tables) == 1 and prog.n_temps == 1 and prog.worthwhile()  # the SMALL register file
    # two arrays: two slots; a third, or two that do not fit the cap together: no program
    c = table_node(np.zeros((64, 3)), row(220, 440))
    m.right = c
    prog = _VoiceProgram(None, m, V)
    assert [ins for ins in prog.code if ins[0] == 'OscTable'] == [('OscTable', 0, 0, 0, 0), ('OscTable', 0, 1, 1, -1)]
    big1, big2 = table_node(np.zeros((2048, 5)), row(220, 440)), table_node(np.zeros((2048, 4)), row(220, 440))
    m.left, m.right = big1, big2
    assert _VoiceProgram.compile(None, m, V) is None

    # behind a filter, under an envelope
    lp = fx.LowPass(); lp.input = bare; lp.cutoff = fix(row(500, 5000))
    prog = _VoiceProgram(None, lp, V)
    assert prog.code == [('OscTable', 0, 0, 0, -1), ('Filter', 0, 0, 0, 0)] and prog.depth == 1

    # with a band filter, or a PM carrier: no interpreter variant has both, the per-node schedule keeps the graph
    bp = fx.BandPass(); bp.input = table_node(table, row(220, 440)); bp.low = fix(row(300, 400)); bp.high = fix(row(900, 1200))
    assert _VoiceProgram.compile(None, bp, V) is None
    pm = ext.PMSine(); pm.hertz = fix(row(220, 440)); pm.index = fix([[1.0]]); pm.mod = table_node(table, row(110, 220))
    assert _VoiceProgram.compile(None, pm, V) is None


def test_wavetable_in_a_control_path_is_refused_with_its_reason():
    from signals_amd.engine import NotBatchable, _Batch, _ControlProgram
    w = table_node(np.zeros((8, 1)), [[3.0]])
    with pytest.raises(NotBatchable, match='wavetable oscillator has no block-rate program'):
        _ControlProgram((w,), 4)
    g = fx.Gain(); g.left = w; g.right = fix([[100.0]])
    with pytest.raises(NotBatchable, match='wavetable oscillator has no block-rate program'):
        _ControlProgram((g,), 4)
    lp = fx.LowPass(); lp.input = w; lp.cutoff = fix([[10.0]])
    with pytest.raises(NotBatchable, match='wavetable oscillator has no block-rate program'):
        _ControlProgram((lp,), 4, channels=1)
    batch = _Batch(types.SimpleNamespace(rate=48000), 0, 256, 4, False)
    with pytest.raises(NotBatchable, match='wavetable oscillator has no block-rate schedule'):
        batch._control_node(w, 'hertz')


def test_sharded_renderer_hands_every_rank_the_table_and_its_slice_of_select(monkeypatch):
    """parallel.ShardedRenderer plans rank r's engine over build(lo, hi): the rank's Wavetable carries the one table array and its own
    columns of hertz / select, and its voice program stages that table"""
    from signals_amd import parallel
    from signals_amd.engine import BatchRenderer, _VoiceProgram
    V, world, table = 12, 3, np.arange(16.0).reshape(8, 2)
    hertz, select = np.linspace(100, 200, V)[None, :], (np.arange(V) % 2)[None, :].astype(float)
    built = {}

    def build(lo, hi):
        w = table_node(table, hertz[:, lo:hi], select=select[:, lo:hi])
        g = fx.Gain(); g.left = w; g.right = sine([[3.0]])
        bus = ext.SumBus(); bus.input = g
        built[(lo, hi)] = w
        return bus
    monkeypatch.setattr(parallel.dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(parallel.dist, 'get_world_size', lambda: world)
    covered = []
    for rank in range(world):
        monkeypatch.setattr(parallel.dist, 'get_rank', lambda rank=rank: rank)
        r = parallel.ShardedRenderer(build, V, 1, fuse_program='always')
        assert (r.rank, r.world) == (rank, world) and (r.lo, r.hi) == parallel.shard_voices(V, world, rank)
        assert isinstance(r.renderer, BatchRenderer) and r.renderer.fuse_program == 'always'
        w = built[(r.lo, r.hi)]
        assert r.renderer.node.input.sig.left.sig is w and w.channels == r.hi - r.lo
        assert w.get_state().table is table                                   # replicated: the same array on every shard
        assert np.array_equal(w.select.sig.get_state().value, select[:, r.lo:r.hi])      # scattered like hertz
        assert np.array_equal(w.hertz.sig.get_state().value, hertz[:, r.lo:r.hi])
        prog = _VoiceProgram(None, r.renderer.node.input.sig, r.hi - r.lo)
        assert prog.tables == [w] and prog.code[0] == ('OscTable', 0, 0, 0, 0)
        covered += list(range(r.lo, r.hi))
    assert covered == list(range(V))


# ---------------------------------------------------------------------------------------------- specialised build
def test_flags_of_a_table_program():
    code = [('OscTable', 0, 0, 0, -1), ('Filter', 0, 0, 0, 0)]
    f = set(specialise.flags(code, 1, 0, 1, 0, 2, 2))
    assert {'-DSIG_VP_STATIC_CODE={0xf000d,0x1}', '-DSIG_VP_S_NO=1', '-DSIG_VP_S_NF=1', '-DSIG_VP_S_EXT=0'} <= f


@pytest.mark.skipif(specialise.hipcc() is None, reason='no hipcc in this environment')
def test_the_specialised_table_program_builds(tmp_path, monkeypatch):
    monkeypatch.setattr(specialise, 'CACHE', tmp_path)
    code = [('OscTable', 0, 0, 0, 0), ('Filter', 0, 0, 0, 0), ('Gain', 0, 1, 0, 0)]
    image = specialise.build(code, 1, 2, 1, 0, 2, 2)
    assert b'sig_vp_specialised' in image and b'sig_vp_specialised_info' in image


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize('T', [2, 8])
def test_reference_restatement_against_a_direct_loop(T):
    rng = np.random.default_rng(T)
    table = rng.uniform(-1, 1, (T, 3))
    table[0, 1], table[T - 1, 1] = 1.0, -1.0                                  # a jump across the wrap in column 1
    points = np.arange(0, 2 * T + 1) / T - 0.5                                # t exactly on table points, negative ones included
    last = (T - 1 + np.array([0.0, 0.25, 0.5, 0.999])) / T                    # the last segment: interpolates towards entry 0
    t = np.concatenate([points, last, last - 3.0, rng.uniform(-4, 4, 40), [-2.0 ** -60, 1.0 - 2.0 ** -53, 7.0]])[:, None]
    select = np.array([[0.0, 1.0, 2.0, -1.0, 5.0, 1.7, np.nan]])
    got = lookup(table, t, select)
    assert got.shape == (t.shape[0], 7) and got.dtype == np.float64
    for r in range(t.shape[0]):
        for v in range(7):
            assert got[r, v] == wavetable_loop(table, float(t[r, 0]), float(select[0, v])), (r, v)
    tbl = table.astype(np.float32).astype(np.float64)
    on_points = lookup(table, points[:, None], np.array([[1.0]]))[:, 0]
    assert np.array_equal(on_points, tbl[np.arange(-T // 2, 2 * T + 1 - T // 2) % T, 1])      # t on a point: the entry itself
    wrap = lookup(table, np.array([[(T - 0.5) / T]]), np.array([[1.0]]))[0, 0]
    assert wrap == tbl[T - 1, 1] + 0.5 * (tbl[0, 1] - tbl[T - 1, 1]) == 0.0   # half-way along the last segment: between -1 and entry 0's 1
    assert lookup(table, np.array([[-2.0 ** -60]]), np.array([[1.0]]))[0, 0] == tbl[0, 1]      # np.mod rounds to 1.0: u == T wraps


def test_reference_renders_blocks_with_per_block_rows():
    table = band_limited_saw(64, 8)
    hertz = np.array([[100.0, 200.0], [300.0, 400.0]])
    got = wavetable(table, 50, 4, hertz, phase=[[0.25]], blocks=2)
    n = np.arange(50, 58)[:, None]
    want = np.concatenate([lookup(table, n[:4] / 48000 * hertz[:1] + 0.25), lookup(table, n[4:] / 48000 * hertz[1:] + 0.25)])
    assert np.array_equal(got, want)
    assert abs(band_limited_saw(2048, 16)).max() < 1.2 and band_limited_saw(2048, 16).shape == (2048, 1)
