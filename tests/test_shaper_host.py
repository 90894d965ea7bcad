"""The table-lookup waveshaper without a GPU: the node API of ext.Shaper and its state validation, name resolution and the .sigs
loader, sig_shaper_table's export and argument checks, the Shape instruction's encoding and argument checks (the power-of-two rule
per use), how the engine's planner classifies the node and the programs it compiles for it, the control-path refusal, sharding,
the specialised build of a program with the instruction, and the numpy restatement (tests/shaper_reference.py) against a direct
loop."""
import ctypes
import math
import pathlib
import types

import numpy as np
import pytest

from signals_amd import SignalFlags, _native, specialise
from signals_amd.chain import BadStateValue, BlockCachingEmitter
from signals_amd.chain import ext, fixed, fx, osc

import shaper_reference as SR

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


def saw(hz):
    o = osc.Sawtooth(); o.hertz = fix(hz)
    return o


def shaper_node(table, input_, select=None):
    n = ext.Shaper()
    n.get_state().table = table
    n.input = input_
    if select is not None:
        n.select = fix(select)
    return n


def table_node(table, hertz, select=None):
    n = ext.Wavetable()
    n.get_state().table = table
    n.hertz = fix(hertz)
    if select is not None:
        n.select = fix(select)
    return n


# ---------------------------------------------------------------------------------------------- the restatement
def special_inputs(T):
    eps = 2.0 ** -52
    return np.concatenate([SR.knots(T), [1.0, -1.0, 1.0 + eps, -(1.0 + eps), np.inf, -np.inf, np.nan, 0.0, -0.0],
                           np.random.default_rng(T).uniform(-1.5, 1.5, 4096)])


@pytest.mark.parametrize('T', [2, 5, 2049])
def test_reference_restatement_against_a_direct_loop(T):
    rng = np.random.default_rng(100 + T)
    table = rng.uniform(-1, 1, (T, 3))
    x = special_inputs(T)[:, None]
    select = np.array([[0.0, 1.0, 2.0, -1.0, 5.0, 1.7, np.nan]])
    got = SR.shape(table, x, select)
    floats = SR.python_table(table)                                           # (converted once for the loop below)
    assert got.shape == (x.shape[0], 7) and got.dtype == np.float64
    # every input, every column rule (the columns 0, 1, 2 and the clipped / NaN selects): no case is left out
    for r in range(x.shape[0]):
        for v in range(7):
            want = SR.shaper_loop(floats, float(x[r, 0]), float(select[0, v]))
            assert got[r, v] == want or (math.isnan(want) and math.isnan(got[r, v])), (T, r, v, x[r, 0])
    tbl = table.astype(np.float32).astype(np.float64)
    assert np.array_equal(got[:T, 1], tbl[:, 1])                              # on a knot: the entry itself
    at = {v: T + k for k, v in enumerate(('+1', '-1', '+1+', '-1-', '+inf', '-inf', 'nan', '+0', '-0'))}
    for name in ('+1', '+1+', '+inf'):
        assert got[at[name], 0] == tbl[T - 1, 0]                              # the last segment at f = 1; beyond: clipped
    for name in ('-1', '-1-', '-inf'):
        assert got[at[name], 0] == tbl[0, 0]
    assert np.isnan(got[at['nan']]).all() and not np.isnan(np.delete(got, at['nan'], axis=0)).any()
    assert got[at['+0'], 0] == got[at['-0'], 0]
    if T % 2:
        assert got[at['+0'], 2] == tbl[(T - 1) // 2, 2]                       # 2^k + 1 points: a knot at x = 0


def test_reference_renders_blocks_with_per_block_rows_and_the_curves():
    table = np.concatenate([SR.tanh_curve(9, 3.0), SR.chebyshev_curve(9, 3)], axis=1)
    x = np.linspace(-1.2, 1.2, 8)[:, None] * np.ones((1, 2))
    got = SR.shaper(table, x, select=[[0.0, 1.0], [1.0, 0.0]], blocks=2)
    want = np.concatenate([SR.shape(table, x[:4], [[0.0, 1.0]]), SR.shape(table, x[4:], [[1.0, 0.0]])])
    assert np.array_equal(got, want)
    t = SR.tanh_curve(513, 3.0)
    assert t.shape == (513, 1) and t[0, 0] == -1.0 and t[256, 0] == 0.0 and t[512, 0] == 1.0
    assert abs(SR.lipschitz(t) - 3.0 / np.tanh(3.0)) < 0.01                   # about 3: the slope at 0
    c = SR.chebyshev_curve(513, 3)
    assert np.allclose(c[:, 0], 4 * SR.knots(513) ** 3 - 3 * SR.knots(513)) and 8.9 < SR.lipschitz(c) <= 9.0
    f = SR.fold_curve(513, 2.5)
    assert abs(f).max() <= 1.0 and f[256, 0] == 0.0 and abs(SR.lipschitz(f) - 2.5) < 1e-6
    assert SR.lipschitz(np.array([[-1.0], [1.0]])) == 1.0                     # the default table: the identity


# ---------------------------------------------------------------------------------------------- the node
def test_node_api():
    cls = ext.Shaper
    assert cls.port_names() == ['input', 'select']
    assert cls.flags() & SignalFlags.EFFECT and not cls.flags() & SignalFlags.GENERATOR
    assert issubclass(cls, BlockCachingEmitter) and not issubclass(cls, fx.Effect)
    assert 'table' in cls().state_attrs()
    assert np.array_equal(cls().get_state().table, [[-1.0], [1.0]])           # the identity on [-1, 1]: a hard clip
    n = shaper_node(np.zeros((5, 3)), saw(np.full((1, 6), 220.0)), select=[[1.0]])
    assert n.channels == 6                                                    # ImplicitChannels: the one width that is not 1
    n.select = fix(np.zeros((1, 4)))
    with pytest.raises(ValueError):
        n.channels                                                            # 6 and 4: no single width
    doc = cls.__doc__
    for words in ('clip(x, -1, 1)', 'min(floor(u), T - 2)', 'Out of scope', 'control path', 'band filter', 'phase-modulation',
                  'oversampling', 'morphing', 'frame-rate `select`', 'closed-form, row-walker and cascade'):
        assert words in doc, words


@pytest.mark.parametrize('bad', [np.zeros(8), np.zeros((2, 2, 2)), np.zeros((1, 4)), np.zeros((2, 1), dtype=complex), np.zeros((16385, 1)),
                                 np.zeros((8192, 3)), np.zeros((4, 0)), [[0.0], [1.0]], None, np.array([['a'], ['b']])],
                         ids=['1-D', '3-D', 'T=1', 'complex', 'T*W=16385', 'T*W=24576', 'W=0', 'a list', 'None', 'strings'])
def test_state_validation_refuses(bad):
    n = ext.Shaper()
    with pytest.raises(BadStateValue):
        n.get_state().table = bad


def test_state_validation_accepts():
    n = ext.Shaper()
    for good in (np.zeros((2, 1)), np.zeros((3, 1)), np.zeros((2049, 7)), np.zeros((16384, 1)), np.zeros((2, 8192)),
                 np.zeros((48, 3), dtype=np.float32), np.array([[-1], [0], [1]]), np.arange(6, dtype=np.uint8).reshape(3, 2)):
        n.get_state().table = good
    n.get_state().table = np.array([[-3], [0], [3]])                          # int64, what a .sigs value arrives as
    assert n.get_state().table.dtype == np.int64
    got = n.resident_table()                                                  # (the CPU device here) converted to float32
    assert got.dtype.is_floating_point and got.element_size() == 4 and got.tolist() == [[-3.0], [0.0], [3.0]]
    n.get_state().table[1, 0] = 5                                             # an in-place edit is seen at the next reply
    assert n.resident_table().tolist() == [[-3.0], [5.0], [3.0]]


def test_class_resolves_by_qualified_name_and_loads_from_a_patch():
    from signals_amd.chain import discovery, sigs
    from signals_amd.chain.driver import load_signal
    assert load_signal('signals_amd.chain.ext.Shaper') is ext.Shaper
    assert load_signal('signals.chain.ext.Shaper') is ext.Shaper
    assert discovery.load_signal('signals.chain.ext.Shaper') is ext.Shaper
    p = sigs.loads('+ 1a signals.chain.fixed.Fixed value=[[220.0]]\n+ 1b signals.chain.fixed.Fixed value=[[1]]\n'
                   '+ 1c signals.chain.osc.Sawtooth\n'
                   '+ 2a signals.chain.ext.Shaper table=[[-1,-2],[0,0],[1,2]]\n> 1a 1c.hertz\n> 1c 2a.input\n> 1b 2a.select')
    node = p['2a']
    assert isinstance(node, ext.Shaper) and node.input.sig is p['1c'] and node.select.sig is p['1b']
    assert node.get_state().table.shape == (3, 2) and node.get_state().table.dtype.kind == 'i'
    with pytest.raises(BadStateValue):
        sigs.loads('+ 1a signals.chain.ext.Shaper table=[[0]]')


# ---------------------------------------------------------------------------------------------- C ABI
def test_entry_point_is_exported_and_declared(lib):
    assert 'sig_shaper_table' in _native.EXPORTS
    raw = ctypes.CDLL(str(_native.LIB_PATH))
    assert raw.sig_shaper_table is not None
    assert lib.sig_abi_version() == 7                                         # additive, like sig_osc_bank_table
    header = (ROOT / 'include' / 'signals_amd.h').read_text()
    assert 'SIG_VP_SHAPE = 14' in header and 'int sig_shaper_table(' in header
    assert '#define SIG_ABI_VERSION 7' in header


def test_shaper_table_argument_errors_do_not_reach_the_device(lib):
    p = 64                                                                    # (never dereferenced: every call fails its checks)
    args = dict(rows=256, voices=8, x=p, xdt=0, xld=8, xs=1, select=p, ss=1, srs=0, rps=0, table=p, T=5, W=3,
                out=p, odt=0, old=8, stream=None)

    def call(**over):
        a = dict(args, **over)
        return lib.sig_shaper_table(*(a[k] for k in args))
    assert call(table=None) == INV and call(x=None) == INV and call(out=None) == INV
    assert call(T=1) == INV and call(T=0) == INV and call(T=-3) == INV        # T >= 2
    assert call(T=2049, W=8) == INV and call(T=16384, W=2) == INV and call(T=2, W=8193) == INV   # over the cap
    assert call(W=0) == INV
    assert call(old=4) == INV                                                 # rows narrower than the voices
    assert call(xld=4) == INV and call(xs=2) == INV and call(xld=-8) == INV   # input rows: narrower than the voices, strides 0 / 1
    assert call(ss=2) == INV and call(srs=-1) == INV and call(rps=-1) == INV  # select rows: strides 0 / 1, row stride >= 0
    assert call(odt=2) == INV and call(xdt=2) == INV and call(rows=-1) == INV and call(voices=-1) == INV
    assert call(rows=0) == 0 and call(voices=0, old=0) == 0                   # accepted, nothing to launch
    assert call(rows=0, T=3) == 0 and call(rows=0, T=48) == 0                 # any T >= 2, no power of two asked
    assert call(rows=0, T=2049, W=7) == 0 and call(rows=0, T=2, W=8192) == 0  # the cap itself is inside
    assert call(rows=0, xld=0, xs=0, select=None) == 0                        # a one-row, one-column input; select unplugged


def test_instruction_encoding():
    assert _native.VP_OPS['Shape'] == 14
    assert _native.voice_program_words([('Shape', 0, 0, 0, -1)]) == [0xf000e]             # no select: slot 15
    assert _native.voice_program_words([('Shape', 0, 0, 1, 2)]) == [0x2100e]
    assert 'Shape' not in _native.VP_EXT_OPS and _native.VP_TABLE_OPS == ('OscTable', 'Shape')


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


def test_voice_program_shape_programs(lib):
    buf = (ctypes.c_float * 64)()

    def tables(*geometry):
        t = _native.VpTablesT()
        t.n_tables = len(geometry)
        for k, (ptr, points, waves) in enumerate(geometry):
            t.table[k] = _native.VpTable(ptr, points, waves)
        return t

    def run(code, tabs, nblocks=1, **kw):
        P, keep = _program(code, **kw)
        return lib.sig_voice_program_ex(ctypes.byref(P), 48000, 0, 256, nblocks, 100, 8, 2 if nblocks else 1, 0, None, 0, None, 0, 0, None,
                                        ctypes.addressof(buf), 8, None, None, ctypes.byref(tabs) if tabs is not None else None)
    one = tables((64, 5, 3))
    src, shape = ('Osc', 2, 0, 0, 0), ('Shape', 0, 0, 0, -1)
    assert run([src, shape], None) == INV                                     # the instruction without its tables
    assert run([src, shape], tables()) == INV
    assert run([src, ('Shape', 0, 0, 1, -1)], one) == INV                     # table slot 1 of 1
    assert run([src, ('Shape', 0, 0, 0, 1)], one) == INV                      # select: parameter slot 1 of 1
    assert run([src, ('Shape', 0, 0, 0, 0)], one, n_params=0) == INV
    assert run([src, ('Shape', 0, 0, 0, -2)], one) == INV
    assert run([src, shape], tables((None, 5, 3))) == INV                     # null table
    assert run([src, shape], tables((64, 1, 4))) == INV                       # T = 1
    assert run([src, shape], tables((64, 2049, 8))) == INV                    # over the cap
    assert run([src, shape], tables((64, 2049, 4), (64, 2049, 4))) == INV     # the cap is shared
    assert run([src, shape, ('Band', 0, 0, 0, 0)], one, types=['bp', 'bp']) == INV        # no variant with a band ...
    assert run([src, shape, ('OscPM', 0, 1, 0, 0)], one, n_oscs=2) == INV     # ... or a PM carrier
    # accepted (no blocks: no launch): Shape on a 5-point and on a 48-point table, with and without select
    assert run([src, shape], one, nblocks=0) == 0
    assert run([src, ('Shape', 0, 0, 0, 0)], tables((64, 48, 1)), nblocks=0) == 0
    assert run([src, ('Shape', 0, 0, 1, -1)], tables((64, 64, 1), (64, 3, 2)), nblocks=0) == 0
    # the power-of-two rule is per use: an OscTable word keeps it, also on a slot a Shape word shares
    look = ('OscTable', 0, 0, 0, -1)
    assert run([look], tables((64, 48, 1))) == INV
    assert run([look, shape], tables((64, 48, 1))) == INV                     # one 48-point slot read by both
    assert run([look, shape], tables((64, 64, 1)), nblocks=0) == 0
    assert run([look, ('Shape', 0, 0, 1, -1)], tables((64, 64, 1), (64, 48, 1)), nblocks=0) == 0     # each its own slot
    assert run([look, ('Shape', 0, 0, 1, -1)], tables((64, 48, 1), (64, 64, 1))) == INV
    # sig_voice_program is the same call without tables
    P, keep = _program([src, shape])
    assert lib.sig_voice_program(ctypes.byref(P), 48000, 0, 256, 1, 100, 8, 2, 0, None, 0, None, 0, 0, None,
                                 ctypes.addressof(buf), 8, None, None) == INV


# ---------------------------------------------------------------------------------------------- planning
def test_purity_and_modulation_classification():
    from signals_amd.engine import _KNOWN_TYPES, _audio_ports, _control_ports, _ctl_const, _foreign, _is_pure, _modulated
    assert ext.Shaper in _KNOWN_TYPES
    s = shaper_node(np.zeros((5, 2)), saw([[440.0]]), select=[[1.0]])
    assert not _foreign(s)
    assert _control_ports(s) == [s.select] and _audio_ports(s) == [s.input]
    assert all(_ctl_const(p) for p in _control_ports(s)) and not _modulated(s) and _is_pure(s, {})       # position-pure like Gain
    swept = shaper_node(np.zeros((5, 2)), saw([[440.0]])); swept.select = sine([[2.0]])
    assert _modulated(swept) and not _is_pure(swept, {})                      # select re-read every block: tails
    lp = fx.LowPass(); lp.input = saw([[440.0]]); lp.cutoff = fix([[900.0]])
    assert not _is_pure(shaper_node(np.zeros((5, 2)), lp), {})                # behind a filter: as impure as its input


def test_voice_program_words():
    from signals_amd.engine import _VoiceProgram
    V = 8
    row = lambda lo, hi: np.linspace(lo, hi, V).reshape(1, V)
    curve = SR.tanh_curve(513, 3.0)
    s = shaper_node(curve, saw(row(220, 440)))
    prog = _VoiceProgram(None, s, V)
    assert prog.code == [('Osc', _native.OSC_KINDS['Sawtooth'], 0, 0, 0), ('Shape', 0, 0, 0, -1)]     # the input, then the word
    assert _native.voice_program_words(prog.code) == [0x40, 0xf000e]
    assert (len(prog.oscs), len(prog.params), len(prog.filters), prog.n_temps, prog.depth) == (1, 0, 0, 0, 0)
    assert prog.tables == [s]
    batch = types.SimpleNamespace(owner=types.SimpleNamespace(specialise=False), N=256, _pure={})
    assert _VoiceProgram(batch, s, V).worthwhile()                            # the SMALL register file

    sel = shaper_node(curve, saw(row(220, 440)), select=row(0, 2))
    assert _VoiceProgram(None, sel, V).code[-1] == ('Shape', 0, 0, 0, 0)      # select = parameter 0

    # Shaper(LowPass(Wavetable)) sharing one array: one slot, read by both words (a power of two then); the depth is the input's
    shared = np.zeros((64, 2))
    lp = fx.LowPass(); lp.input = table_node(shared, row(220, 440)); lp.cutoff = fix(row(500, 5000))
    both = shaper_node(shared, lp)
    prog = _VoiceProgram(None, both, V)
    assert prog.code == [('OscTable', 0, 0, 0, -1), ('Filter', 0, 0, 0, 0), ('Shape', 0, 0, 0, -1)]
    assert len(prog.tables) == 1 and prog.depth == 1

    # two Shapers with two arrays: two slots; a third array: no program, the graph stays per node
    inner = shaper_node(SR.fold_curve(513, 2.0), saw(row(220, 440)))
    two = shaper_node(curve, inner)
    prog = _VoiceProgram(None, two, V)
    assert [ins for ins in prog.code if ins[0] == 'Shape'] == [('Shape', 0, 0, 0, -1), ('Shape', 0, 0, 1, -1)]
    assert prog.tables == [inner, two]
    three = shaper_node(SR.chebyshev_curve(513, 3), shaper_node(curve, shaper_node(SR.fold_curve(513, 2.0), saw(row(220, 440)))))
    assert _VoiceProgram.compile(None, three, V) is None
    big = shaper_node(np.zeros((2049, 4)), shaper_node(np.zeros((2049, 4)), saw(row(220, 440))))
    assert _VoiceProgram.compile(None, big, V) is None                        # two that do not fit the cap together

    # with a band filter, or a PM carrier: no interpreter variant has both, the per-node schedule keeps the graph
    bp = fx.BandPass(); bp.input = shaper_node(curve, saw(row(220, 440))); bp.low = fix(row(300, 400)); bp.high = fix(row(900, 1200))
    assert _VoiceProgram.compile(None, bp, V) is None
    pm = ext.PMSine(); pm.hertz = fix(row(220, 440)); pm.index = fix([[1.0]]); pm.mod = saw(row(110, 220))
    assert _VoiceProgram.compile(None, shaper_node(curve, pm), V) is None


def test_shaper_in_a_control_path_is_refused_with_its_reason():
    from signals_amd.engine import NotBatchable, _Batch, _ControlProgram
    s = shaper_node(SR.tanh_curve(9, 3.0), sine([[3.0]]))
    with pytest.raises(NotBatchable, match='waveshaper has no block-rate program'):
        _ControlProgram((s,), 4)
    g = fx.Gain(); g.left = s; g.right = fix([[100.0]])
    with pytest.raises(NotBatchable, match='waveshaper has no block-rate program'):
        _ControlProgram((g,), 4)
    lp = fx.LowPass(); lp.input = s; lp.cutoff = fix([[10.0]])
    with pytest.raises(NotBatchable, match='waveshaper has no block-rate program'):
        _ControlProgram((lp,), 4, channels=1)
    batch = _Batch(types.SimpleNamespace(rate=48000), 0, 256, 4, False)
    with pytest.raises(NotBatchable, match='waveshaper has no block-rate schedule'):
        batch._control_node(s, 'right')


def test_sharded_renderer_hands_every_rank_the_table_and_its_slice_of_select(monkeypatch):
    """parallel.ShardedRenderer plans rank r's engine over build(lo, hi): the rank's Shaper carries the one table array and its own
    columns of select, and its voice program stages that table -- nothing in parallel.py knows the node"""
    from signals_amd import parallel
    from signals_amd.engine import BatchRenderer, _VoiceProgram
    V, world, table = 12, 3, np.linspace(-1, 1, 10).reshape(5, 2)
    hertz, select = np.linspace(100, 200, V)[None, :], (np.arange(V) % 2)[None, :].astype(float)
    built = {}

    def build(lo, hi):
        s = shaper_node(table, saw(hertz[:, lo:hi]), select=select[:, lo:hi])
        g = fx.Gain(); g.left = s; g.right = sine([[3.0]])
        bus = ext.SumBus(); bus.input = g
        built[(lo, hi)] = s
        return bus
    monkeypatch.setattr(parallel.dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(parallel.dist, 'get_world_size', lambda: world)
    covered = []
    for rank in range(world):
        monkeypatch.setattr(parallel.dist, 'get_rank', lambda rank=rank: rank)
        r = parallel.ShardedRenderer(build, V, 1, fuse_program='always')
        assert (r.rank, r.world) == (rank, world) and (r.lo, r.hi) == parallel.shard_voices(V, world, rank)
        assert isinstance(r.renderer, BatchRenderer) and r.renderer.fuse_program == 'always'
        s = built[(r.lo, r.hi)]
        assert r.renderer.node.input.sig.left.sig is s and s.channels == r.hi - r.lo
        assert s.get_state().table is table                                   # replicated: the same array on every shard
        assert np.array_equal(s.select.sig.get_state().value, select[:, r.lo:r.hi])      # scattered like hertz
        assert np.array_equal(s.input.sig.hertz.sig.get_state().value, hertz[:, r.lo:r.hi])
        prog = _VoiceProgram(None, r.renderer.node.input.sig, r.hi - r.lo)
        assert prog.tables == [s] and prog.code[:2] == [('Osc', _native.OSC_KINDS['Sawtooth'], 0, 0, 0), ('Shape', 0, 0, 0, 0)]
        covered += list(range(r.lo, r.hi))
    assert covered == list(range(V))


# ---------------------------------------------------------------------------------------------- specialised build
def test_flags_of_a_shape_program():
    code = [('Osc', 2, 0, 0, 0), ('Shape', 0, 0, 0, -1)]
    f = set(specialise.flags(code, 1, 0, 0, 0, 2, 2))
    assert {'-DSIG_VP_STATIC_CODE={0x40,0xf000e}', '-DSIG_VP_S_TAB=1', '-DSIG_VP_S_NO=1', '-DSIG_VP_S_EXT=0'} <= f
    assert '-DSIG_VP_S_TAB=1' in specialise.flags([('OscTable', 0, 0, 0, -1)], 1, 0, 0, 0, 2, 2)
    plain = specialise.flags([('Osc', 2, 0, 0, 0), ('Gain', 0, 0, 0, 0)], 1, 1, 0, 0, 2, 2)
    assert not any('SIG_VP_S_TAB' in x for x in plain)                        # programs without either word keep their flags


@pytest.mark.skipif(specialise.hipcc() is None, reason='no hipcc in this environment')
def test_the_specialised_shape_program_builds(tmp_path, monkeypatch):
    monkeypatch.setattr(specialise, 'CACHE', tmp_path)
    code = [('Osc', 2, 0, 0, 0), ('Shape', 0, 0, 0, 0), ('Gain', 0, 1, 0, 0)]
    image = specialise.build(code, 1, 2, 0, 0, 2, 2)
    assert b'sig_vp_specialised' in image and b'sig_vp_specialised_info' in image
