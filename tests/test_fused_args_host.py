"""Argument handling of the 13 fused entry points (signals_amd/csrc/fused_voice.hip), on a host without a device: the checks
run before any HIP call.  For each entry point a well-formed call with no blocks returns 0, and the same call with exactly one
argument spoiled returns hipErrorInvalidValue -- one spoiled argument from every class the entry checks.  The pointers are
host buffers: with no blocks (or a rejected call) nothing dereferences them."""
import ctypes

import pytest

INV = 1     # hipErrorInvalidValue
V = 64      # voices

HEAD = ['osc_kind', 'filt_type', 'rate', 'position', 'block_frames', 'nblocks', 'context', 'voices']
PAIR_HEAD = ['osc_kind', 'osc2_kind', 'pair_op'] + HEAD[1:]
HP = ['hertz', 'hertz_stride', 'phase', 'phase_stride']
HP_FM = ['hertz', 'hertz_stride', 'hertz_rows', 'hertz_hist', 'phase', 'phase_stride', 'phase_rows', 'phase_hist']
PAIR = ['hertz2', 'hertz2_stride', 'phase2', 'phase2_stride', 'mix', 'mix_stride']
CG = ['cutoff', 'cutoff_stride', 'gain', 'gain_stride']
CG_ROWS = ['cutoff', 'cutoff_stride', 'cutoff_rows', 'gain', 'gain_stride', 'gain_rows']
BUS = ['bus_gains', 'bus_gains_ld', 'bus_channels', 'workspace']
TAIL = ['out', 'out_ld', 'status', 'stream']

ENTRIES = {
    'sig_fused_osc_biquad': HEAD + HP + CG + TAIL,
    'sig_fused_osc_pair_biquad': PAIR_HEAD + HP + PAIR + CG_ROWS + TAIL,
    'sig_fused_osc_biquad_rows': HEAD + HP + CG_ROWS + TAIL,
    'sig_fused_osc_biquad_fm': HEAD + HP_FM + CG_ROWS + TAIL,
    'sig_fused_osc_biquad_devpos': [('position_dev' if p == 'position' else p) for p in HEAD] + HP + CG + TAIL,
    'sig_fused_osc_biquad_mix': HEAD + HP + CG + ['matrix'] + TAIL,
    'sig_fused_voice_bus': HEAD + HP + CG + BUS + TAIL,
    'sig_fused_voice_bus_walk': HEAD + HP + CG + BUS + TAIL,
    'sig_fused_voice_bus_prepared': HEAD + HP + CG + BUS + TAIL + ['consts', 'consts_ready'],
    'sig_fused_voice_pair_bus': PAIR_HEAD + HP + PAIR + CG_ROWS + BUS + TAIL,
    'sig_fused_voice_bus_rows': HEAD + HP + CG_ROWS + BUS + TAIL,
    'sig_fused_voice_bus_fm': HEAD + HP_FM + CG_ROWS + BUS + TAIL,
    'sig_fused_voice_bus_bound': None,      # arguments in a caller-held struct, see call()
}

POINTERS = {'hertz', 'phase', 'cutoff', 'gain', 'hertz2', 'phase2', 'mix', 'hertz_hist', 'phase_hist', 'bus_gains', 'workspace',
            'out', 'status', 'stream', 'matrix', 'consts', 'position_dev'}
INT64 = {'position', 'out_ld', 'bus_gains_ld'}


class BoundCall(ctypes.Structure):          # include/signals_amd.h: sig_fused_voice_bus_call
    _fields_ = ([(n, ctypes.c_int32) for n in ('osc_kind', 'filt_type', 'rate', 'block_frames', 'nblocks', 'context', 'voices',
                                                'hertz_stride', 'phase_stride', 'cutoff_stride', 'gain_stride', 'bus_channels')] +
                [(n, ctypes.c_void_p) for n in ('hertz', 'phase', 'cutoff', 'gain', 'bus_gains')] +
                [('bus_gains_ld', ctypes.c_int64), ('out_ld', ctypes.c_int64)] +
                [(n, ctypes.c_void_p) for n in ('workspace', 'status', 'consts')])


BUFFER = (ctypes.c_double * 4096)()
PTR = ctypes.addressof(BUFFER)


def good(name):
    """a well-formed call of the entry with no blocks"""
    bus = 'bus' in name
    g = dict(osc_kind=0, osc2_kind=1, pair_op=1, filt_type=0, rate=48000, position=0, position_dev=PTR, block_frames=256,
             nblocks=0, context=100, voices=V,
             hertz=PTR, hertz_stride=1, phase=PTR, phase_stride=1, cutoff=PTR, cutoff_stride=1, gain=PTR, gain_stride=1,
             hertz2=PTR, hertz2_stride=1, phase2=PTR, phase2_stride=0, mix=PTR, mix_stride=1,
             hertz_rows=0, hertz_hist=PTR, phase_rows=1, phase_hist=None,           # hertz: one row per block (there are none) + the row in front
             cutoff_rows=1, gain_rows=1, matrix=PTR,
             bus_gains=PTR, bus_gains_ld=V, bus_channels=2, workspace=PTR,
             out=PTR, out_ld=2 if bus else V, status=None, stream=None, consts=PTR, consts_ready=0)
    return g


def call(lib, name, args):
    fn = getattr(lib, name)
    fn.restype = ctypes.c_int
    if name == 'sig_fused_voice_bus_bound':
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]
        block = BoundCall(**{f: args[f] for f, _ in BoundCall._fields_})
        return fn(ctypes.addressof(block), args['position'], args['out'], args['consts_ready'], args.get('walk', 0), args['stream'])
    params = ENTRIES[name]
    fn.argtypes = [ctypes.c_void_p if p in POINTERS else ctypes.c_int64 if p in INT64 else ctypes.c_int32 for p in params]
    return fn(*[args[p] for p in params])


def parameters(name):
    if name == 'sig_fused_voice_bus_bound':
        return {f for f, _ in BoundCall._fields_} | {'position', 'out', 'stream', 'consts_ready'}
    return set(ENTRIES[name])


def spoils(name):
    """(label, {argument: bad value}) for every class of argument the entry checks"""
    have = parameters(name)
    bus = 'bus' in name
    every = [
        ('filter type', {'filt_type': 2}),
        ('non-positive rate', {'rate': 0}),
        ('negative position', {'position': -1}),
        ('null position_dev', {'position_dev': None}),
        ('negative voices', {'voices': -1}),
        ('null hertz', {'hertz': None}),
        ('null cutoff', {'cutoff': None}),
        ('null out', {'out': None}),
        ('null workspace', {'workspace': None}),
        ('hertz stride', {'hertz_stride': 2}),
        ('phase stride', {'phase_stride': 2}),
        ('cutoff stride', {'cutoff_stride': -1}),
        ('gain stride', {'gain_stride': 2}),
        ('out_ld too small', {'out_ld': 1 if bus else V - 1}),
        ('cutoff rows', {'cutoff_rows': 3}),
        ('gain rows', {'gain_rows': 2}),
        ('pair op', {'pair_op': 3}),
        ('no pair op', {'pair_op': 0}),
        ('second kind', {'osc2_kind': 4}),
        ('null second hertz', {'hertz2': None}),
        ('second stride', {'hertz2_stride': 2}),
        ('missing mix row', {'mix': None}),
        ('FM rows without their history row', {'hertz_hist': None}),
        ('phase rows without their history row', {'phase_rows': 0}),
        ('phase history without a phase', {'phase_hist': PTR, 'phase': None}),
        ('bus_gains_ld < voices', {'bus_gains_ld': V - 1}),
        ('no gains on two channels', {'bus_gains': None}),
        ('null matrix', {'matrix': None}),
    ]
    out = [(label, bad) for label, bad in every if set(bad) <= have]
    if 'hertz_hist' in have:
        out.append(('FM with block_frames < context', {'block_frames': 50}))
    if name == 'sig_fused_osc_biquad_mix':
        out.append(('voices % 64', {'voices': 96, 'out_ld': 96}))
    if name in ('sig_fused_voice_bus_prepared', 'sig_fused_voice_bus_bound'):
        out.append(('null consts', {'consts': None}))
    return out


CASES = [(name, label, bad) for name in ENTRIES for label, bad in spoils(name)]


@pytest.fixture(scope='module')
def lib():
    from signals_amd import _native
    if not _native.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(str(_native.LIB_PATH))


def test_thirteen_entry_points():
    assert len(ENTRIES) == 13
    assert sum(label == 'filter type' for _, label, _ in CASES) == 13       # (every entry has cases)


@pytest.mark.parametrize('name', list(ENTRIES))
def test_well_formed_empty_call_returns_zero(lib, name):
    assert call(lib, name, good(name)) == 0
    if name == 'sig_fused_voice_bus_bound':
        assert call(lib, name, dict(good(name), walk=1, consts=None)) == 0     # (the walker needs no constants)


@pytest.mark.parametrize('name,label,bad', CASES, ids=[f'{n}-{l}'.replace(' ', '_') for n, l, _ in CASES])
def test_one_spoiled_argument_is_rejected(lib, name, label, bad):
    assert call(lib, name, dict(good(name), **bad)) == INV


@pytest.mark.parametrize('name', list(ENTRIES))
def test_empty_problem_returns_zero_only_after_the_checks(lib, name):
    for empty in ({'block_frames': 0}, {'voices': 0}):
        args = dict(good(name), **empty)
        if 'hertz_hist' in parameters(name) and 'block_frames' in empty:
            continue                                                           # (FM: block_frames < context is itself rejected)
        assert call(lib, name, args) == 0
        assert call(lib, name, dict(args, rate=0)) == INV


@pytest.mark.parametrize('name', list(ENTRIES))
def test_unknown_oscillator_kind_is_rejected_before_any_launch(lib, name):
    """the kind is looked at where the kernel is chosen, after the empty-problem return: one block, and nothing is launched"""
    args = dict(good(name), nblocks=1, hertz_rows=1)
    assert call(lib, name, dict(args, osc_kind=4)) == INV
    assert call(lib, name, dict(args, osc_kind=-1)) == INV
    assert call(lib, name, dict(good(name), osc_kind=4)) == 0                  # (no blocks: not looked at)


@pytest.mark.parametrize('name', ['sig_fused_voice_bus', 'sig_fused_voice_bus_rows', 'sig_fused_voice_bus_fm', 'sig_fused_voice_pair_bus'])
def test_unsupported_bus_width_is_rejected_before_any_launch(lib, name):
    args = dict(good(name), nblocks=1, hertz_rows=1, bus_channels=3, out_ld=3)
    assert call(lib, name, args) == INV
