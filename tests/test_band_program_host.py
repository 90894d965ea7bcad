"""Band filters in the voice program and the per-block band entry point, without a GPU: the Band instruction's encoding, the
specialised build's macros and image, and argument checks of sig_band_coldstart_blocks / sig_voice_program that return
hipErrorInvalidValue before any device work."""
import ctypes

import pytest

from signals_amd import _native, specialise

INV = 1     # hipErrorInvalidValue
BAND = [('Osc', 2, 0, 0, 0), ('Band', 0, 0, 0, 0)]


@pytest.fixture(scope='module')
def lib():
    if not _native.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return _native.lib()


def test_band_instruction_encoding():
    assert _native.VP_OPS['Band'] == 11                                      # SIG_VP_BAND (include/signals_amd.h)
    assert _native.voice_program_words(BAND) == [0x40, 0xb]
    assert _native.voice_program_words([('Band', 0, 2, 0, 0)]) == [0x20b]      # slots 2 and 3


def test_flags_count_two_filter_slots_and_no_extended_handlers():
    f = set(specialise.flags(BAND, 1, 0, 2, 0, 2, 2))
    assert {'-DSIG_VP_S_NF=2', '-DSIG_VP_S_EXT=0', '-DSIG_VP_STATIC_CODE={0x40,0xb}'} <= f
    assert '-DSIG_VP_S_EXT=1' in specialise.flags(BAND + [('Amp', 0, 0, 0, 0)], 1, 1, 2, 0, 2, 2)


@pytest.mark.skipif(specialise.hipcc() is None, reason='no hipcc in this environment')
def test_the_specialised_band_program_builds(tmp_path, monkeypatch):
    monkeypatch.setattr(specialise, 'CACHE', tmp_path)
    code = BAND + [('Gain', 0, 0, 0, 0)]
    image = specialise.build(code, 1, 1, 2, 0, 2, 2)
    assert b'sig_vp_specialised' in image and b'sig_vp_specialised_info' in image


def test_band_blocks_entry_point_is_exported(lib):
    assert 'sig_band_coldstart_blocks' in _native.EXPORTS
    assert ctypes.CDLL(str(_native.LIB_PATH)).sig_band_coldstart_blocks is not None


def test_band_blocks_argument_errors_do_not_reach_the_device(lib):
    f = lib.sig_band_coldstart_blocks
    p = 64                                                                     # (never dereferenced: every call fails its checks)
    args = dict(type=2, rate=48000, position=0, N=256, K=4, ctx=100, voices=8, low=p, ls=1, high=p, hs=1, blocks=4,
                x=p, in_ld=8, hist=0, y=p, out_ld=8, dtype=0, status=None, stream=None)

    def call(**over):
        a = dict(args, **over)
        return f(a['type'], a['rate'], a['position'], a['N'], a['K'], a['ctx'], a['voices'], a['low'], a['ls'], a['high'], a['hs'],
                 a['blocks'], a['x'], a['in_ld'], a['hist'], a['y'], a['out_ld'], a['dtype'], a['status'], a['stream'])
    assert call(low=None) == INV                                               # null rows
    assert call(high=None) == INV
    assert call(blocks=2) == INV                                               # neither 1 nor nblocks
    assert call(blocks=0) == INV
    assert call(ls=2) == INV                                                   # strides 0 / 1
    assert call(hs=-1) == INV
    assert call(type=0) == INV                                                 # not a band type
    assert call(position=50, hist=10) == INV                                   # too few context rows
    assert call(N=0) == 0 and call(K=0, blocks=1) == 0                         # accepted, nothing to launch


def _program(code, types, levels=None, depth=1):
    P = _native.VoiceProgramT()
    P.n_ins = len(code)
    for k, (op, kind, a, b, c) in enumerate(code):
        P.ins[k] = _native.VpIns(_native.VP_OPS[op], kind, a, b, c)
    row = ctypes.c_double(440.0)
    P.n_oscs = 1
    P.hertz[0] = _native.VpRows(ctypes.cast(ctypes.pointer(row), ctypes.c_void_p).value, 0, 1)
    P.phase[0] = _native.VpRows(None, 0, 1)
    P.n_filters = len(types)
    for k, t in enumerate(types):
        P.cutoff[k] = _native.VpRows(ctypes.cast(ctypes.pointer(row), ctypes.c_void_p).value, 0, 1)
        P.filter_type[k] = _native.FILT_TYPES[t]
        P.filter_level[k] = (levels or [1] * len(types))[k]
    P.depth = depth
    return P, row


def test_voice_program_refuses_inconsistent_band_slots(lib):
    buf = (ctypes.c_float * 64)()

    def run(code, types, levels=None, depth=1):
        P, keep = _program(code, types, levels, depth)
        return lib.sig_voice_program(ctypes.byref(P), 48000, 0, 256, 1, 100, 8, 2, 0, None, 0, None, 0, 0, None,
                                     ctypes.addressof(buf), 8, None, None)
    assert run(BAND, ['bp']) == INV                                            # slot a + 1 missing
    assert run(BAND, ['lp', 'lp']) == INV                                      # a Band over low / high pass slots
    assert run(BAND, ['bp', 'bs']) == INV                                      # two band types in one filter
    assert run(BAND, ['bp', 'bp'], levels=[1, 2], depth=2) == INV              # one node: one level
    assert run([('Osc', 2, 0, 0, 0), ('Filter', 0, 0, 0, 0)], ['bp']) == INV   # a Filter instruction on a band slot
    assert run([('Osc', 2, 0, 0, 0), ('Band', 0, 1, 0, 0)], ['bp', 'bp', 'bp']) == INV   # pairs start at a run's first slot
