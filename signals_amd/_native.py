"""ctypes binding of `signals_amd/csrc/libsignals_amd.so` (C ABI: include/signals_amd.h).

torch tensors are the buffer substrate; only their `data_ptr()`, strides and the current HIP stream
cross the boundary.  There is NO CPU fallback: a missing library or a non-GPU tensor raises.
"""
from __future__ import annotations

import ctypes
import pathlib

import torch

import os

# SIG_LIB_PATH: load another build of the same ABI (kernel tuning A/B runs only)
LIB_PATH = pathlib.Path(os.environ.get('SIG_LIB_PATH') or pathlib.Path(__file__).resolve().parent / 'csrc' / 'libsignals_amd.so')

F32, F64 = 0, 1
OSC_KINDS = {'Sine': 0, 'Square': 1, 'Sawtooth': 2, 'Triangle': 3}
FILT_TYPES = {'lp': 0, 'hp': 1, 'bp': 2, 'bs': 3, 'rlp': 4, 'rhp': 5,     # rlp / rhp: a voice program's resonant slots (SIG_FILT_RES_*)
              'eqbp': 6, 'eqnotch': 7, 'eqap': 8, 'eqpeak': 9, 'eqls': 10, 'eqhs': 11,    # SIG_FILT_EQ_*: the equaliser biquads (chain/ext.py EqFilter)
              'ladder': 12}                 # SIG_FILT_LADDER: the 4-pole ladder (chain/ext.py Ladder), run by sig_ladder_coldstart alone
EQ_GAIN_TYPES = ('eqpeak', 'eqls', 'eqhs')  # the equaliser types that read a gain
EW_OPS = {'Gain': 0, 'Mix': 1, 'RingMod': 2, 'Amp': 3}
STATUS_BAD_CUTOFF = 1
STATUS_BAD_RESONANCE = 2
STATUS_BAD_GAIN = 4
ABI_VERSION = 7
SINE_FAST_MAX_CYCLES = 2.0 ** 26     # sig_osc.h kSineFastMaxT: |t| up to which the fused Sine kernels advance the phase incrementally

ADSR_PARAMS = ('attack', 'decay', 'sustain', 'release', 'gate_on', 'gate_off')


class NativeError(RuntimeError):
    """The HIP library is missing, was given a CPU tensor, or returned a hipError_t."""


class CtlIns(ctypes.Structure):
    """sig_ctl_ins: one instruction of a block-rate control program"""
    _fields_ = [('op', ctypes.c_int32), ('kind', ctypes.c_int32), ('a', ctypes.c_int32), ('b', ctypes.c_int32), ('c', ctypes.c_int32),
                ('dst', ctypes.c_int32), ('stride', ctypes.c_int32), ('rows', ctypes.c_int32), ('cols', ctypes.c_int32),
                ('reserved', ctypes.c_int32), ('row', ctypes.c_void_p)]


class CtlOut(ctypes.Structure):
    """sig_ctl_out: a register written to a (nblocks, cols) float64 output"""
    _fields_ = [('reg', ctypes.c_int32), ('cols', ctypes.c_int32), ('out', ctypes.c_void_p), ('front', ctypes.c_void_p)]


CTL_OPS = {'Row': 0, 'Osc': 1, 'Gain': 2, 'Mix': 3, 'RingMod': 4, 'Amp': 5, 'Noise': 6, 'Filter': 7, 'AdsrArgs': 8, 'Adsr': 9}
CTL_WINDOWED_OPS = (6, 7)      # run only through sig_control_program_windowed
CTL_ENVELOPE_OPS = (8, 9)      # the ADSR pair: run only through sig_control_program_envelope (which runs the windowed ones too)
CTL_MAX_REGS, CTL_MAX_INS = 48, 48


# ---- sig_voice_program: the per-voice graph as code for the accumulator machine of voice_program.hip
VP_OPS = {'Osc': 0, 'Filter': 1, 'Gain': 2, 'Mul': 3, 'Mix': 4, 'Save': 5, 'Load': 6, 'Const': 7, 'Amp': 8, 'Adsr': 9, 'Noise': 10,
          'Band': 11, 'OscPM': 12, 'OscTable': 13, 'Shape': 14, 'FilterQ': 15, 'OscUni': 16, 'OscBlep': 17, 'FilterEq': 18, 'OscSync': 19}
VP_EXT_OPS = ('Amp', 'Adsr', 'Noise')       # the instructions of the extended handlers (the full register file, or SIG_VP_S_EXT)
VP_MAX_INS, VP_MAX_OSCS, VP_MAX_PARAMS, VP_MAX_FILTERS, VP_MAX_TEMPS, VP_MAX_HIST = 32, 4, 8, 4, 4, 3
VP_MAX_TABLES = 2
VP_TABLE_OPS = ('OscTable', 'Shape')        # the instructions of the table variant (SIG_VP_S_TAB): table slot b, select = parameter slot c | -1
VP_RES_OPS = ('FilterQ',)                   # the instruction of the resonant variant (SIG_VP_S_RES): filter slot a, q = parameter slot c | -1
VP_EQ_OPS = ('FilterEq',)                   # FilterQ on an equaliser slot (ext.py EqFilter; SIG_VP_S_RES and SIG_VP_S_EQ): gain = parameter slot b | -1 too; the same family
VP_UNI_OPS = ('OscUni',)                    # the instruction of the unison variant (SIG_VP_S_UNI): oscillator slot a, unison slot b = 0, spread = parameter slot c | -1
VP_BLEP_OPS = ('OscBlep',)                  # OscUni with the band-limited waveforms (ext.py BlepOsc; SIG_VP_S_UNI and SIG_VP_S_BLEP): the same operands, the same family
VP_SYNC_OPS = ('OscSync',)                  # OscBlep with a slave oscillator reset by the master (ext.py SyncOsc; SIG_VP_S_UNI and SIG_VP_S_SYNC): ratio = parameter slot b | -1 too; the same family
VP_MAX_UNISON = 1                           # SIG_VP_MAX_UNISON: unison slots of a voice program (one `copies` array per launch)
# the families of which a single-family interpreter variant (and sig_voice_program, _ex, _unison) has at most one; a program with two
# or more of them is a MIXED program (sig_voice_program_mixed, SIG_VP_S_MIXED)
VP_FAMILIES = {'band': ('Band',), 'pm': ('OscPM',), 'table': VP_TABLE_OPS, 'resonant': VP_RES_OPS, 'unison': VP_UNI_OPS}
VP_VARIANTS = ('plain', 'band', 'pm', 'table', 'shape', 'resonant', 'unison', 'blep', 'mixed')    # SIG_VP_FAMILY_*: the interpreter's variants (`voice_program_variant`)
UNISON_MAX_COPIES = 16                      # SIG_UNISON_MAX_COPIES: copies of a unison oscillator (ext.py UnisonOsc)
TABLE_MAX_POINTS = 16384                    # SIG_TABLE_MAX_POINTS: entries of a wavetable or a shaper table (of a voice program's tables together)
ADDITIVE_MAX_PARTIALS = 64                  # SIG_ADDITIVE_MAX_PARTIALS: rows of an additive oscillator's table (ext.py Additive): harmonics per voice
DELAY_CONTEXT = 100                         # SIG_DELAY_CONTEXT: the rows of context in front of a delay line's block, the filters' window
DELAY_MAX_FRAMES = 99                       # SIG_DELAY_MAX_FRAMES: the longest delay (ext.py Delay): the context minus the one further row the interpolation reads
DELAY_MAX_TAPS = 16                         # SIG_DELAY_MAX_TAPS: taps of a delay line
FIR_CONTEXT = 100                           # SIG_FIR_CONTEXT: the rows of context in front of a FIR filter's block, the filters' window
FIR_MAX_TAPS = 101                          # SIG_FIR_MAX_TAPS: taps of a FIR filter (ext.py FIR): x[n - 100] .. x[n], the window a filter is handed
FIR_MAX_POINTS = 4096                       # SIG_FIR_MAX_POINTS: taps x columns of a FIR filter's table
SAMPLER_MAX_POINTS = 1 << 26                # SIG_SAMPLER_MAX_POINTS: frames x recordings of a sampler's table (ext.py Sampler), resident in HBM
MODAL_MAX_MODES = 64                        # SIG_MODAL_MAX_MODES: modes of one set of a modal bank (ext.py Modal)
MODAL_MAX_POINTS = 2048                     # SIG_MODAL_MAX_POINTS: sets x modes of a modal bank's table, float64 (r, a, lambda) rows held in LDS


class VpIns(ctypes.Structure):
    _fields_ = [('op', ctypes.c_int32), ('kind', ctypes.c_int32), ('a', ctypes.c_int32), ('b', ctypes.c_int32), ('c', ctypes.c_int32)]


class VpRows(ctypes.Structure):
    _fields_ = [('ptr', ctypes.c_void_p), ('col_stride', ctypes.c_int32), ('rows', ctypes.c_int32)]


class VoiceProgramT(ctypes.Structure):
    """sig_voice_program_t (host memory)"""
    _fields_ = [('n_ins', ctypes.c_int32), ('ins', VpIns * VP_MAX_INS),
                ('n_oscs', ctypes.c_int32), ('hertz', VpRows * VP_MAX_OSCS), ('phase', VpRows * VP_MAX_OSCS),
                ('n_params', ctypes.c_int32), ('params', VpRows * VP_MAX_PARAMS),
                ('n_filters', ctypes.c_int32), ('cutoff', VpRows * VP_MAX_FILTERS), ('filter_type', ctypes.c_int32 * VP_MAX_FILTERS),
                ('filter_level', ctypes.c_int32 * VP_MAX_FILTERS),
                ('n_temps', ctypes.c_int32), ('depth', ctypes.c_int32),
                ('adsr', ctypes.c_void_p * 6), ('adsr_stride', ctypes.c_int32 * 6), ('noise_seed', ctypes.c_uint64 * 2)]


class VpTable(ctypes.Structure):
    _fields_ = [('ptr', ctypes.c_void_p), ('points', ctypes.c_int32), ('waves', ctypes.c_int32)]


class VpTablesT(ctypes.Structure):
    """sig_vp_tables_t (host memory)"""
    _fields_ = [('n_tables', ctypes.c_int32), ('table', VpTable * VP_MAX_TABLES)]


class VpUnisonT(ctypes.Structure):
    """sig_vp_unison_t (host memory): the copies of a program's OscUni words, by value"""
    _fields_ = [('copies', ctypes.c_int32), ('detune', ctypes.c_double * UNISON_MAX_COPIES), ('offset', ctypes.c_double * UNISON_MAX_COPIES)]


class Operand(ctypes.Structure):
    _fields_ = [('ptr', ctypes.c_void_p), ('row_stride', ctypes.c_int64),
                ('col_stride', ctypes.c_int32), ('dtype', ctypes.c_int32),
                ('row_div', ctypes.c_int32), ('reserved', ctypes.c_int32)]


def _argtypes() -> dict:
    """symbol -> argument types of every entry point of include/signals_amd.h"""
    cint, i32, i64, u64, vp, dp = ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p
    p32, operand = ctypes.POINTER(i32), ctypes.POINTER(Operand)
    fused = [cint, cint, i32, i64, i32, i32, i32, i32]       # kinds, rate, position, block_frames, nblocks, context, voices
    cold = [cint, i32, i64, i32, i32, i32, i32]              # type, rate, position, block_frames, nblocks, context, voices
    rows4 = [dp, i32] * 4                                    # hertz, phase, cutoff, gain: (pointer, stride) each
    params = [dp, i32, i32] * 2                              # cutoff, gain: (pointer, stride, rows) each
    env = [ctypes.POINTER(vp), p32]                          # the ADSR rows: six pointers, six strides
    window = [vp, i64, i64]                                  # input, its leading dimension, history rows
    bus = [dp, i64, i32, vp]                                 # bus gains, their leading dimension, bus channels, workspace
    out = [vp, i64, vp, vp]                                  # out, its leading dimension, status, stream
    program = [i32, i64, i32, i32, i32, i64, i64, vp, i32, vp, i32, vp]
    return {
        'sig_abi_version': [],
        'sig_osc_bank': [cint, i64, i32, i64, i32, dp, i32, dp, i32, vp, i32, i64, vp],
        'sig_osc_bank_mod': [cint, i64, i64, i32, i64, i32, i32, dp, i32, i64, dp, i32, i64, vp, i32, i64, vp],
        'sig_osc_bank_pm': [cint, i64, i64, i32, i64, i32, i32, dp, i32, i64, dp, i32, i64, dp, i32, i64,
                            vp, i32, i64, i32, vp, i32, i64, vp],
        'sig_osc_bank_table': [i64, i64, i32, i64, i32, i32, dp, i32, i64, dp, i32, i64, dp, i32, i64, vp, i32, i32, vp, i32, i64, vp],
        'sig_osc_bank_additive': [i64, i64, i32, i64, i32, i32, dp, i32, i64, dp, i32, i64, dp, i32, i64, vp, i32, i32, vp, i32, i64, vp],
        'sig_osc_bank_unison': [cint, i64, i64, i32, i64, i32, i32, dp, i32, i64, dp, i32, i64, dp, i32, i64, i32, dp, dp, vp, i32, i64, vp],
        'sig_osc_bank_blep': [cint, i64, i64, i32, i64, i32, i32, dp, i32, i64, dp, i32, i64, dp, i32, i64, i32, dp, dp, vp, i32, i64, vp],
        'sig_osc_bank_sync': [cint, i64, i64, i32, i64, i32, i32, dp, i32, i64, dp, i32, i64, dp, i32, i64, dp, i32, i64, i32, dp, dp, vp, i32, i64, vp],
        'sig_shaper_table': [i64, i32, vp, i32, i64, i32, dp, i32, i64, i32, vp, i32, i32, vp, i32, i64, vp],
        'sig_delay_taps': [i32, i64, i32, i32, i32, i32, vp, i32, i64, i32, dp, i32, i64, i32, i32, dp, dp, vp, i32, i64, vp],
        'sig_fir_taps': [i32, i64, i32, i32, i32, i32, vp, i32, i64, i32, dp, i32, i64, i32, dp, i32, i32, vp, i32, i64, vp],
        'sig_sampler_play': [i64, i64, i32, i64, i32, i32] + [dp, i32, i64] * 4 + [vp, i32, i32, i32, i32, vp, i32, i64, vp],
        'sig_modal_bank': [i64, i64, i32, i64, i32, i32] + [dp, i32, i64] * 4 + [dp, i32, i32, vp, i32, i64, vp],
        'sig_biquad_coldstart': cold + [dp, i32, i32] + window + [vp, i64, i32, vp, vp],
        'sig_biquad_coldstart_q': cold + [dp, i32, i32] + [dp, i32, i32] + window + [vp, i64, i32, vp, vp],
        'sig_biquad_coldstart_eq': cold + [dp, i32, i32] * 3 + window + [vp, i64, i32, vp, vp],
        'sig_ladder_coldstart': cold[1:] + [dp, i32, i32] * 3 + [i32] + window + [vp, i64, i32, vp, vp],
        'sig_biquad_coldstart_env': cold + [dp, i32, i32] + env + window + out,
        'sig_biquad_coldstart_bus': cold + [dp, i32, i32] + env + window + bus + out,
        'sig_band_coldstart': cold + [dp, i32, dp, i32] + window + [vp, i64, i32, vp, vp],
        'sig_band_coldstart_blocks': cold + [dp, i32, dp, i32, i32] + window + [vp, i64, i32, vp, vp],
        'sig_elementwise': [cint, i64, i32, operand, operand, operand, vp, i64, i32, vp],
        'sig_sum_bus': [i64, i32, vp, i64, i32, dp, i64, i32, vp, i64, i32, vp],
        'sig_white_noise': [u64, i64, i64, i32, vp, i32, i64, vp],
        'sig_adsr': [i64, i32, i64, i32] + env + [vp, i32, i64, vp],
        'sig_adsr_apply': [i64, i32, i64, i32] + env + [vp, i64, vp, i64, vp],
        'sig_mix_matrix': [i64, i32, vp, i64, vp, vp, i64, vp],
        'sig_advance_position': [vp, i64, vp],
        'sig_fused_osc_biquad': fused + rows4 + out,
        'sig_fused_osc_biquad_devpos': [cint, cint, i32, vp, i32, i32, i32, i32] + rows4 + out,
        'sig_fused_osc_biquad_mix': fused + rows4 + [vp] + out,
        'sig_fused_osc_biquad_rows': fused + [dp, i32] * 2 + params + out,
        'sig_fused_osc_biquad_fm': fused + [dp, i32, i32, dp] * 2 + params + out,
        'sig_fused_osc_pair_biquad': [cint, cint] + fused + [dp, i32] * 5 + params + out,
        'sig_fused_voice_bus': fused + rows4 + bus + out,
        'sig_fused_voice_bus_walk': fused + rows4 + bus + out,
        'sig_fused_voice_bus_prepared': fused + rows4 + bus + out + [vp, i32],
        'sig_fused_voice_bus_bound': [vp, i64, vp, i32, i32, vp],
        'sig_fused_voice_bus_rows': fused + [dp, i32] * 2 + params + bus + out,
        'sig_fused_voice_bus_fm': fused + [dp, i32, i32, dp] * 2 + params + bus + out,
        'sig_fused_voice_pair_bus': [cint, cint] + fused + [dp, i32] * 5 + params + bus + out,
        'sig_fused_voice_bus_workspace': [i32, i64, i32],
        'sig_fused_voice_consts_size': [i32],
        'sig_fused_voice_bus_plan': [cint, i64, i32, i32, i32, i32, p32, p32, p32],
        'sig_fused_geometry': [i32, i32, i32, i32, p32, p32],
        'sig_fused_set_tuning': [i32, i32, i32, i32],
        'sig_fused_cascade_bus': [cint, cint, cint, i32, i64, i64, i32, i32, i32, i32] + [dp, i32] * 5 + env + bus + out,
        'sig_fused_cascade_geometry': [i32, i32, p32, p32],
        'sig_fused_cascade_set_tuning': [i32, i32],
        'sig_latency_voice_bus': [cint, i32, i64, vp, i32, i32, i32] + rows4 + bus + out,
        'sig_latency_voice_bus_workspace': [i32, i32, i32],
        'sig_control_program': program,
        'sig_control_program_windowed': program,
        'sig_control_program_envelope': program,
        'sig_control_program_attach': [p32, i32, ctypes.c_char_p, p32],
        'sig_control_program_attached': [i32] + program,
        'sig_voice_program': [ctypes.POINTER(VoiceProgramT), i32, i64, i32, i32, i32, i32, i32, i32, ctypes.POINTER(i64), i32] + bus + out,
        'sig_voice_program_ex': [ctypes.POINTER(VoiceProgramT), i32, i64, i32, i32, i32, i32, i32, i32, ctypes.POINTER(i64), i32] + bus + out
                                + [ctypes.POINTER(VpTablesT)],
        'sig_voice_program_unison': [ctypes.POINTER(VoiceProgramT), i32, i64, i32, i32, i32, i32, i32, i32, ctypes.POINTER(i64), i32] + bus + out
                                    + [ctypes.POINTER(VpTablesT), ctypes.POINTER(VpUnisonT)],
        'sig_voice_program_mixed': [ctypes.POINTER(VoiceProgramT), i32, i64, i32, i32, i32, i32, i32, i32, ctypes.POINTER(i64), i32] + bus + out
                                   + [ctypes.POINTER(VpTablesT), ctypes.POINTER(VpUnisonT)],
        'sig_voice_program_set_tuning': [i32, i32],
        'sig_voice_program_geometry': [i32, i32, i32, i32, i32, i32, i32, i32, p32, p32],
        'sig_voice_program_variant': [ctypes.POINTER(VoiceProgramT), p32, p32],
        'sig_voice_program_args_size': [],
        'sig_voice_program_attach': [ctypes.POINTER(VoiceProgramT), i32, i32, ctypes.c_char_p],
        'sig_voice_program_detach_all': [],
        'sig_voice_program_use_attached': [i32],
    }


_ARGTYPES = _argtypes()
_RETURNS_INT64 = ('sig_fused_voice_bus_workspace', 'sig_fused_voice_consts_size', 'sig_latency_voice_bus_workspace',
                  'sig_voice_program_args_size')                 # sizes in bytes; every other entry point returns an int (a hipError_t)
EXPORTS = tuple(_ARGTYPES)

_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise NativeError(f'{LIB_PATH} not built: run `python -c "import __graft_entry__ as g; g.build()"` '
                              f'(signals_amd/csrc/build.sh).  There is no CPU fallback.')
        L = ctypes.CDLL(str(LIB_PATH))
        for name, argtypes in _ARGTYPES.items():
            entry = getattr(L, name)
            entry.restype = ctypes.c_int64 if name in _RETURNS_INT64 else ctypes.c_int
            entry.argtypes = argtypes
        if L.sig_abi_version() != ABI_VERSION:
            raise NativeError('libsignals_amd.so ABI version mismatch')
        _lib = L
    return _lib


def _check(err: int, what: str) -> None:
    if err != 0:
        raise NativeError(f'{what} failed: hipError_t {err}')


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.float64:
        return F64
    raise NativeError(f'unsupported buffer dtype {t.dtype}')


def _gpu(*tensors: torch.Tensor) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise NativeError('HIP kernels need tensors resident on an MI355X (got a CPU tensor); no CPU fallback')


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def _stream(t: torch.Tensor) -> int:
    """the hipStream_t torch currently launches on for `t`'s device"""
    if _raw_stream is not None:
        return _raw_stream(t.device.index)              # the same handle as below, without building a Stream object
    return torch.cuda.current_stream(t.device).cuda_stream


def current_stream_handle(device_index: int) -> int:
    """the raw hipStream_t torch currently launches on"""
    if _raw_stream is not None:
        return _raw_stream(device_index)
    return torch.cuda.current_stream(device_index).cuda_stream


def _ctrl_row(t: torch.Tensor | None, what: str):
    """(ptr, stride) of an f64 control row shaped (1,V) or (1,1)."""
    if t is None:
        return None, 0
    if t.dtype != torch.float64 or t.dim() != 2 or t.shape[0] != 1 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise NativeError(f'{what}: control rows are contiguous float64 (1,V) or (1,1), got {tuple(t.shape)} {t.dtype}')
    return t.data_ptr(), (0 if t.shape[1] == 1 else 1)


def _audio(t: torch.Tensor, what: str) -> None:
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise NativeError(f'{what}: audio buffers are 2-D with contiguous channels, got strides {t.stride()}')


def _ctrl_rows(t: torch.Tensor | None, what: str):
    """(ptr, col_stride, row_stride, rows) of f64 control rows shaped (R, V) or (R, 1)"""
    if t is None:
        return None, 0, 0, 1
    if t.dtype != torch.float64 or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise NativeError(f'{what}: control rows are float64 (R,V) or (R,1) with contiguous channels, got '
                          f'{tuple(t.shape)} {t.dtype}')
    return t.data_ptr(), (0 if t.shape[1] == 1 else 1), (0 if t.shape[0] == 1 else t.stride(0)), t.shape[0]


def _ptr(t: torch.Tensor | None):
    """the data pointer of an optional tensor"""
    return None if t is None else t.data_ptr()


def _voice_rows(voices: int, *pairs, form=_ctrl_row) -> list:
    """the flat (ptr, stride, ...) list of per-voice control rows given as (tensor | None, name) pairs, each one column or
    `voices` wide; `form`: `_ctrl_row`, or `_ctrl_rows` for (ptr, col_stride, row_stride, rows) each"""
    flat = []
    for row, name in pairs:
        if row is not None and row.shape[1] not in (1, voices):
            raise NativeError(f'{name} has {row.shape[1]} channels for {voices} voices')
        flat.extend(form(row, name))
    return flat


def _bus_gains(gains: torch.Tensor | None, bus: int, voices: int):
    """(ptr, leading dimension) of the (C, V) bus gains"""
    if gains is None:
        if bus != 1:
            raise NativeError('a bus without gains is mono')
        return None, 0
    if gains.dtype != torch.float64 or gains.shape != (bus, voices) or gains.stride(1) != 1:
        raise NativeError(f'bus gains must be float64 ({bus},{voices}), got {tuple(gains.shape)} {gains.dtype}')
    return gains.data_ptr(), gains.stride(0)


def _envelope(rows: dict | None, voices: int, into: tuple | None = None):
    """(pointers, strides) of the six ADSR control rows (name -> (1,V)|(1,1) f64), or (None, None) without an envelope;
    `into`: the two arrays of six to fill instead of new ones"""
    if rows is None:
        return None, None
    ptrs, strides = into or ((ctypes.c_void_p * 6)(), (ctypes.c_int32 * 6)())
    flat = _voice_rows(voices, *((rows[name], name) for name in ADSR_PARAMS))
    for i in range(6):
        ptrs[i], strides[i] = flat[2 * i], flat[2 * i + 1]
    return ptrs, strides


def _bus_workspace(workspace: torch.Tensor | None, voices: int, rows: int, bus: int, device=None) -> torch.Tensor:
    """the float64 scratch of the fused bus kernels: `workspace` where it is large enough, else a new one on `device`
    (without a device: an error -- a bound call keeps the caller's)"""
    need = lib().sig_fused_voice_bus_workspace(voices, rows, bus)
    fits = workspace is not None and workspace.numel() * workspace.element_size() >= need
    if device is None and not (fits and workspace.dtype == torch.float64):
        raise NativeError('fused bus workspace too small')
    return workspace if fits else torch.empty(need // 8, dtype=torch.float64, device=device)


def _history_input(buf: torch.Tensor, history: int, voices: int, out: torch.Tensor, block_frames: int, nblocks: int, what: str) -> int:
    """the pointer to row `history` of a cold-start filter's input, `voices` wide: `history` context rows, then one row per
    row of `out`"""
    rows = out.shape[0]
    if rows != block_frames * nblocks or buf.shape[0] != history + rows or buf.shape[1] != voices or buf.dtype != out.dtype:
        raise NativeError(f'{what} shapes: in {tuple(buf.shape)} {buf.dtype} history {history} out {tuple(out.shape)} {out.dtype} '
                          f'blocks {nblocks}x{block_frames}')
    return buf.data_ptr() + history * buf.stride(0) * buf.element_size()


def _coldstart_launch(what: str, rate: int, position: int, block_frames: int, nblocks: int, context: int, buf: torch.Tensor, history: int,
                      out: torch.Tensor, status: torch.Tensor | None, *also, per_voice: torch.Tensor | None = None,
                      f32_only: bool = False):
    """what every cold-start filter launch marshals the same way, from `buf` (`history` context rows, then the input rows) and `out`:
    (voices, head, window, dst, tail) -- head = (rate, position, block_frames, nblocks, context, voices) behind the entry's filter type,
    window = (in, in_ld, in_history), dst = (out, out_ld) in front of the entries' buffer dtype, tail = (status, stream).
    `also`: further tensors that must be on the GPU; `per_voice`: the buffer with one column per voice where that is not `out`;
    `f32_only`: refuse another `out`"""
    _gpu(buf, out, status, *also)
    _audio(buf, f'{what} in')
    _audio(out, f'{what} out')
    voices = (out if per_voice is None else per_voice).shape[1]
    if f32_only and out.dtype != torch.float32:
        raise NativeError(f'{what} out must be float32, got {out.dtype}')
    in_ptr = _history_input(buf, history, voices, out, block_frames, nblocks, what)
    return (voices, (rate, position, block_frames, nblocks, context, voices), (in_ptr, buf.stride(0), history),
            (out.data_ptr(), out.stride(0)), (_ptr(status), _stream(out)))


def _parameter_rows(rows: int, rows_per_param: int, *counts) -> int:
    """`rows_per_param` as the oscillator launches take it (0: one parameter row for all), checked against the (rows, name) of
    every parameter"""
    if max(n for n, _ in counts) == 1:
        return 0
    if rows_per_param < 1:
        raise NativeError('per-block oscillator parameters need rows_per_param')
    need = (rows + rows_per_param - 1) // rows_per_param
    for n, name in counts:
        if n not in (1, need):
            raise NativeError(f'{name} has {n} parameter rows, launch needs 1 or {need}')
    return rows_per_param


def _osc_launch(out: torch.Tensor, position: int, step: int, rate: int, rows_per_param: int, *named, also=()):
    """what every oscillator launch marshals the same way, from `out` and the (tensor | None, name) parameter rows, each (1|P, V|1) f64:
    (head, rows, tail) -- head = (position, step, rate, rows, voices, rows_per_param) as the entries take them, rows = one
    [ptr, stride, row_stride] per parameter, tail = (out, dtype, ld, stream); `also`: further tensors that must be on the GPU"""
    _gpu(*(t for t, _ in named), *also, out)
    _audio(out, 'osc out')
    rows, voices = out.shape
    flat = _voice_rows(voices, *named, form=_ctrl_rows)
    rows_per_param = _parameter_rows(rows, rows_per_param, *((flat[4 * i + 3], name) for i, (_, name) in enumerate(named)))
    return ((position, step, rate, rows, voices, rows_per_param), [flat[4 * i:4 * i + 3] for i in range(len(named))],
            (out.data_ptr(), _dt(out), out.stride(0), _stream(out)))


def osc_bank(kind: str, position: int, rate: int, hertz: torch.Tensor, phase: torch.Tensor | None,
             out: torch.Tensor, step: int = 1, rows_per_param: int = 0) -> torch.Tensor:
    """out[(rows, voices)] <- oscillator `kind`; row r is absolute frame `position + r*step`.
    hertz/phase: (1|P, V|1) f64; with P > 1 parameter rows, output row r uses row r // rows_per_param."""
    head, ((hp, hs, hrs), (pp, ps, prs)), tail = _osc_launch(out, position, step, rate, rows_per_param, (hertz, 'hertz'), (phase, 'phase'))
    if step == 1 and head[5] == 0:                      # one parameter row, consecutive frames
        _check(lib().sig_osc_bank(OSC_KINDS[kind], position, rate, *head[3:5], hp, hs, pp, ps, *tail), 'sig_osc_bank')
        return out
    _check(lib().sig_osc_bank_mod(OSC_KINDS[kind], *head, hp, hs, hrs, pp, ps, prs, *tail), 'sig_osc_bank_mod')
    return out


def osc_bank_pm(kind: str, position: int, rate: int, hertz: torch.Tensor, phase: torch.Tensor | None,
                index: torch.Tensor | None, mod: torch.Tensor | None, out: torch.Tensor, step: int = 1,
                rows_per_param: int = 0) -> torch.Tensor:
    """out[(rows, voices)] <- phase-modulation oscillator `kind` (sig_osc_bank_pm): t = (n / rate * hertz + phase) + index * mod.
    hertz / phase / index: (1|P, V|1) f64 like `osc_bank`; mod: float32 | float64 (rows|1, V|1), row n modulates output row n."""
    head, (h, p, i), tail = _osc_launch(out, position, step, rate, rows_per_param, (hertz, 'hertz'), (phase, 'phase'), (index, 'index'),
                                        also=(mod,))
    rows, voices = out.shape
    mp, mdt, mld, mcs = None, F32, 0, 0
    if mod is not None:
        _audio(mod, 'modulator')
        if mod.shape[0] not in (1, rows) or mod.shape[1] not in (1, voices):
            raise NativeError(f'modulator {tuple(mod.shape)} does not broadcast to {(rows, voices)}')
        mp, mdt = mod.data_ptr(), _dt(mod)
        mld, mcs = (0 if mod.shape[0] == 1 else mod.stride(0)), (0 if mod.shape[1] == 1 else 1)
    _check(lib().sig_osc_bank_pm(OSC_KINDS[kind], *head, *h, *p, *i, mp, mdt, mld, mcs, *tail), 'sig_osc_bank_pm')
    return out


def _device_table(table: torch.Tensor, dtype, what: str, axes: str, fits, limits: str) -> tuple:
    """(ptr, rows, columns) of a table a kernel reads: a contiguous 2-D device tensor of `dtype` with `fits(rows, columns)`; `what` and
    `axes` name it in the first refusal, `limits` (a format of shape, rows, cols) is the second"""
    if table is None or table.dtype != dtype or table.dim() != 2 or not table.is_contiguous():
        raise NativeError(f'{what} is a contiguous {str(dtype).split(".")[-1]} ({axes}) tensor')
    rows, cols = table.shape
    if not fits(rows, cols):
        raise NativeError(limits.format(shape=tuple(table.shape), rows=rows, cols=cols))
    return table.data_ptr(), rows, cols


def _table(table: torch.Tensor, pow2: bool = True):
    """(ptr, points, waves) of a wavetable: float32 (T, W) contiguous on the device, T a power of two >= 2, T * W within the cap;
    `pow2` False: a shaper's table, any T >= 2"""
    return _device_table(table, torch.float32, 'a wavetable', 'points, waves',
                         lambda T, W: T >= 2 and not (pow2 and T & (T - 1)) and W >= 1 and T * W <= TABLE_MAX_POINTS,
                         f'table {{shape}}: points {"a power of two " if pow2 else ""}>= 2, points * waves <= {TABLE_MAX_POINTS}')


def osc_bank_table(position: int, rate: int, hertz: torch.Tensor, phase: torch.Tensor | None, select: torch.Tensor | None,
                   table: torch.Tensor, out: torch.Tensor, step: int = 1, rows_per_param: int = 0) -> torch.Tensor:
    """out[(rows, voices)] <- wavetable oscillator (sig_osc_bank_table): the (T, W) float32 `table` read with linear interpolation at
    np.mod(n / rate * hertz + phase, 1) * T, column clip(floor(select), 0, W - 1).  hertz / phase / select: (1|P, V|1) f64 like `osc_bank`."""
    head, (h, p, s), tail = _osc_launch(out, position, step, rate, rows_per_param, (hertz, 'hertz'), (phase, 'phase'), (select, 'select'),
                                        also=(table,))
    _check(lib().sig_osc_bank_table(*head, *h, *p, *s, *_table(table), *tail), 'sig_osc_bank_table')
    return out


def _spectra(table: torch.Tensor):
    """(ptr, partials, waves) of an additive oscillator's amplitudes: float32 (H, W) contiguous on the device, 1 <= H <=
    ADDITIVE_MAX_PARTIALS, H * W within the cap"""
    return _device_table(table, torch.float32, 'a table of partial amplitudes', 'partials, waves',
                         lambda H, W: 1 <= H <= ADDITIVE_MAX_PARTIALS and W >= 1 and H * W <= TABLE_MAX_POINTS,
                         f'table {{shape}}: 1 <= partials <= {ADDITIVE_MAX_PARTIALS}, partials * waves <= {TABLE_MAX_POINTS}')


def osc_bank_additive(position: int, rate: int, hertz: torch.Tensor, phase: torch.Tensor | None, select: torch.Tensor | None,
                      table: torch.Tensor, out: torch.Tensor, step: int = 1, rows_per_param: int = 0) -> torch.Tensor:
    """out[(rows, voices)] <- additive oscillator (sig_osc_bank_additive): the sum of the harmonics h = 1 .. k of the phase
    np.mod(n / rate * hertz + phase, 1) with the amplitudes of column clip(floor(select), 0, W - 1) of the (H, W) float32 `table`, k the
    partials below half the rate per voice and parameter row.  hertz / phase / select: (1|P, V|1) f64 like `osc_bank`."""
    head, (h, p, s), tail = _osc_launch(out, position, step, rate, rows_per_param, (hertz, 'hertz'), (phase, 'phase'), (select, 'select'),
                                        also=(table,))
    _check(lib().sig_osc_bank_additive(*head, *h, *p, *s, *_spectra(table), *tail), 'sig_osc_bank_additive')
    return out


def _pairs_by_value(pairs, cap: int, what: str, columns: str) -> tuple:
    """(U, first column, second column) of a host (U, 2) array, 1 <= U <= cap, every value finite: two arrays of U doubles a launch
    takes by value"""
    import numpy as np
    c = np.asarray(pairs, dtype=np.float64)
    if c.ndim != 2 or c.shape[1] != 2 or not 1 <= c.shape[0] <= cap or not np.isfinite(c).all():
        raise NativeError(f'{what} must be a finite (1..{cap}, 2) array of {columns} rows, got shape {c.shape}')
    U = c.shape[0]
    return U, (ctypes.c_double * U)(*c[:, 0].tolist()), (ctypes.c_double * U)(*c[:, 1].tolist())


def _copies(copies) -> tuple:
    """(U, detune, offsets) of a unison oscillator's (U, 2) `copies` array"""
    return _pairs_by_value(copies, UNISON_MAX_COPIES, 'unison copies', '(detune, phase offset)')


def _osc_bank_copies(entry: str, kind: str, position: int, rate: int, copies, out, step: int, rows_per_param: int, *named):
    """the one call of sig_osc_bank_unison, sig_osc_bank_blep and sig_osc_bank_sync: the parameter rows, then the copies"""
    head, rows, tail = _osc_launch(out, position, step, rate, rows_per_param, *named)
    _check(getattr(lib(), entry)(OSC_KINDS[kind], *head, *(x for row in rows for x in row), *_copies(copies), *tail), entry)
    return out


def osc_bank_unison(kind: str, position: int, rate: int, hertz: torch.Tensor, phase: torch.Tensor | None, spread: torch.Tensor | None,
                    copies, out: torch.Tensor, step: int = 1, rows_per_param: int = 0) -> torch.Tensor:
    """out[(rows, voices)] <- unison oscillator `kind` (sig_osc_bank_unison): the mean over the U rows (d, p) of `copies` (a host
    (U, 2) array, by value) of wave(n / rate * (hertz * (1 + spread * d)) + (phase + p)).  hertz / phase / spread: (1|P, V|1) f64 like
    `osc_bank`; spread None: unplugged = 0."""
    return _osc_bank_copies('sig_osc_bank_unison', kind, position, rate, copies, out, step, rows_per_param,
                            (hertz, 'hertz'), (phase, 'phase'), (spread, 'spread'))


def osc_bank_blep(kind: str, position: int, rate: int, hertz: torch.Tensor, phase: torch.Tensor | None, spread: torch.Tensor | None,
                  copies, out: torch.Tensor, step: int = 1, rows_per_param: int = 0) -> torch.Tensor:
    """out[(rows, voices)] <- band-limited oscillator `kind` ('Square' | 'Sawtooth' | 'Triangle'; sig_osc_bank_blep): `osc_bank_unison`
    with each copy's waveform corrected by a two-sample polynomial step around its edges (ext.py BlepOsc), the window d =
    min(|hertz * (1 + spread * d_u)| / rate, 0.5) per copy.  Same arguments."""
    return _osc_bank_copies('sig_osc_bank_blep', kind, position, rate, copies, out, step, rows_per_param,
                            (hertz, 'hertz'), (phase, 'phase'), (spread, 'spread'))


def osc_bank_sync(kind: str, position: int, rate: int, hertz: torch.Tensor, phase: torch.Tensor | None, spread: torch.Tensor | None,
                  ratio: torch.Tensor | None, copies, out: torch.Tensor, step: int = 1, rows_per_param: int = 0) -> torch.Tensor:
    """out[(rows, voices)] <- hard-sync oscillator `kind` ('Sawtooth' | 'Square'; sig_osc_bank_sync): `osc_bank_blep` with a slave
    oscillator at max(ratio, 1) times the pitch, reset at every cycle of the master (ext.py SyncOsc).  ratio: (1|P, V|1) f64 like
    spread; None: unplugged = 0, the band-limited oscillator."""
    return _osc_bank_copies('sig_osc_bank_sync', kind, position, rate, copies, out, step, rows_per_param,
                            (hertz, 'hertz'), (phase, 'phase'), (spread, 'spread'), (ratio, 'ratio'))


def shaper_table(x: torch.Tensor, select: torch.Tensor | None, table: torch.Tensor, out: torch.Tensor,
                 rows_per_select: int = 0) -> torch.Tensor:
    """out[(rows, voices)] <- waveshaper (sig_shaper_table): the (T, W) float32 `table` of transfer curves over -1 .. +1 read with linear
    interpolation at (clip(x, -1, 1) + 1) * (T - 1) / 2, column clip(floor(select), 0, W - 1).  x: float32 | float64 (rows|1, V|1);
    select: (1|P, V|1) f64, output row r reads row r // rows_per_select."""
    _gpu(x, select, table, out)
    _audio(out, 'shaper out')
    _audio(x, 'shaper in')
    rows, voices = out.shape
    if x.shape[0] not in (1, rows) or x.shape[1] not in (1, voices):
        raise NativeError(f'shaper input {tuple(x.shape)} does not broadcast to {(rows, voices)}')
    sp, ss, srs, srows = _voice_rows(voices, (select, 'select'), form=_ctrl_rows)
    rows_per_select = _parameter_rows(rows, rows_per_select, (srows, 'select'))
    _check(lib().sig_shaper_table(rows, voices, x.data_ptr(), _dt(x), 0 if x.shape[0] == 1 else x.stride(0), 0 if x.shape[1] == 1 else 1,
                                  sp, ss, srs, rows_per_select, *_table(table, pow2=False),
                                  out.data_ptr(), _dt(out), out.stride(0), _stream(out)), 'sig_shaper_table')
    return out


def _taps(taps) -> tuple:
    """(U, multipliers, gains) of a delay line's (U, 2) `taps` array"""
    return _pairs_by_value(taps, DELAY_MAX_TAPS, 'delay taps', '(multiplier, gain)')


def _window_launch(what: str, rate: int, position: int, block_frames: int, nblocks: int, window: torch.Tensor, history: int,
                   control: torch.Tensor | None, name: str, out: torch.Tensor, also=()):
    """what the window nodes' launches (sig_delay_taps, sig_fir_taps) marshal the same way, from `window` (`history` = min(100,
    position) context rows, then one input row per row of `out`, float32 | float64 (rows, V | 1)) and the per-block control row
    `control` (f64 (1 | nblocks, V | 1), None: unplugged), called `name`: (head, tail) -- head = every argument up to the control row's
    block count, tail = (out, dtype, ld, stream); the entry's own operands go between.  `also`: further tensors that must be on the GPU"""
    _gpu(window, control, *also, out)
    _audio(window, f'{what} in')
    _audio(out, f'{what} out')
    rows, voices = out.shape
    if rows != block_frames * nblocks or window.shape[0] != history + rows or window.shape[1] not in (1, voices):
        raise NativeError(f'{what} shapes: in {tuple(window.shape)} history {history} out {tuple(out.shape)} blocks {nblocks}x{block_frames}')
    ptr, stride, row_stride, blocks = _voice_rows(voices, (control, name), form=_ctrl_rows)
    if blocks not in (1, nblocks):
        raise NativeError(f'{name} has {blocks} rows, launch needs 1 or {nblocks}')
    return ((rate, position, block_frames, nblocks, history, voices,
             window.data_ptr(), _dt(window), window.stride(0), 0 if window.shape[1] == 1 else 1, ptr, stride, row_stride, blocks),
            (out.data_ptr(), _dt(out), out.stride(0), _stream(out)))


def delay_taps(rate: int, position: int, block_frames: int, nblocks: int, window: torch.Tensor, history: int,
               time: torch.Tensor | None, taps, out: torch.Tensor) -> torch.Tensor:
    """out[(nblocks * block_frames, voices)] <- short multi-tap delay line (sig_delay_taps; ext.py Delay): `window` holds `history` =
    min(100, position) context rows, then one input row per row of `out`, float32 | float64 (rows, V | 1); row n of block b is
    sum_u g_u * (x[n - i_u] + f_u * (x[n - i_u - 1] - x[n - i_u])) with d_u = clip(time[b] * rate * m_u, 0, 99) = i_u + f_u, x = 0
    in front of absolute frame 0.  time: f64 (1 | nblocks, V | 1) seconds, None: unplugged = 0; taps: a host (U, 2) array of
    (m_u, g_u) rows, by value."""
    head, tail = _window_launch('delay', rate, position, block_frames, nblocks, window, history, time, 'time', out)
    _check(lib().sig_delay_taps(*head, *_taps(taps), *tail), 'sig_delay_taps')
    return out


def _fir_table(table: torch.Tensor):
    """(ptr, taps, columns) of a FIR filter's table: float64 (L, W) contiguous on the device, 1 <= L <= 101, W >= 1, L * W within the cap"""
    return _device_table(table, torch.float64, 'a FIR table', 'taps, columns',
                         lambda L, W: 1 <= L <= FIR_MAX_TAPS and W >= 1 and L * W <= FIR_MAX_POINTS,
                         f'FIR table {{shape}}: 1 <= taps <= {FIR_MAX_TAPS}, columns >= 1, taps * columns <= {FIR_MAX_POINTS}')


def fir_taps(rate: int, position: int, block_frames: int, nblocks: int, window: torch.Tensor, history: int,
             select: torch.Tensor | None, table: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out[(nblocks * block_frames, voices)] <- dense FIR filter (sig_fir_taps; ext.py FIR): `window` holds `history` =
    min(100, position) context rows, then one input row per row of `out`, float32 | float64 (rows, V | 1); row n of block b is
    h[0, w] * x[n] + h[1, w] * x[n - 1] + ... + h[L - 1, w] * x[n - L + 1], summed in ascending k, with w = clip(floor(select[b]), 0,
    W - 1) and x = 0 in front of absolute frame 0.  select: f64 (1 | nblocks, V | 1), None: unplugged = column 0; table: the (L, W)
    float64 taps on the device."""
    head, tail = _window_launch('fir', rate, position, block_frames, nblocks, window, history, select, 'select', out, also=(table,))
    _check(lib().sig_fir_taps(*head, *_fir_table(table), *tail), 'sig_fir_taps')
    return out


def sampler_play(position: int, rate: int, ratio: torch.Tensor | None, offset: torch.Tensor | None, gate_on: torch.Tensor | None,
                 select: torch.Tensor | None, table: torch.Tensor, loop_start: int, loop_end: int, out: torch.Tensor,
                 step: int = 1, rows_per_param: int = 0) -> torch.Tensor:
    """out[(rows, voices)] <- sample playback (sig_sampler_play; ext.py Sampler): row r is absolute frame n = position + r * step, read
    at u = ((n / rate - gate_on) * rate) * ratio + offset with linear interpolation, silence before the trigger and outside the
    recording, the loop [loop_start, loop_end) wrapped when loop_end != 0.  `table`: the device copy, float32 (W, T) contiguous -- W
    recordings of T frames, each contiguous (the transpose of the node's state).  ratio / offset / gate_on / select: (1|P, V|1) f64
    like `osc_bank`, None: unplugged = 0."""
    named = ((ratio, 'ratio'), (offset, 'offset'), (gate_on, 'gate_on'), (select, 'select'))
    ptr, waves, frames = _device_table(table, torch.float32, 'a sampler table', 'recordings, frames',
                                       lambda W, T: T >= 2 and W >= 1 and T * W <= SAMPLER_MAX_POINTS,
                                       f'sampler table of {{cols}} frames x {{rows}} recordings: frames >= 2, frames * recordings <= {SAMPLER_MAX_POINTS}')
    head, rows, tail = _osc_launch(out, position, step, rate, rows_per_param, *named, also=(table,))
    _check(lib().sig_sampler_play(*head, *(x for row in rows for x in row), ptr, frames, waves, loop_start, loop_end, *tail),
           'sig_sampler_play')
    return out


def _modes(modes: torch.Tensor):
    """(ptr, sets, count) of a modal bank's table: float64 (W, M, 3) contiguous on the device, rows (ratio, amplitude, decay rate),
    1 <= M <= MODAL_MAX_MODES, W * M within the cap (`_device_table`'s two refusals for a table of three axes)"""
    if modes is None or modes.dtype != torch.float64 or modes.dim() != 3 or modes.shape[2] != 3 or not modes.is_contiguous():
        raise NativeError('a table of modes is a contiguous float64 (sets, modes, 3) tensor')
    sets, count = modes.shape[:2]
    if not (1 <= count <= MODAL_MAX_MODES and sets >= 1 and sets * count <= MODAL_MAX_POINTS):
        raise NativeError(f'modes {tuple(modes.shape)}: 1 <= modes <= {MODAL_MAX_MODES}, sets * modes <= {MODAL_MAX_POINTS}')
    return modes.data_ptr(), sets, count


def modal_bank(position: int, rate: int, hertz: torch.Tensor, gate_on: torch.Tensor | None, damp: torch.Tensor | None,
               select: torch.Tensor | None, modes: torch.Tensor, out: torch.Tensor, step: int = 1, rows_per_param: int = 0) -> torch.Tensor:
    """out[(rows, voices)] <- modal resonator bank (sig_modal_bank; ext.py Modal): row r is absolute frame n = position + r * step, the
    sum over the modes (r_i, a_i, lambda_i) of set clip(floor(select), 0, W - 1) of a_i g_i exp(-(lambda_i + damp) e) sin(2 pi e
    hertz r_i) at e = n / rate - gate_on, silence before the strike, g_i the fade below half the rate.  `modes`: the device copy, float64
    (W, M, 3).  hertz / gate_on / damp / select: (1|P, V|1) f64 like `osc_bank`, None: unplugged = 0."""
    named = ((hertz, 'hertz'), (gate_on, 'gate_on'), (damp, 'damp'), (select, 'select'))
    head, rows, tail = _osc_launch(out, position, step, rate, rows_per_param, *named, also=(modes,))
    _check(lib().sig_modal_bank(*head, *(x for row in rows for x in row), *_modes(modes), *tail), 'sig_modal_bank')
    return out


def biquad_coldstart(btype: str, rate: int, position: int, block_frames: int, nblocks: int, context: int,
                     cutoff: torch.Tensor, buf: torch.Tensor, history: int, out: torch.Tensor,
                     status: torch.Tensor | None = None, envelope: dict | None = None) -> torch.Tensor:
    """`buf` holds `history` context rows followed by nblocks*block_frames input rows;
    `out` (nblocks*block_frames, voices) receives the filtered blocks.
    cutoff: f64 (1|nblocks, V|1).  `envelope`: ADSR control rows (name -> (1,V)|(1,1) f64); the stored rows
    are then multiplied by the envelope (float32 buffers only)."""
    voices, head, window, dst, tail = _coldstart_launch('biquad', rate, position, block_frames, nblocks, context, buf, history, out, status,
                                                cutoff, *(envelope or {}).values())
    rows = _block_rows(cutoff, 'cutoff', nblocks, voices)                      # (checked before the type is looked up)
    head = (FILT_TYPES[btype], *head, *rows)
    if envelope is not None:
        if out.dtype != torch.float32:
            raise NativeError('the envelope epilogue is float32 only')
        _check(lib().sig_biquad_coldstart_env(*head, *_envelope(envelope, voices), *window, *dst, *tail), 'sig_biquad_coldstart_env')
        return out
    _check(lib().sig_biquad_coldstart(*head, *window, *dst, _dt(out), *tail), 'sig_biquad_coldstart')
    return out


def _block_rows(t: torch.Tensor, what: str, nblocks: int, voices: int, broadcast: bool = False):
    """(ptr, stride, blocks) of a cold-start filter's control rows: contiguous f64 (1 | nblocks, 1 | voices); narrower than the
    voices: the reference's IndexError (it indexes crit[0, i] for every channel i, fx.py:99) unless `broadcast` (one column for all)"""
    if t.dtype != torch.float64 or t.dim() != 2 or not t.is_contiguous():
        raise NativeError(f'{what} must be a contiguous float64 2-D tensor')
    if t.shape[0] not in (1, nblocks) or t.shape[1] not in (1, voices):
        raise NativeError(f'{what} shape {tuple(t.shape)} vs blocks {nblocks} voices {voices}')
    if t.shape[1] != voices and voices != 1 and not broadcast:
        raise IndexError(f'index {t.shape[1]} is out of bounds for axis 1 with size {t.shape[1]}')
    return t.data_ptr(), 0 if t.shape[1] == 1 else 1, t.shape[0]


def _optional_rows(t: torch.Tensor | None, what: str, nblocks: int, voices: int):
    """`_block_rows` of a control that may be unplugged (None: a null row) and that one column holds for every voice"""
    return (None, 0, 1) if t is None else _block_rows(t, what, nblocks, voices, broadcast=True)


def biquad_coldstart_q(btype: str, rate: int, position: int, block_frames: int, nblocks: int, context: int,
                       cutoff: torch.Tensor, resonance: torch.Tensor | None, buf: torch.Tensor, history: int, out: torch.Tensor,
                       status: torch.Tensor | None = None) -> torch.Tensor:
    """`biquad_coldstart` with a resonance row (sig_biquad_coldstart_q: the resonant low-pass / high-pass of chain/ext.py).
    cutoff: f64 (1|nblocks, V); resonance: f64 (1|nblocks, V|1), a one-column row holds for every voice (the nodes refuse a narrow
    one before they get here); each per block on its own; resonance None: unplugged = 1/sqrt2 (the Butterworth design)."""
    voices, head, window, dst, tail = _coldstart_launch('biquad', rate, position, block_frames, nblocks, context, buf, history, out, status,
                                                cutoff, resonance)
    q = _optional_rows(resonance, 'resonance', nblocks, voices)
    _check(lib().sig_biquad_coldstart_q(FILT_TYPES[btype], *head, *_block_rows(cutoff, 'cutoff', nblocks, voices), *q,
                                        *window, *dst, _dt(out), *tail), 'sig_biquad_coldstart_q')
    return out


def biquad_coldstart_eq(btype: str, rate: int, position: int, block_frames: int, nblocks: int, context: int,
                        cutoff: torch.Tensor, resonance: torch.Tensor | None, gain: torch.Tensor | None, buf: torch.Tensor, history: int,
                        out: torch.Tensor, status: torch.Tensor | None = None) -> torch.Tensor:
    """`biquad_coldstart_q` for the equaliser biquads (sig_biquad_coldstart_eq; btype 'eqbp' | 'eqnotch' | 'eqap' | 'eqpeak' | 'eqls' |
    'eqhs').  cutoff: f64 (1|nblocks, V); resonance and gain (dB): f64 (1|nblocks, V|1), each per block on its own; None: unplugged
    = 1/sqrt2 and 0 dB."""
    voices, head, window, dst, tail = _coldstart_launch('biquad', rate, position, block_frames, nblocks, context, buf, history, out, status,
                                                cutoff, resonance, gain)
    q = _optional_rows(resonance, 'resonance', nblocks, voices)
    g = _optional_rows(gain, 'gain', nblocks, voices)
    _check(lib().sig_biquad_coldstart_eq(FILT_TYPES[btype], *head, *_block_rows(cutoff, 'cutoff', nblocks, voices), *q, *g,
                                         *window, *dst, _dt(out), *tail), 'sig_biquad_coldstart_eq')
    return out


def ladder_coldstart(rate: int, position: int, block_frames: int, nblocks: int, context: int, cutoff: torch.Tensor,
                     resonance: torch.Tensor | None, drive: torch.Tensor | None, poles: int, buf: torch.Tensor, history: int,
                     out: torch.Tensor, status: torch.Tensor | None = None) -> torch.Tensor:
    """the 4-pole ladder low-pass (sig_ladder_coldstart; chain/ext.py Ladder), buffers and blocks as `biquad_coldstart_q`.
    cutoff: f64 (1|nblocks, V); resonance (the feedback k, clipped to 0 .. 4) and drive (the saturator's, max(drive, 0)): f64
    (1|nblocks, V|1), each per block on its own; None: unplugged = 0 -- no feedback, and for drive the kernel without tanh.
    poles: 1 .. 4, the output tap."""
    voices, head, window, dst, tail = _coldstart_launch('ladder', rate, position, block_frames, nblocks, context, buf, history, out, status,
                                                cutoff, resonance, drive)
    k = _optional_rows(resonance, 'resonance', nblocks, voices)
    d = _optional_rows(drive, 'drive', nblocks, voices)
    _check(lib().sig_ladder_coldstart(*head, *_block_rows(cutoff, 'cutoff', nblocks, voices), *k, *d, int(poles),
                                      *window, *dst, _dt(out), *tail), 'sig_ladder_coldstart')
    return out


def _operand(t: torch.Tensor, rows: int, cols: int, what: str) -> Operand:
    """numpy-broadcast operand; an operand with R rows where rows % R == 0 is a per-block control operand
    (R blocks of rows // R frames each)."""
    if t.dim() != 2 or t.shape[1] not in (1, cols) or t.shape[0] < 1 or rows % t.shape[0]:
        raise NativeError(f'{what}: shape {tuple(t.shape)} does not broadcast to {(rows, cols)}')
    rs = 0 if t.shape[0] == 1 else t.stride(0)
    cs = 0 if t.shape[1] == 1 else t.stride(1)
    row_div = 0 if t.shape[0] in (1, rows) else rows // t.shape[0]
    return Operand(t.data_ptr(), rs, cs, _dt(t), row_div, 0)


def elementwise(op: str, a: torch.Tensor, b: torch.Tensor, c: torch.Tensor | None, out: torch.Tensor) -> torch.Tensor:
    _gpu(a, b, c, out)
    _audio(out, 'elementwise out')
    rows, cols = out.shape
    A = _operand(a, rows, cols, 'a')
    B = _operand(b, rows, cols, 'b')
    C = _operand(c, rows, cols, 'c') if c is not None else None
    _check(lib().sig_elementwise(EW_OPS[op], rows, cols, ctypes.byref(A), ctypes.byref(B),
                                 ctypes.byref(C) if C is not None else None,
                                 out.data_ptr(), out.stride(0), _dt(out), _stream(out)), 'sig_elementwise')
    return out


def sum_bus(x: torch.Tensor, gains: torch.Tensor | None, out: torch.Tensor) -> torch.Tensor:
    _gpu(x, gains, out)
    _audio(x, 'bus in')
    _audio(out, 'bus out')
    rows, voices = x.shape
    bus = out.shape[1]
    if out.shape[0] != rows:
        raise NativeError('bus rows mismatch')
    gp, gld = None, 0
    if gains is not None:
        if gains.dtype != torch.float64 or gains.dim() != 2 or gains.shape != (bus, voices) or gains.stride(1) != 1:
            raise NativeError(f'gains must be float64 ({bus},{voices}), got {tuple(gains.shape)} {gains.dtype}')
        gp, gld = gains.data_ptr(), gains.stride(0)
    # the kernel is built for 1, 2 and 4 bus channels; any other width is a few calls over column groups
    c0, esz = 0, out.element_size()
    while c0 < bus:
        w = 4 if bus - c0 >= 4 else (2 if bus - c0 >= 2 else 1)
        _check(lib().sig_sum_bus(rows, voices, x.data_ptr(), x.stride(0), _dt(x),
                                 gp + c0 * gld * 8 if gp is not None else None, gld, w,
                                 out.data_ptr() + c0 * esz, out.stride(0), _dt(out), _stream(out)), 'sig_sum_bus')
        c0 += w
    return out


def white_noise(seed: int, position: int, out: torch.Tensor) -> torch.Tensor:
    _gpu(out)
    _audio(out, 'noise out')
    _check(lib().sig_white_noise(seed, position, out.shape[0], out.shape[1], out.data_ptr(), _dt(out),
                                 out.stride(0), _stream(out)), 'sig_white_noise')
    return out


def adsr(position: int, rate: int, rows: dict, out: torch.Tensor) -> torch.Tensor:
    """rows: name -> f64 control row (1,V)|(1,1) for each of ADSR_PARAMS"""
    _gpu(out, *rows.values())
    _audio(out, 'adsr out')
    _check(lib().sig_adsr(position, rate, out.shape[0], out.shape[1], *_envelope(rows, out.shape[1]), out.data_ptr(), _dt(out),
                          out.stride(0), _stream(out)), 'sig_adsr')
    return out


def mix_matrix(x: torch.Tensor, matrix: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    _gpu(x, matrix, out)
    _audio(x, 'mix_matrix in')
    _audio(out, 'mix_matrix out')
    if x.dtype != torch.float32 or out.dtype != torch.float32 or matrix.dtype != torch.float32:
        raise NativeError('mix_matrix is float32 in / float32 out')
    if matrix.shape != (64, 64) or not matrix.is_contiguous() or x.shape != out.shape or x.shape[1] % 64:
        raise NativeError(f'mix_matrix shapes: x {tuple(x.shape)} matrix {tuple(matrix.shape)} out {tuple(out.shape)}')
    _check(lib().sig_mix_matrix(x.shape[0], x.shape[1], x.data_ptr(), x.stride(0), matrix.data_ptr(),
                                out.data_ptr(), out.stride(0), _stream(out)), 'sig_mix_matrix')
    return out


def fused_osc_biquad(kind: str, btype: str, rate: int, position, block_frames: int, nblocks: int, context: int,
                     hertz: torch.Tensor, phase: torch.Tensor | None, cutoff: torch.Tensor,
                     gain: torch.Tensor | None, out: torch.Tensor, status: torch.Tensor | None = None) -> torch.Tensor:
    """out (nblocks*block_frames, voices) f32 <- [gain *] Filter(Osc), every block cold-started.
    `position`: an int, or a one-element int64 device tensor read by the kernel (hipGraph replay)."""
    _gpu(hertz, phase, cutoff, gain, out, status)
    _audio(out, 'fused out')
    rows, voices = out.shape
    if out.dtype != torch.float32 or rows != block_frames * nblocks:
        raise NativeError(f'fused out must be float32 ({block_frames * nblocks}, V), got {tuple(out.shape)} {out.dtype}')
    ptrs = _voice_rows(voices, (hertz, 'hertz'), (phase, 'phase'), (cutoff, 'cutoff'), (gain, 'gain'))
    entry, name = lib().sig_fused_osc_biquad, 'sig_fused_osc_biquad'
    if isinstance(position, torch.Tensor):
        entry, name, position = lib().sig_fused_osc_biquad_devpos, 'sig_fused_osc_biquad_devpos', _device_position(position)
    _check(entry(OSC_KINDS[kind], FILT_TYPES[btype], rate, position, block_frames, nblocks, context, voices, *ptrs,
                 out.data_ptr(), out.stride(0), _ptr(status), _stream(out)), name)
    return out


def _device_position(position: torch.Tensor) -> int:
    """the pointer of a frame position the kernel reads on the device"""
    if position.dtype != torch.int64 or position.numel() != 1 or not position.is_cuda:
        raise NativeError('device position must be a one-element int64 GPU tensor')
    return position.data_ptr()


def biquad_coldstart_bus(btype: str, rate: int, position: int, block_frames: int, nblocks: int, context: int,
                         cutoff: torch.Tensor, buf: torch.Tensor, history: int, bus_gains: torch.Tensor | None,
                         out: torch.Tensor, envelope: dict | None = None, workspace: torch.Tensor | None = None,
                         status: torch.Tensor | None = None) -> torch.Tensor:
    """out (nblocks*block_frames, C) f32 <- sum over voices of bus_gains * [envelope *] Filter(buf); `buf` holds
    `history` context rows followed by the input rows, like `biquad_coldstart`; `envelope`: ADSR control rows"""
    voices, head, window, dst, tail = _coldstart_launch('biquad bus', rate, position, block_frames, nblocks, context, buf, history, out, status,
                                                cutoff, bus_gains, *(envelope or {}).values(), per_voice=buf, f32_only=True)
    rows, bus = out.shape
    if cutoff.dtype != torch.float64 or cutoff.shape[1] not in (1, voices) or cutoff.shape[0] not in (1, nblocks) \
            or not cutoff.is_contiguous():
        raise NativeError(f'cutoff must be contiguous float64 (1|{nblocks}, 1|{voices}), got {tuple(cutoff.shape)} {cutoff.dtype}')
    workspace = _bus_workspace(workspace, voices, rows, bus, out.device)
    _check(lib().sig_biquad_coldstart_bus(FILT_TYPES[btype], *head, cutoff.data_ptr(), 0 if cutoff.shape[1] == 1 else 1, cutoff.shape[0],
                                          *_envelope(envelope, voices), *window, *_bus_gains(bus_gains, bus, voices), bus,
                                          workspace.data_ptr(), *dst, *tail), 'sig_biquad_coldstart_bus')
    return out


def latency_voice_bus_workspace(voices: int, block_frames: int, bus_channels: int, device) -> torch.Tensor:
    """zeroed scratch of `latency_voice_bus` (per-tile partials + the arrival counter, which must start at zero)"""
    return torch.zeros(lib().sig_latency_voice_bus_workspace(voices, block_frames, bus_channels) // 8, dtype=torch.float64,
                       device=device)


def latency_voice_bus(btype: str, rate: int, position, block_frames: int, context: int, voices: int,
                      hertz: torch.Tensor, phase: torch.Tensor | None, cutoff: torch.Tensor, gain: torch.Tensor | None,
                      bus_gains: torch.Tensor | None, out: torch.Tensor, workspace: torch.Tensor,
                      status: torch.Tensor | None = None) -> torch.Tensor:
    """out (block_frames, C) f32 <- one block of sum over voices of pan * [gain *] Filter(Sine), in one launch.
    `position`: an int, or a one-element int64 device tensor that the launch reads AND advances by block_frames."""
    _gpu(out)
    _audio(out, 'latency bus out')
    rows, bus = out.shape
    if out.dtype != torch.float32 or rows != block_frames:
        raise NativeError(f'latency bus out must be float32 ({block_frames}, C), got {tuple(out.shape)} {out.dtype}')
    call = LatencyVoiceBusCall(btype, rate, block_frames, context, voices, hertz, phase, cutoff, gain, bus_gains, bus, workspace,
                               status)
    pos_int, pos_dev = position, None
    if isinstance(position, torch.Tensor):
        pos_int, pos_dev = 0, _device_position(position)
    _check(call._fn(*call._head, pos_int, pos_dev, *call._mid, out.data_ptr(), out.stride(0), call._status, _stream(out)),
           'sig_latency_voice_bus')
    return out


class LatencyVoiceBusCall:
    """`latency_voice_bus` with everything but the position and the output buffer validated and converted ONCE: the
    per-block host path of latency mode is then one ctypes call (the tensors are kept alive by this object)."""

    def __init__(self, btype: str, rate: int, block_frames: int, context: int, voices: int,
                 hertz: torch.Tensor, phase: torch.Tensor | None, cutoff: torch.Tensor, gain: torch.Tensor | None,
                 bus_gains: torch.Tensor | None, bus_channels: int, workspace: torch.Tensor,
                 status: torch.Tensor | None = None):
        _gpu(hertz, phase, cutoff, gain, bus_gains, workspace, status)
        need = lib().sig_latency_voice_bus_workspace(voices, block_frames, bus_channels)
        if workspace.dtype != torch.float64 or workspace.numel() * 8 < need:
            raise NativeError(f'latency workspace needs {need} bytes of float64 (latency_voice_bus_workspace)')
        ptrs = _voice_rows(voices, (hertz, 'hertz'), (phase, 'phase'), (cutoff, 'cutoff'), (gain, 'gain'))
        gp, gld = _bus_gains(bus_gains, bus_channels, voices)
        self._keep = (hertz, phase, cutoff, gain, bus_gains, workspace, status)
        self._fn = lib().sig_latency_voice_bus
        self._head = (FILT_TYPES[btype], rate)
        self._mid = (block_frames, context, voices, *ptrs, gp, gld, bus_channels, workspace.data_ptr())
        self._status = _ptr(status)
        self.shape = (block_frames, bus_channels)
        self.device = workspace.device

    def __call__(self, position: int, out: torch.Tensor) -> torch.Tensor:
        """`out`: a contiguous float32 (block_frames, bus_channels) tensor on the launch device"""
        err = self._fn(*self._head, position, None, *self._mid, out.data_ptr(), self.shape[1], self._status, _stream(out))
        if err:
            raise NativeError(f'sig_latency_voice_bus failed: hipError_t {err}')
        return out


class FusedVoiceBusCallT(ctypes.Structure):
    """sig_fused_voice_bus_call (host memory)"""
    _fields_ = [(n, ctypes.c_int32) for n in ('osc_kind', 'filt_type', 'rate', 'block_frames', 'nblocks', 'context', 'voices',
                                              'hertz_stride', 'phase_stride', 'cutoff_stride', 'gain_stride', 'bus_channels')] + \
               [(n, ctypes.c_void_p) for n in ('hertz', 'phase', 'cutoff', 'gain', 'bus_gains')] + \
               [('bus_gains_ld', ctypes.c_int64), ('out_ld', ctypes.c_int64), ('workspace', ctypes.c_void_p), ('status', ctypes.c_void_p),
                ('consts', ctypes.c_void_p)]


class FusedVoiceBusCall:
    """`fused_voice_bus` with caller-held closed-form constants (sig_fused_voice_bus_prepared / _walk) and everything but the
    position and the output buffer validated and converted ONCE: the per-batch host path of the batched engine is then one
    ctypes call (at 256 blocks per batch the launch takes ~18 us; the generic binding's per-call validation took longer than
    that).  The tensors are kept alive by this object."""

    def __init__(self, kind: str, btype: str, rate: int, block_frames: int, nblocks: int, context: int, voices: int,
                 hertz: torch.Tensor, phase: torch.Tensor | None, cutoff: torch.Tensor, gain: torch.Tensor | None,
                 bus_gains: torch.Tensor | None, bus_channels: int, workspace: torch.Tensor, status: torch.Tensor | None,
                 consts: torch.Tensor):
        _gpu(hertz, phase, cutoff, gain, bus_gains, workspace, status, consts)
        rows = block_frames * nblocks
        hp, hs, pp, ps, cp, cs, gp_, gs = _voice_rows(voices, (hertz, 'hertz'), (phase, 'phase'), (cutoff, 'cutoff'), (gain, 'gain'))
        gp, gld = _bus_gains(bus_gains, bus_channels, voices)
        _bus_workspace(workspace, voices, rows, bus_channels)
        self._keep = (hertz, phase, cutoff, gain, bus_gains, workspace, status, consts)
        self.shape = (rows, bus_channels)
        # the whole call as one block for sig_fused_voice_bus_bound: six arguments per call instead of 26
        self._block = FusedVoiceBusCallT(OSC_KINDS[kind], FILT_TYPES[btype], rate, block_frames, nblocks, context, voices, hs, ps, cs, gs,
                                         bus_channels, hp, pp, cp, gp_, gp, gld, bus_channels, workspace.data_ptr(), _ptr(status),
                                         _consts(consts, voices))
        self._block_ref = ctypes.byref(self._block)
        self._bound = lib().sig_fused_voice_bus_bound

    def __call__(self, position: int, out: torch.Tensor, consts_ready: bool, walk: bool = False, stream: int | None = None) -> torch.Tensor:
        """`out`: a contiguous float32 (nblocks * block_frames, bus_channels) tensor on the launch device; `stream`: a raw
        hipStream_t to launch on instead of torch's current one (the caller orders it against whoever reads `out`)"""
        s = _stream(out) if stream is None else stream
        err = self._bound(self._block_ref, position, out.data_ptr(), 1 if consts_ready else 0, 1 if walk else 0, s)
        if err:
            raise NativeError(f'sig_fused_voice_bus failed: hipError_t {err}')
        return out


def _consts(consts: torch.Tensor, voices: int) -> int:
    """the pointer of a caller-held buffer for the Sine closed form's per-voice constants"""
    if consts.dtype != torch.float64 or consts.numel() * 8 < lib().sig_fused_voice_consts_size(voices):
        raise NativeError('consts must be float64 of sig_fused_voice_consts_size(voices) bytes')
    return consts.data_ptr()


def fused_geometry(voices: int, block_frames: int, nblocks: int, context: int) -> tuple[int, int]:
    """(voices per lane, blocks per lane) the fused kernels use for this problem size"""
    vpt, span = ctypes.c_int32(), ctypes.c_int32()
    _check(lib().sig_fused_geometry(voices, block_frames, nblocks, context, ctypes.byref(vpt), ctypes.byref(span)),
           'sig_fused_geometry')
    return vpt.value, span.value


def _param_rows(t: torch.Tensor | None, what: str, voices: int, nblocks: int):
    """(ptr, stride, rows) of a per-block parameter: float64 (1|nblocks, V|1), rows contiguous"""
    if t is None:
        return None, 0, 1
    if t.dtype != torch.float64 or t.dim() != 2 or not t.is_contiguous() or t.shape[1] not in (1, voices) or t.shape[0] not in (1, nblocks):
        raise NativeError(f'{what}: per-block parameters are contiguous float64 (1|{nblocks}, 1|{voices}), got {tuple(t.shape)} {t.dtype}')
    return t.data_ptr(), (0 if t.shape[1] == 1 else 1), t.shape[0]


def fused_rows(kind: str, btype: str, rate: int, position: int, block_frames: int, nblocks: int, context: int, voices: int,
               hertz: torch.Tensor, phase: torch.Tensor | None, cutoff: torch.Tensor, gain: torch.Tensor | None,
               out: torch.Tensor, bus_gains: torch.Tensor | None = None, bus: bool = False,
               workspace: torch.Tensor | None = None, status: torch.Tensor | None = None,
               pair: tuple | None = None, hertz_hist: torch.Tensor | None = None,
               phase_hist: torch.Tensor | None = None) -> torch.Tensor:
    """[gain *] Filter(Osc) with cutoff / gain rows read per block: out (nblocks*block_frames, voices) f32
    (sig_fused_osc_biquad_rows), or with `bus` the sum over voices weighted by bus_gains, out (.., C) (sig_fused_voice_bus_rows).
    `pair` = (op, kind2, hertz2, phase2, mix): the filter reads Mix (op 'Mix') or RingMod (op 'RingMod') of the oscillator
    above and a second one (sig_fused_osc_pair_biquad / sig_fused_voice_pair_bus).
    hertz / phase with nblocks rows: block-rate FM (sig_fused_osc_biquad_fm / sig_fused_voice_bus_fm); `hertz_hist` /
    `phase_hist` = the (1, .) row in front of the launch (the previous block's, whose samples are block 0's context)."""
    _gpu(hertz, phase, cutoff, gain, out, bus_gains, workspace, status, hertz_hist, phase_hist,
         *((pair[2], pair[3], pair[4]) if pair else ()))
    _audio(out, 'fused rows out')
    rows = out.shape[0]
    if out.dtype != torch.float32 or rows != block_frames * nblocks:
        raise NativeError(f'fused rows out must be float32 ({block_frames * nblocks}, .), got {tuple(out.shape)} {out.dtype}')
    # the source -- how hertz and phase are marshalled -- decides which pair of entry points (voices out, bus out) runs
    kinds = (OSC_KINDS[kind], FILT_TYPES[btype])
    if hertz_hist is not None or phase_hist is not None or hertz.shape[0] > 1 or (phase is not None and phase.shape[0] > 1):
        if pair is not None:
            raise NativeError('block-rate FM and a second oscillator: no fused entry point')
        names = ('sig_fused_osc_biquad_fm', 'sig_fused_voice_bus_fm')
        source = []
        for t, front, what in ((hertz, hertz_hist, 'hertz'), (phase, phase_hist, 'phase')):
            ptr, stride, count = _param_rows(t, what, voices, nblocks)
            if t is not None and not (front is None and count == 1):
                if front is None or front.dtype != torch.float64 or tuple(front.shape) != (1, t.shape[1]) or not front.is_contiguous():
                    raise NativeError(f'{what}_hist: the row in front of the launch is float64 (1, {t.shape[1]})')
            source += [ptr, stride, count, _ptr(front) if t is not None else None]
    else:
        names = ('sig_fused_osc_biquad_rows', 'sig_fused_voice_bus_rows')
        source = _voice_rows(voices, (hertz, 'hertz'), (phase, 'phase'))
        if pair is not None:
            op, kind2, hertz2, phase2, mixrow = pair
            names = ('sig_fused_osc_pair_biquad', 'sig_fused_voice_pair_bus')
            kinds = (OSC_KINDS[kind], OSC_KINDS[kind2], {'Mix': 1, 'RingMod': 2}[op], FILT_TYPES[btype])
            source += _voice_rows(voices, (hertz2, 'hertz2'), (phase2, 'phase2'), (mixrow, 'mix'))
    sink = ()
    if bus:
        C = out.shape[1]
        workspace = _bus_workspace(workspace, voices, rows, C, out.device)
        sink = (*_bus_gains(bus_gains, C, voices), C, workspace.data_ptr())
    elif out.shape[1] != voices:
        raise NativeError(f'fused rows out has {out.shape[1]} channels for {voices} voices')
    name = names[1 if bus else 0]
    _check(getattr(lib(), name)(*kinds, rate, position, block_frames, nblocks, context, voices, *source,
                                *_param_rows(cutoff, 'cutoff', voices, nblocks), *_param_rows(gain, 'gain', voices, nblocks),
                                *sink, out.data_ptr(), out.stride(0), _ptr(status), _stream(out)), name)
    return out


def fused_cascade_bus(kind: str, btype1: str, btype2: str, rate: int, position: int, first_history_start: int,
                      block_frames: int, nblocks: int, context: int, voices: int,
                      hertz: torch.Tensor, phase: torch.Tensor | None, cutoff1: torch.Tensor, cutoff2: torch.Tensor,
                      gain: torch.Tensor | None, envelope: dict | None, bus_gains: torch.Tensor | None, out: torch.Tensor,
                      workspace: torch.Tensor | None = None, status: torch.Tensor | None = None) -> torch.Tensor:
    """out (nblocks*block_frames, C) f32 <- sum over voices of pan * [gain *] [ADSR *] Filter2(Filter1(Osc)), the two
    filters in series with the reference's block-cache history between them (sig_fused_cascade_bus)"""
    _gpu(hertz, phase, cutoff1, cutoff2, gain, bus_gains, out, workspace, status, *(envelope or {}).values())
    _audio(out, 'fused cascade out')
    rows, bus = out.shape
    if out.dtype != torch.float32 or rows != block_frames * nblocks:
        raise NativeError(f'fused cascade out must be float32 ({block_frames * nblocks}, C), got {tuple(out.shape)} {out.dtype}')
    ptrs = _voice_rows(voices, (hertz, 'hertz'), (phase, 'phase'), (cutoff1, 'cutoff1'), (cutoff2, 'cutoff2'), (gain, 'gain'))
    workspace = _bus_workspace(workspace, voices, rows, bus, out.device)
    _check(lib().sig_fused_cascade_bus(OSC_KINDS[kind], FILT_TYPES[btype1], FILT_TYPES[btype2], rate, position,
                                       first_history_start, block_frames, nblocks, context, voices, *ptrs,
                                       *_envelope(envelope, voices), *_bus_gains(bus_gains, bus, voices), bus,
                                       workspace.data_ptr(), out.data_ptr(), out.stride(0), _ptr(status), _stream(out)),
           'sig_fused_cascade_bus')
    return out


def fused_cascade_geometry(voices: int, nblocks: int) -> tuple[int, int]:
    """(voices per lane, blocks per lane) of `fused_cascade_bus` for this problem size"""
    vpt, span = ctypes.c_int32(), ctypes.c_int32()
    _check(lib().sig_fused_cascade_geometry(voices, nblocks, ctypes.byref(vpt), ctypes.byref(span)), 'sig_fused_cascade_geometry')
    return vpt.value, span.value


def set_fused_cascade_tuning(voices_per_lane: int = 0, blocks_per_lane: int = 0) -> None:
    """tuning / test hook (process-wide): force `fused_cascade_bus`'s launch geometry; the defaults restore the heuristic"""
    _check(lib().sig_fused_cascade_set_tuning(voices_per_lane, blocks_per_lane), 'sig_fused_cascade_set_tuning')


def fused_cascade_model(voices: int, block_frames: int, nblocks: int, context: int = 100, bus_channels: int = 1,
                        osc_ops: float = 5.0, envelope: bool = True) -> dict:
    """f64-rate VALU instructions per stored voice-sample of `fused_cascade_bus` (bench.py's roofline): the exact-phase
    oscillator (5 for a Sawtooth: t = q * hertz + phase, t - 0.5, v_fract_f64, 2 m - 1) and the inner filter (4) on every
    row a lane walks -- span * N output rows and one history block of N + context rows per span -- the outer filter (4)
    on the output rows and the history's last `context` rows, envelope x weight (C) and bus (C) FMAs, the folded flush,
    and the two restarts per (voice, block boundary) (2x2 power by squaring: 10 products of 8 + 6 for `context` = 100)"""
    vpt, span = fused_cascade_geometry(voices, nblocks)
    n, c = block_frames, context
    walked = (span * n + n + c) / (span * n)                    # oscillator + inner filter rows per output row
    products = max(c, 1).bit_length() - 1 + bin(max(c, 1)).count('1')
    restart = 8.0 * products + 6.0
    ops = (osc_ops + 4.0) * walked + 4.0 * (1.0 + c / (span * n)) + (bus_channels if envelope else 0.0) + bus_channels \
        + 17.0 * bus_channels / (16 * vpt) + restart * (2 * (span - 1) + 1) / (span * n)
    return {'f64_ops_per_voice_sample': ops, 'voices_per_lane': vpt, 'blocks_per_lane': span,
            'rows_walked_per_output_row': walked}


def upload_structs(items: list) -> torch.Tensor:
    """a list of ctypes structures of one type as a device byte tensor (a control program, its output table)"""
    arr = (type(items[0]) * len(items))(*items)
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    return host.to(runtime_device())


def runtime_device():
    from . import runtime
    return runtime.device()


def control_program(rate: int, position: int, step: int, nblocks: int, cols: int, program: torch.Tensor, n_ins: int,
                    outs: torch.Tensor, n_outs: int, front_position: int = -1, min_position: int = 0, windowed: bool = False,
                    envelope: bool = False) -> None:
    """run a block-rate control program (sig_control_program): `program` / `outs` are device byte tensors of CtlIns / CtlOut;
    `front_position` >= 0 also evaluates it at that position into the outputs' `front` rows; blocks whose position lies below
    `min_position` are evaluated there.  `windowed`: the program holds Noise / Filter instructions (sig_control_program_windowed);
    `envelope`: it holds ADSR pairs (sig_control_program_envelope, which runs the windowed ones as well)"""
    _gpu(program, outs)
    entry = lib().sig_control_program_envelope if envelope else lib().sig_control_program_windowed if windowed else lib().sig_control_program
    _check(entry(rate, position, step, nblocks, cols, front_position, min_position, program.data_ptr(), n_ins,
                                     outs.data_ptr(), n_outs, _stream(program)), 'sig_control_program')


def control_program_description(ins: list, outs: list) -> list:
    """what a specialised build of control_program.hip is keyed by: [n_ins, n_outs, (op, kind, a, b, c, dst, wide) per
    instruction (wide: bit 0 more than one column, bit 1 window-rate), (reg, wide) per output] -- the program's structure without its pointers (CtlIns / CtlOut lists)"""
    args_op, adsr_op = CTL_OPS['AdsrArgs'], CTL_OPS['Adsr']
    for k, x in enumerate(ins):     # (the uploaded program is device memory: the library cannot look, sig_control_program_envelope)
        if (x.op == adsr_op and (k == 0 or ins[k - 1].op != args_op or (ins[k - 1].cols, ins[k - 1].reserved) != (x.cols, x.reserved))) or \
                (x.op == args_op and (k + 1 >= len(ins) or ins[k + 1].op != adsr_op)):
            raise ValueError(f'control program: instruction {k} is half of an AdsrArgs / Adsr pair')
    words = [len(ins), len(outs)]
    for x in ins:
        words += [x.op, x.kind, x.a, x.b, x.c, x.dst, (1 if x.cols > 1 else 0) | (2 if x.reserved else 0)]
    for o in outs:
        words += [o.reg, 1 if o.cols > 1 else 0]
    return words


def control_program_attach(description: list, image: bytes) -> int:
    """hand the library a build of control_program.hip specialised for this structure; returns the handle to launch it with"""
    arr = (ctypes.c_int32 * len(description))(*description)
    handle = ctypes.c_int32(0)
    _check(lib().sig_control_program_attach(arr, len(description), image, ctypes.byref(handle)), 'sig_control_program_attach')
    return handle.value


def control_program_attached(handle: int, rate: int, position: int, step: int, nblocks: int, cols: int, program: torch.Tensor,
                             n_ins: int, outs: torch.Tensor, n_outs: int, front_position: int = -1, min_position: int = 0) -> None:
    """`control_program` through the specialised kernel behind `handle` (same arguments, same values)"""
    _gpu(program, outs)
    _check(lib().sig_control_program_attached(handle, rate, position, step, nblocks, cols, front_position, min_position,
                                              program.data_ptr(), n_ins, outs.data_ptr(), n_outs, _stream(program)),
           'sig_control_program_attached')


def fused_voice_bus_plan(kind: str, position: int, voices: int, block_frames: int, nblocks: int, context: int) -> dict:
    """what `fused_voice_bus` launches for this problem: {'voices_per_lane', 'blocks_per_lane', 'closed_form', 'kernel'}"""
    vpt, span, closed = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    _check(lib().sig_fused_voice_bus_plan(OSC_KINDS[kind], position, voices, block_frames, nblocks, context,
                                          ctypes.byref(vpt), ctypes.byref(span), ctypes.byref(closed)),
           'sig_fused_voice_bus_plan')
    kernel = f'fused_steady_bus_kernel<{vpt.value}, C>' if closed.value else f'fused_walk_kernel<{kind}, {vpt.value}, gain, C>'
    return {'voices_per_lane': vpt.value, 'blocks_per_lane': span.value, 'closed_form': bool(closed.value), 'kernel': kernel}


def set_fused_tuning(voices_per_lane: int = 0, blocks_per_lane: int = 0, closed_form: int = -1, scan: int = -1) -> None:
    """tuning / test hook (process-wide): force the fused kernels' launch geometry; the defaults restore the heuristics"""
    _check(lib().sig_fused_set_tuning(voices_per_lane, blocks_per_lane, closed_form, scan), 'sig_fused_set_tuning')


def fused_osc_biquad_mix(kind: str, btype: str, rate: int, position: int, block_frames: int, nblocks: int, context: int,
                         hertz: torch.Tensor, phase: torch.Tensor | None, cutoff: torch.Tensor,
                         gain: torch.Tensor | None, matrix: torch.Tensor, out: torch.Tensor,
                         status: torch.Tensor | None = None) -> torch.Tensor:
    """out (nblocks*block_frames, voices) f32 <- ([gain *] Filter(Osc)) @ blockdiag(matrix), 64-voice groups"""
    _gpu(hertz, phase, cutoff, gain, matrix, out, status)
    _audio(out, 'fused mix out')
    rows, voices = out.shape
    if out.dtype != torch.float32 or rows != block_frames * nblocks or voices % 64:
        raise NativeError(f'fused mix out must be float32 ({block_frames * nblocks}, 64*g), got {tuple(out.shape)} {out.dtype}')
    if matrix.dtype != torch.float32 or tuple(matrix.shape) != (64, 64) or not matrix.is_contiguous():
        raise NativeError(f'mix matrix must be contiguous float32 (64, 64), got {tuple(matrix.shape)} {matrix.dtype}')
    ptrs = _voice_rows(voices, (hertz, 'hertz'), (phase, 'phase'), (cutoff, 'cutoff'), (gain, 'gain'))
    _check(lib().sig_fused_osc_biquad_mix(OSC_KINDS[kind], FILT_TYPES[btype], rate, position, block_frames, nblocks, context,
                                          voices, *ptrs, matrix.data_ptr(), out.data_ptr(), out.stride(0), _ptr(status),
                                          _stream(out)), 'sig_fused_osc_biquad_mix')
    return out


def advance_position(position: torch.Tensor, delta: int) -> None:
    """position[0] += delta on the device, in stream order"""
    _gpu(position)
    _check(lib().sig_advance_position(position.data_ptr(), delta, _stream(position)), 'sig_advance_position')


def fused_voice_bus(kind: str, btype: str, rate: int, position: int, block_frames: int, nblocks: int, context: int,
                    voices: int, hertz: torch.Tensor, phase: torch.Tensor | None, cutoff: torch.Tensor,
                    gain: torch.Tensor | None, bus_gains: torch.Tensor | None, out: torch.Tensor,
                    workspace: torch.Tensor | None = None, status: torch.Tensor | None = None,
                    consts: torch.Tensor | None = None, consts_ready: bool = False, walk: bool = False) -> torch.Tensor:
    """out (nblocks*block_frames, bus_channels) f32 <- sum over voices of pan * [gain *] Filter(Osc).
    `consts`: a float64 device buffer of sig_fused_voice_consts_size(voices) bytes the caller keeps across calls for
    the Sine closed form's per-voice constants; `consts_ready`: it already holds them for these parameters.
    `walk`: the row-by-row span walker only (sig_fused_voice_bus_walk): for launches the caller knows to lie beyond the
    closed form's phase range (SINE_FAST_MAX_CYCLES)."""
    _gpu(hertz, phase, cutoff, gain, bus_gains, out, status, consts)
    _audio(out, 'fused bus out')
    rows, bus = out.shape
    if out.dtype != torch.float32 or rows != block_frames * nblocks:
        raise NativeError(f'fused bus out must be float32 ({block_frames * nblocks}, C), got {tuple(out.shape)} {out.dtype}')
    ptrs = _voice_rows(voices, (hertz, 'hertz'), (phase, 'phase'), (cutoff, 'cutoff'), (gain, 'gain'))
    workspace = _bus_workspace(workspace, voices, rows, bus, out.device)
    entry, name, tail = lib().sig_fused_voice_bus, 'sig_fused_voice_bus', ()
    if walk:
        entry, name = lib().sig_fused_voice_bus_walk, 'sig_fused_voice_bus_walk'
    elif consts is not None:
        entry, name = lib().sig_fused_voice_bus_prepared, 'sig_fused_voice_bus_prepared'
        tail = (_consts(consts, voices), 1 if consts_ready else 0)
    _check(entry(OSC_KINDS[kind], FILT_TYPES[btype], rate, position, block_frames, nblocks, context, voices, *ptrs,
                 *_bus_gains(bus_gains, bus, voices), bus, workspace.data_ptr(), out.data_ptr(), out.stride(0), _ptr(status),
                 _stream(out), *tail), name)
    return out


def band_coldstart(btype: str, rate: int, position: int, block_frames: int, nblocks: int, context: int,
                   low: torch.Tensor, high: torch.Tensor, buf: torch.Tensor, history: int, out: torch.Tensor,
                   status: torch.Tensor | None = None) -> torch.Tensor:
    """BandPass ('bp') / BandStop ('bs'): two biquad sections; buffers as in `biquad_coldstart`."""
    return _band_coldstart(False, btype, rate, position, block_frames, nblocks, context, low, high, buf, history, out, status)


def band_coldstart_blocks(btype: str, rate: int, position: int, block_frames: int, nblocks: int, context: int,
                          low: torch.Tensor, high: torch.Tensor, buf: torch.Tensor, history: int, out: torch.Tensor,
                          status: torch.Tensor | None = None) -> torch.Tensor:
    """`band_coldstart` with per-block bands: low / high f64 (1|nblocks, V|1), row b (of a multi-row edge) is block b's.
    A single-row edge beside a multi-row one is repeated for every block."""
    return _band_coldstart(True, btype, rate, position, block_frames, nblocks, context, low, high, buf, history, out, status)


def _band_coldstart(per_block: bool, btype, rate, position, block_frames, nblocks, context, low, high, buf, history, out, status):
    """sig_band_coldstart, or with `per_block` sig_band_coldstart_blocks: the two differ in their band edges' rows"""
    voices, head, window, dst, tail = _coldstart_launch('band', rate, position, block_frames, nblocks, context, buf, history, out, status, low, high)
    blocks = max(low.shape[0], high.shape[0])
    edges = []
    for row, name in ((low, 'low'), (high, 'high')):
        if row.shape[1] != voices and voices != 1:
            raise IndexError(f'index {row.shape[1]} is out of bounds for axis 1 with size {row.shape[1]}')
        if per_block:
            if row.dtype != torch.float64 or row.dim() != 2 or not row.is_contiguous():
                raise NativeError(f'{name} must be a contiguous float64 2-D tensor')
            if row.shape[0] not in (1, nblocks):
                raise NativeError(f'{name} has {row.shape[0]} rows for {nblocks} blocks')
            if row.shape[0] != blocks:
                row = row.expand(blocks, row.shape[1]).contiguous()
        edges.append((row, name))                                              # (an expanded row is kept alive until the call returns)
    if per_block:
        name, entry = 'sig_band_coldstart_blocks', lib().sig_band_coldstart_blocks
        ptrs = _voice_rows(voices, *edges, form=lambda t, what: _ctrl_rows(t, what)[:2]) + [blocks]
    else:
        name, entry = 'sig_band_coldstart', lib().sig_band_coldstart
        ptrs = _voice_rows(voices, *edges)
    _check(entry(FILT_TYPES[btype], *head, *ptrs, *window, *dst, _dt(out), *tail), name)
    return out


def adsr_apply(position: int, rate: int, rows: dict, x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out = ADSR(rows) * x, float32, one pass"""
    _gpu(x, out, *rows.values())
    _audio(x, 'adsr_apply in')
    _audio(out, 'adsr_apply out')
    if x.dtype != torch.float32 or out.dtype != torch.float32 or x.shape != out.shape:
        raise NativeError(f'adsr_apply is float32 (rows, V) in and out, got {tuple(x.shape)} {x.dtype} -> {tuple(out.shape)} {out.dtype}')
    _check(lib().sig_adsr_apply(position, rate, out.shape[0], out.shape[1], *_envelope(rows, out.shape[1]), x.data_ptr(),
                                x.stride(0), out.data_ptr(), out.stride(0), _stream(out)), 'sig_adsr_apply')
    return out


def _vp_rows(t: torch.Tensor | None, what: str, voices: int, control_rows: int) -> VpRows:
    if t is None:
        return VpRows(None, 0, 1)
    if (t.dtype != torch.float64 or t.dim() != 2 or not t.is_contiguous() or t.shape[1] not in (1, voices)
            or t.shape[0] not in (1, control_rows)):
        raise NativeError(f'{what}: rows of a voice program are contiguous float64 (1|{control_rows}, 1|{voices}), got {tuple(t.shape)} {t.dtype}')
    return VpRows(t.data_ptr(), 0 if t.shape[1] == 1 else 1, t.shape[0])


def _program_struct(code: list) -> VoiceProgramT:
    """a sig_voice_program_t that holds the instructions given as (op name, kind, a, b, c) tuples"""
    P = VoiceProgramT()
    P.n_ins = len(code)
    for k, (op, kind, a, b, c) in enumerate(code):
        P.ins[k] = VpIns(VP_OPS[op], kind, a, b, c)
    return P


def voice_program(code: list, oscs: list, params: list, filters: list, n_temps: int, depth: int, rate: int, position: int,
                  block_frames: int, nblocks: int, context: int, voices: int, control_rows: int, hist_positions: list,
                  out: torch.Tensor, bus_gains: torch.Tensor | None = None, bus: bool = False,
                  adsr: dict | None = None, noise_seeds: tuple = (0, 0), workspace: torch.Tensor | None = None,
                  status: torch.Tensor | None = None, blocks_before: int = 0, tables: list | None = None,
                  unison=None) -> torch.Tensor:
    """One launch for a whole per-voice graph (sig_voice_program_ex, or with `unison` sig_voice_program_unison, or -- a program of two or more families, `vp_families` -- sig_voice_program_mixed; `tables`: the float32 (T, W) tables of its OscTable and Shape words; `unison`: the host (U, 2) copies array of its OscUni, OscBlep and OscSync words, by value).  `code`: (op name, kind, a, b, c) tuples; `oscs`: (hertz,
    phase | None) row tensors per oscillator slot; `params`: row tensors per parameter register; `filters`: (cutoff rows,
    'lp' | 'hp' ('rlp' | 'rhp': a resonant slot, run by a FilterQ word whose c names the parameter register of its q rows; 'eqbp' ... 'eqhs': an equaliser slot, run by a FilterEq word whose c names the q rows and whose b the gain rows), level = 1 + the filters in series in front of it) per filter slot.  Rows are float64 (1 | control_rows, 1 | voices).  out (nblocks * block_frames, voices) float32,
    or with `bus` (.., C) = the sum over voices weighted by bus_gains."""
    tensors = [t for pair in oscs for t in pair] + list(params) + [f[0] for f in filters] + list((adsr or {}).values())
    _gpu(out, bus_gains, workspace, status, *tensors, *(tables or ()))
    _audio(out, 'voice program out')
    rows = block_frames * nblocks
    if out.dtype != torch.float32 or out.shape[0] != rows:
        raise NativeError(f'voice program out must be float32 ({rows}, .), got {tuple(out.shape)} {out.dtype}')
    if len(code) > VP_MAX_INS or len(oscs) > VP_MAX_OSCS or len(params) > VP_MAX_PARAMS or len(filters) > VP_MAX_FILTERS \
            or n_temps > VP_MAX_TEMPS or len(hist_positions) > VP_MAX_HIST or len(tables or ()) > VP_MAX_TABLES:
        raise NativeError('voice program larger than the machine')
    P = _program_struct(code)
    P.n_oscs = len(oscs)
    for k, (hz, ph) in enumerate(oscs):
        P.hertz[k] = _vp_rows(hz, 'hertz', voices, control_rows)
        P.phase[k] = _vp_rows(ph, 'phase', voices, control_rows)
    P.n_params = len(params)
    for k, t in enumerate(params):
        P.params[k] = _vp_rows(t, 'parameter', voices, control_rows)
    P.n_filters = len(filters)
    for k, (cut, btype, level) in enumerate(filters):
        if cut.shape[1] != voices and voices != 1:
            raise IndexError(f'index {cut.shape[1]} is out of bounds for axis 1 with size {cut.shape[1]}')      # fx.py:99
        P.cutoff[k] = _vp_rows(cut, 'cutoff', voices, control_rows)
        P.filter_type[k] = FILT_TYPES[btype]
        P.filter_level[k] = level
    P.n_temps, P.depth = n_temps, depth
    _envelope(adsr, voices, into=(P.adsr, P.adsr_stride))
    P.noise_seed[0], P.noise_seed[1] = noise_seeds
    hist = (ctypes.c_int64 * max(1, len(hist_positions)))(*hist_positions)
    C = 0
    gp, gld = None, 0
    if bus:
        C = out.shape[1]
        gp, gld = _bus_gains(bus_gains, C, voices)
        workspace = _bus_workspace(workspace, voices, rows, C, out.device)
    elif out.shape[1] != voices:
        raise NativeError(f'voice program out has {out.shape[1]} channels for {voices} voices')
    held = None
    if tables:
        held = VpTablesT()
        held.n_tables = len(tables)
        wrapped = {b for op, _, _, b, _ in code if op == 'OscTable'}            # slots an oscillator reads: powers of two
        for k, t in enumerate(tables):
            held.table[k] = VpTable(*_table(t, pow2=k in wrapped))
    uni = None
    if unison is not None:
        uni = VpUnisonT()
        uni.copies, detune, offsets = _copies(unison)
        uni.detune[:uni.copies], uni.offset[:uni.copies] = list(detune), list(offsets)
    args = (ctypes.byref(P), rate, position, block_frames, nblocks, context, voices, control_rows, len(hist_positions), hist,
            blocks_before, gp, gld, C, _ptr(workspace), out.data_ptr(), out.stride(0), _ptr(status), _stream(out),
            ctypes.byref(held) if held is not None else None)
    if len(vp_families(code)) >= 2:                       # (a combined program: the one entry that takes it; every other refuses)
        _check(lib().sig_voice_program_mixed(*args, ctypes.byref(uni) if uni is not None else None), 'sig_voice_program_mixed')
    elif uni is None:                                     # (a program without the copies: the entry it always went through)
        _check(lib().sig_voice_program_ex(*args), 'sig_voice_program_ex')
    else:
        _check(lib().sig_voice_program_unison(*args, ctypes.byref(uni)), 'sig_voice_program_unison')
    return out


def vp_families(code: list) -> tuple:
    """the families (keys of VP_FAMILIES) a program given as (op name, kind, a, b, c) tuples has words of"""
    ops = {'OscUni' if op in VP_BLEP_OPS + VP_SYNC_OPS else 'FilterQ' if op in VP_EQ_OPS else op for op, *_ in code}   # (OscBlep, OscSync: words of the unison family; FilterEq: of the resonant family)
    return tuple(name for name, words in VP_FAMILIES.items() if ops & set(words))


def voice_program_words(code: list) -> list:
    """the machine words of a program given as (op name, kind, a, b, c) tuples: op | kind << 5 | a << 8 | b << 12 | c << 16"""
    return [VP_OPS[op] | (kind << 5) | (a << 8) | ((b & 15) << 12) | ((c & 15) << 16) for op, kind, a, b, c in code]   # (OscTable's, Shape's, FilterQ's, OscUni's, OscBlep's, FilterEq's and OscSync's c = -1: 15; FilterEq's and OscSync's b too)


def voice_program_geometry(voices: int, block_frames: int, nblocks: int, context: int, depth: int, bus_channels: int,
                           store_aligned: int, specialised: bool = False) -> tuple:
    """(voices per lane, blocks per lane) sig_voice_program picks for this problem (introspection, no device work);
    store_aligned: 4 | 2 | 1 (see the header); specialised: with a kernel built for four voices per lane at hand"""
    vpt, span = ctypes.c_int32(0), ctypes.c_int32(0)
    _check(lib().sig_voice_program_geometry(voices, block_frames, nblocks, context, depth, bus_channels, int(store_aligned),
                                            1 if specialised else 0, ctypes.byref(vpt), ctypes.byref(span)), 'sig_voice_program_geometry')
    return vpt.value, span.value


def voice_program_variant(code: list, n_oscs: int, n_params: int, n_filters: int, n_temps: int) -> tuple:
    """(family, small_file): the interpreter variant (a name of VP_VARIANTS) sig_voice_program launches for this program and whether it
    runs in the small register file (introspection, no device work)"""
    P = _program_struct(code)
    P.n_oscs, P.n_params, P.n_filters, P.n_temps = n_oscs, n_params, n_filters, n_temps
    family, small = ctypes.c_int32(-1), ctypes.c_int32(-1)
    _check(lib().sig_voice_program_variant(ctypes.byref(P), ctypes.byref(family), ctypes.byref(small)), 'sig_voice_program_variant')
    return VP_VARIANTS[family.value], bool(small.value)


def voice_program_attach(code: list, n_oscs: int, n_params: int, n_filters: int, n_temps: int, voices_per_lane: int,
                         bus_channels: int, image: bytes) -> None:
    """hand the library a specialised build of voice_program.hip for exactly this program (signals_amd/specialise.py): later
    sig_voice_program calls with the same program, slot counts, voices per lane and sink launch it instead of the interpreter.
    Loads the image, runs its self-description kernel and synchronises: a set-up call, not a render call."""
    P = _program_struct(code)
    P.n_oscs, P.n_params, P.n_filters, P.n_temps = n_oscs, n_params, n_filters, n_temps
    _check(lib().sig_voice_program_attach(ctypes.byref(P), voices_per_lane, bus_channels, image), 'sig_voice_program_attach')


def voice_program_detach_all() -> None:
    _check(lib().sig_voice_program_detach_all(), 'sig_voice_program_detach_all')


def voice_program_use_attached(on: bool) -> None:
    """test hook (process-wide): launch attached specialised kernels (default) or always the interpreter"""
    _check(lib().sig_voice_program_use_attached(1 if on else 0), 'sig_voice_program_use_attached')


def set_voice_program_tuning(voices_per_lane: int = 0, blocks_per_lane: int = 0) -> None:
    """tuning / test hook (process-wide): force `voice_program`'s launch geometry; the defaults restore the heuristic"""
    _check(lib().sig_voice_program_set_tuning(voices_per_lane, blocks_per_lane), 'sig_voice_program_set_tuning')
