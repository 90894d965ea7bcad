"""Case table, float64 restatement and bounds for the per-block-row span walker, fused_walk_kernel<KIND, VPT, GAIN, C, ROWS = true>
(signals_amd/csrc/sig_fused_walk.h) behind sig_fused_osc_biquad_rows / sig_fused_voice_bus_rows (swept cutoff, tremolo),
sig_fused_osc_biquad_fm / sig_fused_voice_bus_fm (block-rate hertz / phase rows) and sig_fused_osc_pair_biquad / sig_fused_voice_pair_bus
(Mix or RingMod of two oscillators in front of the filter): `_native.fused_rows`.  Shared by tests/test_fused_rows_host.py and
tests/test_gpu_fused_rows.py.  numpy only.

A case names a launch: the first oscillator's waveform, the filter type, V voices, K blocks of N frames at `position`, the sink ('store':
float32 rows per voice, `offset` columns into a 16-byte-aligned row; 1 or 2: a bus of that many channels, mono without gains), the source
('swept': one hertz / phase row; 'fm': hertz and / or phase rows per block with the row in front of the launch; 'pair': (op, second
waveform, whether a mix row is handed over)) and the shapes of the four parameter tables: 'KV', '1V', 'K1' or None.

Parameter tables are random per block, not LFOs: cutoffs log-uniform in 60 .. 9000 Hz per (block, voice), gains 0.25 .. 1 of either
sign, hertz rows 55 .. 1760 Hz, phase rows in [0, 1).  `special`: 'far' puts voices 0 .. 63 at 6 .. 9 kHz (past 2^26 cycles at FAR),
'qualify' one voice above rate / 4 in the launch's middle block alone and another in the row in front of the launch alone, 'bad_cutoff'
a cutoff of 0 at one (block, voice).

The restatement (`restate`): block b of the launch is chain_ref.crit_filter, designed with cutoff row b, over the window
[osc(kind, p_b - c0, c0, hertz[b - 1], phase[b - 1]) | osc(kind, p_b, N, hertz[b], phase[b]) | after rows], p_b = position + b N,
c0 = min(p_b, CTX), times gain row b; row -1 of a table is the row in front of the launch, a table without one answers its row 0
there.  A paired source is chain_ref.mix / chain_ref.ringmod of that oscillator and a second one.  The bus is chain_ref.sum_bus.

`model` is the kernel's schedule restated in numpy float64 (the b0-normalised recurrence, designs and weights by block, spans): with
nothing wrong it equals the restatement to rounding; its `wrong` switch models the WRONG kernels the case table has to catch.  It
never decides pass or fail against the kernel.

Bounds: the outer bar is the project's 1e-6 max(1, max|ref|).  On the store sink, unpaired, |gain| <= 1: the figures
tests/test_gpu_fused_walker.py holds on the same arithmetic -- 2e-7 for the exact-phase waveforms and the Sine recurrence, 3e-7 where
a Sine voice of the case leaves the recurrence (its wave then takes the float32 sine of the exact phase)."""
import collections
import functools
import math
import zlib

import numpy as np

from oracle import chain_ref as R

RATE = 48000
CTX = R.CONTEXT_FRAMES
FAR = 4 * 172_800_000
SENTINEL = -777.0
SINE_FAST_MAX_CYCLES = 2.0 ** 26
BAD_CUTOFF = 1                                     # SIG_STATUS_BAD_CUTOFF
KINDS = ('Sine', 'Square', 'Sawtooth', 'Triangle')
# (voices per lane, blocks per lane) of tests/test_gpu_fused_walker.py without the 8 voices per lane only the closed form has
GEOMETRIES = ((1, 1), (2, 1), (4, 1), (4, 2), (2, 4), (1, 8), (4, 8), (2, 3))
STEADY_GEOMETRIES = ((0, 0), (8, 4), (8, 1), (2, 3))       # closed_form = 1: fused_steady_bus_kernel<.., GROWS / CROWS>
LAUNCH_CAP = 16                                    # launches of one test (of one case of a parametrised one)
DISCRIMINATION = 1e-3                              # of max|ref|: what rolling a K-row table by one row moves the restatement at least
MISS = 100.0                                       # a wrong kernel misses the outer bar by this factor at least

Case = collections.namedtuple('Case', 'name kind btype V N K position sink source cutoff gain hertz phase offset special')


def case(name, kind, btype, V, N, K, position, sink, source, cutoff, gain, hertz='1V', phase='1V', offset=0, special=None) -> Case:
    return Case(name, kind, btype, V, N, K, position, sink, source, cutoff, gain, hertz, phase, offset, special)


MIX, RING = 'Mix', 'RingMod'
AXES = dict(kind=KINDS, btype=('lp', 'hp'), V=(64, 67, 130, 200), N=(64, 100, 101, 256, 356), K=(1, 5, 9), position=(0, 37, 100, 5000, FAR),
            sink=('store', 1, 2), cutoff=('KV', '1V', 'K1'), gain=('KV', '1V', 'K1', None), hertz=('KV', '1V', 'K1'), phase=('KV', '1V'),
            offset=(0, 1, 2), special=(None, 'far', 'qualify', 'bad_cutoff'))

CASES = (
    # swept cutoff and tremolo (sig_fused_osc_biquad_rows / sig_fused_voice_bus_rows)
    case('swept_sine_lp_store', 'Sine', 'lp', 200, 256, 5, 37, 'store', 'swept', 'KV', '1V'),
    case('swept_saw_hp_store_gain_rows', 'Sawtooth', 'hp', 200, 256, 5, 100, 'store', 'swept', '1V', 'KV', offset=1),
    case('swept_square_hp_bus2', 'Square', 'hp', 200, 256, 5, 5000, 2, 'swept', 'KV', 'KV'),
    case('swept_tri_lp_mono_no_gain', 'Triangle', 'lp', 67, 256, 5, 0, 1, 'swept', 'KV', None),
    case('swept_saw_lp_store_v67', 'Sawtooth', 'lp', 67, 101, 5, 0, 'store', 'swept', 'KV', 'KV'),
    case('swept_tri_hp_store_v130_columns', 'Triangle', 'hp', 130, 356, 5, 37, 'store', 'swept', 'K1', 'K1'),
    case('swept_sine_hp_store_all_tail', 'Sine', 'hp', 64, 100, 5, 100, 'store', 'swept', 'KV', 'KV', offset=2),
    case('swept_square_lp_store_short', 'Square', 'lp', 64, 64, 5, 37, 'store', 'swept', 'KV', '1V'),
    case('swept_sine_lp_bus2_short', 'Sine', 'lp', 67, 64, 5, 0, 2, 'swept', 'KV', 'KV'),
    case('swept_sine_lp_store_far', 'Sine', 'lp', 130, 256, 5, FAR, 'store', 'swept', 'KV', '1V', special='far'),
    case('swept_saw_lp_bus2_k9', 'Sawtooth', 'lp', 64, 101, 9, 5000, 2, 'swept', 'KV', 'K1'),
    case('swept_tri_hp_bus2_n356', 'Triangle', 'hp', 200, 356, 5, FAR, 2, 'swept', '1V', 'KV'),
    case('swept_sine_hp_mono_tremolo', 'Sine', 'hp', 130, 256, 5, 5000, 1, 'swept', '1V', 'KV'),
    case('swept_sine_lp_bus2_both', 'Sine', 'lp', 200, 101, 5, 37, 2, 'swept', 'KV', 'KV'),
    case('swept_sine_hp_mono_cutoff', 'Sine', 'hp', 64, 100, 5, 0, 1, 'swept', 'KV', None),
    case('swept_bad_cutoff', 'Sawtooth', 'lp', 67, 256, 5, 37, 'store', 'swept', 'KV', '1V', special='bad_cutoff'),
    case('swept_one_row_store', 'Sawtooth', 'lp', 64, 256, 5, 37, 'store', 'swept', '1V', '1V'),
    case('swept_one_row_sine_store', 'Sine', 'hp', 200, 101, 5, 5000, 'store', 'swept', '1V', '1V'),
    case('swept_one_row_bus2', 'Sine', 'lp', 130, 256, 5, 37, 2, 'swept', '1V', '1V'),
    case('swept_one_row_mono', 'Triangle', 'hp', 67, 100, 5, 100, 1, 'swept', '1V', None),
    # block-rate FM (sig_fused_osc_biquad_fm / sig_fused_voice_bus_fm): N >= CTX, the kernel's contract
    case('fm_sine_lp_store', 'Sine', 'lp', 200, 256, 5, 37, 'store', 'fm', '1V', '1V', 'KV', 'KV'),
    case('fm_sine_hp_bus2_swept', 'Sine', 'hp', 200, 256, 5, 5000, 2, 'fm', 'KV', 'KV', 'KV', '1V'),
    case('fm_saw_lp_store_phase_rows', 'Sawtooth', 'lp', 67, 100, 5, 37, 'store', 'fm', '1V', None, '1V', 'KV'),
    case('fm_square_hp_mono_columns', 'Square', 'hp', 130, 101, 5, 100, 1, 'fm', 'K1', 'K1', 'K1', '1V'),
    case('fm_tri_lp_store_from_zero', 'Triangle', 'lp', 64, 356, 5, 0, 'store', 'fm', 'KV', '1V', 'KV', 'KV', offset=1),
    case('fm_sine_lp_store_far', 'Sine', 'lp', 130, 256, 5, FAR, 'store', 'fm', '1V', '1V', 'KV', 'KV', special='far'),
    case('fm_sine_lp_store_qualify', 'Sine', 'lp', 200, 256, 5, 5000, 'store', 'fm', '1V', '1V', 'KV', '1V', special='qualify'),
    case('fm_sine_hp_bus2_qualify', 'Sine', 'hp', 200, 101, 5, 37, 2, 'fm', '1V', 'KV', 'KV', 'KV', special='qualify'),
    case('fm_sine_lp_bus2_k9', 'Sine', 'lp', 64, 100, 9, 100, 2, 'fm', '1V', '1V', 'KV', 'KV'),
    case('fm_saw_hp_store_one_block', 'Sawtooth', 'hp', 64, 256, 1, 5000, 'store', 'fm', '1V', '1V', 'KV', 'KV'),
    case('fm_tri_hp_bus2_n356', 'Triangle', 'hp', 67, 356, 5, 100, 2, 'fm', 'KV', '1V', 'KV', 'KV'),
    case('fm_square_lp_store_all_tail', 'Square', 'lp', 130, 100, 5, 0, 'store', 'fm', 'KV', 'KV', '1V', 'KV'),
    case('fm_sine_hp_store_n101', 'Sine', 'hp', 64, 101, 5, 37, 'store', 'fm', '1V', '1V', 'KV', 'KV', offset=2),
    # two oscillators through Mix or RingMod (sig_fused_osc_pair_biquad / sig_fused_voice_pair_bus); False: no mix row handed over
    case('pair_mix_sine_sine', 'Sine', 'lp', 200, 256, 5, 37, 'store', (MIX, 'Sine', True), '1V', '1V'),
    case('pair_mix_saw_square', 'Sawtooth', 'hp', 67, 100, 5, 0, 2, (MIX, 'Square', True), '1V', '1V'),
    case('pair_mix_square_saw', 'Square', 'lp', 130, 101, 5, 100, 'store', (MIX, 'Sawtooth', True), '1V', None),
    case('pair_mix_tri_tri', 'Triangle', 'hp', 64, 356, 5, 5000, 1, (MIX, 'Triangle', True), '1V', '1V'),
    case('pair_ring_sine_saw_short', 'Sine', 'lp', 200, 64, 5, 37, 'store', (RING, 'Sawtooth', True), '1V', '1V', offset=1),
    case('pair_ring_saw_sine_no_mix', 'Sawtooth', 'hp', 64, 256, 5, FAR, 'store', (RING, 'Sine', False), '1V', '1V'),
    case('pair_ring_tri_square_swept', 'Triangle', 'lp', 130, 256, 5, 5000, 2, (RING, 'Square', True), 'KV', 'KV'),
    case('pair_ring_square_tri', 'Square', 'hp', 67, 101, 5, 100, 1, (RING, 'Triangle', False), '1V', None),
    case('pair_mix_sine_tri_far', 'Sine', 'lp', 130, 256, 5, FAR, 'store', (MIX, 'Triangle', True), 'KV', '1V', special='far'),
    case('pair_mix_sine_square_swept', 'Sine', 'hp', 200, 356, 5, 0, 2, (MIX, 'Square', True), 'KV', '1V'),
)
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

BAD_AT = (2, 40)                                   # (block, voice) of the 'bad_cutoff' case
QUALIFY_MIDDLE, QUALIFY_FRONT = 3, 140             # 'qualify': the voices above rate / 4 in the middle block alone / in the row in front alone


def is_pair(c: Case) -> bool:
    return isinstance(c.source, tuple)


def is_fm(c: Case) -> bool:
    return c.source == 'fm'


def channels_of(c: Case) -> int:
    return c.V if c.sink == 'store' else c.sink


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# --------------------------------------------------------------------------------------------------------------------- inputs
Inputs = collections.namedtuple('Inputs', 'hertz hertz_hist phase phase_hist cutoff gain pan hertz2 phase2 mix')
TABLES = ('hertz', 'phase', 'cutoff', 'gain')
DRAW = dict(cutoff=lambda rng, shape: np.exp(rng.uniform(np.log(60.0), np.log(9000.0), shape)),
            gain=lambda rng, shape: rng.uniform(0.25, 1.0, shape) * rng.choice([-1.0, 1.0], shape),
            hertz=lambda rng, shape: rng.uniform(55.0, 1760.0, shape),
            phase=lambda rng, shape: rng.uniform(0.0, 1.0, shape))


def table_shape(code: str, K: int, V: int) -> tuple:
    return (K if code[0] == 'K' else 1, V if code[1] == 'V' else 1)


def inputs_of(c: Case, seed: int = 0) -> Inputs:
    rng = rng_of('fused_rows', c.name, seed)
    t = {k: (None if getattr(c, k) is None else DRAW[k](rng, table_shape(getattr(c, k), c.K, c.V))) for k in TABLES}
    hist = {k: (DRAW[k](rng, (1, t[k].shape[1])) if is_fm(c) and getattr(c, k)[0] == 'K' else None) for k in ('hertz', 'phase')}
    if c.special == 'far':
        for a in (t['hertz'], hist['hertz']):
            if a is not None:
                a[:, :64] = rng.uniform(6000.0, 9000.0, (a.shape[0], 64))
    if c.special == 'qualify':
        t['hertz'][c.K // 2, QUALIFY_MIDDLE] = 13000.0
        hist['hertz'][0, QUALIFY_FRONT] = 15000.0
    if c.special == 'bad_cutoff':
        t['cutoff'][BAD_AT] = 0.0
    pan = None
    if c.sink == 2:
        th = rng.uniform(0.3, np.pi / 2 - 0.3, c.V)
        pan = np.stack([np.cos(th), np.sin(th)])
    hertz2 = phase2 = mix = None
    if is_pair(c):
        hertz2, phase2 = DRAW['hertz'](rng, (1, c.V)), DRAW['phase'](rng, (1, c.V))
        mix = rng.uniform(0.2, 0.8, (1, c.V)) if c.source[2] else None
    return Inputs(t['hertz'], hist['hertz'], t['phase'], hist['phase'], t['cutoff'], t['gain'], pan, hertz2, phase2, mix)


def row_of(table, front, b: int, V: int) -> np.ndarray:
    """(1, V): row b of a table, broadcast to V voices; b = -1: the row in front of the launch, where the table has one"""
    if b < 0 and front is not None:
        return np.broadcast_to(front, (1, V))
    return np.broadcast_to(table[b if table.shape[0] > 1 else 0], (1, V))


def source_rows(c: Case, I: Inputs, b: int, position: int, frames: int) -> np.ndarray:
    """(frames, V) float64: the filter's input from `position` on, made with hertz / phase row b"""
    x = R.osc(c.kind, position, frames, RATE, row_of(I.hertz, I.hertz_hist, b, c.V), row_of(I.phase, I.phase_hist, b, c.V))
    if is_pair(c):
        y = R.osc(c.source[1], position, frames, RATE, I.hertz2, I.phase2)
        x = R.mix(x, y, I.mix) if c.source[0] == MIX else R.ringmod(x, y)       # (RingMod reads no mix row)
    return np.broadcast_to(x, (frames, c.V))


def valid_cutoff(row: np.ndarray) -> np.ndarray:
    return (row > 0.0) & (row < RATE / 2.0)


def restate(c: Case, I: Inputs) -> np.ndarray:
    """(K N, V) float64 per voice, every block cold-started c0 rows early; a voice with a cutoff outside (0, rate / 2) in block b is
    NaN over that block (the reference raises there; the kernel flags the status word)"""
    out = np.empty((c.K * c.N, c.V))
    after = np.zeros((CTX, c.V))                                                # (no kept sample depends on the rows behind the block)
    for b in range(c.K):
        p = c.position + b * c.N
        c0 = min(p, CTX)
        window = np.concatenate([source_rows(c, I, b - 1, p - c0, c0), source_rows(c, I, b, p, c.N), after])
        cutoff = row_of(I.cutoff, None, b, c.V)
        ok = valid_cutoff(cutoff[0])
        y = R.crit_filter(c.btype, window, np.where(ok, cutoff, 1000.0), RATE, c.N, CTX)
        if I.gain is not None:
            y = R.gain(y, row_of(I.gain, None, b, c.V))
        y[:, ~ok] = np.nan
        out[b * c.N:(b + 1) * c.N] = y
    return out


def to_sink(c: Case, I: Inputs, per_voice: np.ndarray) -> np.ndarray:
    return per_voice if c.sink == 'store' else R.sum_bus(per_voice, I.pan)


Built = collections.namedtuple('Built', 'case inputs per_voice ref')


@functools.lru_cache(maxsize=None)
def build(name: str) -> Built:
    """the inputs and the float64 reference of a case, computed once and shared (read-only)"""
    c = BY_NAME[name]
    I = inputs_of(c)
    per_voice = restate(c, I)
    ref = to_sink(c, I, per_voice)
    for a in tuple(I) + (per_voice, ref):
        if a is not None:
            a.setflags(write=False)
    return Built(c, I, per_voice, ref)


# --------------------------------------------------------------------------------------------------------------------- bounds
def outer_bar(ref: np.ndarray) -> float:
    """the project's bar (gpu_helpers.tolerance): 1e-6 of full scale, never below 1e-6"""
    return 1e-6 * max(1.0, float(np.nanmax(np.abs(ref))))


def all_fast(c: Case, I: Inputs) -> bool:
    """whether every Sine voice of the launch qualifies for the recurrence in every row (sig_fused_walk.h seed_sine): below 2^26
    cycles over the launch, at most a quarter turn per row after aliasing, the row in front of the launch included"""
    rows = [I.hertz] + ([I.hertz_hist] if I.hertz_hist is not None else [])
    phases = [I.phase] + ([I.phase_hist] if I.phase_hist is not None else [])
    hz = np.concatenate([np.broadcast_to(r, (r.shape[0], c.V)) for r in rows])
    d = hz / RATE
    t = (c.position + c.K * c.N) / RATE * np.abs(hz).max() + max(float(np.abs(p).max()) for p in phases)
    return bool((np.abs(d - np.rint(d)) <= 0.25).all() and t < SINE_FAST_MAX_CYCLES)


def tight_bound(c: Case, I: Inputs):
    """the bound below the outer bar, or None: store sink, unpaired, |gain| <= 1 (see the module docstring)"""
    if c.sink != 'store' or is_pair(c):
        return None
    assert I.gain is None or np.abs(I.gain).max() <= 1.0
    return 3e-7 if c.kind == 'Sine' and not all_fast(c, I) else 2e-7


def leg_of(c: Case, I: Inputs) -> str:
    """the row of the measured figures a case belongs to"""
    if c.sink != 'store':
        return f'bus C = {c.sink}'
    if is_pair(c):
        return 'store, paired'
    if c.kind != 'Sine':
        return 'store, exact phase'
    if all_fast(c, I):
        return 'store, fast Sine'
    return 'store, Sine on the exact phase under FM' if is_fm(c) else 'store, Sine on the exact phase'


# ----------------------------------------------------------------------------------------------------- what a launch is given
def store_vpt(c: Case, vpt: int) -> int:
    """voices per lane of the store sink (sig_fused_launch.h launch_rows): the largest of 4, 2, 1 not above the forced one that divides
    the voices, the leading dimension (a multiple of 4 in the GPU test) and the view's offset in columns"""
    top = 4
    while top > 1 and (c.V % top or c.offset % top):
        top >>= 1
    return min(vpt, top)


def effective(c: Case, geometry: tuple) -> tuple:
    """(voices per lane, blocks per lane) the walker runs a case with under a forced geometry: blocks shorter than the context do not
    span; the store sink falls back on alignment"""
    vpt, span = geometry
    return (store_vpt(c, vpt) if c.sink == 'store' else vpt), (span if c.N >= CTX else 1)


def k_row_tables(c: Case) -> tuple:
    return tuple(k for k in TABLES if getattr(c, k) is not None and getattr(c, k)[0] == 'K' and c.K > 1)


# ------------------------------------------------------------------------------------- the kernel's schedule, right and wrong
WRONG = ('warm_up_design', 'weights_late', 'front_row', 'row_in_span', 'no_reseed', 'dead_lane', 'column_stride')


def design(btype: str, cutoff: np.ndarray) -> tuple:
    """(b0, a1, a2) of chain_ref.butter2_sos for a row of cutoffs; NaN outside (0, rate / 2)"""
    wn = np.where(valid_cutoff(cutoff), cutoff, np.nan) / (RATE / 2.0)
    k = np.tan(np.pi * wn / 2.0)
    k2 = k * k
    nrm = 1.0 / (1.0 + math.sqrt(2.0) * k + k2)
    return (k2 * nrm if btype == 'lp' else nrm), 2.0 * (k2 - 1.0) * nrm, (1.0 - math.sqrt(2.0) * k + k2) * nrm


def normalised(btype: str, x: np.ndarray, warm: tuple, out: tuple, c0: int) -> np.ndarray:
    """rows c0 .. of y / b0 for the transposed direct form II of [1, +-2, 1] / [1, a1, a2] from zero state over x, the first c0 rows
    under the design `warm`, the others under `out`"""
    s2 = 2.0 if btype == 'lp' else -2.0
    z0, z1 = np.zeros(x.shape[1]), np.zeros(x.shape[1])
    y = np.empty((x.shape[0] - c0, x.shape[1]))
    _, a1, a2 = warm
    for r in range(x.shape[0]):
        if r == c0:
            _, a1, a2 = out
        yn = x[r] + z0
        z0 = s2 * x[r] - a1 * yn + z1
        z1 = x[r] - a2 * yn
        if r >= c0:
            y[r - c0] = yn
    return y


def model(c: Case, I: Inputs, geometry: tuple = (1, 1), wrong: str | None = None) -> np.ndarray:
    """the sink's float64 output as the walker schedules it under `geometry`; `wrong`:
      warm_up_design  the next block's warm-up chain designed with the current block's cutoff
      weights_late    the output weights (b0, gain) swapped one block late
      front_row       row 0 of the FM tables in place of the row in front of the launch
      row_in_span     the FM row indexed by the block's number within the span, not within the launch
      no_reseed       the Sine recurrence not seeded again at a block boundary under FM (the span keeps its first seed's row)
      dead_lane       a dead lane keeps the bus weight of the voice it shadows
      column_stride   a one-column table read with stride `voices` (rows 1 .. lie outside the table: NaN guards)"""
    assert wrong is None or wrong in WRONG
    vpt, span = effective(c, geometry)
    out = np.empty((c.K * c.N, c.V))
    nan_row = np.full((1, c.V), np.nan)

    def rows(name, b):
        table, front = getattr(I, name), (getattr(I, name + '_hist') if name in ('hertz', 'phase') else None)
        if wrong == 'front_row' and b < 0:
            b = 0
        if wrong == 'column_stride' and table.shape[0] > 1 and table.shape[1] == 1 and b > 0:
            return nan_row
        return row_of(table, front, b, c.V)

    def src(b, position, frames):
        shadow = I._replace(hertz=rows('hertz', b), phase=rows('phase', b), hertz_hist=None, phase_hist=None)
        return source_rows(c, shadow, 0, position, frames)

    for b in range(c.K):
        first = b - b % span
        p = c.position + b * c.N
        c0 = min(p, CTX)
        r_warm, r_out, c_warm, w = b - 1, b, b, b
        if wrong == 'warm_up_design' and b != first:
            c_warm = b - 1
        if wrong == 'weights_late' and b != first:
            w = b - 1
        if wrong == 'row_in_span' and is_fm(c):
            r_out, r_warm = b - first, b - first - 1
        if wrong == 'no_reseed' and is_fm(c):
            r_out = r_warm = first - 1
        x = np.concatenate([src(r_warm, p - c0, c0), src(r_out, p, c.N)])
        y = normalised(c.btype, x, design(c.btype, rows('cutoff', c_warm)[0]), design(c.btype, rows('cutoff', b)[0]), c0)
        weight = design(c.btype, rows('cutoff', w)[0])[0]
        if I.gain is not None:
            weight = weight * rows('gain', w)[0]
        out[b * c.N:(b + 1) * c.N] = y * weight
    got = to_sink(c, I, out)
    if wrong == 'dead_lane' and c.sink != 'store':
        lanes = -(-c.V // (64 * vpt)) * 64
        for lane in range(lanes):
            v0 = lane * vpt
            shadowed = v0 if v0 < c.V else 0
            dead = sum(1 for i in range(vpt) if v0 + i >= c.V)
            if dead:
                got = got + dead * (out[:, shadowed:shadowed + 1] * (1.0 if I.pan is None else I.pan[:, shadowed][None, :]))
    return got


def applies(wrong: str, c: Case, geometry: tuple) -> bool:
    """the (case, geometry) legs a wrong kernel cannot pass: where its fault is reached and the tables differ from row to row"""
    vpt, span = effective(c, geometry)
    tables = k_row_tables(c)
    if wrong == 'warm_up_design':
        return 'cutoff' in tables and span > 1
    if wrong == 'weights_late':
        return ('cutoff' in tables or 'gain' in tables) and span > 1
    if wrong == 'front_row':
        return is_fm(c) and c.position > 0
    if wrong == 'row_in_span':
        return is_fm(c) and span < c.K
    if wrong == 'no_reseed':
        return is_fm(c) and c.kind == 'Sine' and c.special is None
    if wrong == 'dead_lane':
        return c.sink != 'store' and c.V % (64 * vpt) != 0
    return any(getattr(c, k) == 'K1' for k in TABLES) and c.K > 1


def misses(got: np.ndarray, ref: np.ndarray) -> bool:
    """whether `got` misses the outer bar by MISS at least: a sample that far off, or one that is not finite where the reference is"""
    finite = np.isfinite(ref)
    if not np.isfinite(got[finite]).all():
        return True
    return bool(np.abs(got[finite] - ref[finite]).max() >= MISS * outer_bar(ref))


# --------------------------------------------------------------------------------- what tests/test_gpu_fused_rows.py launches
BATCHING = ('swept_saw_hp_store_gain_rows', 'swept_sine_lp_store', 'fm_tri_lp_store_from_zero', 'fm_sine_lp_store', 'fm_square_hp_mono_columns',
            'pair_ring_tri_square_swept')                                       # K blocks in one call against K calls of one block
ONE_ROW = ('swept_one_row_store', 'swept_one_row_sine_store', 'swept_one_row_bus2', 'swept_one_row_mono')   # one-row tables: K identical rows, the plain entry
STEADY = ('swept_sine_hp_mono_tremolo', 'swept_sine_lp_bus2_both', 'swept_sine_hp_mono_cutoff', 'swept_sine_lp_bus2_short')   # closed_form = 1
STATUS_CASE = 'swept_bad_cutoff'
REFUSALS = ('FM and a second oscillator', 'cutoff rows neither 1 nor K', 'gain rows neither 1 nor K', 'hertz_hist of the wrong width',
            'phase rows without phase_hist', 'FM below the context', 'Mix without a mix row', 'a bus of four channels')


def launches() -> dict:
    """launches per test of tests/test_gpu_fused_rows.py (of one case of a parametrised one), against LAUNCH_CAP"""
    return {'cases': len(GEOMETRIES), 'batching': 2 + max(BY_NAME[n].K for n in BATCHING), 'one row': 2 * 3 + 3, 'steady': len(STEADY_GEOMETRIES),
            'status': 2 * 2 + 1, 'refusals': 1}
