"""Case table, float64 restatement and bounds for the filter-and-bus pass (signals_amd/csrc/biquad_bus.hip: sig_biquad_coldstart_bus,
out = SumBus(Filter(x)) or SumBus(RingMod(Filter(x), ADSR)) in one pass over a materialised x), shared by tests/test_bus_pass_host.py
and tests/test_gpu_bus_pass.py.  numpy only.

A case names a launch: V voices, K blocks of N frames at `position` under `context` rows of cold start, a bus of C channels ('mono': one
channel without gains), the extra columns of the gains' and of out's leading dimension, the layout of x (`view(array, pad, ld_extra)` of
tests/base_kernel_cases.py: contig and pad4 keep the 16-byte rows of four voices per lane, pad1 and ld1 force one voice per lane), the
shape of the cutoff rows -- row (1, V), one (1, 1), blocks (K, V), blocks_one (K, 1), the per-block rows differing from block to block --,
the filter type and the envelope: None, or how the six ADSR parameters are laid out -- rows: six (1, V) rows; mixed: decay and
sustain (1, 1); mixed2: attack and release (1, 1); one: all six (1, 1).

Inputs are float32-exact, uniform in +-0.25, cutoffs uniform in 200 .. 8000 Hz (a voice that its cutoff leaves inaudible over a short
window draws again), pans cos / sin of angles that keep both above 0.29.  The restatement is, per block, oracle.chain_ref's
crit_filter over the block's window [min(context, position + b N) rows | block], times chain_ref.adsr, then chain_ref.sum_bus.  The same
recurrence once more in np.longdouble (`filter_longdouble`: the butter(2) design and the transposed direct form II step) measures
what the float64 roundings of the recurrence move a sample; it enters the bound alone, never the reference.

Envelope voices: hand-placed ones whose attack, decay, gate-off and release ends fall on the first output row of a block, on the first
and the last row of a chunk of 8 and of 16 window rows and on window rows 63, 64 and 65 (where the kernel refreshes its per-lane
times), in front of the rows of tests/envelopes.py `table(position, N, K)` (edge cases first), cut to V.  A voice that is silent over
the rendered rows is left out while the rows are chosen: every voice of every case contributes at least CONTRIBUTION of max|ref| to
some channel, so that a dropped voice cannot hide under the bound, and max|ref| exceeds FULL_SCALE.

`expected_variant` restates the dispatch of biquad_bus.hip (vec_ok, ring and chunk, voice tiles, which blocks have ragged front or end
row groups): a census for the host test, it never decides pass or fail against the kernel."""
import collections
import functools
import zlib

import numpy as np

import envelopes as E
from base_kernel_cases import LAYOUT, View, f32, ld, view
from oracle import chain_ref as R

RATE = 48000
HOUR = E.HOUR
FAR = 2 ** 31 + 5
SENTINEL = -777.0
CONTRIBUTION = 1e-3            # of max|ref|, per voice, in some channel
FULL_SCALE = 0.1               # max|ref| exceeds this
LAUNCH_CAP = 200
PARAMS = E.PARAMS
BAD_CUTOFF = 1                 # SIG_STATUS_BAD_CUTOFF

Case = collections.namedtuple('Case', 'name V N K context position C gains_extra out_extra layout cutoff btype env seed')


def case(name, V, N, K, context, position, C, layout, cutoff, btype, env=None, gains_extra=0, out_extra=0, seed=0) -> Case:
    return Case(name, V, N, K, context, position, C, gains_extra, out_extra, layout, cutoff, btype, env, seed)


AXES = dict(V=(1, 3, 4, 63, 64, 65, 252, 256, 257, 260, 1028), N=(1, 3, 15, 16, 17, 33, 100, 101, 130), K=(1, 2, 5), context=(0, 6, 100),
            position=(0, 37, 100, 1000, HOUR, FAR), C=('mono', 1, 2, 4), gains_extra=(0, 3), out_extra=(0, 3),
            layout=('contig', 'pad4', 'pad1', 'ld1'), cutoff=('row', 'one', 'blocks', 'blocks_one'), btype=('lp', 'hp'),
            env=(None, 'rows', 'mixed', 'mixed2', 'one'))

# drawn by hand as a sparse crossing of AXES: every value of every axis, every kernel instantiation (voices per lane x envelope x C),
# and the row-group edges of `expected_variant`.  The short low-pass windows go with many voices, the one- and three-voice cases with
# the high-pass, so that FULL_SCALE and CONTRIBUTION hold
CASES = (
    # four voices per lane, no envelope (ring 16; chunks of 16 rows)
    case('v4_one_group', 4, 16, 1, 0, 0, 1, 'contig', 'row', 'hp'),
    case('v4_ragged_front_c2', 64, 17, 2, 6, 37, 2, 'pad4', 'blocks', 'lp', gains_extra=3, out_extra=3),
    case('v4_dead_lane_c4', 252, 33, 2, 100, 1000, 4, 'contig', 'one', 'lp'),
    case('v4_full_tile_mono', 256, 100, 1, 100, HOUR, 'mono', 'pad4', 'row', 'hp'),
    case('v4_ragged_front_c4', 260, 15, 5, 6, 0, 4, 'contig', 'blocks_one', 'lp', gains_extra=3),
    case('v4_short_blocks', 1028, 3, 2, 100, FAR, 2, 'contig', 'row', 'hp', out_extra=3),
    case('v4_one_frame', 64, 1, 5, 100, 100, 1, 'pad4', 'blocks', 'hp'),
    case('v4_position_in_context', 256, 130, 2, 100, 37, 2, 'contig', 'row', 'lp'),
    case('v4_no_context_c4', 4, 101, 1, 0, 1000, 4, 'pad4', 'one', 'hp', out_extra=3),
    case('v4_two_tiles_mono', 260, 16, 1, 6, 100, 'mono', 'contig', 'row', 'lp'),
    case('v4_growing_context', 252, 17, 5, 100, 0, 1, 'pad4', 'blocks_one', 'lp', gains_extra=3),
    case('v4_five_tiles_c4', 1028, 33, 1, 6, 1000, 4, 'contig', 'row', 'lp', gains_extra=3, out_extra=3),
    case('v4_far_c2', 64, 100, 2, 100, FAR, 2, 'contig', 'blocks', 'lp'),
    case('v4_hour_c4', 256, 15, 2, 100, HOUR, 4, 'pad4', 'row', 'lp'),
    # one voice per lane, no envelope
    case('v1_one_sample', 1, 1, 1, 0, 0, 'mono', 'contig', 'one', 'hp', seed=2),      # (a lone sample above FULL_SCALE)
    case('v1_one_voice', 1, 17, 2, 6, 37, 1, 'ld1', 'row', 'hp', gains_extra=3),
    case('v1_three_voices', 3, 3, 5, 100, 1000, 2, 'pad1', 'blocks', 'hp'),
    case('v1_three_voices_c4', 3, 100, 1, 100, 100, 4, 'contig', 'row', 'hp', out_extra=3),
    case('v1_ragged_front_c4', 63, 15, 2, 6, 0, 4, 'contig', 'blocks_one', 'lp', gains_extra=3),
    case('v1_two_tiles', 65, 16, 1, 100, HOUR, 2, 'ld1', 'row', 'lp'),
    case('v1_five_tiles_far', 257, 33, 2, 0, FAR, 1, 'contig', 'one', 'hp'),
    case('v1_four_tiles_pad1', 256, 100, 1, 100, 1000, 2, 'pad1', 'row', 'lp'),
    case('v1_four_tiles_ld1', 252, 130, 1, 6, 100, 'mono', 'ld1', 'row', 'lp'),
    case('v1_idle_waves', 260, 17, 5, 100, 37, 4, 'pad1', 'blocks', 'lp'),
    case('v1_seventeen_tiles', 1028, 15, 1, 100, 1000, 1, 'pad1', 'row', 'lp', gains_extra=3, out_extra=3),
    case('v1_four_voices', 4, 33, 2, 6, HOUR, 2, 'ld1', 'one', 'hp'),
    case('v1_full_lanes_c4', 64, 101, 2, 100, 0, 4, 'pad1', 'blocks_one', 'lp', gains_extra=3),
    case('v1_one_frame', 63, 1, 5, 100, FAR, 'mono', 'contig', 'row', 'hp'),
    # four voices per lane under an envelope (ring 8; chunks of 16 rows at C = 1, of 8 at C = 2 and 4)
    case('e4_c1', 64, 16, 2, 100, 1000, 1, 'contig', 'row', 'lp', env='rows'),
    case('e4_c2_hour', 256, 33, 2, 100, HOUR, 2, 'pad4', 'row', 'lp', env='mixed', gains_extra=3),
    case('e4_c4_refresh', 260, 100, 1, 6, 37, 4, 'contig', 'blocks', 'lp', env='rows', out_extra=3),
    case('e4_mono_from_zero', 252, 130, 2, 100, 0, 'mono', 'contig', 'one', 'hp', env='mixed2'),
    case('e4_c2_far', 64, 17, 5, 100, FAR, 2, 'contig', 'blocks_one', 'hp', env='rows'),
    case('e4_c4_five_tiles', 1028, 101, 1, 100, 100, 4, 'pad4', 'row', 'lp', env='mixed', gains_extra=3),
    case('e4_c1_one_envelope', 256, 15, 2, 0, 0, 1, 'contig', 'row', 'hp', env='one'),
    case('e4_c2_refresh', 64, 130, 1, 100, 37, 2, 'pad4', 'row', 'hp', env='rows'),
    case('e4_c4_short', 4, 3, 5, 6, 1000, 4, 'contig', 'row', 'hp', env='rows'),
    # one voice per lane under an envelope (ring 16; chunks of 16 rows)
    case('e1_c1', 65, 16, 2, 100, 1000, 1, 'ld1', 'row', 'lp', env='rows'),
    case('e1_c2_hour', 63, 33, 1, 6, HOUR, 2, 'contig', 'row', 'hp', env='mixed'),
    case('e1_c4', 257, 100, 2, 100, 37, 4, 'contig', 'blocks', 'lp', env='rows', gains_extra=3, out_extra=3),
    case('e1_mono_from_zero', 256, 130, 1, 100, 0, 'mono', 'pad1', 'row', 'lp', env='mixed2'),
    case('e1_c2_one_envelope', 3, 17, 5, 100, 100, 2, 'pad1', 'one', 'hp', env='one'),
    case('e1_c4_far', 260, 101, 1, 100, FAR, 4, 'ld1', 'row', 'lp', env='rows'),
    case('e1_one_voice', 1, 100, 1, 0, 0, 1, 'contig', 'one', 'hp', env='rows'),
    case('e1_seventeen_tiles', 1028, 15, 2, 100, 1000, 1, 'ld1', 'row', 'lp', env='mixed', out_extra=3),
)
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def channels_of(c: Case) -> int:
    return 1 if c.C == 'mono' else c.C


def history_of(c: Case) -> int:
    return min(c.context, c.position)


def block_context(c: Case, b: int) -> int:
    """the context rows of block b: BlockLoc.before, min(context, position + b N)"""
    return min(c.context, c.position + b * c.N)


# ---------------------------------------------------------------------------------------------------------------- restatement
def cutoff_rows(c: Case, rng) -> np.ndarray:
    rows = c.K if c.cutoff.startswith('blocks') else 1
    return rng.uniform(200.0, 8000.0, (rows, 1 if c.cutoff in ('one', 'blocks_one') else c.V))


def filter_blocks(btype, x, hist, N, K, context, position, cutoff, rate=RATE) -> np.ndarray:
    """(K N, V) float64: per block, chain_ref.crit_filter over [min(context, position + b N) rows | block] from zero state; `x` holds
    `hist` rows in front of the K N rows, `cutoff` (1 | K, 1 | V).  (crit_filter keeps [-(frames + ctx):-ctx], so the `after` rows it is
    given are a row of zeros at least: no sample of the block depends on them)"""
    V = x.shape[1]
    after = max(context, 1)
    out = np.empty((N * K, V))
    for b in range(K):
        start = hist + b * N
        c0 = min(context, position + b * N)
        window = np.concatenate([x[start - c0:start + N], np.zeros((after, V))])
        row = np.broadcast_to(cutoff[b if cutoff.shape[0] > 1 else 0][None, :], (1, V))
        out[b * N:(b + 1) * N] = R.crit_filter(btype, window, row, rate, N, after)
    return out


def filter_longdouble(btype, x, hist, N, K, context, position, cutoff, rate=RATE) -> np.ndarray:
    """`filter_blocks` in np.longdouble, all voices of a row at once: the closed form of butter(2) (chain_ref.butter2_sos) and scipy's
    transposed direct form II step (chain_ref.sosfilt_df2t), every operation rounded once to the longer type"""
    L = np.longdouble
    V = x.shape[1]
    out = np.empty((N * K, V), dtype=L)
    xl = x.astype(L)
    for b in range(K):
        wn = np.broadcast_to(cutoff[b if cutoff.shape[0] > 1 else 0], (V,)).astype(L) / (L(rate) / L(2))
        wn = np.clip(wn, L(0), L(1))
        k = np.tan(L(np.pi) * wn / L(2))                                        # (pi and sqrt2 as the float64 constants of the design)
        k2 = k * k
        nrm = L(1) / (L(1) + L(np.sqrt(2.0)) * k + k2)
        if btype == 'lp':
            b0, b1, b2 = k2 * nrm, L(2) * k2 * nrm, k2 * nrm
        else:
            b0, b1, b2 = nrm, L(-2) * nrm, nrm
        a1, a2 = L(2) * (k2 - L(1)) * nrm, (L(1) - L(np.sqrt(2.0)) * k + k2) * nrm
        start = hist + b * N
        c0 = min(context, position + b * N)
        z0, z1 = np.zeros(V, dtype=L), np.zeros(V, dtype=L)
        for r in range(start - c0, start + N):
            xn = xl[r]
            yn = b0 * xn + z0
            z0 = b1 * xn - a1 * yn + z1
            z1 = b2 * xn - a2 * yn
            if r >= start:
                out[b * N + r - start] = yn
    return out


# ------------------------------------------------------------------------------------------------------------------ envelopes
STAGES = ('attack', 'decay', 'gate_off', 'release')
TARGETS = ('first', 'chunk8_first', 'chunk8_last', 'chunk16_first', 'chunk16_last', 'row63', 'row64', 'row65')
A_FRAMES, D_FRAMES, R_FRAMES, SUSTAIN = 3, 3, 4, 0.5           # the stage lengths the hand-placed voices share
COMMON = {'mixed': ('decay', 'sustain'), 'mixed2': ('attack', 'release'), 'one': PARAMS, 'rows': ()}
Placed = collections.namedtuple('Placed', 'block target stage frame')


def target_rows(c: Case, b: int) -> dict:
    """target name -> window row of block b, for the targets that are output rows of the block"""
    c0, total = block_context(c, b), block_context(c, b) + c.N
    up = lambda m: m * -(-(c0 + 1) // m)                                       # the first multiple of m behind the first output row
    rows = dict(first=c0, chunk8_first=up(8), chunk8_last=up(8) + 7, chunk16_first=up(16), chunk16_last=up(16) + 15, row63=63, row64=64, row65=65)
    return {k: r for k, r in rows.items() if c0 <= r < total}


def _nudge(value, end_of, want):
    """`value` moved by a few units in the last place until end_of(value) == want exactly; None where no neighbour does"""
    for _ in range(64):                                                        # (a step moves the rounded sum by at most one unit of `want`)
        got = end_of(value)
        if got == want:
            return value
        value = np.nextafter(value, np.inf if got < want else -np.inf)
    return None                                                                # (a tie that rounds to even either side of `want`)


def placed_voice(stage: str, frame: int):
    """(attack, decay, sustain, release, gate_on, gate_off) of a voice whose `stage` ends exactly at `frame` / RATE, as sig_adsr.h and
    envelopes.boundaries compute the end: gate_on + attack, + 1 / (1 / decay), gate_off + 1 / (1 / release); gate_off itself"""
    a, d, r, t = A_FRAMES / RATE, D_FRAMES / RATE, R_FRAMES / RATE, frame / RATE
    inv = lambda x: 1.0 / (1.0 / x)
    if stage == 'attack':
        on = _nudge(t - a, lambda v: v + a, t)
        return None if on is None else (a, d, SUSTAIN, r, on, on + 40 / RATE)
    if stage == 'decay':
        on = _nudge(t - a - d, lambda v: v + a + inv(d), t)
        return None if on is None else (a, d, SUSTAIN, r, on, on + 40 / RATE)
    if stage == 'gate_off':
        return (a, d, SUSTAIN, r, t - 12 / RATE, t)
    off = _nudge(t - r, lambda v: v + inv(r), t)
    return None if off is None else (a, d, SUSTAIN, r, off - 12 / RATE, off)


def envelope_candidates(c: Case):
    """((n, 6) parameter rows, the Placed of each hand-placed row): the hand-placed voices of blocks 0, 1 and K - 1, then the rows of
    envelopes.table with the edge cases first"""
    rows, placed = [], []
    for b in sorted({0, min(1, c.K - 1), c.K - 1}):
        for target, r in target_rows(c, b).items():
            frame = c.position + b * c.N - block_context(c, b) + r
            for stage in STAGES:
                voice = placed_voice(stage, frame)
                if voice is not None:
                    rows.append(voice)
                    placed.append(Placed(b, target, stage, frame))
    table, kinds = E.table(c.position, c.N, c.K, seed=zlib.crc32(c.name.encode()) % 997)
    order = np.concatenate([np.nonzero(kinds == k)[0] for k in ('edge', 'aligned', 'grid', 'control')])
    rest = np.stack([table[k][0, order] for k in PARAMS], axis=1)
    return np.concatenate([np.array(rows).reshape(-1, 6), rest]), placed


def common_values(c: Case) -> dict:
    """the (1, 1) parameters of the case's envelope layout: the hand-placed voices' own stage lengths, so that they keep their ends"""
    values = dict(attack=A_FRAMES / RATE, decay=D_FRAMES / RATE, sustain=SUSTAIN, release=R_FRAMES / RATE)
    if c.env == 'one':                                                          # one envelope for all: its attack ends on block K - 1's first row
        frame = c.position + (c.K - 1) * c.N
        values.update(zip(PARAMS, placed_voice('attack', frame) or placed_voice('decay', frame)))
    return {k: values[k] for k in COMMON[c.env]}


# ---------------------------------------------------------------------------------------------------------------------- build
Built = collections.namedtuple('Built', 'case x gains cutoff env out ref y64 y80 level weight placed')


def _pans(C, V, rng):
    """cos in the even channels, sin in the odd ones, of angles that keep both above 0.29: every voice carries weight in every channel"""
    pan = rng.uniform(0.3, np.pi / 2 - 0.3, (C, V))
    return np.where(np.arange(C)[:, None] % 2 == 0, np.cos(pan), np.sin(pan))


def _audible_cutoffs(c: Case, x64, weight, rng):
    """(cutoff rows, y64): cutoffs drawn in 200 .. 8000 Hz; a voice whose filtered rows reach less than 4 CONTRIBUTION of the bus's
    peak at full level -- a low-pass far below the few rows of a short window -- draws again (all voices, where they share one cutoff)"""
    hist = history_of(c)
    cutoff = cutoff_rows(c, rng)
    y64 = filter_blocks(c.btype, x64, hist, c.N, c.K, c.context, c.position, cutoff)
    for _ in range(64):
        bus = R.sum_bus(y64, None if c.C == 'mono' else weight)
        weak = np.nonzero(contributions(y64, 1.0, weight, bus) < 4 * CONTRIBUTION)[0]
        if not len(weak):
            return cutoff, y64
        if cutoff.shape[1] == 1:
            cutoff = cutoff_rows(c, rng)
            weak = np.arange(c.V)
        else:
            cutoff[:, weak] = rng.uniform(200.0, 8000.0, (cutoff.shape[0], len(weak)))
        y64[:, weak] = filter_blocks(c.btype, x64[:, weak], hist, c.N, c.K, c.context, c.position, cutoff if cutoff.shape[1] == 1 else cutoff[:, weak])
    raise AssertionError((c.name, 'voices too quiet to be told from the bound', weak[:8]))


def contributions(y, level, weight, ref) -> np.ndarray:
    """(V,) the largest |w[c, v] level[n, v] y[n, v]| over rows and channels, as a share of max|ref|"""
    return (np.abs(y * level).max(axis=0) * np.abs(weight).max(axis=0)) / np.abs(ref).max()


@functools.lru_cache(maxsize=None)
def build(name: str) -> Built:
    """the operands (x, gains: Views; cutoff: float64 rows; env: name -> (1, V | 1) float64 or None), `out` (a View of zeros) and the
    float64 reference of a case; y64 / y80: the per-voice filter output of the restatement and of its longdouble twin; level: the
    (K N, V) envelope (ones without); weight: the (C, V) gains (ones for 'mono').  Computed once per case and shared (read-only)."""
    c = BY_NAME[name]
    rng = rng_of('bus_pass', c.name, c.seed)
    C, hist, rows = channels_of(c), history_of(c), c.N * c.K
    x = f32(rng.uniform(-0.25, 0.25, (hist + rows, c.V)))
    weight = np.ones((1, c.V)) if c.C == 'mono' else _pans(C, c.V, rng)
    x64 = x.astype(np.float64)
    cutoff, y64 = _audible_cutoffs(c, x64, weight, rng)
    y80 = filter_longdouble(c.btype, x64, hist, c.N, c.K, c.context, c.position, cutoff)
    env, placed, level = None, (), np.ones((rows, c.V))
    if c.env is not None:
        cand, cand_placed = envelope_candidates(c)
        for k, value in common_values(c).items():
            cand[:, PARAMS.index(k)] = value
        if c.env == 'one':
            cand, cand_placed = cand[:1], []
        # a candidate goes to the next free voice if it is heard there: CONTRIBUTION with a margin of 1.5, against the bus of all voices at full level
        scale = np.abs(R.sum_bus(y64, None if c.C == 'mono' else weight)).max()
        chosen, kept, v, i = [], [], 0, 0
        while v < c.V:
            p = cand[i % len(cand)]
            lvl = R.adsr(c.position, rows, RATE, *(np.array([[q]]) for q in p))
            if c.env == 'one' or float(np.abs(y64[:, v:v + 1] * lvl).max() * np.abs(weight[:, v]).max()) >= 1.5 * CONTRIBUTION * scale:
                chosen.append(p)
                if i < len(cand_placed):
                    kept.append((v, cand_placed[i]))
                v += 1
            i += 1
            assert i < 64 * (len(cand) + c.V), (name, 'no audible envelopes left')
        table = np.array(chosen)
        env = {k: (np.array([[table[0, j]]]) if k in COMMON[c.env] else np.ascontiguousarray(table[:, j][None, :])) for j, k in enumerate(PARAMS)}
        level = np.broadcast_to(R.adsr(c.position, rows, RATE, *(env[k] for k in PARAMS)), (rows, c.V)).copy()
        placed = tuple(kept)
    ref = R.sum_bus(y64 * level, None if c.C == 'mono' else weight)
    built = Built(c, view(x, *LAYOUT[c.layout]), None if c.C == 'mono' else view(weight, 0, c.gains_extra), cutoff, env,
                  view(np.zeros((rows, C), dtype=np.float32), 0, c.out_extra), ref, y64, y80, level, weight, placed)
    for a in (x, cutoff, weight, ref, y64, y80, level) + tuple((env or {}).values()):
        a.setflags(write=False)
    return built


def half_ulp32(ref: np.ndarray) -> np.ndarray:
    """half a float32 unit in the last place of `ref`, as base_kernel_cases.bus_bound computes it"""
    _, e = np.frexp(ref)                                                        # |ref| in [2^(e-1), 2^e): ulp 2^(e-24)
    return 0.5 * np.ldexp(1.0, np.maximum(e - 24, -149))


def summation_term(y64, level, weight) -> np.ndarray:
    """V 2^-53 (|y level| @ |w|^T): base_kernel_cases.bus_bound's term for a length-V float64 sum of products in any order"""
    return y64.shape[1] * 2.0 ** -53 * (np.abs(y64 * level) @ np.abs(weight).T)


def recurrence_term(y64, y80, weight) -> np.ndarray:
    """(4 |y64 - y80|) @ |w|^T: the kernel folds b0 into the weight, steps with three fused multiply-adds and sums in tree order -- each
    moves a value by at most what one float64 rounding does, the longdouble distance measures what all the float64 roundings of the
    restatement together do, and the fourth share is the restatement's own"""
    return (4.0 * np.abs(y64.astype(np.longdouble) - y80).astype(np.float64)) @ np.abs(weight).T


def bound_terms(b: Built) -> tuple:
    return half_ulp32(b.ref), summation_term(b.y64, b.level, b.weight), recurrence_term(b.y64, b.y80, b.weight)


# ------------------------------------------------------------------------------------------------------------------ the census
Variant = collections.namedtuple('Variant', 'vec_ok vpt env C ring chunk group voice_tiles idle_waves ragged_front ragged_end short_of_group '
                                            'into_history repeats_last_row')
INSTANTIATIONS = tuple((vpt, env, C) for vpt in (4, 1) for env in (False, True) for C in (1, 2, 4))


def expected_variant(c: Case) -> Variant:
    """the dispatch of biquad_bus.hip restated (launch: vec_ok over voices, the input's leading dimension and pointer; kRing; Tile<C>::R;
    kChunk) and, per block, the row groups its flush meets: ragged_front / ragged_end / short_of_group / into_history are the sets of
    blocks whose first group starts inside the context rows (c % R != 0), whose last group ends past the block ((c + N) % R != 0), that
    are shorter than one group, and (block >= 1) whose context reaches back into the history rows"""
    v = View(np.zeros((1, c.V)), *LAYOUT[c.layout])
    vec = c.V % 4 == 0 and ld(v) % 4 == 0 and v.pad % 4 == 0
    vpt, env, C = (4 if vec else 1), c.env is not None, channels_of(c)
    ring = 8 if env and vec else 16
    group = 16 // C
    chunk = max(ring, group)
    tiles = -(-c.V // (64 * vpt))
    blocks = [(b, block_context(c, b)) for b in range(c.K)]
    return Variant(vec, vpt, env, C, ring, chunk, group, tiles, (c.K * tiles) % 4 != 0,
                   frozenset(b for b, c0 in blocks if c0 % group), frozenset(b for b, c0 in blocks if (c0 + c.N) % group),
                   frozenset(b for b, _ in blocks if c.N < group), frozenset(b for b, c0 in blocks if b and b * c.N < c0),
                   frozenset(b for b, c0 in blocks if (c0 + c.N) % chunk or c0 + c.N < ring))


# ------------------------------------------------------------------------------------- the bit-for-bit invariants and the rest
# (what tests/test_gpu_bus_pass.py launches besides one launch per case, on the cases' own data; the host test takes the census)
BATCHING = ('v4_growing_context', 'v1_idle_waves', 'e4_c2_far', 'e1_c1')          # K blocks in one call against K calls of one block, row 0 of the cutoffs
# (case, live voices, layout): the first `live` voices of the case's buffers against all of them with the other gains at 0.  Both
# renders go through ONE kernel: 252 of 256 keeps four voices per lane; 61 of 64 takes one voice per lane, so its buffer has a
# leading dimension of 65, where 64 voices take one per lane too
DEAD_VOICES = (('e4_c2_hour', 252, 'pad4'), ('v4_far_c2', 61, 'ld1'))
DEAD_VOICES_ACROSS = ('v4_far_c2', 61, 'contig')                                  # a leading dimension of 64: one voice per lane against four, so only within the summation term
BUS_WIDTH = ('v4_far_c2', 'e1_c4')                                                # gain rows [g0, g1, g0, g1] against [g0, g1] against g0 and g1 alone
CUTOFF_ROWS = ('v4_position_in_context', 'e1_c1')                                 # K identical rows against one
LANES = ('v4_dead_lane_c4', 'v4_position_in_context', 'e4_c2_hour', 'e4_c4_refresh')   # four voices per lane against the same data at pad1
STATUS_VALUES = (0.0, RATE / 2.0, float('nan'))
STATUS_CASE = 'v4_ragged_front_c2'
REFUSALS = ('C = 3', 'C = 2 without gains', 'type bp', 'in_history one short', 'out_ld < C', 'cutoff blocks neither 1 nor K')
EMPTY = ('N', 'K', 'V')


def launches() -> dict:
    """the launches of tests/test_gpu_bus_pass.py, by test (the refusals and the empty launches launch nothing; one accepted call behind them)"""
    K = lambda name: BY_NAME[name].K
    return {'cases': len(CASES), 'batching': sum(1 + K(n) for n in BATCHING), 'dead voices': 2 * len(DEAD_VOICES) + 2,
            'bus width': 4 * len(BUS_WIDTH), 'cutoff rows': 2 * len(CUTOFF_ROWS), 'lanes': 2 * len(LANES),
            'status': 4 * len(STATUS_VALUES) + 3, 'refusals': 1}
