"""ADSR parameter tables whose stage boundaries land EXACTLY on sample rows, for the envelope edge tests.

The kernels that walk time forwards (fused_cascade.hip, voice_program.hip and its specialised images) follow the current
stage of each envelope as a line and re-derive it from the definition (oracle/chain_ref.py:adsr) only where the stage's end
(sig_adsr.h: segment_at) is reached.  Continuous random parameters put the ends between rows; round numbers and whole
frame counts put them on rows, where the definition's own comparisons may still pick the old stage.  `table` builds such
rows for one launch window and `boundary_rows` reports which rows of the window hold an exact boundary, so that a test can
assert that it still exercises one."""
import itertools

import numpy as np

RATE = 48000
HOUR = 3600 * RATE                       # frames
PARAMS = ('attack', 'decay', 'sustain', 'release', 'gate_on', 'gate_off')
MS = 1e-3


def _rows(voices):
    """list of (attack, decay, sustain, release, gate_on, gate_off) -> dict of (1, V) float64 rows"""
    a = np.array(voices, dtype=np.float64).reshape(-1, 6)
    return {k: np.ascontiguousarray(a[:, i].reshape(1, -1)) for i, k in enumerate(PARAMS)}


def concat(*tables):
    return {k: np.concatenate([t[k] for t in tables], axis=1) for k in PARAMS}


def round_grid(on_seconds, attack_ms, decay_ms, release_ms, length_ms, sustain=(0.0, 0.5, 1.0)):
    """every combination of round-number parameters, as a user writes them: gate_off = gate_on + length in f64"""
    out = []
    for on, a, d, r, g, s in itertools.product(on_seconds, attack_ms, decay_ms, release_ms, length_ms, sustain):
        out.append((a * MS, d * MS, s, r * MS, on, on + g * MS))
    return _rows(out)


def aligned_draws(n, start, span, seed, max_stage=None):
    """n seeded envelopes whose every time is a whole number of frames over RATE (gate_on = k / RATE with k in
    [start, start + span)), stage lengths from 0 to `max_stage` frames with many of 0 to 3 frames"""
    rng = np.random.default_rng(seed)
    max_stage = max_stage or max(span // 4, 4)

    def stage(size):
        long = rng.integers(0, max_stage + 1, size)
        short = rng.integers(0, 4, size)
        return np.where(rng.random(size) < 0.3, short, long)
    on = start + rng.integers(0, span, n)
    a, d, r, g = stage(n), stage(n), stage(n), stage(n) + rng.integers(-2, 3, n)
    s = np.where(rng.random(n) < 0.25, rng.choice([0.0, 1.0], n), np.round(rng.uniform(0, 1, n), 3))
    return _rows(np.stack([a / RATE, d / RATE, s, r / RATE, on / RATE, (on + g) / RATE], axis=1))


def edge_cases(position, N, K):
    """hand-placed envelopes for the launch window [position, position + K N) in blocks of N: zero-length stages, a release
    during the attack and during the decay, gate_off <= gate_on, a negative gate_on, boundaries on a block's first and last
    rows, on the batch's last row and on the first row of the second block (inside a lane's span when it spans blocks)"""
    f = lambda n: n / RATE                                     # frame -> seconds, as the row times are computed
    p, last = position, position + K * N - 1
    q = N // 4
    v = [
        # (attack, decay, sustain, release, gate_on, gate_off)
        (0.0, 0.0, 0.5, 0.0, f(p + q), f(p + 2 * q)),                       # every stage of zero length
        (0.0, f(q), 0.3, 0.0, f(p + 1), f(p + 3 * q)),                      # no attack, no release
        (f(q), 0.0, 0.7, f(q), f(p + 2), f(p + 3 * q)),                     # no decay
        (f(4 * q), f(q), 0.5, f(q), f(p), f(p + 2 * q)),                    # released during the attack
        (f(q), f(4 * q), 0.2, f(2 * q), f(p), f(p + 3 * q)),                # released during the decay
        (f(q), f(q), 0.5, f(q), f(p + q), f(p + q)),                        # gate_off == gate_on
        (f(q), f(q), 0.5, f(q), f(p + 2 * q), f(p + q)),                    # gate_off < gate_on
        (f(q), f(q), 0.5, f(2 * q), -1.0, f(p + q)),                        # negative gate_on, sustaining at the start
        (f(q), f(q), 0.5, f(N), -3600.0, f(p + 2)),                         # an hour before zero
        (f(N - 1), f(1), 0.4, f(N), f(p), f(p + 3 * N // 2)),               # gate on row 0, attack ends on the block's last row
        (f(1), f(N - 2), 0.6, f(2), f(p + N - 1), f(p + 2 * N)),            # gate on a block's last row, decay ends on row N
        (f(2), f(3), 0.5, f(N), f(p + N), f(last - N + 1)),                 # gate on the second block's first row
        (f(q), f(q), 0.5, f(N), f(p + q), f(last - N + 1)),                 # release ends on the batch's last row
        (f(2), f(2), 0.5, f(2), f(p - 2), f(last - 2)),                     # attack ends on the window's first row
        (f(3), f(N), 0.5, f(1), f(p - 3 - N), f(last)),                     # decay ends on row 0; gate_off on the last row
        (f(1), f(1), 0.5, f(1), f(last - 2), f(last - 1)),                  # one-frame stages at the end of the batch
    ]
    if K > 1:
        v += [(f(N), f(N), 0.5, f(N), f(p), f(p + 2 * N)),                  # boundaries on the first row of blocks 1, 2, 3
              (f(N - 1), f(1), 0.5, f(N), f(p), f(p + 2 * N - 1))]          # ... and on the last row of blocks 0 and 1
    return _rows(v)


def control(n, seed, start):
    """today's continuous random voices (tests/test_gpu_fused_cascade.py: params), gate_on from `start` seconds"""
    rng = np.random.default_rng(seed)
    return _rows(np.stack([rng.uniform(0.001, 0.05, n), rng.uniform(0.01, 0.2, n), rng.uniform(0.2, 0.9, n),
                           rng.uniform(0.02, 0.3, n), start + rng.uniform(0.0, 0.05, n), start + rng.uniform(0.06, 0.12, n)], axis=1))


def table(position, N, K, seed=0, grid=True):
    """(1, V) ADSR rows for a launch window of K blocks of N frames at `position` (a whole number of seconds or not):
    a round-number grid starting at the window, frame-aligned seeded draws inside it, the edge cases, and a control group.
    Returns (rows, kinds) with kinds a (V,) array of 'grid' | 'aligned' | 'edge' | 'control'."""
    W = K * N
    on0 = position / RATE
    parts, kinds = [], []
    if grid:
        ms = W / RATE / MS                                      # the window in milliseconds
        stages = [x for x in (0, 1, 2, 5, 10, 20, 50) if x <= ms / 4]
        lengths = [x for x in (1, 5, 10, 20, 50, 100) if x <= ms / 2]
        ons = [on0 + x * MS for x in (0, 5) if x <= ms / 4]
        parts.append(round_grid(ons, stages, stages[::2], stages[1::2], lengths[:3]))
        kinds.append('grid')
    parts.append(aligned_draws(256, position - W // 8, W, seed))
    kinds.append('aligned')
    parts.append(edge_cases(position, N, K))
    kinds.append('edge')
    parts.append(control(32, seed + 1, on0))
    kinds.append('control')
    rows = concat(*parts)
    return rows, np.concatenate([[k] * p['attack'].shape[1] for k, p in zip(kinds, parts)])


def boundaries(rows):
    """(3, V) the stage ends sig_adsr.h computes as sums -- gate_on + attack, + decay, gate_off + release -- where the
    definition compares a difference ((t - gate_on) - attack < 0, ...), which may round the other way on the row of the
    sum itself (gate_on and gate_off are compared with t directly)"""
    a, d, r, on, off = (np.asarray(rows[k], dtype=np.float64).reshape(-1) for k in ('attack', 'decay', 'release', 'gate_on', 'gate_off'))
    with np.errstate(divide='ignore'):
        inv = lambda x: np.where(x > 0, 1.0 / np.where(x > 0, 1.0 / np.where(x > 0, x, 1.0), 1.0), np.inf)
    return np.stack([np.where(a > 0, on + a, np.inf), on + a + inv(d), off + inv(r)])


def boundary_rows(rows, position, frames, rate=RATE):
    """(frames, V) bool: row n of [position, position + frames) holds one of the `boundaries` exactly, n / rate == end"""
    b = boundaries(rows)
    t = np.arange(position, position + frames, dtype=np.int64).reshape(-1, 1) / rate
    hit = np.zeros((frames, b.shape[1]), dtype=bool)
    for k in range(b.shape[0]):
        n = np.rint(b[k] * rate)
        ok = np.isfinite(n) & (n >= position) & (n < position + frames)
        idx = np.where(ok, n - position, 0).astype(np.int64)
        exact = ok & (t[idx, 0] == b[k])
        hit[idx[exact], np.nonzero(exact)[0]] = True
    return hit
