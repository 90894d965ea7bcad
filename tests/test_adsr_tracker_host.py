"""The piecewise-linear ADSR tracker of the forward-walking kernels (sig_adsr.h: segment_at; fused_cascade.hip,
voice_program.hip) compiled for the host from the real header and walked row by row the way the kernels walk it, against
the definition (oracle/chain_ref.py:adsr) on envelopes whose stage boundaries land exactly on sample rows: the
round-number grid, the GPU tests' tables (tests/envelopes.py) and 10^5 seeded frame-aligned envelopes, some of them hours
into the stream.  No GPU: the header is plain f64 arithmetic under -ffp-contract=off, as on the device."""
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

import envelopes as E

ROOT = pathlib.Path(__file__).resolve().parent.parent
NATIVE = ROOT / 'tests' / 'native'
HEADER = ROOT / 'signals_amd' / 'csrc' / 'sig_adsr.h'
TOL = 1e-6                                                   # the project's bar at full scale 1


@pytest.fixture(scope='module')
def tracker(tmp_path_factory):
    """the harness built against a COPY of sig_adsr.h next to the stub sig_common.h (a quoted include resolves in the
    including header's own directory first, so the copy picks up the stub, not the HIP one)"""
    cxx = shutil.which('g++') or shutil.which('c++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('adsr_tracker')
    shutil.copy(HEADER, d / 'sig_adsr.h')
    shutil.copy(NATIVE / 'sig_common.h', d / 'sig_common.h')
    shutil.copy(NATIVE / 'adsr_tracker.cpp', d / 'adsr_tracker.cpp')
    exe = d / 'adsr_tracker'
    subprocess.run([cxx, '-std=c++17', '-O2', '-ffp-contract=off', '-I', str(d), str(d / 'adsr_tracker.cpp'), '-o', str(exe)],
                   check=True, capture_output=True, text=True)

    def run(groups):
        """groups: [(rows, start, frames, probe_frames)] -> [(tracked (P, V), level (P, V), max |tracked - level| (V,))]"""
        blob = [np.array([len(groups)], dtype=np.int64).tobytes()]
        for rows, start, frames, probes in groups:
            V = rows['attack'].shape[1]
            blob.append(np.array([start, frames, V, len(probes)], dtype=np.int64).tobytes())
            blob.append(np.array([E.RATE], dtype=np.float64).tobytes())
            blob.append(np.stack([rows[k].reshape(-1) for k in E.PARAMS]).astype(np.float64).tobytes())
            blob.append(np.asarray(probes, dtype=np.int64).tobytes())
        (d / 'in.bin').write_bytes(b''.join(blob))
        subprocess.run([str(exe), str(d / 'in.bin'), str(d / 'out.bin')], check=True, timeout=300)
        raw = np.fromfile(d / 'out.bin', dtype=np.float64)
        out, at = [], 0
        for rows, _, _, probes in groups:
            V, P = rows['attack'].shape[1], len(probes)
            tracked = raw[at:at + P * V].reshape(P, V); at += P * V
            level = raw[at:at + P * V].reshape(P, V); at += P * V
            out.append((tracked, level, raw[at:at + V])); at += V
        assert at == raw.size
        return out
    return run


def probe_frames(rows, start, frames, stride, near_boundaries=True):
    """rows to compare with the oracle: around every boundary (rounded to a row), on a stride, and the last rows"""
    p = [np.arange(start, start + frames, stride), np.arange(start + frames - 4, start + frames)]
    if near_boundaries:
        n = np.rint(E.boundaries(rows) * E.RATE).reshape(-1)
        n = np.unique(n[np.isfinite(n)]).astype(np.int64)
        p.append((n[:, None] + np.arange(-2, 3)).reshape(-1))
    p = np.unique(np.concatenate(p))
    return p[(p >= start) & (p < start + frames)]


def oracle_at(rows, probes):
    from oracle import chain_ref as R
    return np.concatenate([R.adsr(int(n), 1, E.RATE, **rows) for n in probes])


def check(tracker, groups, what):
    """every group: the header's level() is the oracle at the probes (bit for bit), the tracked level is within TOL of the
    oracle there and of level() on every row walked; returns the number of exact-boundary rows the groups walked"""
    hits = 0
    for (rows, start, frames, probes), (tracked, level, maxdiff) in zip(groups, tracker(groups)):
        ref = oracle_at(rows, probes)
        assert np.array_equal(level, ref), (what, start)
        err = np.abs(tracked - ref).max(axis=0)
        bad = np.nonzero(~(np.maximum(err, maxdiff) < TOL))[0]
        if bad.size:
            v = bad[np.argmax(np.maximum(err, maxdiff)[bad])]
            raise AssertionError(f'{what}: {bad.size} of {err.size} envelopes off by more than {TOL} (group at frame {start}); '
                                 f'worst {max(err[v], maxdiff[v]):.3g} for ' +
                                 ', '.join(f'{k}={rows[k][0, v]!r}' for k in E.PARAMS))
        hits += int(E.boundary_rows(rows, start, frames).any(axis=0).sum())
    return hits


def _grid_groups():
    groups = []
    for on in (0.0, 0.5, 1.0, 2.0, 10.0, 60.0, 3600.0):
        rows = E.round_grid([on], [0, 1, 5, 10, 20, 50, 100], [0, 10, 50, 100, 200], [0, 10, 100, 200, 500], [5, 50, 300, 1000])
        start, frames = max(int(on * E.RATE) - 2, 0), int(1.7 * E.RATE)
        groups.append((rows, start, frames, probe_frames(rows, start, frames, 397)))
    return groups


def test_round_number_grid_walked_by_the_tracker(tracker):
    """gate_on {0, 0.5, 1, 2, 10, 60, 3600} s x attack {0, 1, 5, 10, 20, 50, 100} ms x decay {0, 10, 50, 100, 200} ms x
    release {0, 10, 100, 200, 500} ms x gate length {5, 50, 300, 1000} ms x sustain {0, 0.5, 1}: 14700 envelopes, each
    walked over 1.7 s from two rows before its gate_on"""
    groups = _grid_groups()
    hits = check(tracker, groups, 'round grid')
    assert hits > 5000, hits                                 # most envelopes have a boundary exactly on a row


@pytest.mark.parametrize('position', [0, 24_000, E.HOUR, int(2.3 * E.HOUR), 10 * E.HOUR])
def test_gpu_tables_walked_by_the_tracker(tracker, position):
    """the tables of tests/test_gpu_envelope_edges.py (round grid at the window, frame-aligned draws, edge cases, control
    voices) over their launch windows, started where the kernels start them"""
    groups = []
    for N, K in ((1024, 9), (256, 6), (32, 48)):
        rows, kinds = E.table(position, N, K, seed=position % 1000 + N)
        start, frames = position, K * N                          # the kernels derive the stage at the first output row
        groups.append((rows, start, frames, probe_frames(rows, start, frames, 7)))
        hit = E.boundary_rows(rows, position, K * N).any(axis=0)
        for kind in ('grid', 'aligned', 'edge'):
            assert hit[kinds == kind].sum() >= 8, (N, kind)
    check(tracker, groups, f'tables at {position}')


def test_seeded_frame_aligned_sweep(tracker):
    """10^5 envelopes with every time a whole number of frames (stages of 0 to 1200 frames, many of 0 to 3), in 100 groups
    whose gate_on lie from frame 0 to 10 h into the stream"""
    rng = np.random.default_rng(2024)
    starts = np.concatenate([rng.integers(4, 48_000 * 60, 70), rng.integers(E.HOUR, 10 * E.HOUR, 27),
                             [int(2.3 * E.HOUR), 10 * E.HOUR, 10 * E.HOUR + 1]])
    groups = []
    for g, s in enumerate(starts):
        rows = E.aligned_draws(1000, int(s), 400, seed=g, max_stage=1200)
        start, frames = int(s) - 4, 400 + 4 * 1200 + 40
        groups.append((rows, start, frames, probe_frames(rows, start, frames, 211, near_boundaries=False)))
    hits = check(tracker, groups, 'frame-aligned sweep')
    assert hits > 50_000, hits
