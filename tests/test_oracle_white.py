"""White noise's definition in the oracle (oracle/chain_ref.py: white), on the host: SplitMix64's published outputs, the
structure of the samples, their statistics, and the shipped header (signals_amd/csrc/sig_noise.h) compiled for the host
against the same grid.  The reference draws np.random.rand from the global unseeded generator (noise.py:22-23), so there the
parity is statistical only; the build's generator is a fully specified function and is pinned bit for bit."""
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

from oracle import chain_ref as R

ROOT = pathlib.Path(__file__).resolve().parent.parent
NATIVE = ROOT / 'tests' / 'native'
HEADER = ROOT / 'signals_amd' / 'csrc' / 'sig_noise.h'

SEEDS = (0, 1, 12345, 2 ** 63, 2 ** 64 - 1)
POSITIONS = (0, 2 ** 32 - 50, 172_800_000, 2 ** 40)
# SplitMix64 seeded with 0 (Steele, Lea, Flood 2014; the reference implementation splitmix64.c by S. Vigna): outputs 1, 2, 3
SPLITMIX64_FROM_0 = (0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F)


def mix64(z: int) -> int:
    """SplitMix64's output function in Python integers (an independent restatement of the numpy one in the oracle)"""
    m = (1 << 64) - 1
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


# ---------------------------------------------------------------- known answers
def test_splitmix64_known_answers():
    """seed 0, pair 0: the hash of frame f is SplitMix64's f-th output -- the low word is channel 0, the high word channel 1"""
    assert np.array_equal(R.white(0, 1, 1, 2), np.array([[8068557, 14819496]]) * 2.0 ** -24)
    for f, h in enumerate(SPLITMIX64_FROM_0, start=1):
        assert mix64(f * 0x9E3779B97F4A7C15 & (2 ** 64 - 1)) == h
        assert int(R.white_hash(0, f, 1, 1)[0, 0]) == h
        want = np.array([[(h & 0xFFFFFFFF) >> 8, h >> 40]]) * 2.0 ** -24
        assert np.array_equal(R.white(0, f, 1, 2), want), f
    assert np.array_equal(R.white(0, 1, 3, 2), np.concatenate([R.white(0, f, 1, 2) for f in (1, 2, 3)]))
    assert np.array_equal(R.white(0, 0, 1, 2), np.zeros((1, 2)))            # mix64(0) = 0


def test_hash_wraps_modulo_2_64():
    top = 2 ** 64 - 1
    assert int(R.white_hash(top, 1, 1, 1)[0, 0]) == mix64(0x9E3779B97F4A7C15 - 1)
    h = mix64(0x9E3779B97F4A7C15 - 1)
    assert np.array_equal(R.white(top, 1, 1, 2), np.array([[(h & 0xFFFFFFFF) >> 8, h >> 40]]) * 2.0 ** -24)
    # every term in Python integers, frames past 2^32 and pairs whose product wraps several times
    for seed, frame, pair in ((top, 2 ** 40 + 3, 499), (2 ** 63, 2 ** 32, 1), (12345, 2 ** 31, 32), (2 ** 32, 2 ** 62, 2047)):
        want = mix64((seed + frame * 0x9E3779B97F4A7C15 + pair * 0xD1B54A32D192ED03) % 2 ** 64)
        assert int(R.white_hash(seed, frame, 1, pair + 1)[0, pair]) == want, (seed, frame, pair)
    for bad in (-1, 2 ** 64):
        with pytest.raises(ValueError):
            R.white(bad, 0, 1, 1)


# ---------------------------------------------------------------- structure
@pytest.mark.parametrize('seed', SEEDS)
def test_samples_are_24_bit_fractions_pure_in_position_and_channel(seed):
    for pos in POSITIONS:
        x = R.white(seed, pos, 40, 7)
        k = x * 2.0 ** 24
        assert x.dtype == np.float64 and x.shape == (40, 7)
        assert np.array_equal(k, np.floor(k)) and k.min() >= 0 and k.max() < 2 ** 24
        assert np.array_equal(x.astype(np.float32).astype(np.float64), x)          # exact in float32
        for i, j in ((0, 0), (1, 6), (17, 3), (39, 5), (39, 6)):
            assert x[i, j] == R.white(seed, pos + i, 1, j + 1)[0, j]
        assert np.array_equal(R.white(seed, pos + 11, 20, 4), x[11:31, :4])
        # channels 2m and 2m + 1 are the two words of one hash; an unpaired last channel is the low word of its own
        h = R.white_hash(seed, pos, 40, 4)
        bits = R.white_bits(seed, pos, 40, 7).astype(np.uint64)
        assert np.array_equal(bits[:, 0:6:2] | (bits[:, 1:6:2] << np.uint64(32)), h[:, :3])
        assert np.array_equal(bits[:, 6], h[:, 3] & np.uint64(0xFFFFFFFF))


def test_white_node_in_graphs():
    """the node answers its own `channels` columns from a block cache, at frame rate and at block rate, under filters,
    element-wise nodes and a bus"""
    w = R.White(seed=7, channels=3)
    assert np.array_equal(R.render(w, 1000, 64, 3), R.white(7, 1000, 64, 3))
    assert np.array_equal(R.render(w, 1010, 1, 3), R.white(7, 1010, 1, 3))         # (served from the cached block)
    assert np.array_equal(R.render(w, 5000, 1, 3), R.white(7, 5000, 1, 3))
    assert R.render(w, 5000, 1, 3).shape == (1, 3)
    cut = np.array([[300.0, 1000.0, 5000.0]])
    got = R.render_stream(R.Filter('lp', R.White(7, 3), R.Fixed(cut)), 0, 128, 3, 3)
    src = lambda q, n: R.white(7, q, n, 3)
    want = np.concatenate([R.filter_block('lp', src, b * 128, 128, 48000, cut) for b in range(3)])
    assert np.array_equal(got, want)
    g = R.Binary('Gain', R.White(7, 3), R.Fixed([[0.5]]))
    assert np.array_equal(R.render(g, 40, 16, 3), 0.5 * R.white(7, 40, 16, 3))
    bus = R.SumBus(R.Binary('RingMod', R.White(7, 3), R.White(8, 3)))
    bus.in_channels = 3
    assert np.allclose(R.render(bus, 0, 16, 1)[:, 0], (R.white(7, 0, 16, 3) * R.white(8, 0, 16, 3)).sum(axis=1))
    one = R.render(R.Filter('lp', R.White(7, 3), R.Fixed(cut)), 4800, 1, 3)          # a block-rate read of a filtered White
    assert one.shape == (1, 3) and np.array_equal(one, R.filter_block('lp', src, 4800, 1, 48000, cut))


# ---------------------------------------------------------------- statistics of the definition
def stats(x):
    return (abs(x.mean() - 0.5), abs(x.var() - 1 / 12), abs(np.corrcoef(x[:-1].ravel(), x[1:].ravel())[0, 1]),
            abs(np.corrcoef(x[:, :-1].ravel(), x[:, 1:].ravel())[0, 1]))


def test_oracle_statistics():
    """the bounds tests/test_gpu_engine.py::test_white_noise_statistics holds the kernel to, on 4096 x 65 blocks"""
    worst = np.zeros(4)
    for seed in SEEDS:
        for pos in POSITIONS:
            x = R.white(seed, pos, 4096, 65)
            assert x.min() >= 0.0 and x.max() < 1.0
            s = stats(x)
            assert s[0] < 5e-3 and s[1] < 2e-3 and s[2] < 0.01 and s[3] < 0.01, (seed, pos, s)
            worst = np.maximum(worst, s)
    print('worst |mean - 1/2|, |var - 1/12|, lag-1 correlation along frames, along channels:', worst)


# ---------------------------------------------------------------- the shipped header, compiled for the host
@pytest.fixture(scope='module')
def header(tmp_path_factory):
    """sig_noise.h built against the stub sig_common.h next to a COPY of it (a quoted include resolves in the including
    header's own directory first), as tests/test_adsr_tracker_host.py builds sig_adsr.h"""
    cxx = shutil.which('g++') or shutil.which('c++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('noise_hash')
    shutil.copy(HEADER, d / 'sig_noise.h')
    shutil.copy(NATIVE / 'sig_common.h', d / 'sig_common.h')
    shutil.copy(NATIVE / 'noise_hash.cpp', d / 'noise_hash.cpp')
    exe = d / 'noise_hash'
    subprocess.run([cxx, '-std=c++17', '-O2', '-ffp-contract=off', '-I', str(d), str(d / 'noise_hash.cpp'), '-o', str(exe)],
                   check=True, capture_output=True, text=True)

    def run(groups):
        """groups: [(seed, position, frames, channels)] -> [(bits uint32, value float32)], each (frames, channels)"""
        blob = [np.array([len(groups)], dtype=np.int64).tobytes()]
        for seed, pos, n, c in groups:
            blob.append(np.array([seed], dtype=np.uint64).tobytes() + np.array([pos, n, c], dtype=np.int64).tobytes())
        (d / 'in.bin').write_bytes(b''.join(blob))
        subprocess.run([str(exe), str(d / 'in.bin'), str(d / 'out.bin')], check=True, timeout=300)
        raw, out, at = (d / 'out.bin').read_bytes(), [], 0
        for _, _, n, c in groups:
            bits = np.frombuffer(raw, dtype=np.uint32, count=n * c, offset=at).reshape(n, c); at += 4 * n * c
            value = np.frombuffer(raw, dtype=np.float32, count=n * c, offset=at).reshape(n, c); at += 4 * n * c
            out.append((bits, value))
        assert at == len(raw)
        return out
    return run


def test_shipped_header_equals_the_oracle(header):
    """noise_bits and noise_value of sig_noise.h -- what noise.hip and control_program.hip compile -- over the seeds and
    positions of the statistics test and blocks that straddle frames 2^31 and 2^32, 65 channels (an unpaired last one)"""
    groups = [(s, p, 300, 65) for s in SEEDS for p in POSITIONS + (2 ** 31 - 40,)]
    groups += [(2 ** 32, 1, 64, 1000), (2 ** 63 - 1, 2 ** 40 - 17, 64, 3), (0, 1, 3, 2)]
    for (seed, pos, n, c), (bits, value) in zip(groups, header(groups)):
        assert np.array_equal(bits, R.white_bits(seed, pos, n, c)), (seed, pos)
        assert np.array_equal(value.astype(np.float64), R.white(seed, pos, n, c)), (seed, pos)
    bits, value = header([(0, 1, 3, 2)])[0]
    assert [int(b) for b in bits[:, 0]] == [h & 0xFFFFFFFF for h in SPLITMIX64_FROM_0]
    assert [int(b) for b in bits[:, 1]] == [h >> 32 for h in SPLITMIX64_FROM_0]


# ---------------------------------------------------------------- the node's seed
def test_seed_is_an_unsigned_64_bit_word():
    """the seed travels as a uint64 argument, a uint64[2] struct field and an instruction's pointer field: larger values have
    no single meaning across the routes and are refused"""
    from signals_amd.chain import noise
    assert noise.White.State(seed=2 ** 64 - 1).seed == 2 ** 64 - 1
    assert noise.White.State(seed=2 ** 63).seed == 2 ** 63
    for bad in (2 ** 64, 2 ** 70, -1):
        with pytest.raises(ValueError):
            noise.White.State(seed=bad)
    w = noise.White()
    w.get_state().seed = 2 ** 64 - 1
    with pytest.raises(ValueError):
        w.get_state().seed = 2 ** 64
    assert w.get_state().seed == 2 ** 64 - 1
