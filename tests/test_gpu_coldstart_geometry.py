"""The cold-start filter entries under every launch geometry their host dispatchers can choose: each (voice, block) chain is
independent of the geometry, so the same input must come out bitwise equal, voice by voice, whichever kernel, voices per lane and
span rendered it.  The shapes are the smallest that reach each choice under the dispatchers' rules (biquad.hip launch_biquad,
band.hip launch_band):

  base       V = 256, K = 2048 blocks of N = 8 frames, context 4, at position 0 (block 0 has no context) and 3 N
  plain, 4   K identical cutoff rows: per-block rows switch the span walker off; 1 voice tile x 2048 blocks is not < 2048 items,
             so four voices per lane stay (ring 8)
  walker     one cutoff row, N > context: tiles * K / 1024 = span 2 (four voices per lane), span 4 where the layout halves the lanes' voices
  2 voices   the same data in buffers whose leading dimension is V + 2, viewed from column 2: rows 8-byte aligned only
  1 voice    leading dimension V + 1, viewed from column 1

The resonant and the equaliser entries have the plain kernel only, the band entries four voices or one.  The first geometry of
each entry is also held against the CPU restatements (oracle/chain_ref.py, tests/resonant_reference.py, tests/eq_reference.py), at
some voices of every lane group and the first, middle and last blocks, within the bound the entry's existing test uses; an error
that every geometry shares does not get past that.  The bus entry sums voices in an order that depends on the geometry: it is
called directly by tests/test_gpu_bus_pass.py."""
import functools

import numpy as np
import pytest
import torch

from gpu_helpers import tolerance
from helpers import f32, maxerr
import eq_reference as EQ
import resonant_reference as RR
from signals_amd import _native

pytestmark = pytest.mark.gpu

RATE = 48000
V, K, N, CTX = 256, 2048, 8, 4
DEV = 'cuda:0'
ENTRIES = {'plain': 'lp', 'env': 'hp', 'q': 'lp', 'eq': 'eqpeak', 'band': 'bp', 'band_blocks': 'bp'}


def uniform(lo, hi, seed, rows=1):
    return np.random.default_rng(seed).uniform(lo, hi, (rows, V))


# per-voice control rows; the input keeps the outputs near 1, where the existing tests' 1e-6 is meant
CONTROLS = dict(cutoff=uniform(200.0, 8000.0, 1), q=uniform(0.5, 4.0, 3), gain=uniform(-12.0, 12.0, 4), low=uniform(200.0, 1000.0, 5),
                high=uniform(2000.0, 8000.0, 6))
ADSR = dict(zip(_native.ADSR_PARAMS, (uniform(0.005, 0.05, 2), np.full((1, V), 0.02), np.full((1, V), 0.5), np.full((1, V), 0.05),
                                      np.zeros((1, V)), np.full((1, V), 0.2))))


@functools.lru_cache(maxsize=None)
def signal(position):
    """(history rows, float32-exact input rows) of a render at `position`"""
    hist = min(CTX, position)
    return hist, f32(np.random.default_rng(11).uniform(-0.25, 0.25, (hist + N * K, V))).astype(np.float64)


def layout(x: torch.Tensor, pad: int) -> torch.Tensor:
    """the same data in a buffer `pad` columns wider, viewed from column `pad`"""
    if not pad:
        return x.clone()
    wide = torch.zeros((x.shape[0], x.shape[1] + pad), dtype=x.dtype, device=x.device)
    wide[:, pad:] = x
    return wide[:, pad:]


def render(entry, position, dtype, pad, blocks):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    rows = lambda name: dev(np.broadcast_to(CONTROLS[name], (K, V)) if blocks else CONTROLS[name])
    hist, x = signal(position)
    buf, out = layout(dev(x).to(dtype), pad), layout(torch.zeros((N * K, V), dtype=dtype, device=DEV), pad)
    assert buf.stride(0) == V + pad and out.stride(0) == V + pad
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    head = (ENTRIES[entry], RATE, position, N, K, CTX)
    if entry == 'plain':
        _native.biquad_coldstart(*head, rows('cutoff'), buf, hist, out, status=status)
    elif entry == 'env':
        _native.biquad_coldstart(*head, rows('cutoff'), buf, hist, out, status=status, envelope={k: dev(v) for k, v in ADSR.items()})
    elif entry == 'q':
        _native.biquad_coldstart_q(*head, rows('cutoff'), rows('q'), buf, hist, out, status=status)
    elif entry == 'eq':
        _native.biquad_coldstart_eq(*head, rows('cutoff'), rows('q'), rows('gain'), buf, hist, out, status=status)
    elif blocks:
        _native.band_coldstart_blocks(*head, rows('low'), dev(CONTROLS['high']), buf, hist, out, status=status)
    else:
        _native.band_coldstart(*head, rows('low'), rows('high'), buf, hist, out, status=status)
    assert int(status.item()) == 0
    return out.contiguous()


# (columns of padding, per-block parameter rows); the first is the geometry the others and the restatement are held against
BIQUAD = ((0, True), (0, False), (2, True), (2, False), (1, True), (1, False))
ONE_KERNEL = ((0, True), (0, False), (2, True), (1, False))
BAND = ((0, False), (0, True), (1, False), (1, True))
CASES = [('plain', torch.float32, BIQUAD), ('plain', torch.float64, BIQUAD), ('env', torch.float32, BIQUAD),
         ('q', torch.float32, ONE_KERNEL), ('q', torch.float64, ONE_KERNEL), ('eq', torch.float32, ONE_KERNEL), ('eq', torch.float64, ONE_KERNEL),
         ('band', torch.float32, BAND), ('band', torch.float64, BAND)]


@functools.lru_cache(maxsize=None)
def first(entry, position, dtype, geometry):
    return render(entry, position, dtype, *geometry)


@pytest.mark.parametrize('position', [0, 3 * N])
@pytest.mark.parametrize('entry,dtype,geometries', CASES)
def test_every_geometry_renders_the_same_bits(entry, dtype, geometries, position):
    want = first(entry, position, dtype, geometries[0])
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0.1
    for pad, blocks in geometries[1:]:
        got = render(entry, position, dtype, pad, blocks)
        differ = (got != want).any(dim=0).nonzero().flatten().tolist()
        assert not differ, f'{entry} {dtype} at {position}: {pad} columns of padding, per-block rows {blocks}: voices {differ[:8]} differ'


VOICES = [0, 1, 2, 3, 63, 64, 129, 191, 254, 255]        # every lane group at four, two and one voices per lane, both ends
BLOCKS = [0, 1, 2, K // 2, K - 2, K - 1]


def restated(entry, position, block):
    """block `block` at VOICES by the CPU restatements: (N, len(VOICES)) float64"""
    from oracle import chain_ref as R
    hist, x = signal(position)
    start = hist + block * N
    c = min(CTX, position + block * N)
    window = np.concatenate([x[start - c:start + N, VOICES], np.zeros((CTX, len(VOICES)))])      # (the `after` rows never reach the block)
    at = lambda name: CONTROLS[name][:, VOICES]
    btype = ENTRIES[entry]
    if entry in ('plain', 'env'):
        y = R.crit_filter(btype, window, at('cutoff'), RATE, N, CTX)
        return y * R.adsr(position + block * N, N, RATE, *(ADSR[k][:, VOICES] for k in _native.ADSR_PARAMS)) if entry == 'env' else y
    if entry == 'q':
        return RR.resonant_filter(btype, window, at('cutoff'), at('q'), RATE, N, CTX)
    if entry == 'eq':
        return EQ.eq_filter(btype[2:], window, at('cutoff'), at('q'), at('gain'), RATE, N, CTX)
    return R.band_filter(btype, window, at('low'), at('high'), RATE, N, CTX)


# the bound of the entry's existing test: tests/test_gpu_engine.py (C2 per node) and tests/test_gpu_eq.py 1e-6, the others 1e-6 of
# max(1, full scale) (tests/test_gpu_envelope_edges.py, tests/test_gpu_resonant.py, tests/test_gpu_swept_band.py)
ABSOLUTE = ('plain', 'eq')


@pytest.mark.parametrize('position', [0, 3 * N])
@pytest.mark.parametrize('entry,dtype,geometry', [(e, d, g[0]) for e, d, g in CASES] + [('band_blocks', torch.float32, (0, True))])
def test_first_geometry_against_the_restatement(entry, dtype, geometry, position):
    got = first(entry, position, dtype, geometry)
    picked = torch.tensor(VOICES, device=DEV)
    for block in BLOCKS:
        want = restated(entry, position, block)
        have = got[block * N:(block + 1) * N].index_select(1, picked).cpu().numpy().astype(np.float64)
        bound = 1e-6 if entry in ABSOLUTE else tolerance(want)
        err = maxerr(have, f32(want) if dtype == torch.float32 and entry != 'q' else want)   # (the resonant test holds both buffer types to the float64 rows)
        print('coldstart', entry, dtype, position, 'block', block, 'max|err|', err, 'bound', bound, 'max|oracle|', float(np.abs(want).max()))
        assert err <= bound, (entry, dtype, position, block, err, bound)
