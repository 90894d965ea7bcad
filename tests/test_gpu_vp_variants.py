"""Every cell of the voice-program interpreter's launch table, rendered once: 9 families (plain, band, pm, table, shape, resonant,
unison, blep, mixed) x {small, full register file} x voices per lane {1, 2} x sink {store, 1-channel bus, 2-channel bus} = the 108
kernels of vp_<family>.hip, each against the CPU oracle its family's own GPU test uses (oracle/chain_ref.py and the committed
restatements tests/*_reference.py; tests/mixed_patches.py for mixed).

Shape: 66 voices (two voice tiles at one voice per lane, the second ragged; even, so two per lane is allowed), blocks of 128 frames
(just over the 100-row filter context: the current and the next block's chains both run), 3 blocks from position 0, 48 kHz.

Graphs: per family the smallest voice no fused kernel takes, with its words inside the small register file; the full register file
is the same voice times an ADSR envelope (an extended word).  Before a cell is rendered sig_voice_program_variant must name its
family and register file and sig_voice_program_geometry its voices per lane, and afterwards the batch must have been exactly one
voice_program launch: no cell can pass by running another kernel.

Tolerance: 1e-6 max(1, max|oracle|) on the float32 output against float32(oracle), the families' bar (tests/test_gpu_mixed.py
`tolerance`, which tests/test_gpu_resonant.py, _unison, _blep, _wavetable, _swept_band, _voice_program and -- for a carrier whose
modulator is computed inside the program -- _pm apply too); behind the Shaper times max(1, L), L the curve's Lipschitz constant
(tests/test_gpu_shaper.py).  No sample is excluded."""
import functools

import numpy as np
import pytest

from helpers import RATE, f32, fix, maxerr, mkosc
import mixed_patches as MP
from test_gpu_mixed import tolerance

pytestmark = pytest.mark.gpu

V, N, K, POSITION, CONTEXT = 66, 128, 3, 0, 100
FAMILIES = ('plain', 'band', 'pm', 'table', 'shape', 'resonant', 'unison', 'blep', 'mixed')
SINKS = {'store': 0, 'bus1': 1, 'bus2': 2}


def voice(family, full):
    """(GPU node, oracle node) of one family's voice over the rows of mixed_patches.draw"""
    import blep_reference as BR
    import pm_reference as PR
    import resonant_reference as RR
    import shaper_reference as SR
    import unison_reference as UR
    import wavetable_reference as WR
    from oracle import chain_ref as R
    from signals_amd.chain import ext, fx
    p = MP.draw(V)
    hz, ph, cut = p['hertz'], p['phase'], p['cut']

    def lowpass(src, rsrc):
        f = fx.LowPass(); f.input = src; f.cutoff = fix(cut)
        return f, R.Filter('lp', rsrc, R.Fixed(cut))

    def saw():
        return mkosc('Sawtooth', hz, ph), R.Osc('Sawtooth', R.Fixed(hz), R.Fixed(ph))

    def spread(cls, ref_cls, copies):
        u = cls(); u.hertz = fix(hz); u.phase = fix(ph); u.spread = fix(p['spread'])
        return u, ref_cls('Sawtooth', copies, R.Fixed(hz), R.Fixed(ph), R.Fixed(p['spread']))

    if family == 'plain':                                                     # (a lone Filter(Osc) is a fused kernel's: RingMod of two)
        hz2, cut2 = hz[:, ::-1] * 0.5, cut[:, ::-1]
        hp = fx.HighPass(); hp.input = mkosc('Triangle', hz2); hp.cutoff = fix(cut2)
        a, ra = lowpass(*saw())
        node = fx.RingMod(); node.left = a; node.right = hp
        ref = R.Binary('RingMod', ra, R.Filter('hp', R.Osc('Triangle', R.Fixed(hz2)), R.Fixed(cut2)))
    elif family == 'band':
        low, high = cut * 0.5, cut * 0.5 + 900.0
        src, rsrc = saw()
        node = fx.BandPass(); node.input = src; node.low = fix(low); node.high = fix(high)
        ref = R.BandFilter('bp', rsrc, R.Fixed(low), R.Fixed(high))
    elif family == 'pm':
        c = ext.PMSine(); c.hertz = fix(hz); c.phase = fix(ph); c.index = fix(p['index']); c.mod = mkosc('Sine', hz * p['ratio'])
        rc = PR.PMOsc('Sine', R.Fixed(hz), R.Fixed(ph), R.Fixed(p['index']), R.Osc('Sine', R.Fixed(hz * p['ratio'])))
        node, ref = lowpass(c, rc)
    elif family == 'table':
        w = ext.Wavetable(); w.get_state().table = p['table']; w.hertz = fix(hz); w.phase = fix(ph); w.select = fix(p['select'])
        node, ref = lowpass(w, WR.oracle_node()(p['table'], R.Fixed(hz), R.Fixed(ph), R.Fixed(p['select'])))
    elif family == 'shape':
        src, rsrc = lowpass(*saw())
        node = ext.Shaper(); node.get_state().table = p['curve']; node.input = src
        ref = SR.oracle_node()(p['curve'], rsrc)
    elif family == 'resonant':
        src, rsrc = saw()
        node = ext.ResonantLowPass(); node.input = src; node.cutoff = fix(cut); node.resonance = fix(p['q'])
        ref = RR.oracle_node()('lp', rsrc, R.Fixed(cut), R.Fixed(p['q']))
    elif family == 'unison':
        node, ref = lowpass(*spread(ext.UnisonSawtooth, UR.UnisonOsc, UR.default_copies()))
    elif family == 'blep':
        node, ref = lowpass(*spread(ext.BlepSawtooth, BR.BlepOsc, BR.default_copies()))
    elif family == 'mixed':
        node, ref, _ = MP.patch('supersaw', p)                                # UnisonSawtooth -> ResonantLowPass
    else:
        raise KeyError(family)
    if full:
        env = ext.ADSR()
        for name, row in p['env'].items():
            setattr(env, name, fix(row))
        x = fx.RingMod(); x.left = node; x.right = env
        node, ref = x, R.Binary('RingMod', ref, R.Adsr(**p['env']))
    return node, ref


def scale(family):
    if family != 'shape':
        return 1.0
    import shaper_reference as SR
    return max(1.0, SR.lipschitz(MP.draw(V)['curve']))


@functools.lru_cache(maxsize=None)
def wanted(family, full):
    """the oracle's voice rows (K * N, V) of one family and register file, float64: shared by its six cells"""
    from oracle import chain_ref as R
    _, ref = voice(family, full)
    want = R.render_stream(ref, POSITION, N, K, V)
    want.setflags(write=False)
    return want


def program(family, full):
    """the voice as the engine compiles it: (words, (oscs, params, filters, temps), depth)"""
    from signals_amd.engine import _VoiceProgram
    node, _ = voice(family, full)
    prog = _VoiceProgram.compile(None, node, V, mixed=True)
    assert prog is not None, (family, full)
    return prog.code, (len(prog.oscs), len(prog.params), len(prog.filters), prog.n_temps), prog.depth


def check_cell(family, full, vpl, sink):
    """no silent collapse: this program is launched in this family's kernel, this register file, with this many voices per lane"""
    from signals_amd import _native
    code, counts, depth = program(family, full)
    assert _native.voice_program_variant(code, *counts) == (family, not full), (family, full, code)
    aligned = 2                                                               # (rows, 66) float32 from the allocator: 8-byte aligned, even
    assert _native.voice_program_geometry(V, N, K, CONTEXT, depth, SINKS[sink], aligned)[0] == vpl, (family, full, vpl, sink)


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    import torch
    assert torch.cuda.is_available()
    from signals_amd import _native, runtime
    runtime.set_device('cuda:0')
    _native.lib()
    yield
    _native.set_voice_program_tuning(0, 0)
    _native.voice_program_use_attached(True)


@pytest.mark.parametrize('sink', list(SINKS))
@pytest.mark.parametrize('vpl', [1, 2])
@pytest.mark.parametrize('full', [False, True], ids=['small', 'full'])
@pytest.mark.parametrize('family', FAMILIES)
def test_cell(family, full, vpl, sink):
    import torch
    from oracle import chain_ref as R
    from signals_amd import _native, runtime
    from signals_amd.chain import ext
    from signals_amd.engine import BatchRenderer, KernelTimer
    rows = wanted(family, full)
    pan = MP.draw(V)['pan']
    node, _ = voice(family, full)
    if sink == 'store':
        top, C, want = node, V, rows
    else:
        top = ext.SumBus(); top.input = node
        C = SINKS[sink]
        if sink == 'bus2':
            top.get_state().gains = np.ascontiguousarray(pan)
        want = R.sum_bus(rows, pan if sink == 'bus2' else None)
    tol = tolerance(want) * scale(family)
    _native.set_voice_program_tuning(vpl, 0)
    _native.voice_program_use_attached(False)                                 # the interpreter, whatever image another test attached
    try:
        check_cell(family, full, vpl, sink)
        timer = KernelTimer()
        got = BatchRenderer(top, C, RATE, timer=timer, fuse_program='always', mixed_programs=True,
                            specialise=False).render(POSITION, N, K).cpu().numpy()        # (whatever SIG_SPECIALISE says)
        torch.cuda.synchronize()
        runtime.check_status()
    finally:
        _native.set_voice_program_tuning(0, 0)
        _native.voice_program_use_attached(True)
    names = [rec[0] for rec in timer.records]
    label = 'voice_program[' if sink == 'store' else 'voice_program_bus['
    assert len(names) == 1 and names[0].startswith(label) and '*specialised' not in names[0], (family, full, vpl, sink, names)
    err = maxerr(got, f32(want))
    print('vp variant', family, 'full' if full else 'small', vpl, sink, 'max|err|', err, 'tol', tol, names)
    assert got.shape == want.shape and err <= tol, (family, full, vpl, sink, err, tol)
