"""Every cell of the voice-program interpreter's launch table, rendered once: 13 families (plain, band, pm, table, shape, resonant,
unison, blep, mixed, resonant_eq, mixed_eq, sync, mixed_sync) x {small, full register file} x voices per lane {1, 2} x sink {store,
1-channel bus, 2-channel bus} = the 156 kernels of vp_<family>.hip, each against the CPU oracle its family's own GPU test uses
(oracle/chain_ref.py and the committed restatements tests/*_reference.py; tests/mixed_patches.py for mixed).  FAMILIES is the list
of sig_vp_launch.h's VpLaunch instantiations: tests/test_vp_variant_host.py holds the two equal on every machine.

Shape: 66 voices (two voice tiles at one voice per lane, the second ragged; even, so two per lane is allowed), blocks of 128 frames
(just over the 100-row filter context: the current and the next block's chains both run), 3 blocks from position 0, 48 kHz.

Short blocks (test_short_cell): the same voices in blocks of 32 frames, shorter than the context, so that the kernels' `small`
branch runs (span 1, the chain re-walked from history; every voice here has a filter, depth > 0, or the branch would not be taken):
each family at both register files in the most composite cell, two voices per lane under the 2-channel bus -- history re-walk, lane
pairs and bus flush together.  26 cells, none left out.

Graphs: per family the smallest voice no fused kernel takes, with its words inside the small register file; the full register file
is the same voice times an ADSR envelope (an extended word).  Before a cell is rendered sig_voice_program_variant must name its
family and register file and sig_voice_program_geometry its voices per lane, and afterwards the batch must have been exactly one
voice_program launch: no cell can pass by running another kernel.

The _eq and _sync sets: sig_voice_program_variant answers the nine base variants only; a FilterEq or an OscSync word picks the
second kernel set of that variant at the launch (voice_program.hip vp_launch_call: resonant -> resonant_eq, blep -> sync, mixed ->
mixed_eq or mixed_sync).  So for these four families a cell asserts the base variant (BASE) and that the one launch's label -- the
program's words, `voice_program[OscSync,FilterQ]` -- has the word that selects the set and the words that make it the single-family
or the mixed one (WORDS).  The earlier sets have no handler for either word: a program that reached one of them would skip the word
and miss the oracle.

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
SHORT_N = 32                                                                  # < CONTEXT: the kernels' `small` mode
FAMILIES = ('plain', 'band', 'pm', 'table', 'shape', 'resonant', 'unison', 'blep', 'mixed', 'resonant_eq', 'mixed_eq', 'sync', 'mixed_sync')
SINKS = {'store': 0, 'bus1': 1, 'bus2': 2}
# the second kernel sets: the variant sig_voice_program_variant answers for their programs ...
BASE = {'resonant_eq': 'resonant', 'mixed_eq': 'mixed', 'sync': 'blep', 'mixed_sync': 'mixed'}
# ... and (the words the launch label must have, the words it must not have): what vp_launch_call selects the set by
WORDS = {'resonant_eq': (('FilterEq',), ('OscUni', 'OscSync')), 'mixed_eq': (('FilterEq', 'OscUni'), ('OscSync',)),
         'sync': (('OscSync',), ('FilterQ', 'FilterEq')), 'mixed_sync': (('OscSync', 'FilterQ'), ('FilterEq',))}
EQ_GAINS = (-12.0, 0.0, 12.0)                                                 # dB, tests/test_gpu_eq.py's


def eq_gain():
    """the equaliser voices' gain row: mixed_patches.draw has none; dealt by the voice index as tests/test_gpu_eq.py deals its own"""
    return np.array([EQ_GAINS[(v // 3) % 3] for v in range(V)])[None, :]


def voice(family, full):
    """(GPU node, oracle node) of one family's voice over the rows of mixed_patches.draw"""
    import blep_reference as BR
    import eq_reference as EQ
    import pm_reference as PR
    import resonant_reference as RR
    import shaper_reference as SR
    import sync_reference as SY
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
    elif family in ('resonant_eq', 'mixed_eq'):                               # tests/test_gpu_eq.py's voice: the source at 0.25 into a gained kind
        src, rsrc = saw() if family == 'resonant_eq' else spread(ext.UnisonSawtooth, UR.UnisonOsc, UR.default_copies())
        kind, cls = ('peak', ext.Peaking) if family == 'resonant_eq' else ('ls', ext.LowShelf)
        level, db = np.full((1, V), 0.25), eq_gain()
        g = fx.Gain(); g.left = src; g.right = fix(level)
        node = cls(); node.input = g; node.cutoff = fix(cut); node.resonance = fix(p['q']); node.gain = fix(db)
        ref = EQ.oracle_node()(kind, R.Binary('Gain', rsrc, R.Fixed(level)), R.Fixed(cut), R.Fixed(p['q']), R.Fixed(db))
    elif family in ('sync', 'mixed_sync'):                                    # ratio 1.5 .. 4: the slave is reset inside its cycle
        ratio = 1.0 + p['ratio']
        src = ext.SyncSawtooth(); src.hertz = fix(hz); src.phase = fix(ph); src.spread = fix(p['spread']); src.ratio = fix(ratio)
        rsrc = SY.SyncOsc('Sawtooth', SY.default_copies(), R.Fixed(hz), R.Fixed(ph), R.Fixed(p['spread']), R.Fixed(ratio))
        if family == 'sync':
            node, ref = lowpass(src, rsrc)
        else:                                                                 # tests/test_gpu_sync.py's `resonant` patch
            node = ext.ResonantLowPass(); node.input = src; node.cutoff = fix(cut); node.resonance = fix(p['q'])
            ref = RR.oracle_node()('lp', rsrc, R.Fixed(cut), R.Fixed(p['q']))
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
def wanted(family, full, frames=N):
    """the oracle's voice rows (K * frames, V) of one family, register file and block length, float64: shared by its cells"""
    from oracle import chain_ref as R
    _, ref = voice(family, full)
    want = R.render_stream(ref, POSITION, frames, K, V)
    want.setflags(write=False)
    return want


def program(family, full):
    """the voice as the engine compiles it: (words, (oscs, params, filters, temps), depth)"""
    from signals_amd.engine import _VoiceProgram
    node, _ = voice(family, full)
    prog = _VoiceProgram.compile(None, node, V, mixed=True)
    assert prog is not None, (family, full)
    return prog.code, (len(prog.oscs), len(prog.params), len(prog.filters), prog.n_temps), prog.depth


def check_cell(family, full, vpl, sink, frames=N):
    """no silent collapse: this program is launched in this family's kernel (for the second sets: in its base variant's, see
    check_label for the rest), this register file, with this many voices per lane"""
    from signals_amd import _native
    code, counts, depth = program(family, full)
    assert _native.voice_program_variant(code, *counts) == (BASE.get(family, family), not full), (family, full, code)
    aligned = 2                                                               # (rows, 66) float32 from the allocator: 8-byte aligned, even
    assert _native.voice_program_geometry(V, frames, K, CONTEXT, depth, SINKS[sink], aligned)[0] == vpl, (family, full, vpl, sink)
    return depth


def check_label(family, sink, names):
    """exactly one interpreter launch; for the second kernel sets, with the words that select the set"""
    label = 'voice_program[' if sink == 'store' else 'voice_program_bus['
    assert len(names) == 1 and names[0].startswith(label) and '*specialised' not in names[0], (family, sink, names)
    if family in WORDS:
        words = names[0][len(label):names[0].index(']')].split(',')
        have, have_not = WORDS[family]
        assert all(w in words for w in have) and not any(w in words for w in have_not), (family, sink, names)


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    from gpu_helpers import gpu_ready
    from signals_amd import _native
    gpu_ready()
    yield
    _native.set_voice_program_tuning(0, 0)
    _native.voice_program_use_attached(True)


def render_cell(family, full, vpl, sink, frames, what):
    """one cell: the checks before the launch, the one launch, its label, the rows against the oracle's"""
    import torch
    from oracle import chain_ref as R
    from signals_amd import _native, runtime
    from signals_amd.chain import ext
    from signals_amd.engine import BatchRenderer, KernelTimer
    rows = wanted(family, full, frames)
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
        depth = check_cell(family, full, vpl, sink, frames)
        timer = KernelTimer()
        got = BatchRenderer(top, C, RATE, timer=timer, fuse_program='always', mixed_programs=True,
                            specialise=False).render(POSITION, frames, K).cpu().numpy()   # (whatever SIG_SPECIALISE says)
        torch.cuda.synchronize()
        runtime.check_status()
    finally:
        _native.set_voice_program_tuning(0, 0)
        _native.voice_program_use_attached(True)
    names = [rec[0] for rec in timer.records]
    check_label(family, sink, names)
    err = maxerr(got, f32(want))
    print(what, family, 'full' if full else 'small', vpl, sink, 'max|err|', err, 'tol', tol, names)
    assert got.shape == want.shape and err <= tol, (family, full, vpl, sink, frames, err, tol)
    return depth


@pytest.mark.parametrize('sink', list(SINKS))
@pytest.mark.parametrize('vpl', [1, 2])
@pytest.mark.parametrize('full', [False, True], ids=['small', 'full'])
@pytest.mark.parametrize('family', FAMILIES)
def test_cell(family, full, vpl, sink):
    render_cell(family, full, vpl, sink, N, 'vp variant')


@pytest.mark.parametrize('full', [False, True], ids=['small', 'full'])
@pytest.mark.parametrize('family', FAMILIES)
def test_short_cell(family, full):
    """blocks of 32 frames, two voices per lane, the 2-channel bus: the `small` branch of every family's kernel at both register
    files.  The voice must have a filter (depth > 0) or the branch is not taken, and the geometry must answer span 1"""
    from signals_amd import _native
    _, _, depth = program(family, full)
    assert depth > 0, (family, full)
    _native.set_voice_program_tuning(2, 0)
    try:
        assert _native.voice_program_geometry(V, SHORT_N, K, CONTEXT, depth, 2, 2) == (2, 1), (family, full, depth)
    finally:
        _native.set_voice_program_tuning(0, 0)
    assert render_cell(family, full, 2, 'bus2', SHORT_N, 'vp short block') == depth


