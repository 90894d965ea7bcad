"""The patches of the mixed-program tests (tests/test_mixed_host.py, tests/test_gpu_mixed.py): voice graphs that combine two or more
of the extension families -- band filters, phase-modulation carriers, wavetable oscillators / waveshapers, resonant filters, unison
oscillators -- each built twice over the same rows: through signals_amd's node API and as the oracle graph composed from
oracle.chain_ref and the committed restatements (unison_reference, resonant_reference, shaper_reference, wavetable_reference,
pm_reference).

    supersaw      UnisonSawtooth -> ResonantLowPass
    supersaw_bus  UnisonSawtooth -> ResonantLowPass (cutoff and resonance on block-rate LFOs) -> x ADSR -> SumBus (stereo)
    overdrive     Sawtooth -> ResonantLowPass -> Shaper
    pad           Wavetable (T = 64, W = 2, per-voice select) -> ResonantLowPass
    bell          PMSine(mod = Sine) -> ResonantLowPass
    wah           Wavetable -> BandPass (low and high on a block-rate LFO)
    three         UnisonSawtooth -> ResonantLowPass -> Shaper -> SumBus (stereo): three families, tables and copies in one launch

Rows: resonance in [0.6, 2] keeps every filter's peak near the input's (the Shaper clips at +-1; behind the PM carrier the per-node
route's float32 modulator, index <= 0.25, stays inside the project's 1e-6 bar); hertz in [55, 1760], unison detune within 12 %, so
phases stay positive (v_fract_f64's corner is out of reach, as in test_gpu_unison.py)."""
import numpy as np

from helpers import RATE, fix, mkosc
import pm_reference as PR
import resonant_reference as RR
import shaper_reference as SR
import unison_reference as UR
import wavetable_reference as WR

PATCHES = ('supersaw', 'supersaw_bus', 'overdrive', 'pad', 'bell', 'wah', 'three')
SAW, SINE = 2, 0                                                              # _native.OSC_KINDS


def draw(V, seed=11):
    rng = np.random.default_rng(seed)
    th = rng.uniform(0, np.pi / 2, V)
    table = np.concatenate([WR.band_limited_saw(64, 9), np.sin(2 * np.pi * np.arange(64) / 64)[:, None] ** 3], axis=1)    # (64, 2)
    return dict(hertz=rng.uniform(55, 1760, (1, V)), phase=rng.uniform(0, 1, (1, V)), spread=rng.uniform(0, 1, (1, V)),
                cut=np.geomspace(150.0, 0.3 * RATE, V)[None, :], q=rng.uniform(0.6, 2.0, (1, V)),
                index=rng.uniform(0.0, 0.25, (1, V)), ratio=rng.uniform(0.5, 3.0, (1, V)),
                select=(np.arange(V) % 2).astype(float)[None, :], table=table, curve=SR.tanh_curve(257, 2.0),
                copies3=np.stack([rng.uniform(-0.12, 0.12, 3), rng.uniform(0, 1, 3)], axis=1),
                pan=np.stack([np.cos(th), np.sin(th)]),
                env=dict(attack=rng.uniform(0.002, 0.02, (1, V)), decay=rng.uniform(0.01, 0.05, (1, V)), sustain=rng.uniform(0.3, 0.9, (1, V)),
                         release=rng.uniform(0.01, 0.05, (1, V)), gate_on=rng.uniform(0.0, 0.01, (1, V)), gate_off=rng.uniform(0.04, 0.07, (1, V))))


def lfo_row(row, depth, hz):
    """row * (1 + depth * triangle(hz t)) as a block-rate control: (GPU node, oracle node) -- as in tests/test_gpu_resonant.py"""
    from oracle import chain_ref as R
    from signals_amd.chain import fx
    g = fx.Gain(); g.left = mkosc('Triangle', [[hz]]); g.right = fix(2.0 * depth * row)
    m = fx.Mix(); m.left = g; m.right = fix(2.0 * row); m.mix = fix([[0.5]])
    ref = R.Binary('Mix', R.Binary('Gain', R.Osc('Triangle', R.Fixed([[hz]])), R.Fixed(2.0 * depth * row)), R.Fixed(2.0 * row), R.Fixed([[0.5]]))
    return m, ref


def patch(which, p, copies=None, table=None):
    """(GPU node, oracle node, rendered width) of one patch over the rows `p`.  `copies` / `table`: the arrays both sides read
    (default: the node's seven copies, p['table']) -- an in-place edit reaches both"""
    from oracle import chain_ref as R
    from signals_amd.chain import ext, fx
    V = p['hertz'].shape[1]
    RF, WT, SH = RR.oracle_node(), WR.oracle_node(), SR.oracle_node()
    table = p['table'] if table is None else table

    def unison():
        u = ext.UnisonSawtooth()
        if copies is not None:
            u.get_state().copies = copies
        u.hertz = fix(p['hertz']); u.phase = fix(p['phase']); u.spread = fix(p['spread'])
        held = UR.default_copies() if copies is None else copies
        return u, UR.UnisonOsc('Sawtooth', held, R.Fixed(p['hertz']), R.Fixed(p['phase']), R.Fixed(p['spread']))

    def wavetable():
        w = ext.Wavetable(); w.get_state().table = table
        w.hertz = fix(p['hertz']); w.phase = fix(p['phase']); w.select = fix(p['select'])
        return w, WT(table, R.Fixed(p['hertz']), R.Fixed(p['phase']), R.Fixed(p['select']))

    def rlp(src, rsrc, cutoff=None, q=None):
        (c, rc), (r, rr) = cutoff or (fix(p['cut']), R.Fixed(p['cut'])), q or (fix(p['q']), R.Fixed(p['q']))
        f = ext.ResonantLowPass(); f.input = src; f.cutoff = c; f.resonance = r
        return f, RF('lp', rsrc, rc, rr)

    def shaper(src, rsrc):
        s = ext.Shaper(); s.get_state().table = p['curve']; s.input = src
        return s, SH(p['curve'], rsrc)

    def bus(src, rsrc):
        b = ext.SumBus(); b.input = src; b.get_state().gains = np.ascontiguousarray(p['pan'])
        return b, R.SumBus(rsrc, p['pan']), 2

    if which == 'supersaw':
        return (*rlp(*unison()), V)
    if which == 'supersaw_bus':
        f, rf = rlp(*unison(), cutoff=lfo_row(p['cut'], 0.2, 7.0), q=lfo_row(p['q'], 0.3, 11.0))
        env = ext.ADSR()
        for name, row in p['env'].items():
            setattr(env, name, fix(row))
        x = fx.RingMod(); x.left = f; x.right = env
        return bus(x, R.Binary('RingMod', rf, R.Adsr(**p['env'])))
    if which == 'overdrive':
        saw = mkosc('Sawtooth', p['hertz'], p['phase'])
        return (*shaper(*rlp(saw, R.Osc('Sawtooth', R.Fixed(p['hertz']), R.Fixed(p['phase'])))), V)
    if which == 'pad':
        return (*rlp(*wavetable()), V)
    if which == 'bell':
        c = ext.PMSine(); c.hertz = fix(p['hertz']); c.phase = fix(p['phase']); c.index = fix(p['index'])
        c.mod = mkosc('Sine', p['hertz'] * p['ratio'])
        rc = PR.PMOsc('Sine', R.Fixed(p['hertz']), R.Fixed(p['phase']), R.Fixed(p['index']), R.Osc('Sine', R.Fixed(p['hertz'] * p['ratio'])))
        return (*rlp(c, rc), V)
    if which == 'wah':
        w, rw = wavetable()
        (lo, rlo), (hi, rhi) = lfo_row(p['cut'] * 0.5, 0.3, 5.0), lfo_row(p['cut'] * 0.5 + 900.0, 0.3, 5.0)
        bp = fx.BandPass(); bp.input = w; bp.low = lo; bp.high = hi
        return bp, R.BandFilter('bp', rw, rlo, rhi), V
    if which == 'three':
        return bus(*shaper(*rlp(*unison())))
    raise KeyError(which)
