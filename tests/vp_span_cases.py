"""The cases of tests/test_gpu_vp_spans.py and tests/test_vp_span_cases_host.py: the voices, shapes and launch geometries that put a
block boundary INSIDE a lane's span of the voice-program interpreter (signals_amd/csrc/sig_vp_machine.h), for all 13 kernel families.
Nothing here needs torch or a GPU at import time: the graphs are built inside the functions.

Voices, 66 wide over the rows of mixed_patches.draw(66) (cutoffs geometric from 150 Hz: the 100-row context matters):

    small, full   test_gpu_vp_variants.voice(family, False | True), every family
    swept         one per family: every control row the family's own word reads follows a block-rate triangle LFO
                  (mixed_patches.lfo_row), so it differs in every block -- see `swept`; the band-limited and hard-sync
                  oscillators get three detuned copies there (their default single copy has no spread to sweep)
    deep          two filters in series, fixed controls, for plain, band, resonant, resonant_eq and mixed; the first eight voices'
                  inner filters are slow (20 .. 120 Hz), the outer ones' 150 .. 30 Hz, as in tests/test_gpu_voice_program.py
                  test_cascades_follow_the_block_cache_history, so that the block history in front of a batch matters -- see `deep`

Shapes.  Long blocks: N = 130 frames at 48 kHz.  (130 - 100) % 4 = 2 and (130 - 100) % 8 = 6: the first warm row of the next block's
chains falls inside a row group in both register files (4 rows per group in the full file, 8 in the small one); 130 % 4 = 130 % 8 = 2:
every block ends in single-row groups.  Two consecutive batches of 3 and 4 blocks from position 0; for the deep voices also one batch
of 5 blocks from position 1000 (no block multiple: the render starts from virtual history blocks).  Short blocks: N = 32, 3 blocks.

The LFOs are triangles of 5 .. 12 Hz: over the 7 blocks (19 ms) they stay inside their first, rising quarter period, so no later
block repeats an earlier block's row."""
import contextlib

import numpy as np

V, N, KS, POSITION, CONTEXT = 66, 130, (3, 4), 0, 100
ROW_GROUPS = (4, 8)                                                           # rows per dispatch: the full and the small register file
GEOMETRIES = ((1, 2), (2, 3), (2, 16))                                        # (voices per lane, blocks per lane)
# the blocks each lane owns, per (span, batch size): what the geometries are chosen for (`owned` computes it)
OWNED = {(2, 3): [[0, 1], [2]], (2, 4): [[0, 1], [2, 3]],                     # a ragged last span | two full ones
         (3, 3): [[0, 1, 2]], (3, 4): [[0, 1, 2], [3]],                       # one lane, three blocks | a lone last block
         (16, 3): [[0, 1, 2]], (16, 4): [[0, 1, 2, 3]],                       # the span exceeds the batch: one lane walks it all
         (2, 5): [[0, 1], [2, 3], [4]]}                                       # the fresh start
FRESH = (1000, 5, (1, 2))                                                     # position, blocks, geometry: the deep voices' mid-stream start
SHORT_N, SHORT_K = 32, 3
SHORT_CELLS = ((2, 'bus2'), (1, 'store'))                                     # (voices per lane, sink); the span is 1 in short-block mode
SINKS = {'store': 0, 'bus2': 2}
KINDS = ('small', 'full', 'swept')
DEEP = ('plain', 'band', 'resonant', 'resonant_eq', 'mixed')
SHORT_DEEP = ('band', 'resonant_eq', 'mixed')
# (position, block frames, batch sizes) of the three renders
RENDERS = {'long': (POSITION, N, KS), 'fresh': (FRESH[0], N, (FRESH[1],)), 'short': (0, SHORT_N, (SHORT_K,))}

# the variant and register file sig_voice_program_variant must answer for the swept and the deep voices (family, small file?); the
# small and full voices' are (BASE.get(family, family), not full) as in tests/test_gpu_vp_variants.py
VARIANT = {
    ('swept', 'plain'): ('plain', True), ('swept', 'band'): ('band', True), ('swept', 'pm'): ('pm', True),
    ('swept', 'table'): ('table', True), ('swept', 'shape'): ('shape', True), ('swept', 'resonant'): ('resonant', True),
    ('swept', 'unison'): ('unison', True), ('swept', 'blep'): ('blep', True), ('swept', 'mixed'): ('mixed', False),
    ('swept', 'resonant_eq'): ('resonant', True), ('swept', 'mixed_eq'): ('mixed', True), ('swept', 'sync'): ('blep', True),
    ('swept', 'mixed_sync'): ('mixed', True),
    ('deep', 'plain'): ('plain', True), ('deep', 'band'): ('band', False), ('deep', 'resonant'): ('resonant', True),
    ('deep', 'resonant_eq'): ('resonant', False), ('deep', 'mixed'): ('mixed', True),
}
# the controls each swept voice sweeps: what `swept` returns handles for
SWEPT = {'plain': ('cutoff',), 'band': ('low', 'high'), 'pm': ('index', 'hertz'), 'table': ('select', 'hertz'), 'shape': ('cutoff',),
         'resonant': ('cutoff', 'resonance'), 'unison': ('spread', 'hertz'), 'blep': ('spread', 'hertz'),
         'mixed': ('cutoff', 'resonance'), 'resonant_eq': ('cutoff', 'resonance', 'gain'), 'mixed_eq': ('cutoff', 'resonance', 'gain'),
         'sync': ('ratio', 'spread'), 'mixed_sync': ('ratio', 'spread')}


def voices():
    """every (kind, family) rendered at long blocks: 13 x 3 + 5"""
    from test_gpu_vp_variants import FAMILIES
    return [(kind, family) for kind in KINDS for family in FAMILIES] + [('deep', family) for family in DEEP]


def owned(span, K):
    """the blocks of a batch of K each lane owns: lane g starts at block g * span (sig_vp_machine.h: b_first, nb)"""
    return [list(range(first, min(first + span, K))) for first in range(0, K, span)]


def select_row():
    """a select row just under the boundary between the table's two columns (floor(select) picks the column): times the LFO's
    1 .. 1.33 each voice crosses 1.0 in a block of its own, some between blocks 0 and 1, some between blocks 3 and 4"""
    return np.linspace(0.70, 0.99, V)[None, :]


def gain_row():
    """test_gpu_vp_variants.eq_gain() moved off 0 dB, where a product with the LFO would hold still: -10.5, 1.5, 13.5 dB"""
    from test_gpu_vp_variants import eq_gain
    return eq_gain() + 1.5


def swept(family):
    """(GPU node, oracle node, {control: (oracle node, port)}) of the family's swept voice; the handles name where the oracle graph
    reads each swept control, for `freeze`"""
    import blep_reference as BR
    import eq_reference as EQ
    import mixed_patches as MP
    import pm_reference as PR
    import resonant_reference as RR
    import shaper_reference as SR
    import sync_reference as SY
    import unison_reference as UR
    import wavetable_reference as WR
    from helpers import fix, mkosc
    from oracle import chain_ref as R
    from signals_amd.chain import ext, fx
    p = MP.draw(V)
    hz, ph, cut = p['hertz'], p['phase'], p['cut']
    lfo = MP.lfo_row

    def saw():
        return mkosc('Sawtooth', hz, ph), R.Osc('Sawtooth', R.Fixed(hz), R.Fixed(ph))

    def lowpass(src, rsrc, cutoff=None):
        c, rc = cutoff or (fix(cut), R.Fixed(cut))
        f = fx.LowPass(); f.input = src; f.cutoff = c
        return f, R.Filter('lp', rsrc, rc)

    def spread(cls, ref_cls, copies, sweep_hertz, **more):
        """a unison-like oscillator with a swept spread (and hertz, or what `more` plugs: (GPU node, oracle node) per port);
        `copies` None: the node's own seven, else the array both sides read"""
        (s, rs), (h, rh) = lfo(p['spread'], 0.5, 12.0), (lfo(hz, 0.1, 9.0) if sweep_hertz else (fix(hz), R.Fixed(hz)))
        u = cls(); u.hertz = h; u.phase = fix(ph); u.spread = s
        if copies is None:
            copies = UR.default_copies()
        else:
            u.get_state().copies = copies
        for name, (ctl, _) in more.items():
            setattr(u, name, ctl)
        return u, ref_cls('Sawtooth', copies, rh, R.Fixed(ph), rs, *[r for _, r in more.values()])

    if family == 'plain':                                                     # test_gpu_vp_variants' voice, the low-pass swept
        hz2, cut2 = hz[:, ::-1] * 0.5, cut[:, ::-1]
        hp = fx.HighPass(); hp.input = mkosc('Triangle', hz2); hp.cutoff = fix(cut2)
        a, ra = lowpass(*saw(), cutoff=lfo(cut, 0.2, 7.0))
        node = fx.RingMod(); node.left = a; node.right = hp
        ref = R.Binary('RingMod', ra, R.Filter('hp', R.Osc('Triangle', R.Fixed(hz2)), R.Fixed(cut2)))
        return node, ref, {'cutoff': (ra, 'cutoff')}
    if family == 'band':                                                      # mixed_patches' `wah`: one LFO for both edges, low < high in every block
        (lo, rlo), (hi, rhi) = lfo(cut * 0.5, 0.25, 5.0), lfo(cut * 0.5 + 900.0, 0.25, 5.0)
        src, rsrc = saw()
        node = fx.BandPass(); node.input = src; node.low = lo; node.high = hi
        ref = R.BandFilter('bp', rsrc, rlo, rhi)
        return node, ref, {'low': (ref, 'low'), 'high': (ref, 'high')}
    if family == 'pm':
        (ix, rix), (h, rh) = lfo(p['index'], 0.5, 12.0), lfo(hz, 0.1, 9.0)
        c = ext.PMSine(); c.hertz = h; c.phase = fix(ph); c.index = ix; c.mod = mkosc('Sine', hz * p['ratio'])
        rc = PR.PMOsc('Sine', rh, R.Fixed(ph), rix, R.Osc('Sine', R.Fixed(hz * p['ratio'])))
        return (*lowpass(c, rc), {'index': (rc, 'index'), 'hertz': (rc, 'hertz')})
    if family == 'table':
        (sel, rsel), (h, rh) = lfo(select_row(), 0.5, 10.0), lfo(hz, 0.1, 9.0)
        w = ext.Wavetable(); w.get_state().table = p['table']; w.hertz = h; w.phase = fix(ph); w.select = sel
        rw = WR.oracle_node()(p['table'], rh, R.Fixed(ph), rsel)
        return (*lowpass(w, rw), {'select': (rw, 'select'), 'hertz': (rw, 'hertz')})
    if family == 'shape':
        src, rsrc = lowpass(*saw(), cutoff=lfo(cut, 0.2, 7.0))
        node = ext.Shaper(); node.get_state().table = p['curve']; node.input = src
        return node, SR.oracle_node()(p['curve'], rsrc), {'cutoff': (rsrc, 'cutoff')}
    if family in ('resonant', 'mixed_sync'):                                  # tests/test_gpu_resonant.py's `swept` | tests/test_gpu_sync.py's `resonant`
        if family == 'resonant':
            (src, rsrc), (c, rc), (q, rq) = saw(), lfo(cut, 0.2, 7.0), lfo(p['q'], 0.4, 11.0)
        else:
            src, rsrc = spread(ext.SyncSawtooth, SY.SyncOsc, p['copies3'], False, ratio=lfo(1.0 + p['ratio'], 0.2, 9.0))
            (c, rc), (q, rq) = (fix(cut), R.Fixed(cut)), (fix(p['q']), R.Fixed(p['q']))
        node = ext.ResonantLowPass(); node.input = src; node.cutoff = c; node.resonance = q
        ref = RR.oracle_node()('lp', rsrc, rc, rq)
        if family == 'resonant':
            return node, ref, {'cutoff': (ref, 'cutoff'), 'resonance': (ref, 'resonance')}
        return node, ref, {'ratio': (rsrc, 'ratio'), 'spread': (rsrc, 'spread')}
    if family in ('unison', 'blep'):
        # (the band-limited and the hard-sync nodes' default is ONE clean copy, which no spread moves: three detuned ones)
        cls, ref_cls, copies = ((ext.UnisonSawtooth, UR.UnisonOsc, None) if family == 'unison' else
                                (ext.BlepSawtooth, BR.BlepOsc, p['copies3']))
        src, rsrc = spread(cls, ref_cls, copies, True)
        return (*lowpass(src, rsrc), {'spread': (rsrc, 'spread'), 'hertz': (rsrc, 'hertz')})
    if family == 'sync':
        src, rsrc = spread(ext.SyncSawtooth, SY.SyncOsc, p['copies3'], False, ratio=lfo(1.0 + p['ratio'], 0.2, 9.0))
        return (*lowpass(src, rsrc), {'ratio': (rsrc, 'ratio'), 'spread': (rsrc, 'spread')})
    if family == 'mixed':                                                     # mixed_patches' `supersaw_bus` without its bus
        bus, rbus, _ = MP.patch('supersaw_bus', p)
        node, ref = bus.input.sig, rbus.inputs['input']
        del bus.input                                                         # (the voice has no reader left outside the graph)
        rf = ref.inputs['left']
        return node, ref, {'cutoff': (rf, 'cutoff'), 'resonance': (rf, 'resonance')}
    if family in ('resonant_eq', 'mixed_eq'):                                 # test_gpu_vp_variants' voices, cutoff, q and gain swept
        if family == 'resonant_eq':
            (src, rsrc), kind, cls = saw(), 'peak', ext.Peaking
        else:
            u = ext.UnisonSawtooth(); u.hertz = fix(hz); u.phase = fix(ph); u.spread = fix(p['spread'])
            src, rsrc = u, UR.UnisonOsc('Sawtooth', UR.default_copies(), R.Fixed(hz), R.Fixed(ph), R.Fixed(p['spread']))
            kind, cls = 'ls', ext.LowShelf
        level = np.full((1, V), 0.25)
        (c, rc), (q, rq), (db, rdb) = lfo(cut, 0.2, 7.0), lfo(p['q'], 0.4, 11.0), lfo(gain_row(), 0.3, 9.0)
        g = fx.Gain(); g.left = src; g.right = fix(level)
        node = cls(); node.input = g; node.cutoff = c; node.resonance = q; node.gain = db
        ref = EQ.oracle_node()(kind, R.Binary('Gain', rsrc, R.Fixed(level)), rc, rq, rdb)
        return node, ref, {'cutoff': (ref, 'cutoff'), 'resonance': (ref, 'resonance'), 'gain': (ref, 'gain')}
    raise KeyError(family)


def freeze(handles, control, position):
    """hold one swept control of an oracle graph at the row it has at `position`: what a kernel that did not reload the row for
    the later blocks of its span would compute with"""
    from oracle import chain_ref as R
    node, port = handles[control]
    node.inputs[port] = R.Fixed(R.render(node.inputs[port], position, 1, V))


def deep(family):
    """(GPU node, oracle node) of the family's voice with two filters in series, fixed controls"""
    import eq_reference as EQ
    import mixed_patches as MP
    import resonant_reference as RR
    import unison_reference as UR
    from helpers import fix, mkosc
    from oracle import chain_ref as R
    from signals_amd.chain import ext, fx
    from test_gpu_vp_variants import eq_gain
    p = MP.draw(V)
    hz, ph = p['hertz'], p['phase']
    inner, outer = p['cut'].copy(), p['cut'][:, ::-1].copy()
    inner[0, :8] = np.linspace(20.0, 120.0, 8)                                # slow filters: the block history matters
    outer[0, :8] = np.linspace(150.0, 30.0, 8)
    q2 = np.roll(p['q'], 1, axis=1)
    src, rsrc = mkosc('Sawtooth', hz, ph), R.Osc('Sawtooth', R.Fixed(hz), R.Fixed(ph))

    def single(cls, btype, x, rx):
        f = cls(); f.input = x; f.cutoff = fix(outer)
        return f, R.Filter(btype, rx, R.Fixed(outer))

    def resonant(cls, btype, x, rx, cutoff, q):
        f = cls(); f.input = x; f.cutoff = fix(cutoff); f.resonance = fix(q)
        return f, RR.oracle_node()(btype, rx, R.Fixed(cutoff), R.Fixed(q))

    def eq(cls, kind, x, rx, cutoff, q, db):
        f = cls(); f.input = x; f.cutoff = fix(cutoff); f.resonance = fix(q); f.gain = fix(db)
        return f, EQ.oracle_node()(kind, rx, R.Fixed(cutoff), R.Fixed(q), R.Fixed(db))

    if family == 'plain':                                                     # LowPass -> HighPass
        lp = fx.LowPass(); lp.input = src; lp.cutoff = fix(inner)
        return single(fx.HighPass, 'hp', lp, R.Filter('lp', rsrc, R.Fixed(inner)))
    if family == 'band':                                                      # BandPass -> LowPass
        low, high = inner * 0.5, inner * 0.5 + 900.0
        bp = fx.BandPass(); bp.input = src; bp.low = fix(low); bp.high = fix(high)
        return single(fx.LowPass, 'lp', bp, R.BandFilter('bp', rsrc, R.Fixed(low), R.Fixed(high)))
    if family == 'resonant':                                                  # tests/test_gpu_resonant.py's `hp_lp`
        return resonant(ext.ResonantLowPass, 'lp', *resonant(ext.ResonantHighPass, 'hp', src, rsrc, inner, p['q']), outer, q2)
    if family == 'resonant_eq':                                               # Peaking -> LowShelf, the source at 0.25
        level, db = np.full((1, V), 0.25), eq_gain()
        g = fx.Gain(); g.left = src; g.right = fix(level)
        peak = eq(ext.Peaking, 'peak', g, R.Binary('Gain', rsrc, R.Fixed(level)), inner, p['q'], db)
        return eq(ext.LowShelf, 'ls', *peak, outer, q2, np.roll(db, 1, axis=1))
    if family == 'mixed':                                                     # UnisonSawtooth -> ResonantLowPass -> LowPass
        u = ext.UnisonSawtooth(); u.hertz = fix(hz); u.phase = fix(ph); u.spread = fix(p['spread'])
        ru = UR.UnisonOsc('Sawtooth', UR.default_copies(), R.Fixed(hz), R.Fixed(ph), R.Fixed(p['spread']))
        return single(fx.LowPass, 'lp', *resonant(ext.ResonantLowPass, 'lp', u, ru, inner, p['q']))
    raise KeyError(family)


def build(kind, family):
    """(GPU node, oracle node) of one voice, a fresh graph at every call"""
    if kind == 'swept':
        return swept(family)[:2]
    if kind == 'deep':
        return deep(family)
    from test_gpu_vp_variants import voice
    return voice(family, kind == 'full')


def variant(kind, family):
    """(the variant sig_voice_program_variant must name, small register file?)"""
    if (kind, family) in VARIANT:
        return VARIANT[kind, family]
    from test_gpu_vp_variants import BASE
    return BASE.get(family, family), kind == 'small'


def oracle(ref, render):
    """the oracle's voice rows of one of RENDERS, float64 (blocks * frames, V): consecutive blocks from one graph, as the reference
    is driven"""
    from oracle import chain_ref as R
    position, frames, ks = RENDERS[render]
    return R.render_stream(ref, position, frames, sum(ks), V)


@contextlib.contextmanager
def context_rows(rows):
    """the oracle with every filter cold-started on `rows` rows of context instead of chain_ref.CONTEXT_FRAMES: the constant the
    nodes ask their windows with, and the `ctx` default each filter function keeps its block with"""
    import eq_reference as EQ
    import resonant_reference as RR
    from oracle import chain_ref as R
    functions = (R.crit_filter, R.band_filter, RR.resonant_filter, EQ.eq_filter)
    was = R.CONTEXT_FRAMES
    for f in functions:
        assert f.__defaults__ == (was,), f                                     # `ctx` is the one positional default of each
    try:
        R.CONTEXT_FRAMES = rows
        for f in functions:
            f.__defaults__ = (rows,)
        yield
    finally:
        R.CONTEXT_FRAMES = was
        for f in functions:
            f.__defaults__ = (was,)
