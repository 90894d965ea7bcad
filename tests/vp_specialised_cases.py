"""The cases of tests/test_gpu_vp_specialised.py and tests/test_vp_specialised_cases_host.py: the voices, launch geometries and sinks
at which the SPECIALISED builds of the voice program (signals_amd/specialise.py: voice_program.hip compiled for one program, one
count of voices per lane and one sink) are rendered with more than one block per lane, two and four voices per lane, for all 13
kernel families.  Nothing here needs torch or a GPU at import time: the graphs are built inside the functions.

Voices.  Those of tests/vp_span_cases.py, 66 wide, blocks of N = 130 frames (the next block's chains start inside a row group),
two consecutive batches of 3 and 4 blocks from position 0:

    full          the family's voice times an ADSR (SIG_VP_S_EXT=1), every family.  A specialised image's register file is exact, so
                  the small-file voice -- the same words without the envelope -- would be a subset of this one and is left out
    swept         every family-specific control on a block-rate LFO, every family
    deep          two filters in series: plain, band, resonant, resonant_eq, mixed; also the `fresh` render (5 blocks from position
                  1000) and, for band, resonant_eq and mixed, the `short` one (blocks of 32 frames), on the images they already have

and, new here, for the four-voices-per-lane image (engine/voice_program.py asks for it only where a program keeps no filter state
and no temporaries):

    four          the family's oscillator -- with the Shaper over it for shape -- then a Gain, for plain, pm, table, shape, unison,
                  blep and sync: every family that has an oscillator word of its own, or sits on one without a filter.  (band,
                  resonant, resonant_eq and the three mixed families ARE their filter: no voice of theirs is without filter state.)
                  None of the seven needs a temporary: the PM carrier's modulator and the Shaper's input pass through the
                  accumulator.  68 voices: a multiple of 4, so the store is 16-byte aligned; two voice tiles at one voice per lane,
                  the second ragged, and 17 live lanes at four.  Under a bus the engine folds a constant Gain into the bus weights
                  (engine/batch.py _sched_bus), so the bus image is built for the program WITHOUT its last word: `launched` says so.

Images.  An image is keyed by (program, voices per lane, sink channels); the span is a run-time argument, so cells of different
spans share one.  CELLS lists per kind the (voices per lane, span, sink) of the long render:

    full          (1, 2) store | (2, 3) bus                                       2 images x 13
    swept, deep   (1, 2) store | (1, 2) bus | (2, 3) bus | (2, 16) store          4 images x (13 + 5)
    four          (4, 2) store | (4, 3) bus                                       2 images x 7

26 + 52 + 20 + 14 = IMAGES = 112 images, capped at MAX_IMAGES = 120 (each is a hipcc run of some seconds)."""
import numpy as np

import vp_span_cases as C

V4 = 68                                                                       # the four-per-lane voices' width
GAIN = (0.3, 1.0)                                                             # their Gain row, linear over the voices
SINKS = C.SINKS
KINDS = ('full', 'swept', 'deep', 'four')
FOUR = ('plain', 'pm', 'table', 'shape', 'unison', 'blep', 'sync')
# (voices per lane, blocks per lane, sink) of the long render, per kind
CELLS = {'full': ((1, 2, 'store'), (2, 3, 'bus2')),
         'swept': ((1, 2, 'store'), (1, 2, 'bus2'), (2, 3, 'bus2'), (2, 16, 'store')),
         'deep': ((1, 2, 'store'), (1, 2, 'bus2'), (2, 3, 'bus2'), (2, 16, 'store')),
         'four': ((4, 2, 'store'), (4, 3, 'bus2'))}
IMAGES, MAX_IMAGES = 112, 120
# the variant and register file sig_voice_program_variant answers for the four-per-lane voices (all fit the small file)
FOUR_VARIANT = {'plain': ('plain', True), 'pm': ('pm', True), 'table': ('table', True), 'shape': ('shape', True),
                'unison': ('unison', True), 'blep': ('blep', True), 'sync': ('blep', True)}
# the family switches (-DSIG_VP_S_<name>=1) an image of each family is built with, and no others: what its words call for.
# (OscBlep and OscSync sit on the unison family's copies, FilterEq on the resonant design; sync has no OscBlep word of its own.)
SWITCHES = {'plain': (), 'band': (), 'pm': (), 'table': ('TAB',), 'shape': ('TAB',), 'resonant': ('RES',), 'unison': ('UNI',),
            'blep': ('UNI', 'BLEP'), 'mixed': ('RES', 'UNI', 'MIXED'), 'resonant_eq': ('RES', 'EQ'),
            'mixed_eq': ('RES', 'EQ', 'UNI', 'MIXED'), 'sync': ('UNI', 'SYNC'), 'mixed_sync': ('RES', 'UNI', 'SYNC', 'MIXED')}
ALL_SWITCHES = ('TAB', 'RES', 'EQ', 'UNI', 'BLEP', 'SYNC', 'MIXED')


def voices():
    """every (kind, family) of the table: 13 + 13 + 5 + 7"""
    from test_gpu_vp_variants import FAMILIES
    return ([(kind, family) for kind in ('full', 'swept') for family in FAMILIES] + [('deep', family) for family in C.DEEP] +
            [('four', family) for family in FOUR])


def width(kind):
    return V4 if kind == 'four' else C.V


def aligned(kind):
    """what sig_voice_program_geometry is told about the store: (rows, 68) float32 from the allocator is 16-byte aligned, (rows, 66)
    8-byte"""
    return 4 if kind == 'four' else 2


def rows4(shift=0):
    """the four-per-lane voices' parameter rows (mixed_patches.draw(68) and the Gain row); `shift`: voice v gets voice v + shift's"""
    import mixed_patches as MP
    p = MP.draw(V4)
    p['gain'] = np.linspace(*GAIN, V4)[None, :]
    for name in ('hertz', 'phase', 'spread', 'index', 'ratio', 'select', 'gain'):
        p[name] = np.roll(p[name], -shift, axis=1)
    return p


def four(family, shift=0):
    """(GPU node, oracle node) of the family's voice without filter state or temporaries: its oscillator (under the Shaper for
    shape), then a Gain"""
    import blep_reference as BR
    import pm_reference as PR
    import shaper_reference as SR
    import sync_reference as SY
    import unison_reference as UR
    import wavetable_reference as WR
    from helpers import fix, mkosc
    from oracle import chain_ref as R
    from signals_amd.chain import ext, fx
    p = rows4(shift)
    hz, ph = p['hertz'], p['phase']

    def saw():
        return mkosc('Sawtooth', hz, ph), R.Osc('Sawtooth', R.Fixed(hz), R.Fixed(ph))

    def spread(cls, ref_cls, copies, **more):
        u = cls(); u.hertz = fix(hz); u.phase = fix(ph); u.spread = fix(p['spread'])
        if copies is None:
            copies = UR.default_copies()
        else:
            u.get_state().copies = copies
        for name, row in more.items():
            setattr(u, name, fix(row))
        return u, ref_cls('Sawtooth', copies, R.Fixed(hz), R.Fixed(ph), R.Fixed(p['spread']), *[R.Fixed(row) for row in more.values()])

    if family == 'plain':
        src, rsrc = saw()
    elif family == 'pm':
        src = ext.PMSine(); src.hertz = fix(hz); src.phase = fix(ph); src.index = fix(p['index']); src.mod = mkosc('Sine', hz * p['ratio'])
        rsrc = PR.PMOsc('Sine', R.Fixed(hz), R.Fixed(ph), R.Fixed(p['index']), R.Osc('Sine', R.Fixed(hz * p['ratio'])))
    elif family == 'table':
        src = ext.Wavetable(); src.get_state().table = p['table']; src.hertz = fix(hz); src.phase = fix(ph); src.select = fix(p['select'])
        rsrc = WR.oracle_node()(p['table'], R.Fixed(hz), R.Fixed(ph), R.Fixed(p['select']))
    elif family == 'shape':
        inner, rinner = saw()
        src = ext.Shaper(); src.get_state().table = p['curve']; src.input = inner
        rsrc = SR.oracle_node()(p['curve'], rinner)
    elif family == 'unison':
        src, rsrc = spread(ext.UnisonSawtooth, UR.UnisonOsc, None)
    elif family == 'blep':                                                    # (three detuned copies: the default single one has no spread)
        src, rsrc = spread(ext.BlepSawtooth, BR.BlepOsc, p['copies3'])
    elif family == 'sync':                                                    # ratio 1.5 .. 4: the slave is reset inside its cycle
        src, rsrc = spread(ext.SyncSawtooth, SY.SyncOsc, p['copies3'], ratio=1.0 + p['ratio'])
    else:
        raise KeyError(family)
    g = fx.Gain(); g.left = src; g.right = fix(p['gain'])
    return g, R.Binary('Gain', rsrc, R.Fixed(p['gain']))


def build(kind, family):
    """(GPU node, oracle node) of one voice, a fresh graph at every call"""
    return four(family) if kind == 'four' else C.build(kind, family)


def variant(kind, family):
    """(the variant sig_voice_program_variant must name, small register file?)"""
    return FOUR_VARIANT[family] if kind == 'four' else C.variant(kind, family)


def pan(kind):
    """the 2-channel bus's weights, (2, voices)"""
    import mixed_patches as MP
    return MP.draw(width(kind))['pan']


def oracle(ref, kind, render, position=None):
    """the oracle's voice rows of one of vp_span_cases.RENDERS, float64 (blocks * frames, voices); `position`: another start"""
    from oracle import chain_ref as R
    start, frames, ks = C.RENDERS[render]
    return R.render_stream(ref, start if position is None else position, frames, sum(ks), width(kind))


def launched(kind, family, sink):
    """the voice as the engine compiles it for one sink (a _VoiceProgram): under a bus a constant Gain on top -- the four-per-lane
    voices have one -- is folded into the bus weights and the program is the Gain's input alone, which one node suffices for"""
    from signals_amd.engine import _VoiceProgram
    node = build(kind, family)[0]
    if sink != 'store' and kind == 'four':
        node = node.left.sig
    prog = _VoiceProgram.compile(None, node, width(kind), min_nodes=2 if sink == 'store' else 1, mixed=True)
    assert prog is not None, (kind, family, sink)
    return prog


def image_args(kind, family, vpl, sink):
    """what specialise.build and specialise.flags take for one image"""
    prog = launched(kind, family, sink)
    return prog.code, len(prog.oscs), len(prog.params), len(prog.filters), prog.n_temps, vpl, SINKS[sink]


def images():
    """every (kind, family, voices per lane, sink) an image is built for"""
    return sorted({(kind, family, vpl, sink) for kind, family in voices() for vpl, _, sink in CELLS[kind]})


def cells():
    """every cell of the long render: (kind, family, voices per lane, span, sink)"""
    return [(kind, family, vpl, span, sink) for kind, family in voices() for vpl, span, sink in CELLS[kind]]
