"""The engine's table of node families (`graph._FAMILIES`) against what the hand-kept ladders answered before there was a table,
written down class by class: the ports read at block rate and at frame rate, plugin or not, the refusal in a control path on
either route, the refusal of a voice program.  No GPU."""
import inspect

import pytest

from signals_amd import SignalFlags
from signals_amd.chain import BlockCachingEmitter, ImplicitChannels, Receiver, ext, files, fixed, fx, noise, osc, port, shape, vis
from signals_amd.engine import _audio_ports, _control_ports, _foreign, graph

OSC, PM, TABLE = ('hertz', 'phase'), ('hertz', 'phase', 'index'), ('hertz', 'phase', 'select')
UNISON, SYNC = ('hertz', 'phase', 'spread'), ('hertz', 'phase', 'spread', 'ratio')
Q, EQ = ('cutoff', 'resonance'), ('cutoff', 'resonance', 'gain')
EAGER = ' (the eager node serves one-frame requests)'
FRAME_RATE = ' (its modulator is a frame-rate input)'

# class -> (control ports, audio ports, what a control path calls it | None, how that refusal ends, what a voice program calls it | None)
EXPECTED = {
    fixed.Fixed: ((), (), None, '', None),
    osc.Sine: (OSC, (), None, '', None),
    osc.Square: (OSC, (), None, '', None),
    osc.Sawtooth: (OSC, (), None, '', None),
    osc.Triangle: (OSC, (), None, '', None),
    ext.PMSine: (PM, ('mod',), 'a phase-modulation oscillator', FRAME_RATE, None),
    ext.PMSquare: (PM, ('mod',), 'a phase-modulation oscillator', FRAME_RATE, None),
    ext.PMSawtooth: (PM, ('mod',), 'a phase-modulation oscillator', FRAME_RATE, None),
    ext.PMTriangle: (PM, ('mod',), 'a phase-modulation oscillator', FRAME_RATE, None),
    ext.Wavetable: (TABLE, (), 'a wavetable oscillator', EAGER, None),
    ext.Additive: (TABLE, (), 'a wavetable oscillator', EAGER, 'an additive oscillator'),
    ext.UnisonSine: (UNISON, (), 'a unison oscillator', EAGER, None),
    ext.UnisonSquare: (UNISON, (), 'a unison oscillator', EAGER, None),
    ext.UnisonSawtooth: (UNISON, (), 'a unison oscillator', EAGER, None),
    ext.UnisonTriangle: (UNISON, (), 'a unison oscillator', EAGER, None),
    ext.BlepSquare: (UNISON, (), 'a unison oscillator', EAGER, None),
    ext.BlepSawtooth: (UNISON, (), 'a unison oscillator', EAGER, None),
    ext.BlepTriangle: (UNISON, (), 'a unison oscillator', EAGER, None),
    ext.SyncSawtooth: (SYNC, (), 'a unison oscillator', EAGER, None),
    ext.SyncSquare: (SYNC, (), 'a unison oscillator', EAGER, None),
    noise.White: ((), (), None, '', None),
    fx.LowPass: (('cutoff',), ('input',), None, '', None),
    fx.HighPass: (('cutoff',), ('input',), None, '', None),
    fx.BandPass: (('low', 'high'), ('input',), None, '', None),
    fx.BandStop: (('low', 'high'), ('input',), None, '', None),
    ext.ResonantLowPass: (Q, ('input',), 'a resonant filter', EAGER, None),
    ext.ResonantHighPass: (Q, ('input',), 'a resonant filter', EAGER, None),
    ext.ResonantBandPass: (Q, ('input',), 'a resonant filter', EAGER, None),
    ext.Notch: (Q, ('input',), 'a resonant filter', EAGER, None),
    ext.AllPass: (Q, ('input',), 'a resonant filter', EAGER, None),
    ext.Peaking: (EQ, ('input',), 'a resonant filter', EAGER, None),
    ext.LowShelf: (EQ, ('input',), 'a resonant filter', EAGER, None),
    ext.HighShelf: (EQ, ('input',), 'a resonant filter', EAGER, None),
    ext.Ladder: (('cutoff', 'resonance', 'drive'), ('input',), 'a ladder filter', EAGER, None),
    ext.FIR: (('select',), ('input',), 'a FIR filter', ' -- the eager node serves one-frame requests', None),
    fx.Mix: (('mix',), ('left', 'right'), None, '', None),
    fx.RingMod: ((), ('left', 'right'), None, '', None),
    fx.Gain: (('right',), ('left',), None, '', None),
    fx.Amp: (('right',), ('left',), None, '', None),
    ext.Shaper: (('select',), ('input',), 'a waveshaper', EAGER, None),
    ext.Delay: (('time',), ('input',), 'a delay line', EAGER, None),
    ext.Sampler: (('ratio', 'offset', 'gate_on', 'select'), (), 'a sampler', EAGER, None),
    ext.Modal: (('hertz', 'gate_on', 'damp', 'select'), (), 'a modal bank', EAGER, 'a modal bank'),
    ext.SumBus: ((), ('input',), None, '', None),
    ext.Tap: ((), ('input',), None, '', None),
    vis.Vis: ((), ('input',), None, '', None),
    vis.Wave: ((), ('input',), None, '', None),
    vis.Spec: ((), ('input',), None, '', None),
    files.FileWriter: ((), ('input',), None, '', None),
    files.FileReader: ((), (), None, '', None),
    ext.ADSR: (('attack', 'decay', 'sustain', 'release', 'gate_on', 'gate_off'), (), None, '', None),
    ext.MixMatrix: ((), ('input',), None, '', None),
    shape.Merge: ((), ('left', 'right'), None, '', None),
}


def concrete(cls) -> set:
    """the package's classes at and below `cls` that can be instantiated (a test module may have defined plugins of its own)"""
    here = {cls} if not inspect.isabstract(cls) and cls.__module__.startswith('signals_amd.') else set()
    return here.union(*(concrete(c) for c in cls.__subclasses__()))


class Plugin(BlockCachingEmitter, ImplicitChannels):
    """a node class of the test's own: the table has no row for it"""
    hertz: Receiver.BoundPort = port('hertz')
    input: Receiver.BoundPort = port('input')

    @classmethod
    def flags(cls):
        return super().flags() | SignalFlags.EFFECT

    def _eval(self, request):
        raise NotImplementedError


def test_the_literals_name_every_class_under_the_table():
    assert set().union(*(concrete(row.cls) for row in graph._FAMILIES)) == set(EXPECTED)


@pytest.mark.parametrize('cls', list(EXPECTED), ids=lambda cls: cls.__name__)
def test_a_class_reads_and_refuses_what_its_ladder_branch_did(cls):
    control, audio, phrase, tail, word = EXPECTED[cls]
    node = cls()
    name = node.cls_name()
    assert _control_ports(node) == [getattr(node, p) for p in control]
    assert _audio_ports(node) == [getattr(node, p) for p in audio]
    assert _foreign(node) is False
    for route in ('program', 'schedule'):
        assert graph._no_block_rate(node, route) == (
            None if phrase is None else f'{name} in a control path: {phrase} has no block-rate {route}{tail}')
        assert graph._no_block_rate(node, route, window=True) == (
            f'{name} inside a control filter\'s input: {phrase} has no window-rate {route}' if isinstance(node, ext.PMOsc) else
            graph._no_block_rate(node, route))
    assert graph._no_voice_program(node) == (None if word is None else f'{name}: {word} has no voice-program word')


def test_a_plugin_is_foreign_and_reads_nothing_the_engine_knows_of():
    node = Plugin()
    assert _foreign(node) is True and _control_ports(node) == [] and _audio_ports(node) == []
    assert graph._no_block_rate(node, 'program') is None and graph._no_block_rate(node, 'schedule') is None
    assert graph._no_voice_program(node) is None
    assert graph._modulated(node) is False and graph._is_pure(node, {}) is False
