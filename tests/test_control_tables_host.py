"""Two tables that used to be kept by hand in two places each, checked without a GPU: the files a specialised image is keyed by
(`specialise._sources`: the quoted-include closure of the two kernels) and the extension nodes that are refused in a control path
(the `no_block_rate` column of `graph._FAMILIES`, worded by `_ControlProgram._emit` and `_Batch._control_node`)."""
import pathlib
import re
import shutil
import types
from unittest import mock

import pytest

from signals_amd import specialise
from signals_amd.chain import ext, files, fixed, fx, noise, osc, shape
from signals_amd.engine import NotBatchable, _Batch, _ControlProgram, graph


def closure(csrc: pathlib.Path) -> set:
    """names of the files the two kernels pull in with #include "...", from the source text alone"""
    seen, todo = set(), ['voice_program.hip', 'control_program.hip']
    while todo:
        path = csrc / todo.pop()
        name, path = path.name, path if path.exists() else csrc.parent.parent / 'include' / path.name
        if name not in seen:
            seen.add(name)
            todo += re.findall(r'#\s*include\s*"([^"]+)"', path.read_text())
    return seen


def test_the_digest_reads_the_include_closure():
    read = {pathlib.PurePath(name).name for name in specialise._sources()}
    assert read == closure(specialise.CSRC) | {'signals_amd.h'}
    assert {'sig_vp_launch.h', 'sig_vp_machine.h', 'sig_biquad.h', 'sig_common.h'} <= read      # (the first was missing from the hand-kept list)


def test_a_byte_of_an_included_header_changes_the_digest(tmp_path, monkeypatch):
    csrc = tmp_path / 'signals_amd' / 'csrc'
    csrc.mkdir(parents=True)
    for name in specialise._sources():                      # (the public header lies two directories up, in include/)
        (csrc / name).parent.mkdir(parents=True, exist_ok=True)
        shutil.copy(specialise.CSRC / name, csrc / name)
    monkeypatch.setattr(specialise, 'CSRC', csrc)
    before = specialise._source_digest()
    with open(csrc / 'sig_vp_launch.h', 'ab') as f:
        f.write(b' ')
    assert specialise._source_digest() != before


# what each refusal said before there was one table: class -> (what it is called, how the sentence ends)
EAGER = ' (the eager node serves one-frame requests)'
REFUSED = {ext.PMOsc: ('a phase-modulation oscillator', ' (its modulator is a frame-rate input)'), ext.Wavetable: ('a wavetable oscillator', EAGER),
           ext.UnisonOsc: ('a unison oscillator', EAGER), ext.Shaper: ('a waveshaper', EAGER), ext.ResonantFilter: ('a resonant filter', EAGER),
           ext.Ladder: ('a ladder filter', EAGER), ext.Delay: ('a delay line', EAGER), ext.Sampler: ('a sampler', EAGER),
           ext.FIR: ('a FIR filter', ' -- the eager node serves one-frame requests'), ext.Modal: ('a modal bank', EAGER)}


def node_of(cls):
    node = mock.Mock(spec=cls)
    node.cls_name.return_value = cls.__name__
    return node


def emit(node, window=False):
    return _ControlProgram._emit(types.SimpleNamespace(_reg={}, _window={}), node, window)


def test_both_sites_word_every_entry_as_before():
    refusing = {row.cls: row.no_block_rate for row in graph._FAMILIES if row.no_block_rate is not None}
    assert {cls for cls in refusing if not any(issubclass(cls, above) for above in refusing if above is not cls)} == set(REFUSED)
    assert all(refusing[cls] == next(said for family, said in REFUSED.items() if issubclass(cls, family)) for cls in refusing)
    batch = _Batch(types.SimpleNamespace(rate=48000), 0, 256, 4, False)
    for cls, (phrase, tail) in REFUSED.items():
        name, node = cls.__name__, node_of(cls)
        with pytest.raises(NotBatchable) as e:
            emit(node)
        assert str(e.value) == f'{name} in a control path: {phrase} has no block-rate program{tail}'
        with pytest.raises(NotBatchable) as e:
            emit(node, window=True)
        assert str(e.value) == (f'{name} inside a control filter\'s input: {phrase} has no window-rate program' if cls is ext.PMOsc else
                                f'{name} in a control path: {phrase} has no block-rate program{tail}')
        with pytest.raises(NotBatchable) as e:
            batch._control_node(node, 'cutoff')
        assert str(e.value) == f'cutoff: {name} in a control path: {phrase} has no block-rate schedule{tail}'


def test_every_known_class_is_emitted_or_in_the_table():
    def leaves(cls):
        below = cls.__subclasses__()
        return {cls} if not below else set().union(*(leaves(c) for c in below))
    generic, tabled, branched = set(), set(), set()
    for cls in set().union(*(leaves(t) for t in graph._KNOWN_TYPES)):
        try:
            emit(node_of(cls))
        except NotBatchable as e:
            if str(e).startswith('no block-rate program for'):
                generic.add(cls)
            elif ' has no block-rate program' in str(e):
                tabled.add(cls)
            else:
                branched.add(cls)                           # (a refusal of its own: the band filters')
        except (AttributeError, TypeError):                 # (a branch of its own took the mock and asked it for its ports)
            branched.add(cls)
    # the nodes of a graph's plumbing are no control sources; every other class has a branch in `_emit` or an entry in the table
    known = lambda c: next(k for k in graph._KNOWN_TYPES if issubclass(c, k))
    assert {known(c) for c in generic} == {ext.SumBus, ext.Tap, ext.MixMatrix, files.FileWriter, files.FileReader, shape.Merge}
    assert tabled == {c for c in set().union(*(leaves(t) for t in REFUSED)) if any(issubclass(c, k) for k in graph._KNOWN_TYPES)}
    assert {known(c) for c in branched} == {fixed.Fixed, osc.Osc, noise.White, fx.CritFilter, fx.Mix, fx.RingMod, fx.Gain, fx.Amp, ext.ADSR}
    assert {c for c in branched if issubclass(c, fx.CritFilter)} >= {fx.LowPass, fx.HighPass, fx.BandPass, fx.BandStop}
