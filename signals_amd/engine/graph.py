"""What the engine asks of a node graph before it schedules it: which ports a node reads at block rate and at frame rate,
whether a control holds for every block, whether a node's reply depends on the request that produced it -- all read from one
table of node families, `_FAMILIES`."""
from __future__ import annotations

import typing

from signals_amd import _native
from signals_amd.chain import Emitter, Receiver
from signals_amd.chain import ext, files, fixed, fx, noise, osc, shape

CONTEXT = 100
SCAN_MAX_CHAINS = 16384      # signals_amd/csrc/sig_fused_scan.h: kScanMaxChains
SCAN_MAX_ROWS = 512          # kScanMaxL * 64


class NotBatchable(Exception):
    """This graph needs the eager pull path."""


class _Family(typing.NamedTuple):
    """what the engine knows of a node class and the classes below it"""
    cls: type
    control: tuple = ()                      # names of the ports read with forward_at_block_rate
    audio: tuple = ()                        # names of the ports read at frame rate
    window: bool = False                     # takes a filter's window: request-dependent, min(100, position) history rows
    own_width: bool = False                  # asks its audio ports with their own widths, not the request's
    no_block_rate: tuple | None = None       # not evaluated in a control path: (what a refusal calls it, the refusal's tail)
    no_window_rate: bool = False             # ... and inside a control filter's input the refusal is about the window rate
    no_program: str | None = None            # what the refusal of a voice program calls it: the family has no voice-program word


_EAGER = ' (the eager node serves one-frame requests)'
_FILTER = dict(audio=('input',), window=True)
_UNISON = dict(no_block_rate=('a unison oscillator', _EAGER))
_TABLE = dict(control=('hertz', 'phase', 'select'), no_block_rate=('a wavetable oscillator', _EAGER))
_RESONANT = dict(no_block_rate=('a resonant filter', _EAGER), **_FILTER)

# One row per node family, the most derived class first: a node's row is the first whose class it is an instance of.  The rows
# whose class has no other row's class above it are the families with a kernel schedule (`_KNOWN_TYPES`; `_Batch._SCHEDULES` has
# one entry for each, batch.py checks that).  A class with no row is a plugin (`_foreign`).
_FAMILIES = (
    _Family(fixed.Fixed),
    _Family(osc.Osc, control=('hertz', 'phase')),
    _Family(ext.PMOsc, control=('hertz', 'phase', 'index'), audio=('mod',), no_window_rate=True,
            no_block_rate=('a phase-modulation oscillator', ' (its modulator is a frame-rate input)')),
    _Family(ext.Additive, no_program='an additive oscillator', **_TABLE),     # (a Wavetable to isinstance, but OscTable is not its word)
    _Family(ext.Wavetable, **_TABLE),
    _Family(ext.SyncOsc, control=('hertz', 'phase', 'spread', 'ratio'), **_UNISON),
    _Family(ext.UnisonOsc, control=('hertz', 'phase', 'spread'), **_UNISON),
    _Family(noise.White),
    _Family(ext.GainEqFilter, control=('cutoff', 'resonance', 'gain'), **_RESONANT),
    _Family(ext.ResonantFilter, control=('cutoff', 'resonance'), **_RESONANT),
    _Family(ext.Ladder, control=('cutoff', 'resonance', 'drive'), no_block_rate=('a ladder filter', _EAGER), **_FILTER),
    _Family(ext.FIR, control=('select',), no_block_rate=('a FIR filter', ' -- the eager node serves one-frame requests'), **_FILTER),
    _Family(fx.SingleCritFilter, control=('cutoff',), **_FILTER),
    _Family(fx.DoubleCritFilter, control=('low', 'high'), **_FILTER),
    _Family(fx.CritFilter, **_FILTER),
    _Family(fx.Mix, control=('mix',), audio=('left', 'right')),
    _Family(fx.RingMod, audio=('left', 'right')),
    _Family(fx.Gain, control=('right',), audio=('left',)),
    _Family(fx.Amp, control=('right',), audio=('left',)),
    _Family(ext.Shaper, control=('select',), audio=('input',), no_block_rate=('a waveshaper', _EAGER)),
    _Family(ext.Delay, control=('time',), no_block_rate=('a delay line', _EAGER), **_FILTER),       # (a delay line takes a filter's window)
    _Family(ext.Sampler, control=('ratio', 'offset', 'gate_on', 'select'), no_block_rate=('a sampler', _EAGER)),
    _Family(ext.Modal, control=('hertz', 'gate_on', 'damp', 'select'), no_block_rate=('a modal bank', _EAGER), no_program='a modal bank'),
    _Family(ext.SumBus, audio=('input',), own_width=True),
    _Family(ext.Tap, audio=('input',)),
    _Family(files.FileWriter, audio=('input',)),
    _Family(files.FileReader),
    _Family(ext.ADSR, control=tuple(_native.ADSR_PARAMS)),
    _Family(ext.MixMatrix, audio=('input',)),
    _Family(shape.Merge, audio=('left', 'right'), own_width=True),
)
_PLUGIN = _Family(object)                    # what a class without a row reads: nothing the engine knows of

# the node classes with a kernel schedule, one entry of _Batch._SCHEDULES each
_KNOWN_TYPES = tuple(row.cls for row in _FAMILIES if not any(issubclass(row.cls, other.cls) for other in _FAMILIES if other is not row))

_ROW_OF: dict[type, _Family] = {}


def _family(node: Emitter) -> _Family:
    """the table's row of a node, `_PLUGIN` for a class the table does not hold; looked up once per class"""
    cls = node.__class__                     # (not type(): a test's mock stands for the class it is a spec of)
    if cls not in _ROW_OF:
        _ROW_OF[cls] = next((row for row in _FAMILIES if isinstance(node, row.cls)), _PLUGIN)
    return _ROW_OF[cls]


def _no_block_rate(node: Emitter, route: str, window: bool = False) -> str | None:
    """the refusal of a node in a control path whose family is not evaluated at block rate, None for any other node; `route`:
    'program' | 'schedule', what the refusing site would have run; `window`: inside a control filter's input, where a frame-rate
    input has its own wording (its modulator would have to be a window-rate input)"""
    row = _family(node)
    if row.no_block_rate is None:
        return None
    phrase, tail = row.no_block_rate
    if window and row.no_window_rate:
        return f'{node.cls_name()} inside a control filter\'s input: {phrase} has no window-rate {route}'
    return f'{node.cls_name()} in a control path: {phrase} has no block-rate {route}{tail}'


def _no_voice_program(node: Emitter) -> str | None:
    """the refusal of a node whose family has no voice-program word, None for any other node"""
    phrase = _family(node).no_program
    return None if phrase is None else f'{node.cls_name()}: {phrase} has no voice-program word'


def _ctl_const(port: Receiver.BoundPort) -> bool:
    """a control port whose value cannot change from block to block: unplugged, disabled, or a Fixed"""
    src = port.sig
    return src is None or not src.get_state().enabled or isinstance(src, fixed.Fixed)


def _ctl_unplugged(port: Receiver.BoundPort) -> bool:
    """a control port that reads zeros((1, 1)): nothing plugged, or a disabled source"""
    return port.sig is None or not port.sig.get_state().enabled


def _control_ports(node: Emitter) -> list:
    """ports a node reads with forward_at_block_rate"""
    return [getattr(node, name) for name in _family(node).control]


def _audio_ports(node: Emitter) -> list:
    """ports a node reads at frame rate"""
    return [getattr(node, name) for name in _family(node).audio]


def _modulated(node: Emitter | None) -> bool:
    """some control input of this node is re-evaluated every block (an LFO on a cutoff, FM at block rate ...):
    its reply to a block then depends on which request produced it, like a filter's (the block-rate value is
    read at the REQUEST's position, chain/__init__.py:305-306), so its history rows come from tails, not from
    re-rendering"""
    return node is not None and any(not _ctl_const(p) for p in _control_ports(node))


def _foreign(node: Emitter) -> bool:
    """a node class the engine has no kernel schedule for -- a plugin written against the node API; it is pulled block by
    block through its own respond(), so its reply may depend on the request like a filter's"""
    return _family(node) is _PLUGIN


def _is_pure(node: Emitter | None, memo: dict) -> bool:
    """position-pure: no filter and no per-block control anywhere upstream on the audio path, so any row
    range can be rendered in one launch and history rows can simply be re-rendered"""
    if node is None or not node.get_state().enabled:
        return True
    if node not in memo:
        memo[node] = True       # cycles are rejected elsewhere
        if _family(node).window or _modulated(node) or _foreign(node):
            memo[node] = False
        else:
            memo[node] = all(_is_pure(p.sig, memo) for p in _audio_ports(node))
    return memo[node]
