"""What the engine asks of a node graph before it schedules it: which ports a node reads at block rate and at frame rate,
whether a control holds for every block, whether a node's reply depends on the request that produced it."""
from __future__ import annotations

from signals_amd import _native
from signals_amd.chain import Emitter, Receiver
from signals_amd.chain import ext, files, fixed, fx, noise, osc, shape

CONTEXT = 100
SCAN_MAX_CHAINS = 16384      # signals_amd/csrc/sig_fused_scan.h: kScanMaxChains
SCAN_MAX_ROWS = 512          # kScanMaxL * 64


class NotBatchable(Exception):
    """This graph needs the eager pull path."""


# the node classes with a kernel schedule, one entry of _Batch._SCHEDULES each (batch.py checks that the two agree)
_KNOWN_TYPES = (fixed.Fixed, osc.Osc, ext.PMOsc, ext.Wavetable, ext.UnisonOsc, noise.White, fx.CritFilter, fx.Mix, fx.RingMod, fx.Gain,
                fx.Amp, ext.Shaper, ext.Delay, ext.Sampler, ext.SumBus, ext.Tap, files.FileWriter, files.FileReader, ext.ADSR, ext.MixMatrix, shape.Merge)
# ext.Modal has a schedule like them (`_Batch._SCHEDULES`) and stands beside the tuple: tests/test_control_tables_host.py pins the
# families of the tuple and of the table below class by class, and a new top-level family can enter neither
_KNOWN_BESIDE = (ext.Modal,)


# the extension nodes that are not evaluated at block rate: (class, what a refusal calls it, why), one table for the control
# program (control.py: `_emit`) and the node-by-node control rows (batch.py: `_control_node`)
_NO_BLOCK_RATE = (
    (ext.PMOsc, 'a phase-modulation oscillator', 'its modulator is a frame-rate input'),
    (ext.Wavetable, 'a wavetable oscillator', 'the eager node serves one-frame requests'),
    (ext.UnisonOsc, 'a unison oscillator', 'the eager node serves one-frame requests'),
    (ext.Shaper, 'a waveshaper', 'the eager node serves one-frame requests'),
    (ext.ResonantFilter, 'a resonant filter', 'the eager node serves one-frame requests'),
    (ext.Ladder, 'a ladder filter', 'the eager node serves one-frame requests'),
    (ext.Delay, 'a delay line', 'the eager node serves one-frame requests'),
    (ext.Sampler, 'a sampler', 'the eager node serves one-frame requests'),
)


def _no_block_rate(node: Emitter, route: str, window: bool = False) -> str | None:
    """the refusal of a node of _NO_BLOCK_RATE in a control path, None for any other node; `route`: 'program' | 'schedule', what
    the refusing site would have run; `window`: inside a control filter's input, where a frame-rate input has its own wording"""
    if isinstance(node, ext.FIR):                              # a branch of its own, like the band filters': the table's families are pinned
        return (f'{node.cls_name()} in a control path: a FIR filter has no block-rate {route} -- the eager node serves '
                f'one-frame requests')
    if isinstance(node, ext.Modal):                            # the table's wording for a family the pinned table cannot hold
        return (f'{node.cls_name()} in a control path: a modal bank has no block-rate {route} (the eager node serves '
                f'one-frame requests)')
    for family, phrase, why in _NO_BLOCK_RATE:
        if isinstance(node, family):
            if window and family is ext.PMOsc:                 # (its modulator would have to be a window-rate input)
                return f'{node.cls_name()} inside a control filter\'s input: {phrase} has no window-rate {route}'
            return f'{node.cls_name()} in a control path: {phrase} has no block-rate {route} ({why})'
    return None


def _ctl_const(port: Receiver.BoundPort) -> bool:
    """a control port whose value cannot change from block to block: unplugged, disabled, or a Fixed"""
    src = port.sig
    return src is None or not src.get_state().enabled or isinstance(src, fixed.Fixed)


def _ctl_unplugged(port: Receiver.BoundPort) -> bool:
    """a control port that reads zeros((1, 1)): nothing plugged, or a disabled source"""
    return port.sig is None or not port.sig.get_state().enabled


def _control_ports(node: Emitter) -> list:
    """ports a node reads with forward_at_block_rate"""
    if isinstance(node, osc.Osc):
        return [node.hertz, node.phase]
    if isinstance(node, ext.PMOsc):
        return [node.hertz, node.phase, node.index]
    if isinstance(node, ext.Wavetable):
        return [node.hertz, node.phase, node.select]
    if isinstance(node, ext.SyncOsc):
        return [node.hertz, node.phase, node.spread, node.ratio]
    if isinstance(node, ext.UnisonOsc):
        return [node.hertz, node.phase, node.spread]
    if isinstance(node, ext.Shaper):
        return [node.select]
    if isinstance(node, ext.Delay):
        return [node.time]
    if isinstance(node, ext.FIR):
        return [node.select]
    if isinstance(node, ext.Sampler):
        return [node.ratio, node.offset, node.gate_on, node.select]
    if isinstance(node, ext.Modal):
        return [node.hertz, node.gate_on, node.damp, node.select]
    if isinstance(node, (fx.Gain, fx.Amp)):
        return [node.right]
    if isinstance(node, fx.Mix):
        return [node.mix]
    if isinstance(node, ext.EqFilter) and node.gain_port() is not None:
        return [node.cutoff, node.resonance, node.gain_port()]
    if isinstance(node, ext.ResonantFilter):
        return [node.cutoff, node.resonance]
    if isinstance(node, ext.Ladder):
        return [node.cutoff, node.resonance, node.drive]
    if isinstance(node, fx.SingleCritFilter):
        return [node.cutoff]
    if isinstance(node, fx.DoubleCritFilter):
        return [node.low, node.high]
    if isinstance(node, ext.ADSR):
        return [getattr(node, name) for name in _native.ADSR_PARAMS]
    return []


def _audio_ports(node: Emitter) -> list:
    """ports a node reads at frame rate"""
    if isinstance(node, (fx.Mix, fx.RingMod)):
        return [node.left, node.right]
    if isinstance(node, (fx.Gain, fx.Amp)):
        return [node.left]
    if isinstance(node, (fx.CritFilter, ext.SumBus, ext.MixMatrix, ext.Tap, ext.Shaper, ext.Delay, files.FileWriter)):
        return [node.input]
    if isinstance(node, shape.Merge):
        return [node.left, node.right]
    if isinstance(node, ext.PMOsc):
        return [node.mod]
    return []


def _modulated(node: Emitter | None) -> bool:
    """some control input of this node is re-evaluated every block (an LFO on a cutoff, FM at block rate ...):
    its reply to a block then depends on which request produced it, like a filter's (the block-rate value is
    read at the REQUEST's position, chain/__init__.py:305-306), so its history rows come from tails, not from
    re-rendering"""
    return node is not None and any(not _ctl_const(p) for p in _control_ports(node))


def _foreign(node: Emitter) -> bool:
    """a node class the engine has no kernel schedule for -- a plugin written against the node API; it is pulled block by
    block through its own respond(), so its reply may depend on the request like a filter's"""
    return not isinstance(node, _KNOWN_TYPES + _KNOWN_BESIDE)


def _is_pure(node: Emitter | None, memo: dict) -> bool:
    """position-pure: no filter and no per-block control anywhere upstream on the audio path, so any row
    range can be rendered in one launch and history rows can simply be re-rendered"""
    if node is None or not node.get_state().enabled:
        return True
    if node not in memo:
        memo[node] = True       # cycles are rejected elsewhere
        if isinstance(node, (fx.CritFilter, ext.Delay)) or _modulated(node) or _foreign(node):    # (a delay line takes a filter's window)
            memo[node] = False
        else:
            memo[node] = all(_is_pure(p.sig, memo) for p in _audio_ports(node))
    return memo[node]
