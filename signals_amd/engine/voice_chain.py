"""The fused-chain matcher: [SumBus(] [Gain(] LowPass|HighPass(Osc) [)] [)] as one fused launch, and what the bus launch keeps
from one render to the next."""
from __future__ import annotations

import torch

from signals_amd import _native, runtime
from signals_amd.chain import AUDIO_DTYPE, CTRL_DTYPE, Emitter, as_control
from signals_amd.chain import ext, fixed, fx, osc
from signals_amd.engine.graph import CONTEXT, SCAN_MAX_ROWS, NotBatchable, _ctl_const, _modulated
from signals_amd.engine.timing import _CapturedLaunches


def _deal_over_tiles(order: torch.Tensor, voices_per_lane: int) -> torch.Tensor:
    """the voice permutation of a bus launch from the voices in order of their cutoff (`order`, an int64 index on any device):
    the j-th group of 64 neighbours in cutoff goes to tile j % tiles, slot j // tiles of the voice tiles of 64 *
    voices_per_lane, so every wave gets the same mix of slow- and fast-decaying slots (one wave per SIMD: the launch takes as
    long as its slowest wave).  A ragged last tile stays lane-major"""
    tile = 64 * voices_per_lane
    tiles = order.shape[0] // tile
    perm = order.clone()
    if tiles:
        q = torch.arange(tiles * tile, device=order.device)
        group, lane = q // 64, q % 64
        perm[((group % tiles) * 64 + lane) * voices_per_lane + group // tiles] = order[q]
    return perm


class _SteadyConsts:
    """The Sine closed form's per-voice constants as the bus launch keeps them from call to call (`BatchRenderer._steady_consts`),
    with what was derived from the same parameter uploads; never edited, replaced when a call is bound to it"""

    __slots__ = ('key', 'tensors', 'buffer', 'phase_bound', 'ordered', 'call', 'workspace')

    def __init__(self, key, tensors, buffer, phase_bound, ordered, call=None, workspace=None):
        self.key = key                                     # (ids of the control rows, id of the pan, filter type, rate, voices, min(context, position))
        self.tensors = tensors                             # (control rows, pan), held so that their addresses cannot be recycled
        self.buffer = buffer                               # the f64 device buffer of the constants
        self.phase_bound = phase_bound                     # (per_frame, ph_max) of _VoiceChain.cycles_per_frame_bound
        self.ordered = ordered                             # (control rows, pan) in cutoff order (_VoiceChain.ordered_by_cutoff)
        self.call = call                                   # the FusedVoiceBusCall pre-bound to all of this, or None
        self.workspace = workspace                         # the bus workspace `call` was bound with

    @property
    def context(self) -> int:
        """the context length the constants were built at: min(context, position) of their first launch"""
        return self.key[-1]

    def bound_to(self, call, workspace) -> '_SteadyConsts':
        return _SteadyConsts(self.key, self.tensors, self.buffer, self.phase_bound, self.ordered, call, workspace)


class _TremoloOrder:
    """The cutoff order of a tremolo-only or swept Sine voice under a bus (`BatchRenderer._tremolo_order`), kept while the constant
    rows are"""

    __slots__ = ('key', 'tensors', 'index', 'rows', 'pan')

    def __init__(self, key, tensors, index, rows, pan):
        self.key = key
        self.tensors = tensors                             # the rows and the pan the order was made from, held like _SteadyConsts.tensors
        self.index = index                                 # the voice permutation as a device index, or None (no closed form, no one Fixed row)
        self.rows = rows                                   # [hertz, phase, cutoff | None under a sweep] in that order
        self.pan = pan                                     # the pan in that order


class _BusPipeline:
    """Streams, workspaces, pre-bound calls and output rings of the pipelined replay (`BatchRenderer._pipe`): consecutive batches
    go to the streams in turn, each stream hands out its RING output buffers in turn"""

    RING = 4
    __slots__ = ('held', 'key', 'shape', 'streams', 'work', 'calls', 'handles', 'events', 'outs', 'turn', 'slot', 'current')

    def __init__(self, held: _SteadyConsts, key: list, shape: tuple, streams: list, work: list, calls: list, dev):
        self.held, self.key, self.shape = held, key, shape  # the constants, the live key and the output shape all of this was set up for
        self.streams, self.work, self.calls = streams, work, calls
        self.handles = [s.cuda_stream for s in streams]
        self.events = [torch.cuda.Event() for _ in streams]
        self.outs = [[torch.empty(shape, dtype=AUDIO_DTYPE, device=dev) for _ in range(self.RING)] for _ in streams]
        self.turn, self.slot = 0, [0] * len(streams)
        self.current = None                                # (raw handle, Stream object) of the caller's stream, as last seen

    def next(self):
        """(call, raw stream handle, output buffer, event, stream) of the next batch; moves on to the next stream, and this
        stream to its next buffer"""
        i = self.turn
        self.turn = (i + 1) % len(self.streams)
        slot = self.slot[i]
        self.slot[i] = (slot + 1) % self.RING
        return self.calls[i], self.handles[i], self.outs[i][slot], self.events[i], self.streams[i]


class _VoiceChain:
    """The fusable pattern  [SumBus(] [Gain(] LowPass|HighPass(Osc) [)] [)]  matched on a graph, when nothing else
    consumes the intermediate nodes and every control input is block-invariant.  Launches it as
    sig_fused_osc_biquad (chain) or sig_fused_voice_bus (chain + bus); in the latency regime the chain runs as a
    prefix scan and the bus as its own launch, optionally captured into a hipGraph."""

    def __init__(self, batch: '_Batch', src, filt, gain_node, bus_node, channels: int, pre_gain=None, pair=None):
        self.batch, self.src, self.filt, self.gain_node, self.bus_node = batch, src, filt, gain_node, bus_node
        self.pre_gain = pre_gain                                   # a Gain between oscillator and filter, folded into the output gain
        self.pair = pair                                           # (Mix | RingMod node, second oscillator): the filter reads op(src, second)
        self.pair_rows = None                                      # (hertz2, phase2, mix) as resolve() found them
        self.channels = channels                                   # voices of the chain
        self.gain_ports = [g.right for g in (pre_gain, gain_node) if g is not None]
        self.ports = [src.hertz, src.phase, filt.cutoff] + self.gain_ports
        self.involved = [n for n in (src, filt, gain_node, bus_node, pre_gain, *(pair or ())) if n is not None]
        self.kind, self.btype = src.kind(), str(filt.type())
        self.fm = not (_ctl_const(src.hertz) and _ctl_const(src.phase))   # block-rate frequency / phase modulation (osc.py:28-30)
        self.hist_rows = (None, None)                              # hertz / phase of the block in front of the batch, as resolve() found them
        self.modulated = self.fm or any(not _ctl_const(p) for p in [filt.cutoff] + self.gain_ports)   # per-block parameter rows
        self.general = self.modulated or pair is not None          # the walker's general entry points (sig_fused_*_rows / *_pair / *_fm)
        source = self.kind if pair is None else f'{type(pair[0]).__name__}({self.kind},{pair[1].kind()})'
        self.tag = (f'{source},{self.btype}{",gain" if self.gain_ports else ""}{",per-block" if self.modulated else ""}'
                    f'{",fm" if self.fm else ""}')
        if pair is not None:
            self.ports += [pair[1].hertz, pair[1].phase] + ([pair[0].mix] if isinstance(pair[0], fx.Mix) else [])

    # ---- matching
    @classmethod
    def match_and_launch(cls, batch: '_Batch', node: Emitter, channels: int, hist: int) -> torch.Tensor | None:
        bus_node, mix_node, top = None, None, node
        if isinstance(node, ext.SumBus):
            if not batch.owner.fuse_bus or hist != 0 or node.channels not in (1, 2, 4):
                return None
            bus_node, top = node, node.input.sig
            if top is None or not top.get_state().enabled or len(top.outputs_with_ports) != 1:
                return None
            channels = node.input.channels
        elif isinstance(node, ext.MixMatrix):
            if hist != 0 or channels % 64:
                return None
            mix_node, top = node, node.input.sig
            if top is None or not top.get_state().enabled or len(top.outputs_with_ports) != 1:
                return None
        gain_node, filt = None, top
        if isinstance(top, fx.Gain):
            gain_node, filt = top, top.left.sig
            if not isinstance(filt, fx.SingleCritFilter) or len(filt.outputs_with_ports) != 1:
                return None
        if not isinstance(filt, fx.SingleCritFilter) or not filt.get_state().enabled:
            return None
        src, pre_gain = filt.input.sig, None
        if (isinstance(src, fx.Gain) and src.get_state().enabled and _ctl_const(src.right) and isinstance(src.left.sig, osc.Osc)
                and (src, channels) not in batch._memo):
            # Filter(Gain(Osc)) = Gain(Filter(Osc)): the filter is linear and starts every block from zero state, so a
            # block-invariant gain in front of it is a factor of the output weight (lowpass_test.sigs: Triangle -> Gain ->
            # LowPass).  The Gain may have other readers: they get its rows from the per-node schedule as usual.
            pre_gain, src = src, src.left.sig
        pair = None
        if (pre_gain is None and isinstance(src, (fx.Mix, fx.RingMod)) and src.get_state().enabled and not _modulated(src)
                and len(src.outputs_with_ports) == 1 and (src, channels) not in batch._memo):
            # Filter(Mix | RingMod(Osc, Osc)): both oscillators are evaluated per row inside the walker
            left, right = src.left.sig, src.right.sig
            if (isinstance(left, osc.Osc) and isinstance(right, osc.Osc) and left is not right and right.get_state().enabled
                    and len(right.outputs_with_ports) == 1 and _ctl_const(right.hertz) and _ctl_const(right.phase)):
                pair, src = (src, right), left
        if not isinstance(src, osc.Osc) or not src.get_state().enabled or len(src.outputs_with_ports) != 1:
            return None
        fm = not (_ctl_const(src.hertz) and _ctl_const(src.phase))
        if fm and (pair is not None or batch.N < CONTEXT):
            # two oscillators AND block-rate FM: per node.  Blocks shorter than the context: the context request [p - 100, p) is
            # then contained in no single cached block of the oscillator, so the reference answers it as a block of its own
            # (controls read at p - 100) -- not the previous block's samples the fused walker warms up on: per node too
            return None
        chain = cls(batch, src, filt, gain_node, bus_node, channels, pre_gain, pair)
        controls = chain.resolve()
        if controls is None or not chain.widths_ok(controls):
            return None
        if mix_node is not None:
            return chain.launch_mix(mix_node, controls)
        return chain.launch_bus(node, controls) if bus_node is not None else chain.launch_chain(node, controls, hist)

    def resolve(self):
        """[hertz, phase, cutoff, gain|None] as they are NOW (a Fixed re-uploads when its array changed);
        None if the pattern no longer holds"""
        if not all(n.get_state().enabled for n in self.involved):
            return None
        try:
            if self.pair is not None:
                op, second = self.pair
                self.pair_rows = (self.batch._control_const(second.hertz, 'hertz'), self.batch._control_const(second.phase, 'phase'),
                                  self.batch._control_const(op.mix, 'mix') if isinstance(op, fx.Mix) else None)
            if self.modulated:
                # hertz / phase / cutoff / gain driven by computed block-rate signals (vibrato, an LFO sweep, a tremolo): K rows
                # each, one per block, all of them from ONE control-program launch
                b, o = self.batch, self.batch.owner
                ports = self.ports[:2] + [self.filt.cutoff] + self.gain_ports
                # ... and, under block-rate FM, the hertz / phase of the block in FRONT of the batch (evaluated by the same
                # launch): the reference's oscillators keep their previous block (BlockCachingEmitter), so block 0's context rows
                # are that block's samples -- the previous batch's last block on a contiguous stream, else the context request
                # [pos - c, pos) answered as a block of its own (its controls read at pos - c)
                q = -1
                if self.fm:
                    contiguous = o._stream_end == b.pos and bool(o._prev_block_frames) and o._prev_block_frames >= min(CONTEXT, b.pos)
                    q = b.pos - (o._prev_block_frames if contiguous else min(CONTEXT, b.pos))
                got = b._control_many(ports, q, channels=self.channels)
                vals, fronts = (got, None) if q < 0 else got
                vals = [as_control(t) for t in vals]
                rows, gains = vals[:3], vals[3:]
                if self.fm:
                    self.hist_rows = tuple(None if _ctl_const(p) else as_control(f) for p, f in zip(self.ports[:2], fronts[:2]))
                if len(gains) == 2:
                    gains = [(gains[0] * gains[1]).contiguous()]
                return rows + (gains or [None])
            rows = [self.batch._control_const(p, p.name) for p in self.ports[:2]]
            rows.append(self.batch._control_const(self.filt.cutoff, 'cutoff'))
            gains = [self.batch._control_const(p, p.name) for p in self.gain_ports]
        except NotBatchable:
            return None
        if len(gains) == 2:
            # one output gain: the product of the two rows, kept while both uploads are (so that its identity is as stable as
            # theirs: the closed form's constants are keyed on it)
            held = self.batch.owner._gain_products.get((id(gains[0]), id(gains[1])))
            if held is None or held[0] is not gains[0] or held[1] is not gains[1]:
                self.batch.owner._gain_products.clear()
                held = self.batch.owner._gain_products[(id(gains[0]), id(gains[1]))] = (gains[0], gains[1], (gains[0] * gains[1]).contiguous())
            gains = [held[2]]
        return rows + (gains or [None])

    def widths_ok(self, controls) -> bool:
        hertz, phase, cutoff, gain = controls
        v = self.channels
        source = [hertz, phase] + [t for t in (self.pair_rows or ()) if t is not None]
        return (max(t.shape[1] for t in source) == v and cutoff.shape[1] == v
                and all(t.shape[1] in (1, v) for t in source) and (gain is None or gain.shape[1] in (1, v)))

    def pair_arg(self):
        """the `pair` argument of _native.fused_rows: (op, second kind, hertz2, phase2, mix)"""
        if self.pair is None:
            return None
        return (type(self.pair[0]).__name__, self.pair[1].kind(), *self.pair_rows)

    def cycles_per_frame_bound(self) -> tuple[float, float]:
        """(max |hertz| / rate, max |phase|) over the chain's voices, from the host arrays behind the Fixed controls
        (an unplugged port is 0): bounds |t| = |frame / rate * hertz + phase| of any frame without touching the device"""
        import numpy as np
        out = []
        for p in (self.src.hertz, self.src.phase):
            src = p.sig
            if src is None or not src._state.enabled:
                out.append(0.0)
            else:
                value = np.abs(np.asarray(src._state.value, dtype=np.float64))
                out.append(float(value.max()) if value.size and np.isfinite(value).all() else float('inf'))
        return out[0] / self.batch.rate, out[1]

    def ordered_by_cutoff(self, ctl, pan, voices_per_lane: int):
        """(controls, pan) with the voices re-ordered for the bus launch: groups of 64 neighbours in cutoff, dealt round
        robin over the voice tiles of 64 * voices_per_lane, slot-major (slot i of every lane of a wave = one group).  The bus is a sum
        over voices, so any order renders the same bus up to the rounding of the sum; this one lets the Sine closed
        form drop the decayed homogeneous part of whole voice slots (sig_fused_steady.h: fused_steady_bus_kernel).
        Built once per parameter upload (it is kept with the closed form's constants)."""
        index = self.cutoff_order(ctl, voices_per_lane)
        if index is None:
            return ctl, pan
        v = self.channels
        pick = lambda t: t if t is None or t.shape[1] != v else t.index_select(1, index).contiguous()
        return [pick(t) for t in ctl], pick(pan)

    def cutoff_order(self, ctl, voices_per_lane: int):
        """the permutation of `ordered_by_cutoff` as a device index, or None when the cutoffs are not one Fixed row"""
        import numpy as np
        v, src = self.channels, self.filt.cutoff.sig
        if ctl[2].shape[1] != v or not isinstance(src, fixed.Fixed):
            return None
        cut = np.asarray(src._state.value, dtype=np.float64).reshape(-1)
        if cut.size != v or not np.isfinite(cut).all():
            return None
        return _deal_over_tiles(torch.from_numpy(np.argsort(cut, kind='stable')), voices_per_lane).to(runtime.device())

    def live_key(self, bus_node=None):
        """identities of the resident control tensors (and the bus gains) as they are NOW -- `resident()` re-uploads an
        edited array, which changes the identity; None if the pattern no longer holds.  The cheap per-block check of the
        latency path: a bound call is reused while every identity is unchanged."""
        for n in self.involved:
            if not n._state.enabled:
                return None
        key = []
        for p in self.ports:
            src = p.sig
            if src is None or not src._state.enabled:
                key.append(None)
            elif type(src) is fixed.Fixed:
                key.append(src.resident())
            else:
                return None
        if bus_node is not None:
            key.append(bus_node.resident_gains())
        return key

    def _same_shapes(self, now, then) -> bool:
        return now is not None and all(a.shape == b.shape for a, b in zip(now[:3], then[:3]))

    # ---- chain only: out (K*N, voices)
    def launch_chain(self, node: Emitter, controls, hist: int) -> torch.Tensor:
        b, o, dev = self.batch, self.batch.owner, runtime.device()
        N, K, rate, v = b.N, b.K, b.rate, self.channels
        rows = N * K
        status = o._status_word(self.filt)
        name = f'fused_osc_biquad[{self.tag}]'

        def run(position, ctl, out):
            if self.general:
                return o._launch(name, lambda: _native.fused_rows(self.kind, self.btype, rate, position, N, K, CONTEXT, v,
                                                                  ctl[0], ctl[1], ctl[2], ctl[3], out, status=status,
                                                                  pair=self.pair_arg(), hertz_hist=self.hist_rows[0],
                                                                  phase_hist=self.hist_rows[1]),
                                 units=rows * v)
            return o._launch(name, lambda: _native.fused_osc_biquad(self.kind, self.btype, rate, position, N, K, CONTEXT,
                                                                    ctl[0], ctl[1], ctl[2], ctl[3], out, status=status),
                             units=rows * v)
        if hist:
            # a consumer (a second filter) needs history rows: the launch writes the K blocks, the rows in front
            # come from the tail / a fresh block like any filter's
            result = torch.empty((hist + rows, v), dtype=AUDIO_DTYPE, device=dev)
            run(b.pos, controls, result[hist:])
            b._own_history(node, v, hist, result)
            return result

        def replay(position: int) -> torch.Tensor:
            ctl = self.resolve()
            if not self._same_shapes(ctl, controls):
                o._replay = None
                return o.render(position, N, K)                  # pattern no longer holds: re-plan
            return run(position, ctl, torch.empty((rows, v), dtype=AUDIO_DTYPE, device=dev))
        if node is o.node and not self.modulated:                      # (a replay would re-read the control rows at a stale position)
            o._remember_replay(N, K, replay)
        return run(b.pos, controls, torch.empty((rows, v), dtype=AUDIO_DTYPE, device=dev))

    # ---- chain + MixMatrix: out (K*N, voices), the per-voice rows only ever exist as 32-row LDS tiles
    def launch_mix(self, mix_node, controls) -> torch.Tensor:
        b, o = self.batch, self.batch.owner
        N, K, v = b.N, b.K, self.channels
        if self.general:
            return None                                             # per-block rows / two oscillators: the chain runs fused, the matrix as its own launch
        out = torch.empty((N * K, v), dtype=AUDIO_DTYPE, device=runtime.device())
        matrix, status = mix_node.resident_matrix(), o._status_word(self.filt)
        return o._launch(f'fused_osc_biquad_mix[{self.tag}]',
                         lambda: _native.fused_osc_biquad_mix(self.kind, self.btype, b.rate, b.pos, N, K, CONTEXT,
                                                              controls[0], controls[1], controls[2], controls[3], matrix, out,
                                                              status=status),
                         units=N * K * v)

    # ---- chain + bus: out (K*N, bus channels)
    def launch_bus(self, node: Emitter, controls) -> torch.Tensor:
        b, o, dev = self.batch, self.batch.owner, runtime.device()
        N, K, v = b.N, b.K, self.channels
        rows, bus_c = N * K, self.bus_node.channels
        pan = self.bus_node.resident_gains()
        if pan is not None and pan.shape[1] != v:
            return None
        status = o._status_word(self.filt)
        o._bus_workspace(v, rows, bus_c)
        if self.general:
            return self.launch_bus_general(controls, pan, status)
        # latency regime: too few (voice, block) chains to fill the chip with serial walks -> the chain runs as a
        # time-parallel prefix scan (sig_fused_osc_biquad picks it) and the bus as its own launch
        small = v * K <= o.scan_max_chains and CONTEXT + N <= SCAN_MAX_ROWS
        # one block of a Sine chain: a single launch does chain, bus and (under hipGraph replay) the position advance
        one_launch = small and K == 1 and self.kind == 'Sine' and o.latency_kernel
        if one_launch and (o._latency_ws is None or o._latency_ws[0] != (v, N, bus_c)):
            o._latency_ws = ((v, N, bus_c), _native.latency_voice_bus_workspace(v, N, bus_c, dev))
        replay = _BusReplay(self, controls, pan, status, small, one_launch)
        if node is o.node:
            o._remember_replay(N, K, replay)
        return replay.run(b.pos, controls, pan, torch.empty((rows, bus_c), dtype=AUDIO_DTYPE, device=dev))

    def launch_bus_general(self, controls, pan, status) -> torch.Tensor:
        """chain + bus through the walker's general entry (per-block rows, two oscillators, block-rate FM)"""
        b, o = self.batch, self.batch.owner
        N, K, rate, v = b.N, b.K, b.rate, self.channels
        rows, bus_c = N * K, self.bus_node.channels
        if bus_c not in (1, 2):
            return None
        swept = controls[2].shape[0] > 1                                    # the cutoff is read per block
        if (self.kind == 'Sine' and self.pair is None and not self.fm and controls[2].shape[1] == v
                and (swept or (controls[3] is not None and controls[3].shape[0] > 1 and controls[3].shape[1] == v))):
            # a swept cutoff and / or a tremolo: sig_fused_voice_bus_rows keeps the closed form (per-block filter constants,
            # bus weights rebuilt per block), and the closed form wants its voices ordered by cutoff (ordered_by_cutoff: it
            # drops the decayed homogeneous part per voice slot); the order is kept while the constant rows are.  Under a
            # sweep the order of the batch's first row stands for all of them (an LFO scales every voice's cutoff alike;
            # any order is correct) -- sorted on the device, no host round trip
            held = o._tremolo_order
            key = (id(controls[0]), id(controls[1]), id(controls[2]) if not swept else None, id(pan), K, swept)
            if held is None or held.key != key:
                plan = _native.fused_voice_bus_plan('Sine', b.pos, v, N, K, CONTEXT)
                vpl = min(plan['voices_per_lane'], 8)
                if swept and vpl < 8:
                    vpl = min(vpl, 2)                                        # (per-block constants: eight voices per lane, or two)
                if not plan['closed_form']:
                    index = None
                elif not swept:
                    index = self.cutoff_order(controls, vpl)
                else:
                    index = _deal_over_tiles(torch.argsort(controls[2][0], stable=True), vpl)
                pick = lambda t: t if t is None or index is None or t.shape[1] != v else t.index_select(1, index).contiguous()
                held = o._tremolo_order = _TremoloOrder(key, (controls[0], controls[1], controls[2], pan), index,
                                                        [pick(controls[0]), pick(controls[1]), None if swept else pick(controls[2])],
                                                        pick(pan))
            if held.index is not None:
                pick = lambda t: t if t is None or t.shape[1] != v else t.index_select(1, held.index)
                cut = pick(controls[2]) if swept else held.rows[2]
                gain_rows = controls[3]
                if gain_rows is not None and gain_rows.shape[1] == v:
                    gain_rows = pick(gain_rows)
                controls = [held.rows[0], held.rows[1], cut, gain_rows]
                pan = held.pan
        out = torch.empty((rows, bus_c), dtype=AUDIO_DTYPE, device=runtime.device())
        return o._launch(f'fused_voice_bus[{self.tag}]',
                         lambda: _native.fused_rows(self.kind, self.btype, rate, b.pos, N, K, CONTEXT, v, controls[0], controls[1],
                                                    controls[2], controls[3], out, bus_gains=pan, bus=True,
                                                    workspace=o._workspace, status=status, pair=self.pair_arg(),
                                                    hertz_hist=self.hist_rows[0], phase_hist=self.hist_rows[1]),
                         units=rows * v)


class _BusReplay:
    """One plan of the chain + bus launch over block-invariant rows (`_VoiceChain.launch_bus` builds it, once per plan): what the
    launch needs at any position.  Calling it renders the batch at a new position without re-walking the graph; that is what
    `BatchRenderer._remember_replay` keeps of a graph that is exactly this launch."""

    __slots__ = ('chain', 'owner', 'controls', 'pan', 'N', 'K', 'rows', 'bus_c', 'v', 'rate', 'dev', 'status', 'small', 'one_launch',
                 'chain_name', 'bus_name', 'live', 'call')

    def __init__(self, chain: _VoiceChain, controls, pan, status, small: bool, one_launch: bool):
        b = chain.batch
        self.chain, self.owner, self.controls, self.pan, self.status = chain, b.owner, controls, pan, status
        self.N, self.K, self.rows, self.bus_c = b.N, b.K, b.N * b.K, chain.bus_node.channels
        self.v, self.rate, self.dev = chain.channels, b.rate, runtime.device()
        self.small, self.one_launch = small, one_launch
        self.chain_name, self.bus_name = f'fused_osc_biquad[{chain.tag}]', f'fused_voice_bus[{chain.tag}]'
        self.live = self.call = None                         # live key, LatencyVoiceBusCall of the one-launch block

    def run(self, position, ctl, pan_now, out):
        c, o = self.chain, self.owner
        N, K, rows, bus_c, v, rate, dev, status = self.N, self.K, self.rows, self.bus_c, self.v, self.rate, self.dev, self.status
        if self.one_launch:
            return o._launch(f'latency_voice_bus[{c.tag}]',
                             lambda: _native.latency_voice_bus(c.btype, rate, position, N, CONTEXT, v, ctl[0], ctl[1],
                                                               ctl[2], ctl[3], pan_now, out, o._latency_ws[1],
                                                               status=status), units=rows * v)
        if self.small:
            voices_buf = torch.empty((rows, v), dtype=AUDIO_DTYPE, device=dev)
            o._launch(self.chain_name, lambda: _native.fused_osc_biquad(c.kind, c.btype, rate, position, N, K, CONTEXT,
                                                                        ctl[0], ctl[1], ctl[2], ctl[3], voices_buf,
                                                                        status=status), units=rows * v)
            return o._launch('sum_bus', lambda: _native.sum_bus(voices_buf, pan_now, out), units=rows * v)
        # the Sine closed form's per-voice constants survive from call to call while the control tensors (held here,
        # so their addresses cannot be recycled), the filter type and min(context, position) are the same
        key = (tuple(id(t) for t in ctl), id(pan_now), c.btype, rate, v, min(CONTEXT, position))
        held = o._steady_consts
        ready = held is not None and held.key == key
        if not ready:
            size = _native.lib().sig_fused_voice_consts_size(v) // 8
            buf = held.buffer if held is not None and held.buffer.numel() >= size else torch.empty(size, dtype=CTRL_DTYPE, device=dev)
            plan = _native.fused_voice_bus_plan(c.kind, position, v, N, K, CONTEXT)
            o._steady_consts = held = _SteadyConsts(key, (tuple(ctl), pan_now), buf, c.cycles_per_frame_bound(),
                                                    c.ordered_by_cutoff(ctl, pan_now, plan['voices_per_lane']))
        ctl, pan_now = held.ordered
        # Past |t| = 2^26 cycles the Sine closed form (and the walker's incremental phase) hands over to the exact
        # per-row phase, wave by wave inside the launch -- correct, but the closed-form kernel's built-in fallback is
        # a plain loop meant for a few waves.  max |hertz| and max |phase| are host-side knowledge: when the launch's
        # last frame puts the fastest voice past the limit, the span walker takes the whole launch instead.
        per_frame, ph_max = held.phase_bound
        walk = c.kind == 'Sine' and ph_max + (position + rows) * per_frame >= _native.SINE_FAST_MAX_CYCLES
        if o.timer is None or o.timer.region:
            # the per-batch host path: one pre-bound ctypes call (the binding's per-call validation cost more than the launch at
            # 256 blocks per batch); bound per set of constants, i.e. while the parameter uploads are the same tensors
            call = held.call
            if call is None or call.shape != (rows, bus_c) or held.workspace is not o._workspace:
                call = _native.FusedVoiceBusCall(c.kind, c.btype, rate, N, K, CONTEXT, v, ctl[0], ctl[1], ctl[2], ctl[3], pan_now,
                                                 bus_c, o._workspace, status, held.buffer)
                o._steady_consts = held = held.bound_to(call, o._workspace)
            if o.timer is not None:
                return o.timer.launch(self.bus_name, lambda: call(position, out, ready, walk), units=rows * v)
            return call(position, out, ready, walk)
        return o._launch(self.bus_name, lambda: _native.fused_voice_bus(c.kind, c.btype, rate, position, N, K, CONTEXT, v,
                                                                        ctl[0], ctl[1], ctl[2], ctl[3], pan_now, out,
                                                                        workspace=o._workspace, status=status,
                                                                        consts=held.buffer, consts_ready=ready, walk=walk),
                         units=rows * v)

    def captured(self, position, ctl, pan_now):
        """hipGraph of [scan chain(position on device) -> bus -> position += N*K]; None if capture is refused"""
        c, o = self.chain, self.owner
        N, K, rows, bus_c, v, rate, dev, status = self.N, self.K, self.rows, self.bus_c, self.v, self.rate, self.dev, self.status
        keys = tuple(t.data_ptr() if t is not None else 0 for t in (*ctl, pan_now))
        cap = o._captured
        if cap is None or cap.keys != keys:
            def record(pos_t: torch.Tensor) -> torch.Tensor:
                bus_out = torch.empty((rows, bus_c), dtype=AUDIO_DTYPE, device=dev)
                if self.one_launch:
                    return _native.latency_voice_bus(c.btype, rate, pos_t, N, CONTEXT, v, ctl[0], ctl[1], ctl[2], ctl[3],
                                                     pan_now, bus_out, o._latency_ws[1], status=status)
                vbuf = torch.empty((rows, v), dtype=AUDIO_DTYPE, device=dev)
                _native.fused_osc_biquad(c.kind, c.btype, rate, pos_t, N, K, CONTEXT,
                                         ctl[0], ctl[1], ctl[2], ctl[3], vbuf, status=status)
                return _native.sum_bus(vbuf, pan_now, bus_out)
            try:
                cap = o._captured = _CapturedLaunches(record, N * K, position, keys, self_advancing=self.one_launch)
            except RuntimeError:
                # capture refused (another capture in progress, a profiler that forbids it ...):
                # keep rendering with plain launches
                o.graph_replay, o._captured = False, None
                return None
        return cap.run(position)

    def pipelined(self, position: int):
        """the batch at `position` on the next of `o.pipeline` streams, or None when the fast path does not apply (first
        call, parameters re-uploaded, a position inside the first context, the walker's range): the caller falls through"""
        c, o = self.chain, self.owner
        rows, bus_c, v = self.rows, self.bus_c, self.v
        key = c.live_key(c.bus_node)
        held, pipe = o._steady_consts, o._pipe
        if key is None or held is None or held.context != CONTEXT or position < CONTEXT:
            return None
        if pipe is None or pipe.held is not held or len(pipe.key) != len(key) or not all(a is b for a, b in zip(key, pipe.key)) \
                or pipe.shape != (rows, bus_c):
            # set-up (once per set of parameter uploads): the constants are in held.buffer (made by the plain path on the caller's
            # stream: the device is synchronised once here so that the side streams may read them and the ordered rows)
            held_ctl, held_pan = held.tensors
            if len(key) != len(held_ctl) + 1 or key[-1] is not held_pan or \
                    not all(k is None or k is t for k, t in zip(key, held_ctl)):
                return None                                                # (the constants belong to other uploads: the plain path renews them first)
            torch.cuda.synchronize()
            ctl_o, pan_o = held.ordered
            ws_size = _native.lib().sig_fused_voice_bus_workspace(v, rows, bus_c) // 8
            streams = [torch.cuda.Stream() for _ in range(o.pipeline)]
            work = [torch.empty(ws_size, dtype=CTRL_DTYPE, device=self.dev) for _ in streams]
            calls = [_native.FusedVoiceBusCall(c.kind, c.btype, self.rate, self.N, self.K, CONTEXT, v, ctl_o[0], ctl_o[1], ctl_o[2],
                                               ctl_o[3], pan_o, bus_c, w, self.status, held.buffer) for w in work]
            pipe = o._pipe = _BusPipeline(held, key, (rows, bus_c), streams, work, calls, self.dev)
            torch.cuda.synchronize()
        per_frame, ph_max = held.phase_bound
        if c.kind == 'Sine' and ph_max + (position + rows) * per_frame >= _native.SINE_FAST_MAX_CYCLES:
            return None                                                    # (beyond the closed form's range: the plain path picks the walker)
        call, handle, out, event, stream = pipe.next()
        if o.timer is not None:
            o.timer.launch(self.bus_name, lambda: call(position, out, True, False, stream=handle), units=rows * v)
        else:
            call(position, out, True, False, stream=handle)
        event.record(stream)                                               # the caller's stream waits for this batch
        raw = _native.current_stream_handle(self.dev.index)                # (torch.cuda.current_stream() costs 8 us of Python: the Stream
        cur = pipe.current                                                 # object is kept while the raw handle is the same)
        if cur is None or cur[0] != raw:
            cur = pipe.current = (raw, torch.cuda.current_stream())
        cur[1].wait_event(event)
        return out

    def __call__(self, position: int) -> torch.Tensor:
        c, o = self.chain, self.owner
        if o.pipeline > 1 and not self.small and (o.timer is None or o.timer.region):
            done = self.pipelined(position)
            if done is not None:
                return done
        if self.one_launch and o.timer is None:
            # latency mode, the per-block host path: five identity checks, one allocation, one ctypes call (a hipGraph of
            # this single launch would only add its replay cost: 19.6 us per block against 14.6)
            key, live = c.live_key(c.bus_node), self.live
            if key is not None and live is not None and len(key) == len(live) and all(a is b for a, b in zip(key, live)):
                return self.call(position, torch.empty((self.rows, self.bus_c), dtype=AUDIO_DTYPE, device=self.dev))
        ctl, pan_now = c.resolve(), c.bus_node.resident_gains()
        if not c._same_shapes(ctl, self.controls) or (pan_now is None) != (self.pan is None):
            o._replay = None
            return o.render(position, self.N, self.K)         # pattern no longer holds: re-plan
        if self.small and o.graph_replay and not self.one_launch:
            out = self.captured(position, ctl, pan_now)
            if out is not None:
                return out
        if self.one_launch and o.timer is None:
            key = c.live_key(c.bus_node)
            if key is not None and (pan_now is None or pan_now.shape[1] == self.v) and c.widths_ok(ctl):
                self.live, self.call = key, _native.LatencyVoiceBusCall(c.btype, self.rate, self.N, CONTEXT, self.v, ctl[0], ctl[1],
                                                                        ctl[2], ctl[3], pan_now, self.bus_c, o._latency_ws[1],
                                                                        self.status)
        return self.run(position, ctl, pan_now, torch.empty((self.rows, self.bus_c), dtype=AUDIO_DTYPE, device=self.dev))
