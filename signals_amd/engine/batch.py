"""The per-node scheduler: one render call's buffers, one schedule per node family."""
from __future__ import annotations

import functools

import torch

from signals_amd import _native, runtime
from signals_amd.chain import AUDIO_DTYPE, CTRL_DTYPE, Emitter, Receiver, as_control, broadcast_shape
from signals_amd.chain import ext, files, fixed, fx, noise, osc, shape
from signals_amd.engine.control import _ControlProgram
from signals_amd.engine.graph import CONTEXT, _KNOWN_TYPES, NotBatchable, _audio_ports, _ctl_const, _ctl_unplugged, _family, _is_pure, _modulated, _no_block_rate
from signals_amd.engine.voice_chain import _VoiceChain
from signals_amd.engine.voice_program import _NoProgram, _VoiceProgram


class _Batch:
    """One render call: position, N, K fixed; buffers memoised per (node, channels)."""

    def __init__(self, owner: 'BatchRenderer', position: int, N: int, K: int, continuing: bool):
        self.owner = owner
        self.pos, self.N, self.K = position, N, K
        self.continuing = continuing
        self.rate = owner.rate
        self._pure: dict = {}
        self._memo: dict[tuple[Emitter, int], tuple[torch.Tensor, int]] = {}
        self._need: dict[tuple[Emitter, int], int] = {}
        self._impure: dict[Emitter, torch.Tensor] = {}
        self._ctl_memo: dict[Emitter, torch.Tensor] = {}
        self._widths: list[int] = []            # request widths of the nodes being scheduled (what their control ports are read with)
        self.history_of: int | None = None      # this batch renders the history block in front of a fresh batch at that position

    # -------------------------------------------------------------- control rows
    def _control_const(self, port: Receiver.BoundPort, what: str) -> torch.Tensor:
        """one (1, C) row that holds for every block (Fixed / unplugged); NotBatchable otherwise"""
        src = port.sig
        if src is None or not src.get_state().enabled:
            return Emitter.empty_result()
        if isinstance(src, fixed.Fixed):
            row = src.resident()
            if row.shape[0] != 1:
                raise NotBatchable(f'{what}: multi-row Fixed on a control port')
            return as_control(row)
        raise NotBatchable(f'{what} is driven by {src.cls_name()}; this stage needs block-invariant control rows')

    def _control(self, port: Receiver.BoundPort, what: str) -> torch.Tensor:
        """(1, C) if the value holds for every block, else (K, C): row b is the port's reply to the block-rate
        request at position pos + b*N (forward_at_block_rate of block b)."""
        return self._control_node(port.sig, what)

    def _control_many(self, ports: list, front_position: int = -1, channels: int | None = None):
        """the block-rate replies of several control ports, their subgraphs evaluated in one launch where they consist of
        oscillators, element-wise nodes, Fixed rows, ADSR envelopes, White and LowPass / HighPass over those (else node by node, like `_control`);
        with `front_position` also their one-row replies at that position: (rows, fronts).  `channels`: the request width the
        ports are read with."""
        o = self.owner
        srcs = tuple(p.sig for p in ports)
        key = (tuple(id(x) for x in srcs), self.K, channels)
        try:
            program = o._control_program(key, lambda: _ControlProgram(srcs, self.K, channels=channels, status=o._status_word))
            self._check_windowed(program, [front_position] if front_position >= 0 else [])
            return program.run(o, self.rate, self.pos, self.N, front_position)
        except NotBatchable:
            rows = [self._control(p, p.name) for p in ports]
            if front_position < 0:
                return rows
            front = _Batch(o, front_position, 2, 1, False)
            return rows, [front._control(p, p.name) for p in ports]

    def _control_node(self, src: Emitter | None, what: str) -> torch.Tensor:
        if src is None or not src.get_state().enabled:
            return Emitter.empty_result()
        if src in self._ctl_memo:
            return self._ctl_memo[src]
        o, K, dev = self.owner, self.K, runtime.device()
        if isinstance(src, fixed.Fixed):
            row = src.resident()
            if row.shape[0] != 1:
                raise NotBatchable(f'{what}: multi-row Fixed on a control port')
            result = as_control(row)
        elif isinstance(src, osc.Osc):
            hertz, phase = self._control(src.hertz, 'hertz'), self._control(src.phase, 'phase')
            _, voices = broadcast_shape((1, 1), hertz.shape[-2:], phase.shape[-2:])
            result = torch.empty((K, voices), dtype=CTRL_DTYPE, device=dev)
            o._launch(f'osc_bank[{src.kind()},block-rate]',
                      lambda: _native.osc_bank(src.kind(), self.pos, self.rate, hertz, phase, result,
                                               step=self.N, rows_per_param=1),
                      units=K * voices)
        elif isinstance(src, (fx.SingleCritFilter, fx.DoubleCritFilter, noise.White, ext.ADSR)):
            # a filter, White or an envelope read at one frame per block: a control program of its own -- a filter's input is evaluated
            # per window row inside the launch, nothing of it goes through memory; an envelope's parameter subgraphs are included (as
            # wide as they broadcast, whatever the request's width -- it alone may be read where that width is not known)
            if not self._widths and not isinstance(src, ext.ADSR):
                raise NotBatchable(f'{what}: {src.cls_name()} read where the request width is not known')
            width = self._widths[-1] if self._widths else None
            program = o._control_program(('node', id(src), K, width),
                                         lambda: _ControlProgram((src,), K, channels=width, status=o._status_word))
            self._check_windowed(program, [])
            result = program.run(o, self.rate, self.pos, self.N)[0]
        elif isinstance(src, (fx.Gain, fx.Amp, fx.Mix, fx.RingMod)):
            name = type(src).__name__
            a = self._control(src.left, 'left')
            b = self._control(src.right, 'right')
            c = self._control(src.mix, 'mix') if isinstance(src, fx.Mix) else None
            ops = [a, b] + ([c] if c is not None else [])
            _, cols = broadcast_shape(*((1, t.shape[1]) for t in ops))
            rows = max(t.shape[0] for t in ops)
            result = torch.empty((rows, cols), dtype=CTRL_DTYPE, device=dev)
            o._launch(f'elementwise[{name},block-rate]', lambda: _native.elementwise(name, a, b, c, result),
                      units=rows * cols)
        else:
            refusal = _no_block_rate(src, 'schedule') or f'no block-rate schedule for {src.cls_name()}'
            raise NotBatchable(f'{what}: {refusal}')
        self._ctl_memo[src] = result
        return result

    def _check_windowed(self, program: '_ControlProgram', ahead: list) -> None:
        """where a filter in a control path answers what the batch cannot: the reference's block cache serves a one-frame read
        at p from the `after` window [q + 1, q + 101) of an earlier read at q (chain/cache.py), i.e. the float32 window value --
        blocks of <= 100 frames, and a read within 100 frames behind another one (`ahead`: the positions read in front of this
        batch's blocks, oldest first; the history block rendered in front of a fresh batch)"""
        if not program.windowed:
            return
        if self.N <= CONTEXT and (self.K > 1 or self.continuing):
            raise NotBatchable('a filter in a control path with blocks of <= 100 frames (the next block is served from the '
                               'after-window cache)')
        reads = ahead + [self.pos] + ([self.history_of] if self.history_of is not None else [])
        if any(0 < q1 - q0 <= CONTEXT for q0, q1 in zip(reads, reads[1:])):
            raise NotBatchable('a filter in a control path read within 100 frames in front of a fresh batch (the batch\'s first '
                               'block is served from the after-window cache)')

    # -------------------------------------------------------------- history requirements
    def _require(self, node: Emitter | None, channels: int, hist: int) -> None:
        """propagate how many history rows each (node, channels) buffer must carry"""
        if node is None:
            return
        key = (node, channels)
        if self._need.get(key, -1) >= hist:
            return
        self._need[key] = hist
        if not node.get_state().enabled and not isinstance(node, (ext.Tap, files.FileWriter)):
            return
        family = _family(node)
        if family.window:
            hist = min(CONTEXT, self.pos)
        elif _modulated(node):
            hist = 0                                              # own history comes from the tail / a fresh block
        own_width = family.own_width                              # (a bus, a Merge: they ask with their ports' own widths)
        for port in _audio_ports(node):
            self._require(port.sig, port.channels if own_width else channels, hist)

    # -------------------------------------------------------------- buffers
    def buffer(self, node: Emitter | None, channels: int, hist: int) -> torch.Tensor:
        """(hist + K*N, C') tensor: rows [hist:] are the K blocks, rows [:hist] the node's reply to a
        single block request [pos-hist, pos)."""
        self._require(node, channels, hist)
        full, have = self._materialise(node, channels)
        return full[have - hist:] if have != hist else full

    def _materialise(self, node: Emitter | None, channels: int) -> tuple[torch.Tensor, int]:
        """(buffer, history rows it carries) of one node for this batch, memoised per (node, channels)"""
        key = (node, channels)
        if key in self._memo:
            return self._memo[key]
        if node is not None and isinstance(node, (ext.Tap, files.FileWriter)) and not node.get_state().enabled:
            self._memo[key] = self._materialise(node.input.sig, channels)      # PASSTHRU: disabled = forward input
            return self._memo[key]
        if node is None or not node.get_state().enabled:
            self._memo[key] = (Emitter.empty_result(), 0)                      # (1,1) zeros broadcast everywhere
            return self._memo[key]
        hist = self._need[key]
        rows = hist + self.N * self.K

        self._widths.append(channels)
        try:
            result = _VoiceChain.match_and_launch(self, node, channels, hist) if self.owner.fuse else None
            if result is None and self.owner.fuse_program and hist == 0 and isinstance(node, _VoiceProgram.KERNEL_NODES):
                result = self._program_store(node, channels)
            if result is None:
                for types, build in self._SCHEDULES:
                    if isinstance(node, types):
                        result = build(self, node, channels, hist, rows)
                        break
                else:
                    result = self._sched_foreign(node, channels, hist, rows)
        finally:
            self._widths.pop()
        if isinstance(result, tuple):                                          # a pass-through shares its input's buffer
            self._memo[key] = result
            return result
        if not _is_pure(node, self._pure) and result.shape[0] > 1:
            self._impure[node] = result
        self._memo[key] = (result, hist if result.shape[0] > 1 else 0)
        return self._memo[key]

    def _operand(self, port: Receiver.BoundPort, channels: int, hist: int) -> torch.Tensor:
        """an input as rows [pos-hist, pos+K*N) or a one-row broadcast"""
        full, have = self._materialise(port.sig, channels)
        if full.shape[0] == 1:
            return full
        return full[have - hist:] if have != hist else full

    # -------------------------------------------------------------- one schedule per node family
    def _sched_fixed(self, node, channels, hist, rows):
        value = node.resident()
        if value.shape[0] != 1:
            raise NotBatchable('multi-row Fixed as an audio source')
        return value

    def _sched_osc(self, node, channels, hist, rows):
        hertz, phase = self._control(node.hertz, 'hertz'), self._control(node.phase, 'phase')
        kind = node.kind()
        return self._osc_launch(node, 'osc_bank', kind, functools.partial(_native.osc_bank, kind), (hertz, phase), hist, rows)

    def _sched_pm(self, node, channels, hist, rows):
        """a phase-modulation oscillator: one sig_osc_bank_pm launch over the modulator's rows"""
        hertz, phase, index = (self._control(p, p.name) for p in (node.hertz, node.phase, node.index))
        x = self._operand(node.mod, channels, 0 if _modulated(node) else hist)   # a modulated node's history comes from its tail
        kind = node.kind()
        return self._osc_launch(node, 'osc_bank_pm', kind, functools.partial(_native.osc_bank_pm, kind), (hertz, phase, index, x), hist, rows)

    def _sched_bank(self, node, channels, hist, rows):
        """a generator that is a pure function of the absolute frame and of block-rate rows (ext.Wavetable, ext.Additive, ext.UnisonOsc,
        ext.SyncOsc, ext.Sampler, ext.Modal): one launch of the entry the node states (`bank`), per-block rows when a port is
        modulated; tables, copies and loop bounds go with the call as the node's state holds them now.  No history, no tails"""
        label, kind, operands, call = node.bank(lambda bound: self._control(bound, bound.name), channels)
        return self._osc_launch(node, label, kind, call, operands, hist, rows)

    def _sched_shaper(self, node, channels, hist, rows):
        """a waveshaper: one sig_shaper_table launch over its input's rows (history rows included when a filter reads it), scheduled
        like an element-wise node; per-block select rows when that port is modulated"""
        o, dev = self.owner, runtime.device()
        mod = _modulated(node)
        x = self._operand(node.input, channels, 0 if mod else hist)           # a modulated node's history comes from its tail
        select = self._control(node.select, 'select')
        table = node.resident_table()
        cols = broadcast_shape((1, x.shape[1]), (1, select.shape[1]))[1]
        if x.shape[0] == 1 and not mod:
            result = torch.empty((1, cols), dtype=CTRL_DTYPE, device=dev)      # a one-row reply in, a one-row reply out
            return o._launch('shaper_table[Shaper]', lambda: _native.shaper_table(x, select, table, result), units=cols)
        result = torch.empty((rows, cols), dtype=AUDIO_DTYPE, device=dev)
        main = result[hist:] if mod else result
        o._launch(f'shaper_table[Shaper{",per-block" if mod else ""}]',
                  lambda: _native.shaper_table(x, select, table, main, rows_per_select=self.N if mod else 0), units=main.shape[0] * cols)
        if mod:
            self._own_history(node, cols, hist, result)
        return result

    def _sched_delay(self, node, channels, hist, rows):
        """a delay line: a window node (`_window_node`), one sig_delay_taps launch over the K blocks -- per-block time rows when that port
        is modulated; the taps go with the launch by value.  A request-dependent one-column input: `_delay_uncached`"""
        taps = node.host_taps()

        def bind(window, c0, time, main):
            return (f'delay_taps[{taps.shape[0]}{",per-block" if time.shape[0] > 1 else ""}]',
                    lambda: _native.delay_taps(self.rate, self.pos, self.N, self.K, window, c0, time, taps, main))
        return self._window_node(node, channels, hist, rows, self._control(node.time, 'time'), bind,
                                 uncached=lambda blocks, time, main: self._delay_uncached(node, channels, blocks, time, taps, main))

    def _delay_uncached(self, node, channels, blocks, time, taps, main):
        """a Delay over a request-dependent input that answers ONE column to a wider request.  The block cache files a reply under the
        reply's own shape (chain/cache.py: _write_block_cache), so such a reply never serves a later request of the asked width, neither
        as an exact hit nor as a containing block: the eager path evaluates every `before` request [p - c, p) afresh, with the input's
        controls read at p - c -- not the rows the block in front holds, whose controls were read at p - N.  So every block takes its
        context rows from the input rendered as a block of its own (what `_own_history` does in front of a fresh batch), one launch per
        block.  (A filter never gets here: it raises the reference's IndexError on a one-column input.)"""
        o, N = self.owner, self.N
        for b in range(self.K):
            p = self.pos + b * N
            c = min(CONTEXT, p)
            window = blocks[b * N:(b + 1) * N]
            if c:
                sub = _Batch(o, p - c, c, 1, False)
                sub.history_of = p
                front = sub.buffer(node.input.sig, channels, 0)[:, :window.shape[1]]      # (a voice program stores its one column V times)
                window = torch.cat((front.to(window.dtype), window))
            row = time if time.shape[0] == 1 else time[b:b + 1]
            out = main[b * N:(b + 1) * N]
            o._launch(f'delay_taps[{taps.shape[0]},uncached-input]',
                      lambda: _native.delay_taps(self.rate, p, N, 1, window, c, row, taps, out), units=N * out.shape[1])

    def _osc_launch(self, node, name, kind, call, operands, hist, rows):
        """one launch of an oscillator bank over the batch's rows, as wide as its operands broadcast: `call(position, rate, *operands,
        out, **kw)`"""
        o = self.owner
        _, voices = broadcast_shape((1, 1), *((1, t.shape[1]) for t in operands))
        result = torch.empty((rows, voices), dtype=AUDIO_DTYPE, device=runtime.device())
        if _modulated(node):
            # the parameters are re-read every block: K parameter rows, N output rows each
            main = result[hist:]
            o._launch(f'{name}[{kind},per-block]',
                      lambda: call(self.pos, self.rate, *operands, main, rows_per_param=self.N), units=main.shape[0] * voices)
            self._own_history(node, voices, hist, result)
        else:
            start = self.pos - hist
            o._launch(f'{name}[{kind}]', lambda: call(start, self.rate, *operands, result), units=rows * voices)
        return result

    def _sched_noise(self, node, channels, hist, rows):
        result = torch.empty((rows, channels), dtype=AUDIO_DTYPE, device=runtime.device())
        seed, start = node.get_state().seed, self.pos - hist
        return self.owner._launch('white_noise', lambda: _native.white_noise(seed, start, result), units=rows * channels)

    def _sched_filter(self, node, channels, hist, rows):
        return self._filter(node, channels, hist, rows)

    def _sched_elementwise(self, node, channels, hist, rows):
        o, dev = self.owner, runtime.device()
        if o.fuse and isinstance(node, fx.RingMod):
            enveloped = self._ringmod_with_envelope(node, channels, hist, rows)
            if enveloped is not None:
                return enveloped
        mod = _modulated(node)
        in_hist = 0 if mod else hist                              # a modulated node's history comes from its tail
        a = self._operand(node.left, channels, in_hist)
        if isinstance(node, (fx.Gain, fx.Amp)):
            b, c = self._control(node.right, 'right'), None
        else:
            b = self._operand(node.right, channels, in_hist)
            c = self._control(node.mix, 'mix') if isinstance(node, fx.Mix) else None
        ctl = c if isinstance(node, fx.Mix) else (b if isinstance(node, (fx.Gain, fx.Amp)) else None)
        audio = [a] + ([b] if isinstance(node, (fx.Mix, fx.RingMod)) else [])
        cols = broadcast_shape(*((1, t.shape[1]) for t in audio + ([ctl] if ctl is not None else [])))[1]
        name = type(node).__name__
        if all(t.shape[0] == 1 for t in audio) and not mod:
            result = torch.empty((1, cols), dtype=CTRL_DTYPE, device=dev)         # every operand is a one-row reply
            return o._launch(f'elementwise[{name}]', lambda: _native.elementwise(name, a, b, c, result), units=cols)
        result = torch.empty((rows, cols), dtype=AUDIO_DTYPE, device=dev)
        main = result[hist:] if mod else result
        o._launch(f'elementwise[{name}{",per-block" if mod else ""}]',
                  lambda: _native.elementwise(name, a, b, c, main), units=main.shape[0] * cols)
        if mod:
            self._own_history(node, cols, hist, result)
        return result

    @staticmethod
    def _sole_envelope(node):
        """a RingMod that is x * envelope, the envelope an enabled ADSR with block-invariant parameters that nothing else
        reads: (the ADSR, x's port), else None"""
        for env_port, x_port in ((node.right, node.left), (node.left, node.right)):
            env = env_port.sig
            if isinstance(env, ext.ADSR) and env.get_state().enabled and len(env.outputs_with_ports) == 1 and not _modulated(env):
                return env, x_port
        return None

    def _envelope_rows(self, env) -> dict:
        """the control rows of an envelope whose parameters hold for every block (NotBatchable otherwise)"""
        return env.control_rows(lambda bound: self._control_const(bound, bound.name))

    def _enveloped_filter(self, node, channels):
        """RingMod(filter, ADSR) where nothing else reads the envelope or the filter and the filter's rows are not
        in the batch yet: (filter, ADSR control rows), else None"""
        found = self._sole_envelope(node)
        if found is not None:
            env, flt = found[0], found[1].sig
            if (isinstance(flt, fx.SingleCritFilter) and flt.get_state().enabled
                    and len(flt.outputs_with_ports) == 1 and (flt, channels) not in self._memo):
                ctl = self._envelope_rows(env)
                voices = broadcast_shape((1, 1), *(r.shape for r in ctl.values()))[1]
                if voices in (1, channels):
                    return flt, ctl
        return None

    def _ringmod_with_envelope(self, node, channels, hist, rows):
        """RingMod(x, ADSR) with an envelope nobody else reads: the envelope multiplies x on the fly -- in the
        epilogue of the filter that produces x when nothing else reads that filter (sig_biquad_coldstart_env),
        else in one envelope * x pass (sig_adsr_apply)"""
        found = self._sole_envelope(node)
        if found is None or found[1].sig is None or isinstance(found[1].sig, ext.ADSR):
            return None
        env, x_port = found
        ctl = self._envelope_rows(env)
        voices = broadcast_shape((1, 1), *(r.shape for r in ctl.values()))[1]
        flt = x_port.sig
        if (isinstance(flt, fx.SingleCritFilter) and flt.get_state().enabled and len(flt.outputs_with_ports) == 1
                and voices in (1, channels) and (flt, channels) not in self._memo):
            return self._filter(flt, channels, hist, rows, envelope=ctl, owner_node=node)
        x = self._operand(x_port, channels, hist)
        if x.shape[0] == 1 or x.shape[1] != voices or x.dtype != AUDIO_DTYPE:
            return None
        result = torch.empty((rows, voices), dtype=AUDIO_DTYPE, device=runtime.device())
        start = self.pos - hist
        return self.owner._launch('adsr_apply', lambda: _native.adsr_apply(start, self.rate, ctl, x, result),
                                  units=rows * voices)

    def _sched_bus(self, node, channels, hist, rows):
        o = self.owner
        src_port, gains = node.input, node.resident_gains()
        top = node.input.sig
        if (o.fuse and isinstance(top, fx.Gain) and top.get_state().enabled and _ctl_const(top.right)
                and len(top.outputs_with_ports) == 1 and top.left.sig is not None):
            # a per-voice Gain feeding only this bus is a diagonal scaling of the mix weights:
            # sum_v pan[c,v] * (g[v] * x[n,v]) = sum_v (pan[c,v] * g[v]) * x[n,v]  -- fold it, skip the launch
            g = self._control_const(top.right, 'right')
            voices = top.left.channels
            if g.shape[1] in (1, voices) and (gains is None or gains.shape[1] == voices):
                gains = (gains * g) if gains is not None else g.expand(1, voices).contiguous()
                src_port = top.left
                self._require(src_port.sig, voices, hist)
        fused = self._bus_over_cascade(node, src_port, gains, rows) if o.fuse_cascade and hist == 0 else None
        if fused is None and o.fuse_program and hist == 0:
            fused = self._program_bus(node, src_port, gains, rows)
        if fused is None:
            fused = self._bus_over_filter(node, src_port, gains, hist, rows) if o.fuse and hist == 0 else None
        if fused is not None:
            return fused
        x = self._operand(src_port, src_port.channels, hist)
        if x.shape[0] == 1:
            raise NotBatchable('SumBus over a one-row input')
        result = torch.empty((rows, node.channels), dtype=AUDIO_DTYPE, device=runtime.device())
        return o._launch('sum_bus', lambda: _native.sum_bus(x, gains, result), units=rows * x.shape[1])

    def _program_store(self, node, channels):
        """the per-voice graph under `node` as one interpreted launch (sig_voice_program) storing its rows, or None"""
        memo_keys = {k[0] for k in self._memo}
        prog = _VoiceProgram.compile(self, node, channels, mixed=self.owner.mixed_programs)
        if prog is None or any(n in memo_keys for n in prog.uses if n is not node):
            return None                                                        # (an inner node already has rows in this batch: someone else reads it)
        if self.owner.fuse_program != 'always' and not prog.worthwhile():
            return None
        # the node's natural width: every control row is one column wide -> the reply is (rows, 1), broadcast by the consumer
        try:
            tensors = [c if c is not None else self._control_const(p, p.name) if _ctl_const(p) else None for p, c, _ in prog.controls]
        except NotBatchable:
            return None
        wide = any(t is None or t.shape[1] > 1 for t in tensors) or any(isinstance(n, (noise.White, ext.ADSR)) for n in prog.uses)
        voices = channels if wide else 1
        if voices != channels:
            prog = _VoiceProgram.compile(self, node, voices, mixed=self.owner.mixed_programs)
            if prog is None:
                return None
        out = torch.empty((self.N * self.K, voices), dtype=AUDIO_DTYPE, device=runtime.device())
        try:
            return prog.launch(out, None, False, f'voice_program[{prog.describe()}]')
        except (_NoProgram, NotBatchable):
            return None                                                        # (the per-node schedule decides: it may refuse the batch as a whole)

    def _program_bus(self, node, src_port, gains, rows):
        """SumBus over a per-voice graph no fused kernel covers: graph and bus in one interpreted launch, or None"""
        voices, C = src_port.channels, node.channels
        if C not in (1, 2) or voices is None or (gains is not None and gains.shape[1] != voices):
            return None
        memo_keys = {k[0] for k in self._memo}
        prog = _VoiceProgram.compile(self, src_port.sig, voices, min_nodes=1, mixed=self.owner.mixed_programs)
        if prog is None or any(n in memo_keys for n in prog.uses):
            return None
        if self.owner.fuse_program != 'always' and not prog.worthwhile():
            return None
        if len(src_port.sig.outputs_with_ports) != 1:
            return None                                                        # (the bus input has another reader: its rows must exist)
        out = torch.empty((rows, C), dtype=AUDIO_DTYPE, device=runtime.device())
        try:
            result = prog.launch(out, gains, True, f'voice_program_bus[{prog.describe()}]')
        except (_NoProgram, NotBatchable):
            return None
        if prog.depth:
            self.owner._virtual_history.add(node)
        return result

    def _bus_over_cascade(self, node, src_port, gains, rows):
        """SumBus([RingMod(] Filter2(Filter1(Osc)) [, ADSR)]) with block-invariant controls and no other reader of any of
        them: the whole voice in ONE launch (sig_fused_cascade_bus), nothing per-voice through HBM.  The reference's
        cache history between the two filters is reproduced inside the kernel from where the previous
        block started: position - N on a continuing stream, position - min(100, position) on a fresh graph."""
        o, top, voices, N = self.owner, src_port.sig, src_port.channels, self.N
        C = node.channels
        if C not in (1, 2, 4) or N <= CONTEXT or N % (16 // C):
            return None

        def sole(n, kind):
            return (isinstance(n, kind) and n.get_state().enabled and len(n.outputs_with_ports) == 1 and (n, voices) not in self._memo)
        ctl = None
        f2 = top
        if sole(top, fx.RingMod) and not _modulated(top):
            found = self._sole_envelope(top)
            if found is None or (found[0], voices) in self._memo or not isinstance(found[1].sig, fx.SingleCritFilter):
                return None
            ctl, f2 = self._envelope_rows(found[0]), found[1].sig
        if not sole(f2, fx.SingleCritFilter):
            return None
        f1 = f2.input.sig
        if not sole(f1, fx.SingleCritFilter):
            return None
        src = f1.input.sig
        if not sole(src, osc.Osc) or any(not _ctl_const(p) for p in (src.hertz, src.phase, f1.cutoff, f2.cutoff)):
            return None
        hertz, phase = self._control_const(src.hertz, 'hertz'), self._control_const(src.phase, 'phase')
        cut1, cut2 = self._control_const(f1.cutoff, 'cutoff'), self._control_const(f2.cutoff, 'cutoff')
        if max(hertz.shape[1], phase.shape[1]) != voices or cut1.shape[1] != voices or cut2.shape[1] != voices:
            return None                                                        # (the reference indexes cutoff[0, i] per channel)
        if any(t.shape[1] not in (1, voices) for t in (hertz, phase, *(ctl or {}).values())):
            return None
        if gains is not None and gains.shape[1] != voices:
            return None
        if self.pos == 0:
            history = 0
        elif self.continuing:
            # the block in front of this batch: the kernel re-walks it from where the reference cold-started it.  Only if
            # the previous render kept its history implicit as well (a per-node batch left tails of rounded float32 rows)
            # and that block covers the outer filter's context
            if node not in o._cascade_stream or not o._prev_block_frames or o._prev_block_frames < min(CONTEXT, self.pos):
                return None
            history = self.pos - o._prev_block_frames
        else:
            history = self.pos - min(CONTEXT, self.pos)
        result = torch.empty((rows, C), dtype=AUDIO_DTYPE, device=runtime.device())
        o._bus_workspace(voices, rows, C)
        status = o._status_word(f2)                                            # one word for the launch: both designs report here
        kind, t1, t2 = src.kind(), str(f1.type()), str(f2.type())
        o._virtual_history.add(node)
        out = o._launch(f'fused_cascade_bus[{kind},{t1},{t2}{",env" if ctl else ""}]',
                        lambda: _native.fused_cascade_bus(kind, t1, t2, self.rate, self.pos, history, N, self.K, CONTEXT, voices,
                                                          hertz, phase, cut1, cut2, None, ctl, gains, result,
                                                          workspace=o._workspace, status=status),
                        units=rows * voices)
        return out

    def _bus_over_filter(self, node, src_port, gains, hist, rows):
        """SumBus(Filter(x)) / SumBus(RingMod(Filter(x), ADSR)) with no other reader of the filter (and of the
        RingMod and the envelope): one pass over x, nothing per-voice stored (sig_biquad_coldstart_bus)"""
        o, top, voices = self.owner, src_port.sig, src_port.channels
        if node.channels not in (1, 2, 4):                                     # the bus widths the tile reduction is built for
            return None
        if top is None or not top.get_state().enabled or len(top.outputs_with_ports) != 1 or (top, voices) in self._memo:
            return None
        flt, ctl = top, None
        if isinstance(top, fx.RingMod) and not _modulated(top):
            found = self._enveloped_filter(top, voices)
            if found is None:
                return None
            flt, ctl = found
        if not isinstance(flt, fx.SingleCritFilter) or not flt.get_state().enabled or (flt, voices) in self._memo:
            return None
        if gains is not None and gains.shape[1] != voices:
            return None
        cutoff, window, c0 = self._filter_window(flt, voices)
        if window.dtype != AUDIO_DTYPE or window.shape[1] != voices:
            return None
        result = torch.empty((rows, node.channels), dtype=AUDIO_DTYPE, device=runtime.device())
        o._bus_workspace(voices, rows, node.channels)
        btype, status = str(flt.type()), o._status_word(flt)
        return o._launch(f'biquad_bus[{btype}{",env" if ctl else ""}]',
                         lambda: _native.biquad_coldstart_bus(btype, self.rate, self.pos, self.N, self.K, CONTEXT, cutoff,
                                                              window, c0, gains, result, envelope=ctl,
                                                              workspace=o._workspace, status=status),
                         units=rows * voices)

    def _sched_tap(self, node, channels, hist, rows):
        return self._materialise(node.input.sig, channels)                    # pass-through: same buffer

    def _sched_file_writer(self, node, channels, hist, rows):
        full, have = self._materialise(node.input.sig, channels)              # pass-through + record the batch
        if full.shape[0] > 1:
            node.write_rows(self.pos, self.rate, channels, full[have:])
        return full, have

    def _sched_file_reader(self, node, channels, hist, rows):
        result = node.read_rows(self.pos - hist, rows, self.rate, channels)
        if result.shape[0] != rows:
            raise NotBatchable('FileReader ran past the end of the file inside a batch')
        return result

    def _sched_adsr(self, node, channels, hist, rows):
        ctl = self._envelope_rows(node)
        _, voices = broadcast_shape((1, 1), *(r.shape for r in ctl.values()))
        result = torch.empty((rows, voices), dtype=AUDIO_DTYPE, device=runtime.device())
        start = self.pos - hist
        return self.owner._launch('adsr', lambda: _native.adsr(start, self.rate, ctl, result), units=rows * voices)

    def _sched_mix_matrix(self, node, channels, hist, rows):
        x = self._operand(node.input, channels, hist)
        if x.shape[0] == 1 or x.shape[1] % 64:
            raise ValueError(f'MixMatrix needs (rows, 64*g) audio, got {tuple(x.shape)}')
        if x.dtype != AUDIO_DTYPE or not x.is_contiguous():
            x = x.to(AUDIO_DTYPE).contiguous()
        matrix = node.resident_matrix()
        result = torch.empty_like(x)
        return self.owner._launch('mix_matrix', lambda: _native.mix_matrix(x, matrix, result),
                                  units=x.shape[0] * x.shape[1])

    def _sched_merge(self, node, channels, hist, rows):
        left = self._operand(node.left, node.left.channels, hist)
        right = self._operand(node.right, node.right.channels, hist)
        if left.shape[0] != right.shape[0]:
            raise ValueError('all the input array dimensions except for the concatenation axis must match exactly')
        return torch.cat((left.to(AUDIO_DTYPE), right.to(AUDIO_DTYPE)), dim=1)     # buffer plumbing

    def _sched_foreign(self, node, channels, hist, rows):
        """A node class without a kernel schedule (a plugin, e.g. one written against the reference and answering numpy
        arrays, chain/__init__.py:245-247): its K blocks are pulled one request at a time through its own respond() --
        which pulls ITS inputs through the eager path -- and laid out as one batch buffer, so everything downstream
        still runs one launch per node.  History rows come from the previous batch's tail or a fresh block request."""
        from signals_amd.chain import BadShape, BlockLoc, Request, Shape, adopt_reply
        N, K = self.N, self.K
        blocks = []
        for b in range(K):
            loc = BlockLoc(position=self.pos + b * N, rate=self.rate, shape=Shape(frames=N, channels=channels))
            block = adopt_reply(node.respond(Request(requestor=self.owner.requestor, port='input', loc=loc)))
            if not (Shape.of_array(block) <= loc.shape):
                raise BadShape(node, block.shape, loc.shape)
            blocks.append(block)
        widths = {int(b.shape[1]) for b in blocks}
        if len(widths) != 1:
            raise NotBatchable(f'{node.cls_name()} answered blocks of different widths {sorted(widths)}')
        if all(b.shape[0] == 1 for b in blocks) and K == 1:
            return blocks[0].to(CTRL_DTYPE)                                   # a one-row reply broadcasts, like a Fixed
        result = torch.empty((rows, widths.pop()), dtype=AUDIO_DTYPE, device=runtime.device())
        for b, block in enumerate(blocks):
            result[hist + b * N: hist + (b + 1) * N] = block                  # (a one-row reply broadcasts over its block)
        self._own_history(node, result.shape[1], hist, result)
        return result

    _SCHEDULES = (
        (fixed.Fixed, _sched_fixed),
        (osc.Osc, _sched_osc),
        (ext.PMOsc, _sched_pm),
        ((ext.Wavetable, ext.UnisonOsc, ext.Sampler, ext.Modal), _sched_bank),
        (noise.White, _sched_noise),
        (fx.CritFilter, _sched_filter),
        ((fx.Mix, fx.RingMod, fx.Gain, fx.Amp), _sched_elementwise),
        (ext.Shaper, _sched_shaper),
        (ext.Delay, _sched_delay),
        (ext.SumBus, _sched_bus),
        (ext.Tap, _sched_tap),
        (files.FileWriter, _sched_file_writer),
        (files.FileReader, _sched_file_reader),
        (ext.ADSR, _sched_adsr),
        (ext.MixMatrix, _sched_mix_matrix),
        (shape.Merge, _sched_merge),
    )

    # -------------------------------------------------------------- filters
    @staticmethod
    def _narrow(control: torch.Tensor, channels: int) -> torch.Tensor:
        """the first `channels` columns of a filter's control rows, contiguous; narrower: the reference's IndexError (it indexes
        crit[0, i] for every channel i, fx.py:99)"""
        if control.shape[1] < channels:
            raise IndexError(f'index {control.shape[1]} is out of bounds for axis 1 with size {control.shape[1]}')
        control = control[:, :channels]
        return control if control.is_contiguous() else control.contiguous()

    def _filter_window(self, node: fx.CritFilter, channels: int, cutoff: torch.Tensor | None = None, narrow_ok: bool = False):
        """(cutoff rows, input window with c0 = min(100, pos) context rows in front, c0) of a filter; `cutoff`
        defaults to the single-cutoff filters' control rows.  `narrow_ok` (ext.Delay): a one-column window or control row
        broadcasts over the voices instead of raising"""
        N, K, pos = self.N, self.K, self.pos
        if cutoff is None:
            cutoff = self._control(node.cutoff, 'cutoff')
        c0 = min(CONTEXT, pos)
        src = node.input.sig
        pure_in = _is_pure(src, self._pure)
        if not pure_in and N <= CONTEXT and (K > 1 or self.continuing):
            raise NotBatchable('cascaded filters with block size <= 100 depend on the after-window cache entries')
        window, have = self._materialise(src, channels)
        if window.shape[0] == 1:
            raise ValueError('filter input answered a single row (unplugged or disabled input)')
        window = window[have - c0:] if have != c0 else window
        if window.shape[1] < channels and not (narrow_ok and window.shape[1] == 1):
            raise IndexError(f'index {window.shape[1]} is out of bounds for axis 1 with size {window.shape[1]}')
        if narrow_ok and cutoff.shape[1] == 1:
            return cutoff, window[:, :channels], c0
        return self._narrow(cutoff, channels), window[:, :channels], c0

    def _filter(self, node: fx.CritFilter, channels: int, hist: int, rows: int, envelope: dict | None = None,
                owner_node: Emitter | None = None) -> torch.Tensor:
        """`envelope` / `owner_node`: the filter runs on behalf of RingMod(filter, ADSR) -- its stored rows are
        multiplied by the envelope and the buffer (history rows, tail) belongs to that RingMod node"""
        if isinstance(node, ext.Ladder):
            return self._ladder(node, channels, hist, rows)
        if isinstance(node, ext.FIR):
            return self._fir(node, channels, hist, rows)
        o = self.owner
        N, K, pos = self.N, self.K, self.pos
        band = isinstance(node, fx.DoubleCritFilter)
        cutoff, window, c0 = self._filter_window(node, channels, self._control(node.low, 'low') if band else None)
        result = torch.empty((rows, channels), dtype=AUDIO_DTYPE, device=window.device)
        main = result[hist:]
        btype = str(node.type())
        status = o._status_word(node)
        if band:
            high = self._narrow(self._control(node.high, 'high'), channels)
            if cutoff.shape[0] == 1 and high.shape[0] == 1:
                o._launch(f'band_coldstart[{btype}]',
                          lambda: _native.band_coldstart(btype, self.rate, pos, N, K, CONTEXT, cutoff, high, window, c0, main,
                                                         status=status),
                          units=N * K * channels)
            else:                                                              # a swept band: one design per block
                o._launch(f'band_coldstart[{btype},blocks]',
                          lambda: _native.band_coldstart_blocks(btype, self.rate, pos, N, K, CONTEXT, cutoff, high, window, c0,
                                                                main, status=status),
                          units=N * K * channels)
        elif isinstance(node, ext.ResonantFilter):
            # the resonant low-pass / high-pass: a second control row, each of the two per block on its own (a swept cutoff, a swept q)
            q = None if _ctl_unplugged(node.resonance) else self._narrow(self._control(node.resonance, 'resonance'), channels)
            swept = cutoff.shape[0] > 1 or (q is not None and q.shape[0] > 1)
            if isinstance(node, ext.EqFilter):
                # the equaliser biquads: a third control row for the three gain classes, per block on its own like the other two
                gp = node.gain_port()
                gain = None if gp is None or _ctl_unplugged(gp) else self._narrow(self._control(gp, 'gain'), channels)
                swept = swept or (gain is not None and gain.shape[0] > 1)
                o._launch(f'biquad_coldstart_eq[{btype}{",blocks" if swept else ""}]',
                          lambda: _native.biquad_coldstart_eq(btype, self.rate, pos, N, K, CONTEXT, cutoff, q, gain, window, c0, main,
                                                              status=status),
                          units=N * K * channels)
            else:
                o._launch(f'biquad_coldstart_q[{btype}{",blocks" if swept else ""}]',
                          lambda: _native.biquad_coldstart_q(btype, self.rate, pos, N, K, CONTEXT, cutoff, q, window, c0, main, status=status),
                          units=N * K * channels)
        else:
            o._launch(f'biquad_coldstart[{btype}{",env" if envelope else ""}]',
                      lambda: _native.biquad_coldstart(btype, self.rate, pos, N, K, CONTEXT, cutoff, window, c0, main,
                                                       status=status, envelope=envelope),
                      units=N * K * channels)
        self._own_history(owner_node or node, channels, hist, result)
        return result

    def _window_node(self, node, channels: int, hist: int, rows: int, control: torch.Tensor, bind, uncached=None) -> torch.Tensor:
        """the schedule of a node that takes a filter's window and one launch over the K blocks (ext.Delay, ext.FIR, ext.Ladder): the
        window with c0 = min(100, pos) context rows in front (`_filter_window`: the same NotBatchable for an impure input at N <= 100),
        the result as wide as the window and the first control row `control` broadcast, `bind(window, c0, control, main) -> (label,
        launch)` for rows [hist:], and the node's own history rows from the tail or a fresh block (`_own_history`).  A one-column
        input or control row broadcasts over the voices.  A request-dependent one-column input is answered afresh for every context
        request on the eager path (`_delay_uncached` has the story): `uncached(blocks, control, main)` renders that, without one the
        schedule does not reproduce it: NotBatchable"""
        control, window, c0 = self._filter_window(node, channels, control, narrow_ok=True)
        cols = max(window.shape[1], control.shape[1])
        result = torch.empty((rows, cols), dtype=AUDIO_DTYPE, device=window.device)
        main = result[hist:]
        if window.shape[1] < channels and not _is_pure(node.input.sig, self._pure):
            if uncached is None:
                raise NotBatchable(f'{node.cls_name()} over a request-dependent input of one column (the eager path answers its context '
                                   f'requests afresh)')
            uncached(window[c0:], control, main)
        else:
            label, launch = bind(window, c0, control, main)
            self.owner._launch(label, launch, units=self.N * self.K * cols)
        self._own_history(node, cols, hist, result)
        return result

    def _ladder(self, node: ext.Ladder, channels: int, hist: int, rows: int) -> torch.Tensor:
        """the 4-pole ladder: a window node (`_window_node`), one sig_ladder_coldstart launch over the K blocks; the cutoff, the
        resonance and the drive rows each per block on their own when that port is modulated, the last two None when unplugged.  The
        cutoff is as wide as the voices, so is the result; a position-pure one-column input is widened for the kernel"""
        def bind(window, c0, cutoff, main):
            if window.shape[1] < channels:
                window = window.expand(-1, channels).contiguous()
            k, drive = (None if row is None else self._narrow(row, channels)
                        for row in node.control_rows(lambda bound: self._control(bound, bound.name)))
            poles = int(node.get_state().poles)
            swept = any(row is not None and row.shape[0] > 1 for row in (cutoff, k, drive))
            status = self.owner._status_word(node)
            return (f'ladder_coldstart[{poles}{",drive" if drive is not None else ""}{",blocks" if swept else ""}]',
                    lambda: _native.ladder_coldstart(self.rate, self.pos, self.N, self.K, CONTEXT, cutoff, k, drive, poles, window, c0, main,
                                                     status=status))
        return self._window_node(node, channels, hist, rows, self._narrow(self._control(node.cutoff, 'cutoff'), channels), bind)

    def _fir(self, node: ext.FIR, channels: int, hist: int, rows: int) -> torch.Tensor:
        """the dense FIR filter: a window node (`_window_node`), one sig_fir_taps launch over the K blocks -- per-block select rows when
        that port is modulated; the table is the node's resident copy"""
        def bind(window, c0, select, main):
            table = node.resident_table()
            return (f'fir_taps[{table.shape[0]}{",per-block" if select.shape[0] > 1 else ""}]',
                    lambda: _native.fir_taps(self.rate, self.pos, self.N, self.K, window, c0, select, table, main))
        return self._window_node(node, channels, hist, rows, self._control(node.select, 'select'), bind)

    def _own_history(self, node: Emitter, channels: int, hist: int, result: torch.Tensor) -> None:
        """rows [:hist] of a request-dependent node (filter, or a node with per-block control): the previous
        batch's tail when the stream continues, else the node rendered as its own block [pos-hist, pos) -- what
        the reference's block cache, respectively a fresh graph, would answer"""
        if not hist:
            return
        o, pos = self.owner, self.pos
        tail = o._tails.get(node) if self.continuing else None
        if tail is None and self.continuing and o._cascade_stream and not o._tails_rebuilt:
            o._rebuild_tails(pos)                                              # (the previous batch kept this history implicit)
            tail = o._tails.get(node)
        if tail is not None and tail[0] == pos and tail[1].shape[0] >= hist and tail[1].shape[1] >= channels:
            result[:hist].copy_(tail[1][tail[1].shape[0] - hist:, :channels])
        else:
            sub = _Batch(o, pos - hist, hist, 1, False)
            sub.history_of = pos
            result[:hist].copy_(sub.buffer(node, channels, 0))

    def impure_outputs(self):
        return self._impure.items()


assert set(_KNOWN_TYPES) == {t for types, _ in _Batch._SCHEDULES for t in (types if isinstance(types, tuple) else (types,))}
