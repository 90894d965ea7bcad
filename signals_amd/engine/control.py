"""The block-rate control programs: the subgraphs under control ports compiled into one sig_control_program launch."""
from __future__ import annotations

import torch

from signals_amd import _native, runtime
from signals_amd.chain import CTRL_DTYPE, Emitter, as_control, broadcast_shape
from signals_amd.chain import ext, fixed, fx, noise, osc
from signals_amd.engine.graph import NotBatchable, _ctl_const, _no_block_rate


class _ControlProgram:
    """The block-rate subgraphs under a set of control ports as ONE launch (sig_control_program): oscillators evaluated at
    one frame per block, element-wise nodes, Fixed rows, ADSR envelopes -- the same expressions as the node-by-node launches of
    `_Batch._control_node`, so the same bits.  Compiled once per (ports, K, graph version); Fixed rows are re-checked per run
    (an edited value re-uploads into a new tensor: recompile).  Outputs are owned by the program and overwritten by the
    next run -- their consumers are launches enqueued before that on the same stream."""

    def __init__(self, srcs: tuple, K: int, lead: int = 0, into: dict | None = None, channels: int | None = None, status=None):
        """`lead`: every computed output is rows [lead:] of a (lead + K, cols) buffer `self.full[i]` whose row lead - 1 is the
        `front` row -- the layout sig_voice_program takes its per-block rows in ([rows in front | K blocks]); `into`: {source
        index: (K, cols) tensor} to write into instead of buffers of its own (rows of another program's `full`); `channels`: the
        width of the request the ports are read for (a LowPass / HighPass / White in the subgraph answers exactly that many
        columns); `status`: node -> its status word tensor (the control filters')"""
        self.srcs, self.K = srcs, K
        self.channels, self._status = channels, status
        self._window: dict | None = None                   # inside a filter's input: node -> (register, cols), window-rate
        self.full: dict[int, torch.Tensor] = {}
        self.ins: list = []
        self.keep: list[torch.Tensor] = []                  # tensors the instructions point into
        self.fixed: list[tuple[fixed.Fixed, torch.Tensor]] = []
        self._reg: dict = {}
        dev = runtime.device()
        self._zero = torch.zeros((1, 1), dtype=CTRL_DTYPE, device=dev)
        self.results: list = []                             # per source: a constant row, None (a Fixed: its resident row, per run) or the output
        self.fronts: dict[int, torch.Tensor] = {}           # per computed source: its (1, cols) row at the front position
        outs = []
        for src in srcs:
            if src is None or not src.get_state().enabled:
                self.results.append(Emitter.empty_result())
            elif isinstance(src, fixed.Fixed):
                if src.resident().shape[0] != 1:
                    raise NotBatchable('multi-row Fixed on a control port')
                self.results.append(None)                   # its resident row, fetched per run
            else:
                reg, cols = self._emit(src)
                i = len(self.results)
                if into is not None:
                    out = into[i]
                    if tuple(out.shape) != (K, cols) or not out.is_contiguous():
                        raise NotBatchable('control rows of another width than the buffer they go into')
                    front = torch.empty((1, cols), dtype=CTRL_DTYPE, device=dev)
                elif lead:
                    self.full[i] = torch.empty((lead + K, cols), dtype=CTRL_DTYPE, device=dev)
                    out, front = self.full[i][lead:], self.full[i][lead - 1:lead]
                else:
                    out = torch.empty((K, cols), dtype=CTRL_DTYPE, device=dev)
                    front = torch.empty((1, cols), dtype=CTRL_DTYPE, device=dev)
                outs.append(_native.CtlOut(reg, cols, out.data_ptr(), front.data_ptr()))
                self.results.append(out)
                self.fronts[i] = front
        self.cols = max([c for _, c in self._reg.values()] + [1])
        # Row instructions first (they depend on nothing; the kernel keeps the one-column ones' loads four in flight), registers renumbered
        row_op = _native.CTL_OPS['Row']
        rank = lambda x: 2 if x.op != row_op else (0 if x.cols == 1 else 1)      # one-column rows, wide rows, the rest
        order = sorted(range(len(self.ins)), key=lambda i: (rank(self.ins[i]), i))
        new_of = {old: new for new, old in enumerate(order)}
        self.ins = [self.ins[i] for i in order]
        for x in self.ins:
            x.dst = new_of[x.dst]
            x.a, x.b, x.c = (new_of.get(r, -1) for r in (x.a, x.b, x.c))
        for o in outs:
            o.reg = new_of[o.reg]
        self.n_ins, self.n_outs = len(self.ins), len(outs)
        self.windowed = any(x.op in _native.CTL_WINDOWED_OPS for x in self.ins)      # (sig_control_program_windowed)
        self.envelope = any(x.op in _native.CTL_ENVELOPE_OPS for x in self.ins)      # (sig_control_program_envelope)
        self.description = _native.control_program_description(self.ins, outs)     # (its structure: what a specialised kernel is built for)
        self.program_t = _native.upload_structs(self.ins) if self.ins else None
        self.outs_t = _native.upload_structs(outs) if outs else None

    def _row(self, t: torch.Tensor) -> tuple[int, int]:
        if t.shape[0] != 1:
            raise NotBatchable('multi-row Fixed on a control port')
        t = as_control(t)
        self.keep.append(t)
        cols = t.shape[1]
        return self._push(_native.CtlIns(_native.CTL_OPS['Row'], 0, -1, -1, -1, 0, 0 if cols == 1 else 1, 1, cols, 0, t.data_ptr()), cols)

    def _push(self, ins, cols: int) -> tuple[int, int]:
        reg = len(self.ins)
        if reg >= _native.CTL_MAX_REGS:
            raise NotBatchable('control subgraph larger than one program')
        ins.dst = reg
        self.ins.append(ins)
        return reg, cols

    def _emit(self, src, window: bool = False) -> tuple[int, int]:
        """(register, columns) of a node's value at block rate; `window`: the node is part of a control filter's input and is
        evaluated per window row (`reserved` = 1), its own control ports must then hold for every row (Fixed / unplugged).
        A constant row is emitted at block rate in either place"""
        if src is None or not src.get_state().enabled:
            if None not in self._reg:
                self._reg[None] = self._row(self._zero)
            return self._reg[None]
        window = window and not isinstance(src, fixed.Fixed)
        regs = self._window if window else self._reg
        if src in regs:
            return regs[src]

        def control(port):
            if window and not _ctl_const(port):
                raise NotBatchable(f'{src.cls_name()} inside a control filter\'s input has a modulated {port.name}')
            return self._emit(port.sig)
        if isinstance(src, fixed.Fixed):
            row = src.resident()
            self.fixed.append((src, row))
            got = self._row(row)
        elif isinstance(src, osc.Osc):
            (a, ca), (b, cb) = control(src.hertz), control(src.phase)
            got = self._push(_native.CtlIns(_native.CTL_OPS['Osc'], _native.OSC_KINDS[src.kind()], a, b, -1, 0, 0, 0, max(ca, cb),
                                            int(window), None), max(ca, cb))
        elif isinstance(src, (fx.Gain, fx.Amp, fx.Mix, fx.RingMod)):
            a, ca = self._emit(src.left.sig, window)
            b, cb = control(src.right) if isinstance(src, (fx.Gain, fx.Amp)) else self._emit(src.right.sig, window)
            c, cc = control(src.mix) if isinstance(src, fx.Mix) else (-1, 1)
            cols = broadcast_shape((1, ca), (1, cb), (1, cc))[1]
            got = self._push(_native.CtlIns(_native.CTL_OPS[type(src).__name__], 0, a, b, c, 0, 0, 0, cols, int(window), None), cols)
        elif isinstance(src, ext.ADSR):
            # the envelope read at one frame: six block-rate registers, three of them in the carrier word right in front (an
            # instruction has three operands; the re-ordering above is stable, so the pair stays together)
            (at, de, su, re, on, off), widths = zip(*(control(getattr(src, name)) for name in _native.ADSR_PARAMS))
            cols = broadcast_shape(*((1, c) for c in widths))[1]
            self._push(_native.CtlIns(_native.CTL_OPS['AdsrArgs'], 0, re, on, off, 0, 0, 0, cols, int(window), None), cols)
            got = self._push(_native.CtlIns(_native.CTL_OPS['Adsr'], 0, at, de, su, 0, 0, 0, cols, int(window), None), cols)
        elif isinstance(src, noise.White):
            got = self._push(self._noise(src, window), self._request_width(src))
        elif _no_block_rate(src, 'program', window) is not None:       # (ahead of the filters: a resonant or ladder filter is a CritFilter)
            raise NotBatchable(_no_block_rate(src, 'program', window))
        elif window and isinstance(src, fx.CritFilter):
            raise NotBatchable('a filter whose input contains a filter, in a control path')
        elif isinstance(src, fx.SingleCritFilter):
            got = self._filter(src)
        elif isinstance(src, fx.DoubleCritFilter):
            raise NotBatchable(f'{src.cls_name()} in a control path: only LowPass / HighPass run at block rate')
        elif window:
            raise NotBatchable(f'no window-rate program for {src.cls_name()} inside a control filter\'s input')
        else:
            raise NotBatchable(f'no block-rate program for {src.cls_name()}')
        regs[src] = got
        return got

    def _request_width(self, src) -> int:
        if self.channels is None:
            raise NotBatchable(f'{src.cls_name()} in a control path whose request width is not known here')
        return self.channels

    def _noise(self, src, window: bool):
        cols = self._request_width(src)
        return _native.CtlIns(_native.CTL_OPS['Noise'], 0, -1, -1, -1, 0, 0, 0, cols, int(window), src.get_state().seed)

    def _filter(self, src) -> tuple[int, int]:
        """a LowPass / HighPass read at one frame: its cutoff as a block-rate register, its input subgraph as the window-rate
        run right in front of the filter instruction (control_program.hip)"""
        if self._window is not None:
            raise NotBatchable('a filter whose input contains a filter, in a control path')
        width = self._request_width(src)
        cut, ccut = self._emit(src.cutoff.sig)
        inp = src.input.sig
        if inp is None or not inp.get_state().enabled or isinstance(inp, fixed.Fixed):
            raise NotBatchable(f'{src.cls_name()} in a control path over a one-row input')
        self._window = {}
        try:
            a, ca = self._emit(inp, window=True)
            inside = set(self._window)
        finally:
            self._window = None
        for n in inside:                                   # (what feeds the filter is evaluated per window row, for it alone)
            if any(r is not src and r not in inside for _, r in n.outputs_with_ports):
                raise NotBatchable(f'{n.cls_name()} inside a control filter\'s input has a reader outside that filter')
        if ca < width or ccut < width:                     # fx.py:110-113: the eager path raises IndexError
            raise NotBatchable(f'{src.cls_name()} in a control path narrower than its request')
        status = None if self._status is None else self._status(src)
        return self._push(_native.CtlIns(_native.CTL_OPS['Filter'], _native.FILT_TYPES[str(src.type())], a, cut, -1, 0, 0, 0,
                                         width, 0, None if status is None else status.data_ptr()), width)

    def current(self) -> bool:
        return all(f.resident() is t for f, t in self.fixed)

    def run(self, owner, rate: int, position: int, step: int, front_position: int = -1, min_position: int = 0):
        """the K-row replies; with `front_position` also the (1, cols) replies at that position -> (rows, fronts)"""
        if self.n_outs:
            handle = None
            if owner.specialise:                              # the kernel built for this program's structure (signals_amd/specialise.py)
                from signals_amd import specialise
                handle = specialise.ensure_control(self.description, background=owner.specialise == 'background')
            if handle is not None:
                owner._launch('control_program[block-rate]*specialised',
                              lambda: _native.control_program_attached(handle, rate, position, step, self.K, self.cols, self.program_t,
                                                                       self.n_ins, self.outs_t, self.n_outs, front_position, min_position),
                              units=self.K * self.cols)
            else:
                owner._launch('control_program[block-rate]',
                              lambda: _native.control_program(rate, position, step, self.K, self.cols, self.program_t, self.n_ins,
                                                              self.outs_t, self.n_outs, front_position, min_position,
                                                              windowed=self.windowed, envelope=self.envelope), units=self.K * self.cols)
        rows = [as_control(src.resident()) if r is None else r for src, r in zip(self.srcs, self.results)]
        if any(t.shape[0] not in (1, self.K) or (r is None and t.shape[0] != 1) for t, r in zip(rows, self.results)):
            raise NotBatchable('multi-row Fixed on a control port')             # (edited since the program was compiled)
        if front_position < 0:
            return rows
        return rows, [self.fronts.get(i, rows[i]) for i in range(len(rows))]


class _ProgramRows:
    """The per-block rows of a voice program's computed control ports, laid out as sig_voice_program takes them, each port one
    (control_rows, cols) buffer filled by block-rate control programs (sig_control_program) that write straight into it:
      blocks >= context:  [the block in front | H history blocks | K blocks]   -- the K rows and the row in front of them in one
                          launch, one more launch of one row per further row in front;
      blocks <  context:  [K virtual blocks, controls at max(p - context, 0) | K blocks]; the second group evaluated at the
                          blocks' own positions (`inner` False) or where the oldest cached reply containing the block was
                          evaluated (`inner`: the ports in front of the voice's last filter; header of sig_voice_program)."""

    def __init__(self, srcs: tuple, K: int, lead: int, small: bool, channels: int | None = None, status=None):
        self.srcs, self.K, self.lead, self.small = srcs, K, lead, small
        more = dict(channels=channels, status=status)
        if not small:
            self.main = _ControlProgram(srcs, K, lead=lead, **more)
            self.full = self.main.full
            self.front = [_ControlProgram(srcs, 1, into={i: t[j:j + 1] for i, t in self.full.items()}, **more) for j in range(lead - 1)]
        else:
            probe = _ControlProgram(srcs, K, lead=K, **more)                   # rows [K:] of (2 K, cols) buffers: the blocks themselves
            self.main, self.full = probe, probe.full
            if probe.windowed:
                raise NotBatchable('a filter in a control path with blocks of <= 100 frames (the next block is served from the '
                                   'after-window cache)')
            self.virtual = _ControlProgram(srcs, K, into={i: t[:K] for i, t in self.full.items()}, **more)
            self.first = _ControlProgram(srcs, 1, into={i: t[K:K + 1] for i, t in self.full.items()}, **more)

    def current(self) -> bool:
        return self.main.current()

    def tensors(self) -> list:
        """per source: its rows -- the filled buffer, or the resident (1, cols) row of a Fixed / an unplugged port"""
        return [self.full.get(i, r if r is not None else as_control(src.resident()))
                for i, (src, r) in enumerate(zip(self.srcs, self.main.results))]
