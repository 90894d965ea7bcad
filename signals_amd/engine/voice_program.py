"""The voice-program compiler: the per-voice graph under a node as one sig_voice_program launch."""
from __future__ import annotations

import torch

from signals_amd import _native
from signals_amd.chain import Emitter, as_control
from signals_amd.chain import ext, fixed, fx, noise, osc
from signals_amd.engine.control import _ProgramRows
from signals_amd.engine.graph import CONTEXT, NotBatchable, _audio_ports, _ctl_const, _ctl_unplugged, _is_pure, _modulated, _no_voice_program


class _NoProgram(Exception):
    """this graph is not one voice program"""


class _VoiceProgram:
    """The per-voice graph under a node as ONE launch of sig_voice_program (voice_program.hip): oscillators, LowPass / HighPass / BandPass / BandStop,
    Gain / Amp / Mix / RingMod, Fixed rows, ADSR, White, phase-modulation carriers (ext.PMOsc), wavetable oscillators (ext.Wavetable), waveshapers (ext.Shaper),
    resonant low-pass / high-pass filters (ext.ResonantFilter), equaliser biquads (ext.EqFilter), unison oscillators (ext.UnisonOsc), in any arrangement in which every voice is computed from its own
    parameters only (nothing mixes channels in front of the sink) and no inner node has a reader outside the graph.  Compiled
    here into straight-line code for the kernel's accumulator machine: a binary node parks its left operand in a temporary, a
    node with several readers is computed once and kept in one.  Control ports driven by computed block-rate signals become
    per-block rows (`_ProgramRows`).  The block history stays implicit: the launch re-walks the blocks in
    front of it from where the reference cold-started them, so no tails are kept for what it covers."""

    KERNEL_NODES = (osc.Osc, fx.SingleCritFilter, fx.DoubleCritFilter, fx.Gain, fx.Amp, fx.Mix, fx.RingMod, ext.ADSR, noise.White,
                    ext.PMOsc, ext.Wavetable, ext.Shaper, ext.ResonantFilter, ext.UnisonOsc)

    # the pairs of extension families (_native.VP_FAMILIES) no single-family variant of the interpreter holds: (one family, the
    # others it does not go with, how _NoProgram names the pair), looked up in this order -- every pair is in some row
    _NO_VARIANT = (
        ('band', {'pm'}, 'a band filter and a phase-modulation oscillator'),
        ('table', {'band', 'pm'}, 'a wavetable oscillator or a waveshaper with a band filter or a phase-modulation oscillator'),
        ('resonant', {'band'}, 'a resonant filter and a band filter'),
        ('resonant', {'pm'}, 'a resonant filter and a phase-modulation oscillator'),
        ('resonant', {'table'}, 'a resonant filter and a wavetable oscillator or a waveshaper'),
        ('unison', {'band', 'pm', 'table', 'resonant'}, 'a unison oscillator with a band filter, a phase-modulation oscillator, a wavetable '
                                                        'oscillator, a waveshaper or a resonant filter'),
    )

    def __init__(self, batch: '_Batch', top: Emitter, voices: int, mixed: bool = False):
        """`mixed`: the program may combine two or more of the extension families (_native.VP_FAMILIES); it then runs through
        sig_voice_program_mixed.  Off (the default), such a graph is not a program: _NoProgram names the pair."""
        self.batch, self.top, self.voices, self.mixed = batch, top, voices, mixed
        self.code: list = []
        self.oscs: list = []                     # (hertz control index, phase control index | None)
        self.params: list = []                   # control index per parameter register
        self.filters: list = []                  # (cutoff control index, type, level, node); a band filter: two slots, low then high
        self.bands: list = []                    # the band filter nodes
        self.resonant: list = []                 # (resonant filter node, the parameter register of its q rows | -1)
        self.gains: list = []                    # (equaliser filter node, the parameter register of its gain rows | -1)
        self.controls: list = []                 # (port | None, constant tensor | None, filters between the node and the sink)
        self.adsr = None
        self.seeds: list = []
        self.tables: list = []                   # the Wavetable / Shaper nodes whose tables the launch stages, one slot per distinct state array
        self.unison = None                       # the UnisonOsc node whose `copies` array the launch carries (one distinct array per program)
        self.temps_used, self.temps_free, self.n_temps = set(), [], 0
        self.saved: dict = {}                    # node -> [temporary, readers left]
        self.depth_of: dict = {}
        self.uses: dict = {}
        self.kernel_nodes = 0
        self._count(top)
        for n, uses in self.uses.items():
            if n is not top and len(n.outputs_with_ports) != uses:
                raise _NoProgram(f'{n.cls_name()} has a reader outside the graph')
        self.depth = self._emit(top, 0)
        if len(self.code) > _native.VP_MAX_INS:
            raise _NoProgram('program too long')
        self.families = _native.vp_families(self.code)
        words = {op for op, *_ in self.code}
        if words & set(_native.VP_SYNC_OPS) and words & set(_native.VP_EQ_OPS):
            raise _NoProgram('a hard-sync oscillator and an equaliser filter: no interpreter kernel set has both')
        if len(self.families) >= 2 and not mixed:
            has = set(self.families)
            for one, others, pair in self._NO_VARIANT:
                if one in has and has & others:
                    raise _NoProgram(f'{pair}: no interpreter variant has both')

    # ---- pass 1: readers of every node inside the graph
    def _count(self, n):
        if n is None or not n.get_state().enabled:
            if isinstance(n, ext.Tap):
                self._count(n.input.sig)
            return
        if isinstance(n, ext.Tap):
            return self._count(n.input.sig)
        self.uses[n] = self.uses.get(n, 0) + 1
        if self.uses[n] > 1:
            return
        if _no_voice_program(n) is not None:                                   # (every node `_emit` reaches has passed here first)
            raise _NoProgram(_no_voice_program(n))
        if isinstance(n, self.KERNEL_NODES):
            self.kernel_nodes += 1
        elif not isinstance(n, fixed.Fixed):
            raise _NoProgram(f'no voice-program instruction for {n.cls_name()}')
        for port in _audio_ports(n):
            self._count(port.sig)

    # ---- pass 2: code
    def _control(self, port, below: int, optional: bool = False):
        src = port.sig
        if src is None or not src.get_state().enabled:
            if optional:
                return None
            self.controls.append((None, Emitter.empty_result(), below))
        else:
            self.controls.append((port, None, below))
        return len(self.controls) - 1

    def _param(self, index: int) -> int:
        if len(self.params) >= _native.VP_MAX_PARAMS:
            raise _NoProgram('more parameter registers than the machine has')
        self.params.append(index)
        return len(self.params) - 1

    def _temp(self) -> int:
        if self.temps_free:
            t = self.temps_free.pop()
        else:
            t = self.n_temps
            self.n_temps += 1
            if self.n_temps > _native.VP_MAX_TEMPS:
                raise _NoProgram('more temporaries than the machine has')
        return t

    def _zero(self, below: int) -> int:
        self.controls.append((None, Emitter.empty_result(), below))
        self.code.append(('Const', 0, self._param(len(self.controls) - 1), 0, 0))
        return 0

    def _osc_slot(self, n, below: int) -> int:
        if len(self.oscs) >= _native.VP_MAX_OSCS:
            raise _NoProgram('more oscillators than the machine has slots')
        self.oscs.append((self._control(n.hertz, below), self._control(n.phase, below, optional=True)))
        return len(self.oscs) - 1

    def _table_slot(self, n) -> int:
        """the slot of this node's table: nodes that share one state array share a slot; together inside the LDS cap"""
        table = n.get_state().table
        for k, other in enumerate(self.tables):
            if other.get_state().table is table:
                return k
        if len(self.tables) >= _native.VP_MAX_TABLES or sum(t.get_state().table.size for t in self.tables) + table.size > _native.TABLE_MAX_POINTS:
            raise _NoProgram('more tables than the launch holds')
        self.tables.append(n)
        return len(self.tables) - 1

    def _emit(self, n, below: int) -> int:
        """code that leaves the node's sample in the accumulator; returns the filters in series up to and including it"""
        if isinstance(n, ext.Tap):
            return self._emit(n.input.sig, below)                              # a pass-through, enabled or not
        if n is None or not n.get_state().enabled:
            return self._zero(below)                                           # zeros((1, 1)) (chain/__init__.py:250-254, :297-298)
        if n in self.saved:
            slot = self.saved[n]
            self.code.append(('Load', 0, slot[0], 0, 0))
            slot[1] -= 1
            if slot[1] == 0:
                self.temps_free.append(slot[0])
                del self.saved[n]
            return self.depth_of[n]
        if isinstance(n, fixed.Fixed):
            row = n.resident()
            if row.shape[0] != 1:
                raise _NoProgram('multi-row Fixed as an audio source')
            self.controls.append((None, as_control(row), below))
            self.code.append(('Const', 0, self._param(len(self.controls) - 1), 0, 0))
            depth = 0
        elif isinstance(n, osc.Osc):
            self.code.append(('Osc', _native.OSC_KINDS[n.kind()], self._osc_slot(n, below), 0, 0))
            depth = 0
        elif isinstance(n, ext.PMOsc):
            depth = self._emit(n.mod.sig, below)                               # the modulator's sample: in the accumulator
            self.code.append(('OscPM', _native.OSC_KINDS[n.kind()], self._osc_slot(n, below), self._param(self._control(n.index, below)), 0))
        elif isinstance(n, ext.Wavetable):
            select = -1 if _ctl_unplugged(n.select) else self._param(self._control(n.select, below))
            self.code.append(('OscTable', 0, self._osc_slot(n, below), self._table_slot(n), select))
            depth = 0
        elif isinstance(n, ext.UnisonOsc):
            # an oscillator slot like Osc; the copies are the launch's one unison slot, so every node of the program shares one array
            if self.unison is not None and self.unison.get_state().copies is not n.get_state().copies:
                raise _NoProgram('two unison oscillators with distinct copies arrays: the launch carries one')
            self.unison = self.unison or n
            spread = -1 if _ctl_unplugged(n.spread) else self._param(self._control(n.spread, below))
            if isinstance(n, ext.SyncOsc):
                # OscBlep's operands and the ratio rows in a parameter register the word's b names (-1: unplugged, R = 1)
                ratio = -1 if _ctl_unplugged(n.ratio) else self._param(self._control(n.ratio, below))
                self.code.append(('OscSync', _native.OSC_KINDS[n.kind()], self._osc_slot(n, below), ratio, spread))
            else:
                word = 'OscBlep' if n.bandlimited() else 'OscUni'              # (ext.BlepOsc: the same operands, the band-limited waveforms)
                self.code.append((word, _native.OSC_KINDS[n.kind()], self._osc_slot(n, below), 0, spread))
            depth = 0
        elif isinstance(n, ext.Shaper):
            depth = self._emit(n.input.sig, below)                             # the input's sample: in the accumulator
            select = -1 if _ctl_unplugged(n.select) else self._param(self._control(n.select, below))
            self.code.append(('Shape', 0, 0, self._table_slot(n), select))
        elif isinstance(n, noise.White):
            if len(self.seeds) >= 2 or n.channels != self.voices:
                raise _NoProgram('White: two per program, as wide as the voices')
            self.seeds.append(int(n.get_state().seed))
            self.code.append(('Noise', 0, len(self.seeds) - 1, 0, 0))
            depth = 0
        elif isinstance(n, ext.ADSR):
            if (self.adsr is not None and self.adsr is not n) or _modulated(n):
                raise _NoProgram('one block-invariant envelope per program')
            self.adsr = n
            self.code.append(('Adsr', 0, 0, 0, 0))
            depth = 0
        elif isinstance(n, (fx.Gain, fx.Amp)):
            depth = self._emit(n.left.sig, below)
            self.code.append(('Gain' if isinstance(n, fx.Gain) else 'Amp', 0, self._param(self._control(n.right, below)), 0, 0))
        elif isinstance(n, (fx.Mix, fx.RingMod)):
            left = self._emit(n.left.sig, below)
            kept = self.saved.get(n.right.sig) if n.right.sig is not n.left.sig else None
            if kept is not None:
                # the right operand is a node with several readers that already sits in a temporary: combine straight from it
                t, right, swapped = kept[0], self.depth_of[n.right.sig], 1                    # (the accumulator is the LEFT operand)
                kept[1] -= 1
            else:
                t, swapped = self._temp(), 0
                self.code.append(('Save', 0, t, 0, 0))
                right = self._emit(n.right.sig, below)
            if isinstance(n, fx.Mix):
                self.code.append(('Mix', 0, t, self._param(self._control(n.mix, below)), swapped))     # m L + (1 - m) R  (fx.py:40)
            else:
                self.code.append(('Mul', 0, t, 0, 0))
            if kept is None:
                self.temps_free.append(t)
            elif kept[1] == 0:
                self.temps_free.append(t)
                del self.saved[n.right.sig]
            depth = max(left, right)
        elif isinstance(n, fx.CritFilter):
            src = n.input.sig
            if src is None or not src.get_state().enabled:
                raise _NoProgram('filter without an input')                    # (the per-node schedule raises the reference's error)
            depth = self._emit(src, below + 1) + 1
            band = isinstance(n, fx.DoubleCritFilter)                          # ONE cached node: both slots at its level
            edges = (n.low, n.high) if band else (n.cutoff,)
            if len(self.filters) + len(edges) > _native.VP_MAX_FILTERS:
                raise _NoProgram('more filters than the machine has slots')
            if isinstance(n, ext.EqFilter):
                # a resonant slot of an equaliser type: q as below, the gain rows in a second parameter register the FilterEq word's b
                # names (-1: unplugged = 0 dB, and for the three classes without the port)
                self.filters.append((self._control(n.cutoff, below), str(n.type()), depth, n))
                q = -1 if _ctl_unplugged(n.resonance) else self._param(self._control(n.resonance, below))
                gp = n.gain_port()
                gain = -1 if gp is None or _ctl_unplugged(gp) else self._param(self._control(gp, below))
                self.code.append(('FilterEq', 0, len(self.filters) - 1, gain, q))
                self.resonant.append((n, q))
                self.gains.append((n, gain))
            elif isinstance(n, ext.ResonantFilter):
                # one slot like LowPass / HighPass, of a type of its own; q in a parameter register the FilterQ word names (read per
                # block with the cutoff, where the slot is designed), -1: unplugged = 1/sqrt2
                self.filters.append((self._control(n.cutoff, below), 'r' + str(n.type()), depth, n))
                q = -1 if _ctl_unplugged(n.resonance) else self._param(self._control(n.resonance, below))
                self.code.append(('FilterQ', 0, len(self.filters) - 1, 0, q))
                self.resonant.append((n, q))
            else:
                self.filters += [(self._control(p, below), str(n.type()), depth, n) for p in edges]
                self.code.append(('Band' if band else 'Filter', 0, len(self.filters) - len(edges), 0, 0))
            if band:
                self.bands.append(n)
        else:
            raise _NoProgram(f'no voice-program instruction for {n.cls_name()}')
        self.depth_of[n] = depth
        if self.uses.get(n, 1) > 1:                                            # several readers: computed once, kept in a temporary
            t = self._temp()
            self.code.append(('Save', 0, t, 0, 0))
            self.saved[n] = [t, self.uses[n] - 1]
        return depth

    # ---- control rows and the launch
    def _rows(self):
        """(per control: its row tensor, control_rows, history block starts, blocks rendered before) or None"""
        b, o = self.batch, self.batch.owner
        N, K, pos = b.N, b.K, b.pos
        small = self.depth > 0 and N < CONTEXT
        if small and (self.depth > 2 or N < 16):
            raise NotBatchable('short blocks: two filters in series at most, 16 frames at least')
        want = max(self.depth - 1, 0)
        if small:
            hist, front, lead = [], 0, K
        else:
            starts = o.history_starts(pos, want + 1)
            hist = starts[len(starts) - want:] if want else []
            front = starts[len(starts) - want - 1] if len(starts) > want else 0
            lead = len(hist) + 1
        control_rows = 2 * K if small else lead + K
        tensors: list = [None] * len(self.controls)
        groups: dict = {}
        for i, (port, const, below) in enumerate(self.controls):
            if const is not None:
                tensors[i] = const
            elif _ctl_const(port):
                tensors[i] = b._control_const(port, port.name)
            else:
                if small and below >= 2:
                    raise NotBatchable('short blocks: block-rate control in front of two filters in series')
                groups.setdefault(bool(small and below >= 1), []).append(i)
        for inner, members in groups.items():
            srcs = tuple(self.controls[i][0].sig for i in members)
            rows = o._control_program(('voice-program', tuple(id(x) for x in srcs), K, lead, small),
                                      lambda: _ProgramRows(srcs, K, lead, small, channels=self.voices, status=o._status_word))
            if not small:
                ahead = [front] + hist                                         # where the rows in front of the K blocks are read
                b._check_windowed(rows.main, ahead)
                rows.main.run(o, b.rate, pos, N, front_position=ahead[lead - 1])       # (the last of them in the same launch)
                for j, sub in enumerate(rows.front):
                    sub.run(o, b.rate, ahead[j], 0)
            else:
                rows.virtual.run(o, b.rate, pos - CONTEXT, N)
                if not inner:
                    rows.main.run(o, b.rate, pos, N)
                else:
                    # what feeds the last filter over block b was evaluated m_b = min((100 - N) / N, blocks before it - 1) blocks
                    # earlier (the oldest cached `after` reply containing the block), never before the stream's second block
                    mmax = (CONTEXT - N) // N
                    first = pos - o._stream_blocks * N
                    rows.main.run(o, b.rate, pos - mmax * N, N, min_position=first + N)
                    if o._stream_blocks == 0:
                        rows.first.run(o, b.rate, pos, 0)                      # ... the stream's very first block at its own position
            for i, t in zip(members, rows.tensors()):
                tensors[i] = as_control(t)
        return tensors, control_rows, hist, (o._stream_blocks if small else 0)

    def launch(self, out: torch.Tensor, bus_gains: torch.Tensor | None, bus: bool, label: str) -> torch.Tensor:
        b, o = self.batch, self.batch.owner
        tensors, control_rows, hist, before = self._rows()
        v = self.voices
        widths = [t.shape[1] for t in tensors]
        if any(w not in (1, v) for w in widths):
            raise _NoProgram('control rows of another width than the voices')
        for cut, _, _, _ in self.filters:
            if tensors[cut].shape[1] != v and v != 1:
                raise IndexError(f'index {tensors[cut].shape[1]} is out of bounds for axis 1 with size {tensors[cut].shape[1]}')   # fx.py:99
        for _, q in self.resonant + self.gains:
            if q >= 0 and tensors[self.params[q]].shape[1] != v and v != 1:
                width = tensors[self.params[q]].shape[1]
                raise IndexError(f'index {width} is out of bounds for axis 1 with size {width}')
        adsr = None
        if self.adsr is not None:
            adsr = b._envelope_rows(self.adsr)
            if any(r.shape[1] not in (1, v) for r in adsr.values()):
                raise _NoProgram('envelope rows of another width than the voices')
        oscs = [(tensors[h], tensors[p] if p is not None else None) for h, p in self.oscs]
        params = [tensors[i] for i in self.params]
        filters = [(tensors[c], t, level) for c, t, level, _ in self.filters]
        status = o._status_word(self.filters[0][3]) if self.filters else None
        if bus:
            o._bus_workspace(v, out.shape[0], out.shape[1])
        seeds = tuple(self.seeds + [0, 0])[:2]
        if self.depth:
            o._virtual_history.add(self.top)
        if o.specialise:
            from signals_amd import specialise
            C = out.shape[1] if bus else 0
            aligned = (4 if v % 4 == 0 and out.stride(0) % 4 == 0 and out.data_ptr() % 16 == 0 else
                       2 if v % 2 == 0 and out.stride(0) % 2 == 0 and out.data_ptr() % 8 == 0 else 1)
            # four voices per lane (one wave per SIMD) pay for programs without filter state or temporaries -- an oscillator bank
            # under a bus: 176 -> 144 us per 268 M voice-samples; with two filters 356 -> 396 us, with a temporary 380 -> 899 us.
            # The launch takes four only with such an image attached, so the choice is made here
            for four in ((True, False) if not filters and self.n_temps == 0 else (False,)):
                vpl, _ = _native.voice_program_geometry(v, b.N, b.K, CONTEXT, self.depth, C, aligned, specialised=four)
                make = specialise.ensure_in_background if o.specialise == 'background' else specialise.ensure
                if make(self.code, len(oscs), len(params), len(filters), self.n_temps, vpl, C):
                    label += '*specialised'
                    break
        return o._launch(label, lambda: _native.voice_program(self.code, oscs, params, filters, self.n_temps, self.depth, b.rate, b.pos,
                                                              b.N, b.K, CONTEXT, v, control_rows, hist, out, bus_gains=bus_gains, bus=bus,
                                                              adsr=adsr, noise_seeds=seeds, workspace=o._workspace if bus else None,
                                                              status=status, blocks_before=before,
                                                              tables=[n.resident_table() for n in self.tables],
                                                              unison=self.unison.host_copies() if self.unison is not None else None),
                         units=out.shape[0] * v)

    @classmethod
    def compile(cls, batch: '_Batch', top: Emitter, voices: int, min_nodes: int = 2, mixed: bool = False):
        """the program, or None when the graph is not one (or is a single kernel anyway: under a bus one node is enough, the
        bus being the second -- `min_nodes`); `mixed`: as for the constructor"""
        if top is None or not top.get_state().enabled:
            return None
        try:
            prog = cls(batch, top, voices, mixed=mixed)
        except _NoProgram:
            return None
        return prog if prog.kernel_nodes >= min_nodes else None

    def describe(self) -> str:
        return ','.join(op for op, *_ in self.code)

    def worthwhile(self) -> bool:
        """Does the interpreted launch beat one kernel per node?  Measured (tools/time_voice_program.py, 1024 voices): programs
        that fit the interpreter's SMALL register file -- two filter slots, three oscillators, four parameter registers, one
        temporary, no Amp / ADSR / White -- run at two waves per SIMD, 0.36-0.8 T voice-samples/s against 0.2-0.26 T per node;
        the full register file runs at one wave per SIMD and loses (0.14 T for three filters in series; f64 pow dominates an
        Amp either way).  Blocks shorter than the filter context have no per-node schedule at all (the alternative is the eager
        pull path, ~150 us per block).
        Band filters (two slots each): a swept one (an LFO on `low` / `high`) designs per block either way and takes the program
        under the same rule (tools/time_band.py); graphs whose bands all hold still keep the per-node schedule
        they had before the program knew band filters, unless that schedule cannot batch them (short blocks behind a filter).
        Phase-modulation carriers (OscPM) take the program under the same rule: a two-operator voice under a bus runs at 0.54-0.55 T
        interpreted against 0.22 T per node, 0.40-0.42 against 0.16-0.17 T behind a LowPass (tools/time_pm.py).
        Wavetable oscillators (OscTable) take the program under the same rule: 0.76 T interpreted against 0.32 T per node under a bus,
        0.55 against 0.21 T behind a LowPass (tools/time_wavetable.py).
        Waveshapers (Shape) likewise: 0.56 T interpreted against 0.22 T per node under a bus, 0.43 against 0.16 T with a LowPass in
        front of the shaper (tools/time_shaper.py).
        Resonant filters (FilterQ) take the program under the same rule; the q rows cost one parameter register each
        (tools/time_resonant.py).
        Equaliser biquads (FilterEq) keep FilterQ's rule, a gain costing one register more; their throughput is not measured yet
        (tools/time_eq.py).
        Unison oscillators (OscUni) take the program under the same rule: seven saws per voice under a bus run at 0.33 T interpreted
        against 0.28 T per node, 0.27 against 0.19 T behind a LowPass (tools/time_unison.py) -- a narrower
        margin than the other oscillators', since U copies of f64 work per sample bound both routes.
        Band-limited oscillators (OscBlep) keep OscUni's rule: one copy under a bus 0.46 T interpreted against 0.43 T per node, 0.35
        against 0.24 T behind a LowPass; seven copies 0.132 against 0.122 T behind a LowPass, but 0.155 against 0.156-0.158 T under a
        bare bus (three runs): there the rule costs 1-2 %, which is accepted (tools/time_blep.py).
        Hard-sync oscillators (OscSync) keep OscUni's rule too; their throughput is not measured yet (tools/time_sync.py, DESIGN.md
        section 7).
        Mixed programs (two or more of the families of _native.VP_FAMILIES; only compiled with `mixed_programs=True`) take the program
        under the same rule: measured (tools/time_mixed.py, 1024 voices, stereo bus, N = 256, three routes in alternation, median of 7
        windows of 0.5 s, attached kernels switched off for the interpreter) the interpreter's mixed variant runs UnisonSawtooth ->
        ResonantLowPass at 0.26 T against 0.19 T per node, Wavetable -> ResonantLowPass at 0.49 against 0.29 T, UnisonSawtooth ->
        ResonantLowPass -> Shaper at 0.21 against 0.14 T -- 1.4-1.7x on all three, the spread over the windows below 1 % -- so the
        small-file rule extends to them; the specialised kernels run at 0.39 / 0.82 / 0.30 T.  A mixed program that needs the full register file (an ADSR, three filters ...) stays per node
        interpreted, like any other, and takes the short-block and the specialised routes."""
        b = self.batch
        small_file = (len(self.filters) <= 2 and len(self.oscs) <= 3 and len(self.params) <= 4 and self.n_temps <= 1
                      and self.adsr is None and not self.seeds and not any(op == 'Amp' for op, *_ in self.code))
        if b.owner.specialise is True:                  # ('background': the interpreter renders meanwhile, so its policy decides)
            # a kernel built for this program has no interpreter to pay for: three filters in series 0.54 T against 0.26 per node,
            # an Amp behind a filter level with it (f64 pow either way)
            from signals_amd import specialise
            if specialise.hipcc() is not None:
                return True
        if self.bands and all(_ctl_const(n.low) and _ctl_const(n.high) for n in self.bands):
            return b.N <= CONTEXT and any(not _is_pure(n.input.sig, b._pure) for _, _, _, n in self.filters)
        return small_file or (self.depth > 0 and b.N < CONTEXT)
