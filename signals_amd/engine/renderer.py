"""`BatchRenderer`: what a stream keeps between batches, and the render call."""
from __future__ import annotations

import os
import typing

import torch

from signals_amd import _native, runtime
from signals_amd.chain import CTRL_DTYPE, Emitter, Receiver, graph_clock, port
from signals_amd.engine.batch import _Batch
from signals_amd.engine.graph import CONTEXT, SCAN_MAX_CHAINS, NotBatchable
from signals_amd.engine.timing import KernelTimer, _CapturedLaunches


class _EngineSink(Receiver):
    """stands in for the consumer in requests the engine issues itself (plugin nodes pulled block by block)"""
    input = port('input')
    HOST_ARRAYS = False

    @classmethod
    def flags(cls):
        from signals_amd import SignalFlags
        return SignalFlags(0)


class BatchRenderer:
    """Renders `node` (as seen through a request of `channels` channels at `rate`) in batches of consecutive
    blocks.  Keeps what a stream needs between batches: the last <=100 rows of every request-dependent
    node (tails), the device status words of its filters, and the replay closure of a one-launch plan."""

    def __init__(self, node: Emitter, channels: int, rate: int = 48000, timer: KernelTimer | None = None,
                 fuse: bool = True, fuse_bus: bool = True, graph_replay: bool = False, fuse_program: bool | None = None,
                 specialise: bool | str | None = None, pipeline: int = 1, mixed_programs: bool = False):
        """`fuse`: let Filter(Osc) [and a Gain on top] run as one kernel when the intermediate outputs have
        no other consumer (sig_fused_osc_biquad); `fuse_bus`: also fold a SumBus on top into that launch
        (sig_fused_voice_bus).  fuse=False = one kernel per node, bit-identical to the eager path.
        `fuse_program` (default: as `fuse`): graphs none of the fused kernels covers run as one interpreted launch per sink
        (sig_voice_program) instead of one kernel per node -- where the interpreter beats that schedule (programs that fit its
        small register file, and every block size below the filter context, which the per-node schedule cannot batch at all);
        'always': wherever the graph compiles.
        `specialise`: build the voice-program kernel once more for exactly this graph's program (signals_amd/specialise.py:
        hipcc, a few seconds at the first render, cached on disk) and launch that instead of the interpreter -- the same
        arithmetic as straight-line code, 1.6-2x its rate; without hipcc the interpreter keeps running.  'background': the build
        runs on a worker thread and the interpreter renders until the kernel is attached (a real-time sink never waits for
        the compiler).  Default: off, or the environment's SIG_SPECIALISE=1.
        `mixed_programs` (default off): let a voice program COMBINE the extension nodes -- two or more of band filters, phase-modulation
        carriers, wavetable oscillators / waveshapers, resonant filters and unison oscillators in one graph (UnisonSawtooth ->
        ResonantLowPass, Wavetable -> BandPass ...).  Off, such a graph runs one kernel per node on every route; on, it is one launch
        of the interpreter's mixed variant (sig_voice_program_mixed) or, with `specialise`, of the kernel built for it
        (_VoiceProgram.worthwhile has the policy).
        `pipeline` (2 or 3; default 1 = off): consecutive batches of a graph that is ONE fused launch without history (the C2
        voice graph) go to alternating HIP streams, each with its own workspace, so the tail of one launch overlaps the head of
        the next (a 256-block batch is a single round of waves: 24.4 -> ~18 us per batch).  The caller's stream waits for each
        batch, so the returned tensor is ordered like any other -- but it comes from a ring of 4 buffers per stream and is
        OVERWRITTEN by the (4 x pipeline)-th render after it: consume or copy it before (like `graph_replay`).
        `timer`: optional KernelTimer that brackets every launch with HIP events.
        `graph_replay`: in the latency regime, capture the launch sequence of a one-plan graph into a hipGraph
        and replay it per call; the returned tensor is then owned by the graph and OVERWRITTEN by the next
        render -- only for callers that consume each block before asking for the next (BlockDriver.pull)."""
        self.graph_replay = graph_replay and timer is None
        self._captured: _CapturedLaunches | None = None
        self.fuse = fuse
        self.fuse_bus = fuse and fuse_bus           # also fold a SumBus on top of the chain into the launch
        self.fuse_cascade = fuse and fuse_bus       # SumBus([RingMod(] Filter(Filter(Osc)) [, ADSR)]) in one launch (sig_fused_cascade_bus)
        self.node = node
        self.channels = channels
        self.rate = rate
        self.timer = timer
        self._tails: dict[Emitter, tuple[int, torch.Tensor]] = {}    # node -> (end position, last <=100 rows)
        self._stream_end: int | None = None
        self._ctl_programs: dict = {}                      # compiled block-rate control programs, by (port sources, K)
        self._tremolo_order = None                         # voice_chain._TremoloOrder: the cutoff order of a tremolo-only Sine voice
        self._prev_block_frames: int | None = None         # N of the previous render (where a fused cascade's history block starts)
        self._virtual_history: set = set()                 # bus nodes whose launch of THIS batch kept its filter history implicit (no tails)
        self._cascade_stream: set = set()                  # ... of the previous batch, when this one continues it
        self._tails_rebuilt = False                        # the previous block was re-rendered per node for this batch's tails
        self._recent_blocks: list[tuple[int, int]] = []    # (start, end) of the last few blocks of the contiguous stream rendered so far
        self._stream_blocks = 0                            # blocks of the CURRENT size rendered contiguously since the stream started
        # graphs no fused kernel covers: the per-voice graph as ONE interpreted launch (sig_voice_program) -- True: where that beats
        # one kernel per node (_VoiceProgram.worthwhile), 'always': wherever the graph compiles
        self.fuse_program = fuse if fuse_program is None else (fuse and fuse_program)
        self.specialise = bool(int(os.environ.get('SIG_SPECIALISE', '0'))) if specialise is None else specialise
        self.mixed_programs = bool(mixed_programs)          # voice programs may combine the extension families (sig_voice_program_mixed)
        self.pipeline = max(1, int(pipeline))
        self._pipe = None                                  # voice_chain._BusPipeline: streams, workspaces, pre-bound calls and output rings of the pipelined replay
        self._status: dict[Emitter, runtime.StatusWord] = {}
        self._workspace: torch.Tensor | None = None       # f64 scratch of the fused bus kernel, reused
        self._latency_ws = None                            # ((voices, N, C), zero-initialised scratch of sig_latency_voice_bus)
        self._steady_consts = None                         # voice_chain._SteadyConsts: closed-form constants kept across calls
        self._gain_products: dict = {}                     # (id, id) -> (gain row, gain row, their product): Gain on both sides of a filter
        self.latency_kernel = True                         # one-launch blocks for Sine chains in the latency regime
        self._replay = None                                # (graph version, N, K, launch(position)) of a one-launch plan
        self.scan_max_chains = SCAN_MAX_CHAINS             # latency regime threshold (tests set 0 to force the serial kernels)
        self.requestor = _EngineSink()                     # the `requestor` of requests the engine itself issues to plugin nodes

    # ------------------------------------------------------------------ public
    def render(self, position: int, block_frames: int, nblocks: int) -> torch.Tensor:
        """Rows = nblocks*block_frames frames from `position`; same values as nblocks sequential
        eager requests of `block_frames` frames."""
        if block_frames < 2:
            raise NotBatchable('block-rate (frames == 1) requests go through the eager path')
        if self._replay is not None:
            version, n, k, launch = self._replay
            if version == graph_clock.version and (n, k) == (block_frames, nblocks):
                # the whole graph is ONE fused launch with no history state: replay it at the new position
                # without re-walking the graph (latency mode: ~10 us of host work per block)
                self._stream_end = position + block_frames * nblocks
                return launch(position)
            self._replay = None
        continuing = self._stream_end == position and (bool(self._tails) or bool(self._virtual_history))
        if not continuing:
            self._tails.clear()
        if self._stream_end != position or self._prev_block_frames != block_frames:
            self._stream_blocks = 0                        # (what a block of another size left in the reference's caches is not modelled: a fresh stream)
        if self._stream_end != position:
            self._recent_blocks = []
        self._cascade_stream = self._virtual_history if continuing else set()    # buses the previous batch ran through the fused cascade
        self._virtual_history = set()                      # filled again by launches that keep their history implicit (fused cascade)
        self._tails_rebuilt = False
        batch = _Batch(self, position, block_frames, nblocks, continuing)
        out = batch.buffer(self.node, self.channels, 0)
        self._save_tails(batch, position + block_frames * nblocks)
        self._stream_end = position + block_frames * nblocks
        self._prev_block_frames = block_frames
        self._stream_blocks += nblocks
        if block_frames >= CONTEXT:
            first = max(0, nblocks - 4)
            self._recent_blocks = (self._recent_blocks + [(position + b * block_frames, position + (b + 1) * block_frames)
                                                          for b in range(first, nblocks)])[-4:]
        else:
            self._recent_blocks = []
        return out

    def history_starts(self, position: int, count: int) -> list[int]:
        """where the `count` blocks in front of `position` start, oldest first: the previous renders' blocks while the stream is
        contiguous, then -- a fresh graph -- the virtual blocks the reference's context requests create, [p - 100, p) answered
        as a block of its own (chain/__init__.py:149-153, :431-442), clipped at 0.  Fewer than `count` when position 0 is reached."""
        starts = []
        edge = position
        for start, end in reversed(self._recent_blocks):
            if end != edge or len(starts) == count:
                break
            starts.insert(0, start)
            edge = start
        while len(starts) < count and edge > 0:
            edge = max(edge - CONTEXT, 0)
            starts.insert(0, edge)
        return starts

    def _save_tails(self, batch: '_Batch', end: int, replace: bool = True) -> None:
        """keep the last min(100, rows) rows of every request-dependent node of a batch that ends at `end`"""
        for node, buf in batch.impure_outputs():
            if replace or node not in self._tails:
                self._tails[node] = (end, buf[buf.shape[0] - min(CONTEXT, buf.shape[0]):].clone())

    def _rebuild_tails(self, position: int) -> None:
        """The previous batch ran (part of) the graph through the fused cascade, which leaves no tails, and this one needs
        the per-node schedule for it (a block size the kernel does not take, a node that gained a reader, `fuse_cascade`
        switched off ...): render the previous block [position - prevN, position) per node, as its own block -- an inner
        filter then cold-starts min(100, .) rows in front of it, exactly where the reference cold-started the block it keeps
        cached (chain/__init__.py:431-442, fx.py:93-94) -- and keep the last 100 rows of every request-dependent node."""
        self._tails_rebuilt = True
        prev = self._prev_block_frames
        if not prev or position - prev < 0:
            return
        keep_fuse, keep_virtual, keep_replay = self.fuse_cascade, self._virtual_history, self._replay
        self.fuse_cascade = False
        try:
            sub = _Batch(self, position - prev, prev, 1, False)
            sub.buffer(self.node, self.channels, 0)
            self._save_tails(sub, position, replace=False)
        finally:
            self.fuse_cascade, self._virtual_history, self._replay = keep_fuse, keep_virtual, keep_replay

    def reset(self) -> None:
        self._tails.clear()
        self._virtual_history = set()
        self._recent_blocks = []
        self._stream_blocks = 0
        self._stream_end = None
        self._replay = None
        self._captured = None

    def _remember_replay(self, N: int, K: int, launch) -> None:
        self._replay = (graph_clock.version, N, K, launch)

    # ------------------------------------------------------------------ kernel launch helper
    def _launch(self, name: str, fn: typing.Callable, **meta):
        if self.timer is not None:
            return self.timer.launch(name, fn, **meta)
        return fn()

    def _control_program(self, key, build: typing.Callable):
        """the compiled control program kept under `key`, built again when the graph or a Fixed row behind it has changed"""
        held = self._ctl_programs.get(key)
        if held is None or held[0] != graph_clock.version or not held[1].current():
            if len(self._ctl_programs) > 16:
                self._ctl_programs.clear()
            held = self._ctl_programs[key] = (graph_clock.version, build())
        return held[1]

    def _bus_workspace(self, voices: int, rows: int, bus_channels: int) -> torch.Tensor:
        """the f64 scratch of the fused bus kernels, grown to what this launch needs"""
        need = _native.lib().sig_fused_voice_bus_workspace(voices, rows, bus_channels) // 8
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty(need, dtype=CTRL_DTYPE, device=runtime.device())
        return self._workspace

    def _status_word(self, node: Emitter) -> torch.Tensor:
        word = self._status.get(node)
        if word is None:
            word = self._status[node] = runtime.StatusWord(node.cls_name())
        return word.tensor
