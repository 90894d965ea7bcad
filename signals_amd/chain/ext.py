"""Build-defined nodes under the same plugin API.  The reference names a
voice sum (`shape.Flatten`) but it sums over frames and crashes; these nodes are what BASELINE's
configurations need and are pinned against `oracle/chain_ref.py` ("parity unpinned" by the
reference itself)."""
import abc
import enum
import typing

import attr
import numpy as np
import torch

from signals_amd import SignalFlags, _native, runtime
from signals_amd.chain import fx
from signals_amd.chain import (
    BadStateValue,
    BlockCachingEmitter,
    ImplicitChannels,
    PassThroughResult,
    Receiver,
    Request,
    ResidentCopy,
    as_control,
    broadcast_shape,
    port,
    result_dtype,
    state,
)


def _validate_gains(instance, attribute, new_value):
    if new_value is not None and not (isinstance(new_value, np.ndarray) and new_value.ndim == 2):
        raise BadStateValue(instance, attribute.name, new_value, 'must be None or a 2D array (bus_channels, voices)')


class SumBus(BlockCachingEmitter, Receiver):
    """Voice sum bus: `out[n, c] = sum_v gains[c, v] * input[n, v]`; with `gains=None` a mono sum
    `out[n, 0] = sum_v input[n, v]`.  float64 accumulation in a fixed order (sig_sum_bus)."""
    input: Receiver.BoundPort = port('input')

    @state
    class State(BlockCachingEmitter.State):
        gains: typing.Optional[np.ndarray] = attr.ib(default=None, validator=_validate_gains,
                                                     on_setattr=attr.setters.validate)

    def __init__(self):
        super().__init__()
        self._resident = ResidentCopy(np.float64)

    @classmethod
    def flags(cls) -> SignalFlags:
        return super().flags() | SignalFlags.EFFECT

    @property
    def channels(self) -> int:
        gains = self._state.gains
        return 1 if gains is None else int(gains.shape[0])

    def resident_gains(self) -> typing.Optional[torch.Tensor]:
        gains = self._state.gains
        return None if gains is None else self._resident.of(gains)

    def _eval(self, request: Request) -> torch.Tensor:
        voices = self.input.channels
        x = self.input.request(request.loc.reslice(voices))
        out = torch.empty((x.shape[0], self.channels), dtype=result_dtype(x.shape[0]), device=x.device)
        return _native.sum_bus(x, self.resident_gains(), out)


class ADSR(BlockCachingEmitter, ImplicitChannels):
    """Position-pure piecewise-linear envelope per voice at frame rate; multiply it into a signal with
    `RingMod` (frame-rate product; `Gain.right` is block-rate, fx.py:52).  Ports (all block-rate, seconds
    except `sustain`, a level): attack, decay, sustain, release, gate_on, gate_off.  Definition:
    oracle/chain_ref.py:adsr; kernel: sig_adsr.

    At block rate: plugged into a control port (a filter envelope, `cutoff = Mix(Fixed(peak), Fixed(base), mix=ADSR)`; a pitch
    envelope on `hertz`; `resonance`, `ratio`, `spread`, `index`, `select`) it answers the one-frame request at the block's
    position in float64, the level at t = position / rate.  The batched engine evaluates that as one instruction of the block-rate
    control program (SIG_CTL_ADSR, the same operations, the same bits); its own six ports may then be driven by anything that
    program covers, an LFO on `release` for instance, and under a control-path LowPass / HighPass (a slewed envelope) they must
    be Fixed.  One instance may feed a `RingMod` at frame rate and a control port at once -- one envelope for amplitude and
    cutoff.  The engine computes the two reads separately; this eager path may serve the one-frame read from a cached float32
    block of the frame-rate read that contains it, a relative difference of 2^-24."""
    attack: Receiver.BoundPort = port('attack')
    decay: Receiver.BoundPort = port('decay')
    sustain: Receiver.BoundPort = port('sustain')
    release: Receiver.BoundPort = port('release')
    gate_on: Receiver.BoundPort = port('gate_on')
    gate_off: Receiver.BoundPort = port('gate_off')

    @classmethod
    def flags(cls) -> SignalFlags:
        return super().flags() | SignalFlags.GENERATOR | SignalFlags.EPOCH

    def control_rows(self, fetch) -> dict:
        return {name: as_control(fetch(getattr(self, name))) for name in _native.ADSR_PARAMS}

    def _eval(self, request: Request) -> torch.Tensor:
        rows = self.control_rows(lambda bound: bound.forward_at_block_rate(request))
        frames, voices = broadcast_shape((request.loc.shape.frames, 1), *(r.shape for r in rows.values()))
        out = torch.empty((frames, voices), dtype=result_dtype(frames), device=runtime.device())
        return _native.adsr(request.loc.position, request.loc.rate, rows, out)


class PMOsc(BlockCachingEmitter, ImplicitChannels, abc.ABC):
    """Phase-modulation (FM) oscillator: an oscillator of chain/osc.py whose phase is offset by a frame-rate signal,
    `t = (frame_range / rate * hertz + phase) + index * mod`, `out = wave(t)` in float64 like `osc.Osc` (kernel: sig_osc_bank_pm).
    Ports: hertz, phase, index at block rate; `mod` at frame rate, in cycles per unit of `index` (a full-scale sine modulator
    with index I is the textbook modulation index 2 pi I).  Position-pure when `mod` is: no carried phase.  With `mod` or `index`
    unplugged it is the plain oscillator.  Not an `osc.Osc`: that means a leaf with two control ports to the engine."""
    hertz: Receiver.BoundPort = port('hertz')
    phase: Receiver.BoundPort = port('phase')
    index: Receiver.BoundPort = port('index')
    mod: Receiver.BoundPort = port('mod')

    @classmethod
    def flags(cls) -> SignalFlags:
        return super().flags() | SignalFlags.GENERATOR

    @classmethod
    @abc.abstractmethod
    def kind(cls) -> str:
        """kernel selector: 'Sine' | 'Square' | 'Sawtooth' | 'Triangle'"""
        raise NotImplementedError

    def _eval(self, request: Request) -> torch.Tensor:
        phase = as_control(self.phase.forward_at_block_rate(request))
        hertz = as_control(self.hertz.forward_at_block_rate(request))
        index = as_control(self.index.forward_at_block_rate(request))
        mod = self.mod.forward(request)
        if mod.dtype not in (torch.float32, torch.float64) or (mod.shape[1] > 1 and mod.stride(1) != 1):
            mod = mod.to(result_dtype(mod.shape[0])).contiguous()
        loc = request.loc
        frames, voices = broadcast_shape((loc.shape.frames, 1), hertz.shape, phase.shape, index.shape, mod.shape)
        out = torch.empty((frames, voices), dtype=result_dtype(frames), device=hertz.device)
        return _native.osc_bank_pm(self.kind(), loc.position, loc.rate, hertz, phase, index, mod, out)


class PMSine(PMOsc):

    @classmethod
    def kind(cls) -> str:
        return 'Sine'


class PMSquare(PMOsc):

    @classmethod
    def kind(cls) -> str:
        return 'Square'


class PMSawtooth(PMOsc):

    @classmethod
    def kind(cls) -> str:
        return 'Sawtooth'


class PMTriangle(PMOsc):

    @classmethod
    def kind(cls) -> str:
        return 'Triangle'


class BankEmitter(BlockCachingEmitter, ImplicitChannels, abc.ABC):
    """A generator that is a pure function of the absolute frame and whose only inputs are block-rate rows: it states its launch
    once (`bank`), for this eager path and for the batched engine's schedule (engine/batch.py: `_sched_bank`)."""

    @classmethod
    def flags(cls) -> SignalFlags:
        return super().flags() | SignalFlags.GENERATOR

    @abc.abstractmethod
    def bank(self, fetch, channels: int) -> tuple:
        """(label, kind, rows, call): the launch is named `label[kind]`; `rows` are the control rows, each port's block-rate reply
        through `fetch`, read with a request `channels` wide; `call(position, rate, *rows, out, **kw)` is the `_native` entry with
        what else it takes -- a table, the copies, the loop bounds -- bound in as the node's state holds it now"""
        raise NotImplementedError

    def _eval(self, request: Request) -> torch.Tensor:
        loc = request.loc
        _, _, rows, call = self.bank(lambda bound: bound.forward_at_block_rate(request), loc.shape.channels)
        frames, voices = broadcast_shape((loc.shape.frames, 1), *(r.shape for r in rows))
        out = torch.empty((frames, voices), dtype=result_dtype(frames), device=rows[0].device)
        return call(loc.position, loc.rate, *rows, out)


def _bound(entry, *payload, head=()):
    """`call` of a `bank`: the entry with `head` in front of the position and `payload` between the rows and `out`"""
    return lambda position, rate, *rows_and_out, **kw: entry(*head, position, rate, *rows_and_out[:-1], *payload, rows_and_out[-1], **kw)


def _request_rows(fetch, ports, channels: int) -> list:
    """the block-rate replies of `ports` as contiguous float64 rows at most `channels` wide; a reply narrower than that but wider
    than 1 is the IndexError of a narrow `cutoff` (Sampler, Modal)"""
    rows = []
    for bound in ports:
        row = as_control(fetch(bound))
        if 1 < row.shape[1] < channels:
            raise IndexError(f'index {row.shape[1]} is out of bounds for axis 1 with size {row.shape[1]}')
        row = row[:, :channels]
        rows.append(row if row.is_contiguous() else row.contiguous())
    return rows


def _validate_table(instance, attribute, new_value):
    ok = (isinstance(new_value, np.ndarray) and new_value.ndim == 2 and new_value.dtype.kind in 'fiu'
          and new_value.shape[0] >= 2 and new_value.shape[0] & (new_value.shape[0] - 1) == 0 and new_value.shape[1] >= 1
          and new_value.shape[0] * new_value.shape[1] <= _native.TABLE_MAX_POINTS)
    if not ok:
        raise BadStateValue(instance, attribute.name, new_value,
                            f'must be a 2D real array (points, waves), points a power of two >= 2, points * waves <= '
                            f'{_native.TABLE_MAX_POINTS}')


class Wavetable(BankEmitter):
    """Wavetable oscillator: the state `table` holds W single-cycle waveforms of T points each as a (T, W) array (the
    reference's (frames, channels) orientation), read with linear interpolation at the oscillator phase of chain/osc.py.
    With tbl = float32(table) widened to float64, in float64 and every operation rounded:
        t = frame_range / rate * hertz + phase;  m = np.mod(t, 1.0);  u = m * T;  i = floor(u);  f = u - i
        w = clip(floor(select), 0, W - 1)                                  (per voice; NaN and unplugged: column 0)
        out = tbl[i & (T-1), w] + f * (tbl[(i+1) & (T-1), w] - tbl[i & (T-1), w])
    (kernel: sig_osc_bank_table; restated in numpy by tests/wavetable_reference.py).  Ports, all block-rate: hertz, phase,
    select.  T is a power of two >= 2, T * W <= 16384; integer arrays (what a .sigs value arrives as) are converted; the device
    copy is float32 and follows in-place edits of the array.  Position-pure: no carried phase.  Not an `osc.Osc`: that means a
    closed-form leaf with two control ports to the engine's fused kernels.
    Out of scope: the node inside a block-rate control path (the batched engine answers NotBatchable with the reason and the
    graph keeps the eager path, which serves frames == 1 in float64); a phase-modulated wavetable; morphing between columns
    (`fx.Mix` of two Wavetables does that); per-voice private tables; the closed-form and row-walker fused kernels, which keep
    matching `osc.Osc` only."""
    hertz: Receiver.BoundPort = port('hertz')
    phase: Receiver.BoundPort = port('phase')
    select: Receiver.BoundPort = port('select')

    @state
    class State(BlockCachingEmitter.State):
        table: np.ndarray = attr.ib(factory=lambda: np.array([[0.0], [1.0], [0.0], [-1.0]]), validator=_validate_table,
                                    on_setattr=attr.setters.validate)

    def __init__(self):
        super().__init__()
        self._resident = ResidentCopy(np.float32)

    def resident_table(self) -> torch.Tensor:
        return self._resident.of(self._state.table)

    def _entry(self, table: torch.Tensor) -> tuple:
        """(label, kind, the `_native` entry) of the launch that reads `table`"""
        return 'osc_bank_table', 'Table', _native.osc_bank_table

    def bank(self, fetch, channels: int) -> tuple:
        rows = [as_control(fetch(bound)) for bound in (self.hertz, self.phase, self.select)]   # (select unplugged: zeros((1, 1)) = column 0)
        table = self.resident_table()
        label, kind, entry = self._entry(table)
        return label, kind, rows, _bound(entry, table)


def _validate_spectra(instance, attribute, new_value):
    ok = (isinstance(new_value, np.ndarray) and new_value.ndim == 2 and new_value.dtype.kind in 'fiu'
          and 1 <= new_value.shape[0] <= _native.ADDITIVE_MAX_PARTIALS and new_value.shape[1] >= 1
          and new_value.shape[0] * new_value.shape[1] <= _native.TABLE_MAX_POINTS
          and bool(np.isfinite(new_value).all()))
    if not ok:
        raise BadStateValue(instance, attribute.name, new_value,
                            f'must be a finite 2D real array (partials, waves), 1 <= partials <= {_native.ADDITIVE_MAX_PARTIALS}, '
                            f'partials * waves <= {_native.TABLE_MAX_POINTS}')


def _harmonics(H: int) -> np.ndarray:
    """1 .. H as float64, H checked against the node's limit"""
    if isinstance(H, bool) or not isinstance(H, (int, np.integer)) or not 1 <= H <= _native.ADDITIVE_MAX_PARTIALS:
        raise ValueError(f'partials must be an integer 1 .. {_native.ADDITIVE_MAX_PARTIALS}, got {H!r}')
    return np.arange(1, int(H) + 1, dtype=np.float64)


class Additive(Wavetable):
    """Band-limited additive oscillator: up to 64 harmonics per voice with amplitudes from a table, the partials above half the rate
    dropped per voice and block -- organ drawbars, formant and vocal spectra, and saws, squares and triangles that stay clean up to
    Nyquist under a pitch envelope, which neither `Wavetable` (it aliases as the pitch rises; mip columns cannot follow a sweep) nor
    `BlepOsc` (three fixed shapes) does.  `Wavetable` -- the same three block-rate ports hertz, phase and select, the same `table` state
    name and resident float32 device copy, the same phase t bit for bit -- with the table read as a spectrum: an (H, W) array, row
    h - 1 the amplitude of harmonic h for each of W spectra, 1 <= H <= 64, W >= 1, H * W <= 16384, no power-of-two rule, every value
    finite, negative amplitudes allowed (a triangle needs them); integer arrays convert as they do for `Wavetable`.  The default
    [[1.0]] is a sine.  With `select` it switches timbres, through `fx.Mix` of two nodes it cross-fades them.  With a = float32(table)
    widened to float64, for row n and voice v, in float64 and every operation rounded:
        t  = frame_range / rate * hertz + phase                            (osc.py's order)
        m  = np.mod(t, 1.0)
        w  = clip(floor(select), 0, W - 1)                                 (NaN and unplugged: column 0, as Wavetable)
        nf = (0.5 * rate) / abs(hertz)                                     (IEEE divide; 0 Hz gives inf)
        k  = clip(ceil(nf) - 1, 0, H)                                      (the partials h with h |hertz| < rate / 2; inf gives H)
        g  = min(1.0, nf - k)                                              (the weight of the top kept partial only)
        out = sum over h = 1 .. k of c_h * sin(2 pi h m),   c_h = a[h-1, w] * (g if h == k else 1)
    (kernel: sig_osc_bank_additive; restated in numpy by tests/additive_reference.py).  k and g are per voice and per block, since
    `hertz` is block-rate.  g makes the output continuous in `hertz`: a partial fades linearly to nothing over the last harmonic
    spacing before it reaches Nyquist, so a pitch sweep does not click when a partial drops out; only one partial per voice and block
    is ever scaled.  k = 0 (|hertz| >= rate / 2, +-inf too) gives exactly 0.0 whatever the phase; a NaN `hertz` gives NaN; with
    k >= 1 a non-finite `phase` (or t) gives NaN.  hertz < 0 uses |hertz| for k and g, and its sign enters through t.  There is no
    normalisation: the peak is bounded by the column's sum of |a|.
    Because of the sine the kernel is held to a bound, not to bits: every sample, float32 rows and the float64 of a one-frame request
    alike, within 1e-6 * max(1, A) of the definition with the partial sum in extended precision, A the largest column sum of |a|.
    The kernel takes one sine / cosine pair of 2 pi m per sample and turns it h times by a plane rotation, whose error grows linearly
    in h at every pitch.  Measured on an MI355X over the kernel cases of tests/test_gpu_additive.py: 1.8e-15 at most in front of the float64 store (A up to 2.6, H up
    to 64, the 0.01 Hz voice 7e-16), 5.9e-8 behind the float32 store, which is that store's own rounding of a sample above 1/2: 17 times
    inside the bar.
    Position-pure: no carried phase, no history.  The batched engine renders the node with one kernel per batch; it has no
    voice-program word, so a graph that contains one runs one kernel per node (the nodes around it keep their routes, as with
    `Ladder`), `mixed_programs` and `specialise` or not.
    Spectra (static, numpy on the host, one float64 column each): `Additive.sawtooth(H)`, `Additive.square(H)`,
    `Additive.triangle(H)` converge to `osc.Sawtooth`, `osc.Square`, `osc.Triangle` at the same phase as H grows;
    `Additive.cycle(column, T)` renders a column to a T-point single cycle for a `Wavetable`.
    Out of scope: cosine (phase) terms per partial (a second table and a second accumulation: the spectra here are odd functions of
    the phase); inharmonic partial ratios (the node is a pure function of the wrapped phase m, and sin(2 pi r m) is one only for an
    integer r); a frame-rate `hertz` or `select` (k, g and the column are hoisted per block); per-voice private tables (one table per
    launch sits in LDS); a voice-program word and the closed-form, row-walker and cascade fused kernels (they keep matching `osc.Osc`
    only); the node inside a block-rate control path (the batched engine answers NotBatchable with the reason and the graph keeps
    the eager path, which serves frames == 1 in float64); more than 64 partials (the table's rows, and the recurrence's error bound,
    are sized for 64)."""

    @state
    class State(Wavetable.State):
        table: np.ndarray = attr.ib(factory=lambda: np.array([[1.0]]), validator=_validate_spectra, on_setattr=attr.setters.validate)

    # ---- spectra: numpy on the host, one (H, 1) float64 column each
    @staticmethod
    def sawtooth(H: int = 64) -> np.ndarray:
        """the first H harmonics of osc.Sawtooth, 2 mod(t - 1/2, 1) - 1 = sum 2 / (pi h) (-1)^(h+1) sin(2 pi h t)"""
        h = _harmonics(H)
        return (2.0 / (np.pi * h) * np.where(h % 2 == 1, 1.0, -1.0)).reshape(-1, 1)

    @staticmethod
    def square(H: int = 64) -> np.ndarray:
        """the first H harmonics of osc.Square, sign(1/2 - mod(t, 1)) = sum over odd h of 4 / (pi h) sin(2 pi h t)"""
        h = _harmonics(H)
        return np.where(h % 2 == 1, 4.0 / (np.pi * h), 0.0).reshape(-1, 1)

    @staticmethod
    def triangle(H: int = 64) -> np.ndarray:
        """the first H harmonics of osc.Triangle (peak +1 at t = 1/4): sum over odd h of 8 / (pi h)^2 (-1)^((h-1)/2) sin(2 pi h t)"""
        h = _harmonics(H)
        return np.where(h % 2 == 1, 8.0 / (np.pi * h) ** 2 * np.where(h % 4 == 1, 1.0, -1.0), 0.0).reshape(-1, 1)

    @staticmethod
    def cycle(column, T: int = 2048) -> np.ndarray:
        """one column of amplitudes as a (T, 1) single cycle, sum_h a_h sin(2 pi h i / T) for i = 0 .. T - 1 with every partial
        at full weight: what a `Wavetable` of T points plays where it does not alias (T > 2 H keeps the partials apart)"""
        a = np.asarray(column, dtype=np.float64).reshape(-1)
        if isinstance(T, bool) or not isinstance(T, (int, np.integer)) or T < 2:
            raise ValueError(f'a cycle has an integer number of points >= 2, got {T!r}')
        i = np.arange(int(T), dtype=np.float64)
        h = np.arange(1, a.shape[0] + 1, dtype=np.float64)
        angle = np.mod(np.outer(i, h), float(T)) / float(T)                    # exact: i * h < 2**53
        return (np.sin(2.0 * np.pi * angle) @ a).reshape(-1, 1)

    def _entry(self, table: torch.Tensor) -> tuple:
        return 'osc_bank_additive', f'Additive{table.shape[0]}', _native.osc_bank_additive


UNISON_DETUNE = (-0.11002313, -0.06288439, -0.01952356, 0.0, 0.01991221, 0.06216538, 0.10745242)


def _default_copies() -> np.ndarray:
    """seven copies at the uneven JP-8000 spacing (they never realign periodically), phase offsets a golden-ratio apart"""
    return np.stack([np.array(UNISON_DETUNE), np.mod(np.arange(7) * 0.6180339887498949, 1.0)], axis=1)


def _validate_copies(instance, attribute, new_value):
    ok = (isinstance(new_value, np.ndarray) and new_value.ndim == 2 and new_value.dtype.kind in 'fiu'
          and new_value.shape[1] == 2 and 1 <= new_value.shape[0] <= _native.UNISON_MAX_COPIES
          and bool(np.isfinite(new_value).all()))
    if not ok:
        raise BadStateValue(instance, attribute.name, new_value,
                            f'must be a 2D real array (copies, 2) of finite (detune, phase offset) rows, 1 <= copies <= '
                            f'{_native.UNISON_MAX_COPIES}')


class UnisonOsc(BankEmitter, abc.ABC):
    """Unison oscillator: U detuned copies of one waveform of chain/osc.py per voice, summed and divided by U -- the supersaw, detuned
    square leads, thickened sines.  The state `copies` is a (U, 2) array, 1 <= U <= 16: column 0 the relative detune d[u] of copy u,
    column 1 its phase offset p[u] in cycles.  Ports, all block-rate: hertz, phase, spread (dimensionless; unplugged means zeros,
    like every port: every copy then runs at `hertz`).  For row n and voice v, in float64 and every operation rounded:
        r_u = 1.0 + spread[v] * d[u]
        h_u = hertz[v] * r_u
        q_u = phase[v] + p[u]
        t_u = frame_range / rate * h_u + q_u                               (osc.py's order: frame / rate, times h_u, plus q_u)
        s   = ((w(t_0) + w(t_1)) + w(t_2)) + ...                           (u ascending, w = osc.py's waveform of the kind)
        out = s / U
    (kernel: sig_osc_bank_unison; restated in numpy by tests/unison_reference.py).  With copies = [[0, 0]] this is `osc.Osc` bit for
    bit.  The default is seven copies at the uneven JP-8000 spacing with golden-ratio phase offsets.  Integer arrays (what a .sigs
    value arrives as) are converted; the copies travel by value with each launch, so an in-place edit of the array or a replaced
    array takes effect at the next render.  Position-pure: no carried phase, no table.  Not an `osc.Osc`: that means a closed-form
    leaf with two control ports to the engine's fused kernels.
    Out of scope: a frame-rate `spread`; per-voice private `copies`; stereo spread of the copies (`SumBus` gains pan whole voices);
    a phase-modulated or wavetable unison; the node inside a block-rate control path (the batched engine answers NotBatchable with
    the reason and the graph keeps the eager path, which serves frames == 1 in float64); a combination with a band filter, a
    phase-modulation oscillator, a wavetable oscillator, a waveshaper or a resonant filter in one voice program (such a graph stays
    one kernel per node unless the renderer is given mixed_programs=True); the closed-form, row-walker and cascade fused kernels; band-limiting -- the copies alias like
    `osc.Sawtooth` does (`BlepOsc` below is the band-limited one)."""
    hertz: Receiver.BoundPort = port('hertz')
    phase: Receiver.BoundPort = port('phase')
    spread: Receiver.BoundPort = port('spread')

    @state
    class State(BlockCachingEmitter.State):
        copies: np.ndarray = attr.ib(factory=_default_copies, validator=_validate_copies, on_setattr=attr.setters.validate)

    @classmethod
    @abc.abstractmethod
    def kind(cls) -> str:
        """kernel selector: 'Sine' | 'Square' | 'Sawtooth' | 'Triangle'"""
        raise NotImplementedError

    @classmethod
    def bandlimited(cls) -> bool:
        """False: osc.py's naive waveform per copy (sig_osc_bank_unison, the OscUni word); True: BlepOsc's corrected one
        (sig_osc_bank_blep, the OscBlep word).  Everything else about the node is the same to the engine"""
        return False

    def host_copies(self) -> np.ndarray:
        """the (U, 2) float64 array a launch takes by value, as the state holds it now"""
        return np.ascontiguousarray(self._state.copies, dtype=np.float64)

    def _entry(self) -> tuple:
        """(the name of the `_native` entry, which is the launch's label too; the ports whose rows it takes, in its order)"""
        return 'osc_bank_blep' if self.bandlimited() else 'osc_bank_unison', (self.hertz, self.phase, self.spread)

    def bank(self, fetch, channels: int) -> tuple:
        label, ports = self._entry()
        rows = [as_control(fetch(bound)) for bound in ports]                   # (unplugged: zeros((1, 1)) -- every copy at `hertz`, R = 1)
        kind = self.kind()
        return label, kind, rows, _bound(getattr(_native, label), self.host_copies(), head=(kind,))


class UnisonSine(UnisonOsc):

    @classmethod
    def kind(cls) -> str:
        return 'Sine'


class UnisonSquare(UnisonOsc):

    @classmethod
    def kind(cls) -> str:
        return 'Square'


class UnisonSawtooth(UnisonOsc):

    @classmethod
    def kind(cls) -> str:
        return 'Sawtooth'


class UnisonTriangle(UnisonOsc):

    @classmethod
    def kind(cls) -> str:
        return 'Triangle'


def _single_copy() -> np.ndarray:
    """one copy, no detune, no offset: one clean oscillator"""
    return np.zeros((1, 2))


class BlepOsc(UnisonOsc, abc.ABC):
    """Band-limited square, sawtooth and triangle: `UnisonOsc` -- the same ports hertz, phase and spread, all block-rate, the same
    `copies` state and validator, the same phase t_u per copy bit for bit -- with each copy's waveform corrected by a two-sample
    polynomial band-limited step (PolyBLEP) around its edges, so that the partials above half the rate fold back some 15 dB weaker
    than osc.py's closed forms let them.  The default is copies = [[0, 0]]: one clean oscillator; the JP-8000 array
    (`ext.UNISON_DETUNE`, `UnisonOsc`'s default) gives the anti-aliased supersaw.  There is no Sine: it has no edge.
    For copy u, row n and voice v, in float64 and every operation rounded:
        r_u, h_u, q_u, t_u as UnisonOsc
        d = min(|h_u| / rate, 0.5)                                   (the phase increment per sample; per copy, voice and block)
        step(m)   = 2x - x*x - 1      with x = m / d            if m < d
                  = y*y + 2y + 1      with y = (m - 1) / d      if m > 1 - d
                  = 0                                            otherwise
        corner(m) = (1 - m/d)^3                                  if m < d
                  = ((m - 1)/d + 1)^3                            if m > 1 - d
                  = 0                                            otherwise
        Sawtooth: m = mod(t - 0.5, 1);  w = (2m - 1) - step(m)
        Square:   m = mod(t, 1);        w = (m < 0.5 ? 1 : -1) + step(m) - step(mod(t + 0.5, 1))
        Triangle: m = mod(t - 0.25, 1); w = tri(t - 0.25) + (4/3) d (corner(mod(t + 0.25, 1)) - corner(m))
                  tri(u) = (4 mod(u, 0.5) - 1) * (m < 0.5 ? -1 : 1)       (= 4|m - 0.5| - 1, in osc.py's own order)
        out = (sum over u ascending of w_u) / U
    (kernel: sig_osc_bank_blep, which multiplies by a rounded 1 / d where this divides: within 1e-14; restated in numpy by
    tests/blep_reference.py).  Continuous in t for every kind and every d > 0, so a phase one ulp off moves the sample by
    (2 + 2/d) ulp at most, where the naive edge jumps by 2.  A non-finite t gives NaN.  The naive parts of Square and Triangle drop
    np.sign's isolated zero at the edge (with it the corrected wave would spike at exactly m = 1/2); the Triangle's is written in
    osc.py's order, because 4|m - 0.5| - 1 rounds m - 0.5 below m = 1/4: outside the windows every kind is `osc.Osc` bit for bit.  d = 0 (0 Hz) selects no window:
    the naive value.  hertz < 0 uses |h|: the residual is symmetric under time reversal.  Above rate / 4 the Square's two windows
    overlap, and above rate / 2 d is clamped: the formula is still the definition, but it no longer band-limits there.  The
    correction is a pure function of t and d: position-pure like its parent, no carried state, no table.
    Out of scope: what UnisonOsc leaves out; a band-limited phase-modulation or wavetable oscillator; `osc.*` itself and the
    closed-form, row-walker and cascade fused kernels, which keep the naive forms; a 4-point BLEP; oversampling."""

    @state
    class State(UnisonOsc.State):
        copies: np.ndarray = attr.ib(factory=_single_copy, validator=_validate_copies, on_setattr=attr.setters.validate)

    @classmethod
    def bandlimited(cls) -> bool:
        return True


class BlepSquare(BlepOsc):

    @classmethod
    def kind(cls) -> str:
        return 'Square'


class BlepSawtooth(BlepOsc):

    @classmethod
    def kind(cls) -> str:
        return 'Sawtooth'


class BlepTriangle(BlepOsc):

    @classmethod
    def kind(cls) -> str:
        return 'Triangle'


class SyncOsc(BlepOsc, abc.ABC):
    """Oscillator hard sync, band-limited: a slave sawtooth or square running at `ratio` times the pitch is reset at every cycle of a
    master at `hertz` -- the sync lead, and with a swept ratio the formant-like "tearing" sweep.  `BlepOsc` -- the same ports hertz,
    phase and spread, the same `copies` state, validator and default of one copy, the same master phase t_u per copy bit for bit --
    with one more block-rate port, `ratio` (dimensionless).  Unplugged means zeros, like every port, and a ratio <= 1 means 1: the
    node is then an ordinary band-limited oscillator (the Sawtooth `BlepSawtooth` at phase + 0.5, the Square `BlepSquare`).  There is
    no Sine or Triangle: their reset also changes the slope.  The slave's value is a pure function of the master's phase:
    position-pure, no carried phase, no table.  For copy u, row n and voice v, in float64 and every operation rounded:
        r_u, h_u, q_u, t_u, d and step(m) (at d) as BlepOsc
        R  = max(ratio[v], 1.0)                                          (a ratio that is not finite: NaN rows for that voice)
        m  = mod(t, 1);  s = m * R;  k = floor(s);  f = s - k            (the slave's phase f in its k-th cycle since the reset)
        ds = min(d * R, 0.5)                                             (the slave's increment per sample)
        g  = R - (ceil(R) - 1)                                           (the length of the last, cut slave cycle, in (0, 1])
        estep(p, lo_ok, hi_ok) = 2x - x*x - 1    with x = p / ds         if p < ds      and lo_ok
                               = y*y + 2y + 1    with y = (p - 1) / ds   if p > 1 - ds  and hi_ok
                               = 0                                       otherwise
        Sawtooth: w = (2f - 1) - estep(f, k >= 1, k + 1 < R) - g * step(m)
        Square:   sb = s + 0.5;  kb = floor(sb);  fb = sb - kb
                  w  = (f < 0.5 ? 1 : -1) + estep(f, k >= 1, k + 1 < R) - estep(fb, kb >= 1, kb + 0.5 < R) + (g <= 0.5 ? 0 : 1) * step(m)
        out = (sum over u ascending of w_u) / U
    (kernel: sig_osc_bank_sync, which multiplies by a rounded 1 / d and 1 / ds where this divides: within 1e-14; restated in numpy
    by tests/sync_reference.py).  The slave's edges strictly inside the master's cycle take the residual at the slave's rate; the
    reset at m = 0 -- of height 2 g for the Sawtooth, 0 or 2 for the Square -- takes the one at the master's.  Every choice is a
    select: d = 0 (0 Hz) selects no window, a non-finite t gives NaN, hertz < 0 uses |h|.
    The definition is continuous in t everywhere but for one case: where the last interior edge lies closer to the reset than one
    window -- the Sawtooth: g < ds; the Square: the distance g mod 0.5 < ds where it is not 0 -- that edge's trailing window is cut at
    the reset, and the sample jumps there by what the window had left.  The formula is the definition there too.  Above ds = 0.5
    (ratio * hertz above rate / 2) ds is clamped and the formula no longer band-limits (at 1734 Hz and ratio 13.9 the fold-back is
    +12 dB over the harmonics).  Well below that the slave's own partials already fold: at ratio 5 and 1734 Hz, where the naive
    wave's fold-back is at -5 dB of the harmonics' power, the correction leaves -18 dB (-24 .. -28 dB at ratios 1.5 .. 3.3).
    Out of scope: what BlepOsc leaves out; a frame-rate ratio; soft sync and reversing sync; a synced Sine or Triangle; a combination
    with an equaliser biquad (`EqFilter`) in one voice program (such a graph stays one kernel per node)."""
    ratio: Receiver.BoundPort = port('ratio')

    def _entry(self) -> tuple:
        return 'osc_bank_sync', (self.hertz, self.phase, self.spread, self.ratio)


class SyncSawtooth(SyncOsc):

    @classmethod
    def kind(cls) -> str:
        return 'Sawtooth'


class SyncSquare(SyncOsc):

    @classmethod
    def kind(cls) -> str:
        return 'Square'


def _validate_curves(instance, attribute, new_value):
    ok = (isinstance(new_value, np.ndarray) and new_value.ndim == 2 and new_value.dtype.kind in 'fiu'
          and new_value.shape[0] >= 2 and new_value.shape[1] >= 1
          and new_value.shape[0] * new_value.shape[1] <= _native.TABLE_MAX_POINTS)
    if not ok:
        raise BadStateValue(instance, attribute.name, new_value,
                            f'must be a 2D real array (points, curves), points >= 2, points * curves <= {_native.TABLE_MAX_POINTS}')


class Shaper(BlockCachingEmitter, ImplicitChannels):
    """Table-lookup waveshaper, a memoryless non-linearity (saturation, overdrive, wavefolding, Chebyshev shaping, soft clipping):
    the state `table` holds W transfer curves of T points each as a (T, W) array, spanning input -1 .. +1, read with linear
    interpolation at the input's VALUE.  With tbl = float32(table) widened to float64, in float64 and every operation rounded:
        c = clip(x, -1, 1)                                                 (+-inf clip; NaN stays NaN)
        h = (T - 1) * 0.5;  u = (c + 1.0) * h                              (in [0, T - 1])
        i = min(floor(u), T - 2);  f = u - i                               (f in [0, 1]: x = +1 reads the last segment at f = 1)
        w = clip(floor(select), 0, W - 1)                                  (per voice; NaN and unplugged: column 0)
        out = tbl[i, w] + f * (tbl[i+1, w] - tbl[i, w])                    (NaN where x is NaN)
    (kernel: sig_shaper_table; restated in numpy by tests/shaper_reference.py).  Ports: `input` at frame rate, `select` at block
    rate.  T >= 2, any integer (2^k + 1 points put a knot at x = 0), T * W <= 16384; integer arrays (what a .sigs value arrives
    as) are converted; the device copy is float32 and follows in-place edits of the array.  The default table [[-1], [1]] is the
    identity on [-1, 1]: a hard clip.  Position-pure when its input is, no context rows.  The map is continuous and piecewise
    linear, Lipschitz with L = max_i |tbl[i+1, w] - tbl[i, w]| * (T - 1) / 2.
    Out of scope: the node inside a block-rate control path (the batched engine answers NotBatchable with the reason and the
    graph keeps the eager path, which serves frames == 1 in float64); a combination with a band filter or a phase-modulation
    oscillator in one voice program (such a graph stays one kernel per node unless the renderer is given mixed_programs=True); oversampling and anti-aliasing of the shaper;
    morphing between columns; a frame-rate `select`; the closed-form, row-walker and cascade fused kernels."""
    input: Receiver.BoundPort = port('input')
    select: Receiver.BoundPort = port('select')

    @state
    class State(BlockCachingEmitter.State):
        table: np.ndarray = attr.ib(factory=lambda: np.array([[-1.0], [1.0]]), validator=_validate_curves,
                                    on_setattr=attr.setters.validate)

    def __init__(self):
        super().__init__()
        self._resident = ResidentCopy(np.float32)

    @classmethod
    def flags(cls) -> SignalFlags:
        return super().flags() | SignalFlags.EFFECT

    def resident_table(self) -> torch.Tensor:
        return self._resident.of(self._state.table)

    def _eval(self, request: Request) -> torch.Tensor:
        select = as_control(self.select.forward_at_block_rate(request))        # unplugged: zeros((1, 1)) = column 0
        x = self.input.forward(request)
        if x.dtype not in (torch.float32, torch.float64) or (x.shape[1] > 1 and x.stride(1) != 1):
            x = x.to(result_dtype(x.shape[0])).contiguous()
        frames, voices = broadcast_shape(x.shape, select.shape)
        out = torch.empty((frames, voices), dtype=result_dtype(frames), device=select.device)
        return _native.shaper_table(x, select, self.resident_table(), out)


def _window_eval(node, request: Request, control: torch.Tensor, launch) -> torch.Tensor:
    """One block of a window node (Delay, FIR): `input` is asked for a filter's window -- [<= 100 context rows | block | 100 rows after],
    the rows after requested and discarded -- and `launch(rate, position, frames, 1, window, history, control, out=...)` renders the
    block from its first history + frames rows.  `control`: the node's block-rate control reply; it and the window broadcast from width
    1, narrower than the request otherwise is the IndexError of a narrow `cutoff`; a window that lacks its context rows is the
    reference's ValueError"""
    context_frames = node.context_frames()
    window = node.input.forward_with_context(request, context_frames)
    loc, shape = request.loc, request.loc.shape
    for reply in (window, control):
        if 1 < reply.shape[1] < shape.channels:
            raise IndexError(f'index {reply.shape[1]} is out of bounds for axis 1 with size {reply.shape[1]}')
    history = window.shape[0] - shape.frames - context_frames             # rows the `before` request returned
    if history != min(context_frames, loc.position):
        raise ValueError(f'could not broadcast input array from shape ({window.shape[0] - context_frames},) '
                         f'into shape ({shape.frames},)')
    buf = window[:history + shape.frames, :shape.channels]
    if buf.dtype not in (torch.float32, torch.float64):
        buf = buf.to(result_dtype(shape.frames))
    control = control[:, :shape.channels]
    if not control.is_contiguous():
        control = control.contiguous()
    voices = max(buf.shape[1], control.shape[1])
    out = torch.empty((shape.frames, voices), dtype=result_dtype(shape.frames), device=buf.device)
    return launch(loc.rate, loc.position, shape.frames, 1, buf, history, control, out=out)


def _validate_taps(instance, attribute, new_value):
    ok = (isinstance(new_value, np.ndarray) and new_value.ndim == 2 and new_value.dtype.kind in 'fiu'
          and new_value.shape[1] == 2 and 1 <= new_value.shape[0] <= _native.DELAY_MAX_TAPS
          and bool(np.isfinite(new_value).all()))
    if not ok:
        raise BadStateValue(instance, attribute.name, new_value,
                            f'must be a 2D real array (taps, 2) of finite (time multiplier, gain) rows, 1 <= taps <= '
                            f'{_native.DELAY_MAX_TAPS}')


class Delay(BlockCachingEmitter, ImplicitChannels):
    """Short multi-tap delay line with linear interpolation, up to 99 frames (2 ms at 48 kHz): the flanger
    `Mix(x, Delay(x, time=LFO))`, a feed-forward comb or a multi-tap comb series in front of a filter, a sub-2 ms stereo decorrelator in
    front of `SumBus`, a fractional-sample phase aligner.  The state `taps` is a (U, 2) array, 1 <= U <= 16: row u holds (m_u, g_u),
    a multiplier of `time` and a gain; the default [[1.0, 1.0]] is one tap at `time`.  Ports: `input` at frame rate; `time` (seconds)
    at block rate, read once per block at the block's position like every control (unplugged or disabled: 0).  Per voice v and
    block, in float64 and every operation rounded, the input widened exactly, x[m] = 0 for an absolute frame m < 0:
        t   = time[0, v]
        d_u = clip((t * rate) * m_u, 0, 99)                                (np.clip: NaN stays NaN, +inf -> 99, -inf -> 0)
        i_u = floor(d_u);  f_u = d_u - i_u
        s_u[n] = x[n - i_u] + f_u * (x[n - i_u - 1] - x[n - i_u])
        out[n] = g_0 * s_0[n]  (+ g_1 * s_1[n] + ...  added in ascending u)
    (kernel: sig_delay_taps; restated in numpy by tests/delay_reference.py).  A NaN d_u makes every row of that voice in that block
    NaN; no status bit is set.  One tap (1, 1) at time = 0 is the identity, an integral d the shifted input, both bit for bit.
    The node takes its window exactly as a filter does -- [<= 100 context rows | block | 100 rows after], the rows after discarded
    but requested, so that upstream caches see what a filter would leave them -- and to the batched engine it IS a
    filter: request-dependent, min(100, position) history rows, tails between batches, no batch of blocks <= 100 frames over an
    impure input.  `input` of width 1 broadcasts; `time` or `input` narrower than the request but wider than 1 raises the IndexError
    of a narrow `cutoff`.  Integer arrays (what a .sigs value arrives as) are converted; the taps travel by value with each launch,
    so an in-place edit of the array or a replaced array takes effect at the next render.
    Out of scope: delays beyond 99 frames (chorus, echo, reverb: they need a longer context than the block semantics have, and a ring
    per lane in the voice-program machine); feedback inside the node (a truncated comb series is spelled with `taps`); a frame-rate
    `time`; interpolation above linear; the voice program, the specialised build and the fused kernels (a graph with the node
    renders one kernel per node); the node inside a block-rate control path (the batched engine answers NotBatchable with the reason
    and the graph keeps the eager path, which serves frames == 1 in float64)."""
    input: Receiver.BoundPort = port('input')
    time: Receiver.BoundPort = port('time')

    @state
    class State(BlockCachingEmitter.State):
        taps: np.ndarray = attr.ib(factory=lambda: np.array([[1.0, 1.0]]), validator=_validate_taps, on_setattr=attr.setters.validate)

    @classmethod
    def flags(cls) -> SignalFlags:
        return super().flags() | SignalFlags.EFFECT

    def context_frames(self) -> int:
        return _native.DELAY_CONTEXT

    def host_taps(self) -> np.ndarray:
        """the (U, 2) float64 array a launch takes by value, as the state holds it now"""
        return np.ascontiguousarray(self._state.taps, dtype=np.float64)

    def _eval(self, request: Request) -> torch.Tensor:
        time = as_control(self.time.forward_at_block_rate(request))            # unplugged: zeros((1, 1)), no delay
        return _window_eval(self, request, time, lambda *head, out: _native.delay_taps(*head, self.host_taps(), out))


def _validate_fir_taps(instance, attribute, new_value):
    ok = (isinstance(new_value, np.ndarray) and new_value.ndim == 2 and new_value.dtype.kind in 'fiu'
          and 1 <= new_value.shape[0] <= _native.FIR_MAX_TAPS and new_value.shape[1] >= 1
          and new_value.shape[0] * new_value.shape[1] <= _native.FIR_MAX_POINTS
          and bool(np.isfinite(new_value).all()))
    if not ok:
        raise BadStateValue(instance, attribute.name, new_value,
                            f'must be a finite 2D real array (taps, columns), 1 <= taps <= {_native.FIR_MAX_TAPS}, columns >= 1, '
                            f'taps * columns <= {_native.FIR_MAX_POINTS}')


def _fir_window(name: str, L: int) -> np.ndarray:
    """the (L,) window of a windowed-sinc design, symmetric about (L - 1) / 2.  Blackman and Hann are sampled at (k + 1) / (L + 1), the
    L interior points of the (L + 2)-point window: their end points are zeros, which would waste two of at most 101 taps"""
    k = np.arange(L, dtype=np.float64)
    if name in ('rectangular', 'boxcar', None):
        return np.ones(L)
    a = 2.0 * np.pi * (k + 1.0) / (L + 1.0)
    if name == 'blackman':
        return 0.42 - 0.5 * np.cos(a) + 0.08 * np.cos(2.0 * a)
    if name == 'hann':
        return 0.5 - 0.5 * np.cos(a)
    if name == 'hamming':
        return 0.54 - 0.46 * np.cos(2.0 * np.pi * k / (L - 1)) if L > 1 else np.ones(L)
    raise ValueError(f'unknown window {name!r}: blackman, hamming, hann or rectangular')


def _fir_mirror(h: np.ndarray, sign: float = 1.0) -> np.ndarray:
    """the (L, 1) column whose second half is the first half mirrored (times `sign`), so that h[k] == sign * h[L - 1 - k] bit for bit"""
    L = h.shape[0]
    out = np.array(h, dtype=np.float64)
    half = L // 2
    out[L - half:] = sign * out[:half][::-1]
    return out.reshape(L, 1)


def _fir_sinc(cutoff: float, rate: float, L: int, window: str) -> np.ndarray:
    """the windowed ideal low-pass of `cutoff` Hz, (L,), not normalised"""
    if isinstance(L, bool) or not isinstance(L, (int, np.integer)) or not 1 <= L <= _native.FIR_MAX_TAPS:
        raise ValueError(f'taps must be an integer 1 .. {_native.FIR_MAX_TAPS}, got {L!r}')
    if not (np.isfinite(cutoff) and np.isfinite(rate) and rate > 0 and 0 < cutoff < rate / 2):
        raise ValueError(f'a cutoff lies inside (0, rate / 2), got {cutoff!r} at rate {rate!r}')
    fc = float(cutoff) / float(rate)
    m = np.arange(L, dtype=np.float64) - (L - 1) / 2.0
    return 2.0 * fc * np.sinc(2.0 * fc * m) * _fir_window(window, L)


class FIR(fx.CritFilter):
    """Dense finite-impulse-response filter of up to 101 taps: the one filter class the block structure renders EXACTLY -- x[n - 100]
    .. x[n] is precisely the window a filter is handed, so nothing of the impulse response is truncated, where every recursive
    filter here answers a block from zero state over 100 context rows.  Linear-phase low-pass / high-pass / band-pass (crossovers and
    band splits), a Hilbert transformer (with `Delay` at the group delay as the matched path: single-sideband frequency shifting,
    `RingMod(Delay(x), cos) - RingMod(FIR_hilbert(x), sin)`), a differentiator, a pre-emphasis, a short body or cabinet response.
    The state `taps` is an (L, W) real array, 1 <= L <= 101, W >= 1, L * W <= 4096, every value finite: W impulse responses of L taps,
    column w = h[:, w]; integer arrays (what a .sigs value arrives as) are converted; the device copy is float64 and follows in-place
    edits of the array.  The default [[1.0]] is the identity.  Ports: `input` at frame rate; `select` at block rate, read once per
    block at the block's position like every control (unplugged, disabled or NaN: column 0).  Per voice v and block, in float64 and
    every operation rounded (no fma), the input widened exactly:
        w      = clip(floor(select[0, v]), 0, W - 1)
        x[m]   = +0.0  for an absolute frame m < 0
        acc    = h[0, w] * x[n]
        acc    = acc + h[k, w] * x[n - k]        for k = 1 .. L - 1, ascending
        out[n] = acc
    (kernel: sig_fir_taps; restated in numpy by tests/fir_reference.py).  No tap is skipped: zero taps and the zero-filled rows are
    multiplied and added like the rest, so NaN and +-inf in the input propagate exactly as the numpy restatement's do; no status bit
    is set.  [[1.0]] returns the input and a unit tap at k = d the input d frames late, both bit for bit on finite input.
    The node takes its window exactly as `Delay` does -- [<= 100 context rows | block | 100 rows after], the rows after discarded but
    requested, so that upstream caches see what a filter would leave them -- and to the batched engine it IS a
    filter: request-dependent, min(100, position) history rows, tails between batches, no batch of blocks <= 100 frames over an
    impure input.  `input` of width 1 broadcasts; `select` or `input` narrower than the request but wider than 1 raises the
    IndexError of a narrow `cutoff`.  Like `Ladder` it is an `fx.CritFilter` -- that class is what the engine's planner means by "takes
    a filter's window" -- but not an `fx.SingleCritFilter` or `fx.DoubleCritFilter`: to the voice program and the fused matchers
    those mean a biquad.  Its type is its own (`FIR.Type.fir`); it has no cutoff and no status word.
    Designers (static, numpy on the host): `FIR.lowpass`, `FIR.highpass`, `FIR.bandpass`, `FIR.hilbert`; each returns an (L, 1)
    float64 column, so a bank is an `np.hstack`.  A symmetric or antisymmetric design of L taps has the group delay (L - 1) / 2
    frames at every frequency: 50 frames at the default 101 taps.
    Out of scope: more than 101 taps (partitioned or FFT convolution, and a longer context than the block semantics have); a
    frame-rate `select` and morphing between columns; float32 or matrix-core accumulation; an fma build of the sum (it would halve
    the arithmetic and change the bits: not measured); the voice program, the specialised build and the fused kernels (a graph with
    the node renders one kernel per node); the node inside a block-rate control path (the batched engine answers NotBatchable with
    the reason and the graph keeps the eager path, which serves frames == 1 in float64); the random-graph generator of the tests."""
    select: Receiver.BoundPort = port('select')

    class Type(str, enum.Enum):
        """the node's own filter type: no entry of the biquad kernels takes it"""
        fir = 'fir'

        def __str__(self) -> str:
            return str(self.value)

        @property
        def is_band(self) -> bool:
            return False

    @state
    class State(fx.CritFilter.State):
        taps: np.ndarray = attr.ib(factory=lambda: np.array([[1.0]]), validator=_validate_fir_taps, on_setattr=attr.setters.validate)

    def __init__(self):
        super().__init__()
        self._resident = ResidentCopy(np.float64)

    @classmethod
    def flags(cls) -> SignalFlags:
        return super().flags() | SignalFlags.EFFECT

    def type(self) -> 'FIR.Type':
        return self.Type.fir

    def context_frames(self) -> int:
        return _native.FIR_CONTEXT

    def host_taps(self) -> np.ndarray:
        """the (L, W) float64 array as the state holds it now"""
        return np.ascontiguousarray(self._state.taps, dtype=np.float64)

    def resident_table(self) -> torch.Tensor:
        """the (L, W) float64 device copy of `taps`; an in-place edit or a replaced array is seen at the next render"""
        return self._resident.of(self._state.taps)

    # ---- designers: numpy on the host, one (L, 1) float64 column each
    @staticmethod
    def lowpass(cutoff: float, rate: float, taps: int = 101, window: str = 'blackman') -> np.ndarray:
        """windowed-sinc linear-phase low-pass, h[k] == h[L - 1 - k] bit for bit, unit gain at DC; group delay (L - 1) / 2 frames"""
        h = _fir_mirror(_fir_sinc(cutoff, rate, taps, window))
        return _fir_mirror(h[:, 0] / np.sum(h[:, 0]))

    @staticmethod
    def highpass(cutoff: float, rate: float, taps: int = 101, window: str = 'blackman') -> np.ndarray:
        """the spectral inversion of `lowpass`: a unit tap at the centre minus the low-pass, so odd lengths only; zero gain at DC up to
        rounding; group delay (L - 1) / 2 frames"""
        if isinstance(taps, (int, np.integer)) and taps % 2 == 0:
            raise ValueError(f'a high-pass needs an odd number of taps (a centre tap), got {taps}')
        h = -FIR.lowpass(cutoff, rate, taps, window)
        h[(taps - 1) // 2, 0] += 1.0
        return h

    @staticmethod
    def bandpass(low: float, high: float, rate: float, taps: int = 101, window: str = 'blackman') -> np.ndarray:
        """the difference of two windowed-sinc low-passes, mirrored, unit gain at the band's centre (low + high) / 2; group delay
        (L - 1) / 2 frames"""
        if not low < high:
            raise ValueError(f'a band needs low < high, got {low!r}, {high!r}')
        h = _fir_mirror(_fir_sinc(high, rate, taps, window) - _fir_sinc(low, rate, taps, window))[:, 0]
        m = np.arange(taps, dtype=np.float64) - (taps - 1) / 2.0
        centre = np.pi * (float(low) + float(high)) / float(rate)               # radians per frame
        gain = np.sum(h * np.cos(centre * m))                                  # the zero-phase response of a symmetric h
        if not abs(gain) > 0:
            raise ValueError('the design has no gain at the band centre (too few taps for the band)')
        return _fir_mirror(h / gain)

    @staticmethod
    def hilbert(taps: int = 101, window: str = 'blackman') -> np.ndarray:
        """windowed ideal Hilbert transformer (a 90 degree phase shifter): h[c + m] = 2 / (pi m) for odd m, exactly 0 for even m (the
        centre too), antisymmetric h[k] == -h[L - 1 - k] bit for bit; odd lengths only; group delay (L - 1) / 2 frames, so the matched
        path is a delay of that many frames"""
        if isinstance(taps, bool) or not isinstance(taps, (int, np.integer)) or not 1 <= taps <= _native.FIR_MAX_TAPS or taps % 2 == 0:
            raise ValueError(f'a Hilbert transformer needs an odd number of taps 1 .. {_native.FIR_MAX_TAPS}, got {taps!r}')
        c = (taps - 1) // 2
        m = np.arange(taps) - c
        h = np.zeros(taps)
        odd = (m % 2) != 0
        h[odd] = 2.0 / (np.pi * m[odd]) * _fir_window(window, taps)[odd]
        return _fir_mirror(h, -1.0)

    def _eval(self, request: Request) -> torch.Tensor:
        select = as_control(self.select.forward_at_block_rate(request))        # unplugged: zeros((1, 1)) = column 0
        return _window_eval(self, request, select, lambda *head, out: _native.fir_taps(*head, self.resident_table(), out))


def _validate_recordings(instance, attribute, new_value):
    ok = (isinstance(new_value, np.ndarray) and new_value.ndim == 2 and new_value.dtype.kind in 'fiu'
          and new_value.shape[0] >= 2 and new_value.shape[1] >= 1
          and new_value.shape[0] * new_value.shape[1] <= _native.SAMPLER_MAX_POINTS)
    if not ok:
        raise BadStateValue(instance, attribute.name, new_value,
                            f'must be a 2D real array (frames, recordings), frames >= 2, frames * recordings <= '
                            f'{_native.SAMPLER_MAX_POINTS}')


def _validate_loop(instance, attribute, new_value):
    """what the state alone decides: an integer >= 0, and loop_start < loop_end where a loop is on.  The table's length is checked at
    every render: the table may be set after the bounds (a patch sets its properties in the order written) or replaced later."""
    if isinstance(new_value, (bool, np.bool_)) or not isinstance(new_value, (int, np.integer)) or new_value < 0:
        raise BadStateValue(instance, attribute.name, new_value, 'must be an integer >= 0, in frames')
    start = new_value if attribute.name == 'loop_start' else getattr(instance, 'loop_start', 0)
    end = new_value if attribute.name == 'loop_end' else getattr(instance, 'loop_end', 0)
    if end != 0 and not start < end:
        raise BadStateValue(instance, attribute.name, new_value, f'a loop needs loop_start < loop_end, got {start} and {end}')


class Sampler(BankEmitter):
    """Sample playback: the state `table` holds W recordings of T frames each as a (T, W) array (the reference's (frames, channels)
    orientation), recorded at the graph's rate; every voice plays one of them from a trigger time, at its own speed and start, with
    linear interpolation -- a drum hit per voice, a multisample transposed per voice, a looped pad.  Ports, all at block rate and read
    once per block at the block's position like every control: `ratio` (playback speed, 1 = the original; unplugged reads zeros like
    every port, so set it), `offset` (frames into the recording at the trigger), `gate_on` (seconds, ADSR's meaning), `select` (the
    column: w = clip(floor(select), 0, W - 1), NaN and unplugged = 0, Wavetable's rule).  State: `table`, T >= 2, W >= 1, T * W <=
    2**26, integer arrays (what a .sigs value arrives as) are converted, the device copy is float32 and follows in-place edits and
    replacement; `loop_start`, `loop_end` in frames, loop_end == 0 (the default) = no loop, else 0 <= loop_start < loop_end <= T
    (the order is checked on set, the table's length at every render, where it raises BadStateValue: the table may have been
    replaced).  The node is a pure function of the absolute frame, like `osc.Osc`, `ext.ADSR` and `ext.SyncOsc`: no carried read
    pointer, so a block-rate change of `ratio` moves the read position exactly as a block-rate change of `hertz` moves an oscillator's
    phase -- and it needs no context rows, no history and no tails, and renders from any position.  For absolute frame n and voice v,
    in float64 and every operation rounded, no fused multiply-add, tbl = float32(table) widened to float64:
        q  = n / rate                                  (osc.py's order: one IEEE divide)
        e  = q - gate_on[v]
        s  = e * rate
        u  = s * ratio[v] + offset[v]                  (two roundings)
        not (e >= 0)           -> out = 0              (before the trigger; a NaN gate is silence)
        u is NaN or +-inf      -> out = NaN            (no index is formed from it)
        no loop:  u < 0 or u > T - 1 -> out = 0        (outside the recording)
                  i = floor(u); f = u - i; j = min(i + 1, T - 1)
        loop:     u < 0 -> out = 0
                  L = loop_end - loop_start
                  u >= loop_end:  c = floor((u - loop_start) / L);  u = (u - loop_start) - c * L + loop_start
                                  if that rounds to u >= loop_end:  u = loop_start
                                  (likewise if it falls below loop_start: from 2**53 frames on the rounded quotient can exceed the true one)
                  i = floor(u); f = u - i; j = (i + 1 >= loop_end) ? loop_start : i + 1
        out = tbl[i, w] + f * (tbl[j, w] - tbl[i, w])
    (kernel: sig_sampler_play; restated in numpy by tests/sampler_reference.py).  The rows are float32, a one-frame request float64;
    no status bit is set for any input.  The width is the broadcast of the four control rows; a control narrower than the request but
    wider than 1 raises the IndexError of a narrow `cutoff`.  Amplitude shaping and release are not the node's job:
    `RingMod(Sampler, ADSR)` with the same `gate_on` does them.  `Sampler.table_from_wav(path)` reads a WAV file into a table.
    Out of scope: a carried read pointer (varispeed without jumps); a frame-rate `ratio`; interpolation above linear, and
    anti-aliasing when ratio > 1; a recording rate other than the graph's (fold it into `ratio`); reverse loops and crossfades; the
    voice program, the specialised build and the fused kernels (a graph with the node renders one kernel per node); the node inside a
    block-rate control path (the batched engine answers NotBatchable with the reason and the graph keeps the eager path, which serves
    frames == 1 in float64)."""
    ratio: Receiver.BoundPort = port('ratio')
    offset: Receiver.BoundPort = port('offset')
    gate_on: Receiver.BoundPort = port('gate_on')
    select: Receiver.BoundPort = port('select')

    @state
    class State(BlockCachingEmitter.State):
        table: np.ndarray = attr.ib(factory=lambda: np.array([[0.0], [0.0]]), validator=_validate_recordings,
                                    on_setattr=attr.setters.validate)
        loop_start: int = attr.ib(default=0, validator=_validate_loop, on_setattr=attr.setters.validate)
        loop_end: int = attr.ib(default=0, validator=_validate_loop, on_setattr=attr.setters.validate)

    def __init__(self):
        super().__init__()
        self._resident = ResidentCopy(np.float32, layout=np.transpose)

    @classmethod
    def flags(cls) -> SignalFlags:
        return super().flags() | SignalFlags.EPOCH

    @staticmethod
    def table_from_wav(path) -> np.ndarray:
        """the (T, W) float64 array of a WAV file (PCM_16 or FLOAT, chain/files.py's reader): W = the file's channels.  Host only; the
        file's rate is not looked at -- fold a rate other than the graph's into `ratio`"""
        import pathlib
        from signals_amd.chain import files
        wav = files._WaveFile(pathlib.Path(path), 'r')
        try:
            return np.ascontiguousarray(wav.read(0, wav.frames), dtype=np.float64)
        finally:
            wav.close()

    def loop(self) -> tuple[int, int]:
        """(loop_start, loop_end) checked against the table as it is now: BadStateValue where they no longer fit it"""
        s = self._state
        start, end, frames = int(s.loop_start), int(s.loop_end), s.table.shape[0]
        if end != 0 and not 0 <= start < end <= frames:
            raise BadStateValue(s, 'loop_end', end, f'a loop needs 0 <= loop_start < loop_end <= {frames} frames, got {start} and {end}')
        return start, end

    def resident_table(self) -> torch.Tensor:
        """the device copy: float32 (W, T), every recording contiguous -- the transpose of the state's array"""
        return self._resident.of(self._state.table)

    def control_rows(self, fetch, channels: int) -> list:
        """the four control rows (ratio, offset, gate_on, select) as contiguous float64 rows at most `channels` wide"""
        return _request_rows(fetch, (self.ratio, self.offset, self.gate_on, self.select), channels)

    def bank(self, fetch, channels: int) -> tuple:
        rows = self.control_rows(fetch, channels)
        table, (start, end) = self.resident_table(), self.loop()               # (the loop checked against the table as it is now)
        return 'sampler_play', 'Loop' if end else 'OneShot', rows, _bound(_native.sampler_play, table, start, end)


def _validate_modes(instance, attribute, new_value):
    ok = (isinstance(new_value, np.ndarray) and new_value.ndim in (2, 3) and new_value.shape[-1] == 3 and new_value.dtype.kind in 'fiu'
          and 1 <= new_value.shape[-2] <= _native.MODAL_MAX_MODES and new_value.shape[0] >= 1
          and new_value.size // 3 <= _native.MODAL_MAX_POINTS
          and bool(np.isfinite(new_value[..., :2]).all()) and bool((new_value[..., 0] >= 0).all())
          and bool((new_value[..., 2] > 0).all()))                            # (a NaN t60 fails the comparison; inf passes)
    if not ok:
        raise BadStateValue(instance, attribute.name, new_value,
                            f'must be a real array (sets, modes, 3) or (modes, 3) of rows (ratio >= 0, amplitude, t60 > 0), ratios and '
                            f'amplitudes finite, 1 <= modes <= {_native.MODAL_MAX_MODES}, sets * modes <= {_native.MODAL_MAX_POINTS}')


def _mode_rates(modes: np.ndarray) -> np.ndarray:
    """the table a launch reads: float64 (W, M, 3) rows (ratio, amplitude, lambda = ln(1000) / t60); t60 = inf gives 0"""
    rows = np.array(modes, dtype=np.float64).reshape(-1, modes.shape[-2], 3)
    rows[..., 2] = np.log(1000.0) / rows[..., 2]
    return rows


def _mode_count(M, t60) -> np.ndarray:
    """1 .. M as float64, M and t60 checked against the node's limits"""
    if isinstance(M, bool) or not isinstance(M, (int, np.integer)) or not 1 <= M <= _native.MODAL_MAX_MODES:
        raise ValueError(f'modes must be an integer 1 .. {_native.MODAL_MAX_MODES}, got {M!r}')
    if not (np.isfinite(t60) and t60 > 0):
        raise ValueError(f't60 must be a finite time > 0 in seconds, got {t60!r}')
    return np.arange(1, int(M) + 1, dtype=np.float64)


class Modal(BankEmitter):
    """Modal resonator bank: a struck or plucked source.  Every voice rings up to 64 exponentially decaying sinusoids ("modes") from a
    strike time on, each mode with its own frequency ratio, amplitude and decay time -- bells, bars, marimbas, glasses, plucked strings,
    drum shells: the sounds where a partial has a life of its own, which `Additive` (harmonic ratios, amplitudes fixed per block)
    cannot make.  Ports, all at block rate and read once per block at the block's position like every control: `hertz` (the
    fundamental the ratios multiply), `gate_on` (the strike time in seconds, ADSR's and Sampler's meaning), `damp` (an extra decay rate in
    1 / s added to every mode; unplugged reads 0; a hand laid on the bell is a step on this port), `select` (the mode set: w =
    clip(floor(select), 0, W - 1), NaN and unplugged = 0, Wavetable's rule).  State `modes`: a real array (W, M, 3) -- (M, 3) means
    W = 1 -- whose row i of set w is (ratio r >= 0, amplitude a, t60 in seconds: the time to fall by 60 dB, > 0, inf = undamped);
    1 <= M <= 64, W * M <= 2048, every r and a finite, integer arrays (what a .sigs value arrives as) are converted; checked on set.  The
    default [[1, 1, 1]] is a one-second sine ping.  The device copy is float64 rows (r, a, lambda), lambda = ln(1000) / t60 computed on the
    host (float32 ratios would move a partial by 1e-7 of its frequency: a drifting beat pattern over a long note); it follows in-place
    edits and replacement.  For absolute frame n and voice v, in float64 and every operation rounded, no fused multiply-add, the modes
    i = 0 .. M - 1 added in ascending order:
        q = n / rate                                   (osc.py's order: one IEEE divide)
        e = q - gate_on
        not (e >= 0)          -> out = 0.0             (before the strike; a NaN gate is silence; exact zero, never NaN)
        F_i = hertz * r_i
        g_i = clip(((0.5 * rate) - |F_i|) / |hertz|, 0, 1)         (IEEE: hertz = 0 gives +inf -> 1)
        c_i = e * F_i;  m_i = np.mod(c_i, 1.0)
        k_i = (lambda_i + damp) * e
        out = sum_i (a_i * g_i) * exp(-k_i) * sin(2 pi m_i)        (a mode with g_i == 0 adds exactly 0)
    (kernel: sig_modal_bank; restated in numpy by tests/modal_reference.py).  g_i is Additive's fade: a mode fades linearly to nothing
    over the last |hertz| below half the rate, so a pitch envelope neither aliases nor clicks; a mode at or above half the rate adds
    exactly 0, and with every mode dropped the output is exactly 0.0.  Every mode starts at phase 0, so the onset is continuous and needs
    no attack ramp; a fractional gate_on * rate places the strike between frames.  A `hertz` that is NaN or infinite gives NaN on sounding
    rows (e >= 0) and 0.0 before the strike.  `damp` is used as given: a negative damp lengthens the decays and, below -lambda_i, makes
    mode i GROW (exp of a positive number, inf in the end); a damp that is NaN or infinite gives NaN on sounding rows (the definition's
    inf * 0 at the strike, held for the rest of the note).  No status bit is set for any input.
    One strike is alive per voice -- polyphony is voices: a new gate_on in the future silences the voice until it arrives, as with
    `Sampler`; strike velocity is a `Gain` behind the node.  `hertz` multiplies the ELAPSED TIME, not an integrated phase -- this
    project's oscillator convention, no carried phase: a pitch bend late in a note therefore moves the phase of mode i by e * r_i * (the
    change of hertz) cycles at once, a jump that grows with the time since the strike -- bend early, or change pitch only with a new
    strike.  The decay of a mode is in seconds and does not scale with `hertz`.
    The rows are float32, a one-frame request float64.  The width is the broadcast of the four control rows; a control narrower than the
    request but wider than 1 raises the IndexError of a narrow `cutoff`.
    Because of exp and sin the kernel is held to a bound, not to bits: every sample within 1e-6 * max(1, A) of the definition, A the
    largest set's sum of |a|.  It starts each run of 64 frames (frames 64 k .. 64 k + 63) from the closed form at the voice's first
    sounding frame of the run and advances by one complex multiplication per frame and mode; a sample's bits depend on its frame and
    its voice's parameters only, so a block rendered alone and inside a batch are equal bit for bit.  Measured on an MI355X over the
    kernel cases of tests/test_gpu_modal.py (M up to 64, A up to 4.7): in front of the float64 store 2.1e-12 at most up to position
    1000, 1.0e-9 at 2**24 and 4.6e-7 at 2**31 frames -- a tenth of the bar, and the distance of the float64 definition itself from
    extended precision there: the rounding of n / rate, which the definition takes row by row and the recurrence once per run; behind
    the float32 store 6.0e-8 (that store's own rounding) and the float64 figure at 2**31.
    Position-pure: no state, no history, no context rows.  The batched engine renders the node with one kernel per batch; it has no
    voice-program word, so a graph that contains one runs one kernel per node (the nodes around it keep their routes), `mixed_programs`
    and `specialise` or not.
    Mode sets (static, numpy on the host, (M, 3) each): `Modal.string(M, t60)`, `Modal.bar(M, t60)`, `Modal.bell(t60)`;
    `Modal.stack(sets)` pads sets to a common M and returns (W, M, 3) for `select`.
    Out of scope: a voice-program word, specialised or fused kernels; the node inside a block-rate control path (the batched engine
    answers NotBatchable with the reason and the graph keeps the eager path, which serves frames == 1 in float64); frame-rate ports;
    a phase or a cosine term per mode; more than one strike alive per voice, and strike velocity; excitation by an input signal (a driven
    resonator needs history); more than 64 modes."""
    hertz: Receiver.BoundPort = port('hertz')
    gate_on: Receiver.BoundPort = port('gate_on')
    damp: Receiver.BoundPort = port('damp')
    select: Receiver.BoundPort = port('select')

    @state
    class State(BlockCachingEmitter.State):
        modes: np.ndarray = attr.ib(factory=lambda: np.array([[1.0, 1.0, 1.0]]), validator=_validate_modes,
                                    on_setattr=attr.setters.validate)

    def __init__(self):
        super().__init__()
        self._resident = ResidentCopy(np.float64, layout=_mode_rates)

    # ---- mode sets: numpy on the host, one (M, 3) float64 array of rows (ratio, amplitude, t60) each
    @staticmethod
    def string(M: int = 32, t60: float = 2.0) -> np.ndarray:
        """a plucked string: harmonic ratios i, amplitudes 1 / i, decay times t60 / i (i = 1 .. M)"""
        i = _mode_count(M, t60)
        return np.stack([i, 1.0 / i, float(t60) / i], axis=1)

    @staticmethod
    def bar(M: int = 8, t60: float = 1.0) -> np.ndarray:
        """a free-free bar (marimba, glockenspiel): the Euler-Bernoulli beam's modes lie at the squares of the roots x_i of
        cos(x) cosh(x) = 1 -- 4.7300, 7.8532, 10.9956, 14.1372, 17.2788, then (2 i + 1) pi / 2 to nine digits -- so the ratios are
        (x_i / x_1)^2 = 1, 2.7565, 5.4039, 8.9330, ... (the usual short form ((2 i + 1) / 3.0112)^2 gives 2.7572 for the second);
        amplitudes 1 / i, decay times t60 / ratio (the same number of cycles for every mode)"""
        i = _mode_count(M, t60)
        root = (2.0 * i + 1.0) * (np.pi / 2.0)
        exact = np.array([4.730040744862704, 7.853204624095838, 10.995607838001671, 14.137165491257464, 17.278759657399481])
        root[:5] = exact[:len(root)]
        ratio = (root / root[0]) ** 2
        return np.stack([ratio, 1.0 / i, float(t60) / ratio], axis=1)

    @staticmethod
    def bell(t60: float = 6.0) -> np.ndarray:
        """a minor-third church bell, twelve modes: hum 0.5, prime 1, tierce 1.2, quint 1.5, nominal 2, and above the nominal the just
        intervals a bell founder tunes towards -- deciem 2.5, undeciem 8 / 3, duodeciem 3, double octave 4, upper undeciem 16 / 3, upper
        sixth 20 / 3, triple octave 8 (the ideal partials of a tuned bell as tabulated in Fletcher and Rossing, The Physics of Musical
        Instruments, chapter 21; a cast bell's upper partials lie within a few per cent of them).  The hum rings for t60, a mode of
        ratio r for t60 / (2 r); the amplitudes are a strike's, loudest at the prime and the nominal"""
        _mode_count(1, t60)
        ratio = np.array([0.5, 1.0, 1.2, 1.5, 2.0, 2.5, 8.0 / 3.0, 3.0, 4.0, 16.0 / 3.0, 20.0 / 3.0, 8.0])
        level = np.array([0.6, 1.0, 0.8, 0.5, 1.0, 0.4, 0.3, 0.5, 0.35, 0.2, 0.15, 0.1])
        return np.stack([ratio, level, float(t60) / (2.0 * ratio)], axis=1)

    @staticmethod
    def stack(sets) -> np.ndarray:
        """(W, M, 3) from W sets of (M_w, 3) rows, M the longest: shorter sets are padded with rows (0, 0, 1) of zero amplitude"""
        sets = [np.asarray(s, dtype=np.float64) for s in sets]
        if not sets or any(s.ndim != 2 or s.shape[1] != 3 or s.shape[0] < 1 for s in sets):
            raise ValueError('stack takes one or more (modes, 3) arrays')
        out = np.tile(np.array([0.0, 0.0, 1.0]), (len(sets), max(s.shape[0] for s in sets), 1))
        for w, s in enumerate(sets):
            out[w, :s.shape[0]] = s
        return out

    def resident_modes(self) -> torch.Tensor:
        """the device copy: float64 (W, M, 3) rows (ratio, amplitude, lambda)"""
        return self._resident.of(self._state.modes)

    def control_rows(self, fetch, channels: int) -> list:
        """the four control rows (hertz, gate_on, damp, select) as contiguous float64 rows at most `channels` wide"""
        return _request_rows(fetch, (self.hertz, self.gate_on, self.damp, self.select), channels)

    def bank(self, fetch, channels: int) -> tuple:
        rows, modes = self.control_rows(fetch, channels), self.resident_modes()
        return 'modal_bank', f'Modal{modes.shape[1]}', rows, _bound(_native.modal_bank, modes)


class ResonantFilter(fx.CritFilter, abc.ABC):
    """Resonant 2-pole low-pass / high-pass: the bilinear transform with prewarping of the analogue second-order section with quality
    factor q -- the RBJ cookbook's low-pass / high-pass (alpha = sin(w0) / (2 q)) in another form, the reference's Butterworth
    `fx.LowPass` / `fx.HighPass` at q = 1/sqrt2, a peak of about q at the cutoff above that: filter sweeps, acid basses, resonant pads.
    Ports: `input` at frame rate; `cutoff` (Hz) and `resonance` (q, dimensionless) at block rate.  Per voice and block, in float64:
        wn = clip(cutoff / (rate / 2), 0, 1)                                (as fx.py:99-102; an error unless 0 < wn < 1, NaN too)
        k = tan(pi * wn / 2);  d = 1 / q;  nrm = 1 / (1 + d*k + k*k)
        lp: b = (k*k, 2*k*k, k*k) * nrm        hp: b = (1, -2, 1) * nrm
        a = (1, 2*(k*k - 1)*nrm, (1 - d*k + k*k)*nrm)
    then `CritFilter._filter` exactly as for `fx.LowPass`: zero state over [<= 100 context rows | block], one section, sosfilt's
    transposed direct form II, both controls read once per block at the block's position (kernel: sig_biquad_coldstart_q; restated in
    numpy by tests/resonant_reference.py).  Stable for every q > 0.
    An unplugged or disabled `resonance` means q = 1/sqrt2, the Butterworth response (d = sqrt2 itself) -- NOT the zeros((1, 1)) every
    other unplugged port answers: the one place where this node departs from "unplugged answers zero".  A plugged q that is 0,
    negative, NaN or +-inf is an error like a bad cutoff: the voice's rows are NaN and `runtime.check_status()` raises
    ValueError('...: filter resonance must be finite and > 0').  `resonance` narrower than the request raises the IndexError of a
    narrow `cutoff`.
    Not an `fx.SingleCritFilter`: to the engine's fused kernels that class means a Butterworth filter with one control port.
    The inherited limit: the filter rings for about q * rate / (pi * cutoff) frames, and the reference's 100-frame cold start
     truncates that.  At q = 8 and 48 kHz the share of the impulse response's L1 norm beyond 100 frames
    is 83 % at 200 Hz, 45 % at 1 kHz, 9 % at 3 kHz: the node matches a streaming filter only where the ring time is well under 100
    frames.  That is the reference's block semantics, not a defect of this node.
    Out of scope: the closed-form, row-walker, cascade, enveloped-filter and bus-over-filter fused kernels (none matches the node; the
    voice program is its fast route); the node inside a block-rate control path (the batched engine answers NotBatchable with the
    reason and the graph keeps the eager path); a combination with a band filter, a phase-modulation oscillator, a wavetable
    oscillator or a waveshaper in one voice program (such a graph stays one kernel per node unless the renderer is given mixed_programs=True); band-pass, notch and peaking responses (those are `EqFilter`'s);
    a frame-rate cutoff or q; self-oscillation (q = inf); carried state or a longer context."""
    cutoff: Receiver.BoundPort = port('cutoff')
    resonance: Receiver.BoundPort = port('resonance')

    def _eval(self, request: Request) -> torch.Tensor:
        hertz = as_control(self.cutoff.forward_at_block_rate(request))
        src = self.resonance.sig
        q = None if src is None or not src.get_state().enabled else as_control(self.resonance.forward_at_block_rate(request))
        return self._filter(request, hertz, resonant=True, resonance=q)


class ResonantLowPass(ResonantFilter):
    """`ResonantFilter` with the low-pass numerator b = (k*k, 2*k*k, k*k) * nrm"""

    def type(self) -> fx.CritFilter.Type:
        return self.Type.low_pass


class ResonantHighPass(ResonantFilter):
    """`ResonantFilter` with the high-pass numerator b = (1, -2, 1) * nrm"""

    def type(self) -> fx.CritFilter.Type:
        return self.Type.high_pass


class EqFilter(ResonantFilter, abc.ABC):
    """The RBJ equaliser biquads: band-pass with a constant 0 dB peak (`ResonantBandPass`), `Notch`, `AllPass`, and -- with a third
    control, `gain` in dB -- `Peaking`, `LowShelf`, `HighShelf`: a peaking band to shape a formant, shelves to tilt a voice, a notch or
    an all-pass chain swept by an LFO (the phaser).  `ResonantFilter`'s bilinear transform, s -> (1 - 1/z) / (k (1 + 1/z)), of the
    cookbook's analogue prototypes (BPF, notch, APF, peakingEQ, lowShelf, highShelf), with three free numerator taps.
    Ports: `input` at frame rate; `cutoff` (Hz: the centre, notch, or shelf midpoint frequency) and `resonance` (q) at block rate, both
    exactly as on `ResonantFilter` (an unplugged `resonance` means 1/sqrt2, a bad value the same errors, a narrow control the same
    IndexError); the three gain classes add `gain` (dB) at block rate.  Per voice and block, in float64:
        wn, k = tan(pi * wn / 2) and d = 1 / q as `ResonantFilter`;  A = exp(gain * ln(10) / 40);  g = sqrt(A) * d
        sos = [b * nrm, 1, a1 * nrm, a2 * nrm]
        ResonantBandPass  b = (d*k, 0, -d*k)                                    a1 = 2*(k*k - 1), a2 = 1 - d*k + k*k, 1/nrm = 1 + d*k + k*k
        Notch             b = (1 + k*k, 2*(k*k - 1), 1 + k*k)                   a and nrm as ResonantBandPass
        AllPass           b = (1 - d*k + k*k, 2*(k*k - 1), 1 + d*k + k*k)       a and nrm as ResonantBandPass
        Peaking           b = (1 + d*A*k + k*k, 2*(k*k - 1), 1 - d*A*k + k*k)   a1 = 2*(k*k - 1), a2 = 1 - (d/A)*k + k*k, 1/nrm = 1 + (d/A)*k + k*k
        LowShelf          b = A*(1 + g*k + A*k*k, 2*(A*k*k - 1), 1 - g*k + A*k*k)   a1 = 2*(k*k - A), a2 = A - g*k + k*k, 1/nrm = A + g*k + k*k
        HighShelf         b = A*(A + g*k + k*k, 2*(k*k - A), A - g*k + k*k)         a1 = 2*(A*k*k - 1), a2 = 1 - g*k + A*k*k, 1/nrm = 1 + g*k + A*k*k
    then `CritFilter._filter` exactly as for `ResonantFilter`: zero state over [<= 100 context rows | block], one section, sosfilt's
    transposed direct form II  y = b0 x + z0; z0 = b1 x - a1 y + z1; z1 = b2 x - a2 y,  every control read once per block at the block's
    position (kernel: sig_biquad_coldstart_eq; restated in numpy by tests/eq_reference.py).  `Peaking` at 0 dB has b = a: the input.
    An unplugged or disabled `gain` means 0 dB -- the ordinary zeros((1, 1)) of an unplugged port.  A plugged gain that is NaN or +-inf
    is an error like a bad q: the voice's rows are NaN and `runtime.check_status()` raises ValueError('...: filter gain must be finite').
    `gain` narrower than the request raises the IndexError of a narrow `cutoff`.
    The inherited limit: the 100-frame cold start truncates a ring of about q * rate / (pi * cutoff)
    frames, as for `ResonantFilter`.  It applies most to a high-q `Notch` and `ResonantBandPass` at low cutoffs, whose ring IS the
    response: a notch at 100 Hz and q = 8 rings for some 1200 frames at 48 kHz, and what 100 frames of it reject is far from the
    streaming filter's null.  That is the reference's block semantics, not a defect of this node.
    Out of scope: a frame-rate cutoff, q or gain; the closed-form, row-walker, cascade, enveloped-filter and bus-over-filter fused
    kernels (none matches the node; the voice program is its fast route, through kernels of its own beside the resonant and the mixed
    variant); the node inside a block-rate control path (the batched engine answers NotBatchable with the reason and the graph keeps
    the eager path); a combination with a band filter, a phase-modulation oscillator, a wavetable oscillator, a waveshaper or a unison
    oscillator in one voice program unless the renderer is given mixed_programs=True; the constant-skirt band-pass; the shelf-slope S
    parametrisation (the shelves take q); carried state or a longer context."""

    class Type(str, enum.Enum):
        """the equaliser designs: SIG_FILT_EQ_* by their _native.FILT_TYPES names"""
        band_pass = 'eqbp'
        notch = 'eqnotch'
        all_pass = 'eqap'
        peaking = 'eqpeak'
        low_shelf = 'eqls'
        high_shelf = 'eqhs'

        def __str__(self) -> str:
            return str(self.value)

        @property
        def is_band(self) -> bool:
            return False

        @property
        def has_gain(self) -> bool:
            return self.value in _native.EQ_GAIN_TYPES

    def gain_port(self):
        """the `gain` port of the three gain classes, None for the others"""
        return getattr(self, 'gain', None) if self.type().has_gain else None

    def _eval(self, request: Request) -> torch.Tensor:
        hertz = as_control(self.cutoff.forward_at_block_rate(request))
        src = self.resonance.sig
        q = None if src is None or not src.get_state().enabled else as_control(self.resonance.forward_at_block_rate(request))
        port_ = self.gain_port()
        gain = None
        if port_ is not None and port_.sig is not None and port_.sig.get_state().enabled:
            gain = as_control(port_.forward_at_block_rate(request))
        return self._filter(request, hertz, resonant=True, resonance=q, equaliser=str(self.type()), gain=gain)


class ResonantBandPass(EqFilter):
    """`EqFilter` with b = (d*k, 0, -d*k) * nrm: the band-pass whose peak is 0 dB at every q"""

    def type(self) -> EqFilter.Type:
        return self.Type.band_pass


class Notch(EqFilter):
    """`EqFilter` with b = (1 + k*k, 2*(k*k - 1), 1 + k*k) * nrm: a null at the cutoff, unity gain away from it"""

    def type(self) -> EqFilter.Type:
        return self.Type.notch


class AllPass(EqFilter):
    """`EqFilter` with b = (a2, a1, 1) (the denominator reversed): unit magnitude, a phase turn of 2 pi around the cutoff"""

    def type(self) -> EqFilter.Type:
        return self.Type.all_pass


class GainEqFilter(EqFilter, abc.ABC):
    """the `EqFilter` classes with a `gain` port (dB, block rate; unplugged: 0 dB)"""
    gain: Receiver.BoundPort = port('gain')


class Peaking(GainEqFilter):
    """`EqFilter` with a bell of `gain` dB at the cutoff, q wide; at 0 dB b = a, the input"""

    def type(self) -> EqFilter.Type:
        return self.Type.peaking


class LowShelf(GainEqFilter):
    """`EqFilter` that lifts (or cuts) what lies below the cutoff by `gain` dB; the cutoff is the shelf's midpoint"""

    def type(self) -> EqFilter.Type:
        return self.Type.low_shelf


class HighShelf(GainEqFilter):
    """`EqFilter` that lifts (or cuts) what lies above the cutoff by `gain` dB; the cutoff is the shelf's midpoint"""

    def type(self) -> EqFilter.Type:
        return self.Type.high_shelf


def _validate_poles(instance, attribute, new_value):
    if isinstance(new_value, (bool, np.bool_)) or not isinstance(new_value, (int, np.integer)) or not 1 <= new_value <= 4:
        raise BadStateValue(instance, attribute.name, new_value, 'must be an integer 1, 2, 3 or 4: the output tap, 6 dB/oct per pole')


class Ladder(fx.CritFilter):
    """4-pole transistor-ladder low-pass, 24 dB/oct: four one-pole low-passes in series with the resonance fed back around all four, up
    to self-oscillation, and a saturator in the loop -- the synthesiser filter, which two `ResonantLowPass` in series are not (they give
    the slope, neither the global feedback nor the drive).  Ports: `input` at frame rate; `cutoff` (Hz), `resonance` (the feedback k,
    dimensionless) and `drive` at block rate, read once per block at the block's position like every control.  State: `poles` in
    {1, 2, 3, 4}, default 4, the output tap: 6, 12, 18 or 24 dB/oct (validated on set).  Per voice and block, in float64, the input
    widened exactly, the states s1..s4 = 0 at the window's first row:
        wn = clip(cutoff / (rate / 2), 0, 1)                                (as fx.py:99-102; an error unless 0 < wn < 1, NaN too)
        g  = tan(pi * wn / 2);  G = g / (1 + g);  H = 1 - G
        k  = clip(resonance, 0, 4)
        d  = max(drive, 0)
        c  = 1 / (1 + k * ((G*G) * (G*G)))
        per row:
            S = H * (((s1*G + s2)*G + s3)*G + s4)                           (what the four states put on the output with zero input)
            u = (x - k*S) * c                                               (the zero-delay feedback loop solved in closed form)
            if d > 0:  u = tanh(d*u) / d                                    (the saturator at the loop's summing point)
            for j = 1..4:  v = (u - s_j)*G;  y_j = v + s_j;  s_j = y_j + v;  u = y_j
            out = y_poles
    -- the trapezoidal ("TPT") one-pole, four in series, the linear feedback resolved without a unit delay, the non-linearity applied
    after the solve -- over `CritFilter._filter`'s window: zero state over [<= 100 context rows | block] (kernel: sig_ladder_coldstart,
    which multiplies by a rounded 1 / d where this divides; restated in numpy by tests/ladder_reference.py).  At k = 0, d = 0 it is four
    bilinear one-pole low-passes; the DC gain is 1 / (1 + k); k = 4 is the edge of self-oscillation; the saturator bounds the loop's
    input by 1 / d.
    The controls' edges: an unplugged or disabled `resonance` or `drive` answers the ordinary zeros((1, 1)) of an unplugged port -- no
    feedback, a linear loop (and a kernel without tanh).  k above 4 is 4, below 0 is 0; a k that is NaN or +-inf is an error like a bad
    cutoff: the voice's rows are NaN and `runtime.check_status()` raises the resonant filters' ValueError (SIG_STATUS_BAD_RESONANCE).
    A negative drive (-inf too) is 0; a drive that is NaN or +inf makes the voice's rows NaN and sets no status bit.  `input` of width
    1 broadcasts over the request's channels (wider than 1 but narrower than the request it raises); a plugged `resonance` or `drive`
    narrower than the request raises the IndexError of a narrow `cutoff`, as on `ResonantFilter`.
    Not an `ext.ResonantFilter`, an `fx.SingleCritFilter` or an `fx.DoubleCritFilter`: to the voice program and the fused matchers
    those mean a biquad.  Its type is its own (`Ladder.Type.ladder`, _native.FILT_TYPES['ladder']).  To the batched engine it is a
    filter: request-dependent, min(100, position) history rows, tails between batches, no batch of blocks <= 100 frames over an impure
    input.
    The inherited limit: the resonance rings for far longer than the reference's 100-frame cold start
    lets it.  At k = 3.5 and 48 kHz the share of the impulse response's L1 norm beyond 100 frames is 93 % at 200 Hz, 66 % at 1 kHz,
    29 % at 3 kHz (k = 0: 73 %, 0.1 %, none).  Near k = 4 the ring IS the sound, and 100 frames from zero state truncate it: every block
    hears the first 100 frames of a ring, never a standing self-oscillation.  That is the reference's block semantics, not a defect
    of this node; carried state would lift it, and is out of scope.
    Out of scope: the voice program, the specialised build and the fused kernels (a graph with the node renders one kernel per node;
    the machine's filter slots carry two states each); the node inside a block-rate control path (the batched engine answers
    NotBatchable with the reason and the graph keeps the eager path, which serves frames == 1 in float64); a frame-rate cutoff, k or
    drive; pass-band gain compensation (a `Gain` behind it does that); high-pass and band-pass pole mixes; oversampling; carried
    state."""
    cutoff: Receiver.BoundPort = port('cutoff')
    resonance: Receiver.BoundPort = port('resonance')
    drive: Receiver.BoundPort = port('drive')

    class Type(str, enum.Enum):
        """the node's own filter type: SIG_FILT_LADDER by its _native.FILT_TYPES name"""
        ladder = 'ladder'

        def __str__(self) -> str:
            return str(self.value)

        @property
        def is_band(self) -> bool:
            return False

    @state
    class State(fx.CritFilter.State):
        poles: int = attr.ib(default=4, validator=_validate_poles, on_setattr=attr.setters.validate)

    def type(self) -> 'Ladder.Type':
        return self.Type.ladder

    def control_rows(self, fetch) -> tuple:
        """(resonance, drive): each the port's block-rate reply through `fetch`, or None where nothing enabled is plugged"""
        return tuple(None if bound.sig is None or not bound.sig.get_state().enabled else as_control(fetch(bound))
                     for bound in (self.resonance, self.drive))

    def _eval(self, request: Request) -> torch.Tensor:
        hertz = as_control(self.cutoff.forward_at_block_rate(request))
        k, drive = self.control_rows(lambda bound: bound.forward_at_block_rate(request))
        return self._filter(request, hertz, ladder=(k, drive, int(self._state.poles)))


def _validate_matrix(instance, attribute, new_value):
    if not (isinstance(new_value, np.ndarray) and new_value.shape == (64, 64)):
        raise BadStateValue(instance, attribute.name, new_value, 'must be a (64, 64) array')


class MixMatrix(BlockCachingEmitter, Receiver):
    """Dense 64x64 mix of every group of 64 consecutive voices:
    `out[n, 64g:64g+64] = input[n, 64g:64g+64] @ matrix` (float32, exact-f32 MFMA; sig_mix_matrix).
    Groups must not straddle a GPU shard."""
    input: Receiver.BoundPort = port('input')

    @state
    class State(BlockCachingEmitter.State):
        matrix: np.ndarray = attr.ib(factory=lambda: np.eye(64), validator=_validate_matrix,
                                     on_setattr=attr.setters.validate)

    def __init__(self):
        super().__init__()
        self._resident = ResidentCopy(np.float32)

    @classmethod
    def flags(cls) -> SignalFlags:
        return super().flags() | SignalFlags.EFFECT

    @property
    def channels(self) -> int:
        return self.input.channels

    def resident_matrix(self) -> torch.Tensor:
        return self._resident.of(self._state.matrix)

    def _eval(self, request: Request) -> torch.Tensor:
        x = self.input.forward(request)
        if x.shape[1] % 64:
            raise ValueError(f'MixMatrix needs a multiple of 64 voices, got {x.shape[1]}')
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.to(torch.float32).contiguous()
        return _native.mix_matrix(x, self.resident_matrix(), torch.empty_like(x))


class Tap(PassThroughResult):
    """Stand-in for the reference's side-effect taps (vis.Wave / vis.Spec / files.FileWriter): forwards its
    input unchanged, enabled or not; the original class name and state are kept for round-tripping."""

    def __init__(self, cls_name: str = '', **state):
        super().__init__()
        self.original_cls_name = cls_name
        self.original_state = state

    @classmethod
    def flags(cls) -> SignalFlags:
        return super().flags() | SignalFlags.VIS

    def _eval(self, request: Request) -> torch.Tensor:
        return self.input.forward(request)
