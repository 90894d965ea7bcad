"""The generator of the random graphs over the WHOLE node set (tests/test_random_ext_graphs_host.py, tests/test_gpu_random_ext_graphs.py):
`Builder(seed).build()` returns fresh objects at every call and the same graph for the same seed -- the GPU node graph, the matching
oracle graph (oracle.chain_ref plus the committed restatements of the extension families) and a description of the graph that the
census and the tolerance need without rendering anything.

    sources      Sine / Square / Sawtooth / Triangle, PMSine / PMSawtooth (mod: another audio sub-graph), Wavetable (T = 64, W = 2),
                 UnisonSawtooth (3 copies), BlepSquare / BlepSawtooth, SyncSawtooth / SyncSquare, Sampler (an 800-frame burst table,
                 one-shot and looped, triggers inside the rendered windows), White
    history      LowPass / HighPass, ResonantLowPass / ResonantHighPass, Peaking, LowShelf / HighShelf, Notch, AllPass,
                 ResonantBandPass, BandPass / BandStop, Delay (1, 3 and 16 taps)
    memoryless   Gain, Mix, RingMod, Shaper (two tanh curves), RingMod(x, ADSR) with every stage boundary inside the windows
    sink         half the seeds end in a SumBus, with and without gains

Depth 3, V = 8 voices, every parameter row (1, V) or (1, 1), finished sub-graphs kept in a pool and reused (diamonds), control ports
on a Fixed row or on the block-rate LFO of tests/test_gpu_random_graphs.py (`Mix(Gain(Sine | Triangle, depth), centre, 0.5)`, which
stays inside the port's range), no extension node inside a control path.  A free draw of 32 graphs of this depth holds some 180
nodes of 22 families and leaves families out of the census whatever the weights, so the top of every graph is laid out
(`Builder.diamond`): Mix | RingMod(reader(X), Mix | RingMod(X, Y)), the families of X and Y going round the list with the seed, X
shared between a history reader and a plain one; which reader, every row, width, control, kind and what X and Y read are drawn.  A LowPass ... ResonantBandPass indexes its control rows and
its input per channel (fx.py:99), so those are drawn V wide; a Delay, a Shaper, an element-wise node and a PM carrier broadcast a
one-column input.  Amp is left out: its power law has no gain bound.

The tolerance.  One kernel per node stores every node's output as float32, so every node adds one rounding of the graph's scale and
passes on its inputs' error times its gain.  `G` is the largest product of the gain bounds g(node) along a path from the root to a
leaf; a graph is held to 1e-6 * G * max(1, max |oracle|), the families' bar (tests/test_gpu_mixed.py: tolerance) times G:

    ResonantLowPass / HighPass      max(1, q)
    Peaking, LowShelf, HighShelf    max(1, 10 ** (dB / 20))
    Notch, AllPass, ResonantBandPass  the peak of |H| on a 4096-point grid (eq_reference.eq_sos with the node's rows), at least 1
    Shaper                          max(1, L), L = shaper_reference.lipschitz of its table
    Delay                           max(1, sum |g_u|)
    everything else                 1

For a modulated parameter the bound is the largest over CONTROL_POSITIONS, every position a control can be read at by the renders of
RENDERS and SHORT: the blocks' own positions, the position behind the last block (the `after` request), 100 frames in front of any of
them (the `before` request of short blocks) and the history blocks 100, 200, ... frames in front of a fresh start.  The ranges keep it
small: q in [0.5, 2], equaliser gain in [-12, +6] dB, L <= 2, sum |g_u| <= 1, time in 0 .. 2 ms, cutoffs in 300 .. 6000 Hz.

A draw whose oracle rows are not finite, stay below 0.01 or whose G exceeds 64 is drawn again with the next attempt number: the
attempt is part of the seed's definition (`Builder.attempt`), found once per process and seed on the CPU."""
import collections
import random

import numpy as np

from helpers import OSC, RATE, fix, mkosc
import blep_reference as BR
import delay_reference as DR
import eq_reference as ER
import pm_reference as PR
import resonant_reference as RR
import sampler_reference as SaR
import shaper_reference as SR
import sync_reference as SyR
import unison_reference as UR
import wavetable_reference as WR

V = 8
CONTEXT = 100
SEEDS = range(32)
RENDERS = ((0, 128, (1, 2)), (1000, 256, (2, 1)), (37, 128, (2,)))           # (position, N, batches)
SHORT = (0, 64, (3, 2, 1))                                                    # the program route's short-block render
G_MAX = 64.0

WT_TABLE = np.concatenate([WR.band_limited_saw(64, 9), np.sin(2 * np.pi * np.arange(64) / 64)[:, None] ** 3], axis=1)   # (64, 2)
SAMPLE_TABLE = SaR.burst(800, 2, seed=5)                                      # (800, 2)
LOOP = (120, 680)
EQ_KINDS = {'Peaking': 'peak', 'LowShelf': 'ls', 'HighShelf': 'hs', 'Notch': 'notch', 'AllPass': 'ap', 'ResonantBandPass': 'bp'}
SOURCES = ('Osc', 'PM', 'Wavetable', 'Unison', 'Blep', 'Sync', 'Sampler', 'White')
READERS = ('Crit', 'Resonant', 'Peaking', 'Shelf', 'Notch', 'AllPass', 'ResonantBandPass', 'Band', 'Delay')
MEMORYLESS = ('Gain', 'Shaper', 'Env', 'Mix', 'RingMod')
FEATURED = SOURCES + READERS + MEMORYLESS                                     # (Builder.diamond)
FAMILIES = FEATURED + ('SumBus',)
NO_CONTROL = ('White', 'Band', 'RingMod', 'Env', 'SumBus')                    # families without a port that is ever modulated here
WEIGHT = {'Osc': 3.0, 'Mix': 3.0, 'RingMod': 3.0, 'Env': 1.5, **{f: 1.5 for f in READERS}}   # (two audio inputs make the graphs branch)
SALT = 2                                                                      # of every seed's generators: the first one with which every kind of every family is drawn (the host test's census)
LEAF = 0.05                                                                   # how likely a sub-graph above the last level is a bare source
ALWAYS_WIDE = tuple(f for f in READERS if f != 'Delay') + ('White',)

Entry = collections.namedtuple('Entry', 'family depth reads_history modulated width kind shared_mixed narrow_under_wide inputs')
Graph = collections.namedtuple('Graph', 'node ref channels entries G')
Control = collections.namedtuple('Control', 'gpu ref modulated width at')
Sub = collections.namedtuple('Sub', 'gpu ref index')


def control_positions():
    out = set()
    for pos, N, batches in RENDERS + (SHORT,):
        blocks = [pos + b * N for b in range(sum(batches) + 1)]
        out.update(blocks)
        out.update(p - CONTEXT for p in blocks if p >= CONTEXT)
        q = pos
        while q > 0:
            q = max(q - CONTEXT, 0)
            out.add(q)
    return tuple(sorted(out))


CONTROL_POSITIONS = control_positions()


def peak_response(sos) -> float:
    """max |H| of one second-order section on a 4096-point grid over [0, pi]"""
    z = np.exp(-1j * np.linspace(0.0, np.pi, 4096))
    b0, b1, b2, a0, a1, a2 = sos[0]
    return float(np.abs((b0 + b1 * z + b2 * z * z) / (a0 + a1 * z + a2 * z * z)).max())


_ATTEMPTS: dict = {}


class Builder:
    """builds the SAME random graph every time it is called with the same seed (fresh node objects on both sides)"""

    def __init__(self, seed):
        self.seed = seed

    @property
    def attempt(self) -> int:
        """the first attempt number whose draw is usable (module docstring), found on the CPU from the oracle graph alone"""
        if self.seed not in _ATTEMPTS:
            attempt = 0
            while not self.usable(attempt):
                attempt += 1
            _ATTEMPTS[self.seed] = attempt
        return _ATTEMPTS[self.seed]

    def build(self, gpu: bool = True) -> Graph:
        """Graph(node, ref, channels, entries, G); `gpu=False` leaves the GPU node graph out (node is None)"""
        return self._draw(self.attempt, gpu)

    def usable(self, attempt: int) -> bool:
        if not self._draw(attempt, gpu=False).G <= G_MAX:
            return False
        for pos, N, batches in RENDERS + (SHORT,):
            rows = oracle_rows(self._draw(attempt, gpu=False), pos, N, sum(batches))     # (a fresh oracle graph per render: no cached blocks)
            if not np.isfinite(rows).all() or not np.abs(rows).max() > 0.01:
                return False
        return True

    # ---------------------------------------------------------------------------------------------- the draw
    def _draw(self, attempt: int, gpu: bool) -> Graph:
        from oracle import chain_ref as R
        self.R, self.gpu = R, gpu
        if gpu:
            from signals_amd.chain import ext, fx, noise
            self.fx, self.ext, self.noise = fx, ext, noise
        self.rng = random.Random((SALT * 1000 + self.seed) * 1000 + attempt)
        self.np = np.random.default_rng([SALT, self.seed, attempt])
        self.pool, self.nodes, self.given = [], [], []
        self.narrow = self.swept = self.widen = False
        top = self.diamond()
        node, ref, channels = top.gpu, top.ref, V
        if self.rng.random() < 0.5:
            gains = self.np.uniform(-1, 1, (2, V)) if self.rng.random() < 0.5 else None
            if gpu:
                node = self.ext.SumBus(); node.input = top.gpu
                if gains is not None:
                    node.get_state().gains = gains
            ref = R.SumBus(top.ref, gains)
            ref.in_channels = V
            channels = 1 if gains is None else 2
            self.note('SumBus', 'SumBus', 3, channels, False, [top.index], reader=False)
        entries, G = self.describe()
        return Graph(node, ref, channels, entries, G)

    def family(self, family, depth, wide) -> Sub:
        if family in SOURCES:
            sub = self.source(family, depth, wide)
        else:
            sub = self.filter(family, depth) if family in READERS else self.memoryless(family, depth, wide)
        self.pool.append(sub)
        return sub

    def diamond(self) -> Sub:
        """every seed's graph: Mix | RingMod(reader(X), Mix | RingMod(X, Y)), X and Y sub-graphs one level deep whose families go round
        FEATURED with the seed (X: seed mod 22, Y: seed + 10 mod 22; Mix and RingMod, the last two, are every graph's top), so that
        every family is in three seeds at least.  X is read with 100 history rows by a filter or a Delay on one side and with none on
        the other; its first control port is on the LFO where it has one; where the family can be one column wide it is (and everything
        below it), under a Delay with a per-voice `time`.  Everything else is drawn: which reader, every row, width and control, what
        X and Y read (sources, or finished sub-graphs from the pool), Y as a whole"""
        fx, fy = FEATURED[self.seed % len(FEATURED)], FEATURED[(self.seed + 10) % len(FEATURED)]
        self.narrow, self.swept = fx not in ALWAYS_WIDE, fx not in NO_CONTROL
        x = self.family(fx, 1, not self.narrow)
        narrow, self.narrow, self.swept = self.narrow, False, False
        self.widen = narrow                                                   # (the Delay's `time`: V columns)
        self.given = [x]
        over = self.filter('Delay' if narrow else self.rng.choices(READERS, [WEIGHT.get(f, 1.0) for f in READERS])[0], 2)
        self.pool.append(over)
        y = self.family(fy, 1, False)
        self.given = [x, y]
        plain = self.memoryless(self.rng.choice(['Mix', 'RingMod']), 2, False)     # the reader that asks X for no history
        self.pool.append(plain)
        self.given = [over, plain]
        return self.memoryless(self.rng.choice(['Mix', 'RingMod']), 3, True)

    def note(self, family, kind, depth, width, modulated, inputs, reader, g=1.0) -> int:
        self.nodes.append(dict(family=family, kind=kind, depth=3 - depth, width=width, modulated=modulated, inputs=list(inputs),
                               reader=reader, g=max(1.0, float(g))))
        return len(self.nodes) - 1

    def describe(self):
        """(entries, G): how many history rows every node is read with -- `_Batch._require`'s rule at a position >= 100: a filter or a
        Delay asks its input for 100, a modulated node for none (its own history comes from its tail), every other node for what it is
        asked for itself -- and the gain bound of the worst path"""
        nodes = self.nodes
        root = len(nodes) - 1
        need = [-1] * len(nodes)

        def down(i):
            return CONTEXT if nodes[i]['reader'] else 0 if nodes[i]['modulated'] else need[i]

        def require(i, hist):
            if need[i] >= hist:
                return
            need[i] = hist
            for j in nodes[i]['inputs']:
                require(j, down(i))
        require(root, 0)
        asks = [[] for _ in nodes]                                            # per node: (rows asked for, by whom) of every reader
        asks[root].append((0, None))
        for i, n in enumerate(nodes):
            for j in n['inputs']:
                asks[j].append((down(i), i))
        gain = {}

        def path(i):
            if i not in gain:
                gain[i] = nodes[i]['g'] * max([1.0] + [path(j) for j in nodes[i]['inputs']])
            return gain[i]
        entries = []
        for i, n in enumerate(nodes):
            hists = {h for h, _ in asks[i]}
            readers = {by for _, by in asks[i] if by is not None}
            entries.append(Entry(n['family'], n['depth'], max(hists) > 0, n['modulated'], n['width'], n['kind'],
                                 len(readers) > 1 and max(hists) > 0 and min(hists) == 0,
                                 n['width'] == 1 and any(nodes[r]['width'] == V for r in readers), tuple(n['inputs'])))
        return tuple(entries), path(root)

    # ---------------------------------------------------------------------------------------------- rows and controls
    def row(self, lo, hi, wide=True):
        return self.np.uniform(lo, hi, (1, V if wide else 1))

    def coin(self, p=0.5):
        return self.rng.random() < p

    def wcoin(self, p=0.6):
        """whether a row is V wide (drawn either way; never inside a featured one-column sub-graph)"""
        return self.coin(p) and not self.narrow

    def fixed(self, value) -> Control:
        value = np.array(value, ndmin=2, dtype=np.float64)
        return Control(fix(value) if self.gpu else None, self.R.Fixed(value), False, value.shape[1], lambda p: value)

    def control(self, lo, hi, wide=None, p=0.3) -> Control:
        """a control input: usually a Fixed row, sometimes the block-rate LFO centre + 0.1 (hi - lo) wave, which stays inside
        [lo + 0.2 (hi - lo), hi - 0.2 (hi - lo)]; `wide`: True / False / None (drawn)"""
        R = self.R
        wide = self.wcoin() if wide is None else wide
        wide, self.widen = wide or self.widen, False
        swept, self.swept = self.coin(p) or self.swept, False
        if not swept:
            return self.fixed(self.row(lo, hi, wide))
        kind = self.rng.choice(['Sine', 'Triangle'])
        hz = self.row(0.5, 8.0, wide=wide and self.coin())
        depth = np.array([[0.4 * (hi - lo) / 2]])
        centre = self.row(lo + 0.3 * (hi - lo), hi - 0.3 * (hi - lo), wide) * 2
        mid = None
        if self.gpu:
            g = self.fx.Gain(); g.left = mkosc(kind, hz); g.right = fix(depth)
            mid = self.fx.Mix(); mid.left = g; mid.right = fix(centre); mid.mix = fix([[0.5]])
        ref = R.Binary('Mix', R.Binary('Gain', R.Osc(kind, R.Fixed(hz)), R.Fixed(depth)), R.Fixed(centre), R.Fixed([[0.5]]))
        at = lambda q: R.mix(R.gain(R.osc(kind, q, 1, RATE, hz), depth), centre, np.array([[0.5]]))
        return Control(mid, ref, True, max(hz.shape[1], centre.shape[1]), at)

    @staticmethod
    def largest(f, *controls) -> float:
        """max of f(rows...) over the positions the controls are read at (one evaluation where none is modulated)"""
        positions = CONTROL_POSITIONS if any(c.modulated for c in controls) else (0,)
        return max(float(np.max(f(*(np.broadcast_to(c.at(q), (1, V)) for c in controls)))) for q in positions)

    # ---------------------------------------------------------------------------------------------- audio
    def pick(self, wide, reader):
        """a finished sub-graph from the pool, or None: one that is wide enough, three times as likely where its readers so far are
        all of the other kind (a filter or a Delay on one side, a reader that asks for no history on the other)"""
        fit = [s for s in self.pool if not wide or self.nodes[s.index]['width'] == V]
        if not fit:
            return None
        weights = []
        for s in fit:
            kinds = {self.nodes[i]['reader'] for i, n in enumerate(self.nodes) if s.index in n['inputs']}
            weights.append(3.0 if kinds == {not reader} else 1.0)
        return self.rng.choices(fit, weights)[0]

    def audio(self, depth, wide, reader, share=None) -> Sub:
        """a sub-graph `depth` levels deep at most; `wide`: it must answer V columns; `reader`: a filter or a Delay will read it;
        `share`: how likely it is a sub-graph from the pool (default: 0.4 for a leaf, 0.15 above)"""
        r = self.rng
        if self.given:
            return self.given.pop(0)
        leaf = depth == 0 or (depth < 3 and r.random() < LEAF)
        shared = self.pick(wide, reader) if depth < 3 and r.random() < (share if share is not None else 0.4 if leaf else 0.15) else None
        if shared is not None:
            return shared
        if leaf:
            fit = [f for f in SOURCES if not (self.narrow and f in ALWAYS_WIDE)]
            sub = self.source(r.choices(fit, [WEIGHT.get(f, 1.0) for f in fit])[0], depth, wide)
        else:
            family = r.choices(READERS + MEMORYLESS, [WEIGHT.get(f, 1.0) for f in READERS + MEMORYLESS])[0]
            sub = self.filter(family, depth) if family in READERS else self.memoryless(family, depth, wide)
        self.pool.append(sub)
        return sub

    def source(self, family, depth, wide) -> Sub:
        R, r, gpu = self.R, self.rng, self.gpu
        first = True if wide else None                                        # the first row decides where V columns are asked for
        if family not in ('Sampler', 'White'):
            hertz = self.control(100, 900, first, p=1.0) if self.swept or self.coin(0.15) else self.fixed(self.row(55, 1760, self.wcoin() if first is None else True))
            phase = self.fixed(self.row(0, 1, self.wcoin()))
        inputs, node = [], None
        if family == 'Osc':
            kind = r.choice(['Sine', 'Square', 'Sawtooth', 'Triangle'])
            controls = [hertz, phase]
            if gpu:
                node = OSC[kind](); node.hertz = hertz.gpu; node.phase = phase.gpu
            ref = R.Osc(kind, hertz.ref, phase.ref)
        elif family == 'PM':
            kind = r.choice(['PMSine', 'PMSawtooth'])
            index = self.control(0.0, 0.15, p=0.2)
            mod = self.audio(depth - 1, False, False) if depth > 0 else self.source('Osc', 0, False)
            controls, inputs = [hertz, phase, index], [mod.index]
            if gpu:
                node = getattr(self.ext, kind)(); node.hertz = hertz.gpu; node.phase = phase.gpu; node.index = index.gpu; node.mod = mod.gpu
            ref = PR.PMOsc(kind[2:], hertz.ref, phase.ref, index.ref, mod.ref)
        elif family == 'Wavetable':
            kind = 'Wavetable'
            select = self.control(0.0, 2.0, p=0.2)
            controls = [hertz, phase, select]
            if gpu:
                node = self.ext.Wavetable(); node.get_state().table = WT_TABLE
                node.hertz = hertz.gpu; node.phase = phase.gpu; node.select = select.gpu
            ref = WR.oracle_node()(WT_TABLE, hertz.ref, phase.ref, select.ref)
        elif family == 'Unison':
            kind = 'UnisonSawtooth'
            copies = np.stack([self.np.uniform(-0.12, 0.12, 3), self.np.uniform(0, 1, 3)], axis=1)
            spread = self.control(0.0, 1.0, p=0.2)
            controls = [hertz, phase, spread]
            if gpu:
                node = self.ext.UnisonSawtooth(); node.get_state().copies = copies
                node.hertz = hertz.gpu; node.phase = phase.gpu; node.spread = spread.gpu
            ref = UR.UnisonOsc('Sawtooth', copies, hertz.ref, phase.ref, spread.ref)
        elif family == 'Blep':
            kind = r.choice(['BlepSquare', 'BlepSawtooth'])
            controls = [hertz, phase]
            if gpu:
                node = getattr(self.ext, kind)(); node.hertz = hertz.gpu; node.phase = phase.gpu
            ref = BR.BlepOsc(kind[4:], BR.default_copies(), hertz.ref, phase.ref)
        elif family == 'Sync':
            kind = r.choice(['SyncSawtooth', 'SyncSquare'])
            ratio = self.control(1.0, 5.0, p=0.2)
            controls = [hertz, phase, ratio]
            if gpu:
                node = getattr(self.ext, kind)(); node.hertz = hertz.gpu; node.phase = phase.gpu; node.ratio = ratio.gpu
            ref = SyR.SyncOsc(kind[4:], SyR.default_copies(), hertz.ref, phase.ref, None, ratio.ref)
        elif family == 'Sampler':
            loop = LOOP if self.coin() else (0, 0)
            kind = 'Sampler,loop' if loop[1] else 'Sampler,one-shot'
            ratio = self.control(0.5, 2.0, first, p=0.2)
            offset, select = self.fixed(self.row(0, 20, self.wcoin())), self.fixed(self.row(0, 2, self.wcoin()))
            gate_on = self.fixed(self.row(0.0, 0.01, self.wcoin(0.7)))         # triggers at frames 0 .. 480: inside the first windows
            controls = [ratio, offset, gate_on, select]
            if gpu:
                node = self.ext.Sampler(); st = node.get_state(); st.table = SAMPLE_TABLE
                st.loop_start, st.loop_end = loop
                node.ratio = ratio.gpu; node.offset = offset.gpu; node.gate_on = gate_on.gpu; node.select = select.gpu
            ref = SaR.oracle_node()(SAMPLE_TABLE, ratio.ref, offset.ref, gate_on.ref, select.ref, *loop)
        elif family == 'White':
            kind, seed = 'White', r.randrange(2 ** 32)
            controls = [self.fixed(np.zeros((1, V)))]                         # (V columns whatever is asked: its `channels` state)
            if gpu:
                node = self.noise.White(); node.get_state().channels = V; node.get_state().seed = seed
            ref = R.White(seed, V)
        else:
            raise KeyError(family)
        width = max([c.width for c in controls] + [self.nodes[i]['width'] for i in inputs])
        return Sub(node, ref, self.note(family, kind, depth, width, any(c.modulated for c in controls), inputs, reader=False))

    def filter(self, family, depth) -> Sub:
        """a history reader: V wide, its control rows too (but a Delay's)"""
        R, r, gpu = self.R, self.rng, self.gpu
        node, g = None, 1.0
        if family == 'Delay':
            U = r.choice([1, 3, 16])
            gains = self.np.uniform(-1, 1, U)
            gains *= self.np.uniform(0.5, 1.0) / np.abs(gains).sum()           # sum |g_u| in [0.5, 1]
            taps = np.stack([np.concatenate([[1.0], self.np.uniform(0.1, 1.0, U - 1)]), gains], axis=1)
            time = self.control(0.0, 0.002)
            src = self.audio(depth - 1, False, True)
            if gpu:
                node = self.ext.Delay(); node.get_state().taps = taps; node.input = src.gpu; node.time = time.gpu
            ref = DR.oracle_node()(src.ref, time.ref, taps)
            width = max(time.width, self.nodes[src.index]['width'])
            return Sub(node, ref, self.note('Delay', f'Delay,{U}', depth, width, time.modulated, [src.index], reader=True,
                                            g=np.abs(gains).sum()))
        swept, self.swept = self.swept, False                                 # (a featured filter's own control, not its input's)
        src = self.audio(depth - 1, True, True)
        self.swept = swept
        controls = []
        if family == 'Crit':
            kind = r.choice(['LowPass', 'HighPass'])
            cutoff = self.control(300, 6000, True)
            controls = [cutoff]
            if gpu:
                node = getattr(self.fx, kind)(); node.input = src.gpu; node.cutoff = cutoff.gpu
            ref = R.Filter({'LowPass': 'lp', 'HighPass': 'hp'}[kind], src.ref, cutoff.ref)
        elif family == 'Band':
            kind = r.choice(['BandPass', 'BandStop'])
            lo = self.row(100, 2000)
            low, high = self.fixed(lo), self.fixed(lo * self.np.uniform(1.5, 4.0, (1, V)))
            if gpu:
                node = getattr(self.fx, kind)(); node.input = src.gpu; node.low = low.gpu; node.high = high.gpu
            ref = R.BandFilter({'BandPass': 'bp', 'BandStop': 'bs'}[kind], src.ref, low.ref, high.ref)
        elif family == 'Resonant':
            kind = r.choice(['ResonantLowPass', 'ResonantHighPass'])
            cutoff, q = self.control(300, 6000, True), self.control(0.5, 2.0, True)
            controls = [cutoff, q]
            if gpu:
                node = getattr(self.ext, kind)(); node.input = src.gpu; node.cutoff = cutoff.gpu; node.resonance = q.gpu
            ref = RR.oracle_node()({'ResonantLowPass': 'lp', 'ResonantHighPass': 'hp'}[kind], src.ref, cutoff.ref, q.ref)
            g = self.largest(lambda q: q, q)
        else:
            kind = r.choice(['LowShelf', 'HighShelf']) if family == 'Shelf' else family
            cutoff, q = self.control(300, 6000, True), self.control(0.5, 2.0, True)
            controls = [cutoff, q]
            gain = self.control(-12.0, 6.0, True) if kind in ('Peaking', 'LowShelf', 'HighShelf') else None
            if gpu:
                node = getattr(self.ext, kind)(); node.input = src.gpu; node.cutoff = cutoff.gpu; node.resonance = q.gpu
            if gain is not None:
                controls.append(gain)
                if gpu:
                    node.gain = gain.gpu
                g = self.largest(lambda db: 10.0 ** (db / 20.0), gain)
            else:
                g = self.largest(lambda c, q: [peak_response(ER.eq_sos(ER.scaled(c[0, v], RATE), q[0, v], None, EQ_KINDS[kind]))
                                               for v in range(V)], cutoff, q)
            ref = ER.oracle_node()(EQ_KINDS[kind], src.ref, cutoff.ref, q.ref, None if gain is None else gain.ref)
        return Sub(node, ref, self.note(family, kind, depth, V, any(c.modulated for c in controls), [src.index], reader=True, g=g))

    def memoryless(self, family, depth, wide) -> Sub:
        R, r, gpu = self.R, self.rng, self.gpu
        node, g, controls = None, 1.0, []
        if family == 'Gain':
            right = self.control(0.1, 1.0)
            left = self.audio(depth - 1, wide and right.width == 1, False)
            controls, inputs = [right], [left.index]
            if gpu:
                node = self.fx.Gain(); node.left = left.gpu; node.right = right.gpu
            ref = R.Binary('Gain', left.ref, right.ref)
        elif family == 'Mix':
            mix = self.control(0.1, 0.9)
            left = self.audio(depth - 1, wide and mix.width == 1, False)
            right = self.audio(depth - 1, False, False, share=0.5)
            controls, inputs = [mix], [left.index, right.index]
            if gpu:
                node = self.fx.Mix(); node.left = left.gpu; node.right = right.gpu; node.mix = mix.gpu
            ref = R.Binary('Mix', left.ref, right.ref, mix.ref)
        elif family == 'RingMod':
            left, right = self.audio(depth - 1, wide, False), self.audio(depth - 1, False, False, share=0.5)
            inputs = [left.index, right.index]
            if gpu:
                node = self.fx.RingMod(); node.left = left.gpu; node.right = right.gpu
            ref = R.Binary('RingMod', left.ref, right.ref)
        elif family == 'Shaper':
            table = np.concatenate([SR.tanh_curve(257, self.np.uniform(0.8, 1.8)), SR.tanh_curve(257, self.np.uniform(0.8, 1.8))], axis=1)
            g = SR.lipschitz(table)
            assert g <= 2.0, g
            select = self.control(0.0, 2.0)
            src = self.audio(depth - 1, wide and select.width == 1, False)
            controls, inputs = [select], [src.index]
            if gpu:
                node = self.ext.Shaper(); node.get_state().table = table; node.input = src.gpu; node.select = select.gpu
            ref = SR.oracle_node()(table, src.ref, select.ref)
        elif family == 'Env':
            # an ADSR whose every stage boundary falls inside the rendered windows (frames 0 .. 1768 at 48 kHz), times a sub-graph
            rows = {name: self.row(lo, hi, wide=self.wcoin(0.8))
                    for name, (lo, hi) in dict(attack=(0.001, 0.008), decay=(0.002, 0.008), sustain=(0.2, 0.9), release=(0.002, 0.01),
                                               gate_on=(0.0, 0.006), gate_off=(0.012, 0.03)).items()}
            env_width = max(v.shape[1] for v in rows.values())
            x = self.audio(depth - 1, wide and env_width == 1, False)
            env_first = self.coin()
            e = self.note('ADSR', 'ADSR', depth - 1, env_width, False, [], reader=False)
            inputs = [e, x.index] if env_first else [x.index, e]
            if gpu:
                env = self.ext.ADSR()
                for name, value in rows.items():
                    setattr(env, name, fix(value))
                node = self.fx.RingMod()
                node.left, node.right = (env, x.gpu) if env_first else (x.gpu, env)
            sides = (R.Adsr(**rows), x.ref) if env_first else (x.ref, R.Adsr(**rows))
            ref = R.Binary('RingMod', *sides)
        else:
            raise KeyError(family)
        width = max([c.width for c in controls] + [self.nodes[i]['width'] for i in inputs])
        return Sub(node, ref, self.note(family, family, depth, width, any(c.modulated for c in controls), inputs, reader=False, g=g))


def oracle_rows(graph: Graph, pos: int, N: int, K: int) -> np.ndarray:
    """float64 (K * N, channels): the oracle's sequential blocks of a FRESH graph"""
    from oracle import chain_ref as R
    return R.render_stream(graph.ref, pos, N, K, graph.channels)


def tolerance(graph: Graph, want: np.ndarray) -> float:
    return 1e-6 * graph.G * max(1.0, float(np.abs(want).max()))
