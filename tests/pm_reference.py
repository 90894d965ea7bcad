"""The phase-modulation oscillators of signals_amd/chain/ext.py (PMSine / PMSquare / PMSawtooth / PMTriangle) restated in numpy
on oracle.chain_ref's own functions, for the tests: `hertz`, `phase`, `index` are read at block rate, `mod` at frame rate,

    t = (frame_range / rate * hertz + phase) + index * mod        out = osc_wave(kind, t)

As an oracle Node it takes part in render_stream's cache and context semantics, so graphs with filters around it render as the
reference's pull protocol would."""
import numpy as np

from oracle import chain_ref as R

SLOPE = {'Sine': 2 * np.pi, 'Triangle': 4.0, 'Sawtooth': 2.0, 'Square': 0.0}     # the waveforms' largest slope per cycle
JUMPS = {'Sine': (), 'Triangle': (), 'Sawtooth': (0.5,), 'Square': (0.0, 0.5)}  # phases frac(t) at which a waveform jumps by 2


def pm_cycles(position, frames, rate, hertz, phase, index, mod):
    return R.osc_cycles(position, frames, rate, hertz, phase) + index * mod


class PMOsc(R.Node):
    def __init__(self, kind, hertz=None, phase=None, index=None, mod=None):
        super().__init__(hertz=hertz, phase=phase, index=index, mod=mod)
        self.kind = kind
        self.trace = {}                                  # (position, frames) -> the phase t of that evaluation

    def eval(self, position, frames, channels, rate):
        phase = self._ctrl('phase', position, channels, rate)
        hertz = self._ctrl('hertz', position, channels, rate)
        index = self._ctrl('index', position, channels, rate)
        mod = self._req('mod', position, frames, channels, rate)
        t = pm_cycles(position, frames, rate, hertz, phase, index, mod)
        self.trace[(position, frames)] = t
        return R.osc_wave(self.kind, t)

    def cycles(self, position, frames, blocks):
        """the phases of `blocks` consecutive blocks rendered before (render_stream), as one array; a block the cache served
        from a longer reply (chain_ref.Node.respond) is cut from the first evaluation that contains it"""
        def block(p):
            for (q, f), t in self.trace.items():
                if q <= p and p + frames <= q + f:
                    return t[p - q:p - q + frames]
            raise KeyError((p, frames))
        return np.concatenate([block(position + b * frames) for b in range(blocks)])


class Given(R.Node):
    """rows rendered elsewhere (the float32 modulator a per-node GPU route materialises), answered by position"""
    cached = False

    def __init__(self, rows, position):
        super().__init__()
        self.rows, self.position = np.asarray(rows, dtype=np.float64), position

    def eval(self, position, frames, channels, rate):
        start = position - self.position
        assert 0 <= start and start + frames <= self.rows.shape[0], (position, frames)
        return self.rows[start:start + frames, :channels]


def near_jump(kind, t, band=1e-5):
    """mask of the samples whose phase frac(t) lies within `band` of a jump of the waveform"""
    f = np.mod(t, 1.0)
    mask = np.zeros(t.shape, dtype=bool)
    for j in JUMPS[kind]:
        d = np.abs(f - j)
        mask |= np.minimum(d, 1.0 - d) <= band
    return mask
