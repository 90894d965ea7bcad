"""The modal resonator bank (ext.Modal, sig_modal_bank) restated in numpy: the definition of include/signals_amd.h and the node's
docstring, every operation rounded once in float64 in the order written, the modes added in ascending order -- and the same text in
np.longdouble (`dtype=np.longdouble`; the decision which rows sound stays the float64 one), against which the float64 restatement's
own rounding is measured.  Also the kernel cases that
tests/test_modal_host.py and tests/test_gpu_modal.py share.  numpy alone: importable without torch or a GPU.

Two rules stated in the definition's margin are code here: a mode with g == 0 adds exactly 0 (not 0 * sin(mod(inf, 1))), and a `damp`
that is not finite gives NaN on sounding rows like a `hertz` that is not finite (the formula alone would give NaN only at e == 0)."""
import numpy as np

RATE = 48000
RUN = 64                                      # the kernel's run length: rows between two closed-form starts (sig_modal.h kRun)


def table(modes, dtype=np.float64):
    """(W, M, 3) rows (ratio, amplitude, lambda = ln(1000) / t60) as the node uploads them: lambda is computed in float64 on the host
    and is part of the definition's input, so the longdouble twin widens the same float64 values"""
    m = np.array(modes, dtype=np.float64)
    m = m.reshape(-1, m.shape[-2], 3)
    m[..., 2] = np.log(1000.0) / m[..., 2]
    return m.astype(dtype)


def gain_bound(modes) -> float:
    """A: the largest set's sum of |a|"""
    m = np.asarray(modes, dtype=np.float64)
    return float(np.abs(m.reshape(-1, m.shape[-2], 3)[..., 1]).sum(axis=1).max())


def tolerance(modes) -> float:
    return 1e-6 * max(1.0, gain_bound(modes))


def column(select, W: int) -> np.ndarray:
    """clip(floor(select), 0, W - 1), NaN -> 0"""
    s = np.floor(np.asarray(select, dtype=np.float64))
    with np.errstate(invalid='ignore'):
        return np.where(s >= 1.0, np.minimum(s, W - 1.0), 0.0).astype(np.int64)


def modal_rows(modes, frames_abs, hertz, gate_on, damp, select, rate=RATE, dtype=np.float64) -> np.ndarray:
    """the definition for the absolute frames `frames_abs` (N,) and one row of parameters, each (1, V | 1): (N, V) in `dtype`"""
    T = dtype
    tab = table(modes, T)
    W, M, _ = tab.shape
    hz, gate, dmp = (np.asarray(x, dtype=np.float64).astype(T).reshape(1, -1) for x in (hertz, gate_on, damp))
    sel = column(np.asarray(select, dtype=np.float64).reshape(1, -1), W)
    V = max(x.shape[1] for x in (hz, gate, dmp, sel))
    hz, gate, dmp, sel = (np.broadcast_to(x, (1, V)) for x in (hz, gate, dmp, sel))
    two_pi = T(2.0) * (np.arctan(T(1.0)) * T(4.0) if T is np.longdouble else T(np.pi))
    with np.errstate(all='ignore'):
        q = np.asarray(frames_abs, dtype=np.int64).astype(T)[:, None] / T(rate)
        e = q - gate                                                           # (N, V)
        out = np.zeros(e.shape, dtype=T)
        for i in range(M):                                                     # ascending
            r, a, lam = (tab[sel[0], i, c][None, :] for c in range(3))        # (1, V) each
            F = hz * r
            g = np.clip(((T(0.5) * T(rate)) - np.abs(F)) / np.abs(hz), T(0.0), T(1.0))
            c = e * F
            m = np.mod(c, T(1.0))
            k = (lam + dmp) * e
            term = (a * g) * np.exp(-k) * np.sin(two_pi * m)
            out = out + np.where(g == 0, T(0.0), term)
        out = np.where(np.isfinite(hz) & np.isfinite(dmp), out, T(np.nan))
        # which rows sound is the float64 definition's decision in both precisions: a strike exactly on a frame has e == 0 there
        e64 = np.asarray(frames_abs, dtype=np.int64).astype(np.float64)[:, None] / np.float64(rate) - gate.astype(np.float64)
        return np.where(e64 >= 0, out, T(0.0))


def modal(modes, position, frames, hertz, gate_on=0.0, damp=0.0, select=0.0, blocks=1, step=1, rate=RATE, dtype=np.float64) -> np.ndarray:
    """`blocks` blocks of `frames` rows from `position`, row r at frame position + r * step; a parameter with `blocks` rows is read
    per block"""
    rows = [np.array(x, dtype=np.float64, ndmin=2) for x in (hertz, gate_on, damp, select)]
    out = []
    for b in range(blocks):
        n = position + (b * frames + np.arange(frames, dtype=np.int64)) * step
        out.append(modal_rows(modes, n, *(x[b if x.shape[0] > 1 else 0][None, :] for x in rows), rate=rate, dtype=dtype))
    return np.concatenate(out, axis=0)


# ---------------------------------------------------------------------------------------------- the kernel cases
def mode_table(M: int, W: int = 1, seed: int = 0) -> np.ndarray:
    """(W, M, 3): inharmonic ascending ratios from 0.5 up (about i ** 1.1), signed amplitudes that fall off like 1 / i, decay times of a
    second and less; every fifth row of set 0 undamped (t60 = inf)"""
    rng = np.random.default_rng(100 * M + W + seed)
    i = np.arange(1, M + 1, dtype=np.float64)
    ratio = np.sort(i ** 1.1 * rng.uniform(0.9, 1.1, (W, M)), axis=1)
    ratio[:, 0] = 0.5 if M > 1 else 1.0
    amp = rng.uniform(-1.0, 1.0, (W, M)) / i
    t60 = rng.uniform(0.05, 1.5, (W, M)) / np.sqrt(i)
    t60[0, ::5] = np.inf
    return np.stack([ratio, amp, t60], axis=2)


def hertz_mix(voices: int, modes, rate: int = RATE) -> np.ndarray:
    """(1, voices): 0, 55, 440.3, -440.3, a pitch that puts set 0's top mode inside the last |hertz| below half the rate (0 < g < 1), a
    pitch that drops every mode of every set, NaN -- cycled over the voices, random audio pitches past the list"""
    m = np.asarray(modes).reshape(-1, np.asarray(modes).shape[-2], 3)
    top, low = m[0, :, 0].max(), m[..., 0].min()
    special = [0.0, 55.0, 440.3, -440.3, 0.5 * rate / (top + 0.5), 0.5 * rate / low * 1.01, np.nan, 1733.9]
    hz = np.random.default_rng(voices).uniform(30.0, 3000.0, voices)
    for v in range(voices):
        if v % 11 < len(special):
            hz[v] = special[v % 11]
    return hz.reshape(1, voices)


def gate_mix(voices: int, position: int, rows: int, step: int = 1, rate: int = RATE, offset: int = 0) -> np.ndarray:
    """(1, voices) strike times around a stretch of `rows` rows from `position`: 0, -0.5 s, exactly on a frame inside, a quarter of a
    frame past one, inside the last run, one frame after the stretch, 1e6 s, NaN -- cycled with a stride coprime to hertz_mix's, and
    past the list a different strike per voice, before and inside the stretch"""
    last = position + (rows - 1) * step
    inside = position + (rows // 3) * step
    special = [0.0, -0.5, inside / rate, (inside + 0.25) / rate, (last - min(2, rows - 1) * step) / rate, (last + step) / rate, 1e6, np.nan]
    g = (position + np.random.default_rng(voices + offset).uniform(-3.0 * rows, 0.9 * rows, voices) * step) / rate
    for v in range(voices):
        if (v + offset) % 9 < len(special):
            g[v] = special[(v + offset) % 9]
    return g.reshape(1, voices)


def select_mix(voices: int, blocks: int = 1) -> np.ndarray:
    s = np.random.default_rng(voices).uniform(-1.5, 4.5, (blocks, voices))
    special = [-1.0, 0.5, 2.0, 7.0, np.nan]
    for v in range(voices):
        if v % 6 < len(special):
            s[:, v] = special[v % 6]
    return s


def cases() -> list:
    """the kernel cases: dicts of name, modes (W, M, 3), voices, N, K (rows = N * K; parameters with K rows are read per block),
    position, step, hertz, gate_on, damp, select (each (1 | K, V | 1), or None = unplugged)"""
    out = []

    def add(name, M, W, voices, N, K, position, step=1, **rows):
        modes = rows.pop('modes', None)
        modes = mode_table(M, W) if modes is None else modes
        rng = np.random.default_rng(len(out))
        c = dict(name=name, modes=modes, voices=voices, N=N, K=K, position=position, step=step,
                 hertz=hertz_mix(voices, modes), gate_on=gate_mix(voices, position, N * K, step),
                 damp=np.where(rng.uniform(0, 1, (1, voices)) < 0.5, 0.0, rng.uniform(0.0, 6.0, (1, voices))),
                 select=select_mix(voices) if W > 1 else None)
        c.update(rows)
        out.append(c)

    # voices x frames x positions x M x W: every value of every axis at least once, the mixed pitches, strikes and sets everywhere
    shapes = [(1, 1, 0, 1, 1), (2, 2, 37, 2, 3), (63, RUN - 1, 1000, 63, 1), (65, RUN, 2 ** 24 + 5, 64, 3), (130, RUN + 1, 2 ** 31 + 3, 64, 1),
              (65, 255, 0, 2, 1), (63, 256, 37, 63, 3), (130, 257, 1000, 1, 3), (2, 256, 2 ** 31 + 3, 64, 3), (1, 257, 2 ** 24 + 5, 63, 1)]
    for V, N, pos, M, W in shapes:
        add(f'mix[V={V},N={N},pos={pos},M={M},W={W}]', M, W, V, N, 1, pos)
    # damp 3 on every voice, then unplugged with an unplugged gate (a strike at 0) and select
    add('damp 3[V=65]', 8, 1, 65, 100, 1, 0, damp=np.array([[3.0]]))
    add('unplugged[V=65]', 8, 1, 65, 100, 1, 37, gate_on=None, damp=None, select=None)
    # the issue's host figure: 64 modes, the pitches 55 / 440.3 / 1733.9, struck at the stretch's start, far out
    for pos in (0, 2 ** 24 + 5, 2 ** 31 + 3):
        add(f'string[pos={pos}]', 64, 1, 3, 256, 1, pos, hertz=np.array([[55.0, 440.3, 1733.9]]), gate_on=np.array([[pos / RATE]]),
            damp=None, modes=string64())
    # a frame step: rows three frames apart from a position that is no multiple of it
    add('step 3[V=65]', 16, 3, 65, 130, 1, 37, step=3)
    # per-block rows: all four ports change between blocks, a block length that is no multiple of the run, a retrigger in every block
    K, N, V = 4, 100, 70
    for pos in (0, 1000):
        rng = np.random.default_rng(pos + 7)
        gates = np.concatenate([gate_mix(V, pos + b * N, N, offset=b) for b in range(K)])
        add(f'per block[pos={pos}]', 24, 3, V, N, K, pos, hertz=hertz_mix(V, mode_table(24, 3)) * np.linspace(1.0, 1.5, K)[:, None],
            gate_on=gates, damp=rng.uniform(0.0, 5.0, (K, V)), select=select_mix(V, K) + np.arange(K)[:, None])
    return out


def string64() -> np.ndarray:
    """ext.Modal.string(64, 2.0) without the package: ratios i, amplitudes 1 / i, decay times 2 / i"""
    i = np.arange(1, 65, dtype=np.float64)
    return np.stack([i, 1.0 / i, 2.0 / i], axis=1)


def render_case(c: dict, dtype=np.float64) -> np.ndarray:
    """the restatement's rows of one case, (N * K, voices)"""
    zero = np.zeros((1, 1))
    return modal(c['modes'], c['position'], c['N'], c['hertz'], *(zero if c[k] is None else c[k] for k in ('gate_on', 'damp', 'select')),
                 blocks=c['K'], step=c['step'], dtype=dtype)


def oracle_node():
    """the oracle Node class of the modal bank (imported lazily: the functions above need numpy alone)"""
    from oracle import chain_ref as R

    class Modal(R.Node):
        """takes part in render_stream's cache and context semantics like any oracle node"""

        def __init__(self, modes, hertz=None, gate_on=None, damp=None, select=None):
            super().__init__(hertz=hertz, gate_on=gate_on, damp=damp, select=select)
            self.modes = modes

        def eval(self, position, frames, channels, rate):
            rows = [self._ctrl(name, position, channels, rate) for name in ('hertz', 'gate_on', 'damp', 'select')]
            return modal_rows(self.modes, position + np.arange(frames, dtype=np.int64), *rows, rate=rate)
    return Modal
