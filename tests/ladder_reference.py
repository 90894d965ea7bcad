"""numpy restatement of the 4-pole ladder low-pass (signals_amd/chain/ext.py: Ladder), the build-defined filter the reference has no
counterpart of.  Per voice and block, float64, one operation per line, states s1..s4 = 0 at the window's first row:

    wn = clip(cutoff / (rate / 2), 0, 1)          # as fx.py:99-102; ValueError unless 0 < wn < 1 (NaN too)
    g  = tan(pi * wn / 2);  G = g / (1 + g);  H = 1 - G
    k  = clip(resonance, 0, 4)                    # ValueError for NaN or +-inf
    d  = max(drive, 0)                            # NaN or +inf: NaN rows
    c  = 1 / (1 + k * ((G*G) * (G*G)))
    per row:  S = H * (((s1*G + s2)*G + s3)*G + s4);  u = (x - k*S) * c;  if d > 0: u = tanh(d*u) / d
              for j = 1..4:  v = (u - s_j)*G;  y_j = v + s_j;  s_j = y_j + v;  u = y_j
              out = y_poles

`design` and `ladder_rows` are the definition (no scipy anywhere in the recursion; the voices of a row are one numpy vector);
`ladder_blocks` is what sig_ladder_coldstart computes, with NaN rows where the definition raises or says NaN and the status bits it
sets; `oracle_node` takes part in `render_stream`'s cache and context semantics like `chain_ref.Filter`."""
import numpy as np

CONTEXT_FRAMES = 100
STATUS_BAD_CUTOFF, STATUS_BAD_RESONANCE = 1, 2


def design(cutoff, resonance, drive, rate):
    """(G, H, k, d, c, status bits, nan voices) of one block: `cutoff`, `resonance`, `drive` 1-D float64 arrays of one length
    (`resonance` / `drive` None: unplugged = 0).  Refused voices get G = NaN, so that every row of them follows"""
    cutoff = np.asarray(cutoff, dtype=np.float64)
    voices = cutoff.shape[0]
    resonance = np.zeros(voices) if resonance is None else np.asarray(resonance, dtype=np.float64)
    drive = np.zeros(voices) if drive is None else np.asarray(drive, dtype=np.float64)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        wn = cutoff / (rate / 2)
        wn = np.clip(wn, 0.0, 1.0)
        bad_cut = ~((wn > 0.0) & (wn < 1.0))
        bad_k = ~np.isfinite(resonance)
        k = np.clip(resonance, 0.0, 4.0)
        bad_d = np.isnan(drive) | (drive == np.inf)
        d = np.maximum(drive, 0.0)
        g = np.tan(np.pi * wn / 2.0)
        G = g / (1.0 + g)
        H = 1.0 - G
        G2 = G * G
        G4 = G2 * G2
        c = 1.0 / (1.0 + k * G4)
    nan = bad_cut | bad_k | bad_d
    G = np.where(nan, np.nan, G)
    status = (STATUS_BAD_CUTOFF if bad_cut.any() else 0) | (STATUS_BAD_RESONANCE if bad_k.any() else 0)
    return G, H, k, np.where(nan, 0.0, d), c, status, nan


def ladder_rows(x, G, H, k, d, c, poles, taps=False):
    """the recursion over the rows of `x` (rows, voices) from zero state: (rows, voices) float64, the output of pole `poles`; with
    `taps` also the loop input u behind the saturator, row by row"""
    x = np.asarray(x, dtype=np.float64)
    rows, voices = x.shape
    s = [np.zeros(voices) for _ in range(4)]
    out = np.empty((rows, voices))
    loop = np.empty((rows, voices)) if taps else None
    driven = d > 0.0
    safe_d = np.where(driven, d, 1.0)
    with np.errstate(invalid='ignore', over='ignore'):
        for n in range(rows):
            S = s[0] * G
            S = S + s[1]
            S = S * G
            S = S + s[2]
            S = S * G
            S = S + s[3]
            S = H * S
            u = k * S
            u = x[n] - u
            u = u * c
            if driven.any():
                t = safe_d * u
                t = np.tanh(t)
                t = t / safe_d
                u = np.where(driven, t, u)
            if taps:
                loop[n] = u
            y = None
            for j in range(4):
                v = u - s[j]
                v = v * G
                yj = v + s[j]
                s[j] = yj + v
                u = yj
                if j + 1 == poles:
                    y = yj
            out[n] = y
    return (out, loop) if taps else out


def ladder_blocks(x, history, frames, blocks, cutoff, resonance, drive, poles, rate, ctx=CONTEXT_FRAMES):
    """what sig_ladder_coldstart computes: `x` holds `history` = min(ctx, position) rows in front of blocks * frames rows; block b is
    filtered from zero state over [min(ctx, position + b frames) rows | block] with row b (or the only row) of each control
    ((1 | blocks, V | 1); `resonance` / `drive` None: unplugged).  Returns (out, status bits)"""
    x = np.asarray(x, dtype=np.float64)
    voices = x.shape[1]
    out = np.empty((blocks * frames, voices))
    status = 0

    def row(ctl, b):
        if ctl is None:
            return None
        ctl = np.asarray(ctl, dtype=np.float64)
        return np.broadcast_to(ctl[b if ctl.shape[0] > 1 else 0], (voices,))
    for b in range(blocks):
        start = history + b * frames
        c0 = min(ctx, start)
        G, H, k, d, c, bits, _ = design(row(cutoff, b), row(resonance, b), row(drive, b), rate)
        status |= bits
        out[b * frames:(b + 1) * frames] = ladder_rows(x[start - c0:start + frames], G, H, k, d, c, poles)[c0:]
    return out, status


def impulse_tail_share(cutoff, k, rate, beyond=CONTEXT_FRAMES, rows=200000):
    """the share of the linear impulse response's L1 norm that lies beyond `beyond` frames (what a 100-frame cold start truncates)"""
    G, H, kk, d, c, _, _ = design([cutoff], [k], None, rate)
    x = np.zeros((rows, 1))
    x[0] = 1.0
    h = np.abs(ladder_rows(x, G, H, kk, d, c, 4)[:, 0])
    return float(h[beyond:].sum() / h.sum())


def oracle_node():
    """the oracle Node class of the ladder (imported lazily: the functions above need numpy alone)"""
    from oracle import chain_ref as R

    class Ladder(R.Node):
        """chain_ref.Filter with two more block-rate controls and the ladder's recursion; `resonance` / `drive` None: unplugged.  A
        one-column input broadcasts over the request's channels; a refused control raises what the eager check_status() raises"""

        def __init__(self, input=None, cutoff=None, resonance=None, drive=None, poles=4):
            super().__init__(input=input, cutoff=cutoff, resonance=resonance, drive=drive)
            self.poles = poles

        def eval(self, position, frames, channels, rate):
            cutoff = self._ctrl('cutoff', position, channels, rate)
            k = self._ctrl('resonance', position, channels, rate) if self.inputs.get('resonance') is not None else None
            d = self._ctrl('drive', position, channels, rate) if self.inputs.get('drive') is not None else None
            window = self._with_context('input', position, frames, channels, rate, R.CONTEXT_FRAMES)
            if window.shape[1] not in (1, channels):
                raise IndexError('filter input narrower than the request (fx.py:98-105)')
            window = np.broadcast_to(window, (window.shape[0], channels))
            wide = lambda t: None if t is None else np.broadcast_to(t[0, :channels] if t.shape[1] >= channels else t[0], (channels,))
            G, H, kk, dd, c, status, _ = design(cutoff[0, :channels], wide(k), wide(d), rate)
            if status & STATUS_BAD_CUTOFF:
                raise ValueError('Digital filter critical frequencies must be 0 < Wn < 1')
            if status & STATUS_BAD_RESONANCE:
                raise ValueError('filter resonance must be finite')
            return ladder_rows(window[:window.shape[0] - R.CONTEXT_FRAMES], G, H, kk, dd, c, self.poles)[-frames:]
    return Ladder
