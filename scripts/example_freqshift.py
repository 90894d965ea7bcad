#!/usr/bin/env python3
"""A single-sideband frequency shifter, headless: every partial of a sawtooth moved up by the same few hertz (not scaled, as a pitch
change would), so the harmonics go out of tune against each other.  The analytic pair is a 101-tap Hilbert transformer
(`FIR.hilbert()`, group delay 50 frames) and `Delay` at exactly those 50 frames as the matched path; the carrier pair is two `Sine`
a quarter cycle apart:

    out = 0.5 * (Delay(x, 50 frames) * cos(2 pi s t)  -  FIR_hilbert(x) * sin(2 pi s t))

spelled `Mix(RingMod(Delay, Sine at phase 1/4), RingMod(FIR, Sine at phase 1/2), 0.5)` -- a Sine at phase 1/2 is -sin.  Written to a
WAV file by `FileWriter`.  For the first partials the level of the wanted (upper) sideband, at f + s, and of the suppressed (lower)
one, at f - s, are printed.  The suppression is what the transformer's gain error leaves, |1 - g| / (1 + g): 101 Blackman-windowed
taps at 48 kHz are flat from about 1.3 kHz (g = 0.68 at 440 Hz: 14 dB; 0.966 at 880 Hz: 35 dB; 76 dB and more from 1320 Hz up), so the
low partials of a low note keep part of their other sideband -- more taps would need a longer context than a block has.

    python scripts/example_freqshift.py [FREQUENCY] [-o PATH] [-s SECONDS] [-x SHIFT_HZ]        (needs a GPU)
"""
import argparse
import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))


def fixed(v):
    from signals_amd.chain.fixed import Fixed
    f = Fixed()
    f.get_state().value = np.array(v, ndmin=2, dtype=float)
    return f


def level_db(x: np.ndarray, frequency: float, rate: int) -> float:
    """the amplitude of the component at exactly `frequency`, in dB re 1, by projection on a windowed complex exponential"""
    n = np.arange(len(x))
    w = np.blackman(len(x))
    amp = 2.0 * abs(np.sum(x * w * np.exp(-2j * np.pi * frequency / rate * n))) / np.sum(w)
    return float(20.0 * np.log10(max(amp, 1e-15)))


def main(argv=None) -> pathlib.Path:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('frequency', nargs='?', type=float, default=440.0, help='pitch in Hz (default: %(default)s)')
    parser.add_argument('-o', '--output', default='freqshift.wav')
    parser.add_argument('-s', '--seconds', type=float, default=4.0)
    parser.add_argument('-x', '--shift', type=float, default=5.0, help='shift in Hz, upwards (default: %(default)s)')
    args = parser.parse_args(argv)

    from signals_amd import runtime
    from signals_amd.chain.ext import FIR, Delay
    from signals_amd.chain.files import FileWriter
    from signals_amd.chain.fx import Mix, RingMod
    from signals_amd.chain.osc import Sawtooth, Sine
    from signals_amd.engine import BatchRenderer
    runtime.set_device('cuda:0')

    rate, frames = 48000, 256
    taps = FIR.hilbert()                                                       # 101 taps: group delay 50 frames
    delay = (taps.shape[0] - 1) // 2
    saw = Sawtooth(); saw.hertz = fixed([[args.frequency]])
    real = Delay(); real.input = saw; real.time = fixed([[delay / rate]])      # the matched path: the same 50 frames
    imag = FIR(); imag.get_state().taps = taps; imag.input = saw
    cos = Sine(); cos.hertz = fixed([[args.shift]]); cos.phase = fixed([[0.25]])
    minus_sin = Sine(); minus_sin.hertz = fixed([[args.shift]]); minus_sin.phase = fixed([[0.5]])
    a = RingMod(); a.left = real; a.right = cos
    b = RingMod(); b.left = imag; b.right = minus_sin
    shifted = Mix(); shifted.left = a; shifted.right = b; shifted.mix = fixed([[0.5]])
    writer = FileWriter(); writer.input = shifted
    writer.get_state().path = str(args.output)
    writer.get_state().subtype = 'FLOAT'

    blocks = int(np.ceil(args.seconds * rate / frames))
    out = BatchRenderer(writer, 1, rate).render(0, frames, blocks).cpu().numpy()
    writer.destroy()
    print(f'{blocks} blocks of {frames} frames -> {args.output}: a {args.frequency} Hz sawtooth, every partial moved up by {args.shift} Hz')
    seg = out[rate // 2:rate // 2 + 2 * rate, 0].astype(np.float64)            # two seconds, clear of the start
    if len(seg) == 2 * rate:
        for partial in (1, 2, 3, 4, 8):
            f = partial * args.frequency
            if f + args.shift < rate / 2:
                wanted, other = level_db(seg, f + args.shift, rate), level_db(seg, f - args.shift, rate)
                print(f'  partial {partial}: wanted sideband at {f + args.shift:7.1f} Hz {wanted:6.1f} dB, suppressed sideband at '
                      f'{f - args.shift:7.1f} Hz {other:6.1f} dB: {wanted - other:5.1f} dB apart')
    return pathlib.Path(args.output)


if __name__ == '__main__':
    main()
