#!/usr/bin/env python3
"""A flanger, headless: `Mix(x, Delay(x, time = LFO))` on a sawtooth, the delay swept between 0 and DEPTH milliseconds by a slow sine
(read once per block, like every control), the left channel a quarter of an LFO cycle ahead of the right; written to a WAV file
by `FileWriter`.  The comb's first notch, at 1 / (2 delay), is printed for the two ends of the sweep, with the level the output has
there.

    python scripts/example_flanger.py [FREQUENCY] [-o PATH] [-s SECONDS] [-r LFO_HZ] [-d DEPTH_MS]        (needs a GPU)
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


def level_at(x: np.ndarray, frequency: float, rate: int) -> float:
    """the level around `frequency` in dB relative to the strongest bin"""
    spectrum = np.abs(np.fft.rfft(x * np.hanning(len(x))))
    freqs = np.fft.rfftfreq(len(x), 1.0 / rate)
    near = spectrum[np.abs(freqs - frequency) < 40.0]
    return round(float(20.0 * np.log10(max(near.max(), 1e-12) / spectrum.max())), 1)


def main(argv=None) -> pathlib.Path:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('frequency', nargs='?', type=float, default=110.0, help='pitch in Hz (default: %(default)s)')
    parser.add_argument('-o', '--output', default='flanger.wav')
    parser.add_argument('-s', '--seconds', type=float, default=4.0)
    parser.add_argument('-r', '--lfo', type=float, default=0.25, help='sweep rate in Hz (default: %(default)s)')
    parser.add_argument('-d', '--depth', type=float, default=1.5, help='longest delay in ms, at most 99 frames = 2.06 ms (default: %(default)s)')
    args = parser.parse_args(argv)

    from signals_amd import runtime
    from signals_amd.chain.ext import Delay
    from signals_amd.chain.files import FileWriter
    from signals_amd.chain.fx import Gain, Mix
    from signals_amd.chain.osc import Sawtooth, Sine
    from signals_amd.engine import BatchRenderer
    runtime.set_device('cuda:0')

    rate, frames = 48000, 256
    depth = args.depth / 1000.0
    saw = Sawtooth(); saw.hertz = fixed([[args.frequency]])
    lfo = Sine(); lfo.hertz = fixed([[args.lfo]]); lfo.phase = fixed([[0.25, 0.0]])            # one column per channel
    swing = Gain(); swing.left = lfo; swing.right = fixed([[depth]])
    time = Mix(); time.left = swing; time.right = fixed([[depth]]); time.mix = fixed([[0.5]])    # 0 .. depth seconds
    wet = Delay(); wet.input = saw; wet.time = time
    flanged = Mix(); flanged.left = saw; flanged.right = wet; flanged.mix = fixed([[0.5]])
    writer = FileWriter(); writer.input = flanged
    writer.get_state().path = str(args.output)
    writer.get_state().subtype = 'FLOAT'

    blocks = int(np.ceil(args.seconds * rate / frames))
    out = BatchRenderer(writer, 2, rate).render(0, frames, blocks).cpu().numpy()
    writer.destroy()
    print(f'{blocks} blocks of {frames} frames -> {args.output}: a {args.frequency} Hz sawtooth, delay 0 .. {args.depth} ms at {args.lfo} Hz')
    # the right channel's LFO starts at 0: the delay is depth / 2 there, and depth a quarter cycle later
    quarter = int(rate / args.lfo / 4)
    for name, start, delay in (('mid sweep', 0, depth / 2), ('longest', quarter, depth)):
        seg = out[start:start + 4096, 1]
        if len(seg) == 4096 and delay > 0:
            notch = 1.0 / (2.0 * delay)
            print(f'  {name:9s} delay {delay * 1e3:.3f} ms: first notch at {notch:7.1f} Hz, level there {level_at(seg, notch, rate)} dB')
    return pathlib.Path(args.output)


if __name__ == '__main__':
    main()
