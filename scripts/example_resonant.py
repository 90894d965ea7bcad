#!/usr/bin/env python3
"""A swept resonant saw bass, headless: a Sawtooth through `ext.ResonantLowPass` whose cutoff follows a slow block-rate LFO (the
filter sweep of a subtractive synthesiser) at a fixed resonance, written to a WAV file by `FileWriter`; the level of the output at
the start, the middle and the end of the sweep is printed.

    python scripts/example_resonant.py [FREQUENCY] [-o PATH] [-s SECONDS] [-q RESONANCE] [--low HZ] [--high HZ]        (needs a GPU)
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


def main(argv=None) -> pathlib.Path:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('frequency', nargs='?', type=float, default=55.0, help='pitch in Hz (default: %(default)s)')
    parser.add_argument('-o', '--output', default='resonant.wav')
    parser.add_argument('-s', '--seconds', type=float, default=4.0)
    parser.add_argument('-q', '--resonance', type=float, default=6.0, help='quality factor, > 0; 0.707 is the Butterworth response (default: %(default)s)')
    parser.add_argument('--low', type=float, default=1500.0, help='lowest cutoff of the sweep in Hz (default: %(default)s)')
    parser.add_argument('--high', type=float, default=6000.0, help='highest cutoff of the sweep in Hz (default: %(default)s)')
    args = parser.parse_args(argv)

    from signals_amd import runtime
    from signals_amd.chain.ext import ResonantLowPass
    from signals_amd.chain.files import FileWriter
    from signals_amd.chain.fx import Gain, Mix
    from signals_amd.chain.osc import Sawtooth, Triangle
    from signals_amd.engine import BatchRenderer
    runtime.set_device('cuda:0')

    rate, frames = 48000, 256
    saw = Sawtooth(); saw.hertz = fixed([[args.frequency]])
    # cutoff = centre + half the span * triangle(t / seconds): one sweep up and down over the file (a block-rate control)
    centre, half = 0.5 * (args.high + args.low), 0.5 * (args.high - args.low)
    lfo = Triangle(); lfo.hertz = fixed([[1.0 / args.seconds]])
    swing = Gain(); swing.left = lfo; swing.right = fixed([[2.0 * half]])
    cutoff = Mix(); cutoff.left = swing; cutoff.right = fixed([[2.0 * centre]]); cutoff.mix = fixed([[0.5]])
    bass = ResonantLowPass(); bass.input = saw; bass.cutoff = cutoff; bass.resonance = fixed([[args.resonance]])
    level = Gain(); level.left = bass; level.right = fixed([[0.25]])
    writer = FileWriter(); writer.input = level
    writer.get_state().path = str(args.output)
    writer.get_state().subtype = 'FLOAT'

    blocks = int(np.ceil(args.seconds * rate / frames))
    renderer = BatchRenderer(writer, 1, rate)                   # (kept until check_status: it owns the device status words)
    out = renderer.render(0, frames, blocks).cpu().numpy()
    runtime.check_status()
    writer.destroy()
    print(f'{blocks} blocks of {frames} frames -> {args.output}: a {args.frequency} Hz saw through a resonant low-pass, q = {args.resonance}, '
          f'cutoff {args.low} .. {args.high} Hz')
    third = len(out) // 3
    for name, part in (('start', out[:third]), ('middle', out[third:2 * third]), ('end', out[2 * third:])):
        print(f'  {name:6s} rms {float(np.sqrt(np.mean(part ** 2))):.4f}  peak {float(np.abs(part).max()):.4f}')
    return pathlib.Path(args.output)


if __name__ == '__main__':
    main()
