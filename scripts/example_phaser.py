#!/usr/bin/env python3
"""A phaser, headless: a Sawtooth through four `ext.AllPass` filters in series whose cutoffs follow one slow block-rate LFO, mixed
half and half with the dry voice -- where the chain has turned the phase by an odd multiple of pi the two cancel, and the notches
sweep with the LFO.  Pulled block by block through the node API (the eager path) and written to a WAV file by `FileWriter`; the level
of the output over the thirds of the sweep is printed.

    python scripts/example_phaser.py [FREQUENCY] [-o PATH] [-s SECONDS] [-q RESONANCE] [--low HZ] [--high HZ] [--rate LFO_HZ]     (needs a GPU)
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


def build(frequency, resonance, low, high, lfo_hz):
    """the phaser's top node: Mix(AllPass x 4 (Saw), Saw) * 0.25"""
    from signals_amd.chain.ext import AllPass
    from signals_amd.chain.fx import Gain, Mix
    from signals_amd.chain.osc import Sawtooth, Triangle
    saw = Sawtooth(); saw.hertz = fixed([[frequency]])
    # cutoff = centre + half the span * triangle(lfo_hz t): one block-rate control for the whole chain
    centre, half = 0.5 * (high + low), 0.5 * (high - low)
    lfo = Triangle(); lfo.hertz = fixed([[lfo_hz]])
    swing = Gain(); swing.left = lfo; swing.right = fixed([[2.0 * half]])
    cutoff = Mix(); cutoff.left = swing; cutoff.right = fixed([[2.0 * centre]]); cutoff.mix = fixed([[0.5]])
    wet = saw
    for _ in range(4):
        stage = AllPass(); stage.input = wet; stage.cutoff = cutoff; stage.resonance = fixed([[resonance]])
        wet = stage
    both = Mix(); both.left = wet; both.right = saw; both.mix = fixed([[0.5]])
    level = Gain(); level.left = both; level.right = fixed([[0.25]])
    return level


def main(argv=None) -> pathlib.Path:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('frequency', nargs='?', type=float, default=110.0, help='pitch in Hz (default: %(default)s)')
    parser.add_argument('-o', '--output', default='phaser.wav')
    parser.add_argument('-s', '--seconds', type=float, default=4.0)
    parser.add_argument('-q', '--resonance', type=float, default=0.7, help='quality factor of every stage, > 0 (default: %(default)s)')
    parser.add_argument('--low', type=float, default=400.0, help='lowest cutoff of the sweep in Hz (default: %(default)s)')
    parser.add_argument('--high', type=float, default=3200.0, help='highest cutoff of the sweep in Hz (default: %(default)s)')
    parser.add_argument('--rate', type=float, default=0.5, help='LFO rate in Hz (default: %(default)s)')
    args = parser.parse_args(argv)

    from signals_amd import SignalFlags, runtime
    from signals_amd.chain import BlockLoc, Receiver, Shape, port
    from signals_amd.chain.files import FileWriter
    runtime.set_device('cuda:0')

    class Sink(Receiver):
        input = port('input')
        HOST_ARRAYS = False

        @classmethod
        def flags(cls):
            return SignalFlags(0)

    rate, frames = 48000, 256
    writer = FileWriter(); writer.input = build(args.frequency, args.resonance, args.low, args.high, args.rate)
    writer.get_state().path = str(args.output)
    writer.get_state().subtype = 'FLOAT'
    sink = Sink(); sink.input = writer
    blocks = int(np.ceil(args.seconds * rate / frames))
    out = np.concatenate([sink.input.request(BlockLoc(position=b * frames, rate=rate, shape=Shape(frames=frames, channels=1))).cpu().numpy()
                          for b in range(blocks)])
    runtime.check_status()
    writer.destroy()
    print(f'{blocks} blocks of {frames} frames -> {args.output}: a {args.frequency} Hz saw through four all-pass stages, q = {args.resonance}, '
          f'cutoff {args.low} .. {args.high} Hz at {args.rate} Hz, mixed with the dry voice')
    third = len(out) // 3
    for name, part in (('start', out[:third]), ('middle', out[third:2 * third]), ('end', out[2 * third:])):
        print(f'  {name:6s} rms {float(np.sqrt(np.mean(part ** 2))):.4f}  peak {float(np.abs(part).max()):.4f}')
    return pathlib.Path(args.output)


if __name__ == '__main__':
    main()
