#!/usr/bin/env python3
"""Two clean sounds, headless, each written to a WAV file of its own by `FileWriter` (PREFIX_sweep.wav, PREFIX_supersaw.wav):
an `ext.BlepSawtooth` swept once from --low to --high hertz (a block-rate ramp drives its `hertz` port: the correction follows the
pitch, which a wavetable column cannot), and a band-limited supersaw chord: one `ext.BlepSawtooth` per note carrying
`UnisonSawtooth`'s seven JP-8000 copies.  `--naive` renders the same two sounds with `UnisonSawtooth`, to hear the fold-back the band
limit removes.

    python scripts/example_blep.py [-o PREFIX] [-s SECONDS] [--low HZ] [--high HZ] [--spread X] [--naive] [NOTE ...]        (needs a GPU)
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


def main(argv=None) -> list:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('notes', nargs='*', type=float, default=[57.0, 69.0, 72.0, 76.0, 79.0],
                        help='MIDI note numbers of the chord (default: an A minor seventh over its root)')
    parser.add_argument('-o', '--output', default='blep', help='prefix of the two files (default: %(default)s)')
    parser.add_argument('-s', '--seconds', type=float, default=3.0, help='length of each of the two sounds')
    parser.add_argument('--low', type=float, default=110.0)
    parser.add_argument('--high', type=float, default=7040.0)
    parser.add_argument('--spread', type=float, default=0.6)
    parser.add_argument('--naive', action='store_true', help='UnisonSawtooth instead: the same sounds with their aliases')
    args = parser.parse_args(argv)

    from signals_amd import runtime
    from signals_amd.chain import ext, fx, osc
    from signals_amd.chain.files import FileWriter
    from signals_amd.engine import BatchRenderer
    runtime.set_device('cuda:0')
    Saw = ext.UnisonSawtooth if args.naive else ext.BlepSawtooth
    rate, frames = 48000, 256
    blocks = int(np.ceil(args.seconds * rate / frames))

    def render(top, name):
        writer = FileWriter(); writer.input = top
        writer.get_state().path = str(name)
        writer.get_state().subtype = 'FLOAT'
        out = BatchRenderer(writer, 2, rate).render(0, frames, blocks).cpu().numpy()
        writer.destroy()
        return out

    # the sweep: hertz = low + (high - low) * (ramp + 1) / 2 as Mix(Gain(ramp, high - low), high + low, 1/2), one ramp over the sound
    ramp = osc.Sawtooth(); ramp.hertz = fixed([[1.0 / args.seconds]]); ramp.phase = fixed([[0.5]])
    g = fx.Gain(); g.left = ramp; g.right = fixed([[args.high - args.low]])
    hz = fx.Mix(); hz.left = g; hz.right = fixed([[args.high + args.low]]); hz.mix = fixed([[0.5]])
    saw = Saw(); saw.get_state().copies = np.zeros((1, 2)); saw.hertz = hz
    bus = ext.SumBus(); bus.input = saw; bus.get_state().gains = np.full((2, 1), 0.5)
    paths = [pathlib.Path(f'{args.output}_sweep.wav'), pathlib.Path(f'{args.output}_supersaw.wav')]
    sweep = render(bus, paths[0])

    # the chord: seven detuned band-limited saws per note, fanned out between the speakers
    hertz = 440.0 * 2.0 ** ((np.asarray(args.notes)[None, :] - 69.0) / 12.0)  # (1, voices)
    voices = hertz.shape[1]
    stack = Saw(); stack.get_state().copies = ext.UnisonSawtooth().get_state().copies
    stack.hertz = fixed(hertz); stack.spread = fixed([[args.spread]])
    angle = np.linspace(0.15, 0.85, voices) * np.pi / 2
    bus = ext.SumBus(); bus.input = stack
    bus.get_state().gains = np.stack([np.cos(angle), np.sin(angle)]) * (0.7 / np.sqrt(voices))
    chord = render(bus, paths[1])
    for path, out, what in ((paths[0], sweep, f'one saw swept {args.low:g} -> {args.high:g} Hz'),
                            (paths[1], chord, f'{voices} notes x 7 saws at spread {args.spread}')):
        print(f'{blocks} blocks of {frames} frames -> {path}: {"naive" if args.naive else "band-limited"}, {what}; '
              f'peak {np.abs(out).max():.3f}, rms {np.sqrt(np.mean(out ** 2)):.3f}')
    return paths


if __name__ == '__main__':
    main()
