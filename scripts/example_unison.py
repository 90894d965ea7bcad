#!/usr/bin/env python3
"""A supersaw chord, headless: one `ext.UnisonSawtooth` voice per note -- seven detuned saws each, the node's default layout --
through a `LowPass`, panned across a stereo `SumBus` and written to a WAV file by `FileWriter`.  `--spread` scales the detune
(0: every copy at the note's pitch, a phase-shifted stack; 1: the full JP-8000 spacing).

    python scripts/example_unison.py [-o PATH] [-s SECONDS] [--spread X] [--cutoff HZ] [NOTE ...]        (needs a GPU)
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
    parser.add_argument('notes', nargs='*', type=float, default=[45.0, 57.0, 60.0, 64.0, 67.0],
                        help='MIDI note numbers (default: an A minor seventh over its root)')
    parser.add_argument('-o', '--output', default='supersaw.wav')
    parser.add_argument('-s', '--seconds', type=float, default=3.0)
    parser.add_argument('--spread', type=float, default=0.6)
    parser.add_argument('--cutoff', type=float, default=4000.0, help='low-pass cutoff in Hz (default: %(default)s)')
    args = parser.parse_args(argv)

    from signals_amd import runtime
    from signals_amd.chain.ext import SumBus, UnisonSawtooth
    from signals_amd.chain.files import FileWriter
    from signals_amd.chain.fx import LowPass
    from signals_amd.engine import BatchRenderer
    runtime.set_device('cuda:0')

    rate, frames = 48000, 256
    hertz = 440.0 * 2.0 ** ((np.asarray(args.notes)[None, :] - 69.0) / 12.0)  # (1, voices)
    voices = hertz.shape[1]
    saw = UnisonSawtooth(); saw.hertz = fixed(hertz); saw.spread = fixed([[args.spread]])
    lp = LowPass(); lp.input = saw; lp.cutoff = fixed(np.full((1, voices), args.cutoff))
    angle = np.linspace(0.15, 0.85, voices) * np.pi / 2                       # the notes fanned out between the speakers
    bus = SumBus(); bus.input = lp
    bus.get_state().gains = np.stack([np.cos(angle), np.sin(angle)]) * (0.7 / np.sqrt(voices))
    writer = FileWriter(); writer.input = bus
    writer.get_state().path = str(args.output)
    writer.get_state().subtype = 'FLOAT'

    blocks = int(np.ceil(args.seconds * rate / frames))
    out = BatchRenderer(writer, 2, rate).render(0, frames, blocks).cpu().numpy()
    writer.destroy()
    copies = saw.get_state().copies.shape[0]
    print(f'{blocks} blocks of {frames} frames -> {args.output}: {voices} notes x {copies} saws, spread {args.spread}, '
          f'peak {np.abs(out).max():.3f}, rms {np.sqrt(np.mean(out ** 2)):.3f}')
    return pathlib.Path(args.output)


if __name__ == '__main__':
    main()
