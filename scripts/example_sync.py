#!/usr/bin/env python3
"""The sync sweep, headless, written to a WAV file by `FileWriter`: an `ext.SyncSawtooth` (or `--square`) per note whose `ratio` port
is swept 1 -> 4 and back by a block-rate LFO -- the formant-like "tearing" of oscillator hard sync -- through an
`ext.ResonantLowPass` to a stereo `ext.SumBus`.  With `mixed_programs=True` the oscillator and the filter are one launch.

    python scripts/example_sync.py [-o FILE] [-s SECONDS] [--lfo HZ] [--low R] [--high R] [--cutoff HZ] [-q Q] [--square] [NOTE ...]   (needs a GPU)
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
    parser.add_argument('notes', nargs='*', type=float, default=[45.0, 52.0, 57.0], help='MIDI note numbers (default: A2 E3 A3)')
    parser.add_argument('-o', '--output', default='sync.wav')
    parser.add_argument('-s', '--seconds', type=float, default=4.0)
    parser.add_argument('--lfo', type=float, default=0.25, help='hertz of the ratio sweep (default: one sweep up and down over 4 s)')
    parser.add_argument('--low', type=float, default=1.0, help='lowest ratio')
    parser.add_argument('--high', type=float, default=4.0, help='highest ratio')
    parser.add_argument('--cutoff', type=float, default=6000.0)
    parser.add_argument('-q', '--resonance', type=float, default=1.5)
    parser.add_argument('--square', action='store_true', help='SyncSquare instead of SyncSawtooth')
    args = parser.parse_args(argv)

    from signals_amd import runtime
    from signals_amd.chain import ext, fx, osc
    from signals_amd.chain.files import FileWriter
    from signals_amd.engine import BatchRenderer
    runtime.set_device('cuda:0')
    rate, frames = 48000, 256
    blocks = int(np.ceil(args.seconds * rate / frames))
    hertz = 440.0 * 2.0 ** ((np.asarray(args.notes)[None, :] - 69.0) / 12.0)  # (1, voices)
    voices = hertz.shape[1]

    # ratio = low + (high - low) * (1 - cos) / 2 as Mix(Gain(Sine at phase 3/4, high - low), high + low, 1/2): starts at `low`
    lfo = osc.Sine(); lfo.hertz = fixed([[args.lfo]]); lfo.phase = fixed([[0.75]])
    g = fx.Gain(); g.left = lfo; g.right = fixed([[args.high - args.low]])
    ratio = fx.Mix(); ratio.left = g; ratio.right = fixed([[args.high + args.low]]); ratio.mix = fixed([[0.5]])

    slave = (ext.SyncSquare if args.square else ext.SyncSawtooth)()
    slave.hertz = fixed(hertz); slave.ratio = ratio
    lp = ext.ResonantLowPass(); lp.input = slave; lp.cutoff = fixed(np.full((1, voices), args.cutoff)); lp.resonance = fixed([[args.resonance]])
    angle = np.linspace(0.2, 0.8, voices) * np.pi / 2
    bus = ext.SumBus(); bus.input = lp
    bus.get_state().gains = np.stack([np.cos(angle), np.sin(angle)]) * (0.5 / np.sqrt(voices))
    path = pathlib.Path(args.output)
    writer = FileWriter(); writer.input = bus
    writer.get_state().path = str(path)
    writer.get_state().subtype = 'FLOAT'
    out = BatchRenderer(writer, 2, rate, mixed_programs=True).render(0, frames, blocks).cpu().numpy()
    writer.destroy()
    print(f'{blocks} blocks of {frames} frames -> {path}: {voices} x {"SyncSquare" if args.square else "SyncSawtooth"}, ratio '
          f'{args.low:g} -> {args.high:g} at {args.lfo:g} Hz, ResonantLowPass {args.cutoff:g} Hz q {args.resonance:g}; '
          f'peak {np.abs(out).max():.3f}, rms {np.sqrt(np.mean(out ** 2)):.3f}')
    return path


if __name__ == '__main__':
    main()
