#!/usr/bin/env python3
"""A supersaw lead with a filter sweep, headless: one `ext.UnisonSawtooth` voice per note through an `ext.ResonantLowPass` whose
cutoff follows a slow LFO, shaped by an `ext.ADSR`, panned across a stereo `SumBus` and written to a WAV file by `FileWriter`.  The
unison oscillator and the resonant filter are two extension nodes in one voice: `mixed_programs=True` lets the engine render the
whole voice as one voice program, `specialise=True` builds the kernel for it (without the option each node runs as its own kernel).

    python scripts/example_supersaw.py [-o PATH] [-s SECONDS] [--spread X] [--resonance Q] [--sweep HZ] [NOTE ...]        (needs a GPU)
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
    parser.add_argument('-o', '--output', default='supersaw_sweep.wav')
    parser.add_argument('-s', '--seconds', type=float, default=3.0)
    parser.add_argument('--spread', type=float, default=0.6)
    parser.add_argument('--resonance', type=float, default=3.0, help='q of the low-pass (default: %(default)s)')
    parser.add_argument('--sweep', type=float, default=0.5, help='rate of the cutoff LFO in Hz (default: %(default)s)')
    args = parser.parse_args(argv)

    from signals_amd import runtime
    from signals_amd.chain.ext import ADSR, ResonantLowPass, SumBus, UnisonSawtooth
    from signals_amd.chain.files import FileWriter
    from signals_amd.chain.fx import Gain, Mix, RingMod
    from signals_amd.chain.osc import Sine
    from signals_amd.engine import BatchRenderer
    runtime.set_device('cuda:0')

    rate, frames = 48000, 256
    hertz = 440.0 * 2.0 ** ((np.asarray(args.notes)[None, :] - 69.0) / 12.0)  # (1, voices)
    voices = hertz.shape[1]
    saw = UnisonSawtooth(); saw.hertz = fixed(hertz); saw.spread = fixed([[args.spread]])
    # cutoff = centre + depth sin(2 pi sweep t), read once per block: Mix(Gain(Sine, 2 depth), 2 centre, 1/2)
    centre, depth = np.full((1, voices), 2400.0), np.full((1, voices), 1800.0)
    lfo = Sine(); lfo.hertz = fixed([[args.sweep]])
    swing = Gain(); swing.left = lfo; swing.right = fixed(2.0 * depth)
    cutoff = Mix(); cutoff.left = swing; cutoff.right = fixed(2.0 * centre); cutoff.mix = fixed([[0.5]])
    lp = ResonantLowPass(); lp.input = saw; lp.cutoff = cutoff; lp.resonance = fixed(np.full((1, voices), args.resonance))
    env = ADSR()
    for name, value in dict(attack=0.02, decay=0.3, sustain=0.7, release=0.4, gate_on=0.0, gate_off=max(args.seconds - 0.5, 0.1)).items():
        setattr(env, name, fixed(np.full((1, voices), value)))
    shaped = RingMod(); shaped.left = lp; shaped.right = env
    angle = np.linspace(0.15, 0.85, voices) * np.pi / 2                       # the notes fanned out between the speakers
    bus = SumBus(); bus.input = shaped
    bus.get_state().gains = np.stack([np.cos(angle), np.sin(angle)]) * (0.5 / np.sqrt(voices))
    writer = FileWriter(); writer.input = bus
    writer.get_state().path = str(args.output)
    writer.get_state().subtype = 'FLOAT'

    blocks = int(np.ceil(args.seconds * rate / frames))
    out = BatchRenderer(writer, 2, rate, mixed_programs=True, specialise=True).render(0, frames, blocks).cpu().numpy()
    writer.destroy()
    runtime.check_status()
    copies = saw.get_state().copies.shape[0]
    print(f'{blocks} blocks of {frames} frames -> {args.output}: {voices} notes x {copies} saws, spread {args.spread}, '
          f'q {args.resonance}, sweep {args.sweep} Hz, peak {np.abs(out).max():.3f}, rms {np.sqrt(np.mean(out ** 2)):.3f}')
    return pathlib.Path(args.output)


if __name__ == '__main__':
    main()
