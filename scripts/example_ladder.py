#!/usr/bin/env python3
"""A plucked ladder-filter bass, headless: a Sawtooth through `ext.Ladder` (the 4-pole transistor-ladder low-pass) whose cutoff follows
an ADSR envelope read at block rate -- `cutoff = Mix(Fixed(peak), Fixed(base), mix=ADSR)` -- at resonance k = 3 and drive 2, written
to a WAV file by `FileWriter`; the level of the output over the attack, the decay and the release is printed.

    python scripts/example_ladder.py [FREQUENCY] [-o PATH] [-s SECONDS] [-k RESONANCE] [-d DRIVE] [-p POLES] [--base HZ] [--peak HZ]        (needs a GPU)
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
    parser.add_argument('-o', '--output', default='ladder.wav')
    parser.add_argument('-s', '--seconds', type=float, default=3.0)
    parser.add_argument('-k', '--resonance', type=float, default=3.0, help='feedback, 0 .. 4; 4 is the edge of self-oscillation (default: %(default)s)')
    parser.add_argument('-d', '--drive', type=float, default=2.0, help='saturator drive, 0 = a linear loop (default: %(default)s)')
    parser.add_argument('-p', '--poles', type=int, default=4, help='output tap, 1 .. 4: 6 dB/oct each (default: %(default)s)')
    parser.add_argument('--base', type=float, default=120.0, help='cutoff at rest in Hz (default: %(default)s)')
    parser.add_argument('--peak', type=float, default=5000.0, help='cutoff at the envelope\'s top in Hz (default: %(default)s)')
    args = parser.parse_args(argv)

    from signals_amd import runtime
    from signals_amd.chain.ext import ADSR, Ladder
    from signals_amd.chain.files import FileWriter
    from signals_amd.chain.fx import Gain, Mix
    from signals_amd.chain.osc import Sawtooth
    from signals_amd.engine import BatchRenderer
    runtime.set_device('cuda:0')

    rate, frames = 48000, 256
    saw = Sawtooth(); saw.hertz = fixed([[args.frequency]])
    # the filter envelope: a fast attack, a decay to a fifth of the way up, a release two thirds into the file (a block-rate control)
    env = ADSR()
    env.attack = fixed([[0.01]]); env.decay = fixed([[0.4]]); env.sustain = fixed([[0.2]]); env.release = fixed([[0.5]])
    env.gate_on = fixed([[0.0]]); env.gate_off = fixed([[args.seconds * 2.0 / 3.0]])
    cutoff = Mix(); cutoff.left = fixed([[args.peak]]); cutoff.right = fixed([[args.base]]); cutoff.mix = env
    bass = Ladder(); bass.input = saw; bass.cutoff = cutoff
    bass.resonance = fixed([[args.resonance]]); bass.drive = fixed([[args.drive]])
    bass.get_state().poles = args.poles
    level = Gain(); level.left = bass; level.right = fixed([[0.5]])
    writer = FileWriter(); writer.input = level
    writer.get_state().path = str(args.output)
    writer.get_state().subtype = 'FLOAT'

    blocks = int(np.ceil(args.seconds * rate / frames))
    renderer = BatchRenderer(writer, 1, rate)                   # (kept until check_status: it owns the device status words)
    out = renderer.render(0, frames, blocks).cpu().numpy()
    runtime.check_status()
    writer.destroy()
    print(f'{blocks} blocks of {frames} frames -> {args.output}: a {args.frequency} Hz saw through a {args.poles}-pole ladder, k = {args.resonance}, '
          f'drive {args.drive}, cutoff {args.base} .. {args.peak} Hz on an envelope')
    third = len(out) // 3
    for name, part in (('attack', out[:third]), ('decay', out[third:2 * third]), ('release', out[2 * third:])):
        print(f'  {name:7s} rms {float(np.sqrt(np.mean(part ** 2))):.4f}  peak {float(np.abs(part).max()):.4f}')
    return pathlib.Path(args.output)


if __name__ == '__main__':
    main()
