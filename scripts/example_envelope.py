#!/usr/bin/env python3
"""Two envelope patches, headless, rendered through `BatchRenderer` and written to WAV files by `FileWriter`:
  a plucked voice: a Sawtooth through `ext.ResonantLowPass` whose cutoff falls from `--peak` to `--base` Hz with an `ext.ADSR`
      (cutoff = Mix(Fixed(peak), Fixed(base), mix=ADSR): a filter envelope), the same envelope instance shaping the amplitude
      through a RingMod;
  a kick: a Sine whose `hertz` falls from 200 to 50 Hz with a fast ADSR (a pitch envelope), a second envelope on the amplitude.
The envelopes on the control ports are read once per block and run as words of the block-rate control program.  The level of
each output over its first, middle and last third is printed.

    python scripts/example_envelope.py [FREQUENCY] [-o PREFIX] [-s SECONDS] [--peak HZ] [--base HZ]        (needs a GPU)
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


def envelope(attack, decay, sustain, release, gate_on, gate_off):
    from signals_amd.chain.ext import ADSR
    env = ADSR()
    env.attack, env.decay, env.sustain = fixed([[attack]]), fixed([[decay]]), fixed([[sustain]])
    env.release, env.gate_on, env.gate_off = fixed([[release]]), fixed([[gate_on]]), fixed([[gate_off]])
    return env


def swept(peak, base, env):
    """base + (peak - base) * env"""
    from signals_amd.chain.fx import Mix
    m = Mix(); m.left = fixed([[peak]]); m.right = fixed([[base]]); m.mix = env
    return m


def main(argv=None) -> list:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('frequency', nargs='?', type=float, default=110.0, help='pitch of the plucked voice in Hz (default: %(default)s)')
    parser.add_argument('-o', '--output', default='envelope', help='the files are PREFIX_pluck.wav and PREFIX_kick.wav')
    parser.add_argument('-s', '--seconds', type=float, default=1.0)
    parser.add_argument('--peak', type=float, default=6000.0, help='cutoff at the top of the envelope in Hz (default: %(default)s)')
    parser.add_argument('--base', type=float, default=300.0, help='cutoff at rest in Hz (default: %(default)s)')
    args = parser.parse_args(argv)

    from signals_amd import runtime
    from signals_amd.chain.ext import ResonantLowPass
    from signals_amd.chain.files import FileWriter
    from signals_amd.chain.fx import Gain, RingMod
    from signals_amd.chain.osc import Sawtooth, Sine
    from signals_amd.engine import BatchRenderer
    runtime.set_device('cuda:0')
    rate, frames = 48000, 256
    blocks = int(np.ceil(args.seconds * rate / frames))

    # the pluck: one envelope for the cutoff (block rate) and the amplitude (frame rate)
    pluck_env = envelope(0.002, 0.25, 0.15, 0.3, 0.0, 0.6 * args.seconds)
    saw = Sawtooth(); saw.hertz = fixed([[args.frequency]])
    flt = ResonantLowPass(); flt.input = saw; flt.cutoff = swept(args.peak, args.base, pluck_env); flt.resonance = fixed([[2.0]])
    voice = RingMod(); voice.left = flt; voice.right = pluck_env
    pluck = Gain(); pluck.left = voice; pluck.right = fixed([[0.3]])

    # the kick: the pitch on a fast envelope, the amplitude on a slower one
    sine = Sine(); sine.hertz = swept(200.0, 50.0, envelope(0.0, 0.06, 0.0, 0.0, 0.0, args.seconds))
    body = RingMod(); body.left = sine; body.right = envelope(0.001, 0.3, 0.0, 0.0, 0.0, args.seconds)
    kick = Gain(); kick.left = body; kick.right = fixed([[0.8]])

    paths = []
    for name, top in (('pluck', pluck), ('kick', kick)):
        path = pathlib.Path(f'{args.output}_{name}.wav')
        writer = FileWriter(); writer.input = top
        writer.get_state().path = str(path)
        writer.get_state().subtype = 'FLOAT'
        renderer = BatchRenderer(writer, 1, rate)               # (kept until check_status: it owns the device status words)
        out = renderer.render(0, frames, blocks).cpu().numpy()
        runtime.check_status()
        writer.destroy()
        print(f'{name}: {blocks} blocks of {frames} frames -> {path}')
        third = len(out) // 3
        for part_name, part in (('start', out[:third]), ('middle', out[third:2 * third]), ('end', out[2 * third:])):
            print(f'  {part_name:6s} rms {float(np.sqrt(np.mean(part ** 2))):.4f}  peak {float(np.abs(part).max()):.4f}')
        paths.append(path)
    return paths


if __name__ == '__main__':
    main()
