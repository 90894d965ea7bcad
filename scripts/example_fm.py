#!/usr/bin/env python3
"""A two-operator FM bell, headless: a sine carrier phase-modulated by an enveloped sine at an inharmonic ratio (1 : 3.5),
the whole note under a second envelope, rendered through the batched engine and written to a WAV file by `FileWriter`.

    python scripts/example_fm.py [FREQUENCY] [-o PATH] [-s SECONDS] [-i INDEX]        (needs a GPU)
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


def envelope(attack, decay, sustain, release, gate_off):
    from signals_amd.chain.ext import ADSR
    env = ADSR()
    for name, value in dict(attack=attack, decay=decay, sustain=sustain, release=release, gate_on=0.0, gate_off=gate_off).items():
        setattr(env, name, fixed([[value]]))
    return env


def main(argv=None) -> pathlib.Path:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('frequency', nargs='?', type=float, default=220.0, help='carrier frequency in Hz (default: %(default)s)')
    parser.add_argument('-o', '--output', default='fm_bell.wav')
    parser.add_argument('-s', '--seconds', type=float, default=3.0)
    parser.add_argument('-i', '--index', type=float, default=1.2, help='peak phase deviation in cycles (default: %(default)s)')
    args = parser.parse_args(argv)

    from signals_amd import runtime
    from signals_amd.chain.ext import PMSine
    from signals_amd.chain.files import FileWriter
    from signals_amd.chain.fx import Gain, RingMod
    from signals_amd.chain.osc import Sine
    from signals_amd.engine import BatchRenderer
    runtime.set_device('cuda:0')

    modulator = Sine(); modulator.hertz = fixed([[3.5 * args.frequency]])
    bright = RingMod(); bright.left = envelope(0.001, 0.8, 0.05, 0.5, args.seconds * 0.6); bright.right = modulator
    carrier = PMSine(); carrier.hertz = fixed([[args.frequency]]); carrier.index = fixed([[args.index]]); carrier.mod = bright
    note = RingMod(); note.left = envelope(0.002, 1.5, 0.0, 0.3, args.seconds * 0.8); note.right = carrier
    level = Gain(); level.left = note; level.right = fixed([[0.5]])
    writer = FileWriter(); writer.input = level
    writer.get_state().path = str(args.output)
    writer.get_state().subtype = 'FLOAT'

    rate, frames = 48000, 256
    blocks = int(np.ceil(args.seconds * rate / frames))
    out = BatchRenderer(writer, 1, rate).render(0, frames, blocks)
    writer.destroy()
    print(f'{blocks} blocks of {frames} frames -> {args.output}: peak {float(out.abs().max()):.3f}')
    return pathlib.Path(args.output)


if __name__ == '__main__':
    main()
