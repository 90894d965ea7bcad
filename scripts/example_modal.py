#!/usr/bin/env python3
"""Two sounds of the modal resonator bank, headless.  Left channel: a marimba phrase -- `ext.Modal` with the free-free bar's modes
(`Modal.bar`), one voice per note of an arpeggio, every voice struck at its own `gate_on`, summed by `SumBus`.  Right channel: a
bell (`Modal.bell`) struck at the start and stopped by hand a second before the end: a step on `damp`, an `ext.ADSR` whose attack is
one block long.  The mix is written to a WAV file by `FileWriter`; the level of each channel is printed half-way through and at the end.

    python scripts/example_modal.py [FREQUENCY] [-o PATH] [-s SECONDS]        (needs a GPU)
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


def hand(at: float, rate_per_second: float):
    """a block-rate step on `damp`: 0 until `at` seconds, then `rate_per_second` (an ADSR with an attack of a few milliseconds, scaled)"""
    from signals_amd.chain.ext import ADSR
    from signals_amd.chain.fx import Gain
    env = ADSR()
    for name, value in (('attack', 0.005), ('decay', 0.0), ('sustain', 1.0), ('release', 0.0), ('gate_on', at), ('gate_off', 1e6)):
        setattr(env, name, fixed([[value]]))
    g = Gain(); g.left = env; g.right = fixed([[rate_per_second]])
    return g


def main(argv=None) -> pathlib.Path:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('frequency', nargs='?', type=float, default=220.0, help='the phrase\'s root in Hz (default: %(default)s)')
    parser.add_argument('-o', '--output', default='modal.wav')
    parser.add_argument('-s', '--seconds', type=float, default=3.0)
    args = parser.parse_args(argv)

    from signals_amd import runtime
    from signals_amd.chain.ext import Modal, SumBus
    from signals_amd.chain.files import FileWriter
    from signals_amd.chain.shape import Merge
    from signals_amd.engine import BatchRenderer
    runtime.set_device('cuda:0')

    rate, frames = 48000, 256
    steps = np.array([[0, 4, 7, 12, 16, 12, 7, 4]])                            # a major arpeggio up and down, one voice per note
    notes = args.frequency * 2.0 ** (steps / 12.0)
    marimba = Modal(); marimba.get_state().modes = Modal.bar(6, 0.8)
    marimba.hertz = fixed(notes)
    marimba.gate_on = fixed(0.05 + 0.18 * np.arange(steps.shape[1]).reshape(1, -1))
    bus = SumBus(); bus.input = marimba; bus.get_state().gains = np.full((1, steps.shape[1]), 0.4)

    bell = Modal(); bell.get_state().modes = Modal.bell(8.0) * np.array([1.0, 0.2, 1.0])
    bell.hertz = fixed([[args.frequency]])
    bell.damp = hand(args.seconds - 1.0, 30.0)
    both = Merge(); both.left = bus; both.right = bell
    writer = FileWriter(); writer.input = both
    writer.get_state().path = str(args.output)
    writer.get_state().subtype = 'FLOAT'

    blocks = int(np.ceil(args.seconds * rate / frames))
    out = BatchRenderer(writer, 2, rate).render(0, frames, blocks).cpu().numpy()
    writer.destroy()
    rms = lambda x: float(np.sqrt(np.mean(x.astype(np.float64) ** 2)))
    half, last = slice(len(out) // 2 - 2048, len(out) // 2), slice(-2048, None)
    print(f'{blocks} blocks of {frames} frames -> {args.output}: a marimba arpeggio on {args.frequency:g} Hz and a bell stopped at '
          f'{args.seconds - 1.0:g} s')
    print(f'  peak: marimba {np.abs(out[:, 0]).max():.3f}, bell {np.abs(out[:, 1]).max():.3f}')
    print(f'  bell rms half-way {rms(out[half, 1]):.2e}, in the last 2048 frames {rms(out[last, 1]):.2e} (the hand)')
    return pathlib.Path(args.output)


if __name__ == '__main__':
    main()
