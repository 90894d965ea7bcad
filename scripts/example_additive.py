#!/usr/bin/env python3
"""Two sounds of the additive oscillator, headless.  Left channel: a drawbar organ chord -- `ext.Additive` with one column of eight
drawbar levels at the harmonics 1 .. 8 (the sub-octave drawbars are left out: the node's partials are integer multiples of
`hertz`), four voices summed by `SumBus`.  Right channel: a sawtooth of 64 partials under a pitch envelope that sweeps it from
FREQUENCY up four octaves, every partial fading out as it reaches half the rate.  The same sweep is rendered with `osc.Sawtooth`,
and the energy each puts between the harmonics of the sweep's last block (aliasing) is printed.  The mix is written to a WAV file by
`FileWriter`.

    python scripts/example_additive.py [FREQUENCY] [-o PATH] [-s SECONDS]        (needs a GPU)
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


def drawbars(levels=(8, 8, 6, 4, 0, 3, 0, 2)) -> np.ndarray:
    """(8, 1): drawbar levels 0 .. 8 at the harmonics 1 .. 8, in the organ's 3 dB steps, scaled so that the column sums to 1"""
    a = np.where(np.array(levels) > 0, 10.0 ** (3.0 * (np.array(levels, dtype=float) - 8.0) / 20.0), 0.0)
    return (a / a.sum()).reshape(-1, 1)


def pitch_envelope(start: float, octaves: float, seconds: float):
    """a block-rate pitch envelope: an ADSR's attack stage, 0 -> 1 over the first 90 % of `seconds` and held, as the `mix` between the
    end pitch start * 2 ** octaves and the start pitch (a sweep linear in hertz)"""
    from signals_amd.chain.ext import ADSR
    from signals_amd.chain.fx import Mix
    env = ADSR()
    for name, value in (('attack', 0.9 * seconds), ('decay', 0.0), ('sustain', 1.0), ('release', 0.0), ('gate_on', 0.0), ('gate_off', 2 * seconds)):
        setattr(env, name, fixed([[value]]))
    sweep = Mix(); sweep.left = fixed([[start * 2.0 ** octaves]]); sweep.right = fixed([[start]]); sweep.mix = env
    return sweep


def off_harmonic_share(x: np.ndarray, frequency: float, rate: int) -> float:
    """share of the signal's energy that lies further than 2 % of the fundamental from every harmonic"""
    spectrum = np.abs(np.fft.rfft(x * np.hanning(len(x)))) ** 2
    freqs = np.fft.rfftfreq(len(x), 1.0 / rate)
    distance = np.abs(freqs / frequency - np.round(freqs / frequency))
    return float(spectrum[(distance > 0.02) & (freqs > frequency / 2)].sum() / spectrum.sum())


def main(argv=None) -> pathlib.Path:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('frequency', nargs='?', type=float, default=220.0, help='the chord\'s root and the sweep\'s start in Hz (default: %(default)s)')
    parser.add_argument('-o', '--output', default='additive.wav')
    parser.add_argument('-s', '--seconds', type=float, default=2.0)
    args = parser.parse_args(argv)

    from signals_amd import runtime
    from signals_amd.chain.ext import Additive, SumBus
    from signals_amd.chain.files import FileWriter
    from signals_amd.chain.osc import Sawtooth
    from signals_amd.chain.shape import Merge
    from signals_amd.engine import BatchRenderer
    runtime.set_device('cuda:0')

    rate, frames = 48000, 256
    chord = args.frequency * 2.0 ** (np.array([[0, 4, 7, 12]]) / 12.0)         # a major chord and its octave
    organ = Additive(); organ.get_state().table = drawbars(); organ.hertz = fixed(chord)
    bus = SumBus(); bus.input = organ; bus.get_state().gains = np.full((1, 4), 0.25)

    saw = Additive(); saw.get_state().table = 0.5 * Additive.sawtooth(64); saw.hertz = pitch_envelope(args.frequency, 4.0, args.seconds)
    both = Merge(); both.left = bus; both.right = saw
    writer = FileWriter(); writer.input = both
    writer.get_state().path = str(args.output)
    writer.get_state().subtype = 'FLOAT'

    blocks = int(np.ceil(args.seconds * rate / frames))
    out = BatchRenderer(writer, 2, rate).render(0, frames, blocks).cpu().numpy()
    writer.destroy()
    naive = Sawtooth(); naive.hertz = pitch_envelope(args.frequency, 4.0, args.seconds)
    ref = BatchRenderer(naive, 1, rate).render(0, frames, blocks).cpu().numpy()
    top = args.frequency * 16.0                                                # the pitch of the sweep's last blocks
    tail = slice(-8 * frames, None)
    print(f'{blocks} blocks of {frames} frames -> {args.output}: an organ chord on {args.frequency:g} Hz, a saw swept to {top:g} Hz')
    print(f'  peak: organ {np.abs(out[:, 0]).max():.3f}, saw {np.abs(out[:, 1]).max():.3f}')
    for name, x in (('ext.Additive', out[tail, 1]), ('osc.Sawtooth', ref[tail, 0])):
        print(f'  {name:13s} energy between the harmonics at the top of the sweep: {off_harmonic_share(x, top, rate):.2e}')
    return pathlib.Path(args.output)


if __name__ == '__main__':
    main()
