#!/usr/bin/env python3
"""A band-limited sawtooth against the naive one, headless: `ext.Wavetable` reading one period of a saw built from the harmonics
below Nyquist, and `osc.Sawtooth` (the closed-form shape, which aliases), at the same pitch; the two are written to the left and
right channel of a WAV file by `FileWriter`, and the energy each puts between the harmonics (aliasing) is printed.

    python scripts/example_wavetable.py [FREQUENCY] [-o PATH] [-s SECONDS] [-t POINTS]        (needs a GPU)
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


def band_limited_saw(points: int, harmonics: int) -> np.ndarray:
    """(points, 1): the first `harmonics` partials of a sawtooth rising from -1 to 1, one period starting at its zero crossing"""
    k = np.arange(points)[:, None] / points
    h = np.arange(1, harmonics + 1)[None, :]
    return 2.0 / np.pi * np.sum(np.sin(2.0 * np.pi * k * h) / h * (-1.0) ** (h + 1), axis=1, keepdims=True)


def off_harmonic_share(x: np.ndarray, frequency: float, rate: int) -> float:
    """share of the signal's energy that lies further than 2 % of the fundamental from every harmonic"""
    spectrum = np.abs(np.fft.rfft(x * np.hanning(len(x)))) ** 2
    freqs = np.fft.rfftfreq(len(x), 1.0 / rate)
    distance = np.abs(freqs / frequency - np.round(freqs / frequency))
    return float(spectrum[(distance > 0.02) & (freqs > frequency / 2)].sum() / spectrum.sum())


def main(argv=None) -> pathlib.Path:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('frequency', nargs='?', type=float, default=1661.0, help='pitch in Hz (default: %(default)s)')
    parser.add_argument('-o', '--output', default='saws.wav')
    parser.add_argument('-s', '--seconds', type=float, default=2.0)
    parser.add_argument('-t', '--points', type=int, default=2048, help='table length, a power of two (default: %(default)s)')
    args = parser.parse_args(argv)

    from signals_amd import runtime
    from signals_amd.chain.ext import Wavetable
    from signals_amd.chain.files import FileWriter
    from signals_amd.chain.fx import Gain
    from signals_amd.chain.osc import Sawtooth
    from signals_amd.chain.shape import Merge
    from signals_amd.engine import BatchRenderer
    runtime.set_device('cuda:0')

    rate, frames = 48000, 256
    harmonics = max(1, int((rate / 2 - 1) // args.frequency))                 # every partial below Nyquist
    table = Wavetable(); table.hertz = fixed([[args.frequency]]); table.phase = fixed([[0.5]])       # (the naive saw crosses zero at t = 1/2)
    table.get_state().table = band_limited_saw(args.points, harmonics)
    naive = Sawtooth(); naive.hertz = fixed([[args.frequency]])
    both = Merge(); both.left = table; both.right = naive
    level = Gain(); level.left = both; level.right = fixed([[0.5]])
    writer = FileWriter(); writer.input = level
    writer.get_state().path = str(args.output)
    writer.get_state().subtype = 'FLOAT'

    blocks = int(np.ceil(args.seconds * rate / frames))
    out = BatchRenderer(writer, 2, rate).render(0, frames, blocks).cpu().numpy()
    writer.destroy()
    print(f'{blocks} blocks of {frames} frames -> {args.output}: {harmonics} harmonics in a table of {args.points} points')
    for name, column in (('wavetable', 0), ('osc.Sawtooth', 1)):
        print(f'  {name:13s} energy between the harmonics: {off_harmonic_share(out[:, column], args.frequency, rate):.2e}')
    return pathlib.Path(args.output)


if __name__ == '__main__':
    main()
