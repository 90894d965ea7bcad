#!/usr/bin/env python3
"""A sine through two transfer curves, headless: `ext.Shaper` with a tanh(d x) / tanh(d) saturator on the left channel and the
degree-3 Chebyshev polynomial on the right (a full-scale sine comes out as its third harmonic), written to a WAV file by
`FileWriter`; the level of the first five harmonics of each channel is printed.

    python scripts/example_shaper.py [FREQUENCY] [-o PATH] [-s SECONDS] [-d DRIVE] [-t POINTS]        (needs a GPU)
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


def curves(points: int, drive: float) -> np.ndarray:
    """(points, 2): column 0 tanh(drive x) / tanh(drive), column 1 the Chebyshev polynomial T3 = 4 x^3 - 3 x, over -1 .. +1"""
    x = np.linspace(-1.0, 1.0, points)
    return np.stack([np.tanh(drive * x) / np.tanh(drive), 4.0 * x ** 3 - 3.0 * x], axis=1)


def harmonic_levels(x: np.ndarray, frequency: float, rate: int, count: int = 5) -> list:
    """the first `count` harmonics in dB relative to the strongest of them"""
    spectrum = np.abs(np.fft.rfft(x * np.hanning(len(x))))
    freqs = np.fft.rfftfreq(len(x), 1.0 / rate)
    peaks = np.array([spectrum[np.abs(freqs - h * frequency) < frequency / 4].max() for h in range(1, count + 1)])
    return [round(float(v), 1) for v in 20.0 * np.log10(np.maximum(peaks, 1e-12) / peaks.max())]


def main(argv=None) -> pathlib.Path:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('frequency', nargs='?', type=float, default=220.0, help='pitch in Hz (default: %(default)s)')
    parser.add_argument('-o', '--output', default='shaped.wav')
    parser.add_argument('-s', '--seconds', type=float, default=2.0)
    parser.add_argument('-d', '--drive', type=float, default=3.0, help='slope of the saturator at 0, before normalising (default: %(default)s)')
    parser.add_argument('-t', '--points', type=int, default=513, help='table length, 2^k + 1 puts a knot at 0 (default: %(default)s)')
    args = parser.parse_args(argv)

    from signals_amd import runtime
    from signals_amd.chain.ext import Shaper
    from signals_amd.chain.files import FileWriter
    from signals_amd.chain.fx import Gain
    from signals_amd.chain.osc import Sine
    from signals_amd.engine import BatchRenderer
    runtime.set_device('cuda:0')

    rate, frames = 48000, 256
    sine = Sine(); sine.hertz = fixed([[args.frequency]])
    shaper = Shaper(); shaper.input = sine; shaper.select = fixed([[0.0, 1.0]])      # one curve per channel
    shaper.get_state().table = curves(args.points, args.drive)
    level = Gain(); level.left = shaper; level.right = fixed([[0.5]])
    writer = FileWriter(); writer.input = level
    writer.get_state().path = str(args.output)
    writer.get_state().subtype = 'FLOAT'

    blocks = int(np.ceil(args.seconds * rate / frames))
    out = BatchRenderer(writer, 2, rate).render(0, frames, blocks).cpu().numpy()
    writer.destroy()
    print(f'{blocks} blocks of {frames} frames -> {args.output}: a {args.frequency} Hz sine through {args.points}-point curves')
    for name, column in ((f'tanh({args.drive} x)', 0), ('Chebyshev T3', 1)):
        print(f'  {name:13s} harmonics 1-5, dB: {harmonic_levels(out[:, column], args.frequency, rate)}')
    return pathlib.Path(args.output)


if __name__ == '__main__':
    main()
