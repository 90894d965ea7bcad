#!/usr/bin/env python3
"""A sampler, headless: one synthetic recording (a decaying sine burst, made here) played as a chord -- every voice its own `ratio`,
trigger time and start -- shaped by `RingMod(Sampler, ADSR)` with the same `gate_on`, panned under a stereo `SumBus` and written to a
WAV file by `FileWriter`.  The chord is a stack of just intervals over the recording's own pitch, each note struck a little after
the one below; with --loop the burst's tail is looped and the envelope's release ends the note.

    python scripts/example_sampler.py [-o PATH] [-s SECONDS] [-n VOICES] [--loop]        (needs a GPU)
"""
import argparse
import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

RATE = 48000
INTERVALS = (1.0, 5.0 / 4.0, 3.0 / 2.0, 15.0 / 8.0, 2.0, 5.0 / 2.0, 3.0, 15.0 / 4.0)      # a major seventh chord, two octaves


def fixed(v):
    from signals_amd.chain.fixed import Fixed
    f = Fixed()
    f.get_state().value = np.array(v, ndmin=2, dtype=float)
    return f


def recording(seconds: float = 0.75, hertz: float = 220.0, rate: int = RATE) -> np.ndarray:
    """(T, 1): a sine burst with two overtones and an exponential decay, within +-1, ending in silence"""
    t = np.arange(int(seconds * rate)) / rate
    tone = np.sin(2 * np.pi * hertz * t) + 0.4 * np.sin(2 * np.pi * 2 * hertz * t) + 0.2 * np.sin(2 * np.pi * 3 * hertz * t)
    burst = tone * np.exp(-5.0 * t) * np.minimum(t * 400.0, 1.0) * np.minimum((t[-1] - t) * 400.0, 1.0)
    return (burst / np.abs(burst).max())[:, None]


def chord(voices: int, table: np.ndarray, loop: bool = False, strum: float = 0.03):
    """SumBus(RingMod(Sampler, ADSR)) over `voices` voices: (the bus, the per-voice ratios)"""
    from signals_amd.chain.ext import ADSR, Sampler, SumBus
    from signals_amd.chain.fx import RingMod
    v = np.arange(voices)
    ratio = np.array([INTERVALS[k % len(INTERVALS)] * 2.0 ** (k // len(INTERVALS) % 2) for k in v])[None, :]
    gate = (v * strum / max(voices / len(INTERVALS), 1.0))[None, :]            # struck one after the other
    s = Sampler()
    s.get_state().table = table
    if loop:
        s.get_state().loop_end = int(table.shape[0] * 0.6)
        s.get_state().loop_start = int(table.shape[0] * 0.3)
    s.ratio, s.gate_on, s.offset = fixed(ratio), fixed(gate), fixed(np.zeros((1, voices)))
    env = ADSR()
    for name, value in (('attack', 0.002), ('decay', 0.3), ('sustain', 0.5), ('release', 0.25)):
        setattr(env, name, fixed([[value]]))
    env.gate_on, env.gate_off = fixed(gate), fixed(gate + (1.5 if loop else 0.5))
    shaped = RingMod(); shaped.left = s; shaped.right = env
    th = np.linspace(0.15, 0.85, voices) * np.pi / 2
    bus = SumBus(); bus.input = shaped
    bus.get_state().gains = np.ascontiguousarray(np.stack([np.cos(th), np.sin(th)]) / max(voices, 1) * 2.0)
    return bus, ratio


def main(argv=None) -> pathlib.Path:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('-o', '--output', default='sampler.wav')
    parser.add_argument('-s', '--seconds', type=float, default=3.0)
    parser.add_argument('-n', '--voices', type=int, default=8)
    parser.add_argument('--loop', action='store_true', help='loop the middle of the recording; the release ends the note')
    args = parser.parse_args(argv)

    from signals_amd import runtime
    from signals_amd.chain.files import FileWriter
    from signals_amd.engine import BatchRenderer
    runtime.set_device('cuda:0')

    frames = 256
    table = recording()
    bus, ratio = chord(args.voices, table, args.loop)
    writer = FileWriter(); writer.input = bus
    writer.get_state().path = str(args.output)
    writer.get_state().subtype = 'FLOAT'
    blocks = int(np.ceil(args.seconds * RATE / frames))
    out = BatchRenderer(writer, 2, RATE).render(0, frames, blocks).cpu().numpy()
    writer.destroy()
    print(f'{blocks} blocks of {frames} frames -> {args.output}: a {table.shape[0]}-frame recording on {args.voices} voices at ratios '
          f'{", ".join(f"{r:.3f}" for r in ratio[0, :8])}{" ..." if args.voices > 8 else ""}{", looped" if args.loop else ""}')
    print(f'  peak {np.abs(out).max():.3f}, rms left {np.sqrt(np.mean(out[:, 0] ** 2)):.4f} right {np.sqrt(np.mean(out[:, 1] ** 2)):.4f}')
    return pathlib.Path(args.output)


if __name__ == '__main__':
    main()
