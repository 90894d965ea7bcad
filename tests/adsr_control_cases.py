"""The ADSR parameter set of the block-rate envelope tests (tests/test_control_adsr_host.py, tests/test_gpu_control_adsr.py):
five voices as a mix of (1, 1) and (1, V) rows -- every stage non-zero, one each with attack, decay and release of zero length,
one released inside its attack -- with gate times that put stage boundaries exactly on block starts, and the nodes built from it."""
import numpy as np

from helpers import HOUR, RATE

PARAMS = ('attack', 'decay', 'sustain', 'release', 'gate_on', 'gate_off')
V = 5
POSITIONS = (0, 1, 37, 100, 101, HOUR)


def rows(N=256, position=0, voices=V):
    """{name: (1, 1) | (1, voices) float64 row} for blocks of N frames: gate_on = 2 N / rate for every voice (a (1, 1) row: the
    start of block 2), voice 0's attack N / rate long (it ends on the start of block 3), every other time a fraction of N / rate so
    that the whole envelope passes inside nine blocks; `position` = HOUR moves both gates an hour on.  More than five voices repeat
    the five with the gate lengths stretched a little from copy to copy."""
    b = N / RATE                                                # one block in seconds
    reps = -(-voices // V)
    stretch = np.repeat(1.0 + 0.03 * np.arange(reps), V)[:voices]
    tile = lambda v: np.tile(np.array(v, dtype=np.float64), reps)[:voices]
    on = 2 * N / RATE + (HOUR / RATE if position >= HOUR else 0.0)
    #                 all stages     attack 0   decay 0    release 0   released inside the attack
    attack = tile([b,              0.0,       0.6 * b,   0.9 * b,    4.0 * b])
    decay = tile([1.5 * b,         0.8 * b,   0.0,       1.1 * b,    1.0 * b])
    release = tile([2.0 * b,       1.3 * b,   1.7 * b,   0.0,        1.5 * b])
    length = tile([4.0 * b,        3.0 * b,   2.0 * b,   2.5 * b,    0.75 * b]) * stretch
    return {'attack': attack[None, :], 'decay': decay[None, :], 'sustain': np.array([[0.6]]), 'release': release[None, :],
            'gate_on': np.array([[on]]), 'gate_off': (on + length)[None, :]}


def node(p):
    """the ext.ADSR over the rows `p` (a port whose row is None stays unplugged)"""
    from helpers import fix
    from signals_amd.chain import ext
    env = ext.ADSR()
    for name in PARAMS:
        if p.get(name) is not None:
            setattr(env, name, fix(p[name]))
    return env


def oracle(p, positions):
    """(len(positions), V) float64: oracle.chain_ref.adsr at one frame each"""
    from oracle import chain_ref as R
    return np.concatenate([R.adsr(int(q), 1, RATE, **{k: p[k] for k in PARAMS}) for q in positions])
