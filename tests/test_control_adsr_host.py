"""ext.ADSR in block-rate control programs, without a GPU: the AdsrArgs / Adsr pair's layout and description words, the header's
enum, window-rate marking and refusals, the specialised image, programs without the word, and sig_adsr.h's make_voice + level
compiled for the host against the definition (oracle/chain_ref.py:adsr), bit for bit."""
import pathlib
import re
import shutil
import subprocess

import numpy as np
import pytest

import adsr_control_cases as A
from helpers import HOUR, RATE, fix, mkosc
from signals_amd import _native, specialise
from signals_amd.chain import ext, fx
from signals_amd.engine import NotBatchable, _ControlProgram

ROOT = pathlib.Path(__file__).resolve().parent.parent
OPS = {v: k for k, v in _native.CTL_OPS.items()}


def layout(prog):
    return [(OPS[x.op], x.reserved, x.a, x.b, x.c, x.dst, x.cols) for x in prog.ins]


def envelope(wide='attack', V=3):
    """an ADSR over Fixed rows, one of them V columns wide"""
    p = {'attack': [[0.01]], 'decay': [[0.02]], 'sustain': [[0.5]], 'release': [[0.03]], 'gate_on': [[0.0]], 'gate_off': [[0.1]]}
    p = {k: np.array(v) for k, v in p.items()}
    p[wide] = np.repeat(p[wide], V, axis=1)
    return A.node(p)


def swept(env):
    m = fx.Mix(); m.left = fix([[6000.0]]); m.right = fix([[300.0]]); m.mix = env
    return m


def test_program_layout():
    prog = _ControlProgram((swept(envelope()),), 4)
    # rows first (the one-column ones: Mix's two, then decay .. gate_off; then the wide attack), the carrier with release / gate_on /
    # gate_off right in front of the ADSR with attack / decay / sustain, then the Mix; registers renumbered in that order
    assert layout(prog) == [('Row', 0, -1, -1, -1, k, 1) for k in range(7)] + [
        ('Row', 0, -1, -1, -1, 7, 3), ('AdsrArgs', 0, 4, 5, 6, 8, 3), ('Adsr', 0, 7, 2, 3, 9, 3), ('Mix', 0, 0, 1, 9, 10, 3)]
    assert prog.envelope and not prog.windowed
    words = prog.description
    assert words[:2] == [11, 1] and len(words) == 2 + 7 * 11 + 2
    assert words[2 + 7 * 8: 2 + 7 * 11] == [8, 0, 4, 5, 6, 8, 1, 9, 0, 7, 2, 3, 9, 1, 3, 0, 0, 1, 9, 10, 1]
    assert words[-2:] == [10, 1]
    flags = specialise.control_flags(words)
    assert ',{8,0,4,5,6,8,1},{9,0,7,2,3,9,1},{3,0,0,1,9,10,1}}' in flags[0] and flags[1] == '-DSIG_CTL_STATIC_OUTS={{10,1}}'


def test_unplugged_ports_read_the_zero_row():
    env = ext.ADSR(); env.attack = fix([[0.01]]); env.gate_off = fix([[0.5, 0.6]])
    prog = _ControlProgram((env,), 2)
    # attack, the shared zero row, gate_off (wide)
    assert layout(prog) == [('Row', 0, -1, -1, -1, 0, 1), ('Row', 0, -1, -1, -1, 1, 1), ('Row', 0, -1, -1, -1, 2, 2),
                            ('AdsrArgs', 0, 1, 1, 2, 3, 2), ('Adsr', 0, 0, 1, 1, 4, 2)]


def test_a_disabled_envelope_answers_the_zero_row():
    env = envelope(); env.get_state().enabled = False
    prog = _ControlProgram((env,), 2)
    assert prog.ins == [] and tuple(prog.results[0].shape) == (1, 1) and not prog.results[0].any()


def test_enum_agreement():
    header = (ROOT / 'include' / 'signals_amd.h').read_text()
    found = {name: int(value) for name, value in re.findall(r'SIG_CTL_([A-Z]+) = (\d+)', header) if not name.startswith('MAX')}
    assert found == {k.upper(): v for k, v in _native.CTL_OPS.items()}
    assert set(_native.CTL_ENVELOPE_OPS) == {_native.CTL_OPS['AdsrArgs'], _native.CTL_OPS['Adsr']}
    assert _native.CTL_OPS['AdsrArgs'] + 1 == _native.CTL_OPS['Adsr']
    assert 'int sig_control_program_envelope(' in header and 'sig_control_program_envelope' in _native.EXPORTS


def slewed(env, V=3):
    f = fx.LowPass(); f.input = env; f.cutoff = fix([[30.0] * V])
    return f


def test_window_rate_marking():
    prog = _ControlProgram((slewed(envelope()),), 4, channels=3)
    assert prog.windowed and prog.envelope
    ops = [(OPS[x.op], x.reserved) for x in prog.ins]
    assert ops == [('Row', 0)] * 7 + [('AdsrArgs', 1), ('Adsr', 1), ('Filter', 0)]
    wide = [prog.description[2 + 7 * k + 6] for k in range(len(prog.ins))]
    assert wide[-3:] == [3, 3, 1]                                   # bit 1: window-rate, on both halves of the pair


def test_refusals():
    env = envelope()
    env.attack = mkosc('Sine', [[0.5] * 3])
    with pytest.raises(NotBatchable, match=r'ADSR inside a control filter\'s input has a modulated attack'):
        _ControlProgram((slewed(env),), 4, channels=3)
    env = envelope()
    env.attack = mkosc('Sine', [[0.5] * 3])
    prog = _ControlProgram((swept(env),), 4)                        # the same envelope outside a filter: its attack is a register
    assert [OPS[x.op] for x in prog.ins][-4:] == ['Osc', 'AdsrArgs', 'Adsr', 'Mix']


def test_a_malformed_pair_is_refused_before_it_is_uploaded():
    I = lambda op, a, b, c, dst: _native.CtlIns(_native.CTL_OPS[op], 0, a, b, c, dst, 0, 0, 1, 0, None)
    row = lambda dst: _native.CtlIns(_native.CTL_OPS['Row'], 0, -1, -1, -1, dst, 0, 1, 1, 0, None)
    out = [_native.CtlOut(2, 1, None, None)]
    _native.control_program_description([row(0), I('AdsrArgs', 0, 0, 0, 1), I('Adsr', 0, 0, 0, 2)], out)
    for bad in ([row(0), I('Adsr', 0, 0, 0, 1)], [I('Adsr', -1, -1, -1, 0)], [row(0), I('AdsrArgs', 0, 0, 0, 1)],
                [row(0), I('AdsrArgs', 0, 0, 0, 1), I('Gain', 0, 0, -1, 2), I('Adsr', 0, 0, 0, 3)]):
        with pytest.raises(ValueError, match='pair'):
            _native.control_program_description(bad, out)


def test_attach_checks_the_pairs_of_its_description():
    """the entry reads the description on the host, before it touches the image or a device: a malformed pair is
    hipErrorInvalidValue (1)"""
    row, out = [0, 0, -1, -1, -1, 0, 0], [2, 0]
    for bad in ([2, 1] + row + [9, 0, 0, 0, 0, 1, 0] + [1, 0],                                  # no carrier
                [3, 1] + row + [8, 0, 0, 0, 0, 1, 0] + [2, 0, 0, 0, -1, 2, 0] + out,            # a carrier without its ADSR
                [3, 1] + row + [8, 0, 0, 0, 0, 1, 2] + [9, 0, 0, 0, 0, 2, 0] + out,             # the halves at different rates
                [2, 1] + row + [8, 0, 0, 0, 0, 1, 0] + [1, 0]):                                 # a carrier at the end
        with pytest.raises(_native.NativeError, match=r'hipError_t 1$'):
            _native.control_program_attach(bad, b'never read')


def test_programs_without_the_word_keep_their_words():
    s = mkosc('Sine', [[2.0]])
    g = fx.Gain(); g.left = s; g.right = fix([[3.0, 4.0]])
    prog = _ControlProgram((g,), 8)
    assert not prog.windowed and not prog.envelope
    assert prog.description == [5, 1, 0, 0, -1, -1, -1, 0, 0, 0, 0, -1, -1, -1, 1, 0, 0, 0, -1, -1, -1, 2, 1,
                                1, 0, 0, 1, -1, 3, 0, 2, 0, 3, 2, -1, 4, 1, 4, 1]


@pytest.mark.skipif(specialise.hipcc() is None, reason='no hipcc in this environment')
def test_the_specialised_envelope_program_builds(tmp_path, monkeypatch):
    monkeypatch.setattr(specialise, 'CACHE', tmp_path)
    for prog in (_ControlProgram((swept(envelope()),), 4), _ControlProgram((slewed(envelope()),), 4, channels=3)):
        image = specialise._compile('control_program.hip', specialise.control_flags(prog.description), 'ctl')
        assert b'sig_ctl_specialised' in image


@pytest.mark.skipif(specialise.hipcc() is None, reason='no hipcc in this environment')
def test_the_specialised_build_refuses_a_lone_adsr(tmp_path, monkeypatch):
    monkeypatch.setattr(specialise, 'CACHE', tmp_path)
    words = [2, 1, 0, 0, -1, -1, -1, 0, 0, 9, 0, 0, 0, 0, 1, 0, 1, 0]
    with pytest.raises(specialise.SpecialiseError):
        specialise._compile('control_program.hip', specialise.control_flags(words), 'ctl')


# ---------------------------------------------------------------- the arithmetic, on the host
@pytest.fixture(scope='module')
def level(tmp_path_factory):
    """make_voice + level built against a COPY of sig_adsr.h next to the stub sig_common.h (tests/test_adsr_tracker_host.py)"""
    cxx = shutil.which('g++') or shutil.which('c++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('adsr_level')
    shutil.copy(ROOT / 'signals_amd' / 'csrc' / 'sig_adsr.h', d / 'sig_adsr.h')
    for name in ('sig_common.h', 'adsr_level.cpp'):
        shutil.copy(ROOT / 'tests' / 'native' / name, d / name)
    exe = d / 'adsr_level'
    subprocess.run([cxx, '-std=c++17', '-O2', '-ffp-contract=off', '-I', str(d), str(d / 'adsr_level.cpp'), '-o', str(exe)],
                   check=True, capture_output=True, text=True)

    def run(p, positions):
        full = np.stack([np.broadcast_to(p[k], (1, A.V)).reshape(-1) for k in A.PARAMS]).astype(np.float64)
        blob = [np.array([A.V, len(positions)], dtype=np.int64).tobytes(), np.array([RATE], dtype=np.float64).tobytes(),
                full.tobytes(), np.asarray(positions, dtype=np.int64).tobytes()]
        (d / 'in.bin').write_bytes(b''.join(blob))
        subprocess.run([str(exe), str(d / 'in.bin'), str(d / 'out.bin')], check=True, timeout=60)
        return np.fromfile(d / 'out.bin', dtype=np.float64).reshape(len(positions), A.V)
    return run


@pytest.mark.parametrize('pos', A.POSITIONS)
def test_host_arithmetic_equals_the_definition(level, pos):
    N, K = 256, 9
    p = A.rows(N, pos)
    positions = [pos + b * N for b in range(K)] + list(range(pos, pos + K * N, 7))
    got, want = level(p, positions), A.oracle(p, positions)
    assert want.shape == (len(positions), A.V)
    assert len({float(x) for x in want.reshape(-1)}) > 50           # (the envelopes move inside the window)
    assert np.array_equal(got, want)


def test_the_parameter_set_puts_boundaries_on_block_starts():
    N = 256
    p = A.rows(N, 0)
    assert p['gate_on'][0, 0] == (2 * N) / RATE and p['gate_on'][0, 0] + p['attack'][0, 0] == (3 * N) / RATE
    assert (p['attack'] == 0).any() and (p['decay'] == 0).any() and (p['release'] == 0).any()
    assert ((p['gate_off'] - p['gate_on']) < p['attack']).any()
    assert {r.shape for r in p.values()} == {(1, 1), (1, A.V)}
    assert A.rows(N, HOUR)['gate_on'][0, 0] == p['gate_on'][0, 0] + HOUR / RATE
