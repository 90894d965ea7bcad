"""Filters and White in block-rate control programs, without a GPU: which instructions are window-rate and how registers are
numbered, the specialised build's description words and image, and the NotBatchable messages of the shapes left to the eager
path."""
import numpy as np
import pytest

from signals_amd import _native, specialise
from signals_amd.chain import fixed, fx, noise, osc
from signals_amd.engine import NotBatchable, _ControlProgram

OPS = {v: k for k, v in _native.CTL_OPS.items()}


def fix(v):
    f = fixed.Fixed()
    f.get_state().value = np.array(v, ndmin=2, dtype=float)
    return f


def smoothed(V=1, ftype='LowPass'):
    """Mix(Gain(Filter(Square), scale), offset, 0.5)"""
    sq = osc.Square(); sq.hertz = fix([[3.0] * V])
    f = getattr(fx, ftype)(); f.input = sq; f.cutoff = fix([[4.0] * V])
    g = fx.Gain(); g.left = f; g.right = fix([[2700.0]])
    m = fx.Mix(); m.left = g; m.right = fix([[600.0]]); m.mix = fix([[0.5]])
    return m, f


def layout(prog):
    return [(OPS[x.op], x.reserved, x.a, x.b, x.c, x.dst, x.cols) for x in prog.ins]


def test_filter_program_layout():
    m, _ = smoothed(V=2)
    prog = _ControlProgram((m,), 4, channels=2)
    assert prog.windowed
    # rows first (the one-column ones: the Square's unplugged phase, scale, offset, mix; then cutoff and hertz), the window run
    # (the Square), the filter, then the block-rate scaling; registers renumbered in that order
    assert layout(prog) == [('Row', 0, -1, -1, -1, 0, 1), ('Row', 0, -1, -1, -1, 1, 1), ('Row', 0, -1, -1, -1, 2, 1),
                            ('Row', 0, -1, -1, -1, 3, 1), ('Row', 0, -1, -1, -1, 4, 2), ('Row', 0, -1, -1, -1, 5, 2),
                            ('Osc', 1, 5, 0, -1, 6, 2), ('Filter', 0, 6, 4, -1, 7, 2), ('Gain', 0, 7, 1, -1, 8, 2),
                            ('Mix', 0, 8, 2, 3, 9, 2)]
    assert prog.ins[7].kind == _native.FILT_TYPES['lp']
    assert _ControlProgram((smoothed(V=2, ftype='HighPass')[0],), 4, channels=2).ins[7].kind == _native.FILT_TYPES['hp']


def test_description_marks_window_rate_instructions():
    m, _ = smoothed(V=1)
    prog = _ControlProgram((m,), 4, channels=1)
    words = prog.description
    assert words[:2] == [len(prog.ins), 1]
    wide = [words[2 + 7 * k + 6] for k in range(len(prog.ins))]
    assert wide == [0, 0, 0, 0, 0, 0, 2, 0, 0, 0]                 # bit 1: window-rate; one column throughout
    assert specialise.control_flags(words)[0].startswith('-DSIG_CTL_STATIC_INS={{0,0,-1,-1,-1,0,0},')


def test_noise_instruction_carries_its_seed():
    w = noise.White(); w.get_state().channels = 3; w.get_state().seed = 12345
    f = fx.LowPass(); f.input = w; f.cutoff = fix([[1.0] * 3])
    prog = _ControlProgram((f,), 2, channels=3)
    kinds = [(OPS[x.op], x.reserved, x.cols) for x in prog.ins]
    assert kinds == [('Row', 0, 3), ('Noise', 1, 3), ('Filter', 0, 3)]
    assert prog.ins[1].row == 12345
    block_rate = _ControlProgram((w,), 2, channels=3)
    assert [(OPS[x.op], x.reserved) for x in block_rate.ins] == [('Noise', 0)] and block_rate.windowed


def test_programs_without_filters_keep_their_words():
    s = osc.Sine(); s.hertz = fix([[2.0]])
    g = fx.Gain(); g.left = s; g.right = fix([[3.0, 4.0]])
    prog = _ControlProgram((g,), 8)
    assert not prog.windowed
    assert prog.description == [5, 1, 0, 0, -1, -1, -1, 0, 0, 0, 0, -1, -1, -1, 1, 0, 0, 0, -1, -1, -1, 2, 1,
                                1, 0, 0, 1, -1, 3, 0, 2, 0, 3, 2, -1, 4, 1, 4, 1]


@pytest.mark.skipif(specialise.hipcc() is None, reason='no hipcc in this environment')
def test_the_specialised_filter_program_builds(tmp_path, monkeypatch):
    monkeypatch.setattr(specialise, 'CACHE', tmp_path)
    m, _ = smoothed(V=1)
    w = noise.White(); w.get_state().channels = 4
    f = fx.HighPass(); f.input = w; f.cutoff = fix([[2.0] * 4])
    for prog in (_ControlProgram((m,), 4, channels=1), _ControlProgram((f,), 4, channels=4)):
        image = specialise._compile('control_program.hip', specialise.control_flags(prog.description), 'ctl')
        assert b'sig_ctl_specialised' in image


def message(src, channels=2):
    with pytest.raises(NotBatchable) as e:
        _ControlProgram((src,), 4, channels=channels)
    return str(e.value)


def test_out_of_scope_messages():
    m, f = smoothed(V=2)
    inner = fx.LowPass(); inner.input = f.input.sig; inner.cutoff = fix([[9.0] * 2]); f.input = inner
    assert 'input contains a filter' in message(m)
    m, f = smoothed(V=2)
    f.input.sig.hertz = osc.Sine()
    assert 'modulated hertz' in message(m)
    m, f = smoothed(V=2)
    r = fx.RingMod(); r.left = f.input.sig; r.right = fix([[1.0]])
    assert 'reader outside that filter' in message(m)
    b = fx.BandPass(); b.input = osc.Sine(); b.low = fix([[100.0]]); b.high = fix([[200.0]])
    assert 'only LowPass / HighPass' in message(b)
    m, _ = smoothed(V=1)
    assert 'narrower than its request' in message(m, channels=2)
    assert 'request width is not known' in message(smoothed(V=2)[0], channels=None)
