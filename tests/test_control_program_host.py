"""The case table of tests/control_program_cases.py, checked without a GPU: every case passes `validate` (the gate in front of the
GPU), the table still holds every edge it was written for, `reference` equals the oracle's own graph evaluation read at block rate,
and `to_ctl` reproduces the struct layout of include/signals_amd.h."""
import ctypes
import pathlib
import re

import numpy as np
import pytest
import torch

import control_program_cases as K
from oracle import chain_ref as R

HEADER = pathlib.Path(__file__).resolve().parent.parent / 'include' / 'signals_amd.h'


@pytest.mark.parametrize('case', K.CASES, ids=lambda c: c.name)
def test_every_case_passes_validate(case):
    K.validate(case)


def test_validate_refuses_what_could_index_outside():
    base = K.BY_NAME['filter_2']
    edit = lambda k, **kw: base._replace(ins=base.ins[:k] + (base.ins[k]._replace(**kw),) + base.ins[k + 1:])
    broken = [edit(7, a=9), edit(7, dst=48), edit(0, data=np.zeros((1, 3))), edit(0, rows=2), edit(4, reserved=0),
              base._replace(outs=((8, 3, True),)), base._replace(outs=((4, 3, True),)), edit(6, a=1), edit(4, cols=1),
              base._replace(ins=base.ins * 7), base._replace(launch=base.launch._replace(cols=1))]
    for case in broken:
        with pytest.raises(AssertionError):
            K.validate(case)
    pair = K.BY_NAME['adsr_2']
    k = next(k for k, i in enumerate(pair.ins) if i.op == K.ADSRARGS)
    with pytest.raises(AssertionError):
        K.validate(pair._replace(ins=pair.ins[:k] + (pair.ins[k]._replace(op=K.GAIN, c=-1),) + pair.ins[k + 1:]))
    with pytest.raises(AssertionError):                      # rows = nblocks beside a front position
        K.validate(K.BY_NAME['rows_per_block_3']._replace(launch=K.BY_NAME['rows_per_block_3'].launch._replace(front_position=5)))


def test_names_are_unique_and_structures_are_shared():
    assert len(K.BY_NAME) == len(K.CASES)
    structures = {}
    for case in K.CASES:
        if case.structure is not None:
            structures.setdefault(case.structure, set()).add(structure_of(case))
    assert set(structures) == set(K.SPECIALISED) and len(K.SPECIALISED) <= 10
    assert all(len(v) == 1 for v in structures.values()), {k: len(v) for k, v in structures.items()}


def structure_of(case) -> tuple:
    """what a specialised build is keyed by (`_native.control_program_description`)"""
    return (tuple((i.op, i.kind, i.a, i.b, i.c, i.dst, (1 if i.cols > 1 else 0) | (2 if i.reserved else 0)) for i in case.ins),
            tuple((reg, 1 if cols > 1 else 0) for reg, cols, _ in case.outs))


def test_the_edges_the_table_is_there_for():
    by_group = lambda g: [c for c in K.CASES if c.group == g]
    ops = lambda c: {i.op for i in c.ins}
    # every op, every variant, every waveform at block rate and at window rate, both filter kinds on both paths
    assert set().union(*(ops(c) for c in K.CASES)) == set(range(10))
    assert {K.variant_of(c) for c in K.CASES} == set(K.VARIANTS)
    for win in (0, 1):
        assert {i.kind for c in K.CASES for i in c.ins if i.op == K.OSC and i.reserved == win} == set(K.OSC_NAMES)
        assert {i.op for c in K.CASES for i in c.ins if i.reserved == win} >= {K.OSC, K.GAIN, K.MIX, K.NOISE, K.ADSRARGS, K.ADSR}
    assert {(i.kind, i.cols > 1) for c in K.CASES for i in c.ins if i.op == K.FILTER} == {(0, False), (0, True), (1, False), (1, True)}
    # columns: the four programs at every chunk edge of both kernels; outputs of three widths in one launch at 257
    for prefix, need in (('plain', set()), ('filter', {K.FILTER, K.OSC, K.RINGMOD}), ('noise', {K.NOISE}), ('adsr', {K.ADSR})):
        cases = {c.launch.cols: c for c in by_group('columns') if c.name.split('_')[0] == prefix and c.launch.rate == 48000}
        assert set(cases) == set(K.COLS) == {1, 2, 127, 128, 129, 255, 256, 257, 300}, prefix
        assert all(need <= ops(c) for c in cases.values()), prefix
        assert all(any(i.cols == c.launch.cols and i.op in need for i in c.ins) for c in cases.values() if need), prefix
    assert [cols for _, cols, _ in K.BY_NAME['plain_257'].outs] == [1, 129, 257]
    assert {c.launch.cols for c in by_group('columns') if c.launch.rate == 44100} == set(K.COLS)
    wide_filter = next(i for i in K.BY_NAME['filter_257'].ins if i.op == K.FILTER)
    assert [K.BY_NAME['filter_257'].ins[w].op for w in K.window_runs(K.BY_NAME['filter_257'])[wide_filter.dst]] == [K.OSC, K.RINGMOD]
    # window length: every h in 0 .. 100 on the one-column path (both kinds) and the wide one; the named positions; 44100 once
    narrow = lambda c: all(i.cols == 1 for i in c.ins if i.op == K.FILTER)
    for name in ('sweep_narrow_lp', 'sweep_narrow_hp', 'sweep_wide_lp', 'sweep_narrow_lp_44100'):
        c = K.BY_NAME[name]
        assert K.window_lengths(c) == set(range(101)) and c.launch.nblocks == 103 and narrow(c) == ('narrow' in name), name
    assert K.BY_NAME['sweep_wide_lp'].launch.cols == 3 and K.BY_NAME['sweep_narrow_lp_44100'].launch.rate == 44100
    met = {c.launch.position for c in by_group('window length') if narrow(c) and c.launch.step == 256 and c.launch.nblocks == 3}
    assert met == {2, 99, 100, 101, 2 ** 31 - 300, 2 ** 40 - 17}
    # window contents: a run of three (Osc, Gain by a ROW, Mix with a ROW) per waveform, window-rate Noise, a window-rate ADSR pair,
    # filters with separate runs (narrow and wide) each followed by a block-rate Gain / Mix
    c = K.BY_NAME['windows_5']
    runs = K.window_runs(c)
    shapes = {tuple(c.ins[w].op for w in run) for run in runs.values()}
    assert shapes == {(K.OSC, K.GAIN, K.MIX), (K.NOISE,)} and len(runs) == 5
    assert {c.ins[f].cols > 1 for f in runs} == {False, True}
    assert all(c.ins[f + 1].op in (K.GAIN, K.MIX) and not c.ins[f + 1].reserved and f in (c.ins[f + 1].a, c.ins[f + 1].b) for f in runs)
    c = K.BY_NAME['adsr_window_3']
    assert {tuple(c.ins[w].op for w in run) for run in K.window_runs(c).values()} == {(K.ADSRARGS, K.ADSR)}
    # rows: rows = 1 with stride 0 and 1; rows = nblocks with stride 0 and 1; a wide ROW narrower than the launch; no front there
    forms = {(i.rows > 1, i.stride) for c in K.CASES for i in c.ins if i.op == K.ROW}
    assert forms == {(False, 0), (False, 1), (True, 0), (True, 1)}
    for c in by_group('rows'):
        assert c.launch.front_position == -1 and any(i.rows == c.launch.nblocks > 1 for i in c.ins)
    assert any(i.op == K.ROW and 1 < i.cols < K.BY_NAME['rows_per_block_257'].launch.cols for i in K.BY_NAME['rows_per_block_257'].ins)
    # size: n_ins 1 and 2, every k0, 48 instructions in each variant with every op of the variant and three outputs
    assert {1, 2, K.MAX_INS} <= {len(c.ins) for c in by_group('size')}
    assert {K.leading_rows(c.ins) for c in by_group('size')} >= {0, 1, 3, 4, 5, 8}
    for variant, need in (('plain', set(range(6))), ('windowed', set(range(6)) | {K.FILTER}), ('envelope', set(range(6)) | {K.FILTER, K.ADSRARGS, K.ADSR})):
        c = K.BY_NAME[f'big_{variant}']
        assert len(c.ins) == 48 and K.variant_of(c) == variant and need <= ops(c) and len(c.outs) == 3 and K.leading_rows(c.ins) == 8
        assert {i.kind for i in c.ins if i.op == K.OSC} == set(K.OSC_NAMES)
        assert len(K.cone(c, c.outs[-1][0])) >= 40                            # a dependent chain, not 48 independent words
    # launch
    L = [c.launch for c in by_group('launch')]
    assert {1, 2, 9} <= {x.nblocks for x in L}
    assert any(x.nblocks == 0 and x.front_position >= 0 for x in L) and K.NO_OUTPUTS in K.BY_NAME
    for lo in (0, 37):
        clamped = {K.variant_of(c) for c in by_group('launch')
                   if c.launch[:4] == (48000, -300, 128, 6) and c.launch.min_position == lo}
        assert clamped == set(K.VARIANTS), lo
    assert any(x.front_position >= 0 and {f for _, _, f in c.outs} == {True, False} for c, x in zip(by_group('launch'), L))
    assert any(x.step == 0 for x in L)
    # operands: each operand of each two- and three-operand op in turn -1; NaNs and numbers under Amp
    c = K.BY_NAME['operands_300']
    absent = {(i.op, tuple(r == -1 for r in K.operands(i))) for i in c.ins if i.op not in (K.ROW,)}
    for op in (K.OSC, K.GAIN, K.RINGMOD, K.AMP):
        assert {(op, (True, False)), (op, (False, True))} <= absent, op
    assert {(K.MIX, (True, False, False)), (K.MIX, (False, True, False)), (K.MIX, (False, False, True))} <= absent
    amp = K.reference(c)[-1][0]
    assert np.isnan(amp).any() and np.isfinite(amp).any() and (amp[np.isfinite(amp)] < 0).all()
    # status: one bad column among 300, in the second chunk of the interpreter and the first of the specialised kernel
    bad, good = K.BY_NAME['status_bad'], K.BY_NAME['status_good']
    cut = lambda c: c.ins[next(i for i in c.ins if i.op == K.FILTER).b].data
    assert np.flatnonzero(cut(bad)[0] >= 24000).tolist() == [200] and (cut(good) < 22050).all() and (cut(good) > 0).all()
    assert all(i.data is True for c in (bad, good) for i in c.ins if i.op == K.FILTER)
    assert np.isnan(K.reference(bad)[1][0][:, 200]).all() and np.isfinite(np.delete(K.reference(bad)[1][0], 200, axis=1)).all()
    assert [what for what, _, _ in K.REFUSALS] == ['n_ins = 49', 'cols = 0', 'rate = 0', 'front_position = -2', 'min_position = -1']
    assert max(c.launch.nblocks * c.launch.cols for c in K.CASES) <= 103 * 300


def test_references_are_worth_comparing_with():
    for case in K.CASES:
        for (rows, front), (reg, cols, has_front) in zip(K.reference(case), case.outs):
            assert rows.shape == (case.launch.nblocks, cols) and (front is None or front.shape == (1, cols)), case.name
            assert (front is not None) == (has_front and case.launch.front_position >= 0), case.name
            if case.group not in ('operands', 'status'):
                assert np.isfinite(rows).all(), case.name
        if case.launch.nblocks * case.launch.cols >= 6 and case.launch.step > 0:
            assert any(len(np.unique(rows)) > 2 for rows, _ in K.reference(case)), case.name
    sweep = K.reference(K.BY_NAME['sweep_narrow_lp'])[1][0][:, 0]
    assert len(np.unique(sweep)) > 90                               # the filter moves with every further history row


# ------------------------------------------------------------------------------------------- reference == the oracle's graph
class Reply(R.Node):
    """the node of one instruction as the project's nodes answer: `cols` columns whatever the request's width (a narrower subgraph
    under a wider request), and float32 audio when the reply has more than one row (a filter's history rows)"""
    cached = False

    def __init__(self, inner, cols, audio):
        super().__init__()
        self.inner, self.cols, self.audio = inner, cols, audio

    def eval(self, position, frames, channels, rate):
        x = np.asarray(self.inner.respond(position, frames, self.cols, rate), dtype=np.float64)
        return x.astype(np.float32).astype(np.float64) if self.audio and frames > 1 else x


def graph_of(case, reg, made=None):
    """the oracle graph of an output register, or None where the program has no graph (a ROW with one row per block, an ADSR whose
    parameters are computed)"""
    made = {} if made is None else made
    if reg < 0:
        return None                                                  # an unplugged port answers zeros((1, 1)): a register of -1
    if reg in made:
        return made[reg]
    i = case.ins[reg]
    sub = lambda r: graph_of(case, r, made)
    missing = lambda *regs: any(r >= 0 and sub(r) is None for r in regs)
    node = None
    if i.op == K.ROW:
        node = R.Fixed(i.data) if i.rows == 1 else None
    elif i.op == K.OSC:
        node = None if missing(i.a, i.b) else R.Osc(K.OSC_NAMES[i.kind], sub(i.a), sub(i.b))
    elif i.op in (K.GAIN, K.RINGMOD, K.AMP, K.MIX):
        name = {K.GAIN: 'Gain', K.RINGMOD: 'RingMod', K.AMP: 'Amp', K.MIX: 'Mix'}[i.op]
        node = None if missing(i.a, i.b, i.c) else R.Binary(name, sub(i.a), sub(i.b), sub(i.c))
    elif i.op == K.NOISE:
        node = R.White(i.data, i.cols)
    elif i.op == K.ADSR:
        g = case.ins[reg - 1]
        regs = dict(zip(('attack', 'decay', 'sustain', 'release', 'gate_on', 'gate_off'), (i.a, i.b, i.c, g.a, g.b, g.c)))
        if all(r < 0 or (case.ins[r].op == K.ROW and case.ins[r].rows == 1) for r in regs.values()):
            node = R.Adsr(**{k: np.zeros((1, 1)) if r < 0 else case.ins[r].data for k, r in regs.items()})
    elif i.op == K.FILTER:
        node = None if missing(i.a, i.b) else R.Filter(K.FILT_NAMES[i.kind], sub(i.a), sub(i.b), closed_form=True, loop=True)
    if node is not None:
        node.cached = False        # (a cached multi-row reply, computed from float32 rows, must not answer a later one-row request)
    made[reg] = None if node is None else Reply(node, i.cols, bool(i.reserved))
    return made[reg]


GRAPH_CASES = [c for c in K.CASES if c.group != 'status' or c.name == 'status_good']


@pytest.mark.parametrize('case', GRAPH_CASES, ids=lambda c: c.name)
def test_reference_is_the_oracles_block_rate_read(case):
    L = case.launch
    made, compared = {}, 0
    for (rows, front), (reg, cols, _) in zip(K.reference(case), case.outs):
        node = graph_of(case, reg, made)
        if node is None:
            assert case.group in ('rows', 'size'), (case.name, reg)      # per-block rows; the 48-word chain's computed ADSR parameters
            continue
        with np.errstate(all='ignore'):
            want = [np.broadcast_to(node.respond(p, 1, cols, L.rate), (1, cols)) for p in K.frames_of(case)]
            assert np.array_equal(rows, np.concatenate(want) if want else np.zeros((0, cols)), equal_nan=True), (case.name, reg)
            if front is not None:
                assert np.array_equal(front, np.broadcast_to(node.respond(L.front_position, 1, cols, L.rate), (1, cols)), equal_nan=True)
        compared += 1
    assert compared or case.group == 'rows', case.name


def test_most_cases_have_a_graph():
    whole = [c for c in K.CASES if all(graph_of(c, reg) is not None for reg, _, _ in c.outs)]
    assert len(whole) >= len(K.CASES) - 8, len(whole)


# --------------------------------------------------------------------------------------------------------------- struct layout
def header_fields(name: str) -> list:
    """(type, field) of a typedef struct of include/signals_amd.h, comments stripped"""
    text = re.sub(r'/\*.*?\*/', '', HEADER.read_text(), flags=re.S)
    body = re.search(r'typedef struct \{([^}]*)\}\s*' + name + r'\s*;', text).group(1)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            ctype, names = decl.rsplit(' ', 1)[0], None
            m = re.match(r'((?:const\s+)?\w+\s*\**)\s*(.*)', decl)
            ctype, names = m.group(1).replace(' ', ''), m.group(2)
            fields += [(ctype, n.strip().lstrip('*')) for n in names.split(',')]
    return fields


def test_struct_layout_matches_the_header():
    from signals_amd import _native
    size = {'int32_t': 4, 'constdouble*': 8, 'double*': 8}
    for name, struct in (('sig_ctl_ins', _native.CtlIns), ('sig_ctl_out', _native.CtlOut)):
        fields = header_fields(name)
        assert [f for _, f in fields] == [f for f, _ in struct._fields_], name
        offset = 0
        for ctype, field in fields:
            offset = -(-offset // size[ctype]) * size[ctype]
            assert getattr(struct, field).offset == offset and getattr(struct, field).size == size[ctype], (name, field)
            offset += size[ctype]
        assert ctypes.sizeof(struct) == -(-offset // 8) * 8, name
    assert ctypes.sizeof(_native.CtlIns) == 48 and ctypes.sizeof(_native.CtlOut) == 24
    assert K.MAX_INS == _native.CTL_MAX_INS and dict(Row=K.ROW, Osc=K.OSC, Gain=K.GAIN, Mix=K.MIX, RingMod=K.RINGMOD, Amp=K.AMP,
                                                     Noise=K.NOISE, Filter=K.FILTER, AdsrArgs=K.ADSRARGS, Adsr=K.ADSR) == _native.CTL_OPS
    assert (K.SINE, K.SQUARE, K.SAWTOOTH, K.TRIANGLE) == tuple(_native.OSC_KINDS[n] for n in ('Sine', 'Square', 'Sawtooth', 'Triangle'))
    assert (K.LOWPASS, K.HIGHPASS) == (_native.FILT_TYPES['lp'], _native.FILT_TYPES['hp'])


@pytest.mark.parametrize('name', ['filter_257', 'adsr_2', 'rows_per_block_3', 'front_null'])
def test_to_ctl_on_the_cpu_reproduces_the_layout(name):
    from signals_amd import _native
    case = K.BY_NAME[name]
    up = K.to_ctl(case, 'cpu')
    L = case.launch
    assert up.program.dtype == torch.uint8 and up.program.numel() == 48 * len(case.ins) and up.outs.numel() == 24 * len(case.outs)
    words = np.frombuffer(up.program.numpy().tobytes(), dtype=np.int32).reshape(len(case.ins), 12)
    pointers = np.frombuffer(up.program.numpy().tobytes(), dtype=np.uint64).reshape(len(case.ins), 6)[:, 5]
    for k, i in enumerate(case.ins):
        assert words[k, :10].tolist() == [i.op, i.kind, i.a, i.b, i.c, i.dst, i.stride, i.rows, i.cols, i.reserved]
        if i.op == K.ROW:
            assert int(pointers[k]) == up.rows[k].data_ptr() and up.rows[k].shape == (i.rows, i.cols) and up.rows[k].is_contiguous()
            assert np.array_equal(up.rows[k].numpy(), i.data)
        elif i.op == K.FILTER:
            assert int(pointers[k]) == up.status[k].data_ptr() and int(up.status[k][0]) == 0
        elif i.op != K.NOISE:
            assert int(pointers[k]) == 0
    outs = np.frombuffer(up.outs.numpy().tobytes(), dtype=np.uint64).reshape(len(case.outs), 3)
    for k, (reg, cols, has_front) in enumerate(case.outs):
        assert int(outs[k, 0]) == reg | (cols << 32) and int(outs[k, 1]) == up.buffers[k].data_ptr()
        assert up.buffers[k].numel() == L.nblocks * cols + K.GUARD
        assert (up.buffers[k].view(torch.int64) == K.guard_bits()).all()
        assert int(outs[k, 2]) == (up.fronts[k].data_ptr() if has_front else 0)
        assert up.fronts[k] is None or up.fronts[k].numel() == cols + K.GUARD
    assert _native.control_program_description(up.ins_list, up.outs_list)[:2] == [len(case.ins), len(case.outs)]
    assert np.isnan(K.GUARD_VALUE)
