"""The fused bus launch's kept state without a GPU: which C entries one render of the C2 voice graph SumBus(Gain(LowPass(Sine)))
calls, and which kept objects survive it, across the transitions the replay goes through -- the first render, the context length
changing, constants reused, a parameter array edited in place, another Fixed plugged in, the Sine closed form's range running out,
and the one-launch latency block with its bound call.  The library is a stub that records the name of every entry called (nothing
is rendered); the pipelined and the captured replay need real streams and stay with tests/test_gpu_engine.py."""
import math

import numpy as np
import pytest

from signals_amd import _native
from signals_amd.chain import ext, fixed, fx, osc

RATE = 48000
V, N, C = 64, 256, 2


# the two places where this test reads the engine's kept state
def steady(r):
    """(key, bound FusedVoiceBusCall | None) of the closed form's constants the renderer keeps"""
    held = r._steady_consts
    return held.key, held.call


def latency(r):
    """(live key, bound LatencyVoiceBusCall) of the one-launch block's replay, or None"""
    replay = r._replay[3]
    return None if replay.call is None else (replay.live, replay.call)


@pytest.fixture(autouse=True)
def _cpu_device():
    from signals_amd import runtime
    old = runtime._device
    runtime.set_device('cpu')
    yield
    runtime._device = old


@pytest.fixture
def stubbed(monkeypatch):
    """every entry point of the library answers 0 and is recorded as (name, arguments) when it is CALLED (a bound call keeps its
    entry from one render to the next); the bus plan answers one voice per lane, closed form"""
    calls = []

    class Lib:
        def __getattr__(self, name):
            def entry(*a):
                calls.append((name, a))
                if name == 'sig_fused_voice_bus_plan':
                    for ref, value in zip(a[-3:], (1, 8, 1)):
                        ref._obj.value = value
                return 0
            return entry
    stub = Lib()
    monkeypatch.setattr(_native, 'lib', lambda: stub)
    monkeypatch.setattr(_native, '_gpu', lambda *a: None)
    monkeypatch.setattr(_native, '_stream', lambda t: 0)
    return calls


def fix(v):
    f = fixed.Fixed()
    f.get_state().value = np.ascontiguousarray(np.array(v, ndmin=2, dtype=float))
    return f


def c2():
    rng = np.random.default_rng(5)
    sine = osc.Sine(); sine.hertz = fix(rng.uniform(55, 1760, (1, V))); sine.phase = fix(rng.uniform(0, 1, (1, V)))
    lp = fx.LowPass(); lp.input = sine; lp.cutoff = fix(rng.uniform(200, 8000, (1, V)))
    gain = fx.Gain(); gain.left = lp; gain.right = fix(rng.uniform(0, 1, (1, V)) / V)
    bus = ext.SumBus(); bus.input = gain
    th = rng.uniform(0, np.pi / 2, V)
    bus.get_state().gains = np.ascontiguousarray(np.stack([np.cos(th), np.sin(th)]))
    return bus, sine, lp, gain


def took(calls):
    """the entries called since the last look, in order"""
    names = [name for name, _ in calls]
    del calls[:]
    return names


# what one batch launch costs in entries: re-deriving the constants asks for their size and the launch plan, binding a call asks for
# the workspace and the constants' size once more (its argument checks), the launch itself is the bound entry
RENEW = ['sig_fused_voice_consts_size', 'sig_fused_voice_bus_plan']
BIND = ['sig_fused_voice_bus_workspace', 'sig_fused_voice_consts_size']
LAUNCH = ['sig_fused_voice_bus_bound']


def test_batch_launch_keeps_its_constants_and_its_bound_call(stubbed):
    """K = 8, the batch kernels (scan_max_chains = 0): the constants and the pre-bound call live as long as the context length and
    the parameter uploads do"""
    from signals_amd.engine import BatchRenderer
    K = 8
    bus, sine, lp, gain = c2()
    r = BatchRenderer(bus, C, RATE)
    r.scan_max_chains = 0
    bound_args = lambda: [a for name, a in stubbed if name == 'sig_fused_voice_bus_bound'][-1]

    # the first render plans the graph: the bus workspace, then constants, a bound call and its launch (nothing ready, no walk)
    out = r.render(0, N, K)
    assert tuple(out.shape) == (N * K, C)
    assert bound_args()[1:2] + bound_args()[3:5] == (0, 0, 0)
    assert took(stubbed) == ['sig_fused_voice_bus_workspace'] + RENEW + BIND + LAUNCH
    plan = r._replay[3]
    key0, call0 = steady(r)
    assert call0 is not None and key0[-1] == 0                                    # built inside the first context: min(100, 0)

    # the second render replays the plan; the context length is 100 now, so the constants are rebuilt and a new call is bound
    r.render(N * K, N, K)
    assert bound_args()[1:2] + bound_args()[3:5] == (N * K, 0, 0)
    assert took(stubbed) == RENEW + BIND + LAUNCH
    key1, call1 = steady(r)
    assert r._replay[3] is plan and key1 != key0 and key1[:-1] == key0[:-1] and key1[-1] == 100 and call1 is not call0

    # the third: the same constants (ready), the same call object, one entry
    r.render(2 * N * K, N, K)
    assert bound_args()[1:2] + bound_args()[3:5] == (2 * N * K, 1, 0)
    assert took(stubbed) == LAUNCH
    assert steady(r)[0] == key1 and steady(r)[1] is call1 and r._replay[3] is plan

    # an in-place edit of the cutoff array: another upload, another key, a new call; the plan stays
    lp.cutoff.sig.get_state().value[0, :] *= 0.5
    r.render(3 * N * K, N, K)
    assert bound_args()[3:5] == (0, 0)
    assert took(stubbed) == RENEW + BIND + LAUNCH
    key2, call2 = steady(r)
    assert key2 != key1 and call2 is not call1 and r._replay[3] is plan
    r.render(4 * N * K, N, K)
    assert took(stubbed) == LAUNCH and steady(r)[1] is call2

    # another Fixed plugged in: the graph's version moves on, the graph is planned again (the workspace is asked for again)
    from signals_amd.chain import graph_clock
    version = graph_clock.version
    sine.hertz = fix(sine.hertz.sig.get_state().value * 2.0)
    assert graph_clock.version != version
    r.render(5 * N * K, N, K)
    assert took(stubbed) == ['sig_fused_voice_bus_workspace'] + RENEW + BIND + LAUNCH
    assert r._replay[3] is not plan and r._replay[0] == graph_clock.version
    key3, call3 = steady(r)
    assert key3 != key2 and call3 is not call2

    # where the batch's last frame puts the fastest voice past the closed form's phase range, the span walker takes the launch
    per_frame = float(np.abs(sine.hertz.sig.get_state().value).max()) / RATE
    ph_max = float(np.abs(sine.phase.sig.get_state().value).max())
    edge = math.ceil((_native.SINE_FAST_MAX_CYCLES - ph_max) / per_frame) - N * K       # the first position that walks
    assert ph_max + (edge + N * K) * per_frame >= _native.SINE_FAST_MAX_CYCLES > ph_max + (edge - 1 + N * K) * per_frame
    r.render(edge - 1, N, K)
    assert bound_args()[1:2] + bound_args()[3:5] == (edge - 1, 1, 0)
    r.render(edge, N, K)
    assert bound_args()[1:2] + bound_args()[3:5] == (edge, 1, 1)
    assert took(stubbed) == LAUNCH + LAUNCH and steady(r) == (key3, call3)


def test_latency_block_reuses_its_bound_call_while_the_uploads_hold(stubbed):
    """K = 1, the defaults: one sig_latency_voice_bus launch per block; from the second replay on through one bound call, rebuilt
    after an edit"""
    from signals_amd.engine import BatchRenderer
    bus, sine, lp, gain = c2()
    r = BatchRenderer(bus, C, RATE)
    WS, ONE = 'sig_latency_voice_bus_workspace', 'sig_latency_voice_bus'

    # planning: the bus workspace, the latency kernel's zeroed scratch, one generic launch (it checks the scratch's size)
    r.render(0, N, 1)
    assert took(stubbed) == ['sig_fused_voice_bus_workspace', WS, WS, ONE]
    plan = r._replay[3]
    assert latency(r) is None and r._steady_consts is None

    # the first replay binds the call (one size check) and still launches through the generic entry (another)
    r.render(N, N, 1)
    assert took(stubbed) == [WS, WS, ONE]
    key, call = latency(r)
    assert isinstance(call, _native.LatencyVoiceBusCall) and call.shape == (N, C)
    assert len(key) == 5 and key[2] is lp.cutoff.sig.resident() and key[4] is bus.resident_gains()

    # from then on: the bound call alone, the same object
    for b in (2, 3):
        r.render(b * N, N, 1)
        assert [(name, a[2]) for name, a in stubbed] == [(ONE, b * N)]
        assert took(stubbed) == [ONE] and latency(r)[1] is call and r._replay[3] is plan

    # an in-place edit: the identities no longer hold, the call is bound again; then reused again
    gain.right.sig.get_state().value[0, :7] *= 0.5
    r.render(4 * N, N, 1)
    assert took(stubbed) == [WS, WS, ONE]
    key2, call2 = latency(r)
    assert call2 is not call and key2[3] is gain.right.sig.resident() and key2[3] is not key[3] and r._replay[3] is plan
    r.render(5 * N, N, 1)
    assert took(stubbed) == [ONE] and latency(r)[1] is call2
