"""Interaction metrics of the closed-loop evaluation on the GPU: the mpc_interaction_metrics kernel against its host build on
the streams of tests/interaction_host.py (state and records: integers equal, f64 to atol 1e-8, the traffic tests'
device-to-host bound - the two call different cos and sin), the stated scenarios of tests/test_interaction_cpu.py through the
kernel, the captured evaluation step against the eager one, and the entry point's argument checks.

The streams use seed 100 B + K.  For them no compared quantity of the host build lies within 1e-9 of its threshold (asserted
per case), so a difference between kernel and host build can only be one of arithmetic."""
import ctypes
import functools
import math

import numpy as np
import pytest

import interaction_host as ih
from test_evaluate_cpu import CFG, Env
from test_interaction_cpu import SHIPPED, forced_braking_states, pet_states

pytestmark = pytest.mark.gpu
ATOL, MARGIN, STEPS = 1e-8, 1e-9, 40


def _dev():
    import torch
    return torch.device("cuda", 0)


class SlotEnv:
    """What InteractionMetrics.update reads of an environment: the slots as device tensors."""
    traffic = "idm"

    def __init__(self, s, dev):
        import torch
        for k, v in ih.state_of(s).items():
            setattr(self, k, torch.from_numpy(v.astype(bool) if k == "oactive" else v).to(dev))


def run_kernel(states, B, Q, K, ref_xy):
    import torch
    from mpc_rl_for_avs_amd import evaluate
    dev = _dev()
    m = evaluate.InteractionMetrics(B, Q, dev, "hip", ref_xy, ih.DT, K)
    for s in states:
        done = torch.from_numpy(np.ascontiguousarray(s["done"], np.uint8)).to(dev)
        m.update(SlotEnv(s, dev), done, reset=bool(s.get("reset")))
    torch.cuda.synchronize(dev)
    return m


@functools.lru_cache(maxsize=None)
def _stream(B, K, M):
    """40 steps with done forced on chosen steps: on the first, on two in a row, past the quota, and a reset in mid-episode"""
    ref = ih.STRAIGHT_REF if M == 2 else SHIPPED
    return ref, ih.random_stream(100 * B + K, B, K, STEPS, ref, done_at=(1, 12, 13, 25, 33), reset_at=(20,))


@pytest.mark.parametrize("Q,M", [(1, 2), (2, 85), (1, 85), (2, 2)])
@pytest.mark.parametrize("K", [1, 4, 9])
@pytest.mark.parametrize("B", [1, 5, 17])        # four environments share a wave: 5 crosses it, 17 leaves a partial group
def test_kernel_is_the_host_build(B, K, Q, M):
    from mpc_rl_for_avs_amd import evaluate
    ref, states = _stream(B, K, M)
    assert ref.shape[0] == M
    h = ih.run_host(states, B, Q, K, ref, evaluate.conflict_points(ref))
    assert h.margin[0] > MARGIN, h.margin[0]
    m = run_kernel(states, B, Q, K, ref)
    ih.assert_planes_close({n: getattr(m, n).cpu().numpy() for n in ih.PLANES}, h.planes(), "kernel vs host build", ATOL)


def _records(states):
    from mpc_rl_for_avs_amd import evaluate
    m = run_kernel(states, 1, 1, 1, ih.STRAIGHT_REF)
    h = ih.run_host(states, 1, 1, 1, ih.STRAIGHT_REF, evaluate.conflict_points(ih.STRAIGHT_REF))
    ih.assert_planes_close({n: getattr(m, n).cpu().numpy() for n in ih.PLANES}, h.planes(), "kernel vs host build", ATOL)
    return {k: v[0, 0] for k, v in m.records().items()}


def test_stated_scenarios_through_the_kernel():
    r = _records(forced_braking_states())
    assert (r["steps"], r["yield_steps"], r["forced_brake_steps"], r["forced_brake_events"]) == (1, 1, 1, 1)
    assert r["max_forced_decel"] == 6.0 and r["speed_deficit"] == 6.0 * ih.DT
    r = _records(forced_braking_states(copies=2))
    assert (r["steps"], r["yield_steps"], r["forced_brake_steps"], r["forced_brake_events"]) == (2, 2, 2, 1)
    for far in (forced_braking_states(prog=-10.5), forced_braking_states(ego=(4.5, 30.0, -math.pi / 2, 0.0))):
        r = _records(far)
        assert r["steps"] == 1 and not any(r[k] for k in ("yield_steps", "forced_brake_steps", "forced_brake_events"))
        assert r["max_forced_decel"] == 0.0 and r["speed_deficit"] == 0.0
    r = _records(pet_states(4, 6))
    assert (r["conflicts"], r["ego_first"], r["pet_critical"]) == (1, 1, 1) and r["min_pet"] == 2.0 * ih.DT
    r = _records(pet_states(6, 4))
    assert (r["conflicts"], r["ego_first"], r["pet_critical"]) == (1, 0, 1) and r["min_pet"] == 2.0 * ih.DT
    r = _records(pet_states(6, 4, replaced_at=5))
    assert (r["conflicts"], r["ego_first"], r["pet_critical"]) == (0, 0, 0) and r["min_pet"] == math.inf


def _eval(**kw):
    from mpc_rl_for_avs_amd import evaluate, rollout
    from mpc_rl_for_avs_amd.engine import MPCEngine
    from mpc_rl_for_avs_amd.pure_mpc import PureMPC_Agent
    agent = PureMPC_Agent(Env(), dict(CFG), engine=MPCEngine(horizon=20, device=0), collision_cost=False)
    env = rollout.SyntheticIntersectionEnv(16, device=_dev(), seed=7, traffic="idm")
    return evaluate.evaluate_agent(agent, env, episodes_per_env=1, seed=7, metrics=True, **kw)


def _assert_same(got, want):
    assert got.keys() == want.keys()
    for k in got:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8)), k


def test_graph_and_eager_evaluations_give_the_same_interaction_metrics():
    from mpc_rl_for_avs_amd import evaluate
    g = _eval(interaction=True, use_graph=True)
    e = _eval(interaction=True, use_graph=False)
    off = _eval(interaction=False, use_graph=True)
    assert set(g.interaction) == set(evaluate.INTERACT_I32 + evaluate.INTERACT_F64)
    _assert_same(g.interaction, e.interaction)
    assert np.array_equal(g.interaction["steps"], g.records["steps"]) and g.steps == e.steps
    assert off.interaction is None
    for a in (g, e):
        _assert_same(a.records, off.records)
        _assert_same(a.drive, off.drive)
    assert "yield_step_frac" in g.summary() and "yield_step_frac" not in off.summary()


def test_kernel_refuses_invalid_arguments():
    """host-side checks: nothing is launched with a bad pointer"""
    import torch
    from mpc_rl_for_avs_amd import engine
    lib = engine.load_library()
    dev = _dev()
    B, K, Q, M = 4, 3, 2, 5
    z = lambda *sh, dt=torch.float64: torch.zeros(sh, dtype=dt, device=dev)
    a = dict(ego=z(B, 4), opos=z(B, K, 2), ospeed=z(B, K), ohead=z(B, K), oactive=z(B, K, dt=torch.uint8),
             oroute=z(B, K, dt=torch.int32), oprog=z(B, K), otarget=torch.ones((B, K), dtype=torch.float64, device=dev),
             done=z(B, dt=torch.uint8), ref=z(M, 2), conflict=torch.full((12, 2), -1.0, dtype=torch.float64, device=dev),
             si=z(18, B, dt=torch.int32), sf=z(34, B), ri=z(7, B, Q, dt=torch.int32), rf=z(3, B, Q))
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(B=B, K=K, Q=Q, M=M, reset=0, dt=0.1, **null):
        assert set(null) <= set(a) and not any(v is not None for v in null.values())
        return lib.mpc_interaction_metrics(0, B, K, Q, M, reset, dt, *[p(None if n in null else a[n]) for n in a], stream)

    assert call(reset=1) == 0 and call() == 0
    assert call(reset=1, done=None) == 0                         # a reset launch needs no done
    assert call(B=0) == 0
    bad = [dict(B=-1), dict(Q=0), dict(K=0), dict(K=10), dict(M=0), dict(M=129), dict(dt=0.0), dict(dt=-0.1), dict(done=None)]
    bad += [{n: None} for n in a if n != "done"] + [dict(ego=None, reset=1), dict(conflict=None, reset=1)]
    for kw in bad:
        assert call(**kw) == -1, kw                              # MPC_ERR_INVALID_ARG
        assert b"mpc_interaction_metrics" in lib.mpc_last_error(), kw
    torch.cuda.synchronize(dev)
