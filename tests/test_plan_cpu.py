"""The plan metrics and the plan trace of the closed-loop evaluation on the CPU: the host build of csrc/mpc_plan.hpp, the
evaluator's numpy path and a plain-Python restatement (tests/plan_host.py) against one another, bit for bit, on streams with
the edge cases forced; lead error, clearance and replanning jump against answers that need no implementation to state; a
ring that does not leak across episodes; the plan trace against the trace recorder's host build; the argument checks and the
signature table; evaluate_agent with and without plan= on the torch environment; a sanitizer run of the host build in a
stand-alone program."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import conftest
import episode_trace_host as eth
import plan_host as ph
from mpc_rl_for_avs_amd import evaluate, rollout

INF = ph.INF
SIZES, HORIZONS, ROWS = [1, 5, 33], [1, 2, 20], [1, 2, 10, 17]
SPREAD = (1, 5, 10, 20)
SHAPES = [(B, N, R, (1,)) for B in SIZES for N in HORIZONS for R in ROWS] + [(B, 20, R, SPREAD) for B in SIZES for R in ROWS]
Q = 5                                                       # one turn through the ages; most environments end more episodes
RESET_AT = 6                                                # the launch before which the stream's second reset launch comes


def _ages(Lmax):
    return [a for a in (1, 2, Lmax - 1, Lmax, Lmax + 3) if a >= 1]


def _launches(Lmax):
    """a few short episodes, the reset launch, then one turn through the ages and five launches more"""
    return RESET_AT + sum(_ages(Lmax)) + 5


def _ends(Lmax):
    """environment b's episodes: until the reset launch one of 1 - 3 steps, from it on (the reset launch restarts every
    episode) the ages 1, 2, Lmax - 1, Lmax, Lmax + 3 in turn (those >= 1), starting with the b-th of them"""
    ages = _ages(Lmax)

    def ends(b):
        out = [t for t in range(RESET_AT) if (t + b) % 3 == 0]
        t, k = RESET_AT - 1, b
        while t < _launches(Lmax):
            t += ages[k % len(ages)]
            k += 1
            out.append(t)
        return out
    return ends


def _stream(B, N, R, leads):
    """30 launches and more: as many as every age up to max(leads) + 3 needs after the reset launch"""
    Lmax = max(leads)
    return ph.random_stream(B, N, R, seed=1000 * B + 10 * N + R + len(leads), launches=max(_launches(Lmax), 30), reset_at=RESET_AT,
                            ends=_ends(Lmax))


def ended_ages(steps, b):
    """the ages at which environment b's episodes end, the reset launches restarting the count"""
    ages, t = [], 0
    for s in steps:
        if s.get("reset"):
            t = 0
            continue
        t += 1
        if s["done"][b]:
            ages.append(t)
            t = 0
    return ages


def _run_host(steps, B, N, R, leads, **kw):
    h = ph.HostPlan(B, Q, N, R, leads, **kw)
    for s in steps:
        h.update(s)
    return h


def _run_numpy(steps, B, N, R, leads, **kw):
    m = evaluate.PlanMetrics(B, Q, "cpu", "torch", N=N, R=R, leads=leads, **kw)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    for s in steps:
        if s.get("reset"):
            m.update(None, None, None, None, None, None, reset=True)
        else:
            m.update(t(s["plan_X"]), t(s["plan_U"]), t(s["status"]), t(s["acted"]), t(s["terminal_obs"]), t(s["done"]))
    return {n: getattr(m, n).numpy() for n in ph.PLANES}


# ---- 1: three statements of one update ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,N,R,leads", SHAPES)
def test_host_build_numpy_path_and_plain_python_agree_bit_for_bit(B, N, R, leads):
    steps, Lmax = _stream(B, N, R, leads), max(leads)
    assert len(steps) >= 32 and sum(1 for s in steps if s.get("reset")) == 2 and steps[RESET_AT + 1].get("reset")
    assert any(s["status"][b] in ph.UNSOLVED for s in steps[1:] if not s.get("reset") for b in range(B))
    reached = set(ended_ages(steps[RESET_AT + 1:], 0))                             # after the reset launch in the middle
    assert {1, 2, Lmax, Lmax + 3} <= reached and (Lmax < 2 or Lmax - 1 in reached), reached
    host = _run_host(steps, B, N, R, leads).planes()
    ph.assert_planes_equal(_run_numpy(steps, B, N, R, leads), host, ("numpy", B, N, R, leads))
    ph.assert_planes_equal(ph.replay(steps, B, Q, N, R, leads), host, ("python", B, N, R, leads))
    assert host["rec_i32"][0].max() >= Lmax + 3 and (host["state_i32"][4] == Q).all()
    assert len(ended_ages(steps[RESET_AT + 1:], 0)) > Q                            # an environment past its quota
    used = [i for i, h in enumerate(ph.pad(leads)) if h]
    assert all(host["rec_i32"][4 + i].max() > 0 for i in used), host["rec_i32"][4:8].max(axis=(1, 2))   # every lead in a record


def test_an_invalid_plan_on_the_step_of_a_done_and_before_it_is_counted_and_skipped():
    B, N, R = 1, 2, 2
    X = np.zeros((B, N + 1, 4))
    acted = np.zeros((B, R, 8), np.float32)
    acted[:, 1, :3] = (1.0, 3.0, 4.0)                                              # clearance 5 at every stage
    term = np.zeros((B, R, 8), np.float32)
    step = lambda st, d: dict(plan_X=X, plan_U=np.ones((B, N, 2)), status=np.array([st], np.int32), acted=acted,
                              terminal_obs=term, done=np.array([d], np.uint8))
    h = _run_host([dict(reset=True), step(0, 0), step(3, 0), step(1, 1)], B, N, R, (1,))
    assert h.rec_i32[:4, 0, 0].tolist() == [3, 1, 0, 0] and h.rec_i32[4, 0, 0] == 1   # one valid plan, one lead error
    assert h.rec_f64[0, 0, 0] == 5.0 and h.rec_f64[5, 0, 0] == 0.0


# ---- 2: answers stated without an implementation -------------------------------------------------------------------------------

def _straight(T, N, B=1, R=1, offset=0.5, dones=()):
    """plans X_t[k] = (t + k, 0) against outcomes (t + 1 + offset, 0); t counts the launches"""
    steps = [dict(reset=True)]
    for t in range(T):
        X = np.zeros((B, N + 1, 4))
        X[:, :, 0] = t + np.arange(N + 1)
        term = np.zeros((B, R, 8), np.float32)
        term[:, 0, 1] = t + 1 + offset
        steps.append(dict(plan_X=X, plan_U=np.zeros((B, N, 2)), status=np.zeros(B, np.int32), acted=np.zeros((B, R, 8), np.float32),
                          terminal_obs=term, done=np.full(B, 1 if t in dones or t == T - 1 else 0, np.uint8)))
    return steps


@pytest.mark.parametrize("run", [_run_host, lambda *a, **k: type("P", (), _run_numpy(*a, **k))], ids=["host", "numpy"])
def test_every_lead_error_of_a_plan_that_is_late_by_one_half_is_one_half(run):
    T, N = 25, 20
    r = run(_straight(T, N), 1, N, 1, SPREAD)
    assert r.rec_i32[4:8, 0, 0].tolist() == [T - h + 1 for h in SPREAD]            # lead h is scored from age h on
    assert (r.rec_f64[5:9, 0, 0] == 0.5).all() and (r.rec_f64[9:13, 0, 0] == 0.5).all()   # an alignment off by one gives 1.5
    assert r.rec_f64[0, 0, 0] == INF and r.rec_i32[2, 0, 0] == 0                   # R = 1: nothing to clear


def test_clearance_is_three_four_five_at_a_known_stage():
    B, N, R, k = 1, 4, 3, 3
    X = np.zeros((B, N + 1, 4))
    X[0, :, 0] = 100.0 * np.arange(N + 1)                                          # far apart but at stage k
    acted = np.zeros((B, R, 8), np.float32)
    # row 2 is present: it moves with (10, 0) from (300 + 3 - 10 k dt, 4), so at stage k it is (303, 4)
    acted[0, 2] = (1.0, 300.0, 4.0, 10.0, 0.0, 0.0, 0.0, 1.0)
    acted[0, 1] = (0.0, 300.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)                       # absent, and on the path
    s = dict(plan_X=X, plan_U=np.zeros((B, N, 2)), status=np.zeros(B, np.int32), acted=acted,
             terminal_obs=np.zeros((B, R, 8), np.float32), done=np.ones(B, np.uint8))
    for dt in (1.0, 0.1):
        acted[0, 2, 1] = np.float32(303.0 - 10.0 * k * dt)
        for gap, conflicts in ((5.0, 0), (5.5, 1)):
            h = _run_host([dict(reset=True), s], B, N, R, (1,), dt=dt, gap=gap)
            assert h.rec_f64[0, 0, 0] == 5.0 and h.rec_i32[2, 0, 0] == conflicts, (dt, gap)


def test_replanning_jump_is_the_difference_to_the_previous_plans_second_control():
    B, N, R, T = 1, 3, 1, 4
    steps = _straight(T, N)
    for t, s in enumerate(steps[1:]):
        s["plan_U"] = np.zeros((B, N, 2))
        s["plan_U"][0, 0] = (2.0 * t, -0.25 * t)                                   # this plan's first control
        s["plan_U"][0, 1] = (2.0 * t + 0.5, 1.0)                                   # what it intends for the next step
    h = _run_host(steps, B, N, R, (1,))
    # U_t[0] - U_{t-1}[1] = (2 t - (2 (t - 1) + 0.5), -0.25 t - 1) = (1.5, -0.25 t - 1) for t = 1, 2, 3
    assert h.rec_i32[3, 0, 0] == 3 and h.rec_f64[1, 0, 0] == 1.5 and h.rec_f64[3, 0, 0] == 1.5
    assert h.rec_f64[2, 0, 0] == (1.25 + 1.5 + 1.75) / 3.0 and h.rec_f64[4, 0, 0] == 1.75
    one = _straight(T, 1)                                                          # N = 1: the previous plan's only control
    for t, s in enumerate(one[1:]):
        s["plan_U"] = np.full((B, 1, 2), 3.0 * t)
    assert _run_host(one, B, 1, R, (1,)).rec_f64[1:3, 0, 0].tolist() == [3.0, 3.0]


def test_the_ring_does_not_leak_across_a_done():
    """episode 1 has 12 steps, episode 2 has 7: no lead beyond an episode's age is ever scored, and lead 5 of episode 2 counts
    3 errors (ages 5, 6, 7), all exactly 0.5 although the ring still holds episode 1's pairs"""
    N, T = 20, 19
    steps = _straight(T, N, dones=(11,))
    for kind in (_run_host, lambda *a: type("P", (), _run_numpy(*a))):
        r = kind(steps, 1, N, 1, SPREAD)
        assert r.rec_i32[0, 0, :2].tolist() == [12, 7] and not r.rec_i32[0, 0, 2:].any()
        assert r.rec_i32[4:8, 0, 0].tolist() == [12, 8, 3, 0] and r.rec_i32[4:8, 0, 1].tolist() == [7, 3, 0, 0]
        scored = r.rec_i32[4:8, 0, :2] > 0
        assert (r.rec_f64[9:13, 0, :2][scored] == 0.5).all() and (r.rec_f64[9:13, 0, :2][~scored] == 0.0).all()


# ---- 3: the plan trace against the trace recorder's host build ------------------------------------------------------------------

@pytest.mark.parametrize("W", [1, 3, 8])
def test_plan_trace_keeps_the_plan_behind_every_action_frame(W):
    B, R, N, C, keep = 6, 2, 3, 2, eth.ALL
    steps = eth.random_stream(B, R, 3, W, C, keep, seed=40 + W)
    rng = np.random.default_rng(W)
    rec, planes = eth.HostTrace(B, R, 3, W, C, keep), ph.HostPlanTrace(B, N, 3, W, C)
    tr = evaluate.EpisodeTrace(B, 3, "cpu", "torch", R=R, keep="all", capacity=C, window=W, plan=True, horizon=N)
    t_ = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))
    slots = []
    for n, s in enumerate(steps):
        if not s.get("reset"):
            s["plan_X"], s["plan_U"] = rng.standard_normal((B, N + 1, 4)), rng.standard_normal((B, N, 2))
            s["plan_U"][:, 0] = s["action"]                                        # the first control IS the action
            s["plan_X"][:, 0, 0], s["plan_X"][:, 0, 1] = np.arange(B), n           # who planned it, and when
        rec.update(s)
        planes.update(s, rec.slot)
        slots.append(rec.slot.copy())
        tr.update(*[t_(s.get(k)) for k in eth.STEP_INPUTS], reset=bool(s.get("reset")), plan_X=t_(s.get("plan_X")),
                  plan_U=t_(s.get("plan_U")))
    assert rec.counts[0] >= 4 and rec.counts[1] == C and rec.counts[2] >= 2        # more selected than the store holds
    assert any((sl == -1).any() for sl in slots)
    for i in range(C):
        b, j, T, first = rec.index[i, :4]
        L = min(T, W)
        assert ph.same_bits(planes.kept_U[i, :L, 0], rec.kept_act[i, :L])          # frame i matches action frame i
        assert (planes.kept_X[i, :L, 0, 0] == b).all() and (np.diff(planes.kept_X[i, :L, 0, 1]) == 1).all()
        assert planes.kept_X[i, L - 1, 0, 1] == rec.index[i, 5]                    # the last plan is that of the launch it ended on
    got = {n: getattr(tr, {"state_i32": "plan_state_i32"}.get(n, n)).numpy() for n in ph.TRACE_PLANES}
    ph.assert_planes_equal(got, planes.planes(), ("numpy", W), ph.TRACE_PLANES)
    eth.assert_planes_equal({n: None if getattr(tr, n) is None else getattr(tr, n).numpy() for n in eth.PLANES}, rec.planes(), W)
    ep = tr.traces().episode(0)
    assert ph.same_bits(ep["plan_U"][:, 0], ep["action"]) and ep["plan_X"].shape == (min(int(rec.index[0, 2]), W), N + 1, 4)
    assert tr.nbytes == evaluate.EpisodeTrace.bytes_for(B, R, W, C, plan=True, horizon=N)


def test_traces_with_plans_survive_save_and_load(tmp_path):
    B, R, N, W, C = 6, 2, 2, 3, 4
    tr = evaluate.EpisodeTrace(B, 3, "cpu", "torch", R=R, keep="all", capacity=C, window=W, plan=True, horizon=N)
    t_ = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))
    for s in eth.random_stream(B, R, 3, W, C, eth.ALL, seed=3):
        X, U = (None, None) if s.get("reset") else (torch.randn(B, N + 1, 4).double(), torch.randn(B, N, 2).double())
        tr.update(*[t_(s.get(k)) for k in eth.STEP_INPUTS], reset=bool(s.get("reset")), plan_X=X, plan_U=U)
    a = tr.traces()
    a.save(tmp_path / "t.npz")
    b = evaluate.EpisodeTraces.load(tmp_path / "t.npz")
    assert len(a) == C and ph.same_bits(a.plan_X, b.plan_X) and ph.same_bits(a.plan_U, b.plan_U)
    assert ph.same_bits(a.episode(1)["plan_X"], b.episode(1)["plan_X"])
    plain = evaluate.EpisodeTrace(B, 3, "cpu", "torch", R=R)
    assert plain.config.keys() == {"R", "keep", "capacity", "window", "seen", "env_offset"} and plain.traces().plan_X is None
    assert evaluate.EpisodeTrace(B, 3, "cpu", "torch", **tr.config).N == N
    with pytest.raises(ValueError, match="horizon"):
        evaluate.EpisodeTrace(B, 3, "cpu", "torch", plan=True)
    with pytest.raises(ValueError, match="plan_X"):
        s = eth.random_stream(B, R, 3, W, C, eth.ALL, seed=3)[1]
        tr.update(*[t_(s.get(k)) for k in eth.STEP_INPUTS])


# ---- 4: argument checks, one per rule --------------------------------------------------------------------------------------------

def test_host_build_refuses_invalid_arguments_by_rule():
    B, N, R = 2, 4, 3
    s = ph.random_stream(B, N, R, seed=1, launches=1)[1]
    nan = float("nan")
    rules = [(dict(B=-1), "B >= 0"), (dict(N=0), "MPC_MAX_HORIZON"), (dict(N=65), "MPC_MAX_HORIZON"), (dict(R=0), "MPC_MAX_OTHERS"),
             (dict(R=18), "MPC_MAX_OTHERS"), (dict(Q=0), "Q >= 1"), (dict(dt=0.0), "dt > 0"), (dict(dt=nan), "dt > 0"),
             (dict(gap=-0.5), "gap >= 0"), (dict(gap=nan), "gap >= 0"), (dict(leads=(1, 5, 0, 0)), "lead in 0 .. N"),
             (dict(leads=(-1, 1, 0, 0)), "lead in 0 .. N"), (dict(leads=(0, 0, 0, 0)), "one lead used"),
             (dict(order=2), "order"), (dict(order=-1), "order")]
    for sizes, text in rules:
        h = ph.HostPlan(B, Q, N, R, (1, 4))
        assert h.call(s, sizes=sizes) == -1 and text in h.why, (sizes, h.why)
        assert h.call({}, reset=True, sizes=sizes) == -1 and not h.state_i32.any()
    h = ph.HostPlan(B, Q, N, R, (1, 4))
    for name in ph.PLANES:
        assert h.call(s, null=(name,)) == -1 and h.call({}, reset=True, null=(name,)) == -1, name
    for name in ph.STEP_INPUTS:
        assert h.call({k: v for k, v in s.items() if k != name}) == -1, name
    assert h.call({}, reset=True) == 0 and h.call(s) == 0 and h.call(s, sizes=dict(gap=0.0, order=1, leads=(4, 0, 0, 0))) == 0
    assert ph.HostPlan(0, Q, N, R, (1,)).call({k: v[:0] for k, v in s.items()}) == 0
    t = ph.HostPlanTrace(B, N, Q, 3, 2)
    slot = np.full(B, -1, np.int32)
    for sizes in (dict(B=-1), dict(N=0), dict(N=65), dict(Q=0), dict(W=0), dict(W=4097), dict(C=0)):
        assert t.call(s, slot, sizes=sizes) == -1, sizes
    for name in ph.TRACE_PLANES:
        assert t.call(s, slot, null=(name,)) == -1, name
    assert t.call(s, None) == -1 and t.call({}, None, reset=True) == 0 and t.call(s, slot) == 0


def test_plan_metrics_refuses_invalid_arguments():
    for kw in (dict(N=0), dict(N=65), dict(R=0), dict(R=18), dict(dt=0.0), dict(gap=-1.0), dict(gap=float("nan")),
               dict(leads=()), dict(leads=(0, 0)), dict(leads=(1, 2, 3, 4, 5)), dict(leads=(-1,)), dict(leads=(1, 21))):
        with pytest.raises(ValueError):
            evaluate.PlanMetrics(2, 1, "cpu", "torch", **{**dict(N=20), **kw})
    with pytest.raises(ValueError, match="beyond the horizon"):
        evaluate.PlanMetrics(2, 1, "cpu", "torch", N=8, leads=(1, 9))
    assert evaluate.default_leads(20) == (1, 5, 10, 20) and evaluate.default_leads(1) == (1,)
    assert evaluate.default_leads(2) == (1, 2) and evaluate.default_leads(5) == (1, 2, 5)
    m = evaluate.PlanMetrics(2, 1, "cpu", "torch", N=4, R=3, leads=(1, 4))
    assert m.leads == (1, 4, 0, 0) and m.Lmax == 4 and evaluate.PlanMetrics(2, 1, "cpu", "torch", **m.config).config == m.config
    s = {k: torch.from_numpy(v) for k, v in ph.random_stream(2, 4, 3, seed=1, launches=1)[1].items()}
    good = [s[k] for k in ph.STEP_INPUTS]
    for i, bad in enumerate((s["plan_X"].float(), s["plan_U"][:, :3], s["status"].long(), s["acted"].double(),
                             s["terminal_obs"][:1], s["done"].int())):
        with pytest.raises(ValueError):
            m.update(*(good[:i] + [bad] + good[i + 1:]))
    with pytest.raises(ValueError, match="order"):
        m.update(*good, order=2)
    assert not m.state_i32.any()


# ---- 5: the binding --------------------------------------------------------------------------------------------------------------

def _prototype(name):
    from test_abi import _header_text
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", _header_text())
    assert m, f"{name}: no prototype in include/mpc_mi355x.h"
    out = []
    for decl in m.group(1).split(","):
        ctype, pname = re.fullmatch(r"\s*(.*?)(\w+)\s*", decl, flags=re.S).groups()
        ctype = " ".join(ctype.replace("*", " * ").split())
        out.append((pname, "ptr" if ctype.endswith("*") else {"int32_t": "i32", "uint32_t": "u32", "double": "f64"}[ctype]))
    return out


def test_plan_signature_table_and_exports_are_the_header():
    from mpc_rl_for_avs_amd import engine
    from test_abi import _declared_symbols
    assert sorted(engine.PLAN_SIGNATURES) == ["mpc_plan_metrics", "mpc_plan_trace"]
    assert engine._TABLES.index(engine.PLAN_SIGNATURES) == len(engine._TABLES) - 2 and len(engine._TABLES) == 5
    others = [t for t in engine._TABLES if t is not engine.PLAN_SIGNATURES]
    assert not set(engine.PLAN_SIGNATURES) & set().union(*others)
    lib = engine.load_library()
    kinds = dict(i32=ctypes.c_int32, f64=ctypes.c_double, ptr=ctypes.c_void_p)
    for name, sig in engine.PLAN_SIGNATURES.items():
        assert list(sig) == _prototype(name) and len({n for n, _ in sig}) == len(sig), name
        assert list(getattr(lib, name).argtypes) == [kinds[k] for _, k in sig] and getattr(lib, name).restype is ctypes.c_int
        assert callable(engine.caller(name))
        with pytest.raises(TypeError, match=name):
            engine.call(name, device=0)
    new = {"mpc_predict_batch_plan", "mpc_ltv_predict_batch_plan", "mpc_plan_metrics", "mpc_plan_trace"}
    assert new <= set(engine._EXPORTS) and sorted(engine._EXPORTS) == _declared_symbols() and engine.ABI_VERSION == 8
    i, u, vp = ctypes.c_int32, ctypes.c_uint32, ctypes.c_void_p
    old, new_ = _prototype("mpc_predict_batch"), _prototype("mpc_predict_batch_plan")
    assert [n for n, _ in new_] == [n for n, _ in old[:8]] + ["U", "X"] + [n for n, _ in old[8:]]
    assert list(lib.mpc_predict_batch_plan.argtypes) == [vp, i, vp, i, vp, vp, u] + [vp] * 6
    old, new_ = _prototype("mpc_ltv_predict_batch"), _prototype("mpc_ltv_predict_batch_plan")
    assert [n for n, _ in new_] == [n for n, _ in old[:6]] + ["U", "X"] + [n for n, _ in old[6:]]
    assert list(lib.mpc_ltv_predict_batch_plan.argtypes) == [vp, i, vp, i, u] + [vp] * 6
    assert evaluate.PLAN_STATE_I32 == 10 and evaluate.PLAN_STATE_F64 == 15 and len(evaluate.PLAN_I32) == 8 and \
        len(evaluate.PLAN_F64) == 13


# ---- 6: the evaluator --------------------------------------------------------------------------------------------------------------

class _Horizon:
    horizon = 6


class ConstantVelocityPlanner:
    """An agent with a plan and no solver: it coasts (act = 0) and plans that the ego keeps its velocity; every fifth solve
    of environment 1 is reported unsolved."""
    engine = _Horizon()

    def __init__(self, dt):
        self.dt, self.calls = dt, 0

    def act_batch_torch(self, obs, deterministic=False, seed=0, env_offset=0, plan=False):
        B, N = obs.shape[0], self.engine.horizon
        out = dict(act=torch.zeros(B, 2, dtype=torch.float64), status=torch.zeros(B, dtype=torch.int32),
                   iters=torch.ones(B, dtype=torch.int32))
        if self.calls % 5 == 4 and B > 1:
            out["status"][1] = 1
        self.calls += 1
        if plan:
            ego = obs[:, 0].double()
            k = torch.arange(N + 1, dtype=torch.float64)[None, :] * self.dt
            X = torch.zeros(B, N + 1, 4, dtype=torch.float64)
            X[:, :, 0], X[:, :, 1] = ego[:, 1:2] + k * ego[:, 3:4], ego[:, 2:3] + k * ego[:, 4:5]
            out.update(plan_X=X, plan_U=torch.zeros(B, N, 2, dtype=torch.float64), plan_order=0)
        return out


def _evaluate(agent=None, B=8, on_step=None, **kw):
    import policy_ref as pr
    env = rollout.SyntheticIntersectionEnv(B, device="cpu", seed=21, n_others=4, backend="torch", traffic="idm")
    agent = rollout.PPOAgent(pr.make_policy(64, 2, -0.5, use_sde=False, seed=8)) if agent is None else agent(float(env.dt))
    kw.setdefault("trace", dict(keep="all", capacity=B, window=50))
    return evaluate.evaluate_agent(agent, env, episodes_per_env=1, use_graph=False, poll_every=5, seed=1, metrics=True,
                                   on_step=on_step, **kw)


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), k


def _same_results(a, b):
    _same(a.records, b.records)
    _same(a.drive, b.drive)
    assert a.steps == b.steps and a.traces.counts == b.traces.counts
    _same(a.traces.index, b.traces.index)
    for n in ("scene", "action", "reward", "frame_i32"):
        assert getattr(a.traces, n).tobytes() == getattr(b.traces, n).tobytes(), n


def test_evaluate_agent_with_plan_none_is_evaluate_agent_without():
    keys0, keys1 = [], []
    base = _evaluate(on_step=lambda d: keys0.append(tuple(d)))
    none = _evaluate(plan=None, on_step=lambda d: keys1.append(tuple(d)))
    _same_results(base, none)
    assert keys0 == keys1 and "plan_X" not in keys0[1] and base.plan is None and none.plan is None
    strip = lambda d: {k: v for k, v in d.items() if k not in ("seconds", "env_steps_per_s")}
    assert strip(base.summary()) == strip(none.summary()) and not any("plan" in k or "pred_err" in k for k in none.summary())
    assert none.traces.plan_X is None and "plan_X" not in none.traces.episode(0)
    # the same holds for an agent that has a plan and is not asked for it
    _same_results(_evaluate(ConstantVelocityPlanner), _evaluate(ConstantVelocityPlanner, plan=None))


def test_evaluate_agent_with_a_plan_scores_it_and_changes_nothing_else():
    frames = []
    keep = lambda d: frames.append({k: v.clone() if torch.is_tensor(v) else v for k, v in d.items()})
    base = _evaluate(ConstantVelocityPlanner)
    res = _evaluate(ConstantVelocityPlanner, plan=dict(leads=(1, 3, 6), gap=6.0), on_step=keep,
                    trace=dict(keep="all", capacity=8, window=50, plan=True))
    _same_results(base, res)
    B, N, dt = 8, 6, res.dt
    assert res.plan["leads"] == (1, 3, 6, 0) and set(res.plan) == set(evaluate.PLAN_I32 + evaluate.PLAN_F64) | {"leads"}
    assert (res.plan["steps"] == res.records["steps"]).all() and res.plan["plans_valid"].sum() < res.plan["steps"].sum()
    assert {"plan_X", "plan_U", "plan_order"} <= set(frames[1]) and "plan_X" not in frames[0]
    # the records again, from what on_step saw, by the host build
    h = ph.HostPlan(B, 1, N, 10, (1, 3, 6), dt=dt, gap=6.0)
    h.update(dict(reset=True))
    for before, f in zip(frames, frames[1:]):                                      # acted: what the step before left in obs
        h.update({k: (before["obs"] if k == "acted" else f[k]).numpy() for k in ph.STEP_INPUTS})
    assert ph.same_bits(h.rec_i32[:, :, 0], np.stack([res.plan[k][:, 0] for k in evaluate.PLAN_I32]).astype(np.int32))
    assert ph.same_bits(h.rec_f64[:, :, 0], np.stack([res.plan[k][:, 0] for k in evaluate.PLAN_F64]))
    # a coasting ego does what a constant-velocity plan says: the lead-1 error is the f32 rounding of the observation
    s = res.summary()
    assert 0.0 <= s["pred_err_lead1_mean"] < 1e-4 and set(s) >= {"plan_conflict_frac", "min_plan_gap", "pred_err_lead3_mean",
                                                                 "pred_err_lead6_mean", "replan_accel_mean", "replan_steer_mean",
                                                                 "plans_valid_frac"}
    assert s["replan_accel_mean"] == 0.0 and 0.0 < s["plans_valid_frac"] < 1.0 and "pred_err_lead0_mean" not in s
    # the trace: the plan behind every action frame, the one on_step saw on that step of that environment
    ep = res.traces.episode(0)
    b, T = ep["env"], ep["steps"]
    assert ep["plan_X"].shape == (T, N + 1, 4) and ep["plan_U"].shape == (T, N, 2)
    mine = [f for f in frames[1:]][:T]                                             # episode 0 of environment b: its first T steps
    assert ph.same_bits(ep["plan_X"], np.stack([f["plan_X"][b].numpy() for f in mine]))


def test_plan_needs_an_agent_with_a_plan_and_leads_within_the_horizon():
    with pytest.raises(ValueError, match="has no plan"):
        _evaluate(plan=True)
    with pytest.raises(ValueError, match="has no plan"):
        _evaluate(trace=dict(keep="all", plan=True))
    with pytest.raises(ValueError, match="beyond the horizon"):
        _evaluate(ConstantVelocityPlanner, plan=dict(leads=(1, 7)))
    with pytest.raises(ValueError, match="plan must be built"):
        _evaluate(ConstantVelocityPlanner, plan=evaluate.PlanMetrics(8, 1, "cpu", "torch", N=5))
    import policy_ref as pr
    agent = rollout.PPOAgent(pr.make_policy(64, 2, -0.5, use_sde=False, seed=8))
    with pytest.raises(ValueError, match="has no plan"):
        agent.act_batch_torch(torch.zeros(2, 10, 8), plan=True)
    res = _evaluate(ConstantVelocityPlanner, plan=True, trace=None)
    assert res.plan["leads"] == (1, 3, 6, 0)                                       # (1, N // 4, N // 2, N) at N = 6


# ---- 7: sanitizers: a stand-alone program, nothing loaded into Python -----------------------------------------------------------

def test_host_build_runs_clean_under_address_and_undefined_behaviour_sanitizers():
    out = os.path.join(conftest.ROOT, "tests", "_build", "plan_san_main")
    src = os.path.join(conftest.ROOT, "tests", "plan_san_main.cpp")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in [src] + ph.DEPS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                        "-static-libubsan", "-std=c++17", "-Wno-unknown-pragmas", "-ffp-contract=off", "-o", out, src],
                       check=True)
    res = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip().endswith("plan_san_main: ok"), res.stdout + res.stderr
