"""The MPC's plan on the GPU: mpc_predict_batch_plan / mpc_ltv_predict_batch_plan against the entries they replace (the same
bits with and without U / X, cold and warm-started, on device and host pointers) and the plan itself against the problem data,
the model's dynamics and the solve entries; the mpc_plan_metrics and mpc_plan_trace kernels against their host build on the
streams of tests/test_plan_cpu.py, bit for bit; the library's refusals; the captured evaluation step against the eager one,
with and without plan=, and the recorded lead errors recomputed from what on_step saw."""
import ctypes

import numpy as np
import pytest

import episode_trace_host as eth
import plan_host as ph
from conftest import ltv_states
from test_evaluate_cpu import CFG, Env
from test_plan_cpu import Q, SHAPES, _run_host, _stream

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda", 0)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ---- 1: the plan out of the observation-level entries ----------------------------------------------------------------------------

def _flags(cc, warm):
    from mpc_rl_for_avs_amd import engine
    return engine.FLAG_DEVICE_PTRS | (engine.FLAG_COLLISION_COST if cc else 0) | (engine.FLAG_WARM_START if warm else 0)


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("cc", [False, True], ids=["plain", "collision_cost"])
@pytest.mark.parametrize("B", [1, 64, 257])
def test_predict_batch_plan_is_predict_batch_and_the_plan_is_the_solves(B, cc, warm):
    import torch
    from mpc_rl_for_avs_amd import engine, synth
    dev, N, V = _dev(), 20, 5
    old, null, full, host = (engine.MPCEngine(horizon=N, device=0) for _ in range(4))
    w = torch.ones((B, 3), dtype=torch.float64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=dev)
    solved = 0
    for step in range(5):                                                          # the detector memory and the warm start carry on
        obs_h = synth.make_obs_batch(B, V, seed=900 + 10 * step + B)
        obs, rows = torch.from_numpy(obs_h).to(dev), obs_h.shape[1]               # ten rows, V of the others present
        a = old.predict_batch_torch(obs, w, collision_cost=cc, warm_start=warm, sync=True)
        act, st, it = z(B, 2), z(B, dt=torch.int32), z(B, dt=torch.int32)
        rc = null._lib.mpc_predict_batch_plan(null._h, B, _p(obs), rows, _p(w), None, _flags(cc, warm), _p(act), None, None, _p(st),
                                              _p(it), stream)
        assert rc == 0
        c = full.predict_batch_torch(obs, w, collision_cost=cc, warm_start=warm, sync=True, plan=True)
        torch.cuda.synchronize(dev)
        for got in (dict(act=act, status=st, iters=it), c):
            for k in ("act", "status", "iters"):
                assert a[k].cpu().numpy().tobytes() == got[k].cpu().numpy().tobytes(), (step, k)
        U, X = c["plan_U"].cpu().numpy(), c["plan_X"].cpu().numpy()
        assert c["plan_order"] == 0 and np.array_equal(U[:, 0], c["act"].cpu().numpy())
        inp = full.last_inputs(B, rows)
        assert np.array_equal(X[:, 0], inp["state"])
        _, x_next = full.eval_nlp(inp["ego_index"], np.ones((B, 3)), inp["is_collide"], X, U, vref=inp["vref"])
        defect = np.abs(X[:, 1:] - x_next).max()
        print(f"B={B} cc={cc} warm={warm} step={step}: dynamics defect {defect:.3e}")
        assert defect <= 1e-9                        # 1.4e-14 measured on coordinates of order 100 m (README)
        h = host.predict_batch(obs_h, np.ones((B, 3)), collision_cost=cc, warm_start=warm, plan=True)
        assert h["plan_order"] == 0
        for k, want in (("act", c["act"]), ("status", c["status"]), ("iters", c["iters"]), ("plan_U", c["plan_U"]),
                        ("plan_X", c["plan_X"])):
            assert h[k].tobytes() == want.cpu().numpy().tobytes(), (step, k, "host pointers")
        solved += int(((a["status"] == 0) | ((a["status"] >= 5) & (a["status"] <= 7))).sum())
    assert solved > 0.5 * 5 * B
    for e in (old, null, full, host):
        e.close()


def test_detect_only_writes_no_plan():
    import torch
    from mpc_rl_for_avs_amd import engine, synth
    dev, B, N, V = _dev(), 8, 20, 5
    e = engine.MPCEngine(horizon=N, device=0)
    obs = torch.from_numpy(synth.make_obs_batch(B, V, seed=5)).to(dev)
    rows = int(obs.shape[1])
    U, X = torch.full((B, N, 2), 7.0, dtype=torch.float64, device=dev), torch.full((B, N + 1, 4), 7.0, dtype=torch.float64, device=dev)
    rc = e._lib.mpc_predict_batch_plan(e._h, B, _p(obs), rows, None, None, engine.FLAG_DEVICE_PTRS | engine.FLAG_DETECT_ONLY, None,
                                       _p(U), _p(X), None, None, None)
    torch.cuda.synchronize(dev)
    assert rc == 0 and (U == 7.0).all() and (X == 7.0).all()
    e.close()


def test_ltv_predict_batch_plan_is_ltv_predict_batch_and_the_plan_is_ltv_solve_batchs():
    import torch
    from mpc_rl_for_avs_amd import engine
    from test_ltv_gpu import _obs_from_state
    dev, B, N = _dev(), 12, 20
    old, full, host, solve = (engine.MPCEngine(horizon=N, device=0) for _ in range(4))
    profile = np.zeros((B, N, 2))                                                  # what every environment has stored
    X = c = None
    for step in range(3):
        st = ltv_states(B, seed=40 + step)
        st[:, 2] = np.minimum(st[:, 2], 10.5)
        if step == 1:
            st[1, 2] = 11.5                                                        # above MAX_SPEED: no feasible point
        obs_h = _obs_from_state(st)
        obs = torch.from_numpy(obs_h).to(dev)
        a = old.ltv_predict_batch_torch(obs, sync=True)
        c = full.ltv_predict_batch_torch(obs, out=c, sync=True, plan=True)        # the same tensors every call
        before = None if X is None else X.copy()
        for k in ("act", "status", "iters"):
            assert a[k].cpu().numpy().tobytes() == c[k].cpu().numpy().tobytes(), (step, k)
        act, status = c["act"].cpu().numpy(), c["status"].cpu().numpy()
        U, X = c["plan_U"].cpu().numpy(), c["plan_X"].cpu().numpy()
        ok = status == 0
        assert c["plan_order"] == 1 and ok.sum() >= B - 1 and np.array_equal(U[ok, 0], act[ok])
        # the state the kernel parses: float32 arithmetic on the observation's ego row
        ego = obs_h[:, 0]
        parsed = np.stack([ego[:, 1], ego[:, 2], np.sqrt(ego[:, 3] * ego[:, 3] + ego[:, 4] * ego[:, 4]), ego[:, 5]], axis=1)
        want = solve.ltv_solve_batch(parsed.astype(np.float64), profile, want_traj=True)
        assert np.array_equal(want["status"], status) and np.array_equal(want["U"], U)
        written = status != 3                                                      # MPC_STATUS_INFEASIBLE_START: no X
        assert np.array_equal(want["X"][written], X[written]) and written.sum() >= B - 1
        if step == 1:
            assert status[1] == 3 and np.array_equal(X[1], before[1]) and np.array_equal(U[1], profile[1])   # left as they were
        h = host.ltv_predict_batch(obs_h, plan=True)
        assert h["plan_U"].tobytes() == U.tobytes() and h["act"].tobytes() == act.tobytes()
        assert np.array_equal(h["plan_X"][written], X[written]) and not h["plan_X"][~written].any()
        profile = U
    for e in (old, full, host, solve):
        e.close()


# ---- 2: the kernels against the host build ---------------------------------------------------------------------------------------

# the CPU test's N x R product with both sets of leads - 0, 1, 2, 9, 16, 18, 20, 32, 180 and 320 (stage, row) pairs for the sixteen
# lanes of a group - and B = 3, 4, 5 beside its sizes: four environments per wave, so 1, 3, 5 and 33 leave a partial wave
KERNEL_SHAPES = sorted({(N, R, leads) for _, N, R, leads in SHAPES})


@pytest.mark.parametrize("N,R,leads", KERNEL_SHAPES)
@pytest.mark.parametrize("B", [1, 3, 4, 5, 33])
def test_metrics_kernel_is_the_host_build_bit_for_bit(B, N, R, leads):
    import torch
    from mpc_rl_for_avs_amd import evaluate
    dev = _dev()
    steps = _stream(B, N, R, leads)
    m = evaluate.PlanMetrics(B, Q, dev, "hip", N=N, R=R, leads=leads)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for i, s in enumerate(steps):
        if s.get("reset"):
            m.update(None, None, None, None, None, None, reset=True)
        else:
            m.update(t(s["plan_X"]), t(s["plan_U"]), t(s["status"]), t(s["acted"]), t(s["terminal_obs"]), t(s["done"]), order=i % 2)
    torch.cuda.synchronize(dev)
    ph.assert_planes_equal({n: getattr(m, n).cpu().numpy() for n in ph.PLANES}, _run_host(steps, B, N, R, leads).planes(),
                           ("kernel", B, N, R, leads))


@pytest.mark.parametrize("W", [1, 3, 8])
def test_trace_kernel_is_the_host_build_bit_for_bit(W):
    import torch
    from mpc_rl_for_avs_amd import evaluate
    dev, B, R, N, C = _dev(), 6, 2, 20, 2
    steps = eth.random_stream(B, R, 3, W, C, eth.ALL, seed=40 + W)
    rng = np.random.default_rng(W)
    rec, planes = eth.HostTrace(B, R, 3, W, C, eth.ALL), ph.HostPlanTrace(B, N, 3, W, C)
    tr = evaluate.EpisodeTrace(B, 3, dev, "hip", R=R, keep="all", capacity=C, window=W, plan=True, horizon=N)
    t_ = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for s in steps:
        if not s.get("reset"):
            s["plan_X"], s["plan_U"] = rng.standard_normal((B, N + 1, 4)), rng.standard_normal((B, N, 2))
            s["plan_U"][:, 0] = s["action"]
        rec.update(s)
        planes.update(s, rec.slot)
        tr.update(*[t_(s.get(k)) for k in eth.STEP_INPUTS], reset=bool(s.get("reset")), plan_X=t_(s.get("plan_X")),
                  plan_U=t_(s.get("plan_U")))
    torch.cuda.synchronize(dev)
    got = {n: getattr(tr, {"state_i32": "plan_state_i32"}.get(n, n)).cpu().numpy() for n in ph.TRACE_PLANES}
    ph.assert_planes_equal(got, planes.planes(), ("kernel", W), ph.TRACE_PLANES)
    eth.assert_planes_equal({n: None if getattr(tr, n) is None else getattr(tr, n).cpu().numpy() for n in eth.PLANES},
                            rec.planes(), W)
    for i in range(C):
        L = min(int(rec.index[i, 2]), W)
        assert ph.same_bits(got["kept_U"][i, :L, 0], rec.kept_act[i, :L])


def test_kernels_refuse_invalid_arguments_by_name():
    import torch
    from mpc_rl_for_avs_amd import engine
    dev, B, N, R, W, C = _dev(), 4, 4, 3, 3, 2
    z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=dev)
    i32, u8, f32 = torch.int32, torch.uint8, torch.float32
    good = dict(device=0, B=B, N=N, R=R, Q=Q, reset=0, order=0, dt=0.1, gap=2.5, lead0=1, lead1=4, lead2=0, lead3=0,
                plan_X=z(B, N + 1, 4), plan_U=z(B, N, 2), status=z(B, dt=i32), acted=z(B, R, 8, dt=f32),
                terminal_obs=z(B, R, 8, dt=f32), done=z(B, dt=u8), state_i32=z(10, B, dt=i32), state_f64=z(15, B),
                ring_xy=z(B, 4, 4, 2), ring_valid=z(B, 4, dt=i32), rec_i32=z(8, B, Q, dt=i32), rec_f64=z(13, B, Q), stream=None)
    nan = float("nan")
    engine.call("mpc_plan_metrics", **dict(good, reset=1, plan_X=None, plan_U=None, status=None, acted=None, terminal_obs=None,
                                           done=None))
    engine.call("mpc_plan_metrics", **good)
    engine.call("mpc_plan_metrics", **dict(good, B=0))
    for kw, word in ((dict(B=-1), "B >= 0"), (dict(N=0), "MPC_MAX_HORIZON"), (dict(N=65), "MPC_MAX_HORIZON"),
                     (dict(R=0), "MPC_MAX_OTHERS"), (dict(R=18), "MPC_MAX_OTHERS"), (dict(Q=0), "Q >= 1"), (dict(dt=0.0), "dt > 0"),
                     (dict(dt=nan), "dt > 0"), (dict(gap=-1.0), "gap >= 0"), (dict(gap=nan), "gap >= 0"),
                     (dict(lead1=5), "lead in 0 .. N"), (dict(lead3=-1), "lead in 0 .. N"), (dict(lead0=0, lead1=0), "one lead used"),
                     (dict(order=2), "order"), (dict(state_i32=None), "null state"), (dict(ring_valid=None), "null state"),
                     (dict(rec_f64=None), "null state"), (dict(plan_X=None), "step-input"), (dict(done=None), "step-input"),
                     (dict(reset=1, state_f64=None), "null state")):
        with pytest.raises(engine.EngineError, match="mpc_plan_metrics.*" + word):
            engine.call("mpc_plan_metrics", **dict(good, **kw))
    torch.cuda.synchronize(dev)
    assert good["state_i32"][0].cpu().tolist() == [1] * B                          # one step since the reset: a refusal launches nothing
    tgood = dict(device=0, B=B, N=N, Q=Q, W=W, C=C, reset=0, plan_X=good["plan_X"], plan_U=good["plan_U"], done=good["done"],
                 slot=torch.full((B,), -1, dtype=i32, device=dev), state_i32=z(2, B, dt=i32), ring_X=z(B, W, N + 1, 4),
                 ring_U=z(B, W, N, 2), kept_X=z(C, W, N + 1, 4), kept_U=z(C, W, N, 2), stream=None)
    engine.call("mpc_plan_trace", **dict(tgood, reset=1, plan_X=None, plan_U=None, done=None, slot=None))
    engine.call("mpc_plan_trace", **tgood)
    for kw, word in ((dict(B=-1), "bad size"), (dict(N=0), "bad size"), (dict(N=65), "bad size"), (dict(Q=0), "bad size"),
                     (dict(W=0), "bad size"), (dict(W=4097), "bad size"), (dict(C=0), "bad size"), (dict(ring_X=None), "null state"),
                     (dict(kept_U=None), "null state"), (dict(slot=None), "step-input"), (dict(plan_U=None), "step-input")):
        with pytest.raises(engine.EngineError, match="mpc_plan_trace.*" + word):
            engine.call("mpc_plan_trace", **dict(tgood, **kw))
    torch.cuda.synchronize(dev)
    assert tgood["state_i32"][0].cpu().tolist() == [1] * B


# ---- 3: the evaluation ------------------------------------------------------------------------------------------------------------

def _pure():
    from mpc_rl_for_avs_amd.engine import MPCEngine
    from mpc_rl_for_avs_amd.pure_mpc import PureMPC_Agent
    return PureMPC_Agent(Env(), dict(CFG), engine=MPCEngine(horizon=20, device=0), collision_cost=False)


TRACE = dict(keep="all", capacity=64, window=200)


def _eval(agent, B=64, **kw):
    from mpc_rl_for_avs_amd import evaluate, rollout
    env = rollout.SyntheticIntersectionEnv(B, device=_dev(), seed=7, n_others=4, traffic="idm")
    return evaluate.evaluate_agent(agent, env, episodes_per_env=1, seed=7, metrics=True, **kw)


def _assert_same(a, b):
    assert set(a) == set(b)
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), k


def _assert_same_traces(a, b, planes):
    assert a.counts == b.counts
    _assert_same(a.index, b.index)
    for i in range(len(a)):
        x, y = a.episode(i), b.episode(i)
        for k in planes:
            assert x[k].tobytes() == y[k].tobytes(), (i, k)


OLD_PLANES, PLAN_PLANES = ("scene", "action", "reward", "status", "iters", "flags"), ("plan_X", "plan_U")


@pytest.fixture(scope="module")
def agent():
    return _pure()


@pytest.fixture(scope="module")
def planned(agent):
    return _eval(agent, use_graph=True, plan=True, trace=dict(TRACE, plan=True))


def test_graph_eager_and_a_second_run_are_bit_identical_with_a_plan(agent, planned):
    frames = []
    keep = lambda d: frames.append({k: d[k].cpu().numpy().copy() for k in ("plan_X", "terminal_obs", "status", "done") if k in d})
    eager = _eval(agent, use_graph=False, plan=True, trace=dict(TRACE, plan=True), on_step=keep)
    again = _eval(agent, use_graph=True, plan=True, trace=dict(TRACE, plan=True))
    for other in (eager, again):
        assert planned.steps == other.steps
        _assert_same(planned.records, other.records)
        _assert_same(planned.drive, other.drive)
        _assert_same(planned.plan, other.plan)
        _assert_same_traces(planned.traces, other.traces, OLD_PLANES + PLAN_PLANES)
    p, s = planned.plan, planned.summary()
    print("plan summary:", {k: v for k, v in s.items() if "plan" in k or "pred_err" in k or "replan" in k})
    print("lead-1 error, maximum over the episodes:", float(p["lead0_max"].max()))
    assert p["leads"] == (1, 5, 10, 20) and (p["steps"] == planned.records["steps"]).all() and p["plans_valid"].sum() > 0
    assert len(planned.traces) == 64 and planned.traces.episode(0)["plan_X"].shape[1:] == (21, 4)
    # the recorded lead errors again, in numpy, from what on_step saw: plan p's stage h against the scene after step p + h - 1
    B = 64
    steps = np.zeros(B, int)
    first_done = np.zeros(B, bool)
    n, total, top = np.zeros((4, B), int), np.zeros((4, B)), np.zeros((4, B))
    hist = []
    for f in frames[1:]:
        hist.append(f)
        t = len(hist) - 1
        live = ~first_done
        for i, h in enumerate(p["leads"]):
            if h > t + 1:
                continue
            src = hist[t + 1 - h]
            ok = live & ((src["status"] == 0) | ((src["status"] >= 5) & (src["status"] <= 7)))
            ex = f["terminal_obs"][:, 0, 1].astype(np.float64) - src["plan_X"][:, h, 0]
            ey = f["terminal_obs"][:, 0, 2].astype(np.float64) - src["plan_X"][:, h, 1]
            e = np.sqrt(ex * ex + ey * ey)
            n[i] += ok
            total[i] = np.where(ok, total[i] + e, total[i])
            top[i] = np.where(ok & (e > top[i]), e, top[i])
        first_done |= f["done"] != 0
    for i in range(4):                                                             # first episodes: every environment starts at launch 1
        assert np.array_equal(n[i], eager.plan[f"lead{i}_n"][:, 0]) and np.array_equal(top[i], eager.plan[f"lead{i}_max"][:, 0])
        assert np.array_equal(np.where(n[i] > 0, total[i] / np.maximum(n[i], 1), 0.0), eager.plan[f"lead{i}_mean"][:, 0])


def test_plan_none_is_the_evaluation_with_a_plan_in_everything_else(agent, planned):
    plain = _eval(agent, use_graph=True, trace=dict(TRACE))
    assert plain.plan is None and plain.traces.plan_X is None and plain.steps == planned.steps
    _assert_same(plain.records, planned.records)
    _assert_same(plain.drive, planned.drive)
    _assert_same_traces(plain.traces, planned.traces, OLD_PLANES)
    # the kept plan is the plan that produced the action frame: its first control is the action
    for i in range(len(planned.traces)):
        ep = planned.traces.episode(i)
        assert ep["plan_U"][:, 0].tobytes() == ep["action"].tobytes(), i


def test_a_delayed_actuator_makes_the_outcome_leave_the_plan(agent, planned):
    delayed = _eval(agent, use_graph=True, plan=True, actuation=dict(delay=2))
    a, b = planned.summary()["pred_err_lead1_mean"], delayed.summary()["pred_err_lead1_mean"]
    print(f"lead-1 error: {a:.3e} m without an actuator model, {b:.3e} m with two steps of delay")
    assert b > a


def test_the_ppo_baseline_has_no_plan():
    import policy_ref as pr
    import torch
    from mpc_rl_for_avs_amd import rollout
    ppo = rollout.PPOAgent(pr.make_policy(64, 2, -0.5, use_sde=False, seed=8).to(_dev()))
    with pytest.raises(ValueError, match="has no plan"):
        _eval(ppo, B=4, plan=True)
    with pytest.raises(ValueError, match="has no plan"):
        ppo.act_batch_torch(torch.zeros(4, 10, 8, device=_dev()), plan=True)
