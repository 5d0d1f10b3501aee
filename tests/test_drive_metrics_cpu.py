"""Safety and comfort metrics of the closed-loop evaluation on the CPU: the host build of csrc/mpc_drive_metrics.hpp and the
evaluator's torch path against a plain-Python restatement of the definitions (tests/drive_metrics_host.py), bit for bit, on
random streams with the edge cases forced; the geometry against values that need no implementation to state; evaluate_agent
with metrics on the torch environment, and unchanged without."""
import math

import numpy as np
import pytest
import torch

import drive_metrics_host as dmh
from mpc_rl_for_avs_amd import evaluate, rollout
from mpc_rl_for_avs_amd.pure_mpc import PureMPC_Agent
from test_evaluate_cpu import CFG, Env, StubEngine

DT = 0.1
T_STEPS = 80
SHAPES = [(1, 1, 1, 1), (3, 2, 2, 1), (5, 10, 17, 3), (4, 17, 128, 2), (7, 10, 18, 1)]     # B, R, M, Q
PLANES = ("rec_i32", "rec_f64", "state_i32", "state_f64")


def random_route(M, rng):
    """A polyline of M points, roughly 1.5 m apart, that turns; with M >= 4 one point is repeated (a segment of length 0)."""
    ang = np.cumsum(rng.normal(0, 0.15, M))
    ref = np.cumsum(np.stack([1.5 * np.cos(ang), 1.5 * np.sin(ang)], axis=1), axis=0) + rng.uniform(-5, 5, 2)
    if M >= 4:
        ref[2] = ref[1]
    return np.ascontiguousarray(ref)


def _scene(B, R, ref, rng, k_present=None, overlap=False):
    """[B, R, 8] f32: an ego near the route and 0 .. R - 1 other vehicles within 20 m of it, present rows first; overlap:
    row 1 is present and its rectangle overlaps the ego's."""
    k = rng.integers(0, R, B) if k_present is None else np.full(B, min(k_present, R - 1))
    h, sp = rng.uniform(-math.pi, math.pi, (B, R)), rng.uniform(0, 15, (B, R))
    xy = np.zeros((B, R, 2))
    xy[:, 0] = ref[rng.integers(0, len(ref), B)] + rng.normal(0, 1.5, (B, 2))
    xy[:, 1:] = xy[:, :1] + rng.uniform(-20, 20, (B, R - 1, 2))
    if overlap and R > 1:
        xy[:, 1] = xy[:, 0] + (0.5, -0.25)
        k = np.maximum(k, 1)
    present = np.arange(R)[None, :] <= k[:, None]
    cols = [np.ones((B, R)), xy[..., 0], xy[..., 1], sp * np.cos(h), sp * np.sin(h), h, np.sin(h), np.cos(h)]
    return (np.stack(cols, axis=-1) * present[..., None]).astype(np.float32)


def random_stream(B, R, M, Q, seed, T=T_STEPS, reset_at=40):
    """(ref_xy, steps): T steps of B environments, done with probability 0.1.  Forced: environment 0 ends an episode on its
    first step; a reset launch before step `reset_at`; a step with no other vehicle present (step 3); two overlapping
    rectangles (step 5, when R > 1).  Most environments idle after their Q episodes."""
    rng = np.random.default_rng(seed)
    ref = random_route(M, rng)
    obs = _scene(B, R, ref, rng)
    steps = [dict(reset=True, obs=obs.copy())]
    for k in range(T):
        if k == reset_at:
            obs = _scene(B, R, ref, rng)
            steps.append(dict(reset=True, obs=obs.copy()))
        tobs = _scene(B, R, ref, rng, k_present=0 if k == 3 else None, overlap=k == 5)
        # the ego mostly moves on from where it was, so that accelerations and jerks are of a driving size
        tobs[:, 0, 3:5] = obs[:, 0, 3:5] + rng.normal(0, 0.3, (B, 2)).astype(np.float32)
        done = rng.random(B) < 0.1
        if k == 0:
            done[0] = True
        obs = tobs.copy()
        fresh = _scene(B, R, ref, rng)
        obs[done] = fresh[done]
        steps.append(dict(terminal_obs=tobs, obs=obs.copy(), act=rng.normal(0, 1, (B, 2)), done=done))
    return ref, steps


def run_host(ref, steps, B, R, Q):
    h = dmh.HostDrive(B, Q, ref, DT, R)
    for s in steps:
        h.update(s, reset=bool(s.get("reset")))
    return h


def assert_planes_equal(got, want, what=""):
    for name in PLANES:
        g = np.ascontiguousarray(got[name] if isinstance(got, dict) else getattr(got, name))
        w = np.ascontiguousarray(want[name] if isinstance(want, dict) else getattr(want, name))
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name)
        if not np.array_equal(g.view(np.uint8), w.view(np.uint8)):
            idx = np.argwhere(g != w)[:5]
            raise AssertionError(f"{what} {name} differs at {idx.tolist()}: {[g[tuple(i)] for i in idx]} != "
                                 f"{[w[tuple(i)] for i in idx]}")


@pytest.mark.parametrize("B,R,M,Q", SHAPES)
def test_host_build_is_the_plain_python_restatement_bit_for_bit(B, R, M, Q):
    ref, steps = random_stream(B, R, M, Q, seed=1000 * B + R)
    h = run_host(ref, steps, B, R, Q)
    want = dmh.replay(steps, B, Q, ref, DT, R)
    assert_planes_equal(h, want, "host build vs replay")
    # the forced cases occurred
    first = [s for s in steps if not s.get("reset")]
    assert first[0]["done"][0] and run_host(ref, steps[:2], B, R, Q).rec_i32[0, 0, 0] == 1      # an episode of one step
    assert sum(1 for s in steps if s.get("reset")) == 2
    assert not first[3]["terminal_obs"][:, 1:, 0].any()
    dones = np.sum([s["done"] for s in first[40:]], axis=0)
    assert (dones > Q).any() and (h.state_i32[4] == Q).any()               # idle after the quota
    rec = h.records()
    assert not np.isnan(h.rec_f64).any() and not np.isnan(h.state_f64).any()
    assert not np.signbit(h.rec_f64).any()                                 # no -0.0 (nor anything negative)
    if R > 1:
        t = first[5]["terminal_obs"][0].astype(np.float64)                 # the overlapping rectangles of step 5
        assert t[1, 0] == 1 and dmh.host_box_gap(t[0, 1:3], t[0, [7, 6]], t[1, 1:3], t[1, [7, 6]]) == 0.0
        assert (rec["min_box_gap"] <= rec["min_centre_gap"]).all()
    else:
        assert np.isinf(rec["min_box_gap"][rec["steps"] > 0]).all()
    assert (rec["rms_jerk"][rec["steps"] == 1] == 0).all() and (rec["max_jerk"] >= rec["rms_jerk"] * (1 - 1e-15)).all()


@pytest.mark.parametrize("B,R,M,Q", SHAPES)
def test_torch_backend_is_the_host_build_bit_for_bit(B, R, M, Q):
    ref, steps = random_stream(B, R, M, Q, seed=1000 * B + R)
    h = run_host(ref, steps, B, R, Q)
    d = evaluate.DriveMetrics(B, Q, "cpu", "torch", ref, DT, R)
    for s in steps:
        t = {k: torch.as_tensor(v) for k, v in s.items() if k != "reset"}
        if s.get("reset"):
            d.update(None, t["obs"], None, None, reset=True)
        else:
            d.update(t["terminal_obs"], t["obs"], t["act"], t["done"])
    assert_planes_equal({n: getattr(d, n).numpy() for n in PLANES}, h, "torch vs host build")
    got, want = d.records(), h.records()
    assert set(got) == set(evaluate.DRIVE_I32 + evaluate.DRIVE_F64) == set(dmh.I32 + dmh.F64)
    for k in got:
        assert np.array_equal(got[k], want[k]), k


# ---- geometry, stated without any implementation ---------------------------------------------------------------------------

def _torch_box_gap(p, h, q, g):
    t = lambda v: torch.tensor([float(v)], dtype=torch.float64)
    return float(evaluate._box_gap(t(p[0]), t(p[1]), t(h[0]), t(h[1]), t(q[0]), t(q[1]), t(g[0]), t(g[1]))[0])


def _torch_ttc(r, u):
    t = lambda v: torch.tensor([float(v)], dtype=torch.float64)
    return float(evaluate._ttc(t(r[0]), t(r[1]), t(u[0]), t(u[1]))[0])


BOX_GAPS = [dmh.host_box_gap, lambda p, h, q, g: dmh.box_gap(p[0], p[1], h[0], h[1], q[0], q[1], g[0], g[1]), _torch_box_gap]
TTCS = [dmh.host_ttc, lambda r, u: dmh.ttc(r[0], r[1], u[0], u[1]), _torch_ttc]
IDS = ["host", "python", "torch"]


@pytest.mark.parametrize("gap", BOX_GAPS, ids=IDS)
def test_box_gap_of_known_configurations(gap):
    east, north = (1.0, 0.0), (0.0, 1.0)
    assert gap((0.0, 0.0), east, (0.0, 3.5), east) == 1.5                  # side by side: 3.5 - 2 * 1.0
    assert gap((0.0, 0.0), east, (7.0, 0.0), east) == 2.0                  # nose to tail: 7.0 - 2 * 2.5
    assert gap((0.0, 0.0), east, (6.0, 4.0), east) == math.sqrt(5.0)       # corner to corner: (6 - 5, 4 - 2), exact in f64
    assert gap((0.0, 0.0), east, (0.0, 0.0), north) == 0.0                 # a cross: no corner inside the other rectangle
    assert gap((3.0, -2.0), east, (3.0, -2.0), east) == 0.0


@pytest.mark.parametrize("ttc", TTCS, ids=IDS)
def test_time_to_collision_of_known_configurations(ttc):
    assert ttc((20.0, 0.0), (-10.0, 0.0)) == 1.75                          # (20 - 2.5) / 10
    assert ttc((20.0, 0.0), (10.0, 0.0)) == math.inf                       # receding
    assert ttc((20.0, 0.0), (0.0, 0.0)) == math.inf                        # same velocity
    assert ttc((20.0, 0.0), (0.0, -10.0)) == math.inf                      # passes 20 m away
    assert ttc((2.5, 0.0), (-10.0, 0.0)) == 0.0 and ttc((1.0, 1.0), (5.0, 5.0)) == 0.0     # |r| <= 2.5


def test_cross_track_error_of_known_configurations():
    line = np.array([[0.0, 0.0], [2.0, 0.0]])
    d = evaluate.DriveMetrics(1, 1, "cpu", "torch", line, DT, 1)
    t = lambda v: torch.tensor([[float(v)]], dtype=torch.float64)
    tx = lambda p: float(evaluate._sqrt(evaluate._seg2(t(p[0]), t(p[1]), d._e0[None, :, 0], d._e0[None, :, 1], d._d[None, :, 0],
                                                  d._d[None, :, 1]).min(dim=1).values)[0])
    for xte in (dmh.host_xte, lambda p, r: dmh.xte(p[0], p[1], r), lambda p, r: tx(p)):
        assert xte((1.0, 1.0), line) == 1.0
        assert xte((3.0, 0.0), line) == 1.0                                # beyond the end: the distance to the end point
        assert xte((-3.0, 4.0), line) == 5.0
    for xte in (dmh.host_xte, lambda p, r: dmh.xte(p[0], p[1], r)):
        assert xte((3.0, 4.0), np.array([[0.0, 0.0]])) == 5.0              # M == 1: the distance to the point
        assert xte((1.0, 1.0), np.array([[0.0, 0.0], [0.0, 0.0], [2.0, 0.0]])) == 1.0      # a repeated point


H_SAMPLE = 0.0025


def _boundary(p, ang):
    """The rectangle's boundary as points H_SAMPLE apart along each edge, in order around it (5600 points)."""
    c, s = math.cos(ang), math.sin(ang)
    ax, nrm = np.array([c, s]), np.array([-s, c])
    cs = [np.asarray(p) + a * 2.5 * ax + b * 1.0 * nrm for a, b in ((1, 1), (-1, 1), (-1, -1), (1, -1))]
    pts = []
    for k in range(4):
        e0, e1 = cs[k], cs[(k + 1) % 4]
        n = int(round(np.linalg.norm(e1 - e0) / H_SAMPLE))
        pts.append(e0 + (np.arange(n) / n)[:, None] * (e1 - e0))
    return np.concatenate(pts)


def _sampled_gap(a, b, stride=32):
    """min |x - y| over the sampled boundaries.  Coarse pass on every `stride`-th point: s_coarse >= s.  The closest fine pair
    lies within stride / 2 samples of coarse points a', b' with |a' - b'| <= s + stride * H_SAMPLE <= s_coarse + stride *
    H_SAMPLE, so only the cells of such coarse points are compared point by point."""
    dist = lambda x, y: np.sqrt(((x[:, None, :] - y[None, :, :]) ** 2).sum(-1))
    ca, cb = a[::stride], b[::stride]
    dc = dist(ca, cb)
    lim = dc.min() + stride * H_SAMPLE
    cells = lambda pts, hit: pts[np.unique((np.nonzero(hit)[0][:, None] * stride +
                                            np.arange(-stride // 2, stride // 2 + 1)[None, :]).ravel() % len(pts))]
    return dist(cells(a, (dc <= lim).any(axis=1)), cells(b, (dc <= lim).any(axis=0))).min(), dc.min()


def test_box_gap_against_sampled_boundaries_on_random_pairs():
    """Sampling can only overestimate the gap, by at most H_SAMPLE / 2 on each boundary: s - h <= gap <= s (with 1e-12 for
    the roundings of the sampled distances themselves)."""
    rng = np.random.default_rng(42)
    n = 0
    while n < 200:
        p, q = rng.uniform(-3, 3, 2), rng.uniform(-3, 3, 2) + rng.uniform(-9, 9, 2)
        ha, ga = rng.uniform(-math.pi, math.pi, 2)
        s, s_coarse = _sampled_gap(_boundary(p, ha), _boundary(q, ga))
        if s_coarse < 0.2:                       # overlapping or nearly touching: sampling cannot tell a gap from a crossing
            continue
        n += 1
        h, g = (math.cos(ha), math.sin(ha)), (math.cos(ga), math.sin(ga))
        gap = dmh.host_box_gap(p, h, q, g)
        assert s - H_SAMPLE - 1e-12 <= gap <= s + 1e-12, (p, ha, q, ga, gap, s)
        assert _torch_box_gap(p, h, q, g) == gap


# ---- the evaluator ---------------------------------------------------------------------------------------------------------

TODAY_SUMMARY = {"success_rate", "collision_rate", "avg_steps", "avg_speed", "avg_travel_time", "mean_return", "unsolved_frac",
                 "episodes", "env_steps", "seconds", "env_steps_per_s"}
TODAY_STEP = {"ego", "done", "truncated", "crashed", "arrived", "reward", "status", "iters"}
DRIVE_SUMMARY = {"near_miss_rate", "min_box_gap_mean", "min_ttc_median", "episodes_with_traffic", "ttc_exposure",
                 "hard_brake_rate", "max_abs_alon_mean", "max_abs_alat_mean", "rms_jerk_mean", "max_steer_rate_mean", "mean_xte",
                 "max_xte"}


def _evaluate(B, Q, traffic="constant", **kw):
    env = rollout.SyntheticIntersectionEnv(B, device="cpu", seed=3, n_others=4, backend="torch", traffic=traffic)
    agent = PureMPC_Agent(Env(), dict(CFG), engine=StubEngine(), collision_cost=True)
    seen = []
    take = lambda d: {k: (v.clone().numpy() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
    res = evaluate.evaluate_agent(agent, env, episodes_per_env=Q, use_graph=False, poll_every=5,
                                  on_step=lambda d: seen.append(take(d)), **kw)
    return res, seen, env


@pytest.mark.parametrize("traffic", ["constant", "idm"])
def test_evaluate_agent_with_metrics_on_the_cpu_environment(traffic):
    B, Q = 4, 2
    res, seen, env = _evaluate(B, Q, traffic, metrics=True)
    d = res.drive
    assert set(d) == set(evaluate.DRIVE_I32 + evaluate.DRIVE_F64)
    assert np.array_equal(d["steps"], res.records["steps"])                # slot for slot the same episodes
    assert set(seen[0]) == {"reset", "ego", "obs"} and set(seen[1]) == TODAY_STEP | {"terminal_obs", "obs", "act"}
    want = dmh.replay(seen, B, Q, env.ref_xy.numpy(), env.dt, rollout.VEHICLES_COUNT)
    for i, k in enumerate(evaluate.DRIVE_I32):
        assert np.array_equal(d[k], want["rec_i32"][i]), k
    for i, k in enumerate(evaluate.DRIVE_F64):
        assert np.array_equal(d[k].view(np.int64), want["rec_f64"][i].view(np.int64)), k
    s = res.summary()
    assert set(s) == TODAY_SUMMARY | DRIVE_SUMMARY
    assert 0 <= s["near_miss_rate"] <= 100 - s["collision_rate"] and 0 <= s["ttc_exposure"] <= 1
    assert 0 <= s["hard_brake_rate"] <= 1 and s["episodes_with_traffic"] == int(np.isfinite(d["min_box_gap"]).sum())
    assert s["max_xte"] == d["max_xte"].max() and s["mean_xte"] == pytest.approx(d["mean_xte"].mean())
    # the environment clamps the acceleration to 5 m/s^2; turning adds v (1 - cos(dtheta)) / dt < 0.05 to what is observed
    assert d["max_abs_alon"].max() < 5.05
    # an episode that crashed got closer than the crash distance, and its rectangles at least as close
    crashed = res.records["collision"]
    assert (d["min_centre_gap"][crashed] < evaluate.CRASH_DISTANCE + 1e-4).all()          # f32 observation of the f64 scene
    assert (d["min_box_gap"] <= d["min_centre_gap"]).all()


def test_evaluate_agent_without_metrics_is_what_it_was():
    res, seen, _ = _evaluate(8, 1)
    assert res.drive is None
    assert set(res.summary()) == TODAY_SUMMARY
    assert set(seen[0]) == {"reset", "ego"} and all(set(s) == TODAY_STEP for s in seen[1:])
    with_metrics, _, _ = _evaluate(8, 1, metrics=True)
    for k, v in res.records.items():
        assert np.array_equal(v, with_metrics.records[k]), k


def test_drive_metrics_refuses_invalid_arguments():
    ref = np.zeros((3, 2))
    for kw in (dict(Q=0), dict(rows=0), dict(rows=18), dict(dt=0.0), dict(ref_xy=None), dict(ref_xy=np.zeros((129, 2))),
               dict(ref_xy=np.zeros((0, 2))), dict(backend="foo")):
        args = dict(B=2, Q=1, device="cpu", backend="torch", ref_xy=ref, dt=DT, rows=10)
        args.update(kw)
        with pytest.raises(ValueError):
            evaluate.DriveMetrics(**args)
    d = evaluate.DriveMetrics(2, 1, "cpu", "torch", ref, DT, 10)
    with pytest.raises(ValueError):
        d.update(None, torch.zeros(2, 9, 8), None, None, reset=True)


def test_kernel_backed_drive_metrics_refuse_a_bad_tensor_before_any_library_call(monkeypatch):
    """backend "hip" built on the CPU: the constructor loads no library, and every bad tensor is a ValueError before the
    entry point is even looked up"""
    from mpc_rl_for_avs_amd import engine

    def caller(name):
        raise AssertionError(f"{name} reached the library")

    monkeypatch.setattr(engine, "caller", caller)
    d = evaluate.DriveMetrics(2, 1, "cpu", "hip", np.zeros((3, 2)), DT, 10)
    good = dict(terminal_obs=torch.zeros(2, 10, 8), obs=torch.zeros(2, 10, 8), action=torch.zeros(2, 2, dtype=torch.float64),
                done=torch.zeros(2, dtype=torch.bool))
    bad = dict(terminal_obs=[torch.zeros(2, 10, 8, device="meta"), torch.zeros(2, 10, 8, dtype=torch.float64),
                             torch.zeros(2, 9, 8), torch.zeros(2, 10, 16)[:, :, ::2]],
               obs=[torch.zeros(2, 10, 8, device="meta"), torch.zeros(2, 10, 8, dtype=torch.float16), torch.zeros(1, 10, 8),
                    torch.zeros(2, 8, 10).transpose(1, 2)],
               action=[torch.zeros(2, 2, dtype=torch.float64, device="meta"), torch.zeros(2, 2),
                       torch.zeros(2, 3, dtype=torch.float64), torch.zeros(2, 4, dtype=torch.float64)[:, ::2]],
               done=[torch.zeros(2, dtype=torch.bool, device="meta"), torch.zeros(2, dtype=torch.int32),
                     torch.zeros(3, dtype=torch.bool), torch.zeros(4, dtype=torch.uint8)[::2]])
    for name, tensors in bad.items():
        for t in tensors:
            with pytest.raises(ValueError, match=name):
                d.update(**dict(good, **{name: t}))
    for t in bad["obs"]:
        with pytest.raises(ValueError, match="obs"):
            d.update(None, t, None, None, reset=True)
    with pytest.raises(AssertionError, match="mpc_drive_metrics reached the library"):
        d.update(**good)                                     # the checks above were the only thing in the way
