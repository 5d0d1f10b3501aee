"""The perception model of the closed-loop evaluation on the CPU: the host build of csrc/mpc_perception.hpp and the
evaluator's CPU path against a plain-Python restatement of the model (tests/perception_host.py), bit for bit, on random streams
with the edge cases forced; occlusion and range against answers that need no implementation to state; the draws; evaluate_agent
with a perception model on the torch environment, and unchanged without; a sanitizer run of the host build in a stand-alone
program."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import conftest
import drive_metrics_host as dmh
import perception_host as ph
from mpc_rl_for_avs_amd import evaluate, rollout
from mpc_rl_for_avs_amd.pure_mpc import PureMPC_Agent
from test_evaluate_cpu import CFG, Env, StubEngine

T_STEPS, RESET_AT = 40, 20
SHAPES = [(1, 1, 0), (3, 2, 1), (5, 10, 4), (4, 17, 8)]                                  # B, R, S
STEP_NONE, STEP_ALL, STEP_GAP, STEP_OVERLAP, STEP_INSIDE, STEP_DROP_ALL = 3, 4, 5, 6, 7, 8
KEY = dict(seed=0x9E3779B97F4A7C15, env_offset=7)
ALL_ON = dict(range=30.0, occlusion=True, min_points=2, p_drop=0.3, sigma_pos=0.2, sigma_vel=0.3, sigma_head=0.02, **KEY)
PARAMS = {"off": dict(KEY), "range": dict(range=30.0, **KEY), "occlusion": dict(occlusion=True, **KEY),
          "occlusion3": dict(occlusion=True, min_points=3, **KEY), "dropout": dict(p_drop=0.3, **KEY),
          "pos": dict(sigma_pos=0.2, **KEY), "vel": dict(sigma_vel=0.3, **KEY), "head": dict(sigma_head=0.02, **KEY),
          "all": ALL_ON}


def random_occluders(S, rng):
    """S rotated rectangles [S, 4, 2] (corners in order) around the origin."""
    c, a = rng.uniform(-35, 35, (S, 2)), rng.uniform(-math.pi, math.pi, S)
    hw, hh = rng.uniform(2, 10, S), rng.uniform(2, 10, S)
    ax, ay = np.stack([np.cos(a), np.sin(a)], axis=1), np.stack([-np.sin(a), np.cos(a)], axis=1)
    sg = [(-1, -1), (1, -1), (1, 1), (-1, 1)]
    return np.ascontiguousarray(np.stack([c + s * hw[:, None] * ax + t * hh[:, None] * ay for s, t in sg], axis=1))


def scene(B, R, rng, kind=None):
    """[B, R, 8] f32: an ego within 10 m of the origin and other vehicles within 45 m of it.  Present rows first, unless kind
    is "gap" (row 1 absent, row 2 present) or "scattered" (any pattern); "none" / "all": no / every other row present;
    "overlap": rows 1 and 2 present with overlapping rectangles; "inside": row 1 present, the ego's position in its rectangle."""
    h, sp = rng.uniform(-math.pi, math.pi, (B, R)), rng.uniform(0, 15, (B, R))
    xy = np.zeros((B, R, 2))
    xy[:, 0] = rng.uniform(-10, 10, (B, 2))
    xy[:, 1:] = xy[:, :1] + rng.uniform(-45, 45, (B, R - 1, 2))
    k = rng.integers(0, R, B)
    k = {"none": 0 * k, "all": 0 * k + R - 1, "overlap": np.maximum(k, min(2, R - 1)), "inside": np.maximum(k, min(1, R - 1)),
         "gap": np.maximum(k, min(2, R - 1))}.get(kind, k)
    present = np.arange(R)[None, :] <= k[:, None]
    if kind == "scattered":
        present = rng.random((B, R)) < 0.5
    if kind == "gap" and R > 2:
        present[:, 1] = False
    if kind == "overlap" and R > 2:
        xy[:, 2] = xy[:, 1] + (0.5, -0.25)
    if kind == "inside" and R > 1:
        xy[:, 1] = xy[:, 0] + (0.5, -0.25)
    present[:, 0] = True
    cols = [np.ones((B, R)), xy[..., 0], xy[..., 1], sp * np.cos(h), sp * np.sin(h), h, np.sin(h), np.cos(h)]
    full = np.stack(cols, axis=-1)
    if kind == "scattered":                  # absent rows hold -0.0 where the value was negative: the output must not
        return (full * present[..., None]).astype(np.float32)
    return np.where(present[..., None], full, 0.0).astype(np.float32)


FORCED = {STEP_NONE: "none", STEP_ALL: "all", STEP_GAP: "gap", STEP_OVERLAP: "overlap", STEP_INSIDE: "inside"}


def random_stream(B, R, S, seed, T=T_STEPS):
    """(occluders [S, 4, 2], steps): T launches on random scenes, the first and launch RESET_AT with reset; the FORCED scenes;
    launch STEP_DROP_ALL runs with p_drop = 1; from launch 30 on the present rows are scattered."""
    rng = np.random.default_rng(seed)
    occ = random_occluders(S, rng)
    steps = []
    for k in range(T):
        s = dict(obs=scene(B, R, rng, FORCED.get(k, "scattered" if k >= 30 else None)), reset=k in (0, RESET_AT))
        if k == STEP_DROP_ALL:
            s["p_drop"] = 1.0
        steps.append(s)
    return occ, steps


def stream_of(B, R, S):
    return random_stream(B, R, S, seed=1000 * B + R)


def run_host(occ, steps, B, R, params):
    h = ph.HostPerception(B, R, occ, **params)
    outs = []
    for s in steps:
        over = {"p_drop": s["p_drop"]} if "p_drop" in s else {}
        seen = h.apply(s["obs"], reset=s["reset"], **over)
        outs.append((seen, h.row_class.copy()))
    return outs, h.counts.copy(), h.ctr.copy()


def run_class(occ, steps, B, R, params, device="cpu", backend="torch"):
    p = evaluate.Perception(B, device, backend, R=R, occluders=occ, **params)
    outs = []
    for s in steps:
        obs = torch.from_numpy(s["obs"]).to(p.device)
        out = torch.full_like(obs, float("nan"))
        keep = p.p_drop
        p.p_drop = s.get("p_drop", keep)
        p.apply(obs, out, reset=s["reset"])
        p.p_drop = keep
        outs.append((out.cpu().numpy(), p.row_class.cpu().numpy().copy()))
    return outs, p.counts.cpu().numpy(), p.ctr.cpu().numpy()


def assert_runs_equal(got, want, what):
    (g_outs, g_counts, g_ctr), (w_outs, w_counts, w_ctr) = got, want
    assert len(g_outs) == len(w_outs)
    for k, ((gs, gc), (ws, wc)) in enumerate(zip(g_outs, w_outs)):
        assert gs.dtype == ws.dtype == np.float32 and gs.shape == ws.shape, (what, k)
        if not np.array_equal(gs.view(np.uint32), ws.view(np.uint32)):
            idx = np.argwhere(gs.view(np.uint32) != ws.view(np.uint32))[:5]
            raise AssertionError(f"{what}: obs_seen of launch {k} differs at {idx.tolist()}: "
                                 f"{[gs[tuple(i)] for i in idx]} != {[ws[tuple(i)] for i in idx]}")
        assert np.array_equal(gc, wc), (what, "row_class", k)
    assert g_counts.dtype == w_counts.dtype == np.int64 and np.array_equal(g_counts, w_counts), (what, "counts")
    assert np.array_equal(g_ctr, w_ctr), (what, "ctr")


def _inside(p, row):
    """p strictly inside the 5 x 2 rectangle of the row"""
    dx, dy, c, s = p[0] - row[1], p[1] - row[2], row[7], row[6]
    return abs(dx * c + dy * s) < 2.5 and abs(dy * c - dx * s) < 1.0


@pytest.mark.parametrize("name", list(PARAMS))
@pytest.mark.parametrize("B,R,S", SHAPES)
def test_host_build_is_the_plain_python_restatement_bit_for_bit(B, R, S, name):
    params = PARAMS[name]
    occ, steps = stream_of(B, R, S)
    got = run_host(occ, steps, B, R, params)
    want = ph.replay(steps, B, R, occ, **params)
    assert_runs_equal(got, want, "host build vs restatement")
    outs, counts, ctr = got
    # the forced cases occurred
    obs = lambda k: steps[k]["obs"].astype(np.float64)
    assert [s["reset"] for s in steps].count(True) == 2 and (ctr == T_STEPS - RESET_AT).all()
    assert not obs(STEP_NONE)[:, 1:, 0].any() and not outs[STEP_NONE][0][:, 1:].any()
    assert (obs(STEP_ALL)[:, :, 0] == 1).all()
    assert (outs[STEP_DROP_ALL][1][:, 1:] != ph.SEEN).all() and not outs[STEP_DROP_ALL][0][:, 1:].any()
    if R > 1:
        t = obs(STEP_INSIDE)[0]
        assert t[1, 0] == 1 and _inside(t[0, 1:3], t[1])
    if R > 2:
        t = obs(STEP_GAP)
        assert not t[:, 1, 0].any() and (t[:, 2, 0] == 1).all()
        t = obs(STEP_OVERLAP)[0]
        assert t[1, 0] == t[2, 0] == 1 and dmh.host_box_gap(t[1, 1:3], t[1, [7, 6]], t[2, 1:3], t[2, [7, 6]]) == 0.0
    # the invariants of every output
    for k, (seen, cls) in enumerate(outs):
        true = steps[k]["obs"]
        assert not np.isnan(seen).any(), k                                     # every element written, none NaN
        there = seen[:, :, 0] != 0
        assert not np.signbit(seen[~there]).any(), k                           # a zero row is +0.0 in every column
        assert not seen[~there].any() and (np.diff(there.astype(np.int8), axis=1) <= 0).all(), k      # contiguous
        assert np.array_equal(seen[:, 0].view(np.uint32), true[:, 0].view(np.uint32)) and (cls[:, 0] == ph.SEEN).all()
        assert np.array_equal(there[:, 1:].sum(axis=1), (cls[:, 1:] == ph.SEEN).sum(axis=1))
        assert np.array_equal(cls[:, 1:] == ph.ABSENT, true[:, 1:, 0] == 0)
    assert (counts[0] == counts[1:].sum(axis=0)).all()
    assert R == 1 or any(np.signbit(s["obs"][s["obs"][:, :, 0] == 0]).any() for s in steps)     # ... with -0.0 in the input
    # a feature that is on shows, one that is off does not (rows enough to tell: R >= 10)
    if R >= 10:
        on = dict(ph.OFF, **params)
        every = np.concatenate([cls[:, 1:].ravel() for _, cls in outs])         # all launches (the counts restart at the reset)
        total = {k: int((every == c).sum()) for k, c in zip(ph.COUNTS[1:], (ph.SEEN, ph.OUT_OF_RANGE, ph.OCCLUDED, ph.DROPPED))}
        assert (total["out_of_range"] > 0) == (on["range"] < ph.INF)
        assert (total["occluded"] > 0) == on["occlusion"]
        assert total["dropped"] > 0 and total["seen"] > 0                      # launch STEP_DROP_ALL drops in every set


@pytest.mark.parametrize("name", list(PARAMS))
@pytest.mark.parametrize("B,R,S", SHAPES)
def test_torch_backend_is_the_host_build_bit_for_bit(B, R, S, name):
    occ, steps = stream_of(B, R, S)
    assert_runs_equal(run_class(occ, steps, B, R, PARAMS[name]), run_host(occ, steps, B, R, PARAMS[name]), "torch vs host build")


@pytest.mark.parametrize("run", [run_host, run_class], ids=["host", "torch"])
@pytest.mark.parametrize("B,R,S", SHAPES)
def test_all_parameters_off_is_the_identity_on_contiguous_inputs(B, R, S, run):
    occ, steps = stream_of(B, R, S)
    outs, counts, _ = run(occ, steps, B, R, dict(KEY))
    checked = 0
    for k, (seen, cls) in enumerate(outs):
        true = steps[k]["obs"]
        there = true[:, 1:, 0] != 0
        if "p_drop" in steps[k] or (np.diff(there.astype(np.int8), axis=1) > 0).any() or np.signbit(true[:, 1:][~there]).any():
            continue                                     # dropout forced, a gap, or absent rows that are not +0.0
        assert seen.tobytes() == true.tobytes(), k
        checked += 1
    assert checked >= 25


# ---- answers stated without an implementation --------------------------------------------------------------------------------

def _row(x, y, heading=0.0, present=1.0):
    return [present, x, y, 0.0, 0.0, heading, math.sin(heading), math.cos(heading)] if present else [0.0] * 8


def _classes_host(rows, occ, **params):
    obs = np.array([rows], np.float32)
    h = ph.HostPerception(1, len(rows), occ, **params)
    h.apply(obs, reset=True)
    return h.row_class[0].tolist()


def _classes_python(rows, occ, **params):
    obs = np.array([rows], np.float32)
    outs, _, _ = ph.replay([dict(obs=obs, reset=True)], 1, len(rows), occ, **params)
    return outs[0][1][0].tolist()


def _classes_torch(rows, occ, **params):
    obs = torch.tensor([rows], dtype=torch.float32)
    p = evaluate.Perception(1, "cpu", "torch", R=len(rows), occluders=occ, **params)
    p.apply(obs, torch.empty_like(obs), reset=True)
    return p.row_class[0].tolist()


CLASSES = [_classes_host, _classes_python, _classes_torch]
IDS = ["host", "python", "torch"]
EGO, A = _row(0.0, 0.0), _row(10.0, 0.0)
S, O = ph.SEEN, ph.OCCLUDED


@pytest.mark.parametrize("classes", CLASSES, ids=IDS)
def test_occlusion_by_a_vehicle_of_known_configurations(classes):
    for m in range(1, 6):
        # B straight behind A: the sight lines to its centre and its four corners all pass through A
        assert classes([EGO, A, _row(25.0, 0.0)], None, occlusion=True, min_points=m) == [S, S, O]
        # B 8 m to the side: every sight line passes above A (at x = 12.5 the lowest is at y = 7 * 12.5 / 27.5 > 1)
        assert classes([EGO, A, _row(25.0, 8.0)], None, occlusion=True, min_points=m) == [S, S, S]
    # B at (25, 3): the sight lines to (27.5, 4) and (22.5, 4) pass A's rear edge x = 7.5 at y = 1.09 and 1.33, above A; those
    # to (22.5, 2), (27.5, 2) and the centre (25, 3) at y = 0.67, 0.55 and 0.9, through it
    for m, want in ((1, S), (2, S), (3, O), (4, O), (5, O)):
        assert classes([EGO, A, _row(25.0, 3.0)], None, occlusion=True, min_points=m) == [S, S, want]
    # without occlusion nothing is hidden; an absent A hides nothing; the order of the rows does not matter
    assert classes([EGO, A, _row(25.0, 0.0)], None) == [S, S, S]
    assert classes([EGO, _row(0, 0, present=0.0), _row(25.0, 0.0)], None, occlusion=True) == [S, ph.ABSENT, S]
    assert classes([EGO, _row(25.0, 0.0), A], None, occlusion=True) == [S, O, S]
    # a vehicle that is itself out of range or dropped still blocks the view
    assert classes([EGO, A, _row(25.0, 0.0)], None, occlusion=True, p_drop=1.0) == [S, ph.DROPPED, O]
    far = [_row(0.0, 0.0), _row(25.0, 0.0), _row(40.0, 0.0)]
    assert classes(far, None, occlusion=True, range=20.0) == [S, ph.OUT_OF_RANGE, ph.OUT_OF_RANGE]
    assert classes(far, None, occlusion=True, range=30.0) == [S, S, ph.OUT_OF_RANGE]


def test_the_crossing_test_is_strict():
    for crosses in (ph.host_crosses, ph.crosses):
        p, s = (0.0, 0.0), (15.0, 2.0)                   # passes exactly through A's corner (7.5, 1)
        corners = [(12.5, 1.0), (7.5, 1.0), (7.5, -1.0), (12.5, -1.0)]
        assert not any(crosses(p, s, corners[k], corners[(k + 1) % 4]) for k in range(4))
        assert crosses(p, (15.0, 1.0), corners[1], corners[2])                 # through the rear edge at y = 0.5
        assert not crosses(p, (7.5, 0.5), corners[1], corners[2])              # ends on the edge: touching
        assert not crosses((7.5, -3.0), (7.5, 3.0), corners[1], corners[2])    # collinear overlap
        assert not crosses(p, (5.0, 0.0), corners[1], corners[2])              # stops short


@pytest.mark.parametrize("classes", CLASSES, ids=IDS)
def test_occlusion_by_a_building_of_known_configuration(classes):
    square = np.array([[[-40.0, 10.0], [-10.0, 10.0], [-10.0, 40.0], [-40.0, 40.0]]])
    assert np.array_equal(evaluate.corner_buildings()[1], square[0])           # the quadrant x < 0, y > 0
    ego = _row(2.0, 45.0, -math.pi / 2)
    # from (2, 45) the line to (-30, 2) enters the square through x = -10 at y = 28.9 and leaves through y = 10 at x = -24;
    # the line to (2, 20) runs along x = 2, outside
    got = classes([ego, _row(-30.0, 2.0), _row(2.0, 20.0, -math.pi / 2)], square, occlusion=True)
    assert got == [S, O, S]
    assert classes([ego, _row(-30.0, 2.0), _row(2.0, 20.0, -math.pi / 2)], square) == [S, S, S]
    b = evaluate.corner_buildings(setback=6.0, size=30.0, road_half_width=4.0)
    assert b.shape == (4, 4, 2) and sorted(map(tuple, np.sign(b.mean(axis=1)).tolist())) == [(-1, -1), (-1, 1), (1, -1), (1, 1)]
    assert np.abs(b).min() == 10.0 and np.abs(b).max() == 40.0


@pytest.mark.parametrize("classes", CLASSES, ids=IDS)
def test_range_is_inclusive_to_the_last_bit(classes):
    one_ulp_further = float(np.nextafter(np.float32(10.0), np.float32(np.inf)))
    assert classes([EGO, _row(10.0, 0.0)], None, range=10.0) == [S, S]
    assert classes([EGO, _row(one_ulp_further, 0.0)], None, range=10.0) == [S, ph.OUT_OF_RANGE]
    assert classes([EGO, _row(6.0, 8.0)], None, range=10.0) == [S, S]          # 36 + 64 = 100, exact
    assert classes([EGO, _row(1e6, 0.0)], None) == [S, S]                      # off: +inf


# ---- the draws ---------------------------------------------------------------------------------------------------------------

def test_noise_sample_statistics_and_restatement():
    n = ph.host_noise(KEY["seed"], 3, 5, 0, 100000)
    assert abs(n.mean()) < 0.02 and abs(n.var() - 1.0) < 0.03
    assert np.abs(n).max() <= 2.0 * 1.7320508075688772
    key = ph.rng_key(KEY["seed"] ^ ph.SALT, 3, 5)
    assert [ph.unit_noise(key, 4 * j) for j in range(200)] == n[:200].tolist()


@pytest.mark.parametrize("run", [run_host, run_class], ids=["host", "torch"])
def test_draws_are_keyed_by_the_global_environment_id(run):
    R, T = 10, 6
    rng = np.random.default_rng(5)
    one = scene(1, R, rng, "all")
    steps = [dict(obs=np.repeat(one, 6, axis=0), reset=k == 0) for k in range(T)]      # six environments, the same scene
    params = dict(ALL_ON, range=ph.INF, occlusion=False, env_offset=0)
    outs, counts, _ = run(None, steps, 6, R, params)
    for k, (seen, cls) in enumerate(outs):
        for b in range(1, 6):                            # different env_offset + b: different draws
            assert not np.array_equal(seen[0], seen[b]), (k, b)
        if k:                                            # and different draws on every launch
            assert not np.array_equal(seen, outs[k - 1][0])
    # sharding: the same (seed, id, ctr) gives the same draws on any B and at any position in the batch
    for lo, hi in ((0, 3), (3, 6), (5, 6), (1, 5)):
        part = [dict(obs=s["obs"][lo:hi], reset=s["reset"]) for s in steps]
        p_outs, p_counts, _ = run(None, part, hi - lo, R, dict(params, env_offset=lo))
        for (seen, cls), (ps, pc) in zip(outs, p_outs):
            assert ps.tobytes() == seen[lo:hi].tobytes() and np.array_equal(pc, cls[lo:hi])
        assert np.array_equal(p_counts, counts[:, lo:hi])
    # another seed: other draws
    other, _, _ = run(None, steps, 6, R, dict(params, seed=KEY["seed"] + 1))
    assert not np.array_equal(other[0][0], outs[0][0])


# ---- the evaluator -----------------------------------------------------------------------------------------------------------

TODAY_SUMMARY = {"success_rate", "collision_rate", "avg_steps", "avg_speed", "avg_travel_time", "mean_return", "unsolved_frac",
                 "episodes", "env_steps", "seconds", "env_steps_per_s"}
TODAY_STEP = {"ego", "done", "truncated", "crashed", "arrived", "reward", "status", "iters"}
REAL = dict(range=40.0, occlusion=True, occluders=evaluate.corner_buildings(), p_drop=0.05, sigma_pos=0.2, sigma_vel=0.3,
            sigma_head=0.02, seed=11)


def _evaluate(B, Q, traffic="constant", **kw):
    env = rollout.SyntheticIntersectionEnv(B, device="cpu", seed=3, n_others=4, backend="torch", traffic=traffic)
    agent = PureMPC_Agent(Env(), dict(CFG), engine=StubEngine(), collision_cost=True)
    seen = []
    take = lambda d: {k: (v.clone().numpy() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
    res = evaluate.evaluate_agent(agent, env, episodes_per_env=Q, use_graph=False, poll_every=5,
                                  on_step=lambda d: seen.append(take(d)), **kw)
    return res, seen, env


def _assert_same_records(a, b):
    assert set(a) == set(b)
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), k


@pytest.mark.parametrize("traffic", ["constant", "idm"])
def test_evaluate_agent_with_everything_off_is_evaluate_agent_without(traffic):
    base, seen0, _ = _evaluate(6, 1, traffic, metrics=True)
    off, seen1, env = _evaluate(6, 1, traffic, metrics=True, perception={})
    _assert_same_records(base.records, off.records)
    _assert_same_records(base.drive, off.drive)
    assert base.steps == off.steps and base.perception is None and set(base.summary()) == set(off.summary()) - \
        {"seen_frac", "occluded_frac", "out_of_range_frac", "dropped_frac"}
    p = off.perception
    assert p["present"] == p["seen"] > 0 and p["out_of_range"] == p["occluded"] == p["dropped"] == 0
    for s0, s1 in zip(seen0, seen1):
        assert set(s1) == set(s0) | {"seen", "row_class"}
        assert s1["seen"].tobytes() == s1["obs"].tobytes() == s0["obs"].tobytes()
    given = evaluate.Perception(6, "cpu", "torch", env_offset=0)               # an instance instead of a dict
    again, _, _ = _evaluate(6, 1, traffic, metrics=True, perception=given)
    _assert_same_records(base.records, again.records)
    assert again.perception == given.totals() == p


def test_evaluate_agent_without_perception_is_what_it_was():
    res, seen, _ = _evaluate(8, 1)
    assert res.perception is None and set(res.summary()) == TODAY_SUMMARY
    assert set(seen[0]) == {"reset", "ego"} and all(set(s) == TODAY_STEP for s in seen[1:])


@pytest.mark.parametrize("traffic", ["constant", "idm"])
def test_evaluate_agent_with_a_perception_model_on_the_cpu_environment(traffic):
    B, Q = 4, 2
    res, seen, env = _evaluate(B, Q, traffic, perception=dict(REAL))
    p = res.perception
    assert set(p) == set(evaluate.PERCEPTION_COUNTS)
    assert p["present"] == p["seen"] + p["out_of_range"] + p["occluded"] + p["dropped"] and p["seen"] > 0
    assert set(seen[0]) == {"reset", "ego", "obs", "seen", "row_class"}
    assert all(set(s) == TODAY_STEP | {"obs", "seen", "row_class"} for s in seen[1:])
    steps = [dict(obs=s["obs"], reset=bool(s.get("reset"))) for s in seen]
    kw = {k: v for k, v in REAL.items() if k != "occluders"}
    outs, counts, ctr = ph.replay(steps, B, rollout.VEHICLES_COUNT, REAL["occluders"], env_offset=getattr(env, "env_offset", 0), **kw)
    for s, (want_seen, want_cls) in zip(seen, outs):
        assert s["seen"].tobytes() == want_seen.tobytes() and np.array_equal(s["row_class"], want_cls)
    assert p == dict(zip(ph.COUNTS, counts.sum(axis=1).tolist())) and (ctr == res.steps + 1).all()
    s = res.summary()
    assert set(s) == TODAY_SUMMARY | {"seen_frac", "occluded_frac", "out_of_range_frac", "dropped_frac"}
    assert s["seen_frac"] == p["seen"] / p["present"]
    assert s["seen_frac"] + s["occluded_frac"] + s["out_of_range_frac"] + s["dropped_frac"] == pytest.approx(1.0)
    # the accounting reads the true scene: the records are those of the same steps' flags
    assert int(res.records["steps"].sum()) <= res.env_steps


def test_compare_gives_every_agent_the_same_fresh_perception():
    make_env = lambda: rollout.SyntheticIntersectionEnv(4, device="cpu", seed=3, n_others=4, backend="torch")
    agent = lambda: PureMPC_Agent(Env(), dict(CFG), engine=StubEngine(), collision_cost=True)
    out = evaluate.compare({"a": agent(), "b": agent()}, make_env, 1, perception=dict(REAL), use_graph=False)
    assert out["a"]["seen_frac"] == out["b"]["seen_frac"] < 1.0 and out["a"]["avg_steps"] == out["b"]["avg_steps"]
    inst = evaluate.Perception(4, "cpu", "torch", **REAL)
    out2 = evaluate.compare({"a": agent()}, make_env, 1, perception=inst, use_graph=False)
    assert out2["a"]["seen_frac"] == out["a"]["seen_frac"] and inst.totals()["present"] == 0     # a copy ran, not `inst`


def test_perception_refuses_invalid_arguments():
    for kw in (dict(R=0), dict(R=18), dict(min_points=0), dict(min_points=6), dict(p_drop=-0.1), dict(p_drop=1.5),
               dict(p_drop=float("nan")), dict(sigma_pos=-1.0), dict(sigma_vel=float("nan")), dict(sigma_head=-0.01),
               dict(range=0.0), dict(range=-5.0), dict(range=float("nan")), dict(occluders=np.zeros((9, 4, 2))),
               dict(occluders=np.zeros((2, 3, 2))), dict(occluders=np.full((1, 4, 2), np.nan)), dict(backend="cuda"),
               dict(seed=-1), dict(seed=2 ** 64)):
        args = dict(B=2, device="cpu", backend="torch")
        args.update(kw)
        with pytest.raises(ValueError):
            evaluate.Perception(**args)
    p = evaluate.Perception(2, "cpu", "torch", R=10)
    obs = torch.zeros(2, 10, 8)
    with pytest.raises(ValueError):
        p.apply(obs, obs)                                                      # in place
    with pytest.raises(ValueError):
        p.apply(torch.zeros(2, 9, 8), torch.zeros(2, 9, 8))
    with pytest.raises(ValueError):
        p.apply(obs.double(), torch.zeros(2, 10, 8))
    env = rollout.SyntheticIntersectionEnv(4, device="cpu", seed=3, n_others=4, backend="torch")
    agent = PureMPC_Agent(Env(), dict(CFG), engine=StubEngine(), collision_cost=True)
    with pytest.raises(ValueError):
        evaluate.evaluate_agent(agent, env, use_graph=False, perception=evaluate.Perception(3, "cpu", "torch"))


# ---- sanitizers: a stand-alone program, nothing loaded into Python -----------------------------------------------------------

def test_host_build_runs_clean_under_address_and_undefined_behaviour_sanitizers():
    out = os.path.join(conftest.ROOT, "tests", "_build", "perception_san_main")
    src = os.path.join(conftest.ROOT, "tests", "perception_san_main.cpp")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in [src] + ph.DEPS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                        "-static-libubsan", "-std=c++17", "-Wno-unknown-pragmas", "-ffp-contract=off", "-o", out, src],
                       check=True)
    res = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "perception_san_main: ok" in res.stdout, res.stdout + res.stderr
