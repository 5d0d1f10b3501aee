"""The tracker of the closed-loop evaluation on the CPU: the host build of csrc/mpc_tracker.hpp, the evaluator's CPU path and
a plain-Python restatement of the model (tests/tracker_host.py) against one another, bit for bit, on streams with the edge
cases forced; coasting, expiry and done against answers that need no implementation to state; the off setting as a
permutation of its input; evaluate_agent with a tracker on the torch environment, and unchanged without; the argument checks
and the signature table; a sanitizer run of the host build in a stand-alone program."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import conftest
import episode_stats_host as esh
import tracker_host as th
from mpc_rl_for_avs_amd import evaluate, rollout
from mpc_rl_for_avs_amd.pure_mpc import PureMPC_Agent
from test_evaluate_cpu import CFG, Env, StubEngine

T_STEPS, RESET_AT, DT = 40, 20, 0.1
SHAPES = [(1, 1), (3, 2), (5, 10), (4, 17)]                                              # B, R
# forced launches: no row; every row; a lone row far from everything, then two rows inside its gate; a lone row, then the same
# vehicle exactly 3 m on (d == gate2 for gate 3); every row, then every row 1000 m away
STEP_NONE, STEP_ALL, STEP_LONE, STEP_TWO, STEP_LONE2, STEP_EDGE, STEP_FULL, STEP_FAR = 3, 4, 11, 12, 14, 15, 30, 31
DONE_AT = (8, 26)                                        # launches on which the even environments are done
PARAMS = {"off": dict(), "coast": dict(coast=3), "gains": dict(alpha_pos=0.5, alpha_vel=0.3), "gate0": dict(gate=0.0),
          "gateinf": dict(gate=th.INF), "all": dict(coast=50, alpha_pos=0.5, alpha_vel=0.3)}


def _rows(present, x, y, vx, vy, h):
    full = np.stack([np.ones_like(x), x, y, vx, vy, h, np.sin(h), np.cos(h)], axis=-1)
    return np.where(present[..., None], full, 0.0).astype(np.float32)


def tracker_stream(B, R, seed, T=T_STEPS):
    """T launches: dicts with obs [B, R, 8] f32, reset, done [B] u8 or None.  Vehicles move at constant velocity with an
    occasional jump, rows are absent at random (in place: present rows are not contiguous), the first launch and launch
    RESET_AT reset, the even environments are done on the launches DONE_AT, and the forced launches above."""
    rng = np.random.default_rng(seed)
    pos, vel = rng.uniform(-40, 40, (B, R, 2)), rng.uniform(-10, 10, (B, R, 2))
    steps = []
    for k in range(T):
        jump = rng.random((B, R)) < 0.03
        pos = np.where(jump[..., None], rng.uniform(-40, 40, (B, R, 2)), pos + vel * DT)
        present = rng.random((B, R)) < 0.75
        h = rng.uniform(-math.pi, math.pi, (B, R))
        x, y, vx, vy = pos[..., 0].copy(), pos[..., 1].copy(), vel[..., 0].copy(), vel[..., 1].copy()
        if k == STEP_NONE:
            present[:] = False
        if k in (STEP_ALL, STEP_FULL, STEP_FAR):
            present[:] = True
        if k == STEP_FAR:
            x[:, 1:] += 1000.0
        if k in (STEP_LONE, STEP_TWO, STEP_LONE2, STEP_EDGE):
            present[:] = False
            present[:, 1:2] = True
            vx[:, 1:3], vy[:, 1:3] = {STEP_LONE: 1.0, STEP_TWO: 1.0}.get(k, 0.0), 0.0
            x[:, 1:2], y[:, 1:2] = {STEP_LONE: 500.0, STEP_TWO: 500.6, STEP_LONE2: 600.0, STEP_EDGE: 603.0}[k], 500.0
            if k == STEP_TWO and R > 2:                  # nearer to the track (predicted at 500.1), but the later row
                present[:, 2], x[:, 2], y[:, 2] = True, 499.8, 500.0
        present[:, 0] = True
        done = (np.arange(B) % 2 == 0).astype(np.uint8) if k in DONE_AT else (np.zeros(B, np.uint8) if k % 2 else None)
        steps.append(dict(obs=_rows(present, x, y, vx, vy, h), reset=k in (0, RESET_AT), done=done))
    return steps


def stream_of(B, R):
    return tracker_stream(B, R, seed=1000 * B + R)


def run_host(steps, B, R, params):
    h = th.HostTracker(B, R, **params)
    outs, per_launch = [], []
    for s in steps:
        out = h.apply(s["obs"], s["done"], s["reset"])
        outs.append((out, h.row_slot.copy(), h.row_miss.copy()))
        per_launch.append(h.counts.copy())
    return outs, h.track_f64.copy(), h.track_i32.copy(), h.counts.copy(), per_launch


def run_class(steps, B, R, params, device="cpu", backend="torch"):
    t = evaluate.Tracker(B, device, backend, R=R, **params)
    outs = []
    for s in steps:
        obs = torch.from_numpy(s["obs"]).to(t.device)
        done = None if s["done"] is None else torch.from_numpy(s["done"]).to(t.device)
        out = torch.full_like(obs, float("nan"))
        assert t.apply(obs, out, done=done, reset=s["reset"]) is out
        outs.append((out.cpu().numpy(), t.row_slot.cpu().numpy().copy(), t.row_miss.cpu().numpy().copy()))
    return outs, t.track_f64.cpu().numpy(), t.track_i32.cpu().numpy(), t.counts.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def assert_runs_equal(got, want, what):
    (g_outs, g_tf, g_ti, g_counts), (w_outs, w_tf, w_ti, w_counts) = got[:4], want[:4]
    assert len(g_outs) == len(w_outs)
    for k, ((go, gs, gm), (wo, ws, wm)) in enumerate(zip(g_outs, w_outs)):
        assert go.dtype == wo.dtype == np.float32 and go.shape == wo.shape, (what, k)
        if not np.array_equal(_bits(go), _bits(wo)):
            idx = np.argwhere(_bits(go) != _bits(wo))[:5]
            raise AssertionError(f"{what}: obs_out of launch {k} differs at {idx.tolist()}: "
                                 f"{[go[tuple(i)] for i in idx]} != {[wo[tuple(i)] for i in idx]}")
        assert gs.dtype == ws.dtype == np.uint8 and np.array_equal(gs, ws), (what, "row_slot", k)
        assert gm.dtype == wm.dtype == np.uint8 and np.array_equal(gm, wm), (what, "row_miss", k)
    assert g_tf.dtype == w_tf.dtype == np.float64 and np.array_equal(_bits(g_tf), _bits(w_tf)), (what, "track_f64")
    assert g_ti.dtype == w_ti.dtype == np.int32 and np.array_equal(g_ti, w_ti), (what, "track_i32")
    assert g_counts.dtype == w_counts.dtype == np.int64 and np.array_equal(g_counts, w_counts), (what, "counts")


# ---- 1: host build, torch backend and restatement ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(PARAMS))
@pytest.mark.parametrize("B,R", SHAPES)
def test_host_build_is_the_plain_python_restatement_bit_for_bit(B, R, name):
    params = PARAMS[name]
    steps = stream_of(B, R)
    got = run_host(steps, B, R, params)
    assert_runs_equal(got, th.replay(steps, B, R, **params), "host build vs restatement")
    outs, tf, ti, counts, per_launch = got
    q = dict(th.DEFAULTS, **params)
    # what a launch added to the counts (a reset launch starts them from 0)
    delta = [per_launch[k] - (0 if steps[k]["reset"] else per_launch[k - 1]) for k in range(T_STEPS)]
    n = lambda k, name: delta[k][th.COUNTS.index(name)]
    total = {c: sum(int(d[i].sum()) for d in delta) for i, c in enumerate(th.COUNTS)}
    # the forced cases occurred
    obs = lambda k: steps[k]["obs"]
    assert [s["reset"] for s in steps].count(True) == 2 and any(s["done"] is None for s in steps)
    assert all(steps[k]["done"].any() for k in DONE_AT)
    assert not obs(STEP_NONE)[:, 1:, 0].any() and (n(STEP_NONE, "measured") == 0).all()
    assert (obs(STEP_ALL)[:, :, 0] == 1).all() and (n(STEP_ALL, "measured") == R - 1).all()
    for k in range(T_STEPS):
        assert (n(k, "measured") == (obs(k)[:, 1:, 0] != 0).sum(axis=1)).all(), k
        assert (n(k, "measured") == n(k, "matched") + n(k, "born")).all(), k
    finite_gate = 0.0 < q["gate"] < th.INF
    if R >= 2 and q["gate"] == 3.0:
        assert (n(STEP_LONE2, "born") == 1).all() and (n(STEP_EDGE, "matched") == 1).all()      # d == gate2 associates
    if R >= 3 and finite_gate:
        # the nearer row (to the ego: the earlier one) wins the track of the lone row, the other is born
        assert (n(STEP_LONE, "born") == 1).all() and (n(STEP_TWO, "matched") == 1).all() and (n(STEP_TWO, "born") == 1).all()
        for b in range(B if q["coast"] == 0 and q["alpha_pos"] == 1.0 else 0):   # no older track crowds these out of the rows
            lone = int(outs[STEP_LONE][1][b][outs[STEP_LONE][0][b, :, 1] == 500.0][0])
            two = {float(np.float32(x)): int(s) for x, s in zip(outs[STEP_TWO][0][b, :, 1], outs[STEP_TWO][1][b])}
            assert two[float(np.float32(500.6))] == lone != two[float(np.float32(499.8))] != th.NO_SLOT
    if R == 17 and finite_gate:
        # sixteen tracks met by sixteen far measurements: expired and born anew without coasting, all evicted with it
        assert (n(STEP_FAR, "born") == 16).all() and (n(STEP_FAR, "matched") == 0).all()
        assert (n(STEP_FAR, "evicted") == (16 if q["coast"] > 0 else 0)).all()
        assert (n(STEP_FAR, "expired") == (0 if q["coast"] > 0 else 16)).all()
    if R == 17 and finite_gate and q["coast"] > 0:
        assert total["evicted"] > 0
    if R in (2, 10) and finite_gate and q["coast"] > 0:
        assert total["cut"] > 0 and (n(STEP_FAR, "cut") > 0).all()
    if R >= 2 and q["coast"] <= 3:
        assert total["expired"] > 0
    if R >= 2 and q["coast"] > 0:
        assert total["coasted"] > 0
    # the invariants of every output
    for k, (out, slot, miss) in enumerate(outs):
        assert not np.isnan(out).any(), k                                      # every element written
        there = out[:, :, 0] != 0
        assert not np.signbit(out[~there]).any() and not out[~there].any(), k  # a zero row is +0.0 in every column
        assert (np.diff(there[:, 1:].astype(np.int8), axis=1) <= 0).all(), k   # contiguous
        assert np.array_equal(_bits(out[:, 0]), _bits(obs(k)[:, 0])) and (slot[:, 0] == th.NO_SLOT).all()
        assert np.array_equal(slot[:, 1:] != th.NO_SLOT, there[:, 1:]) and not miss[~there].any() and not miss[:, 0].any()
        for b in range(B):
            used = slot[b][slot[b] != th.NO_SLOT]
            assert len(set(used.tolist())) == len(used) and (used < th.SLOTS).all()
        assert miss.max(initial=0) <= q["coast"]
    assert (ti[:, :, 2] <= q["coast"]).all() and set(np.unique(ti[:, :, 0]).tolist()) <= {0, 1}


@pytest.mark.parametrize("name", list(PARAMS))
@pytest.mark.parametrize("B,R", SHAPES)
def test_torch_backend_is_the_host_build_bit_for_bit(B, R, name):
    steps = stream_of(B, R)
    assert_runs_equal(run_class(steps, B, R, PARAMS[name]), run_host(steps, B, R, PARAMS[name]), "torch vs host build")


# ---- 2: answers stated without an implementation -----------------------------------------------------------------------------

X0, Y0, VX, VY = np.float32(12.5), np.float32(-3.25), np.float32(7.3), np.float32(-1.9)


def _vehicle_frames(hidden=(3, 4, 5), T=7):
    """An ego at rest and one vehicle at constant velocity (its measured position the f32 nearest to the exact one)"""
    frames = []
    for k in range(T):
        obs = np.zeros((1, 3, 8), np.float32)
        obs[0, 0] = [1, 0, 0, 0, 0, 0, 0, 1]
        if k not in hidden:
            obs[0, 1] = [1, float(X0) + k * DT * float(VX), float(Y0) + k * DT * float(VY), VX, VY, 0.25, math.sin(0.25),
                         math.cos(0.25)]
        frames.append(obs)
    return frames


def _step_host(frames, done_at=(), **params):
    h = th.HostTracker(1, 3, **params)
    for k, obs in enumerate(frames):
        out = h.apply(obs, np.array([k in done_at], np.uint8), reset=k == 0)
        yield out[0], h.row_slot[0].copy(), h.row_miss[0].copy(), h.track_i32[0].copy()


def _step_python(frames, done_at=(), **params):
    for k in range(len(frames)):
        steps = [dict(obs=o, reset=j == 0, done=[j in done_at]) for j, o in enumerate(frames[:k + 1])]
        outs, _, ti, _ = th.replay(steps, 1, 3, **params)
        yield outs[-1][0][0], outs[-1][1][0], outs[-1][2][0], ti[0]


def _step_torch(frames, done_at=(), **params):
    t = evaluate.Tracker(1, "cpu", "torch", R=3, **params)
    for k, obs in enumerate(frames):
        out = t.apply(torch.from_numpy(obs), torch.empty(1, 3, 8), done=torch.tensor([k in done_at]), reset=k == 0)
        yield out[0].numpy().copy(), t.row_slot[0].numpy().copy(), t.row_miss[0].numpy().copy(), t.track_i32[0].numpy().copy()


STEPPERS = [_step_host, _step_python, _step_torch]
IDS = ["host", "python", "torch"]


@pytest.mark.parametrize("stepper", STEPPERS, ids=IDS)
def test_a_hidden_vehicle_coasts_at_its_last_velocity_and_keeps_its_slot(stepper):
    frames = _vehicle_frames()
    got = list(stepper(frames, coast=3, gate=3.0))
    x, y = float(frames[2][0, 1, 1]), float(frames[2][0, 1, 2])                # the last measurement, widened exactly
    slot2 = int(got[2][1][1])
    assert slot2 == 0 and [int(g[3][slot2, 1]) for g in got[:3]] == [1, 2, 3]  # born in the lowest slot; age 1, 2, 3
    for k in (3, 4, 5):
        x = x + float(VX) * DT                                                 # repeated sums in f64 ...
        y = y + float(VY) * DT
        out, slot, miss, ti = got[k]
        want = np.array([1.0, x, y, VX, VY, 0.25, math.sin(0.25), math.cos(0.25)]).astype(np.float32)      # ... narrowed once
        assert out[1].tobytes() == want.tobytes(), k
        assert int(miss[1]) == k - 2 and int(slot[1]) == slot2 and not out[2].any()
        assert ti[slot2].tolist() == [1, 3, k - 2]
    out, slot, miss, ti = got[6]
    assert out[1].tobytes() == frames[6][0, 1].tobytes()                       # gains 1: the measurement itself
    assert int(slot[1]) == slot2 and int(miss[1]) == 0 and ti[slot2].tolist() == [1, 4, 0]


@pytest.mark.parametrize("stepper", STEPPERS, ids=IDS)
def test_a_vehicle_hidden_for_longer_than_coast_is_born_anew(stepper):
    got = list(stepper(_vehicle_frames(), coast=2, gate=3.0))
    assert got[3][0][1, 0] == 1 and got[4][0][1, 0] == 1 and [int(g[2][1]) for g in got[3:5]] == [1, 2]
    out, slot, miss, ti = got[5]
    assert not out[1:].any() and (slot == th.NO_SLOT).all() and not ti.any()   # gone, the slots all free
    out, slot, miss, ti = got[6]
    assert int(slot[1]) == 0 and ti[0].tolist() == [1, 1, 0] and int(miss[1]) == 0     # a birth in the lowest free slot


@pytest.mark.parametrize("stepper", STEPPERS, ids=IDS)
def test_done_drops_the_tracks_before_the_frame_is_read(stepper):
    got = list(stepper(_vehicle_frames(), done_at=(4,), coast=3, gate=3.0))
    assert got[3][0][1, 0] == 1 and int(got[3][2][1]) == 1
    out, slot, miss, ti = got[4]
    assert not out[1:].any() and (slot == th.NO_SLOT).all() and not ti.any()
    assert not got[5][0][1:].any()
    assert got[6][3][0].tolist() == [1, 1, 0]
    # a vehicle that is measured on the frame of the done starts a new track with age 1
    seen = list(stepper(_vehicle_frames(hidden=()), done_at=(4,), coast=3, gate=3.0))
    assert [int(g[3][0, 1]) for g in seen] == [1, 2, 3, 4, 1, 2, 3]


# ---- 3: off is a permutation ---------------------------------------------------------------------------------------------------

def _keys(frame):
    """key of every row >= 1 of frame [B, R, 8] f32, formed here: f64 on the widened values, a product each, then the sum"""
    t = frame.astype(np.float64)
    kx, ky = t[:, 1:, 1] - t[:, :1, 1], t[:, 1:, 2] - t[:, :1, 2]
    a, c = kx * kx, ky * ky
    return a + c


def assert_off_is_a_permutation(meas, out):
    """every frame: the present output rows are the present input rows bit for bit, ordered by key (ties by input order are
    not checked: equal keys of different rows do not occur here) -> frames on which the output IS the input exactly"""
    exact = 0
    for b in range(meas.shape[0]):
        rows = meas[b, 1:][meas[b, 1:, 0] != 0]
        key = _keys(meas[b:b + 1])[0][meas[b, 1:, 0] != 0]
        order = np.argsort(key, kind="stable")
        want = np.zeros_like(meas[b])
        want[0], want[1:1 + len(rows)] = meas[b, 0], rows[order]
        assert out[b].tobytes() == want.tobytes(), b
        contiguous = (np.diff((meas[b, 1:, 0] != 0).astype(np.int8)) <= 0).all()
        increasing = (np.diff(key) > 0).all()
        if contiguous and increasing and not np.signbit(meas[b][meas[b, :, 0] == 0]).any():
            assert out[b].tobytes() == meas[b].tobytes(), b
            exact += 1
    return exact


@pytest.mark.parametrize("run", [run_host, run_class], ids=["host", "torch"])
@pytest.mark.parametrize("B,R", SHAPES)
def test_off_is_a_permutation_of_the_stream(B, R, run):
    steps = stream_of(B, R)
    outs = run(steps, B, R, dict(coast=0, alpha_pos=1.0, alpha_vel=1.0, gate=3.0))[0]
    for s, (out, slot, miss) in zip(steps, outs):
        assert (s["obs"][:, 1:, 0][s["obs"][:, 1:, 0] != 0] == 1).all()
        assert_off_is_a_permutation(s["obs"], out)
        assert not miss.any()


@pytest.mark.parametrize("traffic", ["constant", "idm"])
def test_off_is_the_identity_on_the_environments_own_observations(traffic):
    B, T = 64, 200
    env = rollout.SyntheticIntersectionEnv(B, device="cpu", seed=5, n_others=4, backend="torch", traffic=traffic)
    t = evaluate.Tracker(B, "cpu", "torch", dt=float(env.dt))
    obs = env.reset()
    out = torch.empty_like(obs)
    t.apply(obs, out, reset=True)
    frames, exact = B, assert_off_is_a_permutation(obs.numpy(), out.numpy())
    act = torch.zeros(B, 2, dtype=torch.float64)
    for k in range(T):
        act[:, 0] = 1.0 if k % 20 < 10 else -0.5
        obs, _, done, _ = env.step(act)
        t.apply(obs, out, done=done)
        exact += assert_off_is_a_permutation(obs.numpy(), out.numpy())
        frames += B
    print(f"off tracker, traffic={traffic}: {frames - exact} of {frames} frames without strictly increasing keys")
    assert frames - exact <= frames // 100
    assert t.totals()["matched"] > 0 and t.totals()["coasted"] == t.totals()["cut"] == t.totals()["evicted"] == 0


# ---- 4: the evaluator ----------------------------------------------------------------------------------------------------------

TODAY_STEP = {"ego", "done", "truncated", "crashed", "arrived", "reward", "status", "iters"}
DROP = dict(p_drop=0.3, seed=11)


def _evaluate(B, Q, traffic="constant", **kw):
    env = rollout.SyntheticIntersectionEnv(B, device="cpu", seed=3, n_others=4, backend="torch", traffic=traffic)
    agent = PureMPC_Agent(Env(), dict(CFG), engine=StubEngine(), collision_cost=True)
    seen = []
    take = lambda d: {k: (v.clone().numpy() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
    res = evaluate.evaluate_agent(agent, env, episodes_per_env=Q, use_graph=False, poll_every=5,
                                  on_step=lambda d: seen.append(take(d)), **kw)
    return res, seen, env


def _same(a, b):
    assert (a is None) == (b is None)
    if a is not None:
        assert set(a) == set(b)
        for k in a:
            x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), k


@pytest.mark.parametrize("traffic", ["constant", "idm"])
def test_evaluate_agent_with_tracker_none_is_evaluate_agent_without(traffic):
    kw = dict(metrics=True, perception=dict(DROP), interaction=traffic == "idm", trace=dict(keep="all", capacity=8, window=20))
    base, seen0, _ = _evaluate(6, 1, traffic, **kw)
    none, seen1, _ = _evaluate(6, 1, traffic, tracker=None, **kw)
    _same(base.records, none.records)
    _same(base.drive, none.drive)
    _same(base.interaction, none.interaction)
    assert base.perception == none.perception and base.steps == none.steps and base.tracker is None and none.tracker is None
    strip = lambda d: {k: v for k, v in d.items() if k not in ("seconds", "env_steps_per_s")}
    assert strip(base.summary()) == strip(none.summary()) and "coasted_frac" not in none.summary()
    a, b = base.traces, none.traces
    assert a.counts == b.counts and a.seen.tobytes() == b.seen.tobytes() and a.scene.tobytes() == b.scene.tobytes()
    _same(a.index, b.index)
    assert [set(s) for s in seen0] == [set(s) for s in seen1]
    for s0, s1 in zip(seen0, seen1):
        for k in s0:
            assert np.array_equal(s0[k], s1[k]), k


@pytest.mark.parametrize("traffic", ["constant", "idm"])
def test_evaluate_agent_with_a_perception_model_and_a_tracker(traffic):
    B, Q, R = 4, 2, rollout.VEHICLES_COUNT
    settings = dict(coast=5)
    trace = dict(keep="all", capacity=B * Q, window=rollout.EPISODE_STEPS)
    res, seen, env = _evaluate(B, Q, traffic, perception=dict(DROP), tracker=dict(settings), trace=trace)
    assert set(seen[0]) == {"reset", "ego", "obs", "seen", "row_class", "row_slot", "row_miss"}
    assert all(set(s) == TODAY_STEP | {"obs", "seen", "row_class", "row_slot", "row_miss"} for s in seen[1:])
    # what the perception model gave on every frame: its own replay of the true observations
    import perception_host as ph
    p_outs, _, _ = ph.replay([dict(obs=s["obs"], reset=bool(s.get("reset"))) for s in seen], B, R,
                             env_offset=int(getattr(env, "env_offset", 0)), **DROP)
    steps = [dict(obs=p[0], reset=bool(s.get("reset")), done=None if s.get("reset") else s["done"])
             for s, p in zip(seen, p_outs)]
    outs, _, _, counts = th.replay(steps, B, R, dt=float(env.dt), **settings)
    before = np.zeros((7, B), np.int64)
    for k, (s, (want, slot, miss)) in enumerate(zip(seen, outs)):
        assert s["seen"].tobytes() == want.tobytes(), k
        assert np.array_equal(s["row_slot"], slot) and np.array_equal(s["row_miss"], miss), k
    # coasting only adds rows: at least as many present rows as the perception output where nothing was evicted or cut
    host = th.HostTracker(B, R, dt=float(env.dt), **settings)
    checked = 0
    for k, s in enumerate(steps):
        host.apply(s["obs"], s["done"], s["reset"])
        now = host.counts.copy()
        lost = (now - before)[th.COUNTS.index("evicted")] + (now - before)[th.COUNTS.index("cut")]
        before = now
        rows_in, rows_out = (s["obs"][:, 1:, 0] != 0).sum(axis=1), (seen[k]["seen"][:, 1:, 0] != 0).sum(axis=1)
        assert (rows_out[lost == 0] >= rows_in[lost == 0]).all(), k
        checked += int((lost == 0).sum())
    assert checked > 0 and np.array_equal(host.counts, counts)
    assert res.tracker == dict(zip(th.COUNTS, counts.sum(axis=1).tolist())) and set(res.tracker) == set(evaluate.TRACKER_COUNTS)
    t = res.tracker
    assert t["coasted"] > 0 and t["measured"] == t["matched"] + t["born"] == res.perception["seen"]
    assert res.summary()["coasted_frac"] == t["coasted"] / (t["matched"] + t["born"] + t["coasted"])
    # the accounting is unaffected: the records are the replay of the true scene's flags
    want = esh.replay(seen, B, Q)
    assert set(res.records) == set(want)
    for k in want:
        assert np.array_equal(res.records[k], want[k]), k
    # the trace recorder's `seen` plane is the tracker's outputs: frame t of an episode is what the agent acted on at step t
    tr = res.traces
    assert tr.seen is not None and len(tr) == B * Q
    start = np.zeros(B, np.int64)                        # the on_step index of the frame each environment's episode began on
    checked = 0
    for k in range(1, len(seen)):
        for b in np.nonzero(seen[k]["done"])[0]:
            i = [j for j in range(len(tr)) if tr.index["env"][j] == b and tr.index["launch"][j] == k]
            if i:
                e = tr.episode(i[0])
                assert e["steps"] == k - start[b]
                assert e["seen"].tobytes() == np.stack([seen[j]["seen"][b] for j in range(start[b], k)]).tobytes()
                checked += 1
            start[b] = k
    assert checked == B * Q


def test_evaluate_agent_with_a_tracker_alone_reads_the_true_observation():
    res, seen, env = _evaluate(4, 1, tracker=dict(coast=0))
    assert res.perception is None and res.tracker["coasted"] == 0 and res.summary()["coasted_frac"] == 0.0
    assert all("row_class" not in s and "row_slot" in s for s in seen)
    for s in seen:
        assert_off_is_a_permutation(s["obs"], s["seen"])
    given = evaluate.Tracker(4, "cpu", "torch", dt=float(env.dt), coast=2)               # an instance instead of a dict
    again, _, _ = _evaluate(4, 1, tracker=given)
    assert again.tracker == given.totals() and again.tracker["measured"] == res.tracker["measured"]


def test_compare_gives_every_agent_a_fresh_tracker():
    make_env = lambda: rollout.SyntheticIntersectionEnv(4, device="cpu", seed=3, n_others=4, backend="torch")
    agent = lambda: PureMPC_Agent(Env(), dict(CFG), engine=StubEngine(), collision_cost=True)
    results = {}
    out = evaluate.compare({"a": agent(), "b": agent()}, make_env, 1, perception=dict(DROP), tracker=dict(coast=5),
                           results=results, use_graph=False)
    assert out["a"]["coasted_frac"] == out["b"]["coasted_frac"] > 0 and results["a"].tracker == results["b"].tracker
    inst = evaluate.Tracker(4, "cpu", "torch", coast=5)
    out2 = evaluate.compare({"a": agent()}, make_env, 1, perception=dict(DROP), tracker=inst, use_graph=False)
    assert out2["a"]["coasted_frac"] == out["a"]["coasted_frac"] and inst.totals()["measured"] == 0      # a copy ran
    plain = evaluate.compare({"a": agent()}, make_env, 1, perception=dict(DROP), use_graph=False)
    assert "coasted_frac" not in plain["a"]


# ---- 5: argument checks --------------------------------------------------------------------------------------------------------

def test_tracker_refuses_invalid_arguments():
    nan = float("nan")
    for kw in (dict(R=0), dict(R=18), dict(B=-1), dict(dt=0.0), dict(dt=-0.1), dict(dt=nan), dict(gate=-1.0), dict(gate=nan),
               dict(coast=-1), dict(coast=201), dict(coast=1.5), dict(alpha_pos=0.0), dict(alpha_pos=1.5), dict(alpha_pos=nan),
               dict(alpha_vel=0.0), dict(alpha_vel=-0.5), dict(alpha_vel=nan), dict(backend="cuda")):
        args = dict(B=2, device="cpu", backend="torch")
        args.update(kw)
        with pytest.raises(ValueError):
            evaluate.Tracker(**args)
    evaluate.Tracker(2, "cpu", gate=th.INF, coast=200, alpha_pos=1e-3)
    t = evaluate.Tracker(2, "cpu", "torch", R=10)
    obs, out = torch.zeros(2, 10, 8), torch.zeros(2, 10, 8)
    for bad in (dict(obs_meas=obs, out=obs), dict(obs_meas=torch.zeros(2, 9, 8), out=torch.zeros(2, 9, 8)),
                dict(obs_meas=obs.double(), out=out), dict(obs_meas=obs, out=out.double()),
                dict(obs_meas=obs.transpose(0, 1).contiguous().transpose(0, 1), out=out),
                dict(obs_meas=obs, out=out, done=torch.zeros(3, dtype=torch.uint8)),
                dict(obs_meas=obs, out=out, done=torch.zeros(2, dtype=torch.int32)),
                dict(obs_meas=obs.to("meta"), out=out)):
        with pytest.raises(ValueError):
            t.apply(**bad)
    assert not t.counts.any()                            # nothing ran
    env = rollout.SyntheticIntersectionEnv(4, device="cpu", seed=3, n_others=4, backend="torch")
    agent = PureMPC_Agent(Env(), dict(CFG), engine=StubEngine(), collision_cost=True)
    with pytest.raises(ValueError, match="tracker"):
        evaluate.evaluate_agent(agent, env, use_graph=False, tracker=evaluate.Tracker(3, "cpu", "torch"))
    with pytest.raises(ValueError):
        evaluate.evaluate_agent(agent, env, use_graph=False, tracker=dict(coast=-1))


def test_host_build_refuses_invalid_arguments():
    obs = np.zeros((2, 10, 8), np.float32)
    for kw in (dict(dt=0.0), dict(gate=-1.0), dict(gate=float("nan")), dict(coast=-1), dict(coast=201), dict(alpha_pos=0.0),
               dict(alpha_vel=1.5)):
        assert th.HostTracker(2, 10, **kw).step(obs, reset=True)[0] == -1, kw
    assert th.HostTracker(2, 10).step(obs, reset=True, planes=False)[0] == 0


def test_tracker_signature_table_is_the_header():
    """engine.TRACKER_SIGNATURES against the prototype, the way tests/test_abi.py holds engine.SIGNATURES"""
    import ctypes
    from mpc_rl_for_avs_amd import engine
    from test_abi import _prototype
    assert sorted(engine.TRACKER_SIGNATURES) == ["mpc_track_rows"]
    assert not set(engine.TRACKER_SIGNATURES) & (set(engine.SIGNATURES) | set(engine.EVALUATION_SIGNATURES))
    i, d, vp = ctypes.c_int32, ctypes.c_double, ctypes.c_void_p
    argtypes = dict(mpc_track_rows=[i, i, i, i, d, d, i, d, d] + [vp] * 8 + [vp])
    lib = engine.load_library()
    for name, sig in engine.TRACKER_SIGNATURES.items():
        assert list(sig) == _prototype(name), name
        assert len({n for n, _ in sig}) == len(sig), name
        assert list(getattr(lib, name).argtypes) == argtypes[name] and getattr(lib, name).restype is ctypes.c_int, name
        assert name in engine._EXPORTS and callable(engine.caller(name))
    assert engine.ABI_VERSION == 8
    with pytest.raises(TypeError, match="mpc_track_rows"):
        engine.call("mpc_track_rows", device=0)


# ---- 6: sanitizers: a stand-alone program, nothing loaded into Python ----------------------------------------------------------

def test_host_build_runs_clean_under_address_and_undefined_behaviour_sanitizers():
    out = os.path.join(conftest.ROOT, "tests", "_build", "tracker_san_main")
    src = os.path.join(conftest.ROOT, "tests", "tracker_san_main.cpp")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in [src] + th.DEPS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                        "-static-libubsan", "-std=c++17", "-Wno-unknown-pragmas", "-ffp-contract=off", "-o", out, src],
                       check=True)
    res = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "tracker_san_main: ok" in res.stdout, res.stdout + res.stderr
