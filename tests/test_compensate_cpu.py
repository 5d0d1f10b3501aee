"""The delay compensation of the closed-loop evaluation on the CPU: the host build of csrc/mpc_compensate.hpp, the evaluator's CPU
path and a plain-Python restatement of the update (tests/compensate_host.py) against one another on scene streams with the
edge cases forced; the prediction against a plant that is driven through the actuator model's host build; the identity at
steps = 0; re-ordering, absent rows and ties; non-finite commands; the argument checks and the signature table; evaluate_agent
with a compensator on the torch environment, and unchanged without; a sanitizer run of the host build in a stand-alone program.

THE YARDSTICK (shared with tests/test_compensate_gpu.py, `assert_runs_agree`).  Everything computed with + - * and comparisons
alone is compared bit for bit: the command ring, prev, age, counts, every row of the others, their order.  The ego's rollout
goes through sqrt, sin, cos, tan and atan, whose last f64 bits differ between libraries: pred and pring to atol 1e-9 (the bar
of tests/test_traffic_env_gpu.py for the ego state), the ego's output row to one f32 ulp of the expected value (an f64
difference of 1e-12 moves an f32 rounding by at most one place), sums to rtol 1e-9."""
import ctypes
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import actuator_host as ah
import compensate_host as ch
import conftest
from mpc_rl_for_avs_amd import evaluate, rollout

F32, INF, DT = np.float32, ch.INF, 0.1
T_LAUNCHES, RESET_AT, DONE_AT, STEP_NAN, STEP_INF = 12, 2, 3, 7, 9
KEY_GAP = 1e-3                                               # m^2 between any two present rows' keys of a random scene
# evaluate.Compensation's keywords: the nominal actuator off, and with lag, rate limit and limits on
PARAMS = {"off": dict(), "on": dict(tau=(0.1, 0.3), rate=(20.0, 2.0), limits="env")}


def entry_params(kw):
    """Compensation's keywords -> the entry point's parameters (compensate_host.DEFAULTS): alpha = dt / (tau + dt), lo and hi"""
    q = dict(kw)
    dt = q.get("dt", DT)
    tau = q.pop("tau", (0.0, 0.0))
    limits = q.pop("limits", None)
    if limits is None:
        limits = ((-INF, INF), (-INF, INF))
    elif limits == "env":                                                    # the environment's clamp, mpc_synth_env.hpp
        limits = ((-5.0, 5.0), (-math.pi / 4, math.pi / 4))
    return dict(q, alpha=tuple(dt / (t + dt) for t in tau), lo=(limits[0][0], limits[1][0]), hi=(limits[0][1], limits[1][1]))


def ego_row(x, y, th, sp):
    """env::observe's row 0, [..., 8] f32"""
    s, c = np.sin(th), np.cos(th)
    return np.stack([np.ones_like(x), x, y, sp * c, sp * s, th, s, c], axis=-1).astype(F32)


def _keys(rows, h, ex, ey):
    """step 6 and 7 of the header for the rows [n, 8] of one environment about the ego's written (ex, ey) f32"""
    nx = (rows[:, 1].astype(np.float64) + rows[:, 3].astype(np.float64) * h).astype(F32)
    ny = (rows[:, 2].astype(np.float64) + rows[:, 4].astype(np.float64) * h).astype(F32)
    kx, ky = nx.astype(np.float64) - float(ex), ny.astype(np.float64) - float(ey)
    return kx * kx + ky * ky


@functools.lru_cache(maxsize=None)
def scene_stream(B, R, steps, name):
    """T_LAUNCHES launches for Compensation(steps=steps, **PARAMS[name]): dicts with obs [B, R, 8] f32, command [B, 2] f64 and
    done [B] u8 or None; launches 0 and RESET_AT are reset launches (obs alone); environment b's episode ends on launch
    DONE_AT + b % 3, so up to 8 commands follow and every look-ahead is scored.  Scenes are unrelated from launch to launch
    (the update does not ask for more).  The ego stays within +-8 m and 30 m/s, so its prediction stays below 32 m, where an
    f32 ulp is 1.9e-6 m; the others stay within +-15 m and 5 m/s, so a key's arguments stay below 48 m and an ulp of the
    ego's written position moves a key by at most 2 * 2 * 48 * 1.9e-6 = 3.7e-4 m^2: with KEY_GAP between any two present
    keys (asserted here, about the host build's prediction) a library's last bit cannot change the order.  Environment 0's
    ego is at the plant's speed limits on alternate launches; commands reach beyond the environment's clamp; one is NaN and
    one infinite; absent rows hold garbage behind their zero presence, and lie between present ones."""
    kw = dict(PARAMS[name], steps=steps)
    rng = np.random.default_rng(10000 * B + 100 * R + 10 * steps + len(name))
    host = ch.HostCompensator(B, R, **entry_params(kw))
    h = float(steps) * DT
    launches = []
    for k in range(T_LAUNCHES):
        reset = k in (0, RESET_AT)
        th, sp = rng.uniform(-math.pi, math.pi, B), rng.uniform(0.0, 12.0, B)
        sp[0] = (29.5, 0.2, 11.0)[k % 3]
        obs = np.zeros((B, R, 8), F32)
        obs[:, 0] = ego_row(rng.uniform(-8.0, 8.0, B), rng.uniform(-8.0, 8.0, B), th, sp)
        cmd = done = None
        if not reset:
            cmd = np.stack([rng.uniform(-8.0, 8.0, B), rng.uniform(-1.2, 1.2, B)], axis=1)
            if k == STEP_NAN:
                cmd[B - 1, 0] = np.nan
            if k == STEP_INF:
                cmd[B - 1, 1] = -np.inf
            if k % 4 != 2:                                   # environment b's episode ends on launch DONE_AT + b % 3
                done = (k == DONE_AT + np.arange(B) % 3).astype(np.uint8)
        _, pred = host.apply(obs, cmd, done, reset)          # the others do not enter the ego's prediction
        ex, ey = (F32(pred[:, 0]), F32(pred[:, 1])) if steps > 0 else (obs[:, 0, 1], obs[:, 0, 2])
        for b in range(B):
            for _ in range(200):
                n = R - 1
                v = rng.uniform(-5.0, 5.0, (n, 2))
                hd = np.arctan2(v[:, 1], v[:, 0])
                rows = np.stack([(rng.random(n) < 0.7).astype(np.float64), rng.uniform(-15.0, 15.0, n), rng.uniform(-15.0, 15.0, n),
                                 v[:, 0], v[:, 1], hd, np.sin(hd), np.cos(hd)], axis=1).astype(F32)
                key = np.sort(_keys(rows[rows[:, 0] != 0], h, ex[b], ey[b]))
                if key.size < 2 or np.diff(key).min() > KEY_GAP:
                    break
            else:
                raise AssertionError("no scene with separated keys")
            obs[b, 1:] = rows
        assert np.isfinite(obs).all()
        launches.append(dict(obs=obs, reset=True) if reset else dict(obs=obs, command=cmd, done=done))
    return launches


def run_host(launches, B, R, kw, pred=True):
    h = ch.HostCompensator(B, R, **entry_params(kw))
    outs, preds = [], []
    for s in launches:
        rc, out, p = h.step(s["obs"], s.get("command"), s.get("done"), bool(s.get("reset")), pred=pred)
        assert rc == 0
        outs.append(out)
        preds.append(p)
    return outs, preds, h.ring.copy(), h.prev.copy(), h.age.copy(), h.pring.copy(), h.counts.copy(), h.sums.copy()


def run_class(launches, B, R, kw, device="cpu", backend="torch", pred=True):
    a = evaluate.Compensation(B, device, backend, R=R, **dict(dict(dt=DT), **kw))
    if not pred:
        a.pred = None
    outs, preds = [], []
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(a.device)
    for s in launches:
        obs = t(s["obs"])
        out = torch.full_like(obs, float("nan"))
        if s.get("reset"):
            assert a.apply(obs, out, reset=True) is out
        else:
            assert a.apply(obs, out, command=t(s["command"]), done=t(s["done"])) is out
        outs.append(out.cpu().numpy().copy())
        preds.append(None if a.pred is None else a.pred.cpu().numpy().copy())
    n = lambda x: x.cpu().numpy().copy()
    return outs, preds, n(a.ring), n(a.prev), n(a.age), n(a.pring), n(a.counts), n(a.sums)


def run_python(launches, B, R, kw, pred=True):
    return ch.replay(launches, B, R, **entry_params(kw))


RUNNERS = dict(host=run_host, python=run_python, torch=run_class)
KINDS = list(RUNNERS)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same_bits(g, w, what):
    assert g.dtype == w.dtype and g.shape == w.shape, what
    if not np.array_equal(_bits(g), _bits(w)):
        idx = np.argwhere(_bits(g) != _bits(w))[:5]
        raise AssertionError(f"{what} differs at {idx.tolist()}: {[g[tuple(i)] for i in idx]} != {[w[tuple(i)] for i in idx]}")


def assert_runs_agree(got, want, what, steps):
    """the yardstick of this module's docstring; with steps == 0 the ego's row is a copy, so it is compared bit for bit too"""
    assert len(got[0]) == len(want[0])
    for k, (g, w) in enumerate(zip(got[0], want[0])):
        assert not np.isnan(g).any(), (what, k, "an element of out was not written")
        _same_bits(g[:, 1:], w[:, 1:], f"{what}: the others' rows of launch {k}")
        if steps == 0:
            _same_bits(g[:, 0], w[:, 0], f"{what}: the ego's row of launch {k}")
        else:
            off = np.abs(g[:, 0].astype(np.float64) - w[:, 0].astype(np.float64))
            assert (off <= np.spacing(np.abs(w[:, 0])).astype(np.float64)).all(), (what, k, g[:, 0], w[:, 0])
    for k, (g, w) in enumerate(zip(got[1], want[1])):
        if g is not None and w is not None:
            assert g.dtype == w.dtype == np.float64 and g.shape == w.shape
            assert np.allclose(g, w, rtol=0.0, atol=1e-9), (what, "pred", k, np.abs(g - w).max())
    names = ("ring", "prev", "age", "pring", "counts", "sums")
    for name, g, w in zip(names, got[2:], want[2:]):
        if name == "pring":
            assert g.shape == w.shape and np.allclose(g, w, rtol=0.0, atol=1e-9), (what, name, np.abs(g - w).max())
        elif name == "sums":
            assert g.shape == w.shape and np.allclose(g, w, rtol=1e-9, atol=0.0), (what, name, g, w)
        else:
            _same_bits(g, w, f"{what}: {name}")


# ---- 1: host build, restatement and torch backend ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(PARAMS))
@pytest.mark.parametrize("steps", [0, 1, 3, 7])
@pytest.mark.parametrize("R", [1, 10, 17])
@pytest.mark.parametrize("B", [1, 5])
def test_host_build_restatement_and_torch_backend_agree(B, R, steps, name):
    kw = dict(PARAMS[name], steps=steps)
    launches = scene_stream(B, R, steps, name)
    host = run_host(launches, B, R, kw)
    assert_runs_agree(host, run_python(launches, B, R, kw), "host build vs restatement", steps)
    assert_runs_agree(run_class(launches, B, R, kw), host, "torch vs host build", steps)
    assert_runs_agree(run_host(launches, B, R, kw, pred=False), host, "host build without pred", steps)
    outs, preds, ring, prev, age, pring, counts, sums = host
    pushed = T_LAUNCHES - 1 - DONE_AT - np.arange(B) % 3     # the commands since each environment's episode end
    assert age.tolist() == pushed.tolist() and all(np.isfinite(p).all() for p in preds)
    if steps == 0:
        assert not counts.any() and not sums.any()
        assert all(o.tobytes() == s["obs"].tobytes() for o, s in zip(outs, launches))
    else:
        # since the reset launch: one prediction scored per launch from age == steps on, in both episodes
        first = DONE_AT + np.arange(B) % 3 - RESET_AT - 1    # the first episode's commands
        want = np.maximum(first - steps + 1, 0) + np.maximum(pushed - steps + 1, 0)
        assert counts.tolist() == want.tolist() and ((counts > 0) == (sums[1] > 0)).all() and counts.any()
        for o, s in zip(outs, launches):                     # present rows first, the rest zero, nothing lost
            present = o[:, 1:, 0] != 0
            assert (present.sum(axis=1) == (s["obs"][:, 1:, 0] != 0).sum(axis=1)).all()
            assert (np.diff(present.astype(int), axis=1) <= 0).all() and not o[:, 1:][~present].any()
    if name == "on":                                         # the nominal limits hold for prev
        assert (np.abs(prev[:, 0]) <= 5.0).all() and (np.abs(prev[:, 1]) <= math.pi / 4).all()


def test_the_scene_streams_force_the_edge_cases():
    launches = scene_stream(5, 10, 3, "on")
    assert [bool(s.get("reset")) for s in launches] == [k in (0, RESET_AT) for k in range(T_LAUNCHES)]
    assert np.isnan(launches[STEP_NAN]["command"][4, 0]) and np.isinf(launches[STEP_INF]["command"][4, 1])
    assert [s["done"].tolist() for s in launches[DONE_AT:DONE_AT + 3]] == [[1, 0, 0, 1, 0], [0, 1, 0, 0, 1], [0, 0, 1, 0, 0]]
    assert any(s.get("done") is None for s in launches if not s.get("reset"))
    holes = [np.diff((s["obs"][:, 1:, 0] != 0).astype(int), axis=1).max() > 0 for s in launches]
    assert any(holes)                                        # an absent row in front of a present one
    garbage = [s["obs"][:, 1:][s["obs"][:, 1:, 0] == 0].any() for s in launches]
    assert any(garbage)


# ---- 2: the prediction is the future ---------------------------------------------------------------------------------------------

def _observe(state):
    return ego_row(*[np.array([v]) for v in state]).reshape(1, 1, 8)


def _seen_state(obs):
    """the state a compensator reads from row 0: x, y, heading widened, speed = |v|"""
    r = obs[0, 0].astype(np.float64)
    return np.array([r[1], r[2], r[5], math.sqrt(r[3] * r[3] + r[4] * r[4])])


@pytest.mark.parametrize("shaped", [False, True], ids=["delay", "delay_lag_rate_limits"])
@pytest.mark.parametrize("d", [1, 3, 7])
def test_the_prediction_is_the_plant_d_steps_on(d, shaped):
    """A plant (the host build's step_ego) driven through the actuator model's host build with delay d by scripted commands - a
    square wave of +-3 m/s^2 with period 4 and a steering ramp - with an episode end midway.  pred of launch L is the plant's
    state at L + d: to 1e-9 when the plant is rolled on from the state the compensator was shown (the f32 observation,
    widened) through the actions the actuator really applied on steps L .. L + d - 1, which depend on commands the compensator
    already holds; and to 2e-5 m against the true plant, whose state the observation rounds to f32 (half an ulp of a position
    below 64 m is 1.9e-6 m per axis, of a heading below 2 rad 6e-8 rad over at most 0.7 s * 15 m/s, of the velocity 6e-8
    relative: together under 5e-6 m).  After the episode end the first d applied actions of the new episode are zero - the
    actuator applies nothing of the old episode, and the compensator predicts just that."""
    T, END = 30, 13
    model = dict(alpha=(0.5, 1.0 / 3.0), rate=(20.0, 1.5), lo=(-2.5, -0.3), hi=(2.5, 0.3)) if shaped else dict()
    act = ah.HostActuator(1, delay=d, dt=DT, **model)
    comp = ch.HostCompensator(1, 1, steps=d, dt=DT, **model)
    script = lambda t: np.array([[3.0 if (t // 2) % 2 == 0 else -3.0, -0.4 + 0.05 * t]])
    starts = (np.array([2.0, 45.0, -math.pi / 2, 10.0]), np.array([-30.0, -2.0, 0.1, 6.0]))
    state = starts[0]
    obs = _observe(state)
    _, pred = comp.apply(obs, reset=True)
    preds, seen, true, applied, first = [pred[0].copy()], [_seen_state(obs)], [state.copy()], [], [0]
    ended = 0
    for t in range(T):
        cmd = script(t)
        a = act.apply(cmd, np.array([ended], np.uint8))
        applied.append(a[0].copy())
        state = ch.step_ego(state, a[0], DT)
        ended = int(t == END)
        if ended:
            state = starts[1]
        obs = _observe(state)
        _, pred = comp.apply(obs, cmd.copy(), np.array([ended], np.uint8))
        preds.append(pred[0].copy()), seen.append(_seen_state(obs)), true.append(state.copy())
        first.append(t + 1 if ended else first[-1])           # the launch on which the current episode began
    assert any(np.abs(a).max() > 0 for a in applied) and (not shaped or np.abs(np.array(applied)[:, 0]).max() <= 2.5)
    assert all(not np.any(applied[END + 1 + k]) for k in range(d))       # nothing of the old episode is applied in the new one
    checked = 0
    for L in range(T + 1 - d):
        if first[L + d] != first[L]:                          # the episode ends before the prediction's moment
            assert np.isfinite(preds[L]).all()
            continue
        s = seen[L]
        for k in range(d):
            s = ch.step_ego(s, applied[L + k], DT)
        assert np.abs(preds[L] - s).max() <= 1e-9, (L, preds[L], s)
        assert np.hypot(*(preds[L][:2] - true[L + d][:2])) <= 2e-5, (L, preds[L], true[L + d])
        checked += 1
    assert checked == T + 1 - 2 * d and comp.counts[0] == T + 1 - 2 * d and comp.sums[1, 0] <= 2e-5 + 4e-6
    # the compensator's prev is the actuator's applied action, bit for bit
    assert comp.prev.tobytes() == np.array([applied[-1]]).tobytes()


# ---- 3, 4, 5: identity, the others, non-finite commands -----------------------------------------------------------------------

def _one(kind, obs, R, **kw):
    """one environment, a reset launch on `obs` [R, 8] -> out [R, 8]"""
    outs = RUNNERS[kind]([dict(obs=np.ascontiguousarray(obs[None], F32), reset=True)], 1, R, kw)[0]
    return outs[0][0]


def _at_rest(rows):
    """an ego at rest at the origin - its rollout is exact: every action in flight after a reset is zero - and the rows given
    as (presence, x, y, vx, vy)"""
    obs = np.zeros((1 + len(rows), 8), F32)
    obs[0] = [1, 0, 0, 0, 0, 0, 0, 1]
    for i, r in enumerate(rows):
        obs[1 + i, :5] = r
        obs[1 + i, 5:] = [0.25 * (i + 1), 0.5, -0.5]          # marks the row: heading values are copied
    return obs


@pytest.mark.parametrize("kind", KINDS)
def test_steps_zero_copies_every_row_in_place_whatever_the_order(kind):
    obs = _at_rest([(1, 30, 0, 1, 2), (0, 7, 7, 7, 7), (1, 3, 4, -1, 0), (1, -1, 0, 0, 5)])      # far, absent garbage, near
    obs[0] = [1, 2.5, -3.25, 0.1, 9.0, 1.5, 0.9, 0.1]
    assert _one(kind, obs, 5, steps=0).tobytes() == obs.tobytes()
    launches = scene_stream(5, 10, 0, "on")
    outs = RUNNERS[kind](launches, 5, 10, dict(PARAMS["on"], steps=0))[0]
    assert all(o.tobytes() == s["obs"].tobytes() for o, s in zip(outs, launches))


@pytest.mark.parametrize("kind", KINDS)
def test_a_vehicle_that_overtakes_a_nearer_one_in_the_look_ahead_swaps_rows(kind):
    obs = _at_rest([(1, 10, 0, 0, 0), (1, 14, 0, -10, 0), (0, 1, 1, 1, 1), (1, 0, 40, 0, 0)])
    same = _one(kind, obs, 5, steps=1)                        # 14 - 1 = 13: still behind
    assert same[:, 5].tolist() == [0.0, 0.25, 0.5, 1.0, 0.0] and same[2, 1] == 13.0 and not same[4].any()
    out = _one(kind, obs, 5, steps=7)                         # 14 - 7 = 7: in front
    assert out[0].tolist() == [1, 0, 0, 0, 0, 0, 0, 1]
    assert out[:, 5].tolist() == [0.0, 0.5, 0.25, 1.0, 0.0] and out[1, :5].tolist() == [1.0, 7.0, 0.0, -10.0, 0.0]
    assert out[2, :5].tolist() == [1.0, 10.0, 0.0, 0.0, 0.0] and out[3, 2] == 40.0
    assert out[4].tobytes() == np.zeros(8, F32).tobytes()     # the absent row: last, +0.0f everywhere


@pytest.mark.parametrize("kind", KINDS)
def test_equal_keys_keep_the_input_order_and_absent_rows_stay_zero_and_last(kind):
    rows = [(1, 3, 4, 0, 0), (0, 0, 0, 0, 0), (1, -5, 0, 0, 0), (1, 4, -3, 0, 0), (1, 0, 1, 0, 0), (1, 0, 5, 0, 0)]
    out = _one(kind, _at_rest(rows), 7, steps=3)
    assert out[:, 5].tolist() == [0.0, 1.25, 0.25, 0.75, 1.0, 1.5, 0.0]      # the nearest, then the four ties in input order
    assert out[:, 0].tolist() == [1, 1, 1, 1, 1, 1, 0] and not out[6].any() and not np.signbit(out[6]).any()
    moving = [(1, 3, 4, 0, 0), (1, 5, 0, -10, 0), (1, 0, -4, 0, 10)]          # after 0.1 s: (3, 4), (4, 0), (0, -3): 25, 16, 9
    out = _one(kind, _at_rest(moving), 4, steps=1)
    assert out[:, 5].tolist() == [0.0, 0.75, 0.5, 0.25]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("steps", [0, 3])
def test_a_single_row_works(kind, steps):
    obs = np.array([[1, 2.0, 45.0, 0.0, -10.0, -math.pi / 2, -1.0, 0.0]], F32)
    outs, preds = RUNNERS[kind]([dict(obs=obs[None].copy(), reset=True)], 1, 1, dict(steps=steps))[:2]
    assert outs[0].shape == (1, 1, 8) and abs(preds[0][0, 1] - (45.0 - steps * 1.0)) < 1e-5 and abs(preds[0][0, 3] - 10.0) < 1e-6
    assert abs(outs[0][0, 0, 2] - (45.0 - steps)) < 1e-5 and outs[0][0, 0, 0] == 1.0


@pytest.mark.parametrize("kind", KINDS)
def test_a_non_finite_command_counts_as_zero_in_the_ring(kind):
    nan = float("nan")
    obs = _at_rest([])[None]
    cmds = [[1.0, 0.1], [nan, 0.2], [INF, -INF], [3.0, nan], [-0.0, 0.5]]
    launches = [dict(obs=obs, reset=True)] + [dict(obs=obs, command=np.array([c]), done=None) for c in cmds]
    run = RUNNERS[kind](launches, 1, 1, dict(steps=2))
    ring, prev, age = run[2], run[3], run[4]
    assert ring[:5, 0].tolist() == [[1.0, 0.1], [0.0, 0.2], [0.0, 0.0], [3.0, 0.0], [-0.0, 0.5]] and not ring[5:].any()
    assert np.signbit(ring[4, 0, 0]) and not np.signbit(ring[1:4, 0]).any()
    assert age.tolist() == [5] and prev[0].tolist() == [0.0, 0.0]             # the command of two launches ago: (inf, -inf) -> 0
    assert np.isfinite(run[1][-1]).all()


# ---- 6: argument checks -----------------------------------------------------------------------------------------------------------

def test_compensation_refuses_invalid_arguments():
    nan = float("nan")
    for kw in (dict(B=-1), dict(backend="cuda"), dict(R=0), dict(R=18), dict(dt=0.0), dict(dt=nan), dict(steps=-1),
               dict(steps=8), dict(steps=1.5), dict(tau=(-0.1, 0.0)), dict(tau=(0.0, nan)), dict(tau=(INF, 0.0)), dict(tau=1.0),
               dict(rate=(0.0, 1.0)), dict(rate=(1.0, -1.0)), dict(rate=(nan, 1.0)), dict(limits=((1.0, -1.0), (0.0, 0.0))),
               dict(limits=((nan, 1.0), (0.0, 0.0))), dict(limits="road"), dict(limits=(1.0, 2.0, 3.0))):
        args = dict(B=2, device="cpu", backend="torch")
        args.update(kw)
        with pytest.raises(ValueError):
            evaluate.Compensation(**args)
    a = evaluate.Compensation(2, "cpu", R=3, steps=7, tau=(1e3, 0.0), rate=(1e-9, INF), limits=((0.0, 0.0), (-INF, INF)))
    assert a.alpha[1] == 1.0 and 0.0 < a.alpha[0] < 1e-3 and evaluate.Compensation(2, "cpu", **a.config).config == a.config
    assert evaluate.Compensation(2, "cpu", limits="env").limits == ((-5.0, 5.0), (-math.pi / 4, math.pi / 4))
    obs, out = torch.zeros(2, 3, 8), torch.zeros(2, 3, 8)
    cmd = torch.zeros(2, 2, dtype=torch.float64)
    for bad in (dict(obs=obs.double(), out=out, command=cmd), dict(obs=obs, out=out.double(), command=cmd),
                dict(obs=torch.zeros(2, 4, 8), out=out, command=cmd), dict(obs=obs, out=torch.zeros(3, 3, 8), command=cmd),
                dict(obs=obs, out=obs, command=cmd), dict(obs=obs, out=obs, reset=True), dict(obs=obs, out=out),
                dict(obs=obs, out=out, command=cmd.float()), dict(obs=obs, out=out, command=torch.zeros(3, 2, dtype=torch.float64)),
                dict(obs=obs.to("meta"), out=out, command=cmd), dict(obs=None, out=out, command=cmd),
                dict(obs=obs, out=out, command=cmd, done=torch.zeros(3, dtype=torch.uint8)),
                dict(obs=obs, out=out, command=cmd, done=torch.zeros(2, dtype=torch.int32))):
        with pytest.raises(ValueError):
            a.apply(**bad)
    assert not a.age.any() and not a.pring.any()          # nothing ran
    assert a.apply(obs, out, reset=True) is out and a.apply(obs, out, command=cmd, done=torch.zeros(2, dtype=torch.bool)) is out
    assert a.age.tolist() == [1, 1]
    a.reset()
    assert not a.age.any() and not a.ring.any() and a.totals() == dict(scored=0, pos_err_mean=0.0, pos_err_max=0.0)
    m = evaluate.Compensation.matching(evaluate.Actuation(3, "cpu", delay=4, tau=(0.0, 0.2), rate=(9.0, INF), limits="env",
                                                          gain=(1.1, 1.0), sigma=(0.1, 0.0), p_hold=0.1))
    assert (m.B, m.R, m.steps, m.tau, m.rate, m.limits, m.dt) == (3, 10, 4, (0.0, 0.2), (9.0, INF), evaluate.ENV_LIMITS, 0.1)


def test_host_build_refuses_invalid_arguments():
    nan = float("nan")
    obs, cmd = np.zeros((2, 3, 8), F32), np.zeros((2, 2))
    for kw in (dict(steps=-1), dict(steps=8), dict(dt=0.0), dict(dt=nan), dict(alpha=(0.0, 1.0)), dict(alpha=(1.0, 1.5)),
               dict(alpha=(nan, 1.0)), dict(rate=(0.0, 1.0)), dict(rate=(1.0, nan)), dict(lo=(1.0, 0.0), hi=(0.0, 1.0)),
               dict(lo=(nan, 0.0)), dict(hi=(0.0, nan))):
        h = ch.HostCompensator(2, 3, **kw)
        rc, out, _ = h.step(obs, cmd)
        assert rc == -1 and h.step(obs, reset=True)[0] == -1 and np.isnan(out).all() and not h.age.any(), kw
    h = ch.HostCompensator(2, 3)
    for missing in ("obs", "command", "out", "ring", "prev", "age", "pring", "counts", "sums"):
        assert h.step(obs, cmd, missing=(missing,))[0] == -1, missing
    for missing in ("obs", "out", "ring", "prev", "age", "pring", "counts", "sums"):
        assert h.step(obs, reset=True, missing=(missing,))[0] == -1, missing
    assert h.step(obs, cmd, out=obs)[0] == -1 and h.step(obs, reset=True, out=obs)[0] == -1      # out must not be obs
    for R in (0, 18):
        bad = ch.HostCompensator(2, 3)
        bad.R = R
        assert bad.step(np.zeros((2, R, 8), F32), reset=True)[0] == -1
    negative = ch.HostCompensator(2, 3)
    negative.B = -1
    assert negative.step(obs, reset=True)[0] == -1
    assert not h.age.any()
    assert h.step(obs, reset=True, missing=("command", "done", "pred"))[0] == 0          # a reset launch needs neither
    assert h.step(obs, cmd, missing=("done", "pred"))[0] == 0 and h.age.tolist() == [1, 1]
    assert ch.HostCompensator(0, 3).step(np.zeros((0, 3, 8), F32), np.zeros((0, 2)))[0] == 0
    assert ch.HostCompensator(2, 3, steps=7, alpha=(1e-6, 1.0), rate=(1e-9, INF), lo=(0.0, -INF), hi=(0.0, INF)).step(obs, cmd)[0] == 0


# ---- 7: signatures and structs ------------------------------------------------------------------------------------------------------

def _prototype():
    """[(parameter name, kind)] of mpc_compensate's prototype in the header, kinds as engine.COMPENSATION_SIGNATURES spells them"""
    from test_abi import _header_text
    m = re.search(r"\bint\s+mpc_compensate\s*\(([^)]*)\)\s*;", _header_text())
    assert m, "mpc_compensate: no prototype in include/mpc_mi355x.h"
    out = []
    for decl in m.group(1).split(","):
        ctype, pname = re.fullmatch(r"\s*(.*?)(\w+)\s*", decl, flags=re.S).groups()
        ctype = " ".join(ctype.replace("*", " * ").split())
        if ctype.endswith("*"):
            kind = "compensator" if ctype == "const mpc_compensator *" else "ptr"
        else:
            kind = {"int32_t": "i32", "uint64_t": "u64", "double": "f64"}[ctype]
        out.append((pname, kind))
    return out


def test_compensation_signature_table_is_the_header_and_the_other_tables_are_untouched():
    from mpc_rl_for_avs_amd import engine
    from test_abi import _header_text
    assert sorted(engine.COMPENSATION_SIGNATURES) == ["mpc_compensate"]
    tables = (engine.SIGNATURES, engine.EVALUATION_SIGNATURES, engine.TRACKER_SIGNATURES, engine.PLAN_SIGNATURES,
              engine.ACTUATION_SIGNATURES)
    assert len(engine._TABLES) == 5 and all(a is b for a, b in zip(engine._TABLES, tables))
    assert not any("mpc_compensate" in t for t in engine._TABLES)
    sig = engine.COMPENSATION_SIGNATURES["mpc_compensate"]
    assert list(sig) == _prototype() and len({n for n, _ in sig}) == len(sig)
    i, vp = ctypes.c_int32, ctypes.c_void_p
    lib = engine.load_library()
    assert list(lib.mpc_compensate.argtypes) == [i, i, i, i, ctypes.POINTER(engine.CompensatorParams)] + [vp] * 11 + [vp]
    assert lib.mpc_compensate.restype is ctypes.c_int and "mpc_compensate" in engine._EXPORTS
    assert callable(engine.caller("mpc_compensate")) and engine.ABI_VERSION == 8
    with pytest.raises(TypeError, match="mpc_compensate"):
        engine.call("mpc_compensate", device=0)
    body = re.search(r"typedef struct mpc_compensator \{(.*?)\} mpc_compensator;", _header_text(), flags=re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|uint64_t|double)\s+(\w+)(\[2\])?;", body, flags=re.M)
    ctype = dict(int32_t=ctypes.c_int32, uint64_t=ctypes.c_uint64, double=ctypes.c_double)
    want = [(name, ctype[t] * 2 if arr else ctype[t]) for t, name, arr in fields]
    assert len(want) == 7 and [(n, t) for n, t in engine.CompensatorParams._fields_] == want
    assert ctypes.sizeof(engine.CompensatorParams) == 2 * 4 + 8 + 4 * 16


# ---- 8: the evaluator --------------------------------------------------------------------------------------------------------------

from test_actuator_cpu import _evaluate, _same_results                       # noqa: E402  (the PPOAgent run of that module)

LATENCY = dict(delay=3, tau=(0.0, 0.2), limits="env")


@pytest.fixture(scope="module")
def plain():
    return _evaluate()


def test_evaluate_agent_without_a_compensator_and_with_steps_zero_is_the_plain_run(plain):
    none = _evaluate(compensation=None)
    _same_results(plain, none)
    strip = lambda d: {k: v for k, v in d.items() if k not in ("seconds", "env_steps_per_s")}
    assert strip(plain.summary()) == strip(none.summary()) and none.compensation is None
    assert not any(k.startswith("comp_") for k in none.summary())
    frames = []
    zero = _evaluate(compensation=dict(steps=0), on_step=lambda d: frames.append({k: d[k].clone() for k in ("seen", "ahead", "obs")}))
    _same_results(plain, zero)
    assert zero.compensation == dict(scored=0, pos_err_mean=0.0, pos_err_max=0.0)
    assert all(f["seen"].numpy().tobytes() == f["ahead"].numpy().tobytes() == f["obs"].numpy().tobytes() for f in frames)
    assert zero.traces.seen is not None                      # `seen` is recorded with a compensator alone
    given = evaluate.Compensation(8, "cpu", "torch", steps=0, tau=(0.3, 0.3))      # an instance; the model does not matter at 0
    _same_results(plain, _evaluate(compensation=given))
    assert given.age.max() > 0


def test_a_matching_compensator_predicts_the_ego_and_a_mismatched_one_does_not():
    """(b) and (c) of the issue: with the compensator of the actuator's own delay, lag and limits the predicted ego is the ego
    observed three steps later to f32 rounding, comp_pos_err_max <= 1e-3 m (the inputs' rounding over seven steps at 30 m/s is
    about 2e-5 m; one wrong ring index costs more than 1e-2 m); a compensator that looks two steps ahead where the delay is
    three, and knows no lag, exceeds 1e-2 m: the gate bites."""
    frames = []
    good = _evaluate(actuation=dict(LATENCY), compensation=True,
                     on_step=lambda d: frames.append({k: d[k].clone() for k in ("seen", "ahead", "obs")}))
    s = good.summary()
    print("matching:", good.compensation)
    assert good.compensation["scored"] > 0 and s["comp_pos_err_max"] == good.compensation["pos_err_max"] <= 1e-3
    assert 0.0 < s["comp_pos_err_mean"] <= s["comp_pos_err_max"]
    assert all(f["seen"].numpy().tobytes() == f["ahead"].numpy().tobytes() for f in frames)
    assert any(f["ahead"].numpy().tobytes() != f["obs"].numpy().tobytes() for f in frames)       # the agent acts on another scene
    base = _evaluate(actuation=dict(LATENCY))
    assert good.records["return"].tobytes() != base.records["return"].tobytes() and base.compensation is None
    bad = _evaluate(actuation=dict(LATENCY), compensation=dict(steps=2))
    print("mismatched:", bad.compensation)
    assert bad.compensation["scored"] > 0 and bad.compensation["pos_err_max"] > 1e-2


def test_evaluate_agent_refuses_what_a_compensator_cannot_serve():
    import policy_ref as pr
    agent = rollout.PPOAgent(pr.make_policy(64, 2, -0.5, use_sde=False, seed=8))
    env = lambda: rollout.SyntheticIntersectionEnv(4, device="cpu", seed=3, n_others=4, backend="torch")
    run = lambda a=agent, **kw: evaluate.evaluate_agent(a, env(), use_graph=False, **kw)
    with pytest.raises(ValueError, match="actuator"):
        run(compensation=True)
    with pytest.raises(ValueError, match="compensation"):
        run(compensation=evaluate.Compensation(3, "cpu", "torch"))
    with pytest.raises(ValueError, match="compensation"):
        run(compensation=evaluate.Compensation(4, "cpu", "torch", R=9))
    with pytest.raises(ValueError, match="compensation"):
        run(compensation=evaluate.Compensation(4, "meta", "torch"))
    with pytest.raises(ValueError):
        run(compensation=dict(steps=9))

    class Planner:                                           # an agent with a plan, as far as the argument checks look
        HAS_PLAN, engine = True, type("E", (), dict(horizon=20))()

        def act_batch_torch(self, obs, plan=False, **kw):
            raise AssertionError("not reached")
    for kw in (dict(plan=True), dict(trace=dict(plan=True))):
        with pytest.raises(ValueError, match="steps > 0"):
            run(Planner(), compensation=dict(steps=1), **kw)
    assert run(compensation=dict(steps=1), trace=dict(seen=True)).traces.seen is not None


def test_compare_gives_every_agent_a_fresh_compensator():
    import policy_ref as pr
    agent = lambda: rollout.PPOAgent(pr.make_policy(64, 2, -0.5, use_sde=False, seed=9))
    make_env = lambda: rollout.SyntheticIntersectionEnv(4, device="cpu", seed=2, n_others=4, backend="torch")
    results = {}
    out = evaluate.compare({"a": agent(), "b": agent()}, make_env, 1, actuation=dict(delay=2), compensation=True,
                           results=results, use_graph=False)
    ca, cb = results["a"].compensation, results["b"].compensation
    assert ca == cb and ca["scored"] > 0 and out["a"]["comp_pos_err_max"] == out["b"]["comp_pos_err_max"] <= 1e-3      # not accumulated
    inst = evaluate.Compensation(4, "cpu", "torch", steps=2)
    out2 = evaluate.compare({"a": agent()}, make_env, 1, actuation=dict(delay=2), compensation=inst, use_graph=False)
    assert out2["a"]["comp_pos_err_max"] == out["a"]["comp_pos_err_max"] and inst.totals()["scored"] == 0      # a copy ran
    out3 = evaluate.compare({"a": agent()}, make_env, 1, actuation=dict(delay=2), compensation=dict(steps=2), use_graph=False)
    assert out3["a"]["comp_pos_err_mean"] == out["a"]["comp_pos_err_mean"]
    assert "comp_pos_err_max" not in evaluate.compare({"a": agent()}, make_env, 1, use_graph=False)["a"]


# ---- 9: sanitizers: a stand-alone program, nothing loaded into Python ----------------------------------------------------------

def test_host_build_runs_clean_under_address_and_undefined_behaviour_sanitizers():
    out = os.path.join(conftest.ROOT, "tests", "_build", "compensate_san_main")
    src = os.path.join(conftest.ROOT, "tests", "compensate_san_main.cpp")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in [src] + ch.DEPS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                        "-static-libubsan", "-std=c++17", "-Wno-unknown-pragmas", "-ffp-contract=off", "-o", out, src],
                       check=True)
    res = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "compensate_san_main: ok" in res.stdout, res.stdout + res.stderr
