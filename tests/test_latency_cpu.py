"""The sensing latency of the closed-loop evaluation and the compensator that knows of it, on the CPU: the host builds of
csrc/mpc_latency.hpp and of csrc/mpc_compensate.hpp's latency-aware build, the evaluator's CPU path and plain-Python restatements
(tests/latency_host.py, tests/compensate_stale_host.py) against one another on streams with the edge cases forced; tagged frames,
so that "no frame of a finished episode is shown in the next one" is an equality; the latency-0 build against mpc_compensate's
host build; the prediction against a plant driven through the actuator's host build and observed through the latency's; the
signature table; evaluate_agent with a latency on the torch environment; a sanitizer run in a stand-alone program.

THE YARDSTICK (shared with tests/test_latency_gpu.py).  The latency stage copies and counts: out, stale, age, counts and
sums[0] are compared bit for bit; the lag sums go through sqrt and agree to rtol 1e-9, the project's bound for such sums.  The
compensator is held to tests/test_compensate_cpu.py's yardstick, `assert_runs_agree`, unchanged."""
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
import compensate_stale_host as sh
import conftest
import latency_host as lh
from mpc_rl_for_avs_amd import evaluate, rollout
from test_compensate_cpu import (DT, KEY_GAP, PARAMS, _keys, _observe, _same_bits, _seen_state, assert_runs_agree,
                                 ego_row, entry_params)

F32 = np.float32
T_LAT, LAT_RESET_AT = 22, 3                                  # launches of a latency stream (the ring wraps twice), its second reset
LAT_DONE_AT = (6, 7, 9, 18)                                  # + b % 3: consecutive ends, an end while stale < steps, a late one
T_COMP, COMP_RESET_AT = 22, 2
COMP_DONE_AT = (4, 5, 8, 16)                                 # + b % 3
STAGGER_AT = 13                                              # stale_stream(staggered=True): the launch of four different look-aheads
PAIRS = [(0, 0), (0, 1), (0, 3), (0, 7), (1, 0), (1, 2), (2, 1), (3, 0), (3, 3), (3, 4), (1, 6), (7, 0)]     # (d, L), d + L <= 7


# ---- the latency stage ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def frame_stream(B, R):
    """T_LAT launches: dicts with obs [B, R, 8] f32 and done [B] u8 or None, or obs and reset=True (launches 0 and LAT_RESET_AT).
    Every element is TAGGED: obs[b, r, c] of launch k is 4096 k + 512 b' + 8 r + c (b' = b % 8; exact in f32), so the launch a
    frame came from can be read off any of its elements; on every fifth launch the last element of the last row is a NaN with a
    payload and the one before it -0.0, which a copy must keep.  Environment b's episode ends on the launches LAT_DONE_AT + b % 3;
    launches with k % 5 == 0 pass no done at all."""
    launches = []
    b_, r_, c_ = np.meshgrid(np.arange(B) % 8, np.arange(R), np.arange(8), indexing="ij")
    for k in range(T_LAT):
        obs = (4096 * k + 512 * b_ + 8 * r_ + c_).astype(F32)
        if k % 5 == 4:
            obs[:, R - 1, 7] = np.array([0x7FC12345], np.uint32).view(F32)[0]
            obs[:, R - 1, 6] = F32(-0.0)
        if k in (0, LAT_RESET_AT):
            launches.append(dict(obs=obs, reset=True))
            continue
        done = None
        if k % 5 != 0:
            done = np.isin(k - np.arange(B) % 3, LAT_DONE_AT).astype(np.uint8)
        launches.append(dict(obs=obs, done=done))
    return launches


def episode_starts(launches, B):
    """first [T][B]: the launch on which the episode of (launch, environment) began"""
    first, cur = [], np.zeros(B, int)
    for k, s in enumerate(launches):
        if s.get("reset"):
            cur = np.full(B, k)
        elif s.get("done") is not None:
            cur = np.where(np.asarray(s["done"]) != 0, k, cur)
        first.append(cur.copy())
    return first


def lat_host(launches, B, R, steps, stale=True):
    h = lh.HostLatency(B, R, steps)
    outs, stales = [], []
    for s in launches:
        rc, out, st = h.step(s["obs"], s.get("done"), bool(s.get("reset")), stale=stale)
        assert rc == 0
        outs.append(out)
        stales.append(st)
    return outs, stales, h.age.copy(), h.counts.copy(), h.sums.copy()


def lat_class(launches, B, R, steps, device="cpu", backend="torch"):
    a = evaluate.Latency(B, device, backend, R=R, steps=steps)
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(a.device)
    outs, stales = [], []
    for s in launches:
        obs = t(s["obs"])
        out = torch.full_like(obs, float("nan"))
        assert a.apply(obs, out, done=t(s.get("done")), reset=bool(s.get("reset"))) is out
        outs.append(out.cpu().numpy().copy())
        stales.append(a.stale.cpu().numpy().copy())
    n = lambda x: x.cpu().numpy().copy()
    return outs, stales, n(a.age), n(a.counts), n(a.sums)


def lat_python(launches, B, R, steps):
    return lh.replay(launches, B, R, steps)


def assert_latency_runs_agree(got, want, what):
    for k, (g, w) in enumerate(zip(got[0], want[0])):
        _same_bits(g, w, f"{what}: out of launch {k}")
    for k, (g, w) in enumerate(zip(got[1], want[1])):
        if g is not None and w is not None:
            _same_bits(g, w, f"{what}: stale of launch {k}")
    _same_bits(got[2], want[2], f"{what}: age")
    _same_bits(got[3], want[3], f"{what}: counts")
    _same_bits(got[4][0], want[4][0], f"{what}: sums[0]")
    assert np.allclose(got[4][1:], want[4][1:], rtol=1e-9, atol=0.0), (what, got[4], want[4])


def assert_frames_are_of_this_episode(launches, outs, stales, B, steps):
    """the tags: out of launch k is the obs of launch k - stale, bit for bit, stale = min(steps, launches since the episode
    began), so a frame of a finished episode never appears after its done"""
    first = episode_starts(launches, B)
    for k, (out, st) in enumerate(zip(outs, stales)):
        want = np.minimum(steps, k - first[k])
        assert st.tolist() == want.tolist(), (k, st, want)
        for b in range(B):
            src = launches[k - want[b]]["obs"][b]
            assert out[b].tobytes() == src.tobytes(), (k, b)
            tag = int(out[b, 0, 0]) // 4096                  # the launch the frame was pushed on
            assert tag == k - want[b] >= first[k][b]


@pytest.mark.parametrize("steps", [0, 1, 3, 7])
@pytest.mark.parametrize("R", [1, 2, 17])
@pytest.mark.parametrize("B", [1, 5])
def test_latency_host_build_restatement_and_torch_backend_agree(B, R, steps):
    launches = frame_stream(B, R)
    host = lat_host(launches, B, R, steps)
    assert_latency_runs_agree(host, lat_python(launches, B, R, steps), "host build vs restatement")
    assert_latency_runs_agree(lat_class(launches, B, R, steps), host, "torch vs host build")
    assert_latency_runs_agree(lat_host(launches, B, R, steps, stale=False), host, "host build without stale")
    outs, stales, age, counts, sums = host
    assert_frames_are_of_this_episode(launches, outs, stales, B, steps)
    first = episode_starts(launches, B)
    since = T_LAT - LAT_RESET_AT
    assert age.tolist() == (T_LAT - first[-1]).tolist() and counts.tolist() == [since] * B
    assert sums[0].tolist() == [float(sum(s[b] for s in stales[LAT_RESET_AT:])) for b in range(B)]
    if steps == 0:
        assert not sums.any() and all(o.tobytes() == s["obs"].tobytes() for o, s in zip(outs, launches))
    else:
        assert (sums[2] > 0).all() and (sums[1] >= sums[2]).all() and max(int(s.max()) for s in stales) == steps


def test_the_frame_streams_force_the_edge_cases():
    launches = frame_stream(5, 17)
    assert T_LAT >= 20 and [bool(s.get("reset")) for s in launches] == [k in (0, LAT_RESET_AT) for k in range(T_LAT)]
    dones = np.array([s["done"] if s.get("done") is not None else np.zeros(5, np.uint8) for s in launches])
    assert dones[6].tolist() == [1, 0, 0, 1, 0] and dones[7].tolist() == [1, 1, 0, 1, 1] and dones[8].tolist() == [0, 1, 1, 0, 1]
    assert len({tuple(np.flatnonzero(dones[:, b])) for b in range(3)}) == 3      # at different launches per environment
    assert any(s.get("done") is None for s in launches if not s.get("reset"))
    stales = lat_host(launches, 5, 17, 3)[1]
    at = [np.flatnonzero(dones[:, 0])[i] for i in (1, 2)]                        # environment 0: ends again while stale < steps
    assert stales[at[0] - 1][0] == 0 and stales[at[1] - 1][0] == 1 and stales[at[1]][0] == 0
    assert np.isnan(launches[4]["obs"][0, 16, 7]) and np.signbit(launches[4]["obs"][0, 16, 6])


def test_latency_refuses_invalid_arguments():
    for kw in (dict(B=-1), dict(backend="cuda"), dict(R=0), dict(R=18), dict(steps=-1), dict(steps=8), dict(steps=1.5),
               dict(steps=True)):
        with pytest.raises(ValueError):
            evaluate.Latency(**dict(dict(B=2, device="cpu", backend="torch"), **kw))
    a = evaluate.Latency(2, "cpu", R=3, steps=7)
    assert a.config == dict(R=3, steps=7) and evaluate.Latency(2, "cpu", **a.config).config == a.config
    obs, out = torch.zeros(2, 3, 8), torch.zeros(2, 3, 8)
    for bad in (dict(obs=obs.double(), out=out), dict(obs=obs, out=out.double()), dict(obs=torch.zeros(2, 4, 8), out=out),
                dict(obs=obs, out=obs), dict(obs=obs, out=obs, reset=True), dict(obs=None, out=out),
                dict(obs=obs, out=out, done=torch.zeros(3, dtype=torch.uint8)),
                dict(obs=obs, out=out, done=torch.zeros(2, dtype=torch.int32))):
        with pytest.raises(ValueError):
            a.apply(**bad)
    assert not a.age.any() and not a.counts.any()            # nothing ran
    assert a.apply(obs, out, reset=True) is out and a.apply(obs, out, done=torch.zeros(2, dtype=torch.bool)) is out
    assert a.age.tolist() == [2, 2] and a.totals() == dict(frames=4, stale_mean=0.5, ego_lag_mean=0.0, ego_lag_max=0.0)
    a.reset()
    assert not a.age.any() and a.totals() == dict(frames=0, stale_mean=0.0, ego_lag_mean=0.0, ego_lag_max=0.0)
    obs_n = np.zeros((2, 3, 8), F32)
    for steps in (-1, 8):
        assert lh.HostLatency(2, 3, steps).step(obs_n, reset=True)[0] == -1
    h = lh.HostLatency(2, 3, 2)
    for missing in ("obs", "out", "frames", "age", "counts", "sums"):
        assert h.step(obs_n, missing=(missing,))[0] == -1, missing
    assert h.step(obs_n, out=obs_n)[0] == -1 and not h.age.any()
    for R in (0, 18):
        bad = lh.HostLatency(2, 3, 1)
        bad.R = R
        assert bad.step(np.zeros((2, R, 8), F32), reset=True)[0] == -1
    assert h.step(obs_n, missing=("done", "stale"))[0] == 0 and h.age.tolist() == [1, 1]
    assert lh.HostLatency(0, 3, 1).step(np.zeros((0, 3, 8), F32))[0] == 0


# ---- the compensator that knows of the latency ------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def stale_stream(B, R, d, L, name, staggered=False):
    """tests/test_compensate_cpu.py's scene_stream for Compensation(steps=d, latency=L, **PARAMS[name]), T_COMP launches: reset
    launches 0 and COMP_RESET_AT, environment b's episode ends on the launches COMP_DONE_AT + b % 3 (consecutive ends, one
    while the look-ahead still grows, a late one after which more than eight commands follow), launches with k % 4 == 2 pass no
    done; one command is NaN and one infinite.  The look-ahead of a launch differs between environments, h = (d + min(L, age))
    dt: any two present keys are KEY_GAP apart about the host build's predicted ego both at that h and at the longest one,
    (d + L) dt - asserted here, by the argument of that generator's docstring.  staggered: environment b's episode ends on
    launch STAGGER_AT - b % 4 instead (b % 4 == 3: on launch 5), so that on launch STAGGER_AT four neighbouring environments
    are 0, 1, 2 and at least 3 launches into their episodes and their look-aheads all differ."""
    kw = dict(PARAMS[name], steps=d, latency=L)
    rng = np.random.default_rng(100000 * B + 1000 * R + 100 * d + 10 * L + len(name) + 7 * staggered)
    host = sh.HostStaleCompensator(B, R, **entry_params(kw))
    launches = []
    for k in range(T_COMP):
        reset = k in (0, COMP_RESET_AT)
        th, sp = rng.uniform(-math.pi, math.pi, B), rng.uniform(0.0, 12.0, B)
        sp[0] = (29.5, 0.2, 11.0)[k % 3]
        obs = np.zeros((B, R, 8), F32)
        obs[:, 0] = ego_row(rng.uniform(-8.0, 8.0, B), rng.uniform(-8.0, 8.0, B), th, sp)
        cmd = done = None
        if not reset:
            cmd = np.stack([rng.uniform(-8.0, 8.0, B), rng.uniform(-1.2, 1.2, B)], axis=1)
            if k == 7:
                cmd[B - 1, 0] = np.nan
            if k == 11:
                cmd[B - 1, 1] = -np.inf
            if staggered:
                done = (k == np.where(np.arange(B) % 4 == 3, 5, STAGGER_AT - np.arange(B) % 4)).astype(np.uint8)
            elif k % 4 != 2:
                done = np.isin(k - np.arange(B) % 3, COMP_DONE_AT).astype(np.uint8)
        _, pred = host.apply(obs, cmd, done, reset)          # the others do not enter the ego's prediction
        ahead = d + np.minimum(L, host.age)
        ex, ey = (F32(pred[:, 0]), F32(pred[:, 1])) if d + L > 0 else (obs[:, 0, 1], obs[:, 0, 2])
        for b in range(B):
            for _ in range(400):
                n = R - 1
                v = rng.uniform(-5.0, 5.0, (n, 2))
                hd = np.arctan2(v[:, 1], v[:, 0])
                rows = np.stack([(rng.random(n) < 0.7).astype(np.float64), rng.uniform(-15.0, 15.0, n), rng.uniform(-15.0, 15.0, n),
                                 v[:, 0], v[:, 1], hd, np.sin(hd), np.cos(hd)], axis=1).astype(F32)
                here = rows[rows[:, 0] != 0]
                gaps = [np.diff(np.sort(_keys(here, float(a) * DT, ex[b], ey[b]))) for a in (ahead[b], d + L)]
                if len(here) < 2 or min(g.min() for g in gaps) > KEY_GAP:
                    break
            else:
                raise AssertionError("no scene with separated keys")
            obs[b, 1:] = rows
        assert np.isfinite(obs).all()
        launches.append(dict(obs=obs, reset=True) if reset else dict(obs=obs, command=cmd, done=done))
    return launches


def stale_host(launches, B, R, kw, pred=True):
    h = sh.HostStaleCompensator(B, R, **entry_params(kw))
    outs, preds = [], []
    for s in launches:
        rc, out, p = h.step(s["obs"], s.get("command"), s.get("done"), bool(s.get("reset")), pred=pred)
        assert rc == 0
        outs.append(out)
        preds.append(p)
    return outs, preds, h.ring.copy(), h.prev.copy(), h.age.copy(), h.pring.copy(), h.counts.copy(), h.sums.copy()


def stale_class(launches, B, R, kw, device="cpu", backend="torch"):
    from test_compensate_cpu import run_class
    return run_class(launches, B, R, kw, device=device, backend=backend)


def stale_python(launches, B, R, kw):
    return sh.replay(launches, B, R, **entry_params(kw))


@pytest.mark.parametrize("name", list(PARAMS))
@pytest.mark.parametrize("d,L", PAIRS)
@pytest.mark.parametrize("R", [1, 2, 17])
@pytest.mark.parametrize("B", [1, 5])
def test_stale_host_build_restatement_and_torch_backend_agree(B, R, d, L, name):
    kw = dict(PARAMS[name], steps=d, latency=L)
    launches = stale_stream(B, R, d, L, name)
    host = stale_host(launches, B, R, kw)
    identity = 0 if d + L == 0 else 1                        # assert_runs_agree's `steps`: only 0 makes the ego's row a copy
    assert_runs_agree(host, stale_python(launches, B, R, kw), "host build vs restatement", identity)
    assert_runs_agree(stale_class(launches, B, R, kw), host, "torch vs host build", identity)
    assert_runs_agree(stale_host(launches, B, R, kw, pred=False), host, "host build without pred", identity)
    outs, preds, ring, prev, age, pring, counts, sums = host
    first = episode_starts(launches, B)
    assert age.tolist() == (T_COMP - 1 - first[-1]).tolist() and all(np.isfinite(p).all() for p in preds)
    if d + L == 0:
        assert not counts.any() and not sums.any()
        assert all(o.tobytes() == s["obs"].tobytes() for o, s in zip(outs, launches))
    else:
        # one prediction scored on every launch of an episode whose age has reached d + L, since the second reset
        want = sum((k - first[k] >= d + L).astype(int) for k in range(COMP_RESET_AT, T_COMP))
        assert counts.tolist() == want.tolist() and counts.any() and ((counts > 0) == (sums[1] > 0)).all()
        for o, s in zip(outs, launches):                     # present rows first, the rest zero, nothing lost
            present = o[:, 1:, 0] != 0
            assert (present.sum(axis=1) == (s["obs"][:, 1:, 0] != 0).sum(axis=1)).all()
            assert (np.diff(present.astype(int), axis=1) <= 0).all() and not o[:, 1:][~present].any()


@pytest.mark.parametrize("name", list(PARAMS))
@pytest.mark.parametrize("d", [0, 1, 3, 7])
def test_with_latency_zero_the_stale_build_is_mpc_compensates_build_array_for_array(d, name):
    from test_compensate_cpu import run_host, scene_stream
    B, R = 5, 17
    kw = dict(PARAMS[name], steps=d)
    for launches in (scene_stream(B, R, d, name), stale_stream(B, R, d, 0, name)):
        old, new = run_host(launches, B, R, kw), stale_host(launches, B, R, dict(kw, latency=0))
        for k, (a, b) in enumerate(zip(old[0] + old[1], new[0] + new[1])):
            assert a.tobytes() == b.tobytes(), ("out / pred", k)
        for n, a, b in zip(("ring", "prev", "age", "pring", "counts", "sums"), old[2:], new[2:]):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), n
    cls = evaluate.Compensation(B, "cpu", **dict(kw, dt=DT))
    assert cls.latency == 0 and "latency" not in cls.config


@pytest.mark.parametrize("d,L", [(0, 3), (2, 3), (1, 6)])
def test_four_neighbours_with_four_different_look_aheads(d, L):
    B, R = 5, 17
    kw = dict(PARAMS["on"], steps=d, latency=L)
    launches = stale_stream(B, R, d, L, "on", staggered=True)
    first = episode_starts(launches, B)
    assert (STAGGER_AT - first[STAGGER_AT][:4]).tolist() == [0, 1, 2, 8]      # so d + min(L, age) = d, d + 1, d + 2, d + 3
    host = stale_host(launches, B, R, kw)
    assert_runs_agree(host, stale_python(launches, B, R, kw), "host build vs restatement", 1)
    assert_runs_agree(stale_class(launches, B, R, kw), host, "torch vs host build", 1)


def test_stale_compensation_refuses_invalid_arguments():
    for kw in (dict(latency=-1), dict(latency=8), dict(steps=4, latency=4), dict(steps=7, latency=1), dict(latency=1.5)):
        with pytest.raises(ValueError):
            evaluate.Compensation(2, "cpu", **kw)
    a = evaluate.Compensation(2, "cpu", R=3, steps=3, latency=4)
    assert a.config["latency"] == 4 and evaluate.Compensation(2, "cpu", **a.config).config == a.config
    obs, cmd = np.zeros((2, 3, 8), F32), np.zeros((2, 2))
    for kw in (dict(latency=-1), dict(latency=8), dict(steps=4, latency=4), dict(steps=7, latency=1), dict(steps=-1, latency=1),
               dict(latency=1, dt=float("nan")), dict(latency=1, alpha=(float("nan"), 1.0))):
        h = sh.HostStaleCompensator(2, 3, **kw)
        assert h.step(obs, cmd)[0] == -1 and h.step(obs, reset=True)[0] == -1 and not h.age.any(), kw
    assert sh.HostStaleCompensator(2, 3, steps=3, latency=4).step(obs, cmd)[0] == 0
    act = evaluate.Actuation(3, "cpu", delay=2, tau=(0.0, 0.2), limits="env")
    lat = evaluate.Latency(3, "cpu", steps=3)
    m = evaluate.Compensation.matching(act, lat)
    assert (m.B, m.steps, m.latency, m.tau, m.limits) == (3, 2, 3, (0.0, 0.2), evaluate.ENV_LIMITS)
    m = evaluate.Compensation.matching(latency=lat, dt=0.05)
    assert (m.B, m.steps, m.latency, m.tau, m.dt, m.backend) == (3, 0, 3, (0.0, 0.0), 0.05, "torch")
    assert evaluate.Compensation.matching(act).latency == 0 and evaluate.Compensation.matching(actuation=act).steps == 2
    with pytest.raises(ValueError):
        evaluate.Compensation.matching()
    with pytest.raises(ValueError):
        evaluate.Compensation.matching(act, evaluate.Latency(4, "cpu", steps=1))
    with pytest.raises(ValueError):
        evaluate.Compensation.matching(evaluate.Actuation(3, "cpu", delay=5), lat)       # 5 + 3 > 7


# ---- against the future itself -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shaped", [False, True], ids=["delay", "delay_lag_rate_limits"])
@pytest.mark.parametrize("d,L", [(0, 1), (0, 3), (1, 2), (3, 3), (2, 5), (0, 7), (4, 1)])
def test_the_prediction_from_a_stale_scene_is_the_plant_d_steps_on(d, L, shaped):
    """tests/test_compensate_cpu.py's plant, driven through the actuator's host build with delay d by the same scripted
    commands, with an episode end midway; its observations pass through the latency's host build with L steps.  pred of the
    launch n launches into an episode is the plant after n + d steps of the episode: to 1e-9 when the plant is rolled on from
    the state the compensator was shown - the scene of min(L, n) steps ago - through the actions the actuator really applied
    since, and to 2e-5 m against the true plant (that test's bounds and derivation; the look-ahead d + L is at most its 7
    steps).  prev is the actuator's applied action of step n - 1 - L, bit for bit.  A compensator told L - 1 is handed the same
    frames and MUST fail the second bound: the check can tell a latency that is off by one."""
    T, END = 34, 15
    model = dict(alpha=(0.5, 1.0 / 3.0), rate=(20.0, 1.5), lo=(-2.5, -0.3), hi=(2.5, 0.3)) if shaped else dict()
    act = ah.HostActuator(1, delay=d, dt=DT, **model)
    lat = lh.HostLatency(1, 1, L)
    comp = sh.HostStaleCompensator(1, 1, steps=d, latency=L, dt=DT, **model)
    short = sh.HostStaleCompensator(1, 1, steps=d, latency=L - 1, dt=DT, **model)
    script = lambda t: np.array([[3.0 if (t // 2) % 2 == 0 else -3.0, -0.4 + 0.05 * t]])
    starts = (np.array([2.0, 45.0, -math.pi / 2, 10.0]), np.array([-30.0, -2.0, 0.1, 6.0]))
    state = starts[0]
    obs = _observe(state)
    late, stale = lat.apply(obs, reset=True)
    _, pred = comp.apply(late, reset=True)
    _, pred_short = short.apply(late, reset=True)
    preds, wrong, seen, true, applied, first, stales = [pred[0].copy()], [pred_short[0].copy()], [_seen_state(late)], \
        [state.copy()], [], [0], [int(stale[0])]
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
        done = np.array([ended], np.uint8)
        late, stale = lat.apply(obs, done)
        _, pred = comp.apply(late, cmd.copy(), done)
        _, pred_short = short.apply(late, cmd.copy(), done)
        preds.append(pred[0].copy()), wrong.append(pred_short[0].copy()), seen.append(_seen_state(late))
        true.append(state.copy()), stales.append(int(stale[0]))
        first.append(t + 1 if ended else first[-1])           # the launch on which the current episode began
        n = t + 1 - first[-1]                                 # launches into the episode; prev: the applied action of step n - 1 - L
        want = applied[t - L] if n - 1 - L >= 0 else np.zeros(2)
        assert comp.prev[0].tobytes() == np.asarray(want, np.float64).tobytes(), (t, comp.prev, want)
    assert stales == [min(L, k - first[k]) for k in range(T + 1)] and max(stales) == L
    checked, worst, worst_short = 0, 0.0, 0.0
    for n in range(T + 1 - d):
        if first[n + d] != first[n]:                          # the episode ends before the prediction's moment
            assert np.isfinite(preds[n]).all()
            continue
        s = seen[n]
        for k in range(d + stales[n]):
            s = ch.step_ego(s, applied[n - stales[n] + k], DT)
        assert np.abs(preds[n] - s).max() <= 1e-9, (n, preds[n], s)
        off = np.hypot(*(preds[n][:2] - true[n + d][:2]))
        assert off <= 2e-5, (n, preds[n], true[n + d])
        worst, worst_short = max(worst, off), max(worst_short, np.hypot(*(wrong[n][:2] - true[n + d][:2])))
        checked += 1
    assert checked == T + 1 - 2 * d
    assert worst_short > 2e-5, "a compensator told L - 1 passes the check: it cannot tell the latency"
    assert worst_short > 1e-2                                 # in fact it misses by a step's travel
    scored = sum(1 for k in range(T + 1) if k - first[k] >= d + L)
    assert comp.counts[0] == scored > 0 and comp.sums[1, 0] <= 2e-5 + 4e-6


# ---- signatures ---------------------------------------------------------------------------------------------------------------------

def _prototype(name):
    """[(parameter name, kind)] of `name`'s prototype in the header, kinds as engine.LATENCY_SIGNATURES spells them"""
    from test_abi import _header_text
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", _header_text())
    assert m, f"{name}: no prototype in include/mpc_mi355x.h"
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


def test_latency_signature_table_is_the_header_and_the_other_tables_are_untouched():
    from mpc_rl_for_avs_amd import engine
    assert sorted(engine.LATENCY_SIGNATURES) == ["mpc_compensate_stale", "mpc_delay_scene"]
    assert len(engine._TABLES) == 5 and sorted(engine.COMPENSATION_SIGNATURES) == ["mpc_compensate"]
    assert not any(n in t for n in engine.LATENCY_SIGNATURES for t in engine._TABLES + (engine.COMPENSATION_SIGNATURES,))
    i, vp = ctypes.c_int32, ctypes.c_void_p
    lib = engine.load_library()
    for name, sig in engine.LATENCY_SIGNATURES.items():
        assert list(sig) == _prototype(name) and len({n for n, _ in sig}) == len(sig), name
        assert getattr(lib, name).restype is ctypes.c_int and name in engine._EXPORTS and callable(engine.caller(name))
        with pytest.raises(TypeError, match=name):
            engine.call(name, device=0)
    assert list(lib.mpc_delay_scene.argtypes) == [i] * 5 + [vp] * 8 + [vp]
    assert list(lib.mpc_compensate_stale.argtypes) == [i, i, i, i, ctypes.POINTER(engine.CompensatorParams), i] + [vp] * 11 + [vp]
    stale, plain = engine.LATENCY_SIGNATURES["mpc_compensate_stale"], engine.COMPENSATION_SIGNATURES["mpc_compensate"]
    assert [p for p in stale if p != ("latency", "i32")] == list(plain) and engine.ABI_VERSION == 8


# ---- the evaluator ------------------------------------------------------------------------------------------------------------------

from test_actuator_cpu import _evaluate, _same_results                       # noqa: E402  (the PPOAgent run of that module)


@pytest.fixture(scope="module")
def plain():
    return _evaluate()


def test_evaluate_agent_with_latency_zero_is_the_run_without_the_stage(plain):
    none = _evaluate(latency=None)
    _same_results(plain, none)
    assert none.latency is None and not any(k.startswith("sense_") for k in none.summary())
    frames = []
    zero = _evaluate(latency=0, on_step=lambda d: frames.append({k: d[k].clone() for k in ("seen", "obs", "stale")}))
    _same_results(plain, zero)
    assert zero.latency["frames"] > 0 and zero.latency["stale_mean"] == 0.0 == zero.latency["ego_lag_max"]
    assert all(f["seen"].numpy().tobytes() == f["obs"].numpy().tobytes() and not f["stale"].any() for f in frames)
    assert zero.traces.seen is not None                      # `seen` is recorded with a latency model alone
    given = evaluate.Latency(8, "cpu", "torch", steps=0)
    _same_results(plain, _evaluate(latency=given))
    assert given.age.max() > 0
    _same_results(plain, _evaluate(latency=dict(steps=0)))


def test_latency_two_changes_what_the_agent_sees_and_nothing_the_records_read(plain):
    frames = []
    res = _evaluate(latency=2, on_step=lambda d: frames.append({k: d[k].clone() for k in ("seen", "obs", "stale", "done")
                                                                if k in d}))
    s = res.summary()
    print("latency totals:", res.latency)
    assert res.latency["frames"] == 8 * len(frames) and 1.0 < s["sense_stale_mean"] < 2.0
    assert 0.0 < s["sense_ego_lag_mean"] <= s["sense_ego_lag_max"] == res.latency["ego_lag_max"]
    seen_old = 0
    for k, f in enumerate(frames):                           # seen is the TRUE observation of stale steps ago, env by env
        for b in range(8):
            old = int(f["stale"][b])
            assert f["seen"][b].numpy().tobytes() == frames[k - old]["obs"][b].numpy().tobytes(), (k, b)
            seen_old += old > 0
    assert seen_old > 0 and max(int(f["stale"].max()) for f in frames) == 2
    ends = [k for k, f in enumerate(frames) if "done" in f and f["done"][0]]
    assert ends and int(frames[ends[0]]["stale"][0]) == 0    # a new episode starts on its own first scene
    tr = res.traces                                          # the recorder: `scene` the true scenes, `seen` two steps behind
    assert len(tr) > 0 and res.records["return"].tobytes() != plain.records["return"].tobytes()
    for i in range(len(tr)):
        e = tr.episode(i)
        for k in range(len(e["action"])):
            j = k - min(2, e["first"] + k)
            if j >= 0:
                assert e["seen"][k].tobytes() == e["scene"][j].tobytes(), (i, k)


def test_a_matching_compensator_predicts_the_ego_through_latency_and_delay():
    """the issue's closed-loop case: delay 2 with a steering lag, latency 2, the matching compensator, IDM traffic.  The bar is
    tests/test_compensate_cpu.py's: comp_pos_err_max <= 1e-3 m.  A compensator that knows the delay and not the latency misses
    it by far."""
    act = dict(delay=2, tau=(0.0, 0.2), limits="env")
    frames = []
    good = _evaluate(actuation=dict(act), latency=2, compensation=True,
                     on_step=lambda d: frames.append({k: d[k].clone() for k in ("seen", "ahead", "obs")}))
    s = good.summary()
    print("matching, latency 2 + delay 2:", good.compensation, good.latency)
    assert good.compensation["scored"] > 0 and s["comp_pos_err_max"] == good.compensation["pos_err_max"] <= 1e-3
    assert 0.0 < s["comp_pos_err_mean"] <= s["comp_pos_err_max"] and s["sense_stale_mean"] > 1.0
    assert all(f["seen"].numpy().tobytes() == f["ahead"].numpy().tobytes() for f in frames)
    blind = _evaluate(actuation=dict(act), latency=2, compensation=dict(steps=2, tau=(0.0, 0.2), limits="env"))
    print("blind to the latency:", blind.compensation)
    assert blind.compensation["pos_err_max"] > 1e-2
    alone = _evaluate(latency=3, compensation=True)          # no actuator model: the latency alone is matched
    print("latency 3 alone:", alone.compensation)
    assert alone.compensation["scored"] > 0 and alone.compensation["pos_err_max"] <= 1e-3


def test_evaluate_agent_refuses_what_a_latency_cannot_serve():
    import policy_ref as pr
    agent = rollout.PPOAgent(pr.make_policy(64, 2, -0.5, use_sde=False, seed=8))
    env = lambda: rollout.SyntheticIntersectionEnv(4, device="cpu", seed=3, n_others=4, backend="torch")
    run = lambda a=agent, **kw: evaluate.evaluate_agent(a, env(), use_graph=False, **kw)
    with pytest.raises(ValueError, match="actuator model or a latency model"):
        run(compensation=True)
    with pytest.raises(ValueError, match="latency"):
        run(latency=evaluate.Latency(3, "cpu", "torch"))
    with pytest.raises(ValueError, match="latency"):
        run(latency=evaluate.Latency(4, "cpu", "torch", R=9))
    with pytest.raises(ValueError, match="latency"):
        run(latency="2")
    with pytest.raises(ValueError):
        run(latency=8)
    with pytest.raises(ValueError):
        run(latency=4, actuation=dict(delay=4), compensation=True)

    class Planner:                                           # an agent with a plan, as far as the argument checks look
        HAS_PLAN, engine = True, type("E", (), dict(horizon=20))()

        def act_batch_torch(self, obs, plan=False, **kw):
            raise AssertionError("not reached")
    for kw in (dict(plan=True), dict(trace=dict(plan=True))):
        with pytest.raises(ValueError, match="latency of steps > 0"):
            run(Planner(), latency=1, **kw)
    assert run(latency=1, trace=dict(seen=True)).traces.seen is not None


def test_compare_gives_every_agent_a_fresh_latency_model():
    import policy_ref as pr
    agent = lambda: rollout.PPOAgent(pr.make_policy(64, 2, -0.5, use_sde=False, seed=9))
    make_env = lambda: rollout.SyntheticIntersectionEnv(4, device="cpu", seed=2, n_others=4, backend="torch")
    results = {}
    out = evaluate.compare({"a": agent(), "b": agent()}, make_env, 1, actuation=dict(delay=1), latency=2, compensation=True,
                           results=results, use_graph=False)
    assert results["a"].latency == results["b"].latency and results["a"].latency["frames"] > 0          # not accumulated
    assert out["a"]["comp_pos_err_max"] == out["b"]["comp_pos_err_max"] <= 1e-3 and out["a"]["sense_stale_mean"] > 1.0
    inst = evaluate.Latency(4, "cpu", "torch", steps=2)
    out2 = evaluate.compare({"a": agent()}, make_env, 1, actuation=dict(delay=1), latency=inst, compensation=True, use_graph=False)
    assert out2["a"]["sense_ego_lag_max"] == out["a"]["sense_ego_lag_max"] and inst.totals()["frames"] == 0       # a copy ran
    assert "sense_stale_mean" not in evaluate.compare({"a": agent()}, make_env, 1, use_graph=False)["a"]


# ---- sanitizers: a stand-alone program, nothing loaded into Python -----------------------------------------------------------------

def test_host_builds_run_clean_under_address_and_undefined_behaviour_sanitizers():
    out = os.path.join(conftest.ROOT, "tests", "_build", "latency_san_main")
    src = os.path.join(conftest.ROOT, "tests", "latency_san_main.cpp")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in [src] + lh.DEPS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                        "-static-libubsan", "-std=c++17", "-Wno-unknown-pragmas", "-ffp-contract=off", "-o", out, src],
                       check=True)
    res = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "latency_san_main: ok" in res.stdout, res.stdout + res.stderr
