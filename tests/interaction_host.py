"""TEST INFRASTRUCTURE - the interaction metrics of csrc/mpc_interaction.hpp compiled for the host
(tests/cpu_interaction_harness.cpp) behind a numpy wrapper with the layout of evaluate.InteractionMetrics, a plain-Python
restatement (`replay`) written from the header's comment, loops and floats only, and the streams of states the CPU and the
GPU tests share: random ones, closed loops of the host IDM environment (tests/cpu_traffic_env_harness.cpp), hand-built
scenarios."""
import ctypes
import glob
import math
import os
import subprocess

import numpy as np

import conftest

_libs = {}
INF = float("inf")
DT = 0.1
ARRAYS = ("ego", "opos", "ospeed", "ohead", "oactive", "oroute", "oprog", "otarget")
DTYPES = dict(ego=np.float64, opos=np.float64, ospeed=np.float64, ohead=np.float64, oactive=np.uint8, oroute=np.int32,
              oprog=np.float64, otarget=np.float64)
PLANES = ("state_i32", "state_f64", "rec_i32", "rec_f64")
ROUTES, SLOTS = 12, 9
DEPS = glob.glob(os.path.join(conftest.ROOT, "mpc-rl_for_avs_amd", "csrc", "*.hpp"))
STRAIGHT_REF = np.array([[2.0, 50.0], [2.0, -50.0]])


def _build(name):
    if name not in _libs:
        out = os.path.join(conftest.BUILD_DIR, f"libcpu_{name}.so")
        src = os.path.join(conftest.ROOT, "tests", f"cpu_{name}_harness.cpp")
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in [src] + DEPS):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            subprocess.run(["g++"] + conftest.HOST_CXXFLAGS + ["-o", out, src], check=True)
        _libs[name] = ctypes.CDLL(out)
    return _libs[name]


def load():
    lib = _build("interaction")
    lib.interaction_step.argtypes = [ctypes.c_int] * 5 + [ctypes.c_double] + [ctypes.c_void_p] * 18
    lib.interaction_step.restype = ctypes.c_int
    lib.interaction_sigma.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_void_p, ctypes.c_int]
    lib.interaction_sigma.restype = ctypes.c_double
    return lib


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def host_pose(route, s):
    """mpc::env::pose of the host build: x, y, heading"""
    lib = _build("traffic_env")
    r, s = np.asarray([route], np.int32), np.asarray([s], np.float64)
    x, y, h = np.zeros(1), np.zeros(1), np.zeros(1)
    lib.traffic_pose(1, _p(r), _p(s), _p(x), _p(y), _p(h))
    return float(x[0]), float(y[0]), float(h[0])


def host_sigma(x, y, ref_xy):
    ref = np.ascontiguousarray(ref_xy, np.float64)
    return load().interaction_sigma(x, y, _p(ref), ref.shape[0])


def state_of(s):
    """the eight arrays of a state, contiguous in the entry point's types"""
    return {k: np.ascontiguousarray(s[k], DTYPES[k]) for k in ARRAYS}


class HostInteraction:
    """The kernel's state and records as numpy arrays (the layout of include/mpc_mi355x.h), stepped by the host build;
    leader / accel [B, K]: part (a) of the last state; margin: the smallest distance of a compared quantity from its
    threshold over all updates so far."""

    def __init__(self, B, Q, K, ref_xy, conflict, dt=DT):
        self.B, self.Q, self.K, self.dt = B, Q, K, float(dt)
        self.ref_xy = np.ascontiguousarray(ref_xy, np.float64)
        self.conflict = np.ascontiguousarray(conflict, np.float64)
        self.state_i32 = np.zeros((9 + SLOTS, B), np.int32)
        self.state_f64 = np.zeros((4 + ROUTES + 2 * SLOTS, B), np.float64)
        self.rec_i32 = np.zeros((7, B, Q), np.int32)
        self.rec_f64 = np.zeros((3, B, Q), np.float64)
        self.leader, self.accel = np.zeros((B, K), np.int32), np.zeros((B, K))
        self.margin = np.full(1, INF)

    def update(self, s, reset=False):
        a = state_of(s)
        done = None if reset else np.ascontiguousarray(s["done"], np.uint8)
        rc = load().interaction_step(self.B, self.K, self.Q, self.ref_xy.shape[0], 1 if reset else 0, self.dt,
                                     *[_p(a[k]) for k in ARRAYS], _p(done), _p(self.ref_xy), _p(self.conflict),
                                     _p(self.state_i32), _p(self.state_f64), _p(self.rec_i32), _p(self.rec_f64),
                                     _p(self.leader), _p(self.accel), _p(self.margin))
        assert rc == 0

    def planes(self):
        return {n: getattr(self, n) for n in PLANES}

    def records(self):
        from mpc_rl_for_avs_amd.evaluate import INTERACT_F64, INTERACT_I32, records_from_planes
        return records_from_planes(self.rec_i32, self.rec_f64, INTERACT_I32, INTERACT_F64)


def run_host(states, B, Q, K, ref_xy, conflict):
    h = HostInteraction(B, Q, K, ref_xy, conflict)
    for s in states:
        h.update(s, reset=bool(s.get("reset")))
    return h


def assert_planes_close(got, want, what, atol):
    """integers equal, f64 to atol (infinities and the -1 of an unset pass time in the same places)"""
    for n in PLANES:
        g, w = np.asarray(got[n]), np.asarray(want[n])
        assert g.shape == w.shape, (what, n)
        if g.dtype.kind == "i":
            assert np.array_equal(g, w), (what, n, np.argwhere(g != w)[:5])
        else:
            assert np.array_equal(np.isfinite(g), np.isfinite(w)) and np.array_equal(g[~np.isfinite(g)], w[~np.isfinite(w)]), \
                (what, n)
            f = np.isfinite(g)
            assert np.abs(g[f] - w[f]).max(initial=0.0) <= atol, (what, n, np.abs(g[f] - w[f]).max())


# ---- streams of states ---------------------------------------------------------------------------------------------------

def random_stream(seed, B, K, T, ref_xy, done_at=(), reset_at=()):
    """T states after a reset.  The ego moves along its polyline with noise, each vehicle along a route; with some
    probability a slot is emptied or refilled (another vehicle: identity must break), so that passes of both kinds, yielding
    and hard braking all occur.  done on the steps of `done_at` for every other environment (offset by the step), plus a few
    at random; a reset launch before the steps of `reset_at`."""
    rng = np.random.default_rng(seed)
    ref = np.asarray(ref_xy, np.float64)
    seg = np.diff(ref, axis=0) if ref.shape[0] > 1 else np.zeros((1, 2))
    cum = np.concatenate([[0.0], np.cumsum(np.hypot(seg[:, 0], seg[:, 1]))])

    def along(sig):
        i = int(np.clip(np.searchsorted(cum, sig, side="right") - 1, 0, max(len(cum) - 2, 0)))
        L = cum[i + 1] - cum[i] if len(cum) > 1 else 0.0
        t = (sig - cum[i]) / L if L > 0 else 0.0
        d = seg[i] / L if L > 0 else np.array([0.0, -1.0])
        return ref[i] + t * seg[i], math.atan2(d[1], d[0])

    sig = rng.uniform(30.0, 46.0, B)
    route = rng.integers(0, 12, (B, K)).astype(np.int32)
    prog = rng.uniform(45.0, 60.0, (B, K))
    active = rng.uniform(size=(B, K)) < 0.8
    speed, target = rng.uniform(0.0, 12.0, (B, K)), rng.uniform(4.0, 12.0, (B, K))
    out = []
    for n in range(T + 1):
        done = np.zeros(B, np.uint8)
        if n > 0:
            done = (rng.uniform(size=B) < 0.015).astype(np.uint8)
            if n in done_at:
                done[(np.arange(B) + n) % 2 == 0] = 1
            sig = np.where(done != 0, rng.uniform(30.0, 46.0, B), sig + rng.uniform(-0.2, 1.6, B))
            swap = (rng.uniform(size=(B, K)) < 0.04) | (done != 0)[:, None]
            back = rng.uniform(size=(B, K)) < 0.03                # the same slot and route, further back: another vehicle
            prog = np.where(back, prog - rng.uniform(5.0, 30.0, (B, K)), prog + speed * DT * rng.uniform(0.0, 3.0, (B, K)))
            route = np.where(swap, rng.integers(0, 12, (B, K)), route).astype(np.int32)
            prog = np.where(swap, rng.uniform(45.0, 60.0, (B, K)), prog)
            active = np.where(swap, rng.uniform(size=(B, K)) < 0.8, active)
            speed = np.clip(speed + rng.uniform(-1.0, 1.0, (B, K)), 0.0, 14.0)
        ego, opos, ohead = np.zeros((B, 4)), np.zeros((B, K, 2)), np.zeros((B, K))
        for b in range(B):
            p, h = along(sig[b])
            off = rng.uniform(-0.8, 0.8)
            ego[b] = (p[0] - off * math.sin(h), p[1] + off * math.cos(h), h + rng.uniform(-0.1, 0.1), rng.uniform(0.0, 12.0))
            for j in range(K):
                x, y, hh = host_pose(int(route[b, j]), float(prog[b, j]))
                opos[b, j], ohead[b, j] = (x, y), hh
        s = dict(ego=ego, opos=opos, ospeed=speed.copy(), ohead=ohead, oactive=active.astype(np.uint8), oroute=route.copy(),
                 oprog=prog.copy(), otarget=target.copy(), done=done)
        if n == 0 or n in reset_at:
            s["reset"] = True
        out.append(s)
    return out


def closed_loop(seed, B=6, K=9, T=60):
    """T steps of the host IDM environment under a controller that keeps 8 m/s and steers to the route's heading: the states
    after the reset and after every step (with its `done`), and per state the environment's own leader / acceleration
    diagnostics of the step that FOLLOWS it (step_env_idm decides from the state before the step); None for the last."""
    from test_traffic_env_cpu import TrafficHostEnv, load_traffic_lib
    from mpc_rl_for_avs_amd.reference_path import reference_states
    ref = reference_states(DT)
    env = TrafficHostEnv(load_traffic_lib(), B, K, seed=seed)
    env.reset()
    snap = lambda done: dict({k: v.copy() for k, v in state_of({k: getattr(env, k) for k in ARRAYS}).items()}, done=done)
    states, decided = [dict(snap(np.zeros(B, np.uint8)), reset=True)], []
    for _ in range(T):
        d = ref[None, :, :2] - env.ego[:, None, :2]
        idx = np.minimum(np.argmin((d * d).sum(axis=2), axis=1) + 3, ref.shape[0] - 1)
        err = ref[idx, 3] - env.ego[:, 2]
        err = (err + math.pi) % (2 * math.pi) - math.pi
        action = np.stack([np.clip(8.0 - env.ego[:, 3], -5.0, 2.0), np.clip(2.0 * err, -0.6, 0.6)], axis=1)
        _, _, done = env.step(action)
        decided.append((env.leader.copy(), env.accel.copy()))
        states.append(snap(done.astype(np.uint8)))
    return states, decided + [None]


def one_vehicle_state(ego, route, prog, speed=8.0, target=8.0, active=True, done=0, reset=False):
    """B = 1, K = 1: the ego (x, y, heading, speed) and one vehicle at arc length `prog` of `route`"""
    x, y, h = host_pose(route, prog)
    s = dict(ego=np.array([ego], np.float64), opos=np.array([[[x, y]]]), ospeed=np.array([[speed]]), ohead=np.array([[h]]),
             oactive=np.array([[1 if active else 0]], np.uint8), oroute=np.array([[route]], np.int32),
             oprog=np.array([[float(prog)]]), otarget=np.array([[target]]), done=np.array([done], np.uint8))
    if reset:
        s["reset"] = True
    return s


# ---- the plain-Python restatement -----------------------------------------------------------------------------------------

def _wrap(a):
    if a > math.pi:
        a = a - 2.0 * math.pi
    if a <= -math.pi:
        a = a + 2.0 * math.pi
    return a


NOBODY = (INF, 0.0, 0.0, -2)             # ell, heading, speed, who


def _offer(best, j, xj, yj, hj, cj, sj, c, cx, cy, ch, cv):
    ex = cx - xj
    ey = cy - yj
    m0 = ex * cj
    m1 = ey * sj
    ell = m0 + m1
    m2 = ey * cj
    m3 = ex * sj
    w = m2 - m3
    inside = ell > 0.0 and ell <= 40.0 and abs(w) <= 2.0
    counts = c < 0 or (ell > 5.0 and (c < j or abs(_wrap(ch - hj)) < math.pi / 4))
    if inside and counts and ell < best[0]:
        return (ell, ch, cv, c)
    return best


def _idm(v, v0, hj, lead):
    r = v / v0
    r2 = r * r
    interaction = 0.0
    if lead[3] != -2:
        gap = lead[0] - 5.0
        if gap < 0.1:
            gap = 0.1
        proj = lead[2] * math.cos(lead[1] - hj)
        dv = v - proj
        t0 = v * 1.5
        t1 = v * dv
        t2 = t1 / 7.745966692414834
        dyn = t0 + t2
        if dyn < 0.0:
            dyn = 0.0
        q = (5.0 + dyn) / gap
        interaction = q * q
    r4 = r2 * r2
    a = 1.0 - r4
    a = a - interaction
    a = 3.0 * a
    return -6.0 if a < -6.0 else (3.0 if a > 3.0 else a)


def _drives_free(j, K, first, who):
    p, lowest, closed = first, j, False
    for _ in range(K):
        if p < 0 or closed:
            continue
        if p == j:
            closed = True
            continue
        lowest = min(lowest, p)
        p = who[p]
    return closed and lowest == j


def sigma_of(x, y, ref):
    M = len(ref)
    best, idx = INF, 0
    for i in range(max(M - 1, 1)):
        i1 = min(i + 1, M - 1)
        dx = ref[i1][0] - ref[i][0]
        dy = ref[i1][1] - ref[i][1]
        sx = x - ref[i][0]
        sy = y - ref[i][1]
        dd = dx * dx + dy * dy
        t = 0.0
        if dd > 0.0:
            t = (sx * dx + sy * dy) / dd
            t = min(max(t, 0.0), 1.0)
        cx = sx - t * dx
        cy = sy - t * dy
        d2 = cx * cx + cy * cy
        if d2 < best:
            best, idx, t_best, dd_best = d2, i, t, dd
    before = 0.0
    for i in range(idx):
        dx = ref[i + 1][0] - ref[i][0]
        dy = ref[i + 1][1] - ref[i][1]
        before = before + math.sqrt(dx * dx + dy * dy)
    return before + t_best * math.sqrt(dd_best)


def replay(states, B, Q, K, ref_xy, conflict, dt=DT):
    """The interaction metrics of each environment on its own, as plain Python.  Returns the four planes."""
    ref = [[float(v) for v in p] for p in np.asarray(ref_xy)]
    conflict = [[float(v) for v in p] for p in np.asarray(conflict)]
    rec_i, rec_f = np.zeros((7, B, Q), np.int32), np.zeros((3, B, Q))
    st_i, st_f = np.zeros((9 + SLOTS, B), np.int32), np.zeros((4 + ROUTES + 2 * SLOTS, B))
    for b in range(B):
        fresh_counts = lambda: dict(steps=0, yields=0, forced=0, events=0, conflicts=0, critical=0, first=0, prev=0, dec=0.0,
                                    deficit=0.0, pet=INF)
        e, ordinal = fresh_counts(), 0
        te, tv, croute, cprog, csigma = [-1.0] * ROUTES, [-1.0] * SLOTS, [-1] * SLOTS, [0.0] * SLOTS, 0.0
        for s in states:
            if s.get("reset"):
                fresh, ordinal = True, 0
            else:
                fresh = bool(s["done"][b])
                if fresh and ordinal < Q:
                    rec_i[:, b, ordinal] = (e["steps"], e["yields"], e["forced"], e["events"], e["conflicts"], e["critical"],
                                            e["first"])
                    rec_f[:, b, ordinal] = (e["dec"], e["deficit"], e["pet"])
                    ordinal += 1
            if fresh:
                e = fresh_counts()
                te, tv, croute = [-1.0] * ROUTES, [-1.0] * SLOTS, [-1] * SLOTS
            n = e["steps"]
            x, y, th, sp = (float(v) for v in s["ego"][b])
            act = [bool(s["oactive"][b][j]) for j in range(K)]
            pos = [(float(s["opos"][b][j][0]), float(s["opos"][b][j][1])) for j in range(K)]
            head = [float(s["ohead"][b][j]) for j in range(K)]
            spd = [float(s["ospeed"][b][j]) for j in range(K)]
            # (a)
            lead, alt, who = [NOBODY] * K, [NOBODY] * K, [-2] * K
            for j in range(K):
                if not act[j]:
                    continue
                cj, sj = math.cos(head[j]), math.sin(head[j])
                lead[j] = _offer(lead[j], j, pos[j][0], pos[j][1], head[j], cj, sj, -1, x, y, th, sp)
                for k in range(K):
                    if k != j and act[k]:
                        cand = (j, pos[j][0], pos[j][1], head[j], cj, sj, k, pos[k][0], pos[k][1], head[k], spd[k])
                        lead[j] = _offer(lead[j], *cand)
                        alt[j] = _offer(alt[j], *cand)
                who[j] = lead[j][3]
            n_yield, mask, forced, imposed_sum = 0, 0, 0.0, 0.0
            for j in range(K):
                if not act[j]:
                    continue
                v0 = float(s["otarget"][b][j])
                if _drives_free(j, K, who[j], who):
                    lead[j] = NOBODY
                a_with = _idm(spd[j], v0, head[j], lead[j])
                if lead[j][3] != -1:
                    continue
                if _drives_free(j, K, alt[j][3], who):
                    alt[j] = NOBODY
                a_free = _idm(spd[j], v0, head[j], alt[j])
                n_yield += 1
                if -a_with > forced:
                    forced = -a_with
                if a_with < -3.0:
                    mask |= 1 << j
                imposed_sum = imposed_sum + (a_free - a_with)
            # (b)
            sigma = sigma_of(x, y, ref)
            te_new = [False] * ROUTES
            for r in range(ROUTES):
                c = conflict[r][0]
                if n >= 1 and c >= 0.0 and te[r] < 0.0 and csigma < c and c <= sigma:
                    te[r] = float(n - 1) + (c - csigma) / (sigma - csigma)
                    te_new[r] = True
            for j in range(SLOTS):
                route = int(s["oroute"][b][j]) if j < K and act[j] else -1
                if not 0 <= route < ROUTES:
                    route = -1
                prog = float(s["oprog"][b][j]) if route >= 0 else 0.0
                same = (not fresh) and n >= 1 and route >= 0 and croute[j] == route and prog >= cprog[j]
                tv_new = False
                if not same:
                    tv[j] = -1.0
                elif conflict[route][0] >= 0.0 and tv[j] < 0.0 and cprog[j] < conflict[route][1] and conflict[route][1] <= prog:
                    tv[j] = float(n - 1) + (conflict[route][1] - cprog[j]) / (prog - cprog[j])
                    tv_new = True
                if route >= 0 and te[route] >= 0.0 and tv[j] >= 0.0 and (te_new[route] or tv_new):
                    pet = abs(te[route] - tv[j]) * dt
                    e["conflicts"] += 1
                    e["critical"] += 1 if pet < 1.5 else 0
                    e["first"] += 1 if te[route] < tv[j] else 0
                    e["pet"] = min(e["pet"], pet)
                croute[j], cprog[j] = route, prog
            e["steps"] += 1
            e["yields"] += 1 if n_yield > 0 else 0
            e["forced"] += 1 if mask != 0 else 0
            e["events"] += bin(mask & ~e["prev"]).count("1")
            e["prev"] = mask
            e["dec"] = max(e["dec"], forced)
            e["deficit"] = e["deficit"] + imposed_sum * dt
            csigma = sigma
        st_i[:9, b] = (e["steps"], e["yields"], e["forced"], e["events"], e["conflicts"], e["critical"], e["first"], ordinal,
                       e["prev"])
        st_i[9:, b] = croute
        st_f[:4, b] = (e["dec"], e["deficit"], e["pet"], csigma)
        st_f[4:4 + ROUTES, b], st_f[4 + ROUTES:4 + ROUTES + SLOTS, b], st_f[4 + ROUTES + SLOTS:, b] = te, tv, cprog
    return dict(state_i32=st_i, state_f64=st_f, rec_i32=rec_i, rec_f64=rec_f)
