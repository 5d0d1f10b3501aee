"""TEST INFRASTRUCTURE - the build of csrc/mpc_compensate.hpp that knows of a sensing latency (compensate_env<true>,
tests/cpu_latency_harness.cpp) behind a numpy wrapper with the layout of evaluate.Compensation, and a plain-Python restatement
(`compensate`, `replay`) of the update with a latency to check it against, in the manner of tests/compensate_host.py, whose
`shape`, `plant` and `fresh` it uses: Python floats and ints only, f32 roundings through numpy scalars, one operation per
statement."""
import math

import numpy as np

import compensate_host as ch
import latency_host as lh

F32 = np.float32
DEFAULTS = dict(ch.DEFAULTS, latency=0)


def settings(**params):
    q = dict(DEFAULTS)
    q.update(params)
    return q


class HostStaleCompensator(ch.HostCompensator):
    """compensate_host.HostCompensator stepped by the latency-aware host build; `latency` among the parameters."""

    def __init__(self, B, R, **params):
        super().__init__(B, R)
        self.params = settings(**params)

    def step(self, obs, command=None, done=None, reset=False, out=None, pred=True, missing=()):
        q = self.params
        par = np.array([q["dt"], *q["alpha"], *q["rate"], *q["lo"], *q["hi"]], np.float64)
        assert obs.dtype == F32 and obs.shape[1:] == (self.R, 8) and obs.flags.c_contiguous
        if command is not None:
            assert command.dtype == np.float64 and command.shape == (self.B, 2) and command.flags.c_contiguous
        done = None if done is None else np.ascontiguousarray(done, np.uint8)
        out = np.full(obs.shape, np.nan, F32) if out is None else out
        pred = np.full((obs.shape[0], 4), np.nan) if pred else None
        bufs = dict(obs=obs, command=command, done=done, out=out, pred=pred, ring=self.ring, prev=self.prev, age=self.age,
                    pring=self.pring, counts=self.counts, sums=self.sums)
        bufs.update({k: None for k in missing})
        rc = lh.load().compensate_stale_step(
            self.B, self.R, 1 if reset else 0, lh._p(par), q["steps"], q["latency"],
            *[lh._p(bufs[k]) for k in ("obs", "command", "done", "out", "pred", "ring", "prev", "age", "pring", "counts", "sums")])
        return rc, out, pred


def compensate(s, obs, command, q, clear, reset):
    """One environment, one launch of the update with d = steps and L = latency.  s: its state (compensate_host.fresh, changed
    in place); obs [R, 8] f32; command: two Python floats or None -> (out [R, 8] f32, pred [4])."""
    R, d, L, dt = obs.shape[0], q["steps"], q["latency"], q["dt"]
    back = d + L
    if clear:                                                                  # 1
        s["age"] = 0
        s["ring"] = [[0.0, 0.0] for _ in range(8)]
        s["pring"] = [[0.0, 0.0] for _ in range(8)]
        s["prev"] = [0.0, 0.0]
        if reset:
            s["count"], s["sum"], s["top"] = 0, 0.0, 0.0
    else:                                                                      # 2
        age0 = s["age"]
        for c in range(2):
            u = command[c]
            if not (u - u == 0.0):
                u = 0.0
            s["ring"][age0 & 7][c] = u
            if age0 >= L:                                                      # the scene advanced: so does prev
                j = age0 - L - d
                delayed = s["ring"][j & 7][c] if j >= 0 else 0.0
                s["prev"][c] = ch.shape(q, c, delayed, s["prev"][c])
        s["age"] = age0 + 1
    age = s["age"]
    x0, y0 = float(obs[0, 1]), float(obs[0, 2])
    if back > 0 and age >= back:                                               # 3
        px, py = s["pring"][(age - back) & 7]
        dx = px - x0
        dy = py - y0
        a = dx * dx
        b = dy * dy
        e = math.sqrt(a + b)
        s["count"] += 1
        s["sum"] = s["sum"] + e
        if e > s["top"]:
            s["top"] = e
    old = L if L < age else age                                                # s of the header
    ahead = d + old
    vx, vy = float(obs[0, 3]), float(obs[0, 4])                                # 4
    a = vx * vx
    b = vy * vy
    x, y, th, sp = x0, y0, float(obs[0, 5]), math.sqrt(a + b)
    p = list(s["prev"])
    for k in range(ahead):
        i = age - old - d + k
        for c in range(2):
            p[c] = ch.shape(q, c, s["ring"][i & 7][c] if i >= 0 else 0.0, p[c])
        x, y, th, sp = ch.plant(x, y, th, sp, p[0], p[1], dt)
    s["pring"][age & 7] = [x, y]
    pred = [x, y, th, sp]
    if back == 0:                                                              # 8
        return obs.copy(), pred
    out = np.zeros((R, 8), F32)
    sn, cs = math.sin(th), math.cos(th)                                        # 5
    out[0] = [F32(1.0), F32(x), F32(y), F32(sp * cs), F32(sp * sn), F32(th), F32(sn), F32(cs)]
    h = float(ahead) * dt                                                      # 6
    ex, ey = float(out[0, 1]), float(out[0, 2])
    moved = []
    for i in range(1, R):
        if obs[i, 0] == 0.0:
            continue
        sx = float(obs[i, 3]) * h
        nx = F32(float(obs[i, 1]) + sx)
        sy = float(obs[i, 4]) * h
        ny = F32(float(obs[i, 2]) + sy)
        kx = float(nx) - ex                                                    # 7
        ky = float(ny) - ey
        a = kx * kx
        b = ky * ky
        moved.append((a + b, i, [F32(1.0), nx, ny] + list(obs[i, 3:])))
    moved.sort(key=lambda m: (m[0], m[1]))                                     # by key, ties to the lower input row
    for rank, m in enumerate(moved):
        out[1 + rank] = m[2]
    return out, pred


def replay(launches, B, R, **params):
    """compensate_host.replay with a latency among the parameters"""
    q = settings(**params)
    envs = [ch.fresh() for _ in range(B)]
    outs, preds = [], []
    for s in launches:
        reset, done = bool(s.get("reset")), s.get("done")
        out, pred = np.zeros((B, R, 8), F32), np.zeros((B, 4))
        for b in range(B):
            clear = reset or (done is not None and bool(done[b]))
            cmd = None if clear else [float(v) for v in s["command"][b]]
            out[b], pred[b] = compensate(envs[b], s["obs"][b], cmd, q, clear, reset)
        outs.append(out)
        preds.append(pred)
    ring, pring = np.zeros((8, B, 2)), np.zeros((8, B, 2))
    for b, e in enumerate(envs):
        ring[:, b], pring[:, b] = e["ring"], e["pring"]
    return (outs, preds, ring, np.array([e["prev"] for e in envs], np.float64).reshape(B, 2),
            np.array([e["age"] for e in envs], np.int32), pring, np.array([e["count"] for e in envs], np.int64),
            np.array([[e["sum"] for e in envs], [e["top"] for e in envs]], np.float64).reshape(2, B))
