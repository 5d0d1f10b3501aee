"""TEST INFRASTRUCTURE - the perception model of csrc/mpc_perception.hpp compiled for the host
(tests/cpu_perception_harness.cpp) behind a numpy wrapper with the layout of evaluate.Perception, and a plain-Python
restatement (`perceive`, `replay`) of the model to check both against: Python floats and ints only, one operation per
statement, so that nothing can be contracted or reassociated."""
import ctypes
import math
import os
import struct
import subprocess

import numpy as np

import conftest

_lib = None
INF = float("inf")
M64 = (1 << 64) - 1
SALT = 0xC2B2AE3D27D4EB4F
ABSENT, SEEN, OUT_OF_RANGE, OCCLUDED, DROPPED = 0, 1, 2, 3, 4
COUNTS = ("present", "seen", "out_of_range", "occluded", "dropped")
OFF = dict(range=INF, occlusion=False, min_points=1, p_drop=0.0, sigma_pos=0.0, sigma_vel=0.0, sigma_head=0.0, seed=0,
           env_offset=0)
SRC = os.path.join(conftest.ROOT, "tests", "cpu_perception_harness.cpp")
DEPS = [SRC] + [os.path.join(conftest.ROOT, "mpc-rl_for_avs_amd", "csrc", f)
                for f in ("mpc_perception.hpp", "mpc_drive_metrics.hpp", "mpc_synth_env.hpp", "mpc_core.hpp")]


def load():
    global _lib
    if _lib is None:
        out = os.path.join(conftest.BUILD_DIR, "libcpu_perception.so")
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in DEPS):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            subprocess.run(["g++"] + conftest.HOST_CXXFLAGS + ["-o", out, SRC], check=True)
        _lib = ctypes.CDLL(out)
        i, d, vp = ctypes.c_int, ctypes.c_double, ctypes.c_void_p
        _lib.perception_step.argtypes = [i, i, i, i, d, i, i, d, d, d, d, ctypes.c_uint64, i] + [vp] * 6
        _lib.perception_step.restype = i
        _lib.perception_crosses.argtypes, _lib.perception_crosses.restype = [d] * 8, i
        _lib.perception_noise.argtypes = [ctypes.c_uint64, i, ctypes.c_int64, i, i, vp]
        _lib.perception_noise.restype = None
    return _lib


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def host_crosses(p, s, e0, e1):
    return bool(load().perception_crosses(p[0], p[1], s[0], s[1], e0[0], e0[1], e1[0], e1[1]))


def host_noise(seed, env, ctr, slot0, n):
    out = np.zeros(n)
    load().perception_noise(seed, env, ctr, slot0, n, _p(out))
    return out


class HostPerception:
    """The kernel's buffers as numpy arrays (the layout of include/mpc_mi355x.h), stepped by the host build."""

    def __init__(self, B, R, occluders=None, **params):
        self.B, self.R = B, R
        self.params = dict(OFF)
        self.params.update(params)
        self.occluders = np.zeros((0, 4, 2)) if occluders is None else np.ascontiguousarray(occluders, np.float64)
        self.row_class = np.zeros((B, R), np.uint8)
        self.counts = np.zeros((5, B), np.int64)
        self.ctr = np.zeros(B, np.int64)

    def apply(self, obs_true, reset=False, row_class=True, **override):
        obs_true = np.ascontiguousarray(obs_true, np.float32)
        assert obs_true.shape == (self.B, self.R, 8)
        out = np.full((self.B, self.R, 8), np.float32(np.nan))          # every element must be written
        q = dict(self.params)
        q.update(override)
        S = self.occluders.shape[0]
        rc = load().perception_step(self.B, self.R, S, 1 if reset else 0, q["range"], int(q["occlusion"]), q["min_points"],
                                    q["p_drop"], q["sigma_pos"], q["sigma_vel"], q["sigma_head"], q["seed"], q["env_offset"],
                                    _p(obs_true), _p(self.occluders) if S else None, _p(out),
                                    _p(self.row_class) if row_class else None, _p(self.counts), _p(self.ctr))
        assert rc == 0
        return out

    def totals(self):
        return {k: int(self.counts[i].sum()) for i, k in enumerate(COUNTS)}


# ---- the restatement: Python floats and ints ---------------------------------------------------------------------------------

def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def rng_key(seed, env, ctr):
    a = (mix64(seed ^ 0xA5A5A5A5) + (env & M64) * 0x100000001B3) & M64
    return mix64(a) ^ mix64(ctr & M64)


def u01(key, slot):
    bits = mix64((key + slot * 0xD1342543DE82EF95) & M64)
    return float(bits >> 11) * (1.0 / 9007199254740992.0)


def unit_noise(key, k):
    a = u01(key, k) + u01(key, k + 1)
    b = u01(key, k + 2) + u01(key, k + 3)
    c = a + b
    d = c - 2.0
    return d * 1.7320508075688772


def corners(px, py, hx, hy):
    """mpc::drive::corners: the 5.0 x 2.0 rectangle centred at p with axis h = (cos, sin)."""
    lx, ly = 2.5 * hx, 2.5 * hy
    wx, wy = 1.0 * -hy, 1.0 * hx
    fx, fy, bx, by = px + lx, py + ly, px - lx, py - ly
    return [(fx + wx, fy + wy), (bx + wx, by + wy), (bx - wx, by - wy), (fx - wx, fy - wy)]


def cross(ax, ay, bx, by):
    m, n = ax * by, ay * bx
    return m - n


def crosses(p, s, e0, e1):
    ex, ey = e1[0] - e0[0], e1[1] - e0[1]
    rx, ry = s[0] - p[0], s[1] - p[1]
    d1 = cross(ex, ey, p[0] - e0[0], p[1] - e0[1])
    d2 = cross(ex, ey, s[0] - e0[0], s[1] - e0[1])
    d3 = cross(rx, ry, e0[0] - p[0], e0[1] - p[1])
    d4 = cross(rx, ry, e1[0] - p[0], e1[1] - p[1])
    return ((d1 > 0 and d2 < 0) or (d1 < 0 and d2 > 0)) and ((d3 > 0 and d4 < 0) or (d3 < 0 and d4 > 0))


def perceive(rows, occluders, q, env, ctr):
    """One environment: rows = R lists of 8 Python floats (exact f32 values), occluders = list of 4-corner lists, q the
    parameters, env = env_offset + b -> (seen rows [R][8], classes [R], counts [5])."""
    R = len(rows)
    key = rng_key(q["seed"] ^ SALT, env, ctr)
    p = (rows[0][1], rows[0][2])
    rects = [None] + [corners(r[1], r[2], r[7], r[6]) for r in rows[1:]]
    classes, out = [SEEN], [list(rows[0])]
    for i in range(1, R):
        row = rows[i]
        if row[0] == 0.0:
            classes.append(ABSENT)
            continue
        rx, ry = row[1] - p[0], row[2] - p[1]
        a, b = rx * rx, ry * ry
        if a + b > q["range"] * q["range"]:
            classes.append(OUT_OF_RANGE)
            continue
        if q["occlusion"]:
            quads = [rects[j] for j in range(1, R) if j != i and rows[j][0] != 0.0] + [list(o) for o in occluders]
            visible = 0
            for s in [(row[1], row[2])] + rects[i]:
                hidden = any(crosses(p, s, quad[k], quad[(k + 1) % 4]) for quad in quads for k in range(4))
                visible += 0 if hidden else 1
            if visible < q["min_points"]:
                classes.append(OCCLUDED)
                continue
        if u01(key, 32 * i) < q["p_drop"]:
            classes.append(DROPPED)
            continue
        classes.append(SEEN)
        o, k = list(row), 32 * i
        if q["sigma_pos"] != 0.0:
            o[1] = f32(row[1] + q["sigma_pos"] * unit_noise(key, k + 1))
            o[2] = f32(row[2] + q["sigma_pos"] * unit_noise(key, k + 5))
        if q["sigma_vel"] != 0.0:
            o[3] = f32(row[3] + q["sigma_vel"] * unit_noise(key, k + 9))
            o[4] = f32(row[4] + q["sigma_vel"] * unit_noise(key, k + 13))
        if q["sigma_head"] != 0.0:
            eps = q["sigma_head"] * unit_noise(key, k + 17)
            sh, ch = row[6], row[7]
            t1, t2 = eps * sh, eps * ch
            c1, s1 = ch - t1, sh + t2
            m1, m2 = c1 * c1, s1 * s1
            nrm = math.sqrt(m1 + m2)
            o[5] = f32(row[5] + eps)
            if nrm != 0.0:
                o[6], o[7] = f32(s1 / nrm), f32(c1 / nrm)
        out.append(o)
    out += [[0.0] * 8 for _ in range(R - len(out))]
    counts = [sum(c != ABSENT for c in classes[1:])] + [sum(c == w for c in classes[1:])
                                                        for w in (SEEN, OUT_OF_RANGE, OCCLUDED, DROPPED)]
    return out, classes, counts


def replay(steps, B, R, occluders=None, **params):
    """steps: dicts with obs [B, R, 8] f32 (the true observation), optionally reset and p_drop (an override for that launch)
    -> (list of (seen [B, R, 8] f32, row_class [B, R] u8) per step, counts [5, B], ctr [B])."""
    q0 = dict(OFF)
    q0.update(params)
    occ = [] if occluders is None else [[(float(c[0]), float(c[1])) for c in quad] for quad in np.asarray(occluders)]
    counts, ctr, outs = [[0] * B for _ in range(5)], [0] * B, []
    for s in steps:
        q = dict(q0)
        if "p_drop" in s:
            q["p_drop"] = s["p_drop"]
        seen, cls = np.zeros((B, R, 8), np.float32), np.zeros((B, R), np.uint8)
        for b in range(B):
            if s.get("reset"):
                ctr[b] = 0
                for f in range(5):
                    counts[f][b] = 0
            rows = [[float(v) for v in row] for row in s["obs"][b]]
            o, c, n = perceive(rows, occ, q, q["env_offset"] + b, ctr[b])
            seen[b], cls[b] = np.array(o, np.float64).astype(np.float32), c
            for f in range(5):
                counts[f][b] += n[f]
            ctr[b] += 1
        outs.append((seen, cls))
    return outs, np.array(counts, np.int64).reshape(5, B), np.array(ctr, np.int64)
