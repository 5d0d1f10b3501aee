"""TEST INFRASTRUCTURE - the actuator model of csrc/mpc_actuator.hpp compiled for the host (tests/cpu_actuator_harness.cpp)
behind a numpy wrapper with the layout of evaluate.Actuation, and a plain-Python restatement (`actuate`, `replay`) of the model
to check both against: Python floats and ints only, one operation per statement, so that nothing can be contracted or
reassociated."""
import ctypes
import math
import os
import subprocess

import numpy as np

import conftest

_lib = None
INF = float("inf")
M64 = 2 ** 64 - 1
SALT = 0x9FB21C651E98DF25
COUNTS = ("steps", "held", "rate_limited", "saturated", "nonfinite")
# alpha, lo and hi as the entry point takes them (evaluate.Actuation forms them from tau and limits)
DEFAULTS = dict(dt=0.1, delay=0, p_hold=0.0, gain=(1.0, 1.0), offset=(0.0, 0.0), sigma=(0.0, 0.0), alpha=(1.0, 1.0),
                rate=(INF, INF), lo=(-INF, -INF), hi=(INF, INF), seed=0, env_offset=0)
SRC = os.path.join(conftest.ROOT, "tests", "cpu_actuator_harness.cpp")
DEPS = [SRC] + [os.path.join(conftest.ROOT, "mpc-rl_for_avs_amd", "csrc", f)
                for f in ("mpc_actuator.hpp", "mpc_core.hpp", "mpc_synth_env.hpp")]


def load():
    global _lib
    if _lib is None:
        out = os.path.join(conftest.BUILD_DIR, "libcpu_actuator.so")
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in DEPS):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            subprocess.run(["g++"] + conftest.HOST_CXXFLAGS + ["-o", out, SRC], check=True)
        _lib = ctypes.CDLL(out)
        i, vp = ctypes.c_int, ctypes.c_void_p
        _lib.actuator_step.argtypes = [i, i, vp, ctypes.c_uint64, i, i] + [vp] * 8
        _lib.actuator_step.restype = i
    return _lib


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def settings(**params):
    q = dict(DEFAULTS)
    q.update(params)
    return q


class HostActuator:
    """The kernel's buffers as numpy arrays (the layout of include/mpc_mi355x.h), stepped by the host build."""

    def __init__(self, B, **params):
        self.B, self.params = B, settings(**params)
        self.state, self.sums = np.zeros((10, B, 2)), np.zeros((2, B, 2))
        self.age, self.ctr, self.counts = np.zeros(B, np.int32), np.zeros(B, np.int64), np.zeros((5, B), np.int64)

    def step(self, command=None, done_prev=None, reset=False, out=None, missing=()):
        """-> (rc, applied): applied [B, 2] f64, NaN wherever the host build wrote nothing; `out` (may be `command` itself)
        is written instead when given; `missing`: the buffers passed as NULL"""
        q = self.params
        par = np.array([q["dt"], q["p_hold"], *q["gain"], *q["offset"], *q["sigma"], *q["alpha"], *q["rate"], *q["lo"],
                        *q["hi"]], np.float64)
        if command is not None:
            assert command.dtype == np.float64 and command.shape == (self.B, 2) and command.flags.c_contiguous
        done_prev = None if done_prev is None else np.ascontiguousarray(done_prev, np.uint8)
        applied = out if out is not None or reset else np.full((self.B, 2), np.nan)      # a reset launch writes none
        bufs = dict(command=command, done_prev=done_prev, applied=applied,
                    state=self.state, age=self.age, ctr=self.ctr, counts=self.counts, sums=self.sums)
        bufs.update({k: None for k in missing})
        rc = load().actuator_step(self.B, 1 if reset else 0, _p(par), q["seed"], q["delay"], q["env_offset"],
                                  *[_p(bufs[k]) for k in ("command", "done_prev", "applied", "state", "age", "ctr", "counts",
                                                          "sums")])
        return rc, applied

    def apply(self, command, done_prev=None, out=None):
        rc, applied = self.step(command, done_prev, out=out)
        assert rc == 0
        return applied

    def reset(self):
        assert self.step(reset=True)[0] == 0


# ---- the restatement: Python floats and ints ---------------------------------------------------------------------------------

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


def fresh():
    """the state of one environment"""
    return dict(age=0, ctr=0, ring=[[0.0, 0.0] for _ in range(8)], last=[0.0, 0.0], prev=[0.0, 0.0], counts=[0] * 5,
                sum=[0.0, 0.0], top=[0.0, 0.0])


def actuate(s, command, q, env, clear):
    """One environment, one launch.  s: its state (changed in place); command: two Python floats -> applied [2]."""
    if clear:                                                                  # 1
        s["age"] = 0
        s["ring"] = [[0.0, 0.0] for _ in range(8)]
        s["last"], s["prev"] = [0.0, 0.0], [0.0, 0.0]
    key = rng_key(q["seed"] ^ SALT, q["env_offset"] + env, s["ctr"])
    held = q["p_hold"] > 0.0 and u01(key, 0) < q["p_hold"]                     # 4: one draw for both channels
    nonfinite = rate_limited = saturated = False
    applied = []
    for c in range(2):
        u = command[c]                                                         # 2
        if not (u - u == 0.0):
            u = 0.0
            nonfinite = True
        s["ring"][s["age"] & 7][c] = u                                         # 3
        delayed = s["ring"][(s["age"] - q["delay"]) & 7][c] if s["age"] >= q["delay"] else 0.0
        if held:                                                               # 4
            delayed = s["last"][c]
        s["last"][c] = delayed
        prev = s["prev"][c]
        v = delayed                                                            # 5
        if not (q["gain"][c] == 1.0 and q["offset"][c] == 0.0):
            g = q["gain"][c] * delayed
            v = g + q["offset"][c]
        if q["sigma"][c] != 0.0:
            e = q["sigma"][c] * unit_noise(key, 1 + 4 * c)
            v = v + e
        y = v                                                                  # 6
        if q["alpha"][c] != 1.0:
            w = v - prev
            t = q["alpha"][c] * w
            y = prev + t
        if math.isfinite(q["rate"][c]):                                        # 7
            m = q["rate"][c] * q["dt"]
            d = y - prev
            if d > m:
                y = prev + m
                rate_limited = True
            if d < -m:
                y = prev - m
                rate_limited = True
        if y < q["lo"][c]:                                                     # 8
            y = q["lo"][c]
            saturated = True
        if y > q["hi"][c]:
            y = q["hi"][c]
            saturated = True
        s["prev"][c] = y                                                       # 9
        applied.append(y)
        dev = abs(y - u)
        s["sum"][c] = s["sum"][c] + dev
        if dev > s["top"][c]:
            s["top"][c] = dev
    s["age"] += 1
    s["ctr"] += 1
    for f, n in enumerate((True, held, rate_limited, saturated, nonfinite)):
        s["counts"][f] += int(n)
    return applied


def replay(steps, B, **params):
    """steps: dicts with command [B, 2] f64 and optionally done_prev [B], or reset=True (nothing else is read) -> (list of
    applied [B, 2] per step, None for a reset; state [10, B, 2], age [B], ctr [B], counts [5, B], sums [2, B, 2])."""
    q = settings(**params)
    envs = [fresh() for _ in range(B)]
    outs = []
    for s in steps:
        if s.get("reset"):
            envs = [fresh() for _ in range(B)]
            outs.append(None)
            continue
        done = s.get("done_prev")
        out = np.zeros((B, 2))
        for b in range(B):
            out[b] = actuate(envs[b], [float(v) for v in s["command"][b]], q, b, done is not None and bool(done[b]))
        outs.append(out)
    state = np.zeros((10, B, 2))
    for b, e in enumerate(envs):
        state[:8, b], state[8, b], state[9, b] = e["ring"], e["last"], e["prev"]
    return (outs, state, np.array([e["age"] for e in envs], np.int32), np.array([e["ctr"] for e in envs], np.int64),
            np.array([e["counts"] for e in envs], np.int64).T.reshape(5, B).copy(),
            np.stack([np.array([e["sum"] for e in envs]).reshape(B, 2), np.array([e["top"] for e in envs]).reshape(B, 2)]))
