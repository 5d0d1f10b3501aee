"""TEST INFRASTRUCTURE - the episode accounting of csrc/mpc_episode_stats.hpp compiled for the host
(tests/cpu_episode_stats_harness.cpp) behind a numpy wrapper with the layout of evaluate.EpisodeStats, and a plain-Python
restatement of the reference's per-episode bookkeeping (main/model_comparison.py:40-100) to check both against."""
import ctypes
import os
import subprocess

import numpy as np

import conftest

_lib = None


def load():
    global _lib
    if _lib is None:
        out = os.path.join(conftest.BUILD_DIR, "libcpu_episode_stats.so")
        src = os.path.join(conftest.ROOT, "tests", "cpu_episode_stats_harness.cpp")
        deps = [os.path.join(conftest.ROOT, "mpc-rl_for_avs_amd", "csrc", f) for f in ("mpc_episode_stats.hpp", "mpc_core.hpp")]
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in [src] + deps):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            subprocess.run(["g++"] + conftest.HOST_CXXFLAGS + ["-o", out, src], check=True)
        _lib = ctypes.CDLL(out)
        _lib.stats_episode_step.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 14
        _lib.stats_episode_step.restype = ctypes.c_int
    return _lib


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


class HostStats:
    """The kernel's state and records as numpy arrays (the layout of include/mpc_mi355x.h), stepped by the host build."""

    def __init__(self, B, Q):
        self.B, self.Q = B, Q
        self.state_i32 = np.zeros((5, B), np.int32)
        self.state_f64 = np.zeros((3, B), np.float64)
        self.rec_i32 = np.zeros((6, B, Q), np.int32)
        self.rec_f64 = np.zeros((2, B, Q), np.float64)
        self.recorded = np.zeros(1, np.int64)
        self.step_counter = np.zeros(1, np.int64)

    def update(self, s, reset=False):
        """s: dict of numpy arrays done, truncated, crashed, arrived (bool/u8), reward f32, ego [B, 4] f64, status, iters i32"""
        c = lambda k, dt: None if s.get(k) is None else np.ascontiguousarray(s[k], dt)
        args = [c("done", np.uint8), c("truncated", np.uint8), c("crashed", np.uint8), c("arrived", np.uint8),
                c("reward", np.float32), c("ego", np.float64), c("status", np.int32), c("iters", np.int32)]
        rc = load().stats_episode_step(self.B, self.Q, 1 if reset else 0, *[_p(a) for a in args], _p(self.state_i32),
                                       _p(self.state_f64), _p(self.rec_i32), _p(self.rec_f64), _p(self.recorded),
                                       _p(self.step_counter))
        assert rc == 0

    def records(self):
        from mpc_rl_for_avs_amd.evaluate import records_from_planes
        return records_from_planes(self.rec_i32, self.rec_f64)


def solved(st):
    return st == 0 or 5 <= st <= 7


def replay(steps, B, Q, resets=()):
    """model_comparison.py:40-100 for each environment on its own, as plain Python: `steps` is a list of per-step dicts
    (a `reset` entry instead of a dict where the evaluation restarts); returns records [B][Q] as dict of numpy arrays
    with the keys of EvalResult.records (slots never written stay zero)."""
    keys_i = ("steps", "success", "collision", "truncated", "unsolved", "max_iters")
    rec = {k: np.zeros((B, Q), np.int32) for k in keys_i}
    rec.update(avg_speed=np.zeros((B, Q)), **{"return": np.zeros((B, Q))})
    for b in range(B):
        j, n, total_speed, ret, collisions, unsolved, max_iters, carry = 0, 0, 0.0, 0.0, 0, 0, 0, 0.0
        for s in steps:
            if s == "reset" or (isinstance(s, dict) and s.get("reset")):
                ego = s["ego"] if isinstance(s, dict) else None
                j, n, total_speed, ret, collisions, unsolved, max_iters = 0, 0, 0.0, 0.0, 0, 0, 0
                carry = float(ego[b][3])
                continue
            total_speed += carry                     # current_speed, read before env.step (:61)
            n += 1
            ret += float(np.float32(s["reward"][b]))
            if s["crashed"][b]:                      # :75
                collisions += 1
            unsolved += 0 if solved(int(s["status"][b])) else 1
            max_iters = max(max_iters, int(s["iters"][b]))
            if s["done"][b]:
                if j < Q:
                    rec["steps"][b, j] = n
                    rec["success"][b, j] = 1 if s["arrived"][b] else 0      # :78
                    rec["collision"][b, j] = 1 if collisions > 0 else 0
                    rec["truncated"][b, j] = 1 if s["truncated"][b] else 0
                    rec["unsolved"][b, j] = unsolved
                    rec["max_iters"][b, j] = max_iters
                    rec["avg_speed"][b, j] = total_speed / n               # :90
                    rec["return"][b, j] = ret
                    j += 1
                n, total_speed, ret, collisions, unsolved, max_iters = 0, 0.0, 0.0, 0, 0, 0
            carry = float(s["ego"][b][3])
    return rec
