"""TEST INFRASTRUCTURE - the tracker of csrc/mpc_tracker.hpp compiled for the host (tests/cpu_tracker_harness.cpp) behind a
numpy wrapper with the layout of evaluate.Tracker, and a plain-Python restatement (`track`, `replay`) of the model to check
both against: Python floats and ints only, one operation per statement, so that nothing can be contracted or reassociated."""
import ctypes
import os
import struct
import subprocess

import numpy as np

import conftest

_lib = None
INF = float("inf")
SLOTS, NO_SLOT = 16, 255
COUNTS = ("measured", "matched", "born", "coasted", "expired", "evicted", "cut")
DEFAULTS = dict(dt=0.1, gate=3.0, coast=0, alpha_pos=1.0, alpha_vel=1.0)
SRC = os.path.join(conftest.ROOT, "tests", "cpu_tracker_harness.cpp")
DEPS = [SRC] + [os.path.join(conftest.ROOT, "mpc-rl_for_avs_amd", "csrc", f) for f in ("mpc_tracker.hpp", "mpc_core.hpp")]


def load():
    global _lib
    if _lib is None:
        out = os.path.join(conftest.BUILD_DIR, "libcpu_tracker.so")
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in DEPS):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            subprocess.run(["g++"] + conftest.HOST_CXXFLAGS + ["-o", out, SRC], check=True)
        _lib = ctypes.CDLL(out)
        i, d, vp = ctypes.c_int, ctypes.c_double, ctypes.c_void_p
        _lib.tracker_step.argtypes = [i, i, i, d, d, i, d, d] + [vp] * 8
        _lib.tracker_step.restype = i
    return _lib


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


class HostTracker:
    """The kernel's buffers as numpy arrays (the layout of include/mpc_mi355x.h), stepped by the host build."""

    def __init__(self, B, R, **params):
        self.B, self.R = B, R
        self.params = dict(DEFAULTS)
        self.params.update(params)
        self.row_slot, self.row_miss = np.zeros((B, R), np.uint8), np.zeros((B, R), np.uint8)
        self.track_f64, self.track_i32 = np.zeros((B, SLOTS, 7)), np.zeros((B, SLOTS, 3), np.int32)
        self.counts = np.zeros((7, B), np.int64)

    def step(self, meas, done=None, reset=False, planes=True):
        """-> (rc, out): out [B, R, 8] f32, NaN wherever the host build wrote nothing"""
        meas = np.ascontiguousarray(meas, np.float32)
        assert meas.shape == (self.B, self.R, 8)
        done = None if done is None else np.ascontiguousarray(done, np.uint8)
        out = np.full((self.B, self.R, 8), np.float32(np.nan))
        q = self.params
        rc = load().tracker_step(self.B, self.R, 1 if reset else 0, q["dt"], q["gate"], q["coast"], q["alpha_pos"],
                                 q["alpha_vel"], _p(meas), _p(done), _p(out), _p(self.row_slot) if planes else None,
                                 _p(self.row_miss) if planes else None, _p(self.track_f64), _p(self.track_i32), _p(self.counts))
        return rc, out

    def apply(self, meas, done=None, reset=False):
        rc, out = self.step(meas, done, reset)
        assert rc == 0
        return out

    def totals(self):
        return {k: int(self.counts[i].sum()) for i, k in enumerate(COUNTS)}


# ---- the restatement: Python floats and ints ---------------------------------------------------------------------------------

def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def empty():
    return dict(v=[0.0] * 7, alive=0, age=0, miss=0)


def blend(a, alpha, m):
    if alpha == 1.0:
        return m
    r = m - a
    g = alpha * r
    return a + g


def track(slots, rows, q, clear):
    """One environment, one launch.  slots: 16 dicts (v = [x, y, vx, vy, heading, sin_h, cos_h], alive, age, miss), changed in
    place; rows: R lists of 8 Python floats (exact f32 values); q the parameters -> (out rows [R][8], row_slot [R], row_miss
    [R], counts [7])."""
    R = len(rows)
    gate2 = q["gate"] * q["gate"]
    if clear:                                                                  # 1
        for s in range(SLOTS):
            slots[s] = empty()
    for t in slots:                                                            # 2
        if t["alive"]:
            sx = t["v"][2] * q["dt"]
            sy = t["v"][3] * q["dt"]
            t["v"][0] = t["v"][0] + sx
            t["v"][1] = t["v"][1] + sy
    claimed = [False] * SLOTS
    unassociated, measured, matched = [], 0, 0
    for i in range(1, R):                                                      # 3
        row = rows[i]
        if row[0] == 0.0:
            continue
        measured += 1
        best, best_d = None, None
        for s, t in enumerate(slots):
            if not t["alive"] or claimed[s]:
                continue
            dx = row[1] - t["v"][0]
            dy = row[2] - t["v"][1]
            a = dx * dx
            c = dy * dy
            d = a + c
            if d <= gate2 and (best is None or d < best_d):
                best, best_d = s, d
        if best is None:
            unassociated.append(i)
            continue
        claimed[best] = True                                                   # 4
        t = slots[best]
        t["v"][0] = blend(t["v"][0], q["alpha_pos"], row[1])
        t["v"][1] = blend(t["v"][1], q["alpha_pos"], row[2])
        t["v"][2] = blend(t["v"][2], q["alpha_vel"], row[3])
        t["v"][3] = blend(t["v"][3], q["alpha_vel"], row[4])
        t["v"][4:7] = row[5:8]
        t["miss"] = 0
        t["age"] += 1
        matched += 1
    expired = 0
    for s in range(SLOTS):                                                     # 5
        if slots[s]["alive"] and not claimed[s]:
            slots[s]["miss"] += 1
            if slots[s]["miss"] > q["coast"]:
                slots[s] = empty()
                expired += 1
    queue = [s for s in range(SLOTS) if not slots[s]["alive"]]                 # 6
    queue += [s for s in range(SLOTS) if slots[s]["alive"] and not claimed[s]]
    evicted = 0
    for k, i in enumerate(unassociated):
        s = queue[k]
        evicted += slots[s]["alive"]
        slots[s] = dict(v=list(rows[i][1:8]), alive=1, age=1, miss=0)
    ex, ey = rows[0][1], rows[0][2]                                            # 7
    keyed = []
    for s, t in enumerate(slots):
        if t["alive"]:
            kx = t["v"][0] - ex
            ky = t["v"][1] - ey
            a = kx * kx
            c = ky * ky
            keyed.append((a + c, s))
    keyed.sort()                                                               # by key, ties to the lowest slot
    out, row_slot, row_miss = [list(rows[0])], [NO_SLOT], [0]
    for _, s in keyed[:R - 1]:
        out.append([1.0] + [f32(v) for v in slots[s]["v"]])
        row_slot.append(s)
        row_miss.append(slots[s]["miss"])
    coasted = sum(1 for m in row_miss if m > 0)
    cut = len(keyed) - (len(out) - 1)
    while len(out) < R:
        out.append([0.0] * 8)
        row_slot.append(NO_SLOT)
        row_miss.append(0)
    return out, row_slot, row_miss, [measured, matched, len(unassociated), coasted, expired, evicted, cut]


def replay(steps, B, R, **params):
    """steps: dicts with obs [B, R, 8] f32 (the measured observation), optionally reset and done [B] -> (list of (out [B, R, 8]
    f32, row_slot [B, R] u8, row_miss [B, R] u8) per step, track_f64 [B, 16, 7], track_i32 [B, 16, 3], counts [7, B])."""
    q = dict(DEFAULTS)
    q.update(params)
    slots = [[empty() for _ in range(SLOTS)] for _ in range(B)]
    counts, outs = [[0] * B for _ in range(7)], []
    for s in steps:
        out, slot, miss = np.zeros((B, R, 8), np.float32), np.zeros((B, R), np.uint8), np.zeros((B, R), np.uint8)
        reset, done = bool(s.get("reset")), s.get("done")
        for b in range(B):
            if reset:
                for f in range(7):
                    counts[f][b] = 0
            rows = [[float(v) for v in row] for row in s["obs"][b]]
            o, rs, rm, n = track(slots[b], rows, q, reset or (done is not None and bool(done[b])))
            out[b], slot[b], miss[b] = np.array(o, np.float64).astype(np.float32), rs, rm
            for f in range(7):
                counts[f][b] += n[f]
        outs.append((out, slot, miss))
    tf = np.array([[t["v"] for t in env] for env in slots], np.float64).reshape(B, SLOTS, 7)
    ti = np.array([[[t["alive"], t["age"], t["miss"]] for t in env] for env in slots], np.int32).reshape(B, SLOTS, 3)
    return outs, tf, ti, np.array(counts, np.int64).reshape(7, B)
