"""TEST INFRASTRUCTURE - the drive metrics of csrc/mpc_drive_metrics.hpp compiled for the host
(tests/cpu_drive_metrics_harness.cpp) behind a numpy wrapper with the layout of evaluate.DriveMetrics, and a plain-Python
restatement (`replay`) of the metrics' definitions to check both against: floats only, one operation per statement, so
that nothing can be contracted or reassociated."""
import ctypes
import math
import os
import subprocess

import numpy as np

import conftest

_lib = None
INF = float("inf")
I32 = ("steps", "ttc_steps", "close_steps", "hard_brake_steps")
F64 = ("min_centre_gap", "min_box_gap", "min_ttc", "max_abs_alon", "max_abs_alat", "rms_jerk", "max_jerk", "max_steer_rate",
       "mean_xte", "max_xte")


def load():
    global _lib
    if _lib is None:
        out = os.path.join(conftest.BUILD_DIR, "libcpu_drive_metrics.so")
        src = os.path.join(conftest.ROOT, "tests", "cpu_drive_metrics_harness.cpp")
        deps = [os.path.join(conftest.ROOT, "mpc-rl_for_avs_amd", "csrc", f) for f in ("mpc_drive_metrics.hpp", "mpc_core.hpp")]
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in [src] + deps):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            subprocess.run(["g++"] + conftest.HOST_CXXFLAGS + ["-o", out, src], check=True)
        _lib = ctypes.CDLL(out)
        d = ctypes.c_double
        _lib.drive_metrics_step.argtypes = [ctypes.c_int] * 5 + [d] + [ctypes.c_void_p] * 9
        _lib.drive_metrics_step.restype = ctypes.c_int
        _lib.drive_box_gap.argtypes, _lib.drive_box_gap.restype = [d] * 8, d
        _lib.drive_ttc.argtypes, _lib.drive_ttc.restype = [d] * 4, d
        _lib.drive_xte.argtypes, _lib.drive_xte.restype = [d, d, ctypes.c_void_p, ctypes.c_int], d
    return _lib


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def host_box_gap(p, h, q, g):
    """p, q: centres; h, g: axes (cos, sin)"""
    return load().drive_box_gap(p[0], p[1], h[0], h[1], q[0], q[1], g[0], g[1])


def host_ttc(r, u):
    return load().drive_ttc(r[0], r[1], u[0], u[1])


def host_xte(p, ref_xy):
    ref = np.ascontiguousarray(ref_xy, np.float64)
    return load().drive_xte(p[0], p[1], _p(ref), ref.shape[0])


class HostDrive:
    """The kernel's state and records as numpy arrays (the layout of include/mpc_mi355x.h), stepped by the host build."""

    def __init__(self, B, Q, ref_xy, dt, rows):
        self.B, self.Q, self.dt, self.rows = B, Q, float(dt), rows
        self.ref_xy = np.ascontiguousarray(ref_xy, np.float64)
        self.state_i32 = np.zeros((5, B), np.int32)
        self.state_f64 = np.zeros((17, B), np.float64)
        self.rec_i32 = np.zeros((4, B, Q), np.int32)
        self.rec_f64 = np.zeros((10, B, Q), np.float64)

    def update(self, s, reset=False):
        """s: dict of numpy arrays terminal_obs, obs [B, R, 8] f32, act [B, 2] f64, done [B] (a reset needs obs only)"""
        c = lambda k, dt: None if s.get(k) is None else np.ascontiguousarray(s[k], dt)
        args = [c("terminal_obs", np.float32), c("obs", np.float32), c("act", np.float64), c("done", np.uint8)]
        rc = load().drive_metrics_step(self.B, self.rows, self.Q, self.ref_xy.shape[0], 1 if reset else 0, self.dt,
                                       *[_p(a) for a in args], _p(self.ref_xy), _p(self.state_i32), _p(self.state_f64),
                                       _p(self.rec_i32), _p(self.rec_f64))
        assert rc == 0

    def records(self):
        from mpc_rl_for_avs_amd.evaluate import DRIVE_F64, DRIVE_I32, records_from_planes
        return records_from_planes(self.rec_i32, self.rec_f64, DRIVE_I32, DRIVE_F64)


# ---- the plain-Python restatement ---------------------------------------------------------------------------------------

def _dot(ax, ay, bx, by):
    m0 = ax * bx
    m1 = ay * by
    return m0 + m1


def point_segment2(x, y, e0x, e0y, dx, dy):
    """squared distance of (x, y) to the segment from e0 to e0 + d, the parameter clamped to [0, 1]"""
    sx = x - e0x
    sy = y - e0y
    dd = _dot(dx, dy, dx, dy)
    t = 0.0
    if dd > 0.0:
        num = _dot(sx, sy, dx, dy)
        t = num / dd
        if t < 0.0:
            t = 0.0
        if t > 1.0:
            t = 1.0
    tx = t * dx
    ty = t * dy
    cx = sx - tx
    cy = sy - ty
    return _dot(cx, cy, cx, cy)


def rectangle(px, py, hx, hy):
    """corners of the 5.0 x 2.0 rectangle: centre +- 2.5 axis +- 1.0 normal, normal = (-sin, cos), in the order
    (+,+), (-,+), (-,-), (+,-)"""
    nx = -hy
    ny = hx
    lx = 2.5 * hx
    ly = 2.5 * hy
    wx = 1.0 * nx
    wy = 1.0 * ny
    fx = px + lx
    fy = py + ly
    bx = px - lx
    by = py - ly
    return [(fx + wx, fy + wy), (bx + wx, by + wy), (bx - wx, by - wy), (fx - wx, fy - wy)]


def _axis_separates(rx, ry, hx, hy, gx, gy, ax, ay):
    t0 = 2.5 * abs(_dot(hx, hy, ax, ay))
    t1 = 1.0 * abs(_dot(-hy, hx, ax, ay))
    t2 = 2.5 * abs(_dot(gx, gy, ax, ay))
    t3 = 1.0 * abs(_dot(-gy, gx, ax, ay))
    reach = t0 + t1
    reach = reach + t2
    reach = reach + t3
    return abs(_dot(rx, ry, ax, ay)) > reach


def _corners_edges2(cs, es):
    best = INF
    for k in range(4):
        e0, e1 = es[k], es[(k + 1) % 4]
        dx = e1[0] - e0[0]
        dy = e1[1] - e0[1]
        for c in cs:
            d2 = point_segment2(c[0], c[1], e0[0], e0[1], dx, dy)
            if d2 < best:
                best = d2
    return best


def box_gap(px, py, hx, hy, qx, qy, gx, gy):
    rx = qx - px
    ry = qy - py
    apart = False
    for ax, ay in ((hx, hy), (-hy, hx), (gx, gy), (-gy, gx)):
        apart = apart or _axis_separates(rx, ry, hx, hy, gx, gy, ax, ay)
    if not apart:
        return 0.0
    a, b = rectangle(px, py, hx, hy), rectangle(qx, qy, gx, gy)
    return math.sqrt(min(_corners_edges2(a, b), _corners_edges2(b, a)))


def ttc(rx, ry, ux, uy):
    rr = _dot(rx, ry, rx, ry)
    d2 = 2.5 * 2.5
    if rr <= d2:
        return 0.0
    a = _dot(ux, uy, ux, uy)
    b = _dot(rx, ry, ux, uy)
    c = rr - d2
    bb = b * b
    ac = a * c
    disc = bb - ac
    if a == 0.0 or b >= 0.0 or disc < 0.0:
        return INF
    root = math.sqrt(disc)
    num = -b - root
    return num / a


def xte(px, py, ref_xy):
    M = len(ref_xy)
    best = INF
    for i in range(max(M - 1, 1)):
        i1 = min(i + 1, M - 1)
        e0x, e0y = float(ref_xy[i][0]), float(ref_xy[i][1])
        dx = float(ref_xy[i1][0]) - e0x
        dy = float(ref_xy[i1][1]) - e0y
        best = min(best, point_segment2(px, py, e0x, e0y, dx, dy))
    return math.sqrt(best)


def replay(steps, B, Q, ref_xy, dt, rows):
    """The metrics of each environment on its own, as plain Python.  `steps`: per-step dicts (terminal_obs, obs, act, done);
    a dict with `reset` (and obs) where the evaluation restarts.  Returns the four planes of mpc_drive_metrics: rec_i32
    [4, B, Q], rec_f64 [10, B, Q] (slots never written stay zero), state_i32 [5, B], state_f64 [17, B]."""
    rec_i = np.zeros((4, B, Q), np.int32)
    rec_f = np.zeros((10, B, Q), np.float64)
    st_i = np.zeros((5, B), np.int32)
    st_f = np.zeros((17, B), np.float64)
    f = lambda v: float(np.float32(v))                   # an f32 observation widened exactly
    dt = float(dt)
    for b in range(B):
        fresh = lambda: dict(n=0, n_ttc=0, n_close=0, n_brake=0, centre=INF, box=INF, ttc=INF, alon=0.0, alat=0.0, jsum=0.0,
                             jmax=0.0, rate=0.0, xsum=0.0, xmax=0.0)
        e, j = fresh(), 0
        cvx = cvy = ccos = csin = cax = cay = csteer = 0.0
        for s in steps:
            nxt = s["obs"][b][0]
            if s.get("reset"):
                e, j = fresh(), 0
                cax = cay = csteer = 0.0
            else:
                t = s["terminal_obs"][b]
                px, py, vx, vy, hy, hx = f(t[0][1]), f(t[0][2]), f(t[0][3]), f(t[0][4]), f(t[0][6]), f(t[0][7])
                centre = box = tt = INF
                for i in range(1, rows):
                    if t[i][0] == 0:
                        continue
                    qx, qy, wx, wy, gy, gx = f(t[i][1]), f(t[i][2]), f(t[i][3]), f(t[i][4]), f(t[i][6]), f(t[i][7])
                    rx = qx - px
                    ry = qy - py
                    centre = min(centre, math.sqrt(_dot(rx, ry, rx, ry)))
                    box = min(box, box_gap(px, py, hx, hy, qx, qy, gx, gy))
                    ux = wx - vx
                    uy = wy - vy
                    tt = min(tt, ttc(rx, ry, ux, uy))
                x = xte(px, py, ref_xy)
                dvx = vx - cvx
                dvy = vy - cvy
                ax = dvx / dt
                ay = dvy / dt
                steer = float(s["act"][b][1])
                alon = _dot(ax, ay, ccos, csin)
                m0 = ay * ccos
                m1 = ax * csin
                alat = m0 - m1
                e["n"] += 1
                e["n_ttc"] += 1 if tt < 2.0 else 0
                e["n_close"] += 1 if box < 1.0 else 0
                e["n_brake"] += 1 if alon < -3.0 else 0
                e["centre"], e["box"], e["ttc"] = min(e["centre"], centre), min(e["box"], box), min(e["ttc"], tt)
                e["alon"], e["alat"] = max(e["alon"], abs(alon)), max(e["alat"], abs(alat))
                if e["n"] >= 2:
                    dax = ax - cax
                    day = ay - cay
                    jx = dax / dt
                    jy = day / dt
                    j2 = _dot(jx, jy, jx, jy)
                    e["jsum"] = e["jsum"] + j2
                    e["jmax"] = max(e["jmax"], math.sqrt(j2))
                    dsteer = abs(steer - csteer)
                    e["rate"] = max(e["rate"], dsteer / dt)
                e["xsum"] = e["xsum"] + x
                e["xmax"] = max(e["xmax"], x)
                if s["done"][b]:
                    if j < Q:
                        rec_i[:, b, j] = (e["n"], e["n_ttc"], e["n_close"], e["n_brake"])
                        rms = math.sqrt(e["jsum"] / float(e["n"] - 1)) if e["n"] >= 2 else 0.0
                        rec_f[:, b, j] = (e["centre"], e["box"], e["ttc"], e["alon"], e["alat"], rms, e["jmax"], e["rate"],
                                          e["xsum"] / float(e["n"]), e["xmax"])
                        j += 1
                    e = fresh()
                cax, cay, csteer = ax, ay, steer
            cvx, cvy, ccos, csin = f(nxt[3]), f(nxt[4]), f(nxt[7]), f(nxt[6])
        st_i[:, b] = (e["n"], e["n_ttc"], e["n_close"], e["n_brake"], j)
        st_f[:, b] = (e["centre"], e["box"], e["ttc"], e["alon"], e["alat"], e["jsum"], e["jmax"], e["rate"], e["xsum"],
                      e["xmax"], cvx, cvy, ccos, csin, cax, cay, csteer)
    return dict(rec_i32=rec_i, rec_f64=rec_f, state_i32=st_i, state_f64=st_f)
