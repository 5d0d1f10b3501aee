"""Closed-loop evaluation of the MPC and MPC-RL agents for many environments at once (the reference's model comparison,
main/model_comparison.py:40-100, 160-172, 195-199).

The reference runs its agents one episode after the other, one CasADi / IPOPT solve per step, and reports five numbers per
agent: success rate, collision rate, average steps, average speed and average travel time.  `evaluate_agent` runs B
environments of a `SyntheticIntersectionEnv` in closed loop with one agent and records every episode; `compare` does that for
several agents on the same episodes.

Which episodes count: each environment records its first Q = `episodes_per_env` episodes (records [B][Q], N = B Q episodes)
and then idles, stepping with the batch without writing anything.  "The first N episodes to finish" would favour short
episodes, i.e. crashes; a fixed quota per environment does not depend on how long other environments' episodes take, nor on
how the batch is split into shards.

A step is the agent's device action (`act_batch_torch`: policy and / or MPC, enqueue-only, fixed output addresses), the
environment's step, and the accounting.  With the HIP environment the accounting is one kernel (mpc_episode_stats,
csrc/mpc_episode_stats.hpp) and the step is captured once as a hipGraph and replayed; with the torch environment (the CPU
path) it is `EpisodeStats._torch_update`, the same update as a few torch ops.

`metrics=True` adds the safety and comfort metrics of csrc/mpc_drive_metrics.hpp to every episode (`DriveMetrics`: how close
the ego got, time on a collision course, braking, jerk, route keeping), computed per step from the observations inside the
same captured step (mpc_drive_metrics), or by the same update in elementwise torch ops on the CPU path.
"""
from __future__ import annotations

import ctypes
import time
from dataclasses import dataclass

import numpy as np
import torch

from .rollout import EPISODE_STEPS, VEHICLES_COUNT

REC_I32 = ("steps", "success", "collision", "truncated", "unsolved", "max_iters")   # rec_i32 [6][B][Q]
REC_F64 = ("avg_speed", "return")                                                   # rec_f64 [2][B][Q]
_BOOL = ("success", "collision", "truncated")
DRIVE_I32 = ("steps", "ttc_steps", "close_steps", "hard_brake_steps")               # mpc_drive_metrics rec_i32 [4][B][Q]
DRIVE_F64 = ("min_centre_gap", "min_box_gap", "min_ttc", "max_abs_alon", "max_abs_alat", "rms_jerk", "max_jerk",
             "max_steer_rate", "mean_xte", "max_xte")                               # rec_f64 [10][B][Q]
# csrc/mpc_drive_metrics.hpp: the vehicle's half length and half width, the environment's crash distance, and this
# project's thresholds (time to collision [s], box gap [m], longitudinal deceleration [m/s^2])
HALF_LENGTH, HALF_WIDTH, CRASH_DISTANCE = 2.5, 1.0, 2.5
TTC_THRESHOLD, CLOSE_GAP, HARD_BRAKE = 2.0, 1.0, 3.0
MAX_ROWS, MAX_ROUTE = 17, 128                                                       # MPC_MAX_OTHERS + 1, route points


def records_from_planes(rec_i32, rec_f64) -> dict:
    """The record planes of the accounting (include/mpc_mi355x.h layout) -> dict of numpy arrays [B, Q]."""
    rec_i32, rec_f64 = np.asarray(rec_i32), np.asarray(rec_f64)
    out = {k: (rec_i32[i] != 0) if k in _BOOL else rec_i32[i].copy() for i, k in enumerate(REC_I32)}
    out.update({k: rec_f64[i].copy() for i, k in enumerate(REC_F64)})
    return out


def _solved(status):
    return (status == 0) | ((status >= 5) & (status <= 7))       # MPC_STATUS_IS_SOLVED


def _u8(t):
    return t.view(torch.uint8) if t.dtype == torch.bool else t


class EpisodeStats:
    """Running state and records of the accounting, as device tensors in the layout of mpc_episode_stats
    (include/mpc_mi355x.h); `update` is the kernel (backend "hip") or the same update in torch ops (backend "torch")."""

    def __init__(self, B: int, Q: int, device, backend: str = "torch"):
        if Q < 1:
            raise ValueError("episodes_per_env must be >= 1")
        self.B, self.Q, self.device, self.backend = int(B), int(Q), torch.device(device), backend
        z = lambda *s, dt: torch.zeros(s, dtype=dt, device=self.device)
        self.state_i32 = z(5, B, dt=torch.int32)        # steps, crashed, unsolved, max_iters, ordinal
        self.state_f64 = z(3, B, dt=torch.float64)      # speed sum, return, carry_speed
        self.rec_i32 = z(6, B, Q, dt=torch.int32)
        self.rec_f64 = z(2, B, Q, dt=torch.float64)
        self.recorded = z(1, dt=torch.int64)
        if backend == "hip":
            from . import engine as _engine
            self._lib = _engine.load_library()

    def update(self, ego, done=None, truncated=None, crashed=None, arrived=None, reward=None, status=None, iters=None,
               reset=False, step_counter=None):
        if self.backend == "torch":
            self._torch_update(ego, done, truncated, crashed, arrived, reward, status, iters, reset)
            if step_counter is not None and not reset:
                step_counter += 1
            return
        p = lambda t: None if t is None else ctypes.c_void_p(_u8(t).data_ptr())
        rc = self._lib.mpc_episode_stats(
            self.device.index, self.B, self.Q, 1 if reset else 0, p(done), p(truncated), p(crashed), p(arrived), p(reward),
            p(ego), p(status), p(iters), p(self.state_i32), p(self.state_f64), p(self.rec_i32), p(self.rec_f64),
            p(self.recorded), p(step_counter), ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        if rc != 0:
            raise RuntimeError(f"mpc_episode_stats failed ({rc}): {self._lib.mpc_last_error().decode()}")

    @torch.no_grad()
    def _torch_update(self, ego, done, truncated, crashed, arrived, reward, status, iters, reset):
        si, sf, B, Q = self.state_i32, self.state_f64, self.B, self.Q
        if reset:
            si.zero_()
            sf[:2].zero_()
            sf[2].copy_(ego[:, 3])
            self.recorded.zero_()
            return
        steps = si[0] + 1
        crash = (si[1] != 0) | crashed.bool()
        unsolved = si[2] + (~_solved(status)).to(torch.int32)
        max_iters = torch.maximum(si[3], iters.to(torch.int32))
        speed_sum = sf[0] + sf[2]
        ret = sf[1] + reward.to(torch.float64)
        j = si[4]
        done = done.bool()
        write = done & (j < Q)
        slot = torch.arange(B, device=self.device) * Q + torch.clamp(j, max=Q - 1).long()
        i32 = lambda t: t.to(torch.int32)
        new_i = torch.stack([steps, i32(arrived.bool()), i32(crash), i32(truncated.bool()), unsolved, max_iters])
        new_f = torch.stack([speed_sum / steps, ret])
        for rec, new in ((self.rec_i32.view(6, B * Q), new_i), (self.rec_f64.view(2, B * Q), new_f)):
            rec[:, slot] = torch.where(write, new, rec[:, slot])
        self.recorded += write.sum()
        keep = ~done
        for i, t in enumerate((steps, i32(crash), unsolved, max_iters)):
            si[i] = torch.where(keep, t, torch.zeros_like(t))
        si[4] = j + i32(write)
        sf[0] = torch.where(keep, speed_sum, torch.zeros_like(speed_sum))
        sf[1] = torch.where(keep, ret, torch.zeros_like(ret))
        sf[2] = ego[:, 3]

    def records(self) -> dict:
        return records_from_planes(self.rec_i32.cpu().numpy(), self.rec_f64.cpu().numpy())


def drive_records_from_planes(rec_i32, rec_f64) -> dict:
    """The record planes of the drive metrics (include/mpc_mi355x.h layout) -> dict of numpy arrays [B, Q]."""
    rec_i32, rec_f64 = np.asarray(rec_i32), np.asarray(rec_f64)
    out = {k: rec_i32[i].copy() for i, k in enumerate(DRIVE_I32)}
    out.update({k: rec_f64[i].copy() for i, k in enumerate(DRIVE_F64)})
    return out


def _sqrt(x):
    """Correctly rounded square root.  torch.sqrt on the CPU may go through a vector maths library that is accurate to one
    unit in the last place only, which would break the bitwise agreement with the kernel; numpy's is the hardware's."""
    if x.device.type == "cpu":
        return torch.from_numpy(np.sqrt(x.contiguous().numpy()))
    return torch.sqrt(x)


def _seg2(x, y, e0x, e0y, dx, dy):
    """Squared distance of the point (x, y) to the segment e0 + t d, 0 <= t <= 1 (csrc/mpc_drive_metrics.hpp: seg2)."""
    sx, sy = x - e0x, y - e0y
    dd = dx * dx + dy * dy
    pos = dd > 0
    t = (sx * dx + sy * dy) / torch.where(pos, dd, torch.ones_like(dd))
    t = torch.where(pos, t, torch.zeros_like(t))
    t = torch.where(t < 0, torch.zeros_like(t), t)
    t = torch.where(t > 1, torch.ones_like(t), t)
    cx, cy = sx - t * dx, sy - t * dy
    return cx * cx + cy * cy


def _corners(px, py, hx, hy):
    lx, ly = HALF_LENGTH * hx, HALF_LENGTH * hy
    wx, wy = HALF_WIDTH * -hy, HALF_WIDTH * hx
    fx, fy, bx, by = px + lx, py + ly, px - lx, py - ly
    return [(fx + wx, fy + wy), (bx + wx, by + wy), (bx - wx, by - wy), (fx - wx, fy - wy)]


def _corners_to_edges2(c, e):
    best = None
    for k in range(4):
        dx, dy = e[(k + 1) & 3][0] - e[k][0], e[(k + 1) & 3][1] - e[k][1]
        for i in range(4):
            d = _seg2(c[i][0], c[i][1], e[k][0], e[k][1], dx, dy)
            best = d if best is None else torch.minimum(best, d)
    return best


def _box_gap(px, py, hx, hy, qx, qy, gx, gy):
    rx, ry = qx - px, qy - py
    apart = None
    for ax, ay in ((hx, hy), (-hy, hx), (gx, gy), (-gy, gx)):
        reach = HALF_LENGTH * (hx * ax + hy * ay).abs() + HALF_WIDTH * (-hy * ax + hx * ay).abs() + \
            HALF_LENGTH * (gx * ax + gy * ay).abs() + HALF_WIDTH * (-gy * ax + gx * ay).abs()
        sep = (rx * ax + ry * ay).abs() > reach
        apart = sep if apart is None else apart | sep
    px, py, hx, hy, qx, qy, gx, gy = torch.broadcast_tensors(px, py, hx, hy, qx, qy, gx, gy)
    a, b = _corners(px, py, hx, hy), _corners(qx, qy, gx, gy)
    gap = _sqrt(torch.minimum(_corners_to_edges2(a, b), _corners_to_edges2(b, a)))
    return torch.where(apart, gap, torch.zeros_like(gap))


def _ttc(rx, ry, ux, uy):
    rr, d2 = rx * rx + ry * ry, CRASH_DISTANCE * CRASH_DISTANCE
    a, b, c = ux * ux + uy * uy, rx * ux + ry * uy, rr - d2
    disc = b * b - a * c
    closing = (a != 0) & (b < 0) & (disc >= 0)
    t = (-b - _sqrt(torch.where(closing, disc, torch.zeros_like(disc)))) / torch.where(closing, a, torch.ones_like(a))
    t = torch.where(closing, t, torch.full_like(t, float("inf")))
    return torch.where(rr <= d2, torch.zeros_like(t), t)


class DriveMetrics:
    """Running state and records of the safety and comfort metrics, as device tensors in the layout of mpc_drive_metrics
    (include/mpc_mi355x.h; formulas in csrc/mpc_drive_metrics.hpp); `update` is the kernel (backend "hip") or the same update
    in elementwise torch ops (backend "torch": every dot product written a*b + c*d, no reduction but min, so both agree bit
    for bit).  ref_xy [M, 2]: the ego's route; dt: the step length; rows: rows of an observation (ego + others)."""

    def __init__(self, B: int, Q: int, device, backend: str = "torch", ref_xy=None, dt: float = 0.1,
                 rows: int = VEHICLES_COUNT):
        if Q < 1:
            raise ValueError("episodes_per_env must be >= 1")
        if not 1 <= int(rows) <= MAX_ROWS:
            raise ValueError(f"rows must be 1..{MAX_ROWS}")
        if not float(dt) > 0:
            raise ValueError("dt must be > 0")
        if ref_xy is None:
            raise ValueError("DriveMetrics needs the ego's route ref_xy [M, 2]")
        self.B, self.Q, self.device, self.backend = int(B), int(Q), torch.device(device), backend
        self.dt, self.rows = float(dt), int(rows)
        self.ref_xy = torch.as_tensor(ref_xy, dtype=torch.float64).to(self.device).contiguous()
        if self.ref_xy.ndim != 2 or self.ref_xy.shape[1] != 2 or not 1 <= self.ref_xy.shape[0] <= MAX_ROUTE:
            raise ValueError(f"ref_xy must be [M, 2] with 1 <= M <= {MAX_ROUTE}")
        self.M = int(self.ref_xy.shape[0])
        z = lambda *s, dt: torch.zeros(s, dtype=dt, device=self.device)
        self.state_i32 = z(5, B, dt=torch.int32)        # steps, ttc_steps, close_steps, hard_brake_steps, ordinal
        self.state_f64 = z(17, B, dt=torch.float64)     # ten running values, then the carries vx vy cos sin ax ay steer
        self.rec_i32 = z(4, B, Q, dt=torch.int32)
        self.rec_f64 = z(10, B, Q, dt=torch.float64)
        if backend == "hip":
            from . import engine as _engine
            self._lib = _engine.load_library()
        else:                                            # the route's segments: start and end - start
            nseg = max(self.M - 1, 1)
            end = self.ref_xy[torch.clamp(torch.arange(nseg, device=self.device) + 1, max=self.M - 1)]
            self._e0, self._d = self.ref_xy[:nseg], end - self.ref_xy[:nseg]

    def _check(self, t, name, shape, dtype):
        if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {shape}")

    def update(self, terminal_obs, obs, action, done, reset=False):
        B, R = self.B, self.rows
        self._check(obs, "obs", (B, R, 8), torch.float32)
        if not reset:
            self._check(terminal_obs, "terminal_obs", (B, R, 8), torch.float32)
            self._check(action, "action", (B, 2), torch.float64)
            done = _u8(done)
            self._check(done, "done", (B,), torch.uint8)
        if self.backend == "torch":
            self._torch_update(terminal_obs, obs, action, done, reset)
            return
        p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
        rc = self._lib.mpc_drive_metrics(
            self.device.index, B, R, self.Q, self.M, 1 if reset else 0, self.dt, None if reset else p(terminal_obs), p(obs),
            None if reset else p(action), None if reset else p(done), p(self.ref_xy), p(self.state_i32), p(self.state_f64),
            p(self.rec_i32), p(self.rec_f64), ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        if rc != 0:
            raise RuntimeError(f"mpc_drive_metrics failed ({rc}): {self._lib.mpc_last_error().decode()}")

    def _gaps(self, t):
        """Minima over the present rows of the scene t [B, R, 8] (f64): centre gap, box gap, time to collision [B]."""
        inf = torch.full((self.B,), float("inf"), dtype=torch.float64, device=self.device)
        if self.rows == 1:
            return inf, inf.clone(), inf.clone()
        e = lambda c: t[:, 0, c].unsqueeze(1)            # the ego [B, 1] against the other rows [B, R - 1]
        o = lambda c: t[:, 1:, c]
        px, py, vx, vy, hy, hx = e(1), e(2), e(3), e(4), e(6), e(7)
        qx, qy, wx, wy, gy, gx = o(1), o(2), o(3), o(4), o(6), o(7)
        rx, ry = qx - px, qy - py
        present = o(0) != 0
        fold = lambda v: torch.where(present, v, torch.full_like(v, float("inf"))).min(dim=1).values
        return (fold(_sqrt(rx * rx + ry * ry)), fold(_box_gap(px, py, hx, hy, qx, qy, gx, gy)),
                fold(_ttc(rx, ry, wx - vx, wy - vy)))

    @torch.no_grad()
    def _torch_update(self, terminal_obs, obs, action, done, reset):
        si, sf, B, Q, dt = self.state_i32, self.state_f64, self.B, self.Q, self.dt
        nxt = obs[:, 0].to(torch.float64)
        carry = lambda ax, ay, steer: [nxt[:, 3], nxt[:, 4], nxt[:, 7], nxt[:, 6], ax, ay, steer]
        if reset:
            si.zero_()
            sf[:3] = float("inf")
            sf[3:].zero_()
            for i, v in enumerate(carry(0.0, 0.0, 0.0)):
                sf[10 + i] = v
            return
        t = terminal_obs.to(torch.float64)
        centre, box, ttc = self._gaps(t)
        px, py = t[:, 0, 1].unsqueeze(1), t[:, 0, 2].unsqueeze(1)
        xte = _sqrt(_seg2(px, py, self._e0[None, :, 0], self._e0[None, :, 1], self._d[None, :, 0],
                               self._d[None, :, 1]).min(dim=1).values)
        steps = si[0] + 1
        ax, ay = (t[:, 0, 3] - sf[10]) / dt, (t[:, 0, 4] - sf[11]) / dt
        steer = action[:, 1]
        alon, alat = ax * sf[12] + ay * sf[13], ay * sf[12] - ax * sf[13]
        i32 = lambda m: m.to(torch.int32)
        ttc_steps, close_steps = si[1] + i32(ttc < TTC_THRESHOLD), si[2] + i32(box < CLOSE_GAP)
        brake_steps = si[3] + i32(alon < -HARD_BRAKE)
        second = steps >= 2                              # jerk and steering rate need the step before, of the same episode
        jx, jy = (ax - sf[14]) / dt, (ay - sf[15]) / dt
        j2 = jx * jx + jy * jy
        jerk_sum = torch.where(second, sf[5] + j2, sf[5])
        max_jerk = torch.where(second, torch.maximum(sf[6], _sqrt(j2)), sf[6])
        max_rate = torch.where(second, torch.maximum(sf[7], (steer - sf[16]).abs() / dt), sf[7])
        xte_sum = sf[8] + xte
        rms = _sqrt(jerk_sum / torch.where(second, steps - 1, torch.ones_like(steps)).to(torch.float64))
        run_f = [torch.minimum(sf[0], centre), torch.minimum(sf[1], box), torch.minimum(sf[2], ttc),
                 torch.maximum(sf[3], alon.abs()), torch.maximum(sf[4], alat.abs()), jerk_sum, max_jerk, max_rate, xte_sum,
                 torch.maximum(sf[9], xte)]
        new_i = torch.stack([steps, ttc_steps, close_steps, brake_steps])
        new_f = torch.stack(run_f[:5] + [torch.where(second, rms, torch.zeros_like(rms)), max_jerk, max_rate,
                                         xte_sum / steps.to(torch.float64), run_f[9]])
        j = si[4]
        done = done.bool()
        write = done & (j < Q)
        slot = torch.arange(B, device=self.device) * Q + torch.clamp(j, max=Q - 1).long()
        for rec, new in ((self.rec_i32.view(4, B * Q), new_i), (self.rec_f64.view(10, B * Q), new_f)):
            rec[:, slot] = torch.where(write, new, rec[:, slot])
        keep = ~done
        for i in range(4):
            si[i] = torch.where(keep, new_i[i], torch.zeros_like(new_i[i]))
        si[4] = j + i32(write)
        for i, v in enumerate(run_f):
            sf[i] = torch.where(keep, v, torch.full_like(v, float("inf") if i < 3 else 0.0))
        for i, v in enumerate(carry(ax, ay, steer)):
            sf[10 + i] = v

    def records(self) -> dict:
        return drive_records_from_planes(self.rec_i32.cpu().numpy(), self.rec_f64.cpu().numpy())


@dataclass
class EvalResult:
    """records: dict of numpy arrays [B, Q] (steps, success, collision, truncated, avg_speed, return, unsolved, max_iters);
    steps: policy steps the batch took; env_steps = steps * B; seconds: host clock around the stepping loop (it ends in a
    synchronise); drive: the drive metrics' records (dict of numpy arrays [B, Q], keys DRIVE_I32 + DRIVE_F64; slot [b, j]
    is the episode of records' slot [b, j]) when the evaluation ran with metrics=True, else None."""
    records: dict
    dt: float
    steps: int
    env_steps: int
    seconds: float
    drive: dict | None = None

    @property
    def travel_time(self):
        return self.records["steps"] * self.dt                        # model_comparison.py:89

    def summary(self) -> dict:
        """model_comparison.py:195-199 over the B Q episodes (rates in %, means over episodes, the average speed as the mean of
        the per-episode means), plus mean_return, unsolved_frac (unsolved solves / steps of the recorded episodes), episodes,
        env_steps, seconds and env_steps_per_s.  With the drive metrics also: near_miss_rate (% of all episodes that had no
        collision and a min_box_gap below CLOSE_GAP), min_box_gap_mean and min_ttc_median over the episodes where the value
        is finite (inf when there is none), episodes_with_traffic (episodes with a finite min_box_gap), ttc_exposure and
        hard_brake_rate (steps below TTC_THRESHOLD / braking harder than HARD_BRAKE, over all steps), the means over
        episodes max_abs_alon_mean, max_abs_alat_mean, rms_jerk_mean, max_steer_rate_mean, mean_xte, and max_xte (the
        largest of any episode)."""
        out = self._base_summary()
        if self.drive is not None:
            out.update(self._drive_summary())
        return out

    def _drive_summary(self) -> dict:
        r, d = self.records, self.drive
        n = int(d["steps"].size)
        steps_total = max(int(d["steps"].sum()), 1)
        with_traffic = np.isfinite(d["min_box_gap"])
        ttc = d["min_ttc"][np.isfinite(d["min_ttc"])]
        mean = lambda k: float(d[k].mean())
        return dict(near_miss_rate=int((~r["collision"] & (d["min_box_gap"] < CLOSE_GAP)).sum()) / n * 100,
                    min_box_gap_mean=float(d["min_box_gap"][with_traffic].mean()) if with_traffic.any() else float("inf"),
                    min_ttc_median=float(np.median(ttc)) if ttc.size else float("inf"),
                    episodes_with_traffic=int(with_traffic.sum()),
                    ttc_exposure=int(d["ttc_steps"].sum()) / steps_total,
                    hard_brake_rate=int(d["hard_brake_steps"].sum()) / steps_total,
                    max_abs_alon_mean=mean("max_abs_alon"), max_abs_alat_mean=mean("max_abs_alat"),
                    rms_jerk_mean=mean("rms_jerk"), max_steer_rate_mean=mean("max_steer_rate"), mean_xte=mean("mean_xte"),
                    max_xte=float(d["max_xte"].max()))

    def _base_summary(self) -> dict:
        r = self.records
        n = int(r["steps"].size)
        tot = lambda a: sum(float(x) for x in np.asarray(a).ravel())  # episode by episode, as the reference accumulates
        steps_total = int(r["steps"].sum())
        return dict(success_rate=tot(r["success"]) / n * 100, collision_rate=tot(r["collision"]) / n * 100,
                    avg_steps=tot(r["steps"]) / n, avg_speed=tot(r["avg_speed"]) / n, avg_travel_time=tot(self.travel_time) / n,
                    mean_return=tot(r["return"]) / n, unsolved_frac=int(r["unsolved"].sum()) / max(steps_total, 1),
                    episodes=n, env_steps=self.env_steps, seconds=self.seconds,
                    env_steps_per_s=self.env_steps / self.seconds if self.seconds > 0 else float("inf"))


def _engine_of(agent):
    e = getattr(agent, "_engine", None)
    return e if e is not None else getattr(agent, "engine", None)


def _env_state_names(env):
    return [n for n in ("ego", "opos", "ospeed", "ohead", "oactive", "oroute", "oprog", "otarget", "t", "rng_counter")
            if hasattr(env, n)]


@torch.no_grad()
def evaluate_agent(agent, env, episodes_per_env: int = 1, deterministic: bool = False, reset_mpc_on_done: bool = False,
                   use_graph: bool | None = None, poll_every: int = 16, seed: int = 0, on_step=None,
                   metrics: bool = False) -> EvalResult:
    """Run `agent` in closed loop on the B environments of `env` (a SyntheticIntersectionEnv) until each environment has
    finished `episodes_per_env` episodes; returns their records.

    agent: PureMPC_Agent, IterativeLinearMPC_Agent or MPCRLAgent (anything with `act_batch_torch`).  The MPC's action goes to the
    environment in physical units (acceleration m/s^2, steering rad), as in the collector; the reference divides it by 5 and
    pi / 3 (model_comparison.py:55) only because highway-env's ContinuousAction rescales it again.
    deterministic: MPC-RL policies act with their mean; otherwise they sample, keyed by `seed` (and the environment's global id
    on the fused path).  reset_mpc_on_done=False keeps the detector memory / the LTV profile across episodes, like the
    reference's single agent object; True forgets it when an environment restarts.  An agent with warm_start always forgets
    its warm-start memory there.  use_graph (None: with the HIP environment): capture the step once as a hipGraph and replay
    it.  poll_every: steps between reads of the device's episode count.  on_step(inputs): called with the accounting's inputs
    after the reset and after every step (eager path only; tensors, valid until the next step).
    metrics=True: also the safety and comfort metrics of every episode (`DriveMetrics`, EvalResult.drive), updated after the
    accounting inside the step (so inside the captured graph); on_step's dict then also holds terminal_obs, obs and act.
    Every episode ends by EPISODE_STEPS (200) steps, so Q * 200 steps bound the loop; RuntimeError if the episodes are not
    all recorded by then."""
    Q = int(episodes_per_env)
    if Q < 1:
        raise ValueError("episodes_per_env must be >= 1")
    if int(poll_every) < 1:
        raise ValueError("poll_every must be >= 1")
    if not callable(getattr(agent, "act_batch_torch", None)):
        raise ValueError(f"unsupported agent {type(agent).__name__}: needs act_batch_torch (PureMPC_Agent, "
                         "IterativeLinearMPC_Agent, MPCRLAgent)")
    B, dev = env.num_envs, env.device
    hip = getattr(env, "backend", "torch") == "hip"
    eng = _engine_of(agent)
    if use_graph is None:
        use_graph = hip and hasattr(eng, "reserve_envs")
    if use_graph and not hip:
        raise ValueError("use_graph needs the HIP environment on a GPU")
    if use_graph and on_step is not None:
        raise ValueError("on_step needs the eager path (use_graph=False)")
    warm = bool(getattr(agent, "warm_start", False))
    stats = EpisodeStats(B, Q, dev, "hip" if hip else "torch")
    obs = torch.zeros((B, VEHICLES_COUNT, 8), dtype=torch.float32, device=dev)     # the observation the agent acts on
    drive = DriveMetrics(B, Q, dev, "hip" if hip else "torch", env.ref_xy, env.dt, VEHICLES_COUNT) if metrics else None
    kw = dict(deterministic=bool(deterministic), seed=int(seed), env_offset=int(getattr(env, "env_offset", 0)))

    def step():
        out = agent.act_batch_torch(obs, **kw)
        new_obs, reward, done, info = env.step(out["act"])
        if reset_mpc_on_done:
            eng.reset_env_mask_torch(_u8(done))
        elif warm:                    # a new episode must not start from the old one's plan
            eng.reset_env_mask_torch(_u8(done), warm_only=True)
        inputs = dict(ego=env.ego, done=done, truncated=info["truncated"], crashed=info["crashed"], arrived=info["arrived"],
                      reward=reward, status=out["status"], iters=out["iters"])
        stats.update(**inputs, step_counter=out.get("step"))
        if drive is not None:
            drive.update(info["terminal_obs"], new_obs, out["act"], done)
            inputs.update(terminal_obs=info["terminal_obs"], obs=new_obs, act=out["act"])
        obs.copy_(new_obs)
        return out, inputs

    graph = None
    if use_graph:
        # warm-up and capture really step the environment: its state is put back afterwards, and the resets below start the
        # evaluation from there, so a graph run and an eager run see the same episodes
        eng.reserve_envs(B)
        names = _env_state_names(env)
        snap = {n: getattr(env, n).clone() for n in names}
        gen_state = env.gen.get_state()
        obs.copy_(env.reset())
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(2):                       # allocations and lazy initialisation outside the capture
                out, _ = step()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        if out.get("generator") is not None:
            graph.register_generator_state(out["generator"])
        with torch.cuda.graph(graph, stream=side):
            step()
        torch.cuda.synchronize(dev)
        for n in names:
            getattr(env, n).copy_(snap[n])
        env.gen.set_state(gen_state)

    obs.copy_(env.reset())
    if hasattr(agent, "reset_env_state"):
        agent.reset_env_state()
    elif hasattr(eng, "reset_env_state"):
        eng.reset_env_state()
    if hasattr(agent, "restart_actions"):
        agent.restart_actions()
    stats.update(env.ego, reset=True)
    if drive is not None:
        drive.update(None, obs, None, None, reset=True)
    if on_step is not None:
        on_step(dict(reset=True, ego=env.ego, obs=obs) if drive is not None else dict(reset=True, ego=env.ego))
    target, max_steps = B * Q, Q * EPISODE_STEPS
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    n, recorded = 0, 0
    while n < max_steps:
        if graph is not None:
            graph.replay()
        else:
            _, inputs = step()
            if on_step is not None:
                on_step(inputs)
        n += 1
        if n % int(poll_every) == 0 or n == max_steps:
            recorded = int(stats.recorded.item())          # one small copy to the host (synchronises)
            if recorded >= target:
                break
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    seconds = time.perf_counter() - t0
    if recorded < target:
        raise RuntimeError(f"only {recorded} of {target} episodes recorded after {n} steps (bound {max_steps})")
    return EvalResult(records=stats.records(), dt=float(env.dt), steps=n, env_steps=n * B, seconds=seconds,
                      drive=None if drive is None else drive.records())


def compare(agents: dict, make_env, episodes_per_env: int = 1, metrics: bool = False, **kw) -> dict:
    """Evaluate every agent on a fresh environment from make_env() (same seed: the HIP environment keys its draws by seed and
    environment id, so every agent meets the same initial episodes) -> {name: summary}; metrics=True adds the drive metrics'
    keys to every summary."""
    return {name: evaluate_agent(agent, make_env(), episodes_per_env, metrics=metrics, **kw).summary()
            for name, agent in agents.items()}
