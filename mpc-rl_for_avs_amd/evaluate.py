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

`perception=` puts a perception model (csrc/mpc_perception.hpp, `Perception`) between the environment and the agent: limited
range, occlusion by vehicles and by buildings (`corner_buildings`), dropout and bounded noise.  The agent acts on what is
seen; the accounting and the drive metrics keep reading the true scene.

`interaction=True` (reactive traffic only) adds the interaction metrics of csrc/mpc_interaction.hpp to every episode
(`InteractionMetrics`: how often another vehicle yields to the ego, how hard the ego makes it brake, the speed that costs the
traffic, post-encroachment times where a traffic route crosses the ego's), computed per step from the simulator's own slots
inside the same captured step (mpc_interaction_metrics), or by the same update in numpy on the CPU path.

`trace=` keeps the step-by-step record of the episodes someone will look at (csrc/mpc_episode_trace.hpp, `EpisodeTrace`): the
last `window` steps - scenes, actions, rewards, the solve's status, the flags, and with a perception model what the agent saw - of
the episodes that ended with one of the outcomes in `keep`, in a store of `capacity` episodes on the device, filled inside the
same captured step (mpc_episode_trace) in an order that does not depend on timing, or by the same update in numpy on the CPU path.

`tracker=` puts a tracker (csrc/mpc_tracker.hpp, `Tracker`) behind the perception model, or behind the true observation: a
vehicle that vanishes for a few steps stays in the agent's observation, moved on with its last velocity, the noise is smoothed,
and every row the agent gets has an identity (`row_slot`), inside the same captured step (mpc_track_rows), or by the same update
in numpy on the CPU path.

`actuation=` puts an actuator model (csrc/mpc_actuator.hpp, `Actuation`) between the agent and the environment: transport
delay, lost commands, calibration error, noise, first-order lag, rate limits and saturation.  The environment is handed the
applied action instead of the command, inside the same captured step (mpc_actuate), or by the same update in numpy on the CPU
path; every observer's `act` is then the applied action, what the environment was handed.

`plan=` asks the MPC agent for the plan behind every action (mpc_predict_batch_plan / mpc_ltv_predict_batch_plan: the planned
states and controls the solve ended with) and scores it against what happened (csrc/mpc_plan.hpp, `PlanMetrics`): the planned
clearance to the vehicles the agent saw, the ego's distance from where earlier plans put it, and the jump between consecutive
plans, per episode, inside the same captured step (mpc_plan_metrics), or by the same update in numpy on the CPU path.  A trace
recorder with plan=True keeps the plan of every step of the episodes it keeps (mpc_plan_trace).

`compensation=` puts a delay compensator (csrc/mpc_compensate.hpp, `Compensation`) in front of the agent: the agent's command
takes effect `steps` policy steps after the scene it was computed from, so the agent acts on the scene predicted to that moment
- the ego rolled through the commands still in flight with the environment's own vehicle model behind the nominal actuator, the
others moved on with their observed velocity - inside the same captured step (mpc_compensate), or by the same update in numpy
on the CPU path.

`latency=` puts a sensing latency (csrc/mpc_latency.hpp, `Latency`) in front of all of that: the perception model, the tracker
and the agent are handed the true scene of `steps` policy steps ago, inside the same captured step (mpc_delay_scene), or by the
same update in numpy on the CPU path.  A compensator that is told of it (`Compensation(latency=...)`, mpc_compensate_stale)
rolls the ego through the commands issued since that scene as well.
"""
from __future__ import annotations

import ctypes
import inspect
import math
import time
from dataclasses import dataclass

import numpy as np
import torch

from . import engine as _engine
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
# csrc/mpc_perception.hpp: the classes of a row, the planes of `counts`, the salt of the draws, sqrt(3), slots per row
ROW_ABSENT, ROW_SEEN, ROW_OUT_OF_RANGE, ROW_OCCLUDED, ROW_DROPPED = 0, 1, 2, 3, 4
PERCEPTION_COUNTS = ("present", "seen", "out_of_range", "occluded", "dropped")      # mpc_perceive counts [5][B]
PERCEPTION_SALT, UNIT_SCALE, ROW_SLOTS, MAX_OCCLUDERS = 0xC2B2AE3D27D4EB4F, 1.7320508075688772, 32, 8
# csrc/mpc_interaction.hpp: the records, this project's critical post-encroachment time [s], traffic routes, vehicle slots, the
# layout of the running state (counters and previous mask, carried routes; counters, carried arc length, pass times, carried oprog)
INTERACT_I32 = ("steps", "yield_steps", "forced_brake_steps", "forced_brake_events", "conflicts", "pet_critical",
                "ego_first")                                                        # mpc_interaction_metrics rec_i32 [7][B][Q]
INTERACT_F64 = ("max_forced_decel", "speed_deficit", "min_pet")                     # rec_f64 [3][B][Q]
PET_CRITICAL, ROUTES, SLOTS = 1.5, 12, 9
INTERACT_STATE_I32, INTERACT_STATE_F64 = 9 + SLOTS, 4 + ROUTES + 2 * SLOTS
# csrc/mpc_episode_trace.hpp: the outcome bits an EpisodeTrace keeps by name, the columns of its index, its counts, the flag
# bits of a frame, the largest window
TRACE_KEEP = dict(collision=1, truncated=2, success=4, unsolved=8, all=16, failed=3)
TRACE_INDEX = ("env", "ordinal", "steps", "first", "outcome", "launch")             # mpc_episode_trace index [C][6]
TRACE_COUNTS = ("matched", "kept", "dropped", "launches")                           # counts [4]
TRACE_FLAGS = dict(done=1, truncated=2, crashed=4, arrived=8)
TRACE_MAX_WINDOW = 4096
# csrc/mpc_tracker.hpp: the planes of `counts`, the slots per environment, the longest coast, row_slot of a row without a slot
TRACKER_COUNTS = ("measured", "matched", "born", "coasted", "expired", "evicted", "cut")   # mpc_track_rows counts [7][B]
TRACK_SLOTS, TRACK_MAX_COAST, TRACK_NO_SLOT = 16, 200, 255
# csrc/mpc_actuator.hpp: the planes of `counts`, the salt of the draws, the ring's length, the longest delay, the planes of
# `state` that hold what reached the actuator last and what was applied last; the environment's own clamp of the two channels
# (csrc/mpc_synth_env.hpp::step_ego)
ACTUATION_COUNTS = ("steps", "held", "rate_limited", "saturated", "nonfinite")             # mpc_actuate counts [5][B]
ACTUATION_SALT, ACT_RING, ACT_MAX_DELAY, ACT_LAST, ACT_PREV = 0x9FB21C651E98DF25, 8, 7, 8, 9
ENV_LIMITS = ((-5.0, 5.0), (-math.pi / 4, math.pi / 4))
# csrc/mpc_compensate.hpp: the ring's length, the longest look-ahead; csrc/mpc_synth_env.hpp::step_ego: the wheelbase and the
# largest speed
COMP_RING, COMP_MAX_STEPS, ENV_WHEELBASE, ENV_MAX_SPEED = 8, 7, 2.5, 30.0
# csrc/mpc_latency.hpp: the ring's length, the longest latency
LAT_RING, LAT_MAX_STEPS = 8, 7
# csrc/mpc_plan.hpp: the records of mpc_plan_metrics (lead{i}: the i-th of its four leads), the planes of its running state,
# the leads per launch, MPC_MAX_HORIZON
PLAN_I32 = ("steps", "plans_valid", "plan_conflict_steps", "replan_n") + tuple(f"lead{i}_n" for i in range(4))   # rec_i32 [8][B][Q]
PLAN_F64 = ("min_plan_gap", "replan_accel_mean", "replan_steer_mean", "replan_accel_max", "replan_steer_max") + \
    tuple(f"lead{i}_mean" for i in range(4)) + tuple(f"lead{i}_max" for i in range(4))                           # rec_f64 [13][B][Q]
PLAN_STATE_I32, PLAN_STATE_F64, PLAN_LEADS, PLAN_MAX_HORIZON = 10, 15, 4, 64


def records_from_planes(rec_i32, rec_f64, names_i32=REC_I32, names_f64=REC_F64, bools=_BOOL) -> dict:
    """Record planes (include/mpc_mi355x.h layout) -> dict of numpy arrays [B, Q]: plane i of rec_i32 under names_i32[i] (as
    bool for the names in `bools`), plane i of rec_f64 under names_f64[i].  The defaults are the accounting's records; the
    drive metrics' are (DRIVE_I32, DRIVE_F64), the interaction metrics' (INTERACT_I32, INTERACT_F64)."""
    rec_i32, rec_f64 = np.asarray(rec_i32), np.asarray(rec_f64)
    out = {k: (rec_i32[i] != 0) if k in bools else rec_i32[i].copy() for i, k in enumerate(names_i32)}
    out.update({k: rec_f64[i].copy() for i, k in enumerate(names_f64)})
    return out


def _solved(status):
    return (status == 0) | ((status >= 5) & (status <= 7))       # MPC_STATUS_IS_SOLVED


def _u8(t):
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def _check(t, name, shape, dtype, device):
    """`t` as the kernels read it (a bool tensor's bytes where uint8 is wanted); ValueError unless it is a contiguous tensor
    of that dtype and shape on that device.  Every `update` / `apply` checks what it is given with this before it
    dispatches: on the "hip" backend the tensor's address goes to a kernel as it is."""
    if t is not None and dtype == torch.uint8:
        t = _u8(t)
    if t is None or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != device:
        raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {shape} on {device}")
    return t


def _write_back(pairs):
    """Every numpy result `src` of (dst, src) into its tensor `dst`, unless it already is that tensor's memory (on the CPU
    `dst.cpu().numpy()` is)."""
    for dst, src in pairs:
        src = torch.from_numpy(np.ascontiguousarray(src))
        if dst.data_ptr() != src.data_ptr():
            dst.copy_(src)


def _route(ref_xy):
    """The ego's route ref_xy [M, 2], 1 <= M <= MAX_ROUTE -> (ref, e0, d), f64 on the CPU: the points, and of its max(M - 1,
    1) segments the start and end - start (a single point is one segment of length 0)."""
    if ref_xy is None:
        raise ValueError("the ego's route ref_xy [M, 2] is needed")
    ref = torch.as_tensor(ref_xy, dtype=torch.float64).cpu().contiguous()
    if ref.ndim != 2 or ref.shape[1] != 2 or not 1 <= ref.shape[0] <= MAX_ROUTE:
        raise ValueError(f"ref_xy must be [M, 2] with 1 <= M <= {MAX_ROUTE}")
    M = ref.shape[0]
    nseg = max(M - 1, 1)
    return ref, ref[:nseg], ref[torch.clamp(torch.arange(nseg) + 1, max=M - 1)] - ref[:nseg]


class _EpisodeAccounts:
    """What the per-episode accounts share (the rule of csrc/mpc_episode_stats.hpp): the running state of every environment
    (state_i32 [n_i32, B], state_f64 [n_f64, B]) and the records of its first Q episodes (rec_i32 [len(names_i32), B, Q],
    rec_f64 [len(names_f64), B, Q]) as device tensors in the layout of include/mpc_mi355x.h.  An episode that ends with
    ordinal j < Q is written to slot [b][j]; `done` clears the running counters and advances the ordinal up to the quota."""
    _ORDINAL = 4                                         # the plane of state_i32 that `_torch_commit` keeps the ordinal in

    def __init__(self, B: int, Q: int, device, backend: str, n_i32: int, n_f64: int, names_i32, names_f64):
        if Q < 1:
            raise ValueError("episodes_per_env must be >= 1")
        if backend not in ("hip", "torch"):
            raise ValueError("backend must be 'hip' or 'torch'")
        self.B, self.Q, self.device, self.backend = int(B), int(Q), torch.device(device), backend
        self._names = (names_i32, names_f64)
        z = lambda *s, dt: torch.zeros(s, dtype=dt, device=self.device)
        self.state_i32, self.state_f64 = z(n_i32, B, dt=torch.int32), z(n_f64, B, dt=torch.float64)
        self.rec_i32, self.rec_f64 = z(len(names_i32), B, Q, dt=torch.int32), z(len(names_f64), B, Q, dt=torch.float64)

    def _torch_commit(self, done, new_i32, new_f64):
        """The record commit in torch ops: the rows new_i32 [len(names_i32), B] and new_f64 [len(names_f64), B] go to slot
        [b][j] where `done` and j < Q, and the ordinal advances there.  Returns (write, keep): where a record was written,
        and where the episode goes on (the caller clears its running counters elsewhere)."""
        B, Q = self.B, self.Q
        j = self.state_i32[self._ORDINAL]
        done = done.bool()
        write = done & (j < Q)
        slot = torch.arange(B, device=self.device) * Q + torch.clamp(j, max=Q - 1).long()
        for rec, new in ((self.rec_i32, new_i32), (self.rec_f64, new_f64)):
            rec = rec.view(rec.shape[0], B * Q)
            rec[:, slot] = torch.where(write, new, rec[:, slot])
        self.state_i32[self._ORDINAL] = j + write.to(torch.int32)
        return write, ~done

    def records(self) -> dict:
        return records_from_planes(self.rec_i32.cpu().numpy(), self.rec_f64.cpu().numpy(), *self._names)


class EpisodeStats(_EpisodeAccounts):
    """Running state and records of the accounting, as device tensors in the layout of mpc_episode_stats
    (include/mpc_mi355x.h); `update` is the kernel (backend "hip") or the same update in torch ops (backend "torch")."""

    def __init__(self, B: int, Q: int, device, backend: str = "torch"):
        # state_i32: steps, crashed, unsolved, max_iters, ordinal; state_f64: speed sum, return, carry_speed
        super().__init__(B, Q, device, backend, 5, 3, REC_I32, REC_F64)
        self.recorded = torch.zeros(1, dtype=torch.int64, device=self.device)

    def observe(self, frame, reset=False):
        f = frame.get
        self.update(frame["ego"], f("done"), f("truncated"), f("crashed"), f("arrived"), f("reward"), f("status"), f("iters"),
                    reset=reset, step_counter=f("step"))

    def update(self, ego, done=None, truncated=None, crashed=None, arrived=None, reward=None, status=None, iters=None,
               reset=False, step_counter=None):
        B, dev = self.B, self.device
        _check(ego, "ego", (B, 4), torch.float64, dev)
        if step_counter is not None:
            _check(step_counter, "step_counter", (1,), torch.int64, dev)
        if not reset:
            done, truncated, crashed, arrived = [
                _check(t, n, (B,), torch.uint8, dev)
                for n, t in (("done", done), ("truncated", truncated), ("crashed", crashed), ("arrived", arrived))]
            _check(reward, "reward", (B,), torch.float32, dev)
            _check(status, "status", (B,), torch.int32, dev)
            _check(iters, "iters", (B,), torch.int32, dev)
        if self.backend == "torch":
            self._torch_update(ego, done, truncated, crashed, arrived, reward, status, iters, reset)
            if step_counter is not None and not reset:
                step_counter += 1
            return
        _engine.caller("mpc_episode_stats")(
            device=self.device.index, B=self.B, Q=self.Q, reset=1 if reset else 0, done=done, truncated=truncated,
            crashed=crashed, arrived=arrived, reward=reward, ego=ego, status=status, iters=iters, state_i32=self.state_i32,
            state_f64=self.state_f64, rec_i32=self.rec_i32, rec_f64=self.rec_f64, recorded=self.recorded,
            step_counter=step_counter, stream=_engine.current_stream(self.device))

    @torch.no_grad()
    def _torch_update(self, ego, done, truncated, crashed, arrived, reward, status, iters, reset):
        si, sf = self.state_i32, self.state_f64
        if reset:
            si.zero_()
            sf[:2].zero_()
            sf[2].copy_(ego[:, 3])
            self.recorded.zero_()
            return
        steps = si[0] + 1
        crash = (si[1] != 0) | crashed.bool()
        unsolved = si[2] + (~_solved(status)).to(torch.int32)
        max_iters = torch.maximum(si[3], iters)
        speed_sum = sf[0] + sf[2]
        ret = sf[1] + reward.to(torch.float64)
        i32 = lambda t: t.to(torch.int32)
        new_i = torch.stack([steps, i32(arrived.bool()), i32(crash), i32(truncated.bool()), unsolved, max_iters])
        write, keep = self._torch_commit(done, new_i, torch.stack([speed_sum / steps, ret]))
        self.recorded += write.sum()
        for i, t in enumerate((steps, i32(crash), unsolved, max_iters)):
            si[i] = torch.where(keep, t, torch.zeros_like(t))
        sf[0] = torch.where(keep, speed_sum, torch.zeros_like(speed_sum))
        sf[1] = torch.where(keep, ret, torch.zeros_like(ret))
        sf[2] = ego[:, 3]


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


class DriveMetrics(_EpisodeAccounts):
    """Running state and records of the safety and comfort metrics, as device tensors in the layout of mpc_drive_metrics
    (include/mpc_mi355x.h; formulas in csrc/mpc_drive_metrics.hpp); `update` is the kernel (backend "hip") or the same update
    in elementwise torch ops (backend "torch": every dot product written a*b + c*d, no reduction but min, so both agree bit
    for bit).  ref_xy [M, 2]: the ego's route; dt: the step length; rows: rows of an observation (ego + others)."""

    def __init__(self, B: int, Q: int, device, backend: str = "torch", ref_xy=None, dt: float = 0.1,
                 rows: int = VEHICLES_COUNT):
        if not 1 <= int(rows) <= MAX_ROWS:
            raise ValueError(f"rows must be 1..{MAX_ROWS}")
        if not float(dt) > 0:
            raise ValueError("dt must be > 0")
        ref, e0, d = _route(ref_xy)
        # state_i32: steps, ttc_steps, close_steps, hard_brake_steps, ordinal; state_f64: ten running values, then the
        # carries vx vy cos sin ax ay steer
        super().__init__(B, Q, device, backend, 5, 17, DRIVE_I32, DRIVE_F64)
        self.dt, self.rows, self.M = float(dt), int(rows), int(ref.shape[0])
        self.ref_xy, self._e0, self._d = ref.to(self.device), e0.to(self.device), d.to(self.device)

    def observe(self, frame, reset=False):
        self.update(frame.get("terminal_obs"), frame["obs"], frame.get("act"), frame.get("done"), reset)

    def update(self, terminal_obs, obs, action, done, reset=False):
        B, R, dev = self.B, self.rows, self.device
        _check(obs, "obs", (B, R, 8), torch.float32, dev)
        if not reset:
            _check(terminal_obs, "terminal_obs", (B, R, 8), torch.float32, dev)
            _check(action, "action", (B, 2), torch.float64, dev)
            done = _check(done, "done", (B,), torch.uint8, dev)
        if self.backend == "torch":
            self._torch_update(terminal_obs, obs, action, done, reset)
            return
        _engine.caller("mpc_drive_metrics")(
            device=self.device.index, B=B, R=R, Q=self.Q, M=self.M, reset=1 if reset else 0, dt=self.dt,
            terminal_obs=None if reset else terminal_obs, obs=obs, action=None if reset else action,
            done=None if reset else done, ref_xy=self.ref_xy, state_i32=self.state_i32, state_f64=self.state_f64,
            rec_i32=self.rec_i32, rec_f64=self.rec_f64, stream=_engine.current_stream(self.device))

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
        si, sf, dt = self.state_i32, self.state_f64, self.dt
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
        _, keep = self._torch_commit(done, new_i, new_f)
        for i in range(4):
            si[i] = torch.where(keep, new_i[i], torch.zeros_like(new_i[i]))
        for i, v in enumerate(run_f):
            sf[i] = torch.where(keep, v, torch.full_like(v, float("inf") if i < 3 else 0.0))
        for i, v in enumerate(carry(ax, ay, steer)):
            sf[10 + i] = v


def default_leads(N: int) -> tuple:
    """The leads `plan=True` scores: 1, N // 4, N // 2, N with duplicates and zeros dropped."""
    out = []
    for h in (1, int(N) // 4, int(N) // 2, int(N)):
        if h > 0 and h not in out:
            out.append(h)
    return tuple(out)


class PlanMetrics(_EpisodeAccounts):
    """The MPC's plan against what happened, per episode (csrc/mpc_plan.hpp states the update step by step; layouts in
    include/mpc_mi355x.h, mpc_plan_metrics): the planned clearance to where the vehicles the agent saw will be, the distance
    between where the ego ended up and where the plans of `leads` steps ago put it, and the jump between a plan's first
    control and what the previous plan intended for this step.  N: the horizon of the plans; R: rows of an observation; leads:
    up to four leads in 1..N (None: default_leads(N)); gap [m]: a step whose planned clearance is below it is a planned
    conflict (default: the environment's crash distance).  A plan whose status is not solved is counted and skipped.
    `update` after the environment's step is the kernel (backend "hip": enqueue only, capturable) or the same update in numpy
    (backend "torch", for the CPU environment); both give the same bits."""

    def __init__(self, B: int, Q: int, device, backend: str = "torch", N: int = 20, R: int = VEHICLES_COUNT, dt: float = 0.1,
                 leads=None, gap: float = CRASH_DISTANCE):
        N = int(N)
        if not 1 <= N <= PLAN_MAX_HORIZON:
            raise ValueError(f"N must be 1..{PLAN_MAX_HORIZON}")
        if not 1 <= int(R) <= MAX_ROWS:
            raise ValueError(f"R must be 1..{MAX_ROWS}")
        if not float(dt) > 0:
            raise ValueError("dt must be > 0")
        if not float(gap) >= 0:
            raise ValueError("gap must be >= 0")
        leads = default_leads(N) if leads is None else tuple(int(h) for h in leads)
        if not 1 <= len(leads) <= PLAN_LEADS or any(h < 0 for h in leads) or not any(leads):
            raise ValueError(f"leads: 1..{PLAN_LEADS} leads, each >= 1 (0: unused), at least one used")
        if max(leads) > N:
            raise ValueError(f"leads {leads} reach beyond the horizon {N}")
        super().__init__(B, Q, device, backend, PLAN_STATE_I32, PLAN_STATE_F64, PLAN_I32, PLAN_F64)
        self.N, self.R, self.dt, self.gap = N, int(R), float(dt), float(gap)
        self.leads = leads + (0,) * (PLAN_LEADS - len(leads))
        self.Lmax = max(self.leads)
        self.ring_xy = torch.zeros((self.B, self.Lmax, PLAN_LEADS, 2), dtype=torch.float64, device=self.device)
        self.ring_valid = torch.zeros((self.B, self.Lmax), dtype=torch.int32, device=self.device)

    @property
    def config(self) -> dict:
        """The keyword arguments that make a PlanMetrics with the same settings."""
        return dict(N=self.N, R=self.R, dt=self.dt, leads=tuple(h for h in self.leads if h), gap=self.gap)

    def observe(self, frame, reset=False):
        f = frame.get
        self.update(f("plan_X"), f("plan_U"), f("status"), f("acted"), f("terminal_obs"), f("done"), f("plan_order", 0), reset)

    def update(self, plan_X, plan_U, status, acted, terminal_obs, done, order: int = 0, reset: bool = False):
        B, N, R, dev = self.B, self.N, self.R, self.device
        if order not in (0, 1):
            raise ValueError("order must be 0 (x, y, theta, v) or 1 (x, y, v, yaw)")
        if reset:
            plan_X = plan_U = status = acted = terminal_obs = done = None
        else:
            _check(plan_X, "plan_X", (B, N + 1, 4), torch.float64, dev)
            _check(plan_U, "plan_U", (B, N, 2), torch.float64, dev)
            _check(status, "status", (B,), torch.int32, dev)
            _check(acted, "acted", (B, R, 8), torch.float32, dev)
            _check(terminal_obs, "terminal_obs", (B, R, 8), torch.float32, dev)
            done = _check(done, "done", (B,), torch.uint8, dev)
        if self.backend == "torch":
            self._numpy_update(plan_X, plan_U, status, acted, terminal_obs, done, reset)
            return
        l0, l1, l2, l3 = self.leads
        _engine.caller("mpc_plan_metrics")(
            device=self.device.index, B=B, N=N, R=R, Q=self.Q, reset=1 if reset else 0, order=int(order), dt=self.dt,
            gap=self.gap, lead0=l0, lead1=l1, lead2=l2, lead3=l3, plan_X=plan_X, plan_U=plan_U, status=status, acted=acted,
            terminal_obs=terminal_obs, done=done, state_i32=self.state_i32, state_f64=self.state_f64, ring_xy=self.ring_xy,
            ring_valid=self.ring_valid, rec_i32=self.rec_i32, rec_f64=self.rec_f64, stream=_engine.current_stream(self.device))

    def _numpy_update(self, plan_X, plan_U, status, acted, terminal_obs, done, reset):
        """csrc/mpc_plan.hpp over the batch: every statement acts on all environments, in the header's order."""
        B, N, R, Q, L = self.B, self.N, self.R, self.Q, self.Lmax
        planes = (self.state_i32, self.state_f64, self.ring_xy, self.ring_valid, self.rec_i32, self.rec_f64)
        si, sf, ring, ring_valid, ri, rf = (t.cpu().numpy() for t in planes)
        inf = float("inf")
        if reset:
            si[:], sf[:], ring_valid[:] = 0, 0.0, 0
            sf[0] = inf
            _write_back(zip(planes, (si, sf, ring, ring_valid, ri, rf)))
            return
        X, U, a, term = (t.cpu().numpy() for t in (plan_X, plan_U, acted, terminal_obs))
        valid = _solved(status.cpu().numpy())
        done = done.cpu().numpy() != 0
        env, t = np.arange(B), si[0].copy()
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = np.full(B, inf)                                                   # 1
            if R > 1:
                a64 = a.astype(np.float64)
                kd = np.arange(1, N + 1).astype(np.float64) * self.dt
                qx = a64[:, None, 1:, 1] + kd[None, :, None] * a64[:, None, 1:, 3]
                qy = a64[:, None, 1:, 2] + kd[None, :, None] * a64[:, None, 1:, 4]
                ex, ey = X[:, 1:, None, 0] - qx, X[:, 1:, None, 1] - qy
                pair = np.where((a[:, None, 1:, 0] != 0) & valid[:, None, None], ex * ex + ey * ey, inf)
                d2 = pair.reshape(B, -1).min(axis=1)
            c = np.sqrt(d2)
            sf[0] = np.where(valid & (c < sf[0]), c, sf[0])
            si[2] += valid & (c < self.gap)
            si[0] = t + 1                                                          # 2
            si[1] += valid
            at = t % L                                                             # 3
            for i, h in enumerate(self.leads):
                if h > 0:
                    ring[env, at, i] = X[:, h, :2]
            ring_valid[env, at] = valid
            ox, oy = term[:, 0, 1].astype(np.float64), term[:, 0, 2].astype(np.float64)   # 4
            for i, h in enumerate(self.leads):
                if h < 1:
                    continue
                old = h <= t + 1
                p = np.where(old, t + 1 - h, 0) % L
                ok = old & (ring_valid[env, p] != 0)
                ex, ey = ox - ring[env, p, i, 0], oy - ring[env, p, i, 1]
                e = np.sqrt(ex * ex + ey * ey)
                si[5 + i] += ok
                sf[5 + i] = np.where(ok, sf[5 + i] + e, sf[5 + i])
                sf[9 + i] = np.where(ok & (e > sf[9 + i]), e, sf[9 + i])
            both = (t >= 1) & valid & (si[3] != 0)                                 # 5
            for ch in (0, 1):
                jump = np.abs(U[:, 0, ch] - sf[13 + ch])
                sf[1 + ch] = np.where(both, sf[1 + ch] + jump, sf[1 + ch])
                sf[3 + ch] = np.where(both & (jump > sf[3 + ch]), jump, sf[3 + ch])
            si[9] += both
            nxt = 1 if N > 1 else 0
            sf[13], sf[14], si[3] = U[:, nxt, 0], U[:, nxt, 1], valid
            j = si[4].copy()                                                       # 6
            w = np.nonzero(done & (j < Q))[0]
            mean = lambda total, n: np.where(n > 0, total / np.maximum(n, 1), 0.0)
            ri[0, w, j[w]], ri[1, w, j[w]], ri[2, w, j[w]], ri[3, w, j[w]] = si[0, w], si[1, w], si[2, w], si[9, w]
            rf[0, w, j[w]] = sf[0, w]
            for ch in (0, 1):
                rf[1 + ch, w, j[w]] = mean(sf[1 + ch, w], si[9, w])
                rf[3 + ch, w, j[w]] = sf[3 + ch, w]
            for i in range(PLAN_LEADS):
                ri[4 + i, w, j[w]] = si[5 + i, w]
                rf[5 + i, w, j[w]] = mean(sf[5 + i, w], si[5 + i, w])
                rf[9 + i, w, j[w]] = sf[9 + i, w]
        j[w] += 1
        si[:, done], sf[:, done], ring_valid[done] = 0, 0.0, 0
        sf[0, done] = inf
        si[4] = j
        _write_back(zip(planes, (si, sf, ring, ring_valid, ri, rf)))

    def records(self) -> dict:
        """The records (PLAN_I32 + PLAN_F64, numpy arrays [B, Q]) and `leads`, the four leads the lead{i}_* fields belong to."""
        return dict(super().records(), leads=self.leads)


def _wrap_pi(a):
    a = np.where(a > math.pi, a - 2.0 * math.pi, a)
    return np.where(a <= -math.pi, a + 2.0 * math.pi, a)


def route_pieces(route: int) -> list:
    """The centre line of traffic route 3 * entry + turn (csrc/mpc_synth_traffic.hpp: pose) from its entry to the end of the
    map, as pieces in the order they are driven: dicts with s0 (arc length where the piece begins), length, and either
    kind="line" (p0, unit direction u, heading h) or kind="arc" (centre c, radius R, axes a0 and a1 with point(phi) = c +
    R (a0 cos phi + a1 sin phi), heading h0 + sign * phi, phi = (s - s0) / R in [0, pi / 2])."""
    entry, turn = divmod(int(route), 3)
    d = np.array([(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)][entry])
    n = np.array([-d[1], d[0]])
    h0 = (0.0, math.pi / 2, math.pi, -math.pi / 2)[entry]
    if turn == 0:                                          # |coordinate| <= 65 until s = 125
        return [dict(kind="line", s0=0.0, length=125.0, p0=-60.0 * d + 2.0 * n, u=d, h=h0)]
    sign, R = (1.0, 8.0) if turn == 2 else (-1.0, 12.0)    # right: about -10 d + 10 n; left: about -10 d - 10 n
    arc = R * (math.pi / 2)
    end = (-2.0 * d + 10.0 * n) if turn == 2 else (2.0 * d - 10.0 * n)
    return [dict(kind="line", s0=0.0, length=50.0, p0=-60.0 * d + 2.0 * n, u=d, h=h0),
            dict(kind="arc", s0=50.0, length=arc, c=-10.0 * d + sign * 10.0 * n, R=R, a0=-sign * n, a1=d, h0=h0, sign=sign),
            dict(kind="line", s0=50.0 + arc, length=55.0, p0=end, u=sign * n, h=float(_wrap_pi(h0 + sign * math.pi / 2)))]


def conflict_points(ref_xy) -> np.ndarray:
    """[12, 2] = (sigma_c, s_c) per traffic route: the first point along the ego's polyline ref_xy [M, 2] at which the route's
    centre line crosses it with an angle between the two directions of at least pi / 4 (the corridor rule's threshold: merging
    and following are the IDM's business, not a crossing conflict), as arc length along the polyline and along the route;
    sigma_c = -1 (and s_c = -1) where there is none.  Segment against line and segment against arc, in closed form."""
    ref = np.asarray(ref_xy, dtype=np.float64)
    if ref.ndim != 2 or ref.shape[1] != 2 or ref.shape[0] < 1:
        raise ValueError("ref_xy must be [M, 2]")
    cross = lambda a, b: a[0] * b[1] - a[1] * b[0]
    out = np.full((ROUTES, 2), -1.0)
    eps = 1e-12
    for r in range(ROUTES):
        best = None
        sigma0 = 0.0
        for i in range(ref.shape[0] - 1):
            p0, e = ref[i], ref[i + 1] - ref[i]
            L = math.sqrt(e[0] * e[0] + e[1] * e[1])
            if L > 0.0:
                he = math.atan2(e[1], e[0])
                for pc in route_pieces(r):
                    hits = []                              # (parameter along the segment, arc length on the route, heading)
                    if pc["kind"] == "line":
                        det = cross(e, pc["u"])
                        if abs(det) > eps * L:
                            w = pc["p0"] - p0
                            hits.append((cross(w, pc["u"]) / det, cross(w, e) / det, pc["h"]))
                    else:
                        w = p0 - pc["c"]
                        qa, qb, qc = L * L, 2.0 * (w[0] * e[0] + w[1] * e[1]), w[0] * w[0] + w[1] * w[1] - pc["R"] ** 2
                        disc = qb * qb - 4.0 * qa * qc
                        if disc >= 0.0:
                            for a in ((-qb - math.sqrt(disc)) / (2.0 * qa), (-qb + math.sqrt(disc)) / (2.0 * qa)):
                                rel = (w + a * e) / pc["R"]
                                phi = math.atan2(rel[0] * pc["a1"][0] + rel[1] * pc["a1"][1],
                                                 rel[0] * pc["a0"][0] + rel[1] * pc["a0"][1])
                                hits.append((a, pc["R"] * phi, pc["h0"] + pc["sign"] * phi))
                    for a, c, h in hits:
                        if -eps <= a <= 1.0 + eps and -eps <= c <= pc["length"] + eps and \
                                abs(float(_wrap_pi(_wrap_pi(h) - he))) >= math.pi / 4:
                            sigma = sigma0 + min(max(a, 0.0), 1.0) * L
                            if best is None or sigma < best[0]:
                                best = (sigma, pc["s0"] + min(max(c, 0.0), pc["length"]))
            sigma0 += L
        if best is not None:
            out[r] = best
    return out


class _Leader:
    """mpc::env::Leader for B environments at once."""

    def __init__(self, B):
        self.ell = np.full(B, np.inf)
        self.head, self.speed = np.zeros(B), np.zeros(B)
        self.who = np.full(B, -2, np.int64)

    def offer(self, j, xj, yj, hj, cj, sj, c, cx, cy, ch, cv, valid):
        """mpc::env::offer_leader where `valid`"""
        ex, ey = cx - xj, cy - yj
        ell = ex * cj + ey * sj
        w = ey * cj - ex * sj
        take = valid & (ell > 0.0) & (ell <= 40.0) & (np.abs(w) <= 2.0) & (ell < self.ell)
        if c >= 0:
            take = take & (ell > 5.0) & ((c < j) | (np.abs(_wrap_pi(ch - hj)) < math.pi / 4))
        self.ell, self.head = np.where(take, ell, self.ell), np.where(take, ch, self.head)
        self.speed, self.who = np.where(take, cv, self.speed), np.where(take, c, self.who)

    def drop(self, where):
        """no_leader() where `where`"""
        self.ell, self.head = np.where(where, np.inf, self.ell), np.where(where, 0.0, self.head)
        self.speed, self.who = np.where(where, 0.0, self.speed), np.where(where, -2, self.who)


def _idm_acceleration(v, v0, hj, lead):
    """mpc::env::idm_acceleration"""
    r = v / v0
    r2 = r * r
    has = lead.who != -2
    gap = np.where(has, lead.ell, 10.0) - 5.0
    gap = np.where(gap < 0.1, 0.1, gap)
    dv = v - lead.speed * np.cos(lead.head - hj)
    dyn = v * 1.5 + v * dv / 7.745966692414834
    dyn = np.where(dyn < 0.0, 0.0, dyn)
    q = (5.0 + dyn) / gap
    a = 3.0 * (1.0 - r2 * r2 - np.where(has, q * q, 0.0))
    return np.where(a < -6.0, -6.0, np.where(a > 3.0, 3.0, a))


def _drives_free(j, first, who):
    """The circle rule (mpc::env::walk_leaders, K steps) from vehicle j whose leader is first [B], along who [B, K]."""
    B, K = who.shape
    p, lowest, closed = first.copy(), np.full(B, j, np.int64), np.zeros(B, bool)
    rows = np.arange(B)
    for _ in range(K):
        go = (p >= 0) & ~closed
        closed = closed | (go & (p == j))
        go = go & ~closed
        lowest = np.where(go, np.minimum(lowest, p), lowest)
        p = np.where(go, who[rows, np.clip(p, 0, K - 1)], p)
    return closed & (lowest == j)


class InteractionMetrics(_EpisodeAccounts):
    """Running state and records of the interaction metrics, as device tensors in the layout of mpc_interaction_metrics
    (include/mpc_mi355x.h; formulas in csrc/mpc_interaction.hpp); `update(env, done)` after the environment's step is the
    kernel (backend "hip") or the same update in numpy on the CPU (backend "torch": the feature works wherever the environment
    does; cos and sin are numpy's, so it agrees with the kernel to their rounding).  It reads the slots of a
    SyntheticIntersectionEnv with traffic="idm".  ref_xy [M, 2]: the ego's route; dt: the step length; K: the other vehicles."""

    def __init__(self, B: int, Q: int, device, backend: str = "torch", ref_xy=None, dt: float = 0.1, K: int = 4):
        if not 1 <= int(K) <= SLOTS:
            raise ValueError(f"K must be 1..{SLOTS}")
        if not float(dt) > 0:
            raise ValueError("dt must be > 0")
        ref, e0, d = _route(ref_xy)
        super().__init__(B, Q, device, backend, INTERACT_STATE_I32, INTERACT_STATE_F64, INTERACT_I32, INTERACT_F64)
        self.K, self.dt, self.M = int(K), float(dt), int(ref.shape[0])
        # the route, its segments and the conflict table stay on the host for the numpy path
        self._e0, self._d, self._conflict = e0.numpy(), d.numpy(), conflict_points(ref.numpy())
        self.ref_xy, self.conflict = ref.to(self.device), torch.from_numpy(self._conflict).to(self.device)
        B, K, f64 = self.B, self.K, torch.float64
        self._slots = dict(ego=((B, 4), f64), opos=((B, K, 2), f64), ospeed=((B, K), f64), ohead=((B, K), f64),
                           oactive=((B, K), torch.uint8), oroute=((B, K), torch.int32), oprog=((B, K), f64),
                           otarget=((B, K), f64))            # what `update` reads of the environment

    def observe(self, frame, reset=False):
        self.update(frame["env"], frame.get("done"), reset)

    def update(self, env, done, reset=False):
        if getattr(env, "traffic", None) != "idm":
            raise ValueError("the interaction metrics need an environment with traffic='idm'")
        arrays = {name: _check(getattr(env, name), "env." + name, shape, dtype, self.device)
                  for name, (shape, dtype) in self._slots.items()}
        if not reset:
            done = _check(done, "done", (self.B,), torch.uint8, self.device)
        if self.backend == "torch":
            self._numpy_update({k: v.cpu().numpy() for k, v in arrays.items()}, None if reset else done.cpu().numpy(), reset)
            return
        _engine.caller("mpc_interaction_metrics")(
            device=self.device.index, B=self.B, K=self.K, Q=self.Q, M=self.M, reset=1 if reset else 0, dt=self.dt, **arrays,
            done=None if reset else done, ref_xy=self.ref_xy, conflict=self.conflict, state_i32=self.state_i32,
            state_f64=self.state_f64, rec_i32=self.rec_i32, rec_f64=self.rec_f64, stream=_engine.current_stream(self.device))

    def _sigma(self, x, y):
        """The ego's arc length along ref_xy [B] (csrc/mpc_interaction.hpp: sigma)."""
        e0, d = self._e0, self._d
        sx, sy = x[:, None] - e0[None, :, 0], y[:, None] - e0[None, :, 1]
        dx, dy = d[None, :, 0], d[None, :, 1]
        dd = dx * dx + dy * dy
        pos = dd > 0.0
        t = np.where(pos, (sx * dx + sy * dy) / np.where(pos, dd, 1.0), 0.0)
        t = np.where(t < 0.0, 0.0, t)
        t = np.where(t > 1.0, 1.0, t)
        cx, cy = sx - t * dx, sy - t * dy
        idx = np.argmin(cx * cx + cy * cy, axis=1)                       # the first of the nearest
        length = np.sqrt(dd[0])
        before = np.concatenate([[0.0], np.cumsum(length)])[idx]         # left to right
        rows = np.arange(x.shape[0])
        return before + t[rows, idx] * length[idx]

    def _numpy_update(self, s, done, reset):
        B, K, Q, dt = self.B, self.K, self.Q, self.dt
        si, sf = self.state_i32.cpu().numpy(), self.state_f64.cpu().numpy()
        rec_i, rec_f = self.rec_i32.cpu().numpy(), self.rec_f64.cpu().numpy()
        rows = np.arange(B)
        fresh = np.ones(B, bool) if reset else done != 0
        ordinal = np.zeros(B, np.int32) if reset else si[7].copy()
        if not reset:                                    # the episodes that ended: their records, from the states folded so far
            w = np.nonzero(fresh & (ordinal < Q))[0]
            rec_i[:, w, ordinal[w]] = si[:7, w]
            rec_f[:, w, ordinal[w]] = sf[:3, w]
            ordinal[w] += 1
        run_i = np.where(fresh[None], 0, si[:9])
        run_f = np.where(fresh[None], np.array([0.0, 0.0, np.inf])[:, None], sf[:3])
        n = run_i[0].astype(np.int64)
        x, y, th, sp = (s["ego"][:, i] for i in range(4))
        act = s["oactive"] != 0
        # ---- (a) yielding and forced braking
        leads, alts = [], []
        who = np.full((B, K), -2, np.int64)
        for j in range(K):
            xj, yj, hj = s["opos"][:, j, 0], s["opos"][:, j, 1], s["ohead"][:, j]
            cj, sj = np.cos(hj), np.sin(hj)
            lead, alt = _Leader(B), _Leader(B)
            lead.offer(j, xj, yj, hj, cj, sj, -1, x, y, th, sp, act[:, j])
            for k in range(K):
                if k != j:
                    cand = (j, xj, yj, hj, cj, sj, k, s["opos"][:, k, 0], s["opos"][:, k, 1], s["ohead"][:, k], s["ospeed"][:, k],
                            act[:, j] & act[:, k])
                    lead.offer(*cand)
                    alt.offer(*cand)
            who[:, j] = lead.who
            leads.append(lead)
            alts.append(alt)
        n_yield, hard_mask = np.zeros(B, np.int32), np.zeros(B, np.int32)
        forced, imposed_sum = np.zeros(B), np.zeros(B)
        for j in range(K):
            lead, alt = leads[j], alts[j]
            v, v0, hj = s["ospeed"][:, j], np.where(act[:, j], s["otarget"][:, j], 1.0), s["ohead"][:, j]
            lead.drop(_drives_free(j, who[:, j], who))
            yields = act[:, j] & (lead.who == -1)
            alt.drop(_drives_free(j, alt.who, who))
            a_with = _idm_acceleration(v, v0, hj, lead)
            imposed = np.where(yields, _idm_acceleration(v, v0, hj, alt) - a_with, 0.0)
            n_yield += yields
            forced = np.where(yields & (-a_with > forced), -a_with, forced)
            hard_mask |= (yields & (a_with < -HARD_BRAKE)).astype(np.int32) << j
            imposed_sum = imposed_sum + imposed
        # ---- (b) post-encroachment time
        sigma_c, s_c = self._conflict[:, 0], self._conflict[:, 1]
        sigma, sigma_prev = self._sigma(x, y), sf[3]
        with np.errstate(divide="ignore", invalid="ignore"):
            te_old = np.where(fresh[None], -1.0, sf[4:4 + ROUTES])
            te_new = (n >= 1)[None] & (sigma_c >= 0.0)[:, None] & (te_old < 0.0) & (sigma_prev[None] < sigma_c[:, None]) & \
                (sigma_c[:, None] <= sigma[None])
            tau = (n - 1).astype(np.float64)[None] + (sigma_c[:, None] - sigma_prev[None]) / (sigma - sigma_prev)[None]
            te = np.where(te_new, tau, te_old)
            conflicts, critical, ego_first = (np.zeros(B, np.int32) for _ in range(3))
            min_pet = np.full(B, np.inf)
            for j in range(SLOTS):
                inside = j < K
                route_j = s["oroute"][:, j] if inside else np.full(B, -1, np.int32)
                active = (act[:, j] if inside else np.zeros(B, bool)) & (route_j >= 0) & (route_j < ROUTES)
                route = np.where(active, route_j, -1).astype(np.int32)
                prog = np.where(active, s["oprog"][:, j], 0.0) if inside else np.zeros(B)
                croute, cprog, tv_old = si[9 + j], sf[4 + ROUTES + SLOTS + j], sf[4 + ROUTES + j]
                same = ~fresh & (n >= 1) & active & (croute == route) & (prog >= cprog)
                rr = np.clip(route, 0, ROUTES - 1)
                tv_new = same & (sigma_c[rr] >= 0.0) & (tv_old < 0.0) & (cprog < s_c[rr]) & (s_c[rr] <= prog)
                tv = np.where(tv_new, (n - 1).astype(np.float64) + (s_c[rr] - cprog) / (prog - cprog),
                              np.where(same, tv_old, -1.0))
                te_r, te_r_new = te[rr, rows], te_new[rr, rows]
                ev = active & (te_r >= 0.0) & (tv >= 0.0) & (te_r_new | tv_new)
                pet = np.abs(te_r - tv) * dt
                conflicts += ev
                critical += ev & (pet < PET_CRITICAL)
                ego_first += ev & (te_r < tv)
                min_pet = np.where(ev & (pet < min_pet), pet, min_pet)
                sf[4 + ROUTES + j], sf[4 + ROUTES + SLOTS + j], si[9 + j] = tv, prog, route
        sf[4:4 + ROUTES] = te
        events = hard_mask & ~run_i[8]
        si[0] = run_i[0] + 1
        si[1] = run_i[1] + (n_yield > 0)
        si[2] = run_i[2] + (hard_mask != 0)
        si[3] = run_i[3] + np.array([bin(int(v)).count("1") for v in events], np.int32)
        si[4], si[5], si[6] = run_i[4] + conflicts, run_i[5] + critical, run_i[6] + ego_first
        si[7], si[8] = ordinal, hard_mask
        sf[0] = np.where(forced > run_f[0], forced, run_f[0])
        sf[1] = run_f[1] + imposed_sum * dt
        sf[2] = np.where(min_pet < run_f[2], min_pet, run_f[2])
        sf[3] = sigma
        _write_back(((self.state_i32, si), (self.state_f64, sf), (self.rec_i32, rec_i), (self.rec_f64, rec_f)))


def corner_buildings(setback: float = 6.0, size: float = 30.0, road_half_width: float = 4.0) -> np.ndarray:
    """The four buildings on the corners of the junction of csrc/mpc_synth_env.hpp (lane centres at +-2 m, lane half width
    2 m, so the carriageway ends at +-4 m) as static occluders [4][4][2]: axis-aligned squares, one per quadrant in the order
    (+, +), (-, +), (-, -), (+, -), the inner corner at (+-(road_half_width + setback), +-(road_half_width + setback)),
    extending `size` outwards."""
    a = float(road_half_width) + float(setback)
    b = a + float(size)
    out = np.zeros((4, 4, 2))
    for q, (sx, sy) in enumerate(((1, 1), (-1, 1), (-1, -1), (1, -1))):
        x0, x1 = sorted((sx * a, sx * b))
        y0, y1 = sorted((sy * a, sy * b))
        out[q] = [[x0, y0], [x1, y0], [x1, y1], [x0, y1]]
    return out


def _mix64(z):
    """mpc::env::mix64 on numpy uint64 arrays (wrapping arithmetic)."""
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _u01(seed: int, env, ctr, slots):
    """mpc::env::Rng(seed, env, ctr).u01(slot) for env, ctr [B] (int64) and slots [...] -> f64 [B, ...]."""
    with np.errstate(over="ignore"):
        s = np.asarray([(int(seed) ^ 0xA5A5A5A5) & (2 ** 64 - 1)], dtype=np.uint64)
        key = _mix64(_mix64(s) + np.asarray(env, np.int64).astype(np.uint64) * np.uint64(0x100000001B3)) ^ \
            _mix64(np.asarray(ctr, np.int64).astype(np.uint64))
        slots = np.asarray(slots, np.int64).astype(np.uint64)
        bits = _mix64(key.reshape((-1,) + (1,) * slots.ndim) + slots[None] * np.uint64(0xD1342543DE82EF95))
    return (bits >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


class Perception:
    """What the ego sees of the true observation (csrc/mpc_perception.hpp states the model formula by formula): rows beyond
    `range` metres, rows hidden behind other vehicles or behind the static `occluders` [S, 4, 2] (`occlusion`; a row counts
    as visible while at least `min_points` of its centre and four corners are), rows dropped with probability `p_drop`, and
    bounded noise of standard deviation sigma_pos [m], sigma_vel [m/s], sigma_head [rad] on the rest.  The default of every
    parameter switches it off.  The draws are keyed by (seed, env_offset + b, launches since the reset), so they do not
    depend on the batch size or on how the environments are sharded.

    `apply(obs_true, out, reset=False)` fills `out` [B, R, 8] f32 (the seen rows compacted behind the ego's, the rest zero)
    and returns it; `row_class` [B, R] u8 holds the class of every input row of the last launch (ROW_*), `counts` [5, B] i64
    the rows of each of PERCEPTION_COUNTS since the reset, `ctr` [B] i64 the launches.  Backend "hip" is the kernel
    (mpc_perceive, enqueue only, capturable); backend "torch" is the reference path for machines without a GPU: the same
    update in numpy, draws in uint64, the same bits.  The parameters are plain attributes and may be changed between
    launches."""

    def __init__(self, B: int, device, backend: str = "torch", R: int = VEHICLES_COUNT, range: float = float("inf"),
                 occlusion: bool = False, min_points: int = 1, p_drop: float = 0.0, sigma_pos: float = 0.0,
                 sigma_vel: float = 0.0, sigma_head: float = 0.0, occluders=None, seed: int = 0, env_offset: int = 0):
        if backend not in ("hip", "torch"):
            raise ValueError("backend must be 'hip' or 'torch'")
        if int(B) < 0 or not 1 <= int(R) <= MAX_ROWS:
            raise ValueError(f"B must be >= 0 and R 1..{MAX_ROWS}")
        if not 1 <= int(min_points) <= 5:
            raise ValueError("min_points must be 1..5")
        if not 0.0 <= float(p_drop) <= 1.0:
            raise ValueError("p_drop must be in [0, 1]")
        for name, v in (("sigma_pos", sigma_pos), ("sigma_vel", sigma_vel), ("sigma_head", sigma_head)):
            if not float(v) >= 0.0:
                raise ValueError(f"{name} must be >= 0")
        if not float(range) > 0.0:
            raise ValueError("range must be > 0")
        if not 0 <= int(seed) < 2 ** 64:
            raise ValueError("seed must fit 64 unsigned bits")
        self.B, self.R, self.device, self.backend = int(B), int(R), torch.device(device), backend
        self.range, self.occlusion, self.min_points, self.p_drop = float(range), bool(occlusion), int(min_points), float(p_drop)
        self.sigma_pos, self.sigma_vel, self.sigma_head = float(sigma_pos), float(sigma_vel), float(sigma_head)
        self.seed, self.env_offset = int(seed), int(env_offset)
        occ = np.zeros((0, 4, 2)) if occluders is None else np.ascontiguousarray(occluders, dtype=np.float64)
        if occ.ndim != 3 or occ.shape[1:] != (4, 2) or occ.shape[0] > MAX_OCCLUDERS or not np.isfinite(occ).all():
            raise ValueError(f"occluders must be [S, 4, 2] finite corners with S <= {MAX_OCCLUDERS}")
        self.S = int(occ.shape[0])
        self.occluders = torch.from_numpy(occ).to(self.device)
        z = lambda *s, dt: torch.zeros(s, dtype=dt, device=self.device)
        self.row_class = z(self.B, self.R, dt=torch.uint8)
        self.counts = z(5, self.B, dt=torch.int64)
        self.ctr = z(self.B, dt=torch.int64)

    @property
    def config(self) -> dict:
        """The keyword arguments that make a Perception with the same model and the same draws."""
        return dict(R=self.R, range=self.range, occlusion=self.occlusion, min_points=self.min_points, p_drop=self.p_drop,
                    sigma_pos=self.sigma_pos, sigma_vel=self.sigma_vel, sigma_head=self.sigma_head,
                    occluders=self.occluders.cpu().numpy().copy(), seed=self.seed, env_offset=self.env_offset)

    def apply(self, obs_true, out, reset: bool = False):
        _check(obs_true, "obs_true", (self.B, self.R, 8), torch.float32, self.device)
        _check(out, "out", (self.B, self.R, 8), torch.float32, self.device)
        if out.data_ptr() == obs_true.data_ptr() and self.B > 0:
            raise ValueError("out must not be obs_true")
        if self.backend == "torch":
            seen = self._numpy_apply(obs_true.cpu().numpy(), bool(reset))
            out.copy_(torch.from_numpy(seen))
            return out
        params = dict(occlusion=int(self.occlusion), min_points=self.min_points, env_offset=self.env_offset, range=self.range,
                      p_drop=self.p_drop, sigma_pos=self.sigma_pos, sigma_vel=self.sigma_vel, sigma_head=self.sigma_head,
                      seed=self.seed)
        _engine.perceive(self.device.index, self.B, self.R, self.S, bool(reset), params, obs_true,
                         self.occluders if self.S else None, out, self.row_class, self.counts, self.ctr,
                         _engine.current_stream(self.device))
        return out

    def _hidden(self, t, present):
        """[B, K, 5] bool: the sight line from the ego to sample point k of row i strictly crosses an occluding edge."""
        B, K, S = self.B, self.R - 1, self.S
        e = lambda a: a[:, None, None, None, None]                       # the ego [B] against [B, i, point, quad, edge]
        px, py = e(t[:, 0, 1]), e(t[:, 0, 2])
        rect = np.stack([np.stack(c, axis=-1) for c in _corners(t[:, 1:, 1], t[:, 1:, 2], t[:, 1:, 7], t[:, 1:, 6])], axis=2)
        pts = np.concatenate([t[:, 1:, None, 1:3], rect], axis=2)        # [B, K, 5, 2]: the centre, then the corners
        quads = np.concatenate([rect, np.broadcast_to(self.occluders.cpu().numpy()[None], (B, S, 4, 2))], axis=1)
        blocks = np.concatenate([present, np.ones((B, S), bool)], axis=1)[:, None, :] & \
            (np.arange(K)[:, None] != np.arange(K + S)[None, :])[None]   # [B, i, quad]: present, and not row i itself
        e0, e1 = quads, np.roll(quads, -1, axis=2)
        q = lambda a: a[:, None, None, :, :]
        e0x, e0y, e1x, e1y = q(e0[..., 0]), q(e0[..., 1]), q(e1[..., 0]), q(e1[..., 1])
        sx, sy = pts[:, :, :, None, None, 0], pts[:, :, :, None, None, 1]
        cross = lambda ax, ay, bx, by: ax * by - ay * bx
        ex, ey, rx, ry = e1x - e0x, e1y - e0y, sx - px, sy - py
        d1, d2 = cross(ex, ey, px - e0x, py - e0y), cross(ex, ey, sx - e0x, sy - e0y)
        d3, d4 = cross(rx, ry, e0x - px, e0y - py), cross(rx, ry, e1x - px, e1y - py)
        crossing = (((d1 > 0) & (d2 < 0)) | ((d1 < 0) & (d2 > 0))) & (((d3 > 0) & (d4 < 0)) | ((d3 < 0) & (d4 > 0)))
        return (crossing & blocks[:, :, None, :, None]).any(axis=(3, 4))

    def _numpy_apply(self, obs, reset):
        B, R, K = self.B, self.R, self.R - 1
        counts, ctr = self.counts.cpu().numpy(), self.ctr.cpu().numpy()
        if reset:
            counts[:], ctr[:] = 0, 0
        t = obs.astype(np.float64)
        present = obs[:, 1:, 0] != 0
        rx, ry = t[:, 1:, 1] - t[:, :1, 1], t[:, 1:, 2] - t[:, :1, 2]
        far = rx * rx + ry * ry > self.range * self.range
        if self.occlusion and K > 0:
            occluded = (5 - self._hidden(t, present).sum(axis=2)) < self.min_points
        else:
            occluded = np.zeros((B, K), bool)
        rows = np.arange(1, R)
        u = _u01(self.seed ^ PERCEPTION_SALT, self.env_offset + np.arange(B), ctr,
                 ROW_SLOTS * rows[:, None] + np.arange(21)[None, :])                    # [B, K, 21]
        dropped = u[:, :, 0] < self.p_drop
        cls = np.select([~present, far, occluded, dropped], [ROW_ABSENT, ROW_OUT_OF_RANGE, ROW_OCCLUDED, ROW_DROPPED],
                        ROW_SEEN).astype(np.uint8)
        n = lambda k: ((u[:, :, k] + u[:, :, k + 1]) + (u[:, :, k + 2] + u[:, :, k + 3]) - 2.0) * UNIT_SCALE
        noisy = obs[:, 1:].copy()
        if self.sigma_pos != 0.0:
            noisy[:, :, 1] = (t[:, 1:, 1] + self.sigma_pos * n(1)).astype(np.float32)
            noisy[:, :, 2] = (t[:, 1:, 2] + self.sigma_pos * n(5)).astype(np.float32)
        if self.sigma_vel != 0.0:
            noisy[:, :, 3] = (t[:, 1:, 3] + self.sigma_vel * n(9)).astype(np.float32)
            noisy[:, :, 4] = (t[:, 1:, 4] + self.sigma_vel * n(13)).astype(np.float32)
        if self.sigma_head != 0.0:
            eps = self.sigma_head * n(17)
            sh, ch = t[:, 1:, 6], t[:, 1:, 7]
            c1, s1 = ch - eps * sh, sh + eps * ch
            nrm = np.sqrt(c1 * c1 + s1 * s1)
            ok = nrm != 0
            safe = np.where(ok, nrm, 1.0)
            noisy[:, :, 5] = (t[:, 1:, 5] + eps).astype(np.float32)
            noisy[:, :, 6] = np.where(ok, (s1 / safe).astype(np.float32), obs[:, 1:, 6])
            noisy[:, :, 7] = np.where(ok, (c1 / safe).astype(np.float32), obs[:, 1:, 7])
        seen = cls == ROW_SEEN
        out = np.zeros((B, R, 8), np.float32)
        out[:, 0] = obs[:, 0]
        if K > 0:
            order = np.argsort(~seen, axis=1, kind="stable")                           # the seen rows first, in input order
            packed = np.take_along_axis(noisy, order[:, :, None], axis=1)
            keep = np.arange(K)[None, :] < seen.sum(axis=1)[:, None]
            out[:, 1:][keep] = packed[keep]
        for f, c in enumerate((ROW_ABSENT, ROW_SEEN, ROW_OUT_OF_RANGE, ROW_OCCLUDED, ROW_DROPPED)):
            counts[f] += (cls != ROW_ABSENT).sum(axis=1) if f == 0 else (cls == c).sum(axis=1)
        ctr += 1
        row_class = np.concatenate([np.full((B, 1), ROW_SEEN, np.uint8), cls], axis=1)
        _write_back(((self.counts, counts), (self.ctr, ctr), (self.row_class, row_class)))
        return out

    def totals(self) -> dict:
        """Rows >= 1 since the reset, summed over the environments: present, seen, out_of_range, occluded, dropped."""
        c = self.counts.sum(dim=1).cpu().numpy()
        return {k: int(c[i]) for i, k in enumerate(PERCEPTION_COUNTS)}


class Tracker:
    """Tracks the vehicles of an observation across frames (csrc/mpc_tracker.hpp states the model step by step): every
    measured row is associated with the nearest of 16 track slots within `gate` metres of its predicted position (greedy, in
    row order), smoothed by the gains alpha_pos and alpha_vel (1: the measurement itself), a slot that is not measured is moved
    on with its last velocity for up to `coast` launches, and the output rows are the alive slots ordered by their distance to
    the ego.  With coast=0 and both gains 1 the output is the input's present rows, bit for bit, in that order.

    `apply(obs_meas, out, done=None, reset=False)` fills `out` [B, R, 8] f32 and returns it; done [B]: the environments whose
    episode ended on this step (their tracks are dropped before the frame is read).  `row_slot` [B, R] u8 holds the slot behind
    every output row of the last launch (255: none), `row_miss` [B, R] u8 the launches since that slot was measured,
    `track_f64` [B, 16, 7] and `track_i32` [B, 16, 3] the slots (x, y, vx, vy, heading, sin_h, cos_h; alive, age, miss),
    `counts` [7, B] i64 the events of each of TRACKER_COUNTS since the reset.  Backend "hip" is the kernel (mpc_track_rows,
    enqueue only, capturable); backend "torch" is the same update in numpy for the CPU environment, the same bits."""

    def __init__(self, B: int, device, backend: str = "torch", R: int = VEHICLES_COUNT, dt: float = 0.1, gate: float = 3.0,
                 coast: int = 0, alpha_pos: float = 1.0, alpha_vel: float = 1.0):
        if backend not in ("hip", "torch"):
            raise ValueError("backend must be 'hip' or 'torch'")
        if int(B) < 0 or not 1 <= int(R) <= MAX_ROWS:
            raise ValueError(f"B must be >= 0 and R 1..{MAX_ROWS}")
        if not float(dt) > 0.0:
            raise ValueError("dt must be > 0")
        if not float(gate) >= 0.0:
            raise ValueError("gate must be >= 0")
        if int(coast) != coast or not 0 <= int(coast) <= TRACK_MAX_COAST:
            raise ValueError(f"coast must be an integer 0..{TRACK_MAX_COAST}")
        for name, v in (("alpha_pos", alpha_pos), ("alpha_vel", alpha_vel)):
            if not 0.0 < float(v) <= 1.0:
                raise ValueError(f"{name} must be in (0, 1]")
        self.B, self.R, self.device, self.backend = int(B), int(R), torch.device(device), backend
        self.dt, self.gate, self.coast = float(dt), float(gate), int(coast)
        self.alpha_pos, self.alpha_vel = float(alpha_pos), float(alpha_vel)
        z = lambda *s, dt: torch.zeros(s, dtype=dt, device=self.device)
        self.row_slot, self.row_miss = z(self.B, self.R, dt=torch.uint8), z(self.B, self.R, dt=torch.uint8)
        self.track_f64, self.track_i32 = z(self.B, TRACK_SLOTS, 7, dt=torch.float64), z(self.B, TRACK_SLOTS, 3, dt=torch.int32)
        self.counts = z(len(TRACKER_COUNTS), self.B, dt=torch.int64)

    @property
    def config(self) -> dict:
        """The keyword arguments that make a Tracker with the same model."""
        return dict(R=self.R, dt=self.dt, gate=self.gate, coast=self.coast, alpha_pos=self.alpha_pos, alpha_vel=self.alpha_vel)

    def apply(self, obs_meas, out, done=None, reset: bool = False):
        B, R, dev = self.B, self.R, self.device
        _check(obs_meas, "obs_meas", (B, R, 8), torch.float32, dev)
        _check(out, "out", (B, R, 8), torch.float32, dev)
        if out.data_ptr() == obs_meas.data_ptr() and B > 0:
            raise ValueError("out must not be obs_meas")
        if done is not None:
            done = _check(done, "done", (B,), torch.uint8, dev)
        if self.backend == "torch":
            rows = self._numpy_apply(obs_meas.cpu().numpy(), None if done is None else done.cpu().numpy(), bool(reset))
            out.copy_(torch.from_numpy(rows))
            return out
        _engine.caller("mpc_track_rows")(
            device=dev.index, B=B, R=R, reset=1 if reset else 0, dt=self.dt, gate=self.gate, coast=self.coast,
            alpha_pos=self.alpha_pos, alpha_vel=self.alpha_vel, obs_meas=obs_meas, done=done, obs_out=out,
            row_slot=self.row_slot, row_miss=self.row_miss, track_f64=self.track_f64, track_i32=self.track_i32,
            counts=self.counts, stream=_engine.current_stream(dev))
        return out

    def _numpy_apply(self, meas, done, reset):
        """csrc/mpc_tracker.hpp over the batch: the loops over rows stay, every statement acts on all environments."""
        B, R, S = self.B, self.R, TRACK_SLOTS
        tf, ti, counts = self.track_f64.cpu().numpy().copy(), self.track_i32.cpu().numpy().copy(), self.counts.cpu().numpy().copy()
        env = np.arange(B)
        clear = np.ones(B, bool) if reset else (np.zeros(B, bool) if done is None else done != 0)
        if reset:
            counts[:] = 0
        tf[clear], ti[clear] = 0.0, 0                                              # 1
        f = [tf[:, :, c].copy() for c in range(7)]                                 # x, y, vx, vy, heading, sin_h, cos_h [B, S]
        alive, age, miss = ti[:, :, 0] != 0, ti[:, :, 1].copy(), ti[:, :, 2].copy()
        f[0] = np.where(alive, f[0] + f[2] * self.dt, f[0])                        # 2
        f[1] = np.where(alive, f[1] + f[3] * self.dt, f[1])
        m = meas.astype(np.float64)
        present = meas[:, :, 0] != 0
        present[:, 0] = False
        claimed, unassociated = np.zeros((B, S), bool), np.zeros((B, R), bool)
        gate2 = self.gate * self.gate
        blend = lambda a, alpha, v: v if alpha == 1.0 else a + alpha * (v - a)
        for i in range(1, R):                                                      # 3, 4
            dx, dy = m[:, i, 1, None] - f[0], m[:, i, 2, None] - f[1]
            d = dx * dx + dy * dy
            eligible = present[:, i, None] & alive & ~claimed & (d <= gate2)
            best = np.argmin(np.where(eligible, d, np.inf), axis=1)                # the first of the smallest: the lowest slot
            found = eligible[env, best]
            e, s = env[found], best[found]
            claimed[e, s] = True
            f[0][e, s], f[1][e, s] = blend(f[0][e, s], self.alpha_pos, m[e, i, 1]), blend(f[1][e, s], self.alpha_pos, m[e, i, 2])
            f[2][e, s], f[3][e, s] = blend(f[2][e, s], self.alpha_vel, m[e, i, 3]), blend(f[3][e, s], self.alpha_vel, m[e, i, 4])
            for c in (4, 5, 6):
                f[c][e, s] = m[e, i, c + 1]
            miss[e, s] = 0
            age[e, s] += 1
            unassociated[:, i] = present[:, i] & ~found
        coasting = alive & ~claimed                                                # 5
        miss = miss + coasting
        expired = coasting & (miss > self.coast)
        alive, coasting = alive & ~expired, coasting & ~expired
        for a in f + [age, miss]:
            a[expired] = 0
        queue = np.argsort(np.where(alive, np.where(claimed, 2, 1), 0), axis=1, kind="stable")      # 6: free, then coasting
        place = np.cumsum(unassociated, axis=1) - 1
        evicted = np.zeros(B, np.int64)
        was_alive = alive.copy()
        for i in range(1, R):
            e = env[unassociated[:, i]]
            s = queue[e, place[e, i]]
            evicted[e] += was_alive[e, s]
            for c in range(7):
                f[c][e, s] = m[e, i, c + 1]
            alive[e, s], age[e, s], miss[e, s] = True, 1, 0
        out = np.zeros((B, R, 8), np.float32)                                      # 7
        out[:, 0] = meas[:, 0]
        row_slot, row_miss = np.full((B, R), TRACK_NO_SLOT, np.uint8), np.zeros((B, R), np.uint8)
        kx, ky = f[0] - m[:, 0, 1, None], f[1] - m[:, 0, 2, None]
        key = kx * kx + ky * ky
        slot = np.arange(S)
        ahead = alive[:, None, :] & ((key[:, None, :] < key[:, :, None]) |
                                     ((key[:, None, :] == key[:, :, None]) & (slot[None, None, :] < slot[None, :, None])))
        rank = ahead.sum(axis=2)                                                   # [B, S]: alive slots ordered before slot s
        shown = alive & (rank < R - 1)
        e, s = np.nonzero(shown)
        out[e, 1 + rank[e, s], 0] = 1.0
        for c in range(7):
            out[e, 1 + rank[e, s], c + 1] = f[c][e, s].astype(np.float32)
        row_slot[e, 1 + rank[e, s]], row_miss[e, 1 + rank[e, s]] = s, miss[e, s]
        n = (present.sum(axis=1), claimed.sum(axis=1), unassociated.sum(axis=1), (shown & (miss > 0)).sum(axis=1),         # 8
             expired.sum(axis=1), evicted, (alive & ~shown).sum(axis=1))
        for k, v in enumerate(n):
            counts[k] += v
        tf = np.stack(f, axis=2)
        ti = np.stack([alive.astype(np.int32), age, miss.astype(np.int32)], axis=2).astype(np.int32)
        _write_back(((self.track_f64, tf), (self.track_i32, ti), (self.counts, counts), (self.row_slot, row_slot),
                     (self.row_miss, row_miss)))
        return out

    def totals(self) -> dict:
        """Events since the reset, summed over the environments: rows measured, matched to a track, born as a new track;
        output rows that were coasted; tracks expired, evicted by a birth, cut from the output for want of rows."""
        c = self.counts.sum(dim=1).cpu().numpy()
        return {k: int(c[i]) for i, k in enumerate(TRACKER_COUNTS)}


def _pair(name, value):
    """`value` as the two floats of a per-channel parameter (acceleration, steering)"""
    try:
        a, b = value
        return float(a), float(b)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a pair (acceleration, steering)") from None


class Actuation:
    """What the vehicle makes of the agent's command (csrc/mpc_actuator.hpp states the model step by step), per channel
    (acceleration m/s^2, steering rad): the command arrives `delay` whole policy steps late (0..7; zero until then), is lost
    with probability `p_hold` (the previous one is held, both channels together), scaled and shifted by `gain` and `offset`,
    disturbed by bounded noise of standard deviation `sigma`, followed with a first-order lag of time constant `tau` [s]
    (alpha = dt / (tau + dt), formed once here; tau = 0 gives exactly 1), changed by at most `rate` per second, and clamped to
    `limits`: None for (-inf, +inf) on both channels, "env" for the environment's own clamp (+-5 m/s^2, +-pi/4), or
    ((lo, hi), (lo, hi)).  The default of every parameter switches it off: the applied action is then the command bit for bit.
    The draws are keyed by (seed, env_offset + b, launches since the reset), so they do not depend on the batch size or on
    how the environments are sharded.  The parameters are fixed at construction.

    `apply(command, out, done_prev=None)` fills `out` [B, 2] f64 (it may be `command`) and returns it; done_prev [B]: the
    environments whose episode ended on the previous step (their delay line, held command and lag state are cleared before the
    command is read).  `reset()` clears everything.  `state` [10, B, 2] f64 holds the last eight commands, what reached the
    actuator last and what was applied last, `age` [B] i32 the commands of the episode, `ctr` [B] i64 the launches, `counts`
    [5, B] i64 the steps of each of ACTUATION_COUNTS, `sums` [2, B, 2] f64 the sum and the maximum of |applied - command|.
    Backend "hip" is the kernel (mpc_actuate, enqueue only, capturable); backend "torch" is the same update in numpy for the
    CPU environment, the same bits."""

    def __init__(self, B: int, device, backend: str = "torch", dt: float = 0.1, delay: int = 0, p_hold: float = 0.0,
                 gain=(1.0, 1.0), offset=(0.0, 0.0), sigma=(0.0, 0.0), tau=(0.0, 0.0), rate=(math.inf, math.inf),
                 limits=None, seed: int = 0, env_offset: int = 0):
        if backend not in ("hip", "torch"):
            raise ValueError("backend must be 'hip' or 'torch'")
        if int(B) < 0:
            raise ValueError("B must be >= 0")
        if not float(dt) > 0.0:
            raise ValueError("dt must be > 0")
        if int(delay) != delay or not 0 <= int(delay) <= ACT_MAX_DELAY:
            raise ValueError(f"delay must be an integer 0..{ACT_MAX_DELAY}")
        if not 0.0 <= float(p_hold) <= 1.0:
            raise ValueError("p_hold must be in [0, 1]")
        gain, offset, sigma, tau, rate = (_pair(n, v) for n, v in (("gain", gain), ("offset", offset), ("sigma", sigma),
                                                                   ("tau", tau), ("rate", rate)))
        if limits is None:
            limits = ((-math.inf, math.inf), (-math.inf, math.inf))
        elif isinstance(limits, str):
            if limits != "env":
                raise ValueError("limits must be None, 'env' or ((lo, hi), (lo, hi))")
            limits = ENV_LIMITS
        limits = tuple(_pair("limits", v) for v in _pair_of_pairs(limits))
        for c in (0, 1):
            if not (math.isfinite(gain[c]) and math.isfinite(offset[c])):
                raise ValueError("gain and offset must be finite")
            if not (sigma[c] >= 0.0 and math.isfinite(sigma[c])):
                raise ValueError("sigma must be >= 0 and finite")
            if not (tau[c] >= 0.0 and math.isfinite(tau[c])):
                raise ValueError("tau must be >= 0 and finite")
            if not rate[c] > 0.0:
                raise ValueError("rate must be > 0 (inf: no limit)")
            if not limits[c][0] <= limits[c][1]:
                raise ValueError("limits must be lo <= hi")
        if not 0 <= int(seed) < 2 ** 64:
            raise ValueError("seed must fit 64 unsigned bits")
        self.B, self.device, self.backend = int(B), torch.device(device), backend
        self.dt, self.delay, self.p_hold = float(dt), int(delay), float(p_hold)
        self.gain, self.offset, self.sigma, self.tau, self.rate, self.limits = gain, offset, sigma, tau, rate, limits
        self.alpha = tuple(self.dt / (t + self.dt) for t in tau)
        if not all(0.0 < a <= 1.0 for a in self.alpha):
            raise ValueError("tau is too large for dt: alpha = dt / (tau + dt) must be in (0, 1]")
        self.seed, self.env_offset = int(seed), int(env_offset)
        z = lambda *s, dt: torch.zeros(s, dtype=dt, device=self.device)
        self.state, self.sums = z(ACT_PREV + 1, self.B, 2, dt=torch.float64), z(2, self.B, 2, dt=torch.float64)
        self.age, self.ctr = z(self.B, dt=torch.int32), z(self.B, dt=torch.int64)
        self.counts = z(len(ACTUATION_COUNTS), self.B, dt=torch.int64)
        pair = lambda v: (ctypes.c_double * 2)(*v)
        self._params = _engine.ActuatorParams(
            struct_size=ctypes.sizeof(_engine.ActuatorParams), delay=self.delay, env_offset=self.env_offset, reserved=0,
            dt=self.dt, p_hold=self.p_hold, gain=pair(gain), offset=pair(offset), sigma=pair(sigma), alpha=pair(self.alpha),
            rate=pair(rate), lo=pair((limits[0][0], limits[1][0])), hi=pair((limits[0][1], limits[1][1])), seed=self.seed)

    @property
    def config(self) -> dict:
        """The keyword arguments that make an Actuation with the same model and the same draws."""
        return dict(dt=self.dt, delay=self.delay, p_hold=self.p_hold, gain=self.gain, offset=self.offset, sigma=self.sigma,
                    tau=self.tau, rate=self.rate, limits=self.limits, seed=self.seed, env_offset=self.env_offset)

    def _launch(self, reset, command=None, done_prev=None, applied=None):
        _engine.caller("mpc_actuate")(
            device=self.device.index, B=self.B, reset=reset, params=self._params, command=command, done_prev=done_prev,
            applied=applied, state_f64=self.state, age=self.age, ctr=self.ctr, counts=self.counts, sums=self.sums,
            stream=_engine.current_stream(self.device))

    def reset(self) -> None:
        """Everything starts anew: the delay line, the held command, the lag state, the draw counter, the counts, the sums."""
        if self.backend == "hip":
            self._launch(1)
        else:
            for t in (self.state, self.sums, self.age, self.ctr, self.counts):
                t.zero_()

    def apply(self, command, out, done_prev=None):
        B, dev = self.B, self.device
        _check(command, "command", (B, 2), torch.float64, dev)
        _check(out, "out", (B, 2), torch.float64, dev)
        if done_prev is not None:
            done_prev = _check(done_prev, "done_prev", (B,), torch.uint8, dev)
        if self.backend == "torch":
            applied = self._numpy_apply(command.cpu().numpy(), None if done_prev is None else done_prev.cpu().numpy())
            out.copy_(torch.from_numpy(applied))
        else:
            self._launch(0, command, done_prev, out)
        return out

    def _numpy_apply(self, cmd, done_prev):
        """csrc/mpc_actuator.hpp over the batch: every statement acts on all environments, the channels one after the other."""
        B = self.B
        state, sums, age, ctr, counts = (t.cpu().numpy() for t in (self.state, self.sums, self.age, self.ctr, self.counts))
        env = np.arange(B)
        draws = lambda slots: _u01(self.seed ^ ACTUATION_SALT, self.env_offset + env, ctr, slots)
        clear = np.zeros(B, bool) if done_prev is None else done_prev != 0
        age[clear] = 0                                                             # 1
        state[:, clear] = 0.0
        with np.errstate(invalid="ignore", over="ignore"):
            finite = (cmd - cmd) == 0.0                                            # 2
            u = np.where(finite, cmd, 0.0)
            state[age & (ACT_RING - 1), env] = u                                   # 3
            delayed = np.where((age >= self.delay)[:, None], state[(age - self.delay) & (ACT_RING - 1), env], 0.0)
            held = draws(np.arange(1))[:, 0] < self.p_hold if self.p_hold > 0.0 else np.zeros(B, bool)     # 4
            delayed = np.where(held[:, None], state[ACT_LAST], delayed)
            state[ACT_LAST] = delayed
            prev = state[ACT_PREV].copy()
            y, limited, clipped = np.empty((B, 2)), np.zeros((B, 2), bool), np.zeros((B, 2), bool)
            for c in (0, 1):
                v, p = delayed[:, c], prev[:, c]
                if not (self.gain[c] == 1.0 and self.offset[c] == 0.0):            # 5
                    v = self.gain[c] * v + self.offset[c]
                if self.sigma[c] != 0.0:
                    d = draws(1 + 4 * c + np.arange(4))
                    v = v + self.sigma[c] * (((d[:, 0] + d[:, 1]) + (d[:, 2] + d[:, 3]) - 2.0) * UNIT_SCALE)
                yc = v
                if self.alpha[c] != 1.0:                                           # 6
                    yc = p + self.alpha[c] * (v - p)
                if math.isfinite(self.rate[c]):                                    # 7
                    m, d = self.rate[c] * self.dt, yc - p
                    yc = np.where(d > m, p + m, np.where(d < -m, p - m, yc))
                    limited[:, c] = (d > m) | (d < -m)
                lo, hi = self.limits[c]                                            # 8
                below = yc < lo
                yc = np.where(below, lo, yc)
                above = yc > hi
                y[:, c], clipped[:, c] = np.where(above, hi, yc), below | above
            dev = np.abs(y - u)                                                    # 9
        state[ACT_PREV] = y
        sums[0] += dev
        sums[1] = np.where(dev > sums[1], dev, sums[1])
        age += 1
        ctr += 1
        for k, n in enumerate((np.ones(B, bool), held, limited.any(axis=1), clipped.any(axis=1), ~finite.all(axis=1))):
            counts[k] += n
        _write_back(((self.state, state), (self.sums, sums), (self.age, age), (self.ctr, ctr), (self.counts, counts)))
        return y

    def totals(self) -> dict:
        """Since the reset, summed over the environments: steps, and the steps on which the command was held, the rate limit
        acted, the saturation acted, the command was not finite; mean_abs_dev and max_abs_dev (2,): the mean over the steps
        and the maximum of |applied - command| per channel."""
        c = self.counts.sum(dim=1).cpu().numpy()
        s = self.sums.cpu().numpy()
        out = {k: int(c[i]) for i, k in enumerate(ACTUATION_COUNTS)}
        out["mean_abs_dev"] = s[0].sum(axis=0) / max(out["steps"], 1)
        out["max_abs_dev"] = s[1].max(axis=0, initial=0.0)
        return out


def _pair_of_pairs(limits):
    try:
        a, b = limits
        return a, b
    except (TypeError, ValueError):
        raise ValueError("limits must be None, 'env' or ((lo, hi), (lo, hi))") from None


def _step_ego(x, y, th, sp, action, dt):
    """csrc/mpc_synth_env.hpp::step_ego over the batch: action [B, 2] -> the next (x, y, th, sp)"""
    a = np.clip(action[:, 0], ENV_LIMITS[0][0], ENV_LIMITS[0][1])
    delta = np.clip(action[:, 1], ENV_LIMITS[1][0], ENV_LIMITS[1][1])
    beta = np.arctan(0.5 * np.tan(delta))
    nx = x + sp * np.cos(th + beta) * dt
    ny = y + sp * np.sin(th + beta) * dt
    nth = th + sp / ENV_WHEELBASE * np.sin(beta) * dt
    return nx, ny, nth, np.clip(sp + a * dt, 0.0, ENV_MAX_SPEED)


class Compensation:
    """Delay compensation in front of the agent (csrc/mpc_compensate.hpp states the update step by step): the agent's command
    takes effect `steps` whole policy steps (0..7) after the scene it was computed from, so the agent is handed the scene
    predicted to that moment.  The compensator keeps the commands still in flight, rolls the ego through them with the
    environment's own vehicle model behind the NOMINAL actuator - a first-order lag of time constant `tau` [s] per channel
    (alpha = dt / (tau + dt), formed once here), at most `rate` per second, clamped to `limits` (None, "env" or
    ((lo, hi), (lo, hi)), as `Actuation` reads them); no gain, offset, noise or hold: a compensator knows its nominal
    actuator, not its errors - and moves every other vehicle on with its observed velocity, re-ordered by distance to the
    predicted ego.  With steps = 0 the output is the input bit for bit.  `Compensation.matching(actuation)` takes the delay,
    tau, rate and limits of an `Actuation`.  The parameters are fixed at construction.

    `latency` (0 .. 7 - steps): the scene handed in is itself that many policy steps old (`Latency`, or a deployment's own
    sensing latency); the ego is then rolled through steps + min(latency, age) commands - those issued since the scene and those
    in flight -, the others move on by as much, `prev` is the nominal applied action of the step before the scene shown and a
    prediction is scored against the ego that arrives steps + latency launches later (mpc_compensate_stale).  With latency = 0
    everything here is what it is without the argument, and the kernel launched is mpc_compensate's.  With steps + latency = 0
    the output is the input bit for bit.  `Compensation.matching(actuation, latency)` takes the latency of a `Latency`.

    `apply(obs, out, command, done)` fills `out` [B, R, 8] f32 (not `obs`) from the observation `obs` and the agent's command
    [B, 2] f64 of the step that just ran, and returns it; done [B]: the environments whose episode ended on that step (their
    memory is cleared, their command is not read).  `apply(obs, out, reset=True)` starts every environment anew on its first
    scene and needs no command; `reset()` only clears.  `pred` [B, 4] f64 is the predicted ego (x, y, heading, speed) of the
    last launch; `ring` [8, B, 2] f64 the last eight commands, `prev` [B, 2] f64 the nominal applied action of the step that
    just ran, `age` [B] i32 the commands of the episode, `pring` [8, B, 2] f64 the predicted (x, y) of the last eight
    launches; `counts` [B] i64 the predictions scored against the ego observed `steps` launches later, `sums` [2, B] f64 the
    sum and the maximum of that position error [m].  Backend "hip" is the kernel (mpc_compensate, enqueue only, capturable);
    backend "torch" is the same update in numpy for the CPU environment: the same bits wherever only + - * and comparisons
    are involved, and equal to the rounding of the library's sqrt, sin, cos, tan and atan in the ego's rollout."""

    def __init__(self, B: int, device, backend: str = "torch", R: int = VEHICLES_COUNT, dt: float = 0.1, steps: int = 0,
                 tau=(0.0, 0.0), rate=(math.inf, math.inf), limits=None, latency: int = 0):
        if backend not in ("hip", "torch"):
            raise ValueError("backend must be 'hip' or 'torch'")
        if int(B) < 0:
            raise ValueError("B must be >= 0")
        if not 1 <= int(R) <= MAX_ROWS:
            raise ValueError(f"R must be in 1..{MAX_ROWS}")
        if not float(dt) > 0.0:
            raise ValueError("dt must be > 0")
        if int(steps) != steps or not 0 <= int(steps) <= COMP_MAX_STEPS:
            raise ValueError(f"steps must be an integer 0..{COMP_MAX_STEPS}")
        if int(latency) != latency or not 0 <= int(latency) <= COMP_MAX_STEPS - int(steps):
            raise ValueError(f"latency must be an integer >= 0 with steps + latency <= {COMP_MAX_STEPS}")
        tau, rate = _pair("tau", tau), _pair("rate", rate)
        if limits is None:
            limits = ((-math.inf, math.inf), (-math.inf, math.inf))
        elif isinstance(limits, str):
            if limits != "env":
                raise ValueError("limits must be None, 'env' or ((lo, hi), (lo, hi))")
            limits = ENV_LIMITS
        limits = tuple(_pair("limits", v) for v in _pair_of_pairs(limits))
        for c in (0, 1):
            if not (tau[c] >= 0.0 and math.isfinite(tau[c])):
                raise ValueError("tau must be >= 0 and finite")
            if not rate[c] > 0.0:
                raise ValueError("rate must be > 0 (inf: no limit)")
            if not limits[c][0] <= limits[c][1]:
                raise ValueError("limits must be lo <= hi")
        self.B, self.R, self.device, self.backend = int(B), int(R), torch.device(device), backend
        self.dt, self.steps, self.tau, self.rate, self.limits = float(dt), int(steps), tau, rate, limits
        self.latency = int(latency)
        self.alpha = tuple(self.dt / (t + self.dt) for t in tau)
        if not all(0.0 < a <= 1.0 for a in self.alpha):
            raise ValueError("tau is too large for dt: alpha = dt / (tau + dt) must be in (0, 1]")
        z = lambda *s, dt: torch.zeros(s, dtype=dt, device=self.device)
        self.ring, self.pring = z(COMP_RING, self.B, 2, dt=torch.float64), z(COMP_RING, self.B, 2, dt=torch.float64)
        self.prev, self.pred = z(self.B, 2, dt=torch.float64), z(self.B, 4, dt=torch.float64)
        self.age, self.counts, self.sums = z(self.B, dt=torch.int32), z(self.B, dt=torch.int64), z(2, self.B, dt=torch.float64)
        pair = lambda v: (ctypes.c_double * 2)(*v)
        self._params = _engine.CompensatorParams(
            struct_size=ctypes.sizeof(_engine.CompensatorParams), steps=self.steps, dt=self.dt, alpha=pair(self.alpha),
            rate=pair(rate), lo=pair((limits[0][0], limits[1][0])), hi=pair((limits[0][1], limits[1][1])))

    @classmethod
    def matching(cls, actuation=None, latency=None, R: int = VEHICLES_COUNT, dt: float | None = None) -> "Compensation":
        """The compensator of `actuation`'s nominal model: its batch, device, backend and dt, its delay as `steps`, its tau,
        rate and limits - and none of its errors (gain, offset, noise, hold) -, and of `latency`'s steps (a `Latency`) as its
        latency.  Either may be None (not both): without an actuator model the batch, device and backend are the latency
        model's, there is no delay, lag or limit to know of, and dt is the argument (0.1 when None)."""
        if actuation is None and latency is None:
            raise ValueError("matching needs an actuator model or a latency model")
        old = 0 if latency is None else latency.steps
        if actuation is None:
            return cls(latency.B, latency.device, latency.backend, R=R, dt=0.1 if dt is None else dt, latency=old)
        if latency is not None and (latency.B, latency.device, latency.backend) != (actuation.B, actuation.device,
                                                                                     actuation.backend):
            raise ValueError("the actuator model and the latency model must share batch, device and backend")
        return cls(actuation.B, actuation.device, actuation.backend, R=R, dt=actuation.dt, steps=actuation.delay,
                   tau=actuation.tau, rate=actuation.rate, limits=actuation.limits, latency=old)

    @property
    def config(self) -> dict:
        """The keyword arguments that make a Compensation with the same model (latency only when it is not 0)."""
        out = dict(R=self.R, dt=self.dt, steps=self.steps, tau=self.tau, rate=self.rate, limits=self.limits)
        if self.latency:
            out["latency"] = self.latency
        return out

    def reset(self) -> None:
        """Forget everything: the commands in flight, the nominal actuator's state, the predictions, the counts, the sums.
        `apply(..., reset=True)` does the same and then compensates the first scene."""
        for t in (self.ring, self.pring, self.prev, self.age, self.counts, self.sums):
            t.zero_()

    def apply(self, obs, out, command=None, done=None, reset: bool = False):
        B, R, dev = self.B, self.R, self.device
        _check(obs, "obs", (B, R, 8), torch.float32, dev)
        _check(out, "out", (B, R, 8), torch.float32, dev)
        if out is obs or (B > 0 and out.data_ptr() == obs.data_ptr()):
            raise ValueError("out must not be obs")
        if not reset:
            _check(command, "command", (B, 2), torch.float64, dev)
        if done is not None:
            done = _check(done, "done", (B,), torch.uint8, dev)
        if self.backend == "torch":
            o, pred = self._numpy_apply(obs.cpu().numpy(), None if reset else command.cpu().numpy(),
                                        None if done is None else done.cpu().numpy(), bool(reset))
            out.copy_(torch.from_numpy(o))
            if self.pred is not None:
                self.pred.copy_(torch.from_numpy(pred))
        elif self.latency == 0:
            _engine.caller("mpc_compensate")(
                device=dev.index, B=B, R=R, reset=1 if reset else 0, params=self._params, obs=obs,
                command=None if reset else command, done=None if reset else done, out=out, pred=self.pred, ring=self.ring,
                prev=self.prev, age=self.age, pring=self.pring, counts=self.counts, sums=self.sums,
                stream=_engine.current_stream(dev))
        else:
            _engine.caller("mpc_compensate_stale")(
                device=dev.index, B=B, R=R, reset=1 if reset else 0, params=self._params, latency=self.latency, obs=obs,
                command=None if reset else command, done=None if reset else done, out=out, pred=self.pred, ring=self.ring,
                prev=self.prev, age=self.age, pring=self.pring, counts=self.counts, sums=self.sums,
                stream=_engine.current_stream(dev))
        return out

    def _shape(self, delayed, prev):
        """act::shape of the nominal actuator (steps 6 - 8 of csrc/mpc_actuator.hpp) on [B, 2], the channels one after the other"""
        y = np.empty_like(delayed)
        for c in (0, 1):
            v, p = delayed[:, c], prev[:, c]
            yc = v
            if self.alpha[c] != 1.0:                                               # 6
                yc = p + self.alpha[c] * (v - p)
            if math.isfinite(self.rate[c]):                                        # 7
                m, d = self.rate[c] * self.dt, yc - p
                yc = np.where(d > m, p + m, np.where(d < -m, p - m, yc))
            lo, hi = self.limits[c]                                                # 8
            yc = np.where(yc < lo, lo, yc)
            y[:, c] = np.where(yc > hi, hi, yc)
        return y

    def _numpy_apply(self, obs, cmd, done, reset):
        """csrc/mpc_compensate.hpp over the batch: every statement acts on all environments -> (out, pred)"""
        B, d, L, dt, f64 = self.B, self.steps, self.latency, self.dt, np.float64
        ring, pring, prev, age, counts, sums = (t.cpu().numpy() for t in (self.ring, self.pring, self.prev, self.age,
                                                                          self.counts, self.sums))
        env, last, back = np.arange(B), COMP_RING - 1, d + L
        clear = np.ones(B, bool) if reset else np.zeros(B, bool) if done is None else done != 0
        ring[:, clear], pring[:, clear], prev[clear], age[clear] = 0.0, 0.0, 0.0, 0    # 1
        if reset:
            counts[:], sums[:] = 0, 0.0
        push = ~clear
        with np.errstate(invalid="ignore", over="ignore"):
            if push.any():                                                         # 2
                u = np.where((cmd - cmd) == 0.0, cmd, 0.0)
                ring[(age & last)[push], env[push]] = u[push]
                delayed = np.where((age >= back)[:, None], ring[(age - back) & last, env], 0.0)
                moved = push & (age >= L)                                          # prev advances only when the scene did
                prev[moved] = self._shape(delayed, prev)[moved]
                age[push] += 1
            x0, y0 = obs[:, 0, 1].astype(f64), obs[:, 0, 2].astype(f64)
            if back > 0:                                                           # 3
                scored = age >= back
                p = pring[(age - back) & last, env]
                dx, dy = p[:, 0] - x0, p[:, 1] - y0
                e = np.sqrt(dx * dx + dy * dy)
                counts[scored] += 1
                sums[0, scored] += e[scored]
                sums[1] = np.where(scored & (e > sums[1]), e, sums[1])
            vx, vy = obs[:, 0, 3].astype(f64), obs[:, 0, 4].astype(f64)                # 4
            x, y, th, sp = x0, y0, obs[:, 0, 5].astype(f64), np.sqrt(vx * vx + vy * vy)
            p = prev.copy()
            ahead = d + np.minimum(L, age)                                         # d + s, per environment
            for k in range(int(ahead.max(initial=0))):
                i = age - ahead + k
                run = k < ahead
                q = self._shape(np.where((i >= 0)[:, None], ring[i & last, env], 0.0), p)
                nx, ny, nth, nsp = _step_ego(x, y, th, sp, q, dt)
                p = np.where(run[:, None], q, p)
                x, y, th, sp = np.where(run, nx, x), np.where(run, ny, y), np.where(run, nth, th), np.where(run, nsp, sp)
            pring[age & last, env] = np.stack([x, y], axis=1)
            pred = np.stack([x, y, th, sp], axis=1)
            if back == 0:                                                          # 8
                out = obs.copy()
            else:
                s, c = np.sin(th), np.cos(th)                                          # 5
                out = np.zeros_like(obs)
                out[:, 0] = np.stack([np.ones(B), x, y, sp * c, sp * s, th, s, c], axis=1).astype(np.float32)
                h = (ahead.astype(f64) * dt)[:, None]                              # 6
                rows = obs[:, 1:]
                present = rows[:, :, 0] != 0.0
                moved = rows.copy()
                moved[:, :, 0] = 1.0
                moved[:, :, 1] = (rows[:, :, 1].astype(f64) + rows[:, :, 3].astype(f64) * h).astype(np.float32)
                moved[:, :, 2] = (rows[:, :, 2].astype(f64) + rows[:, :, 4].astype(f64) * h).astype(np.float32)
                moved[~present] = 0.0
                kx = moved[:, :, 1].astype(f64) - out[:, 0, 1].astype(f64)[:, None]        # 7
                ky = moved[:, :, 2].astype(f64) - out[:, 0, 2].astype(f64)[:, None]
                key = np.where(present, kx * kx + ky * ky, np.inf)
                order = np.argsort(key, axis=1, kind="stable")                     # ties, and the absent rows, in row order
                out[:, 1:] = np.take_along_axis(moved, order[:, :, None], axis=1)
        _write_back(((self.ring, ring), (self.pring, pring), (self.prev, prev), (self.age, age), (self.counts, counts),
                     (self.sums, sums)))
        return out, pred

    def totals(self) -> dict:
        """Since the reset, over the environments: scored (the predictions that were compared with the ego observed `steps`
        launches later), pos_err_mean and pos_err_max [m]: the mean and the maximum of their position error."""
        scored = int(self.counts.sum().item())
        s = self.sums.cpu().numpy()
        return dict(scored=scored, pos_err_mean=float(s[0].sum()) / max(scored, 1), pos_err_max=float(s[1].max(initial=0.0)))


class Latency:
    """Sensing latency in front of the agent's pipeline (csrc/mpc_latency.hpp states the update step by step): the scene handed
    on is the true scene of `steps` whole policy steps ago (0..7), bit for bit, every row.  A perception model and a tracker
    behind it then see the old frame from where the ego was then.  The first `steps` steps of an episode show the episode's
    first scene, growing older; a frame of a finished episode is never shown in the next one.

    `apply(obs, out, done, reset)` fills `out` [B, R, 8] f32 (not `obs`) from the true scene `obs` and returns it; done [B]:
    the environments whose episode ended on this step, so that obs is the first scene of a new one; reset=True starts every
    environment anew and zeroes the totals.  `stale` [B] i32 is the age, in steps, of the frame handed out by the last launch;
    `frames` [8, B, R, 8] f32 the last eight scenes, `age` [B] i32 the frames of the episode, `counts` [B] i64 the launches,
    `sums` [3, B] f64 the sum of stale, the sum and the maximum of the ego lag [m]: the distance between row 0 of obs and row
    0 of out.  Backend "hip" is the kernel (mpc_delay_scene, enqueue only, capturable); backend "torch" is the same update in
    numpy: the same bits but for the last bit of the lag's sqrt."""

    def __init__(self, B: int, device, backend: str = "torch", R: int = VEHICLES_COUNT, steps: int = 0):
        if backend not in ("hip", "torch"):
            raise ValueError("backend must be 'hip' or 'torch'")
        if int(B) < 0:
            raise ValueError("B must be >= 0")
        if not 1 <= int(R) <= MAX_ROWS:
            raise ValueError(f"R must be in 1..{MAX_ROWS}")
        if isinstance(steps, bool) or int(steps) != steps or not 0 <= int(steps) <= LAT_MAX_STEPS:
            raise ValueError(f"steps must be an integer 0..{LAT_MAX_STEPS}")
        self.B, self.R, self.device, self.backend, self.steps = int(B), int(R), torch.device(device), backend, int(steps)
        z = lambda *s, dt: torch.zeros(s, dtype=dt, device=self.device)
        self.frames = z(LAT_RING, self.B, self.R, 8, dt=torch.float32)
        self.age, self.stale, self.counts = z(self.B, dt=torch.int32), z(self.B, dt=torch.int32), z(self.B, dt=torch.int64)
        self.sums = z(3, self.B, dt=torch.float64)

    @property
    def config(self) -> dict:
        """The keyword arguments that make a Latency with the same model."""
        return dict(R=self.R, steps=self.steps)

    def reset(self) -> None:
        """Forget every frame and the totals.  `apply(..., reset=True)` does the same and then hands on the first scene."""
        for t in (self.frames, self.age, self.stale, self.counts, self.sums):
            t.zero_()

    def apply(self, obs, out, done=None, reset: bool = False):
        B, R, dev = self.B, self.R, self.device
        _check(obs, "obs", (B, R, 8), torch.float32, dev)
        _check(out, "out", (B, R, 8), torch.float32, dev)
        if out is obs or (B > 0 and out.data_ptr() == obs.data_ptr()):
            raise ValueError("out must not be obs")
        if done is not None:
            done = _check(done, "done", (B,), torch.uint8, dev)
        if self.backend == "torch":
            out.copy_(torch.from_numpy(self._numpy_apply(obs.cpu().numpy(), None if done is None else done.cpu().numpy(),
                                                         bool(reset))))
        else:
            _engine.caller("mpc_delay_scene")(
                device=dev.index, B=B, R=R, reset=1 if reset else 0, steps=self.steps, obs=obs,
                done=None if reset else done, out=out, stale=self.stale, frames=self.frames, age=self.age,
                counts=self.counts, sums=self.sums, stream=_engine.current_stream(dev))
        return out

    def _numpy_apply(self, obs, done, reset):
        """csrc/mpc_latency.hpp over the batch: every statement acts on all environments -> out"""
        B, f64 = self.B, np.float64
        frames, age, stale, counts, sums = (t.cpu().numpy() for t in (self.frames, self.age, self.stale, self.counts,
                                                                      self.sums))
        env, last = np.arange(B), LAT_RING - 1
        clear = np.ones(B, bool) if reset else np.zeros(B, bool) if done is None else done != 0
        age[clear] = 0                                                             # 1
        if reset:
            counts[:], sums[:] = 0, 0.0
        frames[age & last, env] = obs                                              # 2
        s = np.minimum(self.steps, age)                                            # 3
        out = frames[(age - s) & last, env]
        stale[:] = s
        dx = obs[:, 0, 1].astype(f64) - out[:, 0, 1].astype(f64)                   # 4
        dy = obs[:, 0, 2].astype(f64) - out[:, 0, 2].astype(f64)
        with np.errstate(invalid="ignore", over="ignore"):
            e = np.sqrt(dx * dx + dy * dy)
            counts += 1
            sums[0] += s
            sums[1] += e
            sums[2] = np.where(e > sums[2], e, sums[2])
        age += 1                                                                   # 5
        _write_back(((self.frames, frames), (self.age, age), (self.stale, stale), (self.counts, counts), (self.sums, sums)))
        return out

    def totals(self) -> dict:
        """Since the reset, over the environments: frames (the launches), stale_mean (the mean age of the frame handed out,
        in steps), ego_lag_mean and ego_lag_max [m]: the mean and the largest distance between the ego of the true scene and
        the ego of the frame handed out."""
        frames = int(self.counts.sum().item())
        s = self.sums.cpu().numpy()
        return dict(frames=frames, stale_mean=float(s[0].sum()) / max(frames, 1),
                    ego_lag_mean=float(s[1].sum()) / max(frames, 1), ego_lag_max=float(s[2].max(initial=0.0)))


def _keep_bits(keep) -> int:
    names = (keep,) if isinstance(keep, str) else tuple(keep)
    bits = 0
    for name in names:
        if name not in TRACE_KEEP:
            raise ValueError(f"keep: {name!r} is not one of {sorted(TRACE_KEEP)}")
        bits |= TRACE_KEEP[name]
    if bits == 0:
        raise ValueError("keep names no outcome")
    return bits


class EpisodeTraces:
    """The episodes an `EpisodeTrace` kept, on the host: `index` (dict of int arrays [n]: env - the global id, env_offset +
    b -, ordinal, steps, first, outcome, launch), `counts` (dict: matched, kept, dropped, launches), the store's planes cut to
    the n kept episodes (scene [n, W + 1, R, 8], seen [n, W, R, 8] or None, action [n, W, 2], reward [n, W], frame_i32
    [n, W, 3]; entries past an episode's L = min(steps, W) are whatever the store held) and `nbytes`, the memory the recorder
    took (running state, rings, work array and store).  `keep` is the bit set the recorder ran with.  plan_X [n, W, N + 1, 4]
    and plan_U [n, W, N, 2] (or None): the plan that produced each action frame, when the recorder ran with plan=True."""

    def __init__(self, index, counts, scene, seen, action, reward, frame_i32, keep, nbytes, plan_X=None, plan_U=None):
        self.index, self.counts, self.keep, self.nbytes = index, counts, int(keep), int(nbytes)
        self.scene, self.seen, self.action, self.reward, self.frame_i32 = scene, seen, action, reward, frame_i32
        self.plan_X, self.plan_U = plan_X, plan_U

    def __len__(self):
        return int(self.index["env"].shape[0])

    @property
    def window(self) -> int:
        return int(self.action.shape[1])

    def episode(self, i: int) -> dict:
        """Kept episode i in chronological order: its index fields as ints (env, ordinal, steps, first, outcome, launch),
        and of its last L = min(steps, W) steps action [L, 2], reward [L], status, iters, flags [L] (TRACE_FLAGS), scene
        [L + 1, R, 8] (scene k is the one step first + k started from; the last is the scene the episode ended in) and,
        when it was recorded, seen [L, R, 8] and plan_X [L, N + 1, 4], plan_U [L, N, 2] (frame k: the plan behind action k)."""
        if not 0 <= int(i) < len(self):
            raise IndexError(f"episode {i} of {len(self)}")
        out = {k: int(v[i]) for k, v in self.index.items()}
        L = min(out["steps"], self.window)
        out.update(action=self.action[i, :L].copy(), reward=self.reward[i, :L].copy(), status=self.frame_i32[i, :L, 0].copy(),
                   iters=self.frame_i32[i, :L, 1].copy(), flags=self.frame_i32[i, :L, 2].copy(),
                   scene=self.scene[i, :L + 1].copy())
        if self.seen is not None:
            out["seen"] = self.seen[i, :L].copy()
        if self.plan_X is not None:
            out.update(plan_X=self.plan_X[i, :L].copy(), plan_U=self.plan_U[i, :L].copy())
        return out

    def save(self, path) -> None:
        """One .npz with everything `load` needs."""
        arrays = {f"index_{k}": v for k, v in self.index.items()}
        arrays.update(counts=np.array([self.counts[k] for k in TRACE_COUNTS], np.int64), scene=self.scene, action=self.action,
                      reward=self.reward, frame_i32=self.frame_i32, keep=np.int64(self.keep), nbytes=np.int64(self.nbytes))
        if self.seen is not None:
            arrays["seen"] = self.seen
        if self.plan_X is not None:
            arrays.update(plan_X=self.plan_X, plan_U=self.plan_U)
        np.savez_compressed(path, **arrays)

    @classmethod
    def load(cls, path) -> "EpisodeTraces":
        with np.load(path) as z:
            return cls({k: z[f"index_{k}"] for k in TRACE_INDEX}, {k: int(v) for k, v in zip(TRACE_COUNTS, z["counts"])},
                       z["scene"], z["seen"] if "seen" in z.files else None, z["action"], z["reward"], z["frame_i32"],
                       int(z["keep"]), int(z["nbytes"]), z["plan_X"] if "plan_X" in z.files else None,
                       z["plan_U"] if "plan_U" in z.files else None)


class EpisodeTrace:
    """The step-by-step record of the episodes someone will look at (csrc/mpc_episode_trace.hpp has the model; layouts in
    include/mpc_mi355x.h, mpc_episode_trace): every environment keeps the last `window` steps of its current episode in
    rings on the device, and an episode of ordinal j < Q that ends with one of the outcomes in `keep` is copied, in
    chronological order, to the next free of `capacity` slots, ordered by (launch on which it ended, environment); one that
    finds the store full is counted as dropped.  keep: a name or an iterable of names from collision, truncated, success,
    unsolved, all; "failed" is collision | truncated.  seen=True also records what the agent acted on (with a perception
    model).  The `action` plane is what the environment was handed: in an evaluation with an actuator model (`Actuation`)
    the applied action, not the agent's command, so a trace can be replayed against the environment.  `update` after the
    environment's step is the kernel (backend "hip": enqueue only, capturable) or the same update in numpy (backend "torch",
    for the CPU environment); both give the same bytes.  Memory is bounded by B, window and capacity alone (`nbytes`).
    plan=True also keeps the plan behind every action frame (mpc_plan_trace, launched right after the recorder's own
    kernels with their `slot`; csrc/mpc_plan.hpp): plan_X [N + 1, 4] and plan_U [N, 2] per frame, N = `horizon`, the agent's."""

    def __init__(self, B: int, Q: int, device, backend: str = "torch", R: int = VEHICLES_COUNT, keep="failed",
                 capacity: int = 64, window: int = EPISODE_STEPS, seen: bool = False, env_offset: int = 0,
                 plan: bool = False, horizon: int | None = None):
        if backend not in ("hip", "torch"):
            raise ValueError("backend must be 'hip' or 'torch'")
        if int(B) < 0 or int(Q) < 1:
            raise ValueError("B must be >= 0 and episodes_per_env >= 1")
        if not 1 <= int(R) <= MAX_ROWS:
            raise ValueError(f"R must be 1..{MAX_ROWS}")
        if not 1 <= int(window) <= TRACE_MAX_WINDOW:
            raise ValueError(f"window must be 1..{TRACE_MAX_WINDOW}")
        if int(capacity) < 1:
            raise ValueError("capacity must be >= 1")
        self.B, self.Q, self.R, self.device, self.backend = int(B), int(Q), int(R), torch.device(device), backend
        self.W, self.C, self.keep, self.seen, self.env_offset = int(window), int(capacity), _keep_bits(keep), bool(seen), \
            int(env_offset)
        B, R, W, C = self.B, self.R, self.W, self.C
        z = lambda *s, dt: torch.zeros(s, dtype=dt, device=self.device)
        f32, f64, i32 = torch.float32, torch.float64, torch.int32
        self.state_i32 = z(4, B, dt=i32)                 # steps, crashed so far, unsolved so far, ordinal
        self.ring_scene, self.ring_seen = z(B, W + 1, R, 8, dt=f32), z(B, W, R, 8, dt=f32) if self.seen else None
        self.ring_act, self.ring_reward, self.ring_i32 = z(B, W, 2, dt=f64), z(B, W, dt=f32), z(B, W, 3, dt=i32)
        self.slot = z(B, dt=i32)
        self.kept_scene, self.kept_seen = z(C, W + 1, R, 8, dt=f32), z(C, W, R, 8, dt=f32) if self.seen else None
        self.kept_act, self.kept_reward, self.kept_i32 = z(C, W, 2, dt=f64), z(C, W, dt=f32), z(C, W, 3, dt=i32)
        self.index, self.counts = z(C, 6, dt=i32), z(4, dt=torch.int64)
        self.plan, self.N = bool(plan), None
        self.plan_state_i32 = self.ring_X = self.ring_U = self.kept_X = self.kept_U = None
        if self.plan:
            if horizon is None or not 1 <= int(horizon) <= PLAN_MAX_HORIZON:
                raise ValueError(f"plan=True needs horizon, the agent's, 1..{PLAN_MAX_HORIZON}")
            N = self.N = int(horizon)
            self.plan_state_i32 = z(2, B, dt=i32)            # steps, ordinal
            self.ring_X, self.ring_U = z(B, W, N + 1, 4, dt=f64), z(B, W, N, 2, dt=f64)
            self.kept_X, self.kept_U = z(C, W, N + 1, 4, dt=f64), z(C, W, N, 2, dt=f64)

    _PLAN_PLANES = ("plan_state_i32", "ring_X", "ring_U", "kept_X", "kept_U")
    _PLANES = ("state_i32", "ring_scene", "ring_seen", "ring_act", "ring_reward", "ring_i32", "slot", "kept_scene", "kept_seen",
               "kept_act", "kept_reward", "kept_i32", "index", "counts")
    _STORE = ("kept_scene", "kept_seen", "kept_act", "kept_reward", "kept_i32", "index")

    @staticmethod
    def bytes_for(B: int, R: int, W: int, C: int, seen: bool = False, plan: bool = False, horizon: int = 0) -> int:
        """The layout formula: running state and work array 20 B, rings ((W + 1) + [W]) 32 R + 32 W per environment; store
        ((W + 1) + [W]) 32 R + 32 W + 24 per slot; counts 32.  With plan: 8 B of running state per environment and
        W (48 N + 32) of plans per environment and per slot."""
        planes = ((W + 1) + (W if seen else 0)) * 32 * R + 32 * W
        plans = W * (48 * horizon + 32) if plan else 0
        return B * (20 + planes + (8 if plan else 0) + plans) + C * (planes + 24 + plans) + 32

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (getattr(self, n) for n in self._PLANES + self._PLAN_PLANES)
                   if t is not None)

    @property
    def config(self) -> dict:
        """The keyword arguments that make an EpisodeTrace with the same settings."""
        return dict(R=self.R, keep=[k for k, bit in TRACE_KEEP.items() if k != "failed" and self.keep & bit],
                    capacity=self.C, window=self.W, seen=self.seen, env_offset=self.env_offset,
                    **(dict(plan=True, horizon=self.N) if self.plan else {}))

    def observe(self, frame, reset=False):
        f = frame.get
        self.update(f("terminal_obs"), frame["obs"], f("seen") if self.seen else None, f("act"), f("reward"), f("done"),
                    f("truncated"), f("crashed"), f("arrived"), f("status"), f("iters"), reset,
                    plan_X=f("plan_X") if self.plan else None, plan_U=f("plan_U") if self.plan else None)

    def update(self, terminal_obs, obs, seen, action, reward, done, truncated, crashed, arrived, status, iters, reset=False,
               plan_X=None, plan_U=None):
        """After the reset of the environments (reset=True: only `obs` is read; the store is zeroed as well) and after every
        step, before the buffer the agent acted on is overwritten.  seen: that buffer when the recorder was built with
        seen=True, else None.  plan_X [B, N + 1, 4], plan_U [B, N, 2]: the step's plan when the recorder was built with
        plan=True, else None."""
        B, R, dev = self.B, self.R, self.device
        _check(obs, "obs", (B, R, 8), torch.float32, dev)
        if not reset:
            if (plan_X is not None or plan_U is not None) != self.plan:
                raise ValueError("plan_X and plan_U must be given exactly when the recorder was built with plan=True")
            if self.plan:
                _check(plan_X, "plan_X", (B, self.N + 1, 4), torch.float64, dev)
                _check(plan_U, "plan_U", (B, self.N, 2), torch.float64, dev)
        flags = {}
        if reset:
            for n in self._STORE + (("kept_X", "kept_U") if self.plan else ()):
                if getattr(self, n) is not None:
                    getattr(self, n).zero_()
            terminal_obs = seen = action = reward = status = iters = None
            flags = dict(done=None, truncated=None, crashed=None, arrived=None)
        else:
            if (seen is not None) != self.seen:
                raise ValueError("seen must be given exactly when the recorder was built with seen=True")
            _check(terminal_obs, "terminal_obs", (B, R, 8), torch.float32, dev)
            if self.seen:
                _check(seen, "seen", (B, R, 8), torch.float32, dev)
            _check(action, "action", (B, 2), torch.float64, dev)
            _check(reward, "reward", (B,), torch.float32, dev)
            _check(status, "status", (B,), torch.int32, dev)
            _check(iters, "iters", (B,), torch.int32, dev)
            for n, t in (("done", done), ("truncated", truncated), ("crashed", crashed), ("arrived", arrived)):
                flags[n] = _check(t, n, (B,), torch.uint8, dev)
        if self.backend == "torch":
            self._numpy_update(terminal_obs, obs, seen, action, reward, flags, status, iters, reset)
            if self.plan:
                self._numpy_plan(None if reset else plan_X, plan_U, flags["done"], reset)
            return
        _engine.caller("mpc_episode_trace")(
            device=self.device.index, B=B, R=R, Q=self.Q, W=self.W, C=self.C, keep=self.keep, reset=1 if reset else 0,
            terminal_obs=terminal_obs, obs=obs, seen=seen, action=action, reward=reward, **flags, status=status, iters=iters,
            **{n: getattr(self, n) for n in self._PLANES}, stream=_engine.current_stream(self.device))
        if self.plan:                                        # right after it, on the same stream: it reads that call's slot
            _engine.caller("mpc_plan_trace")(
                device=self.device.index, B=B, N=self.N, Q=self.Q, W=self.W, C=self.C, reset=1 if reset else 0,
                plan_X=None if reset else plan_X, plan_U=None if reset else plan_U, done=flags["done"], slot=self.slot,
                state_i32=self.plan_state_i32, ring_X=self.ring_X, ring_U=self.ring_U, kept_X=self.kept_X, kept_U=self.kept_U,
                stream=_engine.current_stream(self.device))

    def _numpy_plan(self, plan_X, plan_U, done, reset):
        """mpc_plan_trace (csrc/mpc_plan.hpp) over the batch, after `_numpy_update` has written this step's `slot`"""
        Q, W, C = self.Q, self.W, self.C
        planes = tuple(getattr(self, n) for n in self._PLAN_PLANES)
        st, ring_X, ring_U, kept_X, kept_U = (t.cpu().numpy() for t in planes)
        if reset:
            st[:] = 0
        else:
            X, U, done, slot = plan_X.cpu().numpy(), plan_U.cpu().numpy(), done.cpu().numpy() != 0, self.slot.cpu().numpy()
            t, j = st[0].copy(), st[1].copy()
            live = j < Q
            e = np.nonzero(live)[0]
            ring_X[e, t[e] % W], ring_U[e, t[e] % W] = X[e], U[e]
            for b in np.nonzero(live & done & (slot >= 0) & (slot < C))[0]:
                T = int(t[b]) + 1
                L = min(T, W)
                frames = (T - L + np.arange(L)) % W
                kept_X[slot[b], :L], kept_U[slot[b], :L] = ring_X[b, frames], ring_U[b, frames]
            st[0] = np.where(live, np.where(done, 0, t + 1), st[0])
            st[1] = j + (live & done)
        _write_back(zip(planes, (st, ring_X, ring_U, kept_X, kept_U)))

    def _numpy_update(self, terminal_obs, obs, seen, action, reward, flags, status, iters, reset):
        """csrc/mpc_episode_trace.hpp over the batch: the claim is a cumulative sum in environment order."""
        B, Q, W, C = self.B, self.Q, self.W, self.C
        host = {n: None if getattr(self, n) is None else getattr(self, n).cpu().numpy() for n in self._PLANES}
        si, counts, slot = host["state_i32"], host["counts"], host["slot"]
        n_ = lambda t: t.cpu().numpy()
        if reset:
            si[:], counts[:], slot[:] = 0, 0, -1
            host["ring_scene"][:, 0] = n_(obs)
        else:
            done, truncated, crashed, arrived = (n_(flags[k]) != 0 for k in ("done", "truncated", "crashed", "arrived"))
            status = n_(status)
            t, j = si[0].copy(), si[3].copy()
            live = j < Q
            crash_ever = (si[1] != 0) | crashed
            unsolved_ever = (si[2] != 0) | ~_solved(status)
            outcome = (crash_ever * 1 + truncated * 2 + arrived * 4 + unsolved_ever * 8).astype(np.int32)
            frame_flags = (done * 1 + truncated * 2 + crashed * 4 + arrived * 8).astype(np.int32)
            sel = live & done & (np.bool_(self.keep & 16) | ((outcome & self.keep & 15) != 0))
            place = int(counts[1]) + np.cumsum(sel) - 1
            slot[:] = np.where(sel & (place < C), place, -1)
            m = int(sel.sum())
            k = min(m, max(C - int(counts[1]), 0))
            counts += np.array([m, k, m - k, 1], np.int64)
            e = np.nonzero(live)[0]                          # append
            f = t[e] % W
            host["ring_scene"][e, (t[e] + 1) % (W + 1)] = n_(terminal_obs)[e]
            if self.seen:
                host["ring_seen"][e, f] = n_(seen)[e]
            host["ring_act"][e, f] = n_(action)[e]
            host["ring_reward"][e, f] = n_(reward)[e]
            host["ring_i32"][e, f] = np.stack([status, n_(iters), frame_flags], axis=1)[e]
            for b in np.nonzero(slot >= 0)[0]:               # commit, chronologically
                s, T = int(slot[b]), int(t[b]) + 1
                L = min(T, W)
                first = T - L
                frames, scenes = (first + np.arange(L)) % W, (first + np.arange(L + 1)) % (W + 1)
                host["kept_scene"][s, :L + 1] = host["ring_scene"][b, scenes]
                for name in ("seen", "act", "reward", "i32"):
                    if host["ring_" + name] is not None:
                        host["kept_" + name][s, :L] = host["ring_" + name][b, frames]
                host["index"][s] = [b, j[b], T, first, outcome[b], counts[3]]
            ends = live & done
            go = live & ~done
            si[0] = np.where(ends, 0, np.where(go, t + 1, si[0]))
            si[1] = np.where(ends, 0, np.where(go, crash_ever, si[1]))
            si[2] = np.where(ends, 0, np.where(go, unsolved_ever, si[2]))
            si[3] = j + ends
            host["ring_scene"][ends, 0] = n_(obs)[ends]
        _write_back((getattr(self, name), src) for name, src in host.items() if src is not None)

    def traces(self) -> EpisodeTraces:
        counts = {k: int(v) for k, v in zip(TRACE_COUNTS, self.counts.cpu().numpy())}
        n = counts["kept"]
        cut = lambda t: None if t is None else t[:n].cpu().numpy().copy()
        ix = cut(self.index)
        index = {k: ix[:, i].copy() for i, k in enumerate(TRACE_INDEX)}
        index["env"] = index["env"] + np.int32(self.env_offset)
        return EpisodeTraces(index, counts, cut(self.kept_scene), cut(self.kept_seen), cut(self.kept_act),
                             cut(self.kept_reward), cut(self.kept_i32), self.keep, self.nbytes, cut(self.kept_X),
                             cut(self.kept_U))


@dataclass
class EvalResult:
    """records: dict of numpy arrays [B, Q] (steps, success, collision, truncated, avg_speed, return, unsolved, max_iters);
    steps: policy steps the batch took; env_steps = steps * B; seconds: host clock around the stepping loop (it ends in a
    synchronise); drive: the drive metrics' records (dict of numpy arrays [B, Q], keys DRIVE_I32 + DRIVE_F64; slot [b, j]
    is the episode of records' slot [b, j]) when the evaluation ran with metrics=True, else None; perception: the totals of
    the perception model (`Perception.totals()`: rows present, seen, out_of_range, occluded, dropped over the whole
    evaluation, idle steps included) when the evaluation ran with one, else None; interaction: the interaction metrics'
    records (dict of numpy arrays [B, Q], keys INTERACT_I32 + INTERACT_F64, the same slots) when the evaluation ran with
    interaction=True, else None; traces: the episodes the trace recorder kept (`EpisodeTraces`) when the evaluation ran with
    trace=, else None; tracker: the totals of the tracker (`Tracker.totals()`: measured, matched, born, coasted, expired,
    evicted, cut over the whole evaluation, idle steps included) when the evaluation ran with one, else None; actuation: the
    totals of the actuator model (`Actuation.totals()`: steps, held, rate_limited, saturated, nonfinite, mean_abs_dev and
    max_abs_dev per channel, idle steps included) when the evaluation ran with one, else None; plan: the plan metrics'
    records (`PlanMetrics.records()`: dict of numpy arrays [B, Q], keys PLAN_I32 + PLAN_F64, the same slots, and `leads`) when
    the evaluation ran with plan=, else None; compensation: the totals of the delay compensator (`Compensation.totals()`:
    scored, pos_err_mean, pos_err_max) when the evaluation ran with one, else None; latency: the totals of the latency model
    (`Latency.totals()`: frames, stale_mean, ego_lag_mean, ego_lag_max, idle steps included) when the evaluation ran with one,
    else None."""
    records: dict
    dt: float
    steps: int
    env_steps: int
    seconds: float
    drive: dict | None = None
    perception: dict | None = None
    interaction: dict | None = None
    traces: EpisodeTraces | None = None
    tracker: dict | None = None
    actuation: dict | None = None
    plan: dict | None = None
    compensation: dict | None = None
    latency: dict | None = None

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
        largest of any episode).  With a perception model also seen_frac, occluded_frac, out_of_range_frac and dropped_frac:
        each class as a share of the present rows (0 when no row was ever present).  With the interaction metrics also:
        yield_step_frac and forced_brake_step_frac (states in which a vehicle yields to the ego / brakes for it harder than
        HARD_BRAKE, over all folded states), forced_brake_events_per_episode, max_forced_decel_mean and max_forced_decel_max
        over episodes, speed_deficit_per_episode [m/s], conflicts_per_episode, pet_critical_frac and ego_first_frac (of the
        conflicts; 0 when there is none) and min_pet_p05 (the 5th percentile of min_pet over the episodes with a conflict;
        inf when there is none).  With a tracker also coasted_frac: the output rows that were coasted, as a share of all
        output rows, coasted / (matched + born + coasted) (0 when there was none).  With an actuator model also act_held_frac,
        act_rate_limited_frac and act_saturated_frac (the steps on which a command was lost, the rate limit acted, the
        saturation acted, over all steps) and act_mean_abs_dev_accel [m/s^2], act_mean_abs_dev_steer [rad]: the mean of
        |applied - command| per channel.  With the plan metrics also plans_valid_frac (solved plans over all steps),
        plan_conflict_frac (steps whose planned clearance was below the gap, over the steps with a valid plan), min_plan_gap
        (the smallest of any episode, inf when there is none), pred_err_lead{h}_mean for every lead h in use (the mean
        distance between the ego and where the plan of h steps before put it, over all scored steps; 0 when there is none)
        and replan_accel_mean [m/s^2], replan_steer_mean [rad] (the mean replanning jump over all scored steps).  With a
        delay compensator also comp_pos_err_mean and comp_pos_err_max [m]: the mean and the largest distance between the ego
        it predicted and the ego observed `steps` steps later.  With a latency model also sense_stale_mean (the mean age, in
        steps, of the frame the agent's pipeline was handed) and sense_ego_lag_mean, sense_ego_lag_max [m]: how far the ego
        had moved on from that frame."""
        out = self._base_summary()
        if self.drive is not None:
            out.update(self._drive_summary())
        if self.perception is not None:
            present = max(self.perception["present"], 1)
            out.update({f"{k}_frac": self.perception[k] / present for k in ("seen", "occluded", "out_of_range", "dropped")})
        if self.interaction is not None:
            out.update(self._interaction_summary())
        if self.tracker is not None:
            t = self.tracker
            out["coasted_frac"] = t["coasted"] / max(t["matched"] + t["born"] + t["coasted"], 1)
        if self.actuation is not None:
            a = self.actuation
            out.update({f"act_{k}_frac": a[k] / max(a["steps"], 1) for k in ("held", "rate_limited", "saturated")})
            out.update(act_mean_abs_dev_accel=float(a["mean_abs_dev"][0]), act_mean_abs_dev_steer=float(a["mean_abs_dev"][1]))
        if self.plan is not None:
            out.update(self._plan_summary())
        if self.compensation is not None:
            out.update(comp_pos_err_mean=self.compensation["pos_err_mean"], comp_pos_err_max=self.compensation["pos_err_max"])
        if self.latency is not None:
            out.update(sense_stale_mean=self.latency["stale_mean"], sense_ego_lag_mean=self.latency["ego_lag_mean"],
                       sense_ego_lag_max=self.latency["ego_lag_max"])
        return out

    def _plan_summary(self) -> dict:
        d = self.plan
        valid = int(d["plans_valid"].sum())
        over = lambda mean, n: float((d[mean] * d[n]).sum()) / max(int(d[n].sum()), 1)     # the mean over all scored steps
        out = dict(plans_valid_frac=valid / max(int(d["steps"].sum()), 1),
                   plan_conflict_frac=int(d["plan_conflict_steps"].sum()) / max(valid, 1),
                   min_plan_gap=float(d["min_plan_gap"].min()) if d["min_plan_gap"].size else float("inf"),
                   replan_accel_mean=over("replan_accel_mean", "replan_n"), replan_steer_mean=over("replan_steer_mean", "replan_n"))
        out.update({f"pred_err_lead{h}_mean": over(f"lead{i}_mean", f"lead{i}_n") for i, h in enumerate(d["leads"]) if h})
        return out

    def _interaction_summary(self) -> dict:
        d = self.interaction
        n = int(d["steps"].size)
        steps_total = max(int(d["steps"].sum()), 1)
        conflicts = int(d["conflicts"].sum())
        pets = d["min_pet"][d["conflicts"] > 0]
        return dict(yield_step_frac=int(d["yield_steps"].sum()) / steps_total,
                    forced_brake_events_per_episode=int(d["forced_brake_events"].sum()) / n,
                    forced_brake_step_frac=int(d["forced_brake_steps"].sum()) / steps_total,
                    max_forced_decel_mean=float(d["max_forced_decel"].mean()),
                    max_forced_decel_max=float(d["max_forced_decel"].max()),
                    speed_deficit_per_episode=float(d["speed_deficit"].sum()) / n,
                    conflicts_per_episode=conflicts / n,
                    pet_critical_frac=int(d["pet_critical"].sum()) / max(conflicts, 1),
                    ego_first_frac=int(d["ego_first"].sum()) / max(conflicts, 1),
                    min_pet_p05=float(np.percentile(pets, 5)) if pets.size else float("inf"))

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


def _instance(cls, given, defaults: dict, *args):
    """`given` itself (an instance of cls, or None), or for a dict of cls's keyword arguments cls(*args, **them) with
    `defaults` for those it leaves out."""
    return cls(*args, **{**defaults, **given}) if isinstance(given, dict) else given


@torch.no_grad()
def evaluate_agent(agent, env, episodes_per_env: int = 1, deterministic: bool = False, reset_mpc_on_done: bool = False,
                   use_graph: bool | None = None, poll_every: int = 16, seed: int = 0, on_step=None,
                   metrics: bool = False, perception=None, interaction: bool = False, trace=None,
                   tracker=None, actuation=None, plan=None, compensation=None, latency=None) -> EvalResult:
    """Run `agent` in closed loop on the B environments of `env` (a SyntheticIntersectionEnv) until each environment has
    finished `episodes_per_env` episodes; returns their records.

    agent: PureMPC_Agent, IterativeLinearMPC_Agent, MPCRLAgent or PPOAgent (anything with `act_batch_torch`; the end-to-end
    PPOAgent may have no engine at all, there is then no MPC state to reset or reserve).  The MPC's action goes to the
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
    perception: a `Perception` for this environment's batch, or a dict of its keyword arguments (env_offset defaults to the
    environment's).  The agent then acts on `perception.apply(true observation)`, after the reset (reset=True) and after every
    step inside the step (so inside the captured graph); the accounting and the drive metrics keep reading the true scene
    and the environment's own flags.  on_step's dict then also holds obs (the true observation), seen (what the agent gets;
    the buffer is overwritten by the next step) and row_class; EvalResult.perception holds the totals.  None: nothing changes.
    interaction=True: also the interaction metrics of every episode (`InteractionMetrics`, EvalResult.interaction), updated
    after the drive metrics inside the step (so inside the captured graph) from the environment's slots; ValueError unless the
    environment has traffic="idm".  on_step's dict is unchanged.
    trace: an `EpisodeTrace` for this environment's batch and quota, or a dict of its keyword arguments (env_offset defaults to
    the environment's, seen to whether a perception model is in use): the step-by-step record of the selected episodes
    (EvalResult.traces), updated after the interaction metrics inside the step (so inside the captured graph) and before the
    buffer the agent acted on is overwritten.  Everything else, on_step's dict included, is what it is without it.
    tracker: a `Tracker` for this environment's batch, or a dict of its keyword arguments (dt defaults to the environment's):
    the agent then acts on `tracker.apply(...)` of what the perception model gives (which then writes into a buffer of its
    own), or of the true observation without one; launched right after perception.apply, after the reset (reset=True) and
    inside the step with the step's `done` (so inside the captured graph).  on_step's dict then also holds obs, seen (the
    tracker's output, what the agent gets), row_slot and row_miss; the trace recorder's `seen` is the tracker's output;
    EvalResult.tracker holds the totals.  The accounting and every metric keep reading the true scene.  None: nothing changes.
    actuation: an `Actuation` for this environment's batch, or a dict of its keyword arguments (dt and env_offset default to
    the environment's): the environment is handed `actuation.apply(command)` instead of the agent's command, launched between
    the agent's action and the environment's step (so inside the captured graph) with the `done` of the previous step, and
    reset where the observers get their reset frame, so the graph's warm-up and capture steps leave no trace.  Every
    observer's `act` is then the applied action, what the environment was handed - the drive metrics' `action`, and the
    `action` plane of a trace, which can therefore be replayed against the environment; on_step's dict then also holds act
    (applied) and command (the agent's output).  The agent's own memory of its last action stays its command.
    EvalResult.actuation holds the totals.  None: no launch, no buffer, nothing changes.
    plan (None and False: off): True, a dict of `PlanMetrics`'s keyword arguments such as dict(leads=(1, 5, 10, 20), gap=2.5) (N defaults to the
    agent's horizon, dt to the environment's; True is the empty dict: default_leads(N), the crash distance), or a PlanMetrics
    for this environment's batch and quota and the agent's horizon.  The agent is then asked for its plan
    (act_batch_torch(plan=True): the solve's planned states and controls, mpc_predict_batch_plan), and the plan metrics of
    every episode (EvalResult.plan) are updated after the interaction metrics and before the trace recorder inside the step
    (so inside the captured graph) from the plan, the observation the agent acted on and the scene after the step.
    on_step's dict then also holds plan_X, plan_U and plan_order (valid until the next step; the observation they were planned
    on is the previous call's obs, or seen).  A trace recorder with
    plan=True (a dict of its arguments gets horizon from the agent) asks for the plan in the same way.  ValueError for an
    agent without a plan (PPOAgent) and for leads beyond the horizon.  None: no launch, no buffer, nothing changes.
    compensation: a `Compensation` for this environment's batch, a dict of its keyword arguments (dt defaults to the
    environment's), or True for `Compensation.matching(actuation)` (ValueError without an actuator model).  The agent then
    acts on a buffer of its own, `ahead` = compensation.apply(what it would otherwise act on), filled right after perception
    and tracker: after the reset with reset=True, which also clears the compensator, so the graph's warm-up and capture steps
    leave no trace, and inside the step (so inside the captured graph) with the step's `done` and the agent's command - not
    the applied action: the compensator knows the nominal actuator, not the real one.  `seen` - on_step's, the frame's and
    the trace recorder's (seen=True is then allowed with a compensator alone) - is `ahead`, what the agent acted on; on_step's
    dict also holds it as ahead.  EvalResult.compensation holds the totals.  ValueError with plan= or a trace with plan=True
    when steps > 0: the plan then starts `steps` later than the plan metrics' leads assume.  None: no launch, no buffer,
    nothing changes.
    latency: a `Latency` for this environment's batch, a dict of its keyword arguments, or an int, its `steps`: the sensing
    stages and the agent are handed the true scene of `steps` steps ago, `latency.apply(true observation)`, the first launch
    of what the agent gets: after the reset (always with reset=True, like the compensator, with which it has to count the
    episode's steps alike) and inside the step with the step's `done` (so inside the captured graph), in front of the
    perception model and the tracker, which see the old frame from where the ego was then.  It counts as a filter: on_step's
    dict then holds obs (the true observation), seen (what the agent gets) and stale (the age of that frame per
    environment), and a trace may record seen=True with it alone.  EvalResult.latency holds the totals.  The accounting and
    every metric keep reading the true scene.  compensation=True is then `Compensation.matching(actuation, latency)`, of
    whichever of the two is present.  ValueError with plan= or a trace with plan=True when latency.steps > 0, for the
    compensator's reason: the plan starts from another step than the plan metrics' leads assume.  None: no launch, no buffer,
    nothing changes.
    Every episode ends by EPISODE_STEPS (200) steps, so Q * 200 steps bound the loop; RuntimeError if the episodes are not
    all recorded by then."""
    Q = int(episodes_per_env)
    if Q < 1:
        raise ValueError("episodes_per_env must be >= 1")
    if int(poll_every) < 1:
        raise ValueError("poll_every must be >= 1")
    if not callable(getattr(agent, "act_batch_torch", None)):
        raise ValueError(f"unsupported agent {type(agent).__name__}: needs act_batch_torch (PureMPC_Agent, "
                         "IterativeLinearMPC_Agent, MPCRLAgent, PPOAgent)")
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
    backend, offset = "hip" if hip else "torch", int(getattr(env, "env_offset", 0))
    obs = torch.zeros((B, VEHICLES_COUNT, 8), dtype=torch.float32, device=dev)     # the observation the agent acts on
    if interaction and getattr(env, "traffic", None) != "idm":
        raise ValueError("interaction=True needs an environment with traffic='idm'")
    perception = _instance(Perception, perception, dict(env_offset=offset), B, dev, backend)
    if perception is not None and (perception.B != B or perception.R != VEHICLES_COUNT or perception.device != dev):
        raise ValueError(f"perception must be built for {B} environments of {VEHICLES_COUNT} rows on {dev}")
    tracker = _instance(Tracker, tracker, dict(R=VEHICLES_COUNT, dt=float(env.dt)), B, dev, backend)
    if tracker is not None and (tracker.B != B or tracker.R != VEHICLES_COUNT or tracker.device != dev):
        raise ValueError(f"tracker must be built for {B} environments of {VEHICLES_COUNT} rows on {dev}")
    actuation = _instance(Actuation, actuation, dict(dt=float(env.dt), env_offset=offset), B, dev, backend)
    if actuation is not None and (actuation.B != B or actuation.device != dev):
        raise ValueError(f"actuation must be built for {B} environments on {dev}")
    # with an actuator model: what the environment is handed, and the `done` of the previous step (zero after the reset)
    applied = torch.zeros((B, 2), dtype=torch.float64, device=dev) if actuation is not None else None
    ended = torch.zeros(B, dtype=torch.uint8, device=dev) if actuation is not None else None
    if isinstance(latency, int) and not isinstance(latency, bool):
        latency = dict(steps=latency)
    latency = _instance(Latency, latency, dict(R=VEHICLES_COUNT), B, dev, backend)
    if latency is not None and (not isinstance(latency, Latency) or latency.B != B or latency.R != VEHICLES_COUNT or
                                latency.device != dev):
        raise ValueError(f"latency must be built for {B} environments of {VEHICLES_COUNT} rows on {dev}")
    if compensation is True:
        if actuation is None and latency is None:
            raise ValueError("compensation=True is Compensation.matching(actuation, latency): it needs an actuator model or "
                             "a latency model")
        compensation = Compensation.matching(actuation, latency, R=VEHICLES_COUNT, dt=float(env.dt))
    compensation = _instance(Compensation, compensation, dict(R=VEHICLES_COUNT, dt=float(env.dt)), B, dev, backend)
    if compensation is not None and (compensation.B != B or compensation.R != VEHICLES_COUNT or compensation.device != dev):
        raise ValueError(f"compensation must be built for {B} environments of {VEHICLES_COUNT} rows on {dev}")
    sensing = perception is not None or tracker is not None        # `obs` is something other than the true scene
    # the agent acts on something other than the true scene
    filtered = sensing or compensation is not None or latency is not None
    sensed = torch.zeros_like(obs) if perception is not None and tracker is not None else None    # between the two
    # with a latency model and a sensing stage behind it: the old true scene, between the two
    late = torch.zeros_like(obs) if latency is not None and sensing else None
    # with a compensator: the predicted scene, what the agent acts on
    ahead = torch.zeros_like(obs) if compensation is not None else None
    acting = obs if compensation is None else ahead
    horizon = getattr(eng, "horizon", None)
    plan = {} if plan is True else None if plan is False else plan
    trace_plan = bool(trace.get("plan")) if isinstance(trace, dict) else bool(getattr(trace, "plan", False))
    wants_plan = plan is not None or trace_plan
    if wants_plan and (not getattr(agent, "HAS_PLAN", True) or horizon is None or
                       "plan" not in inspect.signature(agent.act_batch_torch).parameters):
        raise ValueError(f"{type(agent).__name__} has no plan: plan= and a trace with plan=True need an MPC agent")
    if wants_plan and compensation is not None and compensation.steps > 0:
        raise ValueError("plan= and a trace with plan=True are not supported with a compensator of steps > 0: the plan then "
                         "starts `steps` later than the plan metrics' leads assume")
    if wants_plan and latency is not None and latency.steps > 0:
        raise ValueError("plan= and a trace with plan=True are not supported with a latency of steps > 0: the plan then "
                         "starts from another step than the plan metrics' leads assume")
    trace = _instance(EpisodeTrace, trace, dict(R=VEHICLES_COUNT, env_offset=offset, seen=filtered,
                                                **(dict(horizon=horizon) if trace_plan else {})), B, Q, dev, backend)
    if trace is not None:
        if (trace.B, trace.Q, trace.R, trace.device) != (B, Q, VEHICLES_COUNT, dev):
            raise ValueError(f"trace must be built for {B} environments, {Q} episodes each, {VEHICLES_COUNT} rows, on {dev}")
        if trace.seen and not filtered:
            raise ValueError("trace records seen=True only with a perception model, a tracker, a compensator or a latency model")
        if trace.plan and trace.N != horizon:
            raise ValueError(f"trace keeps plans of horizon {trace.N}, the agent's is {horizon}")
    planm = _instance(PlanMetrics, plan, dict(N=horizon, R=VEHICLES_COUNT, dt=float(env.dt)), B, Q, dev, backend)
    if planm is not None and (planm.B, planm.Q, planm.N, planm.R, planm.device) != (B, Q, horizon, VEHICLES_COUNT, dev):
        raise ValueError(f"plan must be built for {B} environments, {Q} episodes each, horizon {horizon}, "
                         f"{VEHICLES_COUNT} rows, on {dev}")
    stats = EpisodeStats(B, Q, dev, backend)
    drive = DriveMetrics(B, Q, dev, backend, env.ref_xy, env.dt, VEHICLES_COUNT) if metrics else None
    inter = InteractionMetrics(B, Q, dev, backend, env.ref_xy, env.dt, env.K) if interaction else None
    # The order of a step's launches, after the agent's and the environment's: the accounting, the drive metrics, the
    # interaction metrics, the plan metrics, the trace recorder - each `observe` of the step's frame - and then perception.apply and
    # tracker.apply (or the plain copy), which overwrite the buffer the agent acted on: the recorder has to have read it by
    # then.
    observers = [o for o in (stats, drive, inter, planm, trace) if o is not None]
    kw = dict(deterministic=bool(deterministic), seed=int(seed), env_offset=offset)
    if wants_plan:
        kw["plan"] = True
    # what on_step is shown of a frame: the accounting's inputs; with metrics=True also the scenes and the action; with a
    # perception model also the true observation, what the agent gets next and (below) the class of every row
    shown = ("ego", "done", "truncated", "crashed", "arrived", "reward", "status", "iters") + \
        (("terminal_obs", "obs", "act") if metrics else ()) + (("obs", "seen") if filtered else ()) + \
        (("act", "command") if actuation is not None else ()) + (("ahead",) if compensation is not None else ()) + \
        (("plan_X", "plan_U", "plan_order") if wants_plan else ())

    def show(frame, **first):
        first.update((k, frame[k]) for k in shown if k in frame)
        if perception is not None:
            first["row_class"] = perception.row_class
        if tracker is not None:
            first["row_slot"], first["row_miss"] = tracker.row_slot, tracker.row_miss
        if latency is not None:
            first["stale"] = latency.stale
        on_step(first)

    def sense(true, reset=False, done=None):
        """`obs` <- what the agent gets of the true observation"""
        if latency is not None:       # first: every stage behind it sees the true scene of `steps` steps ago; a scene without
            # a step's `done` is a first scene: always a reset launch, like the compensator's, so both count the same steps
            true = latency.apply(true, late if sensing else obs, done=done, reset=done is None)
        if not sensing:
            if latency is None:
                obs.copy_(true)
        elif tracker is None:
            perception.apply(true, obs, reset=reset)
        else:
            meas = true if perception is None else perception.apply(true, sensed, reset=reset)
            tracker.apply(meas, obs, done=done, reset=reset)

    def step():
        out = agent.act_batch_torch(acting, **kw)
        act = out["act"] if actuation is None else actuation.apply(out["act"], applied, done_prev=ended)
        new_obs, reward, done, info = env.step(act)
        if reset_mpc_on_done and eng is not None:
            eng.reset_env_mask_torch(_u8(done))
        elif warm:                    # a new episode must not start from the old one's plan
            eng.reset_env_mask_torch(_u8(done), warm_only=True)
        frame = dict(env=env, ego=env.ego, terminal_obs=info["terminal_obs"], obs=new_obs, act=act, reward=reward,
                     done=done, truncated=info["truncated"], crashed=info["crashed"], arrived=info["arrived"],
                     status=out["status"], iters=out["iters"], step=out.get("step"))
        if filtered:
            frame["seen"] = acting    # still what the agent acted on while the observers run; what it gets next after them
        if actuation is not None:
            frame["command"] = out["act"]
        if compensation is not None:
            frame["ahead"] = ahead
        if wants_plan:                # `acted`: the observation the agent acted on, until `sense` overwrites it
            frame.update(plan_X=out["plan_X"], plan_U=out["plan_U"], plan_order=out["plan_order"], acted=acting)
        for o in observers:
            o.observe(frame)
        if actuation is not None:
            ended.copy_(done)
        sense(new_obs, done=done)
        if compensation is not None:
            compensation.apply(obs, ahead, command=out["act"], done=done)
        return out, frame

    def first_obs(reset):
        true = env.reset()
        sense(true, reset=reset)
        if compensation is not None:  # a scene without a command: always a reset launch, which also clears the compensator
            compensation.apply(obs, ahead, reset=True)
        return true if filtered else obs

    graph = None
    if use_graph:
        # warm-up and capture really step the environment: its state is put back afterwards, and the resets below start the
        # evaluation from there, so a graph run and an eager run see the same episodes
        if eng is not None:
            eng.reserve_envs(B)
        snap = {n: t.clone() for n, t in env.state_tensors().items()}
        gen_state = env.gen.get_state()
        first_obs(False)
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
        for n, t in env.state_tensors().items():
            t.copy_(snap[n])
        env.gen.set_state(gen_state)

    true0 = first_obs(True)                  # `obs` itself without a perception model or a tracker
    if hasattr(agent, "reset_env_state"):
        agent.reset_env_state()
    elif hasattr(eng, "reset_env_state"):
        eng.reset_env_state()
    if hasattr(agent, "restart_actions"):
        agent.restart_actions()
    frame = dict(env=env, ego=env.ego, obs=true0)
    if filtered:
        frame["seen"] = acting
    if compensation is not None:
        frame["ahead"] = ahead
    for o in observers:
        o.observe(frame, reset=True)
    if actuation is not None:
        actuation.reset()
        ended.zero_()
    if on_step is not None:
        show(frame, reset=True)
    target, max_steps = B * Q, Q * EPISODE_STEPS
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    n, recorded = 0, 0
    while n < max_steps:
        if graph is not None:
            graph.replay()
        else:
            _, frame = step()
            if on_step is not None:
                show(frame)
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
                      drive=None if drive is None else drive.records(),
                      perception=None if perception is None else perception.totals(),
                      interaction=None if inter is None else inter.records(),
                      traces=None if trace is None else trace.traces(),
                      tracker=None if tracker is None else tracker.totals(),
                      actuation=None if actuation is None else actuation.totals(),
                      plan=None if planm is None else planm.records(),
                      compensation=None if compensation is None else compensation.totals(),
                      latency=None if latency is None else latency.totals())


def compare(agents: dict, make_env, episodes_per_env: int = 1, metrics: bool = False, perception=None,
            interaction: bool = False, trace=None, results=None, tracker=None, actuation=None, plan=None, compensation=None,
            latency=None, **kw) -> dict:
    """Evaluate every agent on a fresh environment from make_env() (same seed: the HIP environment keys its draws by seed and
    environment id, so every agent meets the same initial episodes) -> {name: summary}; metrics=True adds the drive metrics'
    keys to every summary.  perception (a dict of `Perception`'s keyword arguments, or a Perception whose configuration is
    copied): every agent gets a fresh Perception with the same seed, hence the same draws on the same steps.
    interaction=True adds the interaction metrics' keys (the environments must have traffic="idm").  trace (a dict of
    `EpisodeTrace`'s keyword arguments, or an EpisodeTrace whose settings are copied): every agent gets a fresh recorder with
    the same settings.  tracker (a dict of `Tracker`'s keyword arguments, or a Tracker whose configuration is copied): every
    agent gets a fresh tracker.  actuation (a dict of `Actuation`'s keyword arguments, or an Actuation whose configuration is
    copied): every agent gets a fresh actuator model with the same seed, hence the same draws on the same steps.  plan (True, a dict of `PlanMetrics`'s keyword arguments, or a PlanMetrics whose settings are
    copied): every agent gets fresh plan metrics; an agent without a plan (PPOAgent) is evaluated without them.  compensation
    (True, a dict of `Compensation`'s keyword arguments, or a Compensation whose configuration is copied): every agent gets a
    fresh compensator; True is the one that matches every agent's fresh actuator model and latency model.  latency (an int, a dict of `Latency`'s keyword
    arguments, or a Latency whose configuration is copied): every agent gets a fresh latency model.  results: a dict that receives every agent's EvalResult by name (its traces, its records)."""
    perception, trace, tracker, actuation, plan, compensation, latency = (
        x.config if isinstance(x, (Perception, EpisodeTrace, Tracker, Actuation, PlanMetrics, Compensation, Latency)) else x
        for x in (perception, trace, tracker, actuation, plan, compensation, latency))
    plan = {} if plan is True else None if plan is False else plan
    fresh = lambda settings: None if settings is None else dict(settings)
    out = {}
    for name, agent in agents.items():
        planned = getattr(agent, "HAS_PLAN", True)
        settings = fresh(trace)
        if settings is not None and not planned:         # the recorder of an agent without a plan keeps no plan planes
            settings.pop("plan", None), settings.pop("horizon", None)
        res = evaluate_agent(agent, make_env(), episodes_per_env, metrics=metrics, perception=fresh(perception),
                             interaction=interaction, trace=settings, tracker=fresh(tracker), actuation=fresh(actuation),
                             plan=fresh(plan) if planned else None,
                             compensation=compensation if compensation is True else fresh(compensation),
                             latency=fresh(latency) if isinstance(latency, dict) else latency, **kw)
        if results is not None:
            results[name] = res
        out[name] = res.summary()
    return out
