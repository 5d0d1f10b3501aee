"""MPC-in-the-loop rollout collection for many parallel environments (BASELINE configs 4-5).

The reference collects experience with ONE environment and one MPC solve per step:
    policy(obs) -> clip -> mpc_agent.predict(obs, weights_from_RL | ref_speed) -> env.step(mpc_action) -> buffer.add
(`PPO_MPC.collect_rollouts` agents/ppo_mpc.py:353-483, `A2C_MPC.collect_rollouts` agents/a2c_mpc.py:111-180, both
copies of stable-baselines3's on-policy loop with the MPC call spliced in).  `BatchedCollector` is that loop for B
environments at once with every tensor resident on the GPU: the policy is a torch module, the MPC call is
`MPCEngine.predict_batch_torch` (one C-ABI call: device preamble + solve, zero-copy on torch's stream), the
environment steps as vectorised torch ops, and the buffer is a set of device tensors.  With `torch.distributed`
initialised the environments are sharded over the ranks and the MPC actions are all-gathered (RCCL) every step,
the path's only exchange.

highway-env, gymnasium and stable-baselines3 are not available offline, so
  * `SyntheticIntersectionEnv` is a stand-in with the reference's observation layout (config/config.py:10-26:
    10 rows x [presence, x, y, vx, vy, heading, sin_h, cos_h], absolute, sorted by distance), its ego route (the
    reference path of agents/base_agent.py:118-154), the MPC's own vehicle model for the ego (agents/pure_mpc.py:
    220-228), constant-velocity traffic on the four approach lanes, and the reward / termination *shape* of
    envs/intersection_env_Feb2025_v1.py:80-155 (collision, speed, arrival, lane centring, off-road; crash or arrival
    terminates, 200 steps truncate).  It is scaffolding for throughput measurements, not a re-implementation of
    highway-env.
  * `ActorCritic` has the shape of SB3's default `MlpPolicy` used by the reference's `create_ppo_policy /
    create_a2c_policy` (trainers/trainer_utils.py:6-45): flattened 80-d observation, separate 64-64 tanh towers
    for policy and value, diagonal Gaussian over a Box(-1, 1)^dim action (dim 1 = reference speed "v0",
    dim 3 = cost weights "v1", trainers/trainer.py:422-428).
  * `RolloutBuffer.compute_returns_and_advantage` is generalised advantage estimation as SB3 defines it, and
    `OnPolicyTrainer` the PPO / A2C parameter update of the reference's `train()` methods, so that a whole
    collect -> update loop runs without stable-baselines3.
"""
from __future__ import annotations

import os

import math

import numpy as np
import torch

from . import engine as _engine
from .reference_path import reference_states

VEHICLES_COUNT = 10        # config/cfg.yaml:2
EPISODE_STEPS = 200        # duration 10 s + 10 s at 10 Hz (envs/intersection_env_Feb2025_v1.py:153-155, config.py:41)
REWARD = dict(collision=-200.0, high_speed=15.0, arrived=50.0, center_bonus=5.0, off_road=-50.0)  # env :47-52,:96-107
LANE_HALF_WIDTH = 2.0
CRASH_DISTANCE = 2.5
WHEELBASE = 2.5


class SyntheticIntersectionEnv:
    """B independent intersection episodes stepped together on one device (auto-reset like an SB3 VecEnv).

    Two implementations of the same step behind this class: on a GPU the fused HIP kernel `mpc_synth_env_step`
    (the statements of csrc/mpc_synth_env.hpp run by sixteen lanes per environment, csrc/mpc_synth_lanes.hpp: vehicle models,
    respawn, reward, termination, terminal observation, auto-reset and the next observation in ONE launch, counter-based
    random numbers) - `backend="hip"`, the default there; on the CPU, or with
    `backend="torch"`, the vectorised torch ops below (about a hundred small kernels per step on a GPU).  Same state
    tensors, same return values; the two draw different random streams (as torch's CPU and GPU generators do), the
    deterministic part of the step is identical (tests/test_rollout_cpu.py, tests/test_predict_gpu.py).

    traffic="constant" (default): the other vehicles drive straight on at constant velocity.  traffic="idm": they follow one of
    twelve routes through the junction (straight, left, right), keep their distance with the Intelligent Driver Model and brake
    for what is in the corridor in front of them, the ego included (csrc/mpc_synth_traffic.hpp, `mpc_synth_env_step_idm`); three
    more state tensors: oroute (3 * entry + turn), oprog (arc length), otarget (desired speed)."""

    def __init__(self, num_envs: int, device="cpu", seed: int = 0, n_others: int = 4, dt: float = 0.1,
                 spawn_probability: float = 0.3, backend: str = "auto", env_offset: int = 0, traffic: str = "constant"):
        assert 0 <= n_others <= VEHICLES_COUNT - 1
        if traffic not in ("constant", "idm"):
            raise ValueError("traffic must be constant|idm")
        self.traffic = traffic
        self.num_envs, self.K, self.dt = int(num_envs), int(n_others), float(dt)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            # an indexed device, resolved once: the fused step hands the ordinal to hipSetDevice, and "cuda" without an index
            # means the CURRENT device (torch.cuda.set_device(local_rank) under torchrun), not device 0
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.spawn_probability = float(spawn_probability)
        if backend not in ("auto", "hip", "torch"):
            raise ValueError("backend must be auto|hip|torch")
        self.backend = ("hip" if self.device.type == "cuda" else "torch") if backend == "auto" else backend
        if self.backend == "hip" and self.device.type != "cuda":
            raise ValueError("the fused environment step needs a GPU device")
        self.seed, self.env_offset = int(seed), int(env_offset)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(int(seed))
        ref = reference_states(dt)
        self.ref_xy = torch.as_tensor(np.ascontiguousarray(ref[:, :2]), dtype=torch.float64, device=self.device)
        self.M = ref.shape[0]
        B, K = self.num_envs, max(self.K, 1)
        self.ego = torch.zeros((B, 4), dtype=torch.float64, device=self.device)      # x, y, heading, speed
        self.opos = torch.zeros((B, K, 2), dtype=torch.float64, device=self.device)
        self.ospeed = torch.zeros((B, K), dtype=torch.float64, device=self.device)
        self.ohead = torch.zeros((B, K), dtype=torch.float64, device=self.device)
        self.oactive = torch.zeros((B, K), dtype=torch.bool, device=self.device)
        self.t = torch.zeros(B, dtype=torch.int32, device=self.device)
        self._lane_h = torch.tensor([0.0, math.pi / 2, math.pi, -math.pi / 2], dtype=torch.float64, device=self.device)
        if self.traffic == "idm":           # csrc/mpc_synth_traffic.hpp: route = 3 * entry + turn, arc length, desired speed
            self.oroute = torch.zeros((B, K), dtype=torch.int32, device=self.device)
            self.oprog = torch.zeros((B, K), dtype=torch.float64, device=self.device)
            self.otarget = torch.ones((B, K), dtype=torch.float64, device=self.device)
            self._lane_dx = torch.tensor([1.0, 0.0, -1.0, 0.0], dtype=torch.float64, device=self.device)
            self._lane_dy = torch.tensor([0.0, 1.0, 0.0, -1.0], dtype=torch.float64, device=self.device)
        if self.backend == "hip":
            _engine.load_library()          # a missing library fails here, not at the first step
            self.rng_counter = torch.zeros(B, dtype=torch.int64, device=self.device)
            u8 = lambda: torch.zeros(B, dtype=torch.uint8, device=self.device)
            # outputs of the step live at fixed addresses (a captured hipGraph replays against them)
            self._out = dict(obs=torch.zeros((B, VEHICLES_COUNT, 8), dtype=torch.float32, device=self.device),
                             terminal_obs=torch.zeros((B, VEHICLES_COUNT, 8), dtype=torch.float32, device=self.device),
                             reward=torch.zeros(B, dtype=torch.float32, device=self.device),
                             done=u8(), truncated=u8(), crashed=u8(), arrived=u8())

    # ---- fused implementation (csrc/mpc_synth_env.hpp) ---------------------------------------------------------------
    def _hip_call(self, action, reset_all):
        idm = {n: getattr(self, n) for n in ("oroute", "oprog", "otarget")} if self.traffic == "idm" else {}
        _engine.caller("mpc_synth_env_step_idm" if idm else "mpc_synth_env_step")(
            device=self.device.index, B=self.num_envs, K=self.K, dt=self.dt, spawn_probability=self.spawn_probability,
            seed=self.seed, env_offset=self.env_offset, ref_xy=self.ref_xy, M=self.M, action=action, ego=self.ego,
            opos=self.opos, ospeed=self.ospeed, ohead=self.ohead, oactive=self.oactive, **idm, t=self.t,
            rng_counter=self.rng_counter, **self._out, reset_all=1 if reset_all else 0,
            stream=_engine.current_stream(self.device))

    def state_tensors(self) -> dict:
        """name -> tensor of everything a step changes besides its outputs and the torch generator `gen`: what a caller
        that steps for a graph capture snapshots and puts back (in place: the graph replays against these addresses)."""
        names = ("ego", "opos", "ospeed", "ohead", "oactive", "oroute", "oprog", "otarget", "t", "rng_counter")
        return {n: getattr(self, n) for n in names if hasattr(self, n)}

    # ---- random helpers ------------------------------------------------------------------------------------
    def _u(self, shape, lo, hi):
        return lo + (hi - lo) * torch.rand(shape, generator=self.gen, device=self.device, dtype=torch.float64)

    def _spawn_others(self, shape, dlo, dhi):
        """Vehicles on the four approach lanes driving towards the centre (right-hand traffic, lane offset 2 m)."""
        lane = torch.randint(0, 4, shape, generator=self.gen, device=self.device)
        h = self._lane_h[lane]
        d = self._u(shape, dlo, dhi)
        x = -d * torch.cos(h) + torch.where(lane == 1, -2.0, 0.0) + torch.where(lane == 3, 2.0, 0.0)
        y = -d * torch.sin(h) + torch.where(lane == 0, 2.0, 0.0) + torch.where(lane == 2, -2.0, 0.0)
        sp = torch.clamp(8.0 + torch.randn(shape, generator=self.gen, device=self.device, dtype=torch.float64), min=0.0)
        return torch.stack([x, y], dim=-1), sp, h

    # ---- reactive traffic (traffic="idm"; the torch statement of csrc/mpc_synth_traffic.hpp) -----------------------------
    def pose(self, route, s):
        """Position [..., 2] and heading of arc length s on route = 3 * entry + turn (0 straight, 1 left, 2 right): the approach
        lane up to s = 50, then a quarter circle (radius 8 right, 12 left) onto the exit arm's lane, then straight on."""
        entry = torch.div(route, 3, rounding_mode="floor").long()
        turn = route.long() - 3 * entry
        dx, dy, h0 = self._lane_dx[entry], self._lane_dy[entry], self._lane_h[entry]
        nx, ny = -dy, dx
        u = s - 50.0
        sgn = torch.where(turn == 2, 1.0, -1.0).to(torch.float64)          # right: centre -10 d + 10 n, heading h + phi
        R = torch.where(turn == 2, 8.0, 12.0).to(torch.float64)
        length = R * (math.pi / 2)
        straight = (turn == 0) | (u <= 0.0)
        phi = torch.clamp(u, min=0.0) / R
        on_arc = u <= length
        phi = torch.where(on_arc, phi, torch.full_like(phi, math.pi / 2))
        r = torch.where(on_arc, torch.zeros_like(u), u - length)           # beyond the arc: along sgn * n from its end
        c, sn = torch.cos(phi), torch.sin(phi)
        ax = (-10.0 * dx + sgn * 10.0 * nx) + R * (-sgn * nx * c + dx * sn) + r * sgn * nx
        ay = (-10.0 * dy + sgn * 10.0 * ny) + R * (-sgn * ny * c + dy * sn) + r * sgn * ny
        x = torch.where(straight, (s - 60.0) * dx + 2.0 * nx, ax)
        y = torch.where(straight, (s - 60.0) * dy + 2.0 * ny, ay)
        h = torch.where(straight, h0, h0 + sgn * phi)
        h = torch.where(h > math.pi, h - 2 * math.pi, h)
        h = torch.where(h <= -math.pi, h + 2 * math.pi, h)
        return torch.stack([x, y], dim=-1), h

    def _draw_vehicles(self, shape, dlo, dhi):
        """Entry lane, distance from the centre, turn and speed of new vehicles; the desired speed is the drawn one, at least 1."""
        lane = torch.randint(0, 4, shape, generator=self.gen, device=self.device)
        turn = torch.randint(0, 3, shape, generator=self.gen, device=self.device)
        route = (3 * lane + turn).to(torch.int32)
        s = 60.0 - self._u(shape, dlo, dhi)
        sp = torch.clamp(8.0 + torch.randn(shape, generator=self.gen, device=self.device, dtype=torch.float64), min=0.0)
        pos, h = self.pose(route, s)
        return route, s, sp, torch.clamp(sp, min=1.0), pos, h

    @staticmethod
    def _within(a, b, clearance=10.0):
        """[B, K, K]: vehicle j of a closer than `clearance` to vehicle k of b"""
        d = a[:, :, None, :] - b[:, None, :, :]
        return (d * d).sum(dim=-1) < clearance * clearance

    def _traffic_step(self, x, y, th, v):
        """The other vehicles' part of a step: IDM behind the nearest counted candidate in the corridor (the ego at x, y, th,
        v and the others, all as they were before the step), motion along the route, respawn under the spawn rule."""
        dt, K = self.dt, self.K
        act, hj, vj = self.oactive, self.ohead, self.ospeed
        cx = torch.cat([x[:, None], self.opos[..., 0]], dim=1)              # candidates [B, K + 1]: the ego, then the others
        cy = torch.cat([y[:, None], self.opos[..., 1]], dim=1)
        ch = torch.cat([th[:, None], hj], dim=1)
        cv = torch.cat([v[:, None], vj], dim=1)
        cact = torch.cat([torch.ones_like(act[:, :1]), act], dim=1)
        cj, sj = torch.cos(hj)[..., None], torch.sin(hj)[..., None]
        ex, ey = cx[:, None, :] - self.opos[..., 0, None], cy[:, None, :] - self.opos[..., 1, None]
        ell = ex * cj + ey * sj                                            # [B, K, K + 1] in vehicle j's body frame
        w = ey * cj - ex * sj
        inside = (ell > 0.0) & (ell <= 40.0) & (w.abs() <= 2.0)
        ic = torch.arange(-1, K, device=self.device)[None, None, :]
        ij = torch.arange(K, device=self.device)[None, :, None]
        dh = ch[:, None, :] - hj[..., None]
        dh = torch.where(dh > math.pi, dh - 2 * math.pi, dh)
        dh = torch.where(dh <= -math.pi, dh + 2 * math.pi, dh)
        # the ego always; another vehicle a full length ahead that drives j's way, or crosses and has the lower index
        counts = (ic < 0) | ((ell > 5.0) & ((ic < ij) | (dh.abs() < math.pi / 4)))
        valid = inside & counts & cact[:, None, :] & (ic != ij)
        best, arg = torch.where(valid, ell, torch.full_like(ell, float("inf"))).min(dim=2)
        has = torch.isfinite(best) & act
        # a circle of vehicles waiting for each other (merging at a small angle, or following mixed with yielding): walk the
        # map j -> leader(j) K steps; the lowest index of a circle drives free this step (env::walk_leaders)
        who = torch.where(has, arg - 1, torch.full_like(arg, -2))
        wp, lowest = who.clone(), ij[:, :, 0].expand_as(who).clone()
        closed = torch.zeros_like(has)
        for _ in range(K):
            go = (wp >= 0) & ~closed
            closed = closed | (go & (wp == ij[:, :, 0]))
            go = go & ~closed
            lowest = torch.where(go, torch.minimum(lowest, wp), lowest)
            wp = torch.where(go, torch.gather(who, 1, wp.clamp(min=0)), wp)
        has = has & ~(closed & (lowest == ij[:, :, 0]))
        lh, lv = torch.gather(ch, 1, arg), torch.gather(cv, 1, arg)
        gap = torch.clamp(torch.where(has, best, torch.ones_like(best)) - 5.0, min=0.1)
        dv = vj - lv * torch.cos(lh - hj)
        q = (5.0 + torch.clamp(vj * 1.5 + vj * dv / 7.745966692414834, min=0.0)) / gap
        r2 = (vj / self.otarget) ** 2
        acc = torch.clamp(3.0 * (1.0 - r2 * r2 - torch.where(has, q * q, torch.zeros_like(q))), -6.0, 3.0)
        self.oprog.copy_(torch.where(act, self.oprog + vj * dt, self.oprog))
        self.ospeed.copy_(torch.where(act, torch.clamp(vj + acc * dt, 0.0, 30.0), vj))
        pos, h = self.pose(self.oroute, self.oprog)
        self.opos.copy_(torch.where(act[..., None], pos, self.opos))
        self.ohead.copy_(torch.where(act, h, self.ohead))
        stays = act & ~(self.opos.abs().amax(dim=-1) > 65.0)
        drew = ~stays & (torch.rand(stays.shape, generator=self.gen, device=self.device) < self.spawn_probability)
        route, s, sp, v0, pos, h = self._draw_vehicles(stays.shape, 40.0, 60.0)
        # not placed within 10 m of a lower-index vehicle that stays or was drawn, or of a higher-index one that stays
        other = torch.where(stays[..., None], self.opos, pos)
        lower = ij[0] > torch.arange(K, device=self.device)[None, :]       # [K(j), K(k)]: k < j
        diff = ~torch.eye(K, dtype=torch.bool, device=self.device)
        blocks = self._within(pos, other) & diff[None] & (stays[:, None, :] | (lower[None] & drew[:, None, :]))
        placed = drew & ~blocks.any(dim=2)
        self.opos.copy_(torch.where(placed[..., None], pos, self.opos))
        self.ospeed.copy_(torch.where(placed, sp, self.ospeed))
        self.ohead.copy_(torch.where(placed, h, self.ohead))
        self.oroute.copy_(torch.where(placed, route, self.oroute))
        self.oprog.copy_(torch.where(placed, s, self.oprog))
        self.otarget.copy_(torch.where(placed, v0, self.otarget))
        self.oactive.copy_(stays | placed)

    def _reset_where(self, mask):
        B, K = self.num_envs, max(self.K, 1)
        ego = torch.zeros((B, 4), dtype=torch.float64, device=self.device)
        ego[:, 0] = 2.0
        ego[:, 1] = 45.0 + self._u((B,), -5.0, 5.0)          # envs/intersection_env_Feb2025_v1.py:397-410
        ego[:, 2] = -math.pi / 2
        ego[:, 3] = 10.0
        if self.traffic == "idm":
            route, s, sp, v0, pos, h = self._draw_vehicles((B, K), 5.0, 60.0)
            lower = torch.arange(K, device=self.device)[:, None] > torch.arange(K, device=self.device)[None, :]
            placed = ~(self._within(pos, pos) & lower[None]).any(dim=2)    # clear of every lower-index vehicle drawn
            if self.K == 0:
                placed = torch.zeros_like(placed)
            m1 = mask[:, None]
            self.ego.copy_(torch.where(m1, ego, self.ego))
            self.opos.copy_(torch.where(mask[:, None, None], pos, self.opos))
            for dst, src in ((self.ospeed, sp), (self.ohead, h), (self.oactive, placed), (self.oroute, route),
                             (self.oprog, s), (self.otarget, v0)):
                dst.copy_(torch.where(m1, src, dst))
            self.t.copy_(torch.where(mask, torch.zeros_like(self.t), self.t))
            return
        pos, sp, h = self._spawn_others((B, K), 5.0, 60.0)
        m1, m2 = mask[:, None], mask[:, None, None]
        # state tensors are updated in place: a captured hipGraph (BatchedCollector(use_graph=True)) replays against
        # fixed addresses
        self.ego.copy_(torch.where(m1, ego, self.ego))
        self.opos.copy_(torch.where(m2, pos, self.opos))
        self.ospeed.copy_(torch.where(m1, sp, self.ospeed))
        self.ohead.copy_(torch.where(m1, h, self.ohead))
        active = torch.ones((B, K), dtype=torch.bool, device=self.device) if self.K > 0 else \
            torch.zeros((B, K), dtype=torch.bool, device=self.device)
        self.oactive.copy_(torch.where(m1, active, self.oactive))
        self.t.copy_(torch.where(mask, torch.zeros_like(self.t), self.t))

    # ---- observation (config/config.py:10-26) ------------------------------------------------------------------
    def observe(self) -> torch.Tensor:
        """(torch implementation; also the independent check of the fused kernel's observation)"""
        B, K = self.num_envs, max(self.K, 1)
        obs = torch.zeros((B, VEHICLES_COUNT, 8), dtype=torch.float32, device=self.device)
        x, y, th, v = self.ego.unbind(dim=1)
        obs[:, 0, 0] = 1.0
        obs[:, 0, 1], obs[:, 0, 2] = x.float(), y.float()
        obs[:, 0, 3], obs[:, 0, 4] = (v * torch.cos(th)).float(), (v * torch.sin(th)).float()
        obs[:, 0, 5], obs[:, 0, 6], obs[:, 0, 7] = th.float(), torch.sin(th).float(), torch.cos(th).float()
        if self.K > 0:
            d = torch.linalg.norm(self.opos - self.ego[:, None, :2], dim=-1)
            d = torch.where(self.oactive, d, torch.full_like(d, float("inf")))
            order = torch.argsort(d, dim=1, stable=True)                  # `order: sorted`: nearest first, absent last
            g = lambda t: torch.gather(t, 1, order)
            act = g(self.oactive)
            px = torch.gather(self.opos[..., 0], 1, order)
            py = torch.gather(self.opos[..., 1], 1, order)
            sp, hh = g(self.ospeed), g(self.ohead)
            rows = torch.stack([torch.ones_like(px), px, py, sp * torch.cos(hh), sp * torch.sin(hh), hh, torch.sin(hh),
                                torch.cos(hh)], dim=-1)
            rows = torch.where(act[..., None], rows, torch.zeros_like(rows))
            obs[:, 1:1 + K] = rows.float()
        return obs

    def reset(self) -> torch.Tensor:
        if self.backend == "hip":
            self._hip_call(None, True)
            return self._out["obs"]
        self._reset_where(torch.ones(self.num_envs, dtype=torch.bool, device=self.device))
        return self.observe()

    # ---- one policy step ---------------------------------------------------------------------------------------
    def step(self, action: torch.Tensor):
        """action[B, 2] = acceleration [m/s^2], steering angle [rad] (what the RL wrappers hand to env.step,
        agents/ppo_mpc.py:430-432).  Returns obs, reward, done, info like an SB3 VecEnv with auto-reset:
        info = dict(terminal_obs, truncated, crashed, arrived)."""
        if self.backend == "hip":
            if action.dtype != torch.float64 or not action.is_contiguous():
                action = action.to(torch.float64).contiguous()
            self._hip_call(action, False)
            o = self._out
            b = lambda k: o[k].view(torch.bool)
            return o["obs"], o["reward"], b("done"), dict(terminal_obs=o["terminal_obs"], truncated=b("truncated"),
                                                          crashed=b("crashed"), arrived=b("arrived"))
        a = torch.clamp(action[:, 0].to(torch.float64), -5.0, 5.0)                      # config/config.py:31
        delta = torch.clamp(action[:, 1].to(torch.float64), -math.pi / 4, math.pi / 4)  # config/config.py:30
        x, y, th, v = self.ego.unbind(dim=1)
        beta = torch.atan(0.5 * torch.tan(delta))
        dt = self.dt
        nx = x + v * torch.cos(th + beta) * dt
        ny = y + v * torch.sin(th + beta) * dt
        nth = th + v / WHEELBASE * torch.sin(beta) * dt
        nv = torch.clamp(v + a * dt, 0.0, 30.0)
        if self.traffic == "idm":           # the traffic reacts to the ego as it was before the step (x .. v are views)
            x, y, th, v = x.clone(), y.clone(), th.clone(), v.clone()
        self.ego.copy_(torch.stack([nx, ny, nth, nv], dim=1))
        if self.K > 0 and self.traffic == "idm":
            self._traffic_step(x, y, th, v)
            dist = torch.linalg.norm(self.opos - self.ego[:, None, :2], dim=-1)
            crashed = ((dist < CRASH_DISTANCE) & self.oactive).any(dim=1)
        elif self.K > 0:
            step = (self.ospeed * dt)[..., None] * torch.stack([torch.cos(self.ohead), torch.sin(self.ohead)], dim=-1)
            self.opos.add_(step)
            gone = (self.opos.abs().amax(dim=-1) > 65.0) | ~self.oactive
            respawn = gone & (torch.rand(gone.shape, generator=self.gen, device=self.device) < self.spawn_probability)
            pos, sp, h = self._spawn_others(gone.shape, 40.0, 60.0)
            self.opos.copy_(torch.where(respawn[..., None], pos, self.opos))
            self.ospeed.copy_(torch.where(respawn, sp, self.ospeed))
            self.ohead.copy_(torch.where(respawn, h, self.ohead))
            self.oactive.copy_((self.oactive & ~gone) | respawn)
            dist = torch.linalg.norm(self.opos - self.ego[:, None, :2], dim=-1)
            crashed = ((dist < CRASH_DISTANCE) & self.oactive).any(dim=1)
        else:
            crashed = torch.zeros(self.num_envs, dtype=torch.bool, device=self.device)
        dref = torch.linalg.norm(self.ref_xy[None] - self.ego[:, None, :2], dim=-1)
        lateral, idx = dref.min(dim=1)
        on_road = lateral <= LANE_HALF_WIDTH
        arrived = (idx >= self.M - 3) & on_road
        centering = 1.0 - torch.clamp(lateral / LANE_HALF_WIDTH, max=1.0)
        reward = (REWARD["collision"] * crashed + REWARD["high_speed"] * (self.ego[:, 3] / 10.0) +
                  REWARD["arrived"] * arrived + torch.where(on_road, REWARD["center_bonus"] * centering,
                                                            torch.full_like(centering, REWARD["off_road"])))
        self.t.add_(1)
        terminated = crashed | arrived
        truncated = (self.t >= EPISODE_STEPS) & ~terminated
        done = terminated | truncated
        terminal_obs = self.observe()
        self._reset_where(done)
        obs = torch.where(done[:, None, None], self.observe(), terminal_obs)
        return obs, reward.float(), done, dict(terminal_obs=terminal_obs, truncated=truncated, crashed=crashed,
                                               arrived=arrived)


SDE_EPSILON = 1e-6          # StateDependentNoiseDistribution(epsilon=1e-6): the floor of the gSDE variance


class ActorCritic(torch.nn.Module):
    """SB3 `MlpPolicy`-shaped actor-critic: 80 -> 64 -> 64 (tanh) twice, Gaussian head of `action_dim`.

    use_sde=False (default): SB3's DiagGaussianDistribution, a state-independent `log_std` [A].
    use_sde=True: generalized State-Dependent Exploration, SB3 2.4's StateDependentNoiseDistribution at the settings
    ActorCriticPolicy uses (full_std, no expln, no squashing, learn_features=False, epsilon 1e-6) - what the reference's
    PPO agents train with (agents/ppo_mpc.py:114-115).  `log_std` is [H, A]; with latent = pi(obs) and latent_d its detached
    copy, the distribution is Normal(action_net(latent), sqrt(latent_d^2 @ exp(log_std)^2 + 1e-6)) and a sample is
    mean + latent_d @ E[b] with one exploration matrix E[b] = exp(log_std) * Z[b] per environment, Z ~ N(0, 1) [n, H, A]
    redrawn by reset_noise(n)."""

    def __init__(self, action_dim: int, obs_dim: int = VEHICLES_COUNT * 8, hidden: int = 64, use_sde: bool = False,
                 log_std_init: float = 0.0):
        super().__init__()
        mk = lambda: torch.nn.Sequential(torch.nn.Linear(obs_dim, hidden), torch.nn.Tanh(),
                                         torch.nn.Linear(hidden, hidden), torch.nn.Tanh())
        self.pi, self.vf = mk(), mk()
        self.action_net = torch.nn.Linear(hidden, action_dim)
        self.value_net = torch.nn.Linear(hidden, 1)
        self.use_sde = bool(use_sde)
        shape = (hidden, action_dim) if self.use_sde else (action_dim,)
        self.log_std = torch.nn.Parameter(torch.full(shape, float(log_std_init)))
        self.action_dim = action_dim
        if self.use_sde:
            # the matrices move with the module (.to) but are not parameters: buffers outside the state dict
            self.register_buffer("sde_noise", torch.zeros((1,) + shape), persistent=False)
            self.register_buffer("sde_noise_single", torch.zeros(shape), persistent=False)
            self.reset_noise(1)

    # ---- gSDE exploration matrices (StateDependentNoiseDistribution.sample_weights / get_noise) ----------------------------
    @torch.no_grad()
    def reset_noise(self, n: int = 1, generator=None):
        """Redraw the standard-normal Z of the exploration matrices: `sde_noise` [n, H, A] (one per environment) and
        `sde_noise_single` [H, A], the one matrix SB3 uses when the batch is a single observation or does not match n."""
        if not self.use_sde:
            raise RuntimeError("reset_noise: the policy was built without use_sde")
        dev, dt = self.log_std.device, self.log_std.dtype
        self.sde_noise_single = torch.randn(tuple(self.log_std.shape), generator=generator, device=dev, dtype=dt)
        self.sde_noise = torch.randn((int(n),) + tuple(self.log_std.shape), generator=generator, device=dev, dtype=dt)

    def _sde_sample_noise(self, latent_d, std, Z=None):
        """latent_d [B, H] @ E with E = std * Z: per environment (bmm) when Z has one matrix per row of the batch, else the
        single matrix (get_noise's default case)."""
        if Z is None:
            many = self.sde_noise
            Z = many if latent_d.shape[0] != 1 and many.shape[0] == latent_d.shape[0] else self.sde_noise_single
        if Z.dim() == 2:
            return latent_d @ (std * Z)
        return torch.bmm(latent_d[:, None], std * Z)[:, 0]

    def _dist(self, obs):
        latent = self.pi(obs.flatten(1))
        mean = self.action_net(latent)
        if self.use_sde:
            latent_d = latent.detach()
            variance = (latent_d ** 2) @ (self.log_std.exp() ** 2)
            return torch.distributions.Normal(mean, torch.sqrt(variance + SDE_EPSILON), validate_args=False), latent_d
        # validate_args=False: the default argument checks read a device boolean back on the host (a sync per step)
        return torch.distributions.Normal(mean, self.log_std.exp().expand_as(mean), validate_args=False), None

    def forward(self, obs, deterministic: bool = False, generator=None):
        d, latent_d = self._dist(obs)
        if deterministic:
            actions = d.mean
        elif self.use_sde:
            actions = d.mean + self._sde_sample_noise(latent_d, self.log_std.exp())
        else:
            actions = d.mean + d.stddev * torch.randn(d.mean.shape, generator=generator, device=d.mean.device,
                                                      dtype=d.mean.dtype)
        return actions, self.predict_values(obs), d.log_prob(actions).sum(dim=1)

    def predict_values(self, obs):
        return self.value_net(self.vf(obs.flatten(1)))[:, 0]

    # ---- rollout-time forward (no gradients): both towers as ONE 80 -> 128 -> 128 -> (action_dim + 1) network (first
    #      layers side by side, second layer block-diagonal, heads in one matrix) and the Gaussian sample / log-probability
    #      written out - 3 GEMMs, 2 tanh and 6 small kernels instead of 6 + 4 + 12.  Same function as forward(); the fused
    #      weights live in persistent buffers (a captured hipGraph reads them in place) refreshed by refresh_fused().
    #      gSDE: std = exp(log_std) [H, A] and no c0.
    @torch.no_grad()
    def refresh_fused(self):
        A, H = self.action_dim, self.pi[0].out_features
        dev, dt = self.log_std.device, self.log_std.dtype
        if getattr(self, "_fz", None) is None or self._fz["w1"].device != dev:
            z = lambda *shape: torch.zeros(shape, device=dev, dtype=dt)
            self._fz = dict(w1=z(self.pi[0].in_features, 2 * H), b1=z(2 * H), w2=z(2 * H, 2 * H), b2=z(2 * H),
                            wh=z(2 * H, A + 1), bh=z(A + 1))
            if self.use_sde:
                self._fz["std"] = z(H, A)
            else:
                self._fz.update(std=z(A), c0=z(1)[0])
        f = self._fz
        f["w1"][:, :H].copy_(self.pi[0].weight.t())
        f["w1"][:, H:].copy_(self.vf[0].weight.t())
        f["b1"][:H].copy_(self.pi[0].bias)
        f["b1"][H:].copy_(self.vf[0].bias)
        f["w2"][:H, :H].copy_(self.pi[2].weight.t())
        f["w2"][H:, H:].copy_(self.vf[2].weight.t())
        f["b2"][:H].copy_(self.pi[2].bias)
        f["b2"][H:].copy_(self.vf[2].bias)
        f["wh"][:H, :A].copy_(self.action_net.weight.t())
        f["wh"][H:, A].copy_(self.value_net.weight[0])
        f["bh"][:A].copy_(self.action_net.bias)
        f["bh"][A:].copy_(self.value_net.bias)
        f["std"].copy_(self.log_std.exp())
        if not self.use_sde:
            f["c0"].copy_(self.log_std.sum() + 0.5 * A * math.log(2.0 * math.pi))

    @torch.no_grad()
    def act(self, obs, generator=None, noise=None):
        """(actions, values, log_probs) like forward(obs), through the fused weights (call refresh_fused() after every
        change of the parameters).  noise: the sample's standard-normal draws [B, action_dim] instead of the generator's;
        with use_sde the exploration matrices' Z instead of the policy's own ([B, H, A] per environment or [H, A])."""
        f, A = self._fz, self.action_dim
        h = torch.tanh(torch.addmm(f["b1"], obs.flatten(1), f["w1"]))
        h = torch.tanh(torch.addmm(f["b2"], h, f["w2"]))
        out = torch.addmm(f["bh"], h, f["wh"])
        mean = out[:, :A]
        if self.use_sde:
            std = f["std"]
            latent = h[:, :std.shape[0]]
            actions = mean + self._sde_sample_noise(latent, std, noise)
            scale = torch.sqrt((latent ** 2) @ (std ** 2) + SDE_EPSILON)
            log_probs = (-((actions - mean) ** 2) / (2 * scale ** 2) - scale.log() - math.log(math.sqrt(2 * math.pi))).sum(dim=1)
            return actions, out[:, A], log_probs
        if noise is None:
            noise = torch.randn(mean.shape, generator=generator, device=mean.device, dtype=mean.dtype)
        actions = torch.addcmul(mean, noise, f["std"])
        log_probs = (noise * noise).sum(dim=1).mul_(-0.5).sub_(f["c0"])
        return actions, out[:, A], log_probs

    def evaluate_actions(self, obs, actions):
        d, _ = self._dist(obs)
        return self.predict_values(obs), d.log_prob(actions).sum(dim=1), d.entropy().sum(dim=1)

    # ---- stable-baselines3 checkpoints ----------------------------------------------------------------------------------
    _SB3_KEYS = {"mlp_extractor.policy_net.0.weight": "pi.0.weight", "mlp_extractor.policy_net.0.bias": "pi.0.bias",
                 "mlp_extractor.policy_net.2.weight": "pi.2.weight", "mlp_extractor.policy_net.2.bias": "pi.2.bias",
                 "mlp_extractor.value_net.0.weight": "vf.0.weight", "mlp_extractor.value_net.0.bias": "vf.0.bias",
                 "mlp_extractor.value_net.2.weight": "vf.2.weight", "mlp_extractor.value_net.2.bias": "vf.2.bias",
                 "action_net.weight": "action_net.weight", "action_net.bias": "action_net.bias",
                 "value_net.weight": "value_net.weight", "value_net.bias": "value_net.bias", "log_std": "log_std"}

    @classmethod
    def load_sb3(cls, path, device="cpu"):
        """An SB3 `.zip` (BaseAlgorithm.save: `data` JSON + `policy.pth` state dict) of the reference's MlpPolicy agents ->
        (ActorCritic, meta).  `policy.pth` goes through torch.load(weights_only=True); `data` is read as JSON and none of
        its `:serialized:` (pickled) fields is ever unpickled.  meta = dict(version, use_sde, sde_sample_freq, action_dim,
        algorithm) - algorithm "ppo" / "a2c" from the fields PPO alone saves, None when undecidable.
        Like SB3's load, one exploration matrix is drawn for a gSDE policy (reset_noise(1))."""
        import io
        import json
        import zipfile
        try:
            with zipfile.ZipFile(path) as z:
                names = set(z.namelist())
                if "policy.pth" not in names or "data" not in names:
                    raise ValueError(f"{path}: not an SB3 checkpoint (needs `data` and `policy.pth`, has {sorted(names)})")
                data = json.loads(z.read("data").decode("utf-8"))
                sd = torch.load(io.BytesIO(z.read("policy.pth")), map_location="cpu", weights_only=True)
        except zipfile.BadZipFile as e:
            raise ValueError(f"{path}: not a zip archive") from e
        missing = [k for k in cls._SB3_KEYS if k not in sd]
        extra = [k for k in sd if k not in cls._SB3_KEYS]
        if missing or extra:
            raise ValueError(f"{path}: not an 80 -> H -> H MlpPolicy state dict (missing {missing}, unexpected {extra})")
        use_sde = bool(data.get("use_sde", False))
        A, H = int(sd["action_net.weight"].shape[0]), int(sd["mlp_extractor.policy_net.0.weight"].shape[0])
        obs_dim = int(sd["mlp_extractor.policy_net.0.weight"].shape[1])
        want_log_std = (H, A) if use_sde else (A,)
        if tuple(sd["log_std"].shape) != want_log_std:
            raise ValueError(f"{path}: use_sde={use_sde} needs log_std of shape {want_log_std}, "
                             f"the checkpoint has {tuple(sd['log_std'].shape)}")
        pol = cls(A, obs_dim=obs_dim, hidden=H, use_sde=use_sde)
        own = pol.state_dict()
        for k, name in cls._SB3_KEYS.items():
            if tuple(sd[k].shape) != tuple(own[name].shape):
                raise ValueError(f"{path}: {k} has shape {tuple(sd[k].shape)}, expected {tuple(own[name].shape)}")
        pol.load_state_dict({name: sd[k].to(torch.float32) for k, name in cls._SB3_KEYS.items()})
        pol = pol.to(device)
        if use_sde:
            pol.reset_noise(1)
        version = data.get("version")
        # PPO saves its clip range and epoch count; A2C (the other on-policy algorithm with n_steps / gae_lambda) neither
        algorithm = "ppo" if "clip_range" in data else ("a2c" if "gae_lambda" in data and "n_epochs" not in data else None)
        meta = dict(version=version if version in ("v0", "v1") else None, use_sde=use_sde,
                    sde_sample_freq=int(data.get("sde_sample_freq", -1)), action_dim=A, algorithm=algorithm)
        return pol, meta

    def save_sb3(self, path, version=None, algorithm="ppo", **extra):
        """The inverse of load_sb3: a zip with `policy.pth` (the state dict under stable-baselines3's names, _SB3_KEYS, on the
        CPU) and a `data` JSON with use_sde, sde_sample_freq (-1 unless given), version and the fields load_sb3 tells the
        algorithm by: "ppo" writes clip_range, n_epochs and gae_lambda, "a2c" gae_lambda alone, None neither.  `extra`
        adds or overrides JSON fields (n_steps, sde_sample_freq, ...; JSON-serialisable values only).  It stores a trained
        policy of this package for a later load_sb3 / from_sb3 - the reference's save / load.  Loading the file with
        stable-baselines3 itself is NOT verified here (stable-baselines3 is not available to this project's tests): SB3's own
        `data` holds more fields, several of them pickled, than this file carries."""
        import io
        import json
        import zipfile
        if algorithm not in ("ppo", "a2c", None):
            raise ValueError("algorithm must be ppo, a2c or None")
        data = dict(use_sde=self.use_sde, sde_sample_freq=-1, version=version)
        if algorithm == "ppo":
            data.update(clip_range=0.2, n_epochs=10, gae_lambda=0.95)
        elif algorithm == "a2c":
            data.update(gae_lambda=1.0)
        data.update(extra)
        own = self.state_dict()
        sd = {k: own[name].detach().to("cpu").contiguous().clone() for k, name in self._SB3_KEYS.items()}
        blob = io.BytesIO()
        torch.save(sd, blob)
        with zipfile.ZipFile(path, "w") as z:
            z.writestr("data", json.dumps(data))
            z.writestr("policy.pth", blob.getvalue())


CONTROL_SCALE = (5.0, math.pi / 4)     # acceleration_range / steering_range upper bounds (config/config.py:27-32)


def control_scale(device):
    return torch.tensor(CONTROL_SCALE, dtype=torch.float64, device=device)


def map_control(actions, out=None, scale=None):
    """The end-to-end baseline's action [B, 2] -> physical controls [B, 2] float64 (acceleration m/s^2, steering rad) as
    highway-env's ContinuousAction maps it: clip to [-1, 1], then scale onto the symmetric acceleration / steering ranges.
    The torch form of csrc/mpc_rollout_glue.hpp::map_control, same bits.  `out`: written in place (fixed address); `scale`:
    control_scale(device) made beforehand (inside a captured graph nothing may be copied from the host)."""
    c = torch.clamp(actions, -1.0, 1.0).to(torch.float64)
    return torch.mul(c, control_scale(actions.device) if scale is None else scale, out=out)


def _check_direct_policy(policy):
    if int(getattr(policy, "action_dim", 0)) != 2:
        raise ValueError("the end-to-end baseline needs a policy with action_dim 2 (acceleration, steering)")
    if getattr(policy, "use_sde", False):
        raise ValueError("the end-to-end baseline is a Gaussian policy: gSDE (use_sde=True) is not supported "
                         "(the reference's agents/ppo_agent.py leaves SB3's default, off)")


def mpc_inputs(actions, version, default_weights, clip=False):
    """RL action -> (weights[B,3] float64, ref_speed[B] float64 or None) as the reference maps them: "v0" action 0 is the
    reference speed beside default_weights [B, 3], "v1" actions 0..2 are the weights.  clip: to the Box(-1, 1) bounds first
    (PPO's collector, agents/ppo_mpc.py:399-407)."""
    if clip:
        actions = torch.clamp(actions, -1.0, 1.0)
    if version == "v0":
        return default_weights, actions[:, 0].to(torch.float64).contiguous()
    return actions[:, :3].to(torch.float64).contiguous(), None


def fits_fused_policy(policy, engine):
    """Whether the fused policy kernels (FusedPolicy) can run `policy`: SB3's MlpPolicy shape with 80 inputs, both towers side
    by side in 256 columns, at most 8 actions, float32, and an engine that carries the library.  Where the tensors live is
    the caller's part: the collector asks for the HIP environment, the agents for an observation on a GPU."""
    return (isinstance(policy, ActorCritic) and hasattr(engine, "_lib") and policy.pi[0].in_features == VEHICLES_COUNT * 8 and
            2 * policy.pi[0].out_features <= 256 and policy.action_dim <= 8 and policy.log_std.dtype == torch.float32)


class FusedPolicy:
    """The policy step as ONE launch (csrc/mpc_rollout_glue.hpp): forward of both towers, sample, log-probability and what
    the step's next stage reads - mode "v0" / "v1": the MPC's inputs (mpc_policy_act, or mpc_policy_act_sde for a gSDE
    policy), mode "direct": the controls (mpc_policy_control).  `tensors` are the launch's fixed-address buffers:
      act, val, logp   the action [B, A], the value and the log-probability [B]
      w, rs            "v1" the MPC's weights [B, 3] f64, "v0" its reference speed [B] f64
      ctrl             "direct": the controls [B, 2] f64
      noise            Gaussian: the sample's draws [B, A], written by the kernel when it draws and read by it when not;
                       gSDE: None (the kernel draws the matrices and keeps none), deterministic the zero matrices [B, H, A]
      step             int64 [1], the policy steps taken so far, which key the Gaussian draws with (seed, env_offset + b); the
                       caller's accounting advances it (mpc_rollout_record, mpc_episode_stats).  None when deterministic.
      sde_epoch        gSDE, int64 [1]: the epoch that keys the matrices with (seed, env_offset + b); with sde_sample_freq > 0
                       the kernel adds sde_step // sde_sample_freq, `sde_step` an int64 [1] device counter of the caller's.
                       None when deterministic.
    clip: the MPC's inputs from the action clipped to [-1, 1] (PPO's collector)."""

    def __init__(self, policy, B, device, lib, mode, clip=False, seed=0, env_offset=0, deterministic=False,
                 sde_sample_freq=-1, sde_step=None):
        A, H, sde = policy.action_dim, policy.pi[0].out_features, bool(policy.use_sde)
        z = lambda *sh, dt=torch.float32: torch.zeros(sh, dtype=dt, device=device)
        self.policy, self.device, self.mode = policy, device, mode
        t = self.tensors = dict(act=z(B, A), val=z(B), logp=z(B), w=z(B, 3, dt=torch.float64), rs=z(B, dt=torch.float64),
                                noise=(z(B, H, A) if deterministic else None) if sde else z(B, A),
                                ctrl=z(B, 2, dt=torch.float64) if mode == "direct" else None,
                                step=None if deterministic else z(1, dt=torch.int64),
                                sde_epoch=z(1, dt=torch.int64) if sde and not deterministic else None)
        # what every launch passes unchanged (the buffers above are never rebound); launch adds the observation, the
        # policy's weights as they are then, and the stream
        self._fixed = dict(lib=lib, device=device.index, B=int(B), noise_seed=int(seed) & 0xFFFFFFFFFFFFFFFF,
                           env_offset=int(env_offset), actions=t["act"], values=t["val"], log_probs=t["logp"])
        if sde:
            self._fixed.update(sde_noise=t["noise"], sde_epoch=t["sde_epoch"], sde_step=sde_step,
                               sde_sample_freq=int(sde_sample_freq))
        else:
            self._fixed.update(noise=t["noise"], noise_step=t["step"])
        if mode == "direct":
            entry = "mpc_policy_control"
            self._fixed.update(control=t["ctrl"])
        else:
            v1 = mode == "v1"
            entry = "mpc_policy_act_sde" if sde else "mpc_policy_act"
            self._fixed.update(A=A, version_v1=1 if v1 else 0, clip=1 if clip else 0, mpc_weights=t["w"] if v1 else None,
                               mpc_ref_speed=None if v1 else t["rs"])
        self._entry = _engine.caller(entry)

    def launch(self, obs):
        f = self.policy._fz
        std = dict(sde_std=f["std"]) if self.policy.use_sde else dict(std_=f["std"], c0=f["c0"])
        self._entry(obs=obs, H2=f["b1"].numel(), w1=f["w1"], b1=f["b1"], w2=f["w2"], b2=f["b2"], wh=f["wh"],
                    bh=f["bh"], **std, stream=_engine.current_stream(self.device), **self._fixed)


class RolloutBuffer:
    """[n_steps, B, ...] device tensors + GAE (the arithmetic of SB3's RolloutBuffer, which the reference uses as is).

    The float32 fields of a step (observation, action, reward, episode start, value, log-probability and - for PPO - the
    terminal observation and the truncation flag) are columns of ONE [n_steps, B, F] tensor, so that a step writes its row
    with one concatenation and one copy instead of eight; `obs`, `actions`, ... are views of it."""

    def __init__(self, n_steps, num_envs, action_dim, device, gamma=0.99, gae_lambda=0.95, keep_terminal=False):
        T, B, A, O = int(n_steps), int(num_envs), int(action_dim), VEHICLES_COUNT * 8
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=device)
        self._cols = O + A + 4 + ((O + 1) if keep_terminal else 0)
        self._row = z(T, B, self._cols)
        r, c = self._row, O + A
        self.obs = r[..., :O].view(T, B, VEHICLES_COUNT, 8)
        self.actions = r[..., O:c]
        self.rewards, self.episode_starts, self.values, self.log_probs = r[..., c], r[..., c + 1], r[..., c + 2], r[..., c + 3]
        # PPO bootstraps truncated episodes with the value of their terminal observation (agents/ppo_mpc.py:451-461): the
        # observations and flags are kept per step and the values are computed for the whole rollout at once at its end
        # (bootstrap_truncated) - the policy does not change during a rollout - instead of one value tower per step
        self.terminal_obs = r[..., c + 4:c + 4 + O].view(T, B, VEHICLES_COUNT, 8) if keep_terminal else None
        self.truncated = r[..., c + 4 + O] if keep_terminal else None
        self.advantages, self.returns = z(T, B), z(T, B)
        self.mpc_actions = z(T, B, 2, dt=torch.float64)
        self.gamma, self.gae_lambda, self.n_steps, self.pos = float(gamma), float(gae_lambda), T, 0
        self.pos_dev = torch.zeros(1, dtype=torch.int64, device=device)     # the same counter for captured graphs

    def reset(self):
        self.pos = 0
        self.pos_dev.zero_()

    def _pack(self, obs, actions, rewards, episode_starts, values, log_probs, terminal_obs, truncated):
        f = lambda t: t.reshape(t.shape[0], -1)
        cols = [f(obs), f(actions), f(rewards), f(episode_starts), f(values), f(log_probs)]
        if self.terminal_obs is not None:
            cols += [f(terminal_obs), f(truncated)]
        row = torch.cat(cols, dim=1)
        assert row.shape[1] == self._cols
        return row

    def add(self, obs, actions, rewards, episode_starts, values, log_probs, mpc_actions=None, terminal_obs=None,
            truncated=None):
        i = self.pos
        self._row[i] = self._pack(obs, actions, rewards, episode_starts, values, log_probs, terminal_obs, truncated)
        if mpc_actions is not None:
            self.mpc_actions[i] = mpc_actions
        self.pos += 1
        self.pos_dev.add_(1)

    def add_at_device_pos(self, obs, actions, rewards, episode_starts, values, log_probs, mpc_actions, terminal_obs=None,
                          truncated=None):
        """`add` with the row taken from the device-side counter: no host value is baked into a captured graph."""
        i = self.pos_dev
        row = self._pack(obs, actions, rewards, episode_starts, values, log_probs, terminal_obs, truncated)
        self._row.index_copy_(0, i, row.unsqueeze(0))
        self.mpc_actions.index_copy_(0, i, mpc_actions.to(self.mpc_actions.dtype).unsqueeze(0))
        self.pos_dev.add_(1)

    @torch.no_grad()
    def bootstrap_truncated(self, value_fn):
        """rewards += gamma * V(terminal observation) where the episode was truncated, for the whole rollout in one
        evaluation of the value tower"""
        if self.terminal_obs is None:
            return
        T, B = self.rewards.shape
        tv = value_fn(self.terminal_obs.reshape((T * B,) + self.terminal_obs.shape[2:])).reshape(T, B)
        self.rewards += self.gamma * tv * self.truncated

    def compute_returns_and_advantage(self, last_values, dones):
        last_gae = torch.zeros_like(last_values)
        dones = dones.to(last_values.dtype)
        for step in reversed(range(self.n_steps)):
            if step == self.n_steps - 1:
                next_non_terminal, next_values = 1.0 - dones, last_values
            else:
                next_non_terminal, next_values = 1.0 - self.episode_starts[step + 1], self.values[step + 1]
            delta = self.rewards[step] + self.gamma * next_values * next_non_terminal - self.values[step]
            last_gae = delta + self.gamma * self.gae_lambda * next_non_terminal * last_gae
            self.advantages[step] = last_gae
        self.returns = self.advantages + self.values


class BatchedCollector:
    """`collect_rollouts` of the reference for B environments (see module docstring).

    version "v0": the policy's 1-d action is the reference-speed override (agents/ppo_mpc.py:410-414);
    version "v1": its first three components are the cost weights (agents/ppo_mpc.py:416-420).
    version "direct": the end-to-end baseline (agents/ppo_agent.py) - the policy's two outputs are the controls (map_control:
    clipped to [-1, 1] whatever the algorithm, then 5 m/s^2 and pi / 4 rad per unit) and NO MPC runs: a step is policy ->
    controls -> env.step -> buffer row.  `engine` is only the library handle of the fused step (mpc_policy_control) and may
    be None on the torch path; last_mpc = dict(act, status, iters) with zero status / iters, mpc_unconverged stays 0.  The
    MPC's settings (collision_cost, warm_start, reset_mpc_on_done, gather_actions, throughput), an action_dim other than 2
    and gSDE are refused.
    algorithm "ppo" clips the action to the Box(-1, 1) bounds before use and bootstraps truncated episodes with the
    value of the terminal observation (agents/ppo_mpc.py:399-407, 451-461); "a2c" does neither
    (agents/a2c_mpc.py:138-144).
    reset_mpc_on_done=False mirrors the reference, whose single MPC agent keeps its collision memory across
    episode boundaries; True forgets it (`mpc_reset_env_mask`) when an environment restarts.
    warm_start=True (not in the reference) starts every solve from the environment's previous solution advanced by
    one stage (`MPC_FLAG_WARM_START`).
    use_graph: replay the step as one captured hipGraph (default on a GPU; `False` runs it eagerly, ~100 launches from
    Python per step).
    gSDE (a policy built with use_sde=True, ActorCritic): one exploration matrix per environment, redrawn at every rollout
    start (the reference's reset_noise(env.num_envs), agents/ppo_mpc.py:380-381) and, with sde_sample_freq > 0, every
    sde_sample_freq steps of the rollout (:386-388).  The fused step draws the matrices inside mpc_policy_act_sde from a
    device epoch counter (never stored, replayable in the captured graph); the torch step keeps them in `sde_noise`
    [B, H, A], drawn from the collector's generator.
    """

    def __init__(self, env, policy: ActorCritic, engine, version: str = "v0", algorithm: str = "ppo",
                 n_steps: int = 64, gamma: float = 0.99, gae_lambda: float = 0.95,
                 default_weights=(1.0, 1.0, 1.0), collision_cost: bool = False, reset_mpc_on_done: bool = False,
                 gather_actions: bool = False, seed: int = 0, warm_start: bool = False,
                 use_graph: bool | None = None, throughput: bool = False, fused_glue: bool | None = None,
                 sde_sample_freq: int = -1):
        if version not in ("v0", "v1", "direct") or algorithm not in ("ppo", "a2c"):
            raise ValueError("version must be v0|v1|direct and algorithm ppo|a2c")
        if version == "v1" and policy.action_dim < 3:
            raise ValueError("v1 needs an action of at least 3 components (speed, control, input_diff weights)")
        self.direct = version == "direct"
        if self.direct:
            _check_direct_policy(policy)
            given = dict(collision_cost=collision_cost, warm_start=warm_start, reset_mpc_on_done=reset_mpc_on_done,
                         gather_actions=gather_actions, throughput=throughput)
            bad = [k for k, v in given.items() if v]
            if bad:
                raise ValueError(f"version 'direct' runs no MPC: {', '.join(bad)} cannot be set")
        self.env, self.policy, self.engine = env, policy, engine
        self.version, self.algorithm = version, algorithm
        self.collision_cost, self.reset_mpc_on_done, self.gather_actions = collision_cost, reset_mpc_on_done, gather_actions
        self.warm_start = bool(warm_start)
        self.use_sde = bool(getattr(policy, "use_sde", False))
        self.sde_sample_freq = int(sde_sample_freq)
        # several collectors stepping on their own streams (PipelinedCollector): MPC_FLAG_THROUGHPUT, the build of the solve
        # kernel for four resident waves per SIMD whatever this group's batch size (include/mpc_mi355x.h)
        self._mpc_kw = dict(throughput=True) if throughput else {}
        dev = env.device
        B = env.num_envs
        self.buffer = RolloutBuffer(n_steps, B, policy.action_dim, dev, gamma, gae_lambda, keep_terminal=algorithm == "ppo")
        self.default_weights = torch.tensor(default_weights, dtype=torch.float64, device=dev).repeat(B, 1).contiguous()
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed(int(seed))
        self._last_obs = env.reset().clone()                 # persistent tensors, updated in place (graph replays)
        self._last_episode_starts = torch.ones(B, dtype=torch.float32, device=dev)
        # episode counters of the rollout in one tensor (one reduction + one add per step): finished, crashed, arrived
        # episodes and solves that did not converge
        counts = torch.zeros(5, dtype=torch.int64, device=dev)     # [4]: steps the record kernel refused (past the buffer's end)
        self._roll = dict(counts=counts, ep_done=counts[0], crashed=counts[1], arrived=counts[2], unconverged=counts[3],
                          dones=torch.zeros(B, dtype=torch.bool, device=dev))
        self.policy.refresh_fused()
        self.num_timesteps = 0
        self.last_mpc = None
        self._mpc_out = None
        self.gathered_actions = None
        self.gathered_status = None
        # fused_glue (None = whenever possible: fused HIP environment, SB3-shaped policy, real engine): policy forward + sample
        # + MPC inputs in ONE launch (mpc_policy_act) and buffer row + carry-over + counters in one (mpc_rollout_record)
        # instead of ~40 torch kernels - csrc/mpc_rollout_glue.hpp
        can_fuse = (getattr(env, "backend", "") == "hip" and fits_fused_policy(policy, engine) and
                    (self.direct or hasattr(engine, "predict_batch_torch")))
        if fused_glue and not can_fuse:
            raise ValueError("fused_glue needs the fused HIP environment, an ActorCritic policy (80 inputs, hidden <= 128) and the real engine")
        self.fused_glue = can_fuse if fused_glue is None else bool(fused_glue)
        if self.fused_glue:
            # (the Gaussian sample's draws of the last step stay in _fg["noise"]; mpc_rollout_record advances _fg["step"])
            self._policy_step = FusedPolicy(policy, B, dev, engine._lib, version, clip=algorithm == "ppo", seed=seed,
                                            env_offset=getattr(env, "env_offset", 0), sde_sample_freq=self.sde_sample_freq,
                                            sde_step=self.buffer.pos_dev)
            self._fg = self._policy_step.tensors
            self._ticket = torch.zeros(1, dtype=torch.int32, device=dev)
            if self.use_sde:
                # gSDE: a rollout draws from epochs sde_epoch .. sde_epoch + span - 1 (one per sde_sample_freq steps), and
                # _begin_rollout moves past them
                f = self.sde_sample_freq
                self._sde_span = 1 if f <= 0 else -(-int(n_steps) // f)
        if self.direct:
            # what stands in for the MPC's outputs: the controls (written by the step) and a solve status that is always 0
            zi = lambda: torch.zeros(B, dtype=torch.int32, device=dev)
            self._direct = dict(act=self._fg["ctrl"] if self.fused_glue else torch.zeros((B, 2), dtype=torch.float64, device=dev),
                                status=zi(), iters=zi())
            self._control_scale = control_scale(dev)
        if self.use_sde and not self.fused_glue:
            H = policy.log_std.shape[0]
            self.sde_noise = torch.zeros((B, H, policy.action_dim), dtype=policy.log_std.dtype, device=dev)
        # None = the default path: on a GPU with the real engine a step (policy -> MPC -> environment -> buffer row) is
        # captured once as a hipGraph and replayed; eager on the CPU, with stand-in engines, and when the actions are
        # all-gathered (the collective stays outside the graph)
        if use_graph is None:
            use_graph = dev.type == "cuda" and (self.fused_glue if self.direct else
                                                hasattr(engine, "reserve_envs") and hasattr(engine, "predict_batch_torch"))
        self.use_graph = bool(use_graph)
        self._graph = None
        self.graph_fallback_reason = None
        if self.use_graph:
            if not gather_actions:
                self._capture()
            else:
                # sharded runs (config 5): the RCCL all-gather of actions + status is captured INSIDE the graph, so they keep
                # the one-launch step.  Should this RCCL / torch build refuse to capture a collective, the collector RAISES
                # (graph_fallback_reason says why); only with MPC_ALLOW_EAGER_COLLECTIVE_FALLBACK=1 does it step eagerly
                # instead.  The abort is PER RANK: a rank whose capture fails raises here, before any collective of the
                # rollout is issued, and its process ends; the other ranks block in their first all-gather until the process
                # group's timeout or the launcher (torchrun) tears the job down - the same behaviour as any rank dying.
                try:
                    self._capture()
                except Exception as e:      # noqa: BLE001 - whatever the capture raised is the reason reported
                    torch.cuda.synchronize(dev)
                    self._graph, self.use_graph = None, False
                    self.graph_fallback_reason = f"{type(e).__name__}: {e}"
                    # _capture() has put the collector's state back (its finally clause).  What it cannot vouch for is the
                    # communicator an aborted capture of a collective leaves behind: unless the caller asked for the eager
                    # fallback explicitly, a sharded run ends here instead of issuing collectives on it
                    if os.environ.get("MPC_ALLOW_EAGER_COLLECTIVE_FALLBACK", "0") != "1":
                        raise RuntimeError("hipGraph capture of the sharded rollout step failed (" + self.graph_fallback_reason +
                                           "); set MPC_ALLOW_EAGER_COLLECTIVE_FALLBACK=1 to step eagerly instead") from e

    # ---- one rollout = begin, n steps, finish; split so that the step can be captured in a hipGraph and several
    #      collectors can be interleaved (PipelinedCollector)
    @torch.no_grad()
    def _begin_rollout(self):
        self.policy.eval()
        self.policy.refresh_fused()        # the parameters may have been updated since the last rollout
        self.buffer.reset()
        self._roll["counts"].zero_()
        if self.use_sde:                   # new exploration matrices (agents/ppo_mpc.py:380-381)
            self._sde_resample()

    @torch.no_grad()
    def _sde_resample(self):
        if self.fused_glue:
            self._fg["sde_epoch"].add_(self._sde_span)
        else:
            self.sde_noise.normal_(generator=self.gen)      # in place: a captured graph reads it at this address

    @torch.no_grad()
    def _rollout_step_fused(self):
        """The same step with the glue kernels: identical data flow; the float32 sums of the three small matrix products
        are accumulated in index order instead of hipBLASLt's, and the Gaussian sample's noise is drawn by the kernel
        (counter-based; left in self._fg["noise"]) instead of by torch's generator - fed the same noise, ActorCritic.act
        returns the same actions (tests/test_predict_gpu.py::test_fused_glue_step_equals_the_torch_step).  version "direct":
        the policy launch leaves the controls where the MPC's action would be, and the status is the all-zero one."""
        obs, fg = self._last_obs, self._fg
        self._policy_step.launch(obs)
        if self.direct:
            self.last_mpc = self._direct
        else:
            weights, ref_speed = (fg["w"], None) if self.version == "v1" else (self.default_weights, fg["rs"])
            self._mpc_out = self.engine.predict_batch_torch(obs, weights, ref_speed, collision_cost=self.collision_cost,
                                                            warm_start=self.warm_start, out=self._mpc_out, **self._mpc_kw)
            self.last_mpc = self._mpc_out
        mpc_action = self.last_mpc["act"]
        if self.gather_actions:
            from . import sharding
            self.gathered_actions, self.gathered_status = sharding.all_gather_results(mpc_action, self.last_mpc["status"])
        self.env.step(mpc_action)
        if self.reset_mpc_on_done:
            self.engine.reset_env_mask_torch(self.env._out["done"])
        elif self.warm_start:
            self.engine.reset_env_mask_torch(self.env._out["done"], warm_only=True)
        self._record(mpc_action, self.last_mpc["status"])

    def _record(self, mpc_action, status):
        """Buffer row, carry-over to the next step and the rollout's counters in one launch (mpc_rollout_record)."""
        buf, fg, o, r = self.buffer, self._fg, self.env._out, self._roll
        keep = buf.terminal_obs is not None
        _engine.caller("mpc_rollout_record")(
            lib=self.engine._lib, device=self.env.device.index, T=buf.n_steps, B=self.env.num_envs, A=self.policy.action_dim,
            cols=buf._cols, keep_terminal=1 if keep else 0, row=buf._row, mpc_actions_buf=buf.mpc_actions, pos_dev=buf.pos_dev,
            ticket=self._ticket, last_obs=self._last_obs, last_starts=self._last_episode_starts, actions=fg["act"],
            values=fg["val"], log_probs=fg["logp"], mpc_act=mpc_action, mpc_status=status, new_obs=o["obs"],
            reward=o["reward"], done=o["done"], terminal_obs=o["terminal_obs"] if keep else None,
            truncated=o["truncated"] if keep else None, crashed=o["crashed"], arrived=o["arrived"], counts=r["counts"],
            dones_out=r["dones"], step_counter=fg["step"], stream=_engine.current_stream(self.env.device))

    @torch.no_grad()
    def _rollout_step(self, device_pos: bool = False):
        if self.fused_glue:
            self._rollout_step_fused()
            if not device_pos:
                self.buffer.pos += 1
            return
        obs = self._last_obs
        # (noise_feed: a list of per-step draws to consume instead of the generator's - how the tests give this path the
        # draws the glue kernel made)
        feed = getattr(self, "noise_feed", None)
        noise = feed.pop(0) if feed else (self.sde_noise if self.use_sde else None)
        actions, values, log_probs = self.policy.act(obs, generator=self.gen, noise=noise)
        if self.direct:                  # the end-to-end baseline: the action is the control, nothing to solve
            map_control(actions, out=self._direct["act"], scale=self._control_scale)
            self.last_mpc = self._direct
        else:
            weights, ref_speed = mpc_inputs(actions, self.version, self.default_weights, clip=self.algorithm == "ppo")
            self._mpc_out = self.engine.predict_batch_torch(obs, weights, ref_speed, collision_cost=self.collision_cost,
                                                            warm_start=self.warm_start, out=self._mpc_out, **self._mpc_kw)
            self.last_mpc = self._mpc_out
        mpc_action = self.last_mpc["act"]
        if self.gather_actions:
            from . import sharding
            # every rank sees every environment's action and whether its solve converged
            self.gathered_actions, self.gathered_status = sharding.all_gather_results(mpc_action, self.last_mpc["status"])
        new_obs, rewards, dones, info = self.env.step(mpc_action)
        # (PPO, agents/ppo_mpc.py:451-461: a truncated episode's last reward is bootstrapped with the value of its terminal
        # observation - kept here, applied for the whole rollout by _finish_rollout)
        term = dict(terminal_obs=info["terminal_obs"], truncated=info["truncated"]) if self.algorithm == "ppo" else {}
        if self.reset_mpc_on_done:
            self.engine.reset_env_mask_torch(dones.view(torch.uint8))
        elif self.warm_start:            # a new episode must not start from the old one's plan
            self.engine.reset_env_mask_torch(dones.view(torch.uint8), warm_only=True)
        if device_pos:
            self.buffer.add_at_device_pos(obs, actions, rewards, self._last_episode_starts, values, log_probs, mpc_action,
                                          **term)
        else:
            self.buffer.add(obs, actions, rewards, self._last_episode_starts, values, log_probs, mpc_action, **term)
        self._last_obs.copy_(new_obs)
        self._last_episode_starts.copy_(dones)
        r = self._roll
        r["dones"].copy_(dones)
        # like the reference (agents/pure_mpc.py:303-305) an unconverged solve still acts with its last iterate; the
        # collector counts them so that a training run can see what fraction of its actions that was
        st = self.last_mpc["status"]
        r["counts"][:4] += torch.stack((dones, info["crashed"], info["arrived"], (st != 0) & ((st < 5) | (st > 7)))).sum(dim=1)

    def _capture(self):
        """Capture one rollout step (policy -> mpc_predict_batch -> environment step -> buffer row) as a hipGraph: a step
        is ~100 small launches, ~2 ms of host time, which a replay replaces by one launch.  Every tensor the step reads or
        writes across steps lives at a fixed address (environment state, last observation, buffer, counters); the buffer
        row comes from a device-side counter; both random generators are registered with the graph."""
        dev = self.env.device
        env, B = self.env, self.env.num_envs
        if hasattr(self.engine, "reserve_envs"):     # the handle's per-environment buffers must not grow inside the capture
            self.engine.reserve_envs(B)
        # The warm-up and capture steps below really step the environment and the detector.  Everything they touch is
        # snapshotted here and put back afterwards, so that building the collector changes nothing the caller can see:
        # episodes, random streams (both generators, the fused environment's counters), the observation, and the engine's
        # detector records - including records a caller restored with mpc_set_env_state before building the collector
        # (resume).  A graph collector and an eager one with the same seeds therefore produce the same rollouts
        # (tests/test_predict_gpu.py::test_graph_and_eager_collectors_produce_the_same_rollout).
        snap = {n: t.clone() for n, t in env.state_tensors().items()}
        snap_obs, snap_starts = self._last_obs.clone(), self._last_episode_starts.clone()
        gen_states = [self.gen.get_state(), env.gen.get_state()]
        snap_step = self._fg["step"].clone() if self.fused_glue else None
        records = self.engine.save_env_state(B) if hasattr(self.engine, "save_env_state") else None
        side = torch.cuda.Stream(dev)
        try:
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(2):                       # allocations and lazy initialisation happen outside the capture
                    self._rollout_step(device_pos=True)
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize(dev)
            g = torch.cuda.CUDAGraph()
            for gen in (self.gen, self.env.gen):
                g.register_generator_state(gen)
            with torch.cuda.graph(g, stream=side):
                self._rollout_step(device_pos=True)
            self._graph = g
        except BaseException as capture_error:
            # the capture FAILED: put the collector back as if it had never tried, and should the restore itself fail
            # (a synchronize or a state load after an invalidated capture), chain it so that the capture's error stays visible
            try:
                self._restore_after_capture(snap, snap_obs, snap_starts, gen_states, snap_step, records)
            except Exception as restore_error:      # noqa: BLE001
                raise restore_error from capture_error
            raise
        else:
            self._restore_after_capture(snap, snap_obs, snap_starts, gen_states, snap_step, records)

    def _restore_after_capture(self, snap, snap_obs, snap_starts, gen_states, snap_step, records):
        """Put back what the warm-up / capture steps of _capture() touched (in place: a graph replays against these addresses)."""
        env = self.env
        torch.cuda.synchronize(env.device)
        self.buffer.reset()
        for n, t in env.state_tensors().items():
            t.copy_(snap[n])
        self._last_obs.copy_(snap_obs)
        self._last_episode_starts.copy_(snap_starts)
        self.gen.set_state(gen_states[0])
        env.gen.set_state(gen_states[1])
        if snap_step is not None:
            self._fg["step"].copy_(snap_step)
        if records is not None:
            self.engine.load_env_state(records)       # also forgets the warm-start memory the warm-up steps left
        self._roll["counts"].zero_()
        self._roll["dones"].zero_()

    def _step(self):
        f = self.sde_sample_freq
        if self.use_sde and not self.fused_glue and f > 0 and self.buffer.pos > 0 and self.buffer.pos % f == 0:
            self._sde_resample()           # every sde_sample_freq steps (agents/ppo_mpc.py:386-388; the fused step keys by pos)
        if self._graph is not None:
            self._graph.replay()
            self.buffer.pos += 1
        else:
            self._rollout_step()
        self.num_timesteps += self.env.num_envs

    @torch.no_grad()
    def _finish_rollout(self):
        last_values = self.policy.predict_values(self._last_obs)
        if not self.fused_glue:
            self.buffer.bootstrap_truncated(self.policy.predict_values)
            self.buffer.compute_returns_and_advantage(last_values, self._roll["dones"])
            return
        # the same arithmetic in one launch (mpc_rollout_finish) instead of 11 torch kernels per step of the rollout
        buf, dev, B = self.buffer, self.env.device, self.env.num_envs
        T = buf.n_steps
        tv = None
        if buf.terminal_obs is not None:
            tv = self.policy.predict_values(buf.terminal_obs.reshape((T * B,) + buf.terminal_obs.shape[2:])).contiguous()
        _engine.call("mpc_rollout_finish", lib=self.engine._lib, device=dev.index, T=T, B=B, A=self.policy.action_dim,
                     cols=buf._cols, keep_terminal=1 if buf.terminal_obs is not None else 0, row=buf._row,
                     last_values=last_values.contiguous(), dones=self._roll["dones"], terminal_values=tv, gamma=buf.gamma,
                     gae_lambda=buf.gae_lambda, advantages=buf.advantages, returns=buf.returns,
                     stream=_engine.current_stream(dev))

    def _rollout_stats(self, n):
        r = self._roll
        # counts[4]: steps mpc_rollout_record refused because the buffer was already full (the torch path raises IndexError
        # there); read back with the other counters at the end of the rollout and never silent
        refused = int(r["counts"][4])
        if refused:
            raise IndexError(f"{refused} rollout steps were recorded past the end of the buffer ({self.buffer.n_steps} steps)")
        return dict(steps=n * self.env.num_envs, episodes=int(r["ep_done"]), crashed=int(r["crashed"]),
                    arrived=int(r["arrived"]), mpc_unconverged=int(r["unconverged"]), refused_steps=refused)

    def collect_rollouts(self, n_rollout_steps: int | None = None):
        n = self.buffer.n_steps if n_rollout_steps is None else int(n_rollout_steps)
        assert n == self.buffer.n_steps
        self._begin_rollout()
        for _ in range(n):
            self._step()
        self._finish_rollout()
        return self._rollout_stats(n)

    def flat_buffer(self):
        """(obs, actions, log_probs, advantages, returns) with time and environment flattened, for the update"""
        b = self.buffer
        f = lambda t: t.reshape((-1,) + t.shape[2:])
        return f(b.obs), f(b.actions), f(b.log_probs), f(b.advantages), f(b.returns)

    def mean_reward(self):
        return float(self.buffer.rewards.mean())


class PipelinedCollector:
    """Several BatchedCollectors (disjoint environment groups, one engine handle each, one shared policy) stepped
    round-robin on their own HIP streams.  A batched MPC solve ends with a long tail - a few slow instances on an
    otherwise idle GPU - and the groups are independent, so the tail of one group's solve overlaps
    with the policy / preamble / bulk of the others'.  Pays only with `use_graph=True` collectors: in eager mode the host
    needs ~2 ms to launch one group's step and the groups serialise on that.  Same data as running the collectors one
    after the other (each group's chain of operations is unchanged and ordered on its stream); the update sees the
    concatenated buffers."""

    def __init__(self, collectors):
        if not collectors:
            raise ValueError("need at least one collector")
        self.collectors = list(collectors)
        c0 = self.collectors[0]
        if any(c.policy is not c0.policy or c.algorithm != c0.algorithm or c.buffer.n_steps != c0.buffer.n_steps
               for c in self.collectors):
            raise ValueError("the collectors must share the policy, the algorithm and the rollout length")
        if len({id(c.engine) for c in self.collectors}) != len(self.collectors):
            raise ValueError("every collector needs its own engine handle (calls on one handle must not overlap)")
        self.policy, self.algorithm, self.env = c0.policy, c0.algorithm, c0.env
        # streams that really overlap (two that share a hardware queue serialise; engine.concurrent_streams probes each): with
        # more groups than the runtime has queues the rest are taken as they come
        from . import engine as _engine
        dev = c0.env.device
        try:
            self.streams = _engine.concurrent_streams(len(self.collectors), dev)
        except _engine.EngineError:
            self.streams = [torch.cuda.Stream(dev) for _ in self.collectors]

    @property
    def num_timesteps(self):
        return sum(c.num_timesteps for c in self.collectors)

    def collect_rollouts(self, n_rollout_steps: int | None = None):
        n = self.collectors[0].buffer.n_steps if n_rollout_steps is None else int(n_rollout_steps)
        assert all(n == c.buffer.n_steps for c in self.collectors), "a rollout is exactly one buffer of steps"
        cur = torch.cuda.current_stream(self.env.device)
        for s in self.streams:
            s.wait_stream(cur)                      # the groups see everything enqueued so far (policy update, resets)
        for c, s in zip(self.collectors, self.streams):
            with torch.cuda.stream(s):
                c._begin_rollout()
        for _ in range(n):
            for c, s in zip(self.collectors, self.streams):
                with torch.cuda.stream(s):
                    c._step()
        for c, s in zip(self.collectors, self.streams):
            with torch.cuda.stream(s):
                c._finish_rollout()
        for s in self.streams:
            cur.wait_stream(s)                      # ... and the update sees every group's buffer
        stats = [c._rollout_stats(n) for c in self.collectors]
        return {k: sum(d[k] for d in stats) for k in stats[0]}

    def flat_buffer(self):
        parts = [c.flat_buffer() for c in self.collectors]
        return tuple(torch.cat([p[i] for p in parts], dim=0) for i in range(5))

    def mean_reward(self):
        return float(torch.cat([c.buffer.rewards.reshape(-1) for c in self.collectors]).mean())


class OnPolicyTrainer:
    """collect -> update loop of the reference's MPC-RL agents for B environments (`PPO_MPC.learn/train`
    agents/ppo_mpc.py:218-330, `A2C_MPC.train` agents/a2c_mpc.py:182-226; both are stable-baselines3's on-policy
    algorithms with the MPC call inside `collect_rollouts`).  The update is what those `train()` methods compute:

      ppo  n_epochs passes over the buffer in shuffled minibatches; clipped surrogate
           -mean(min(A r, A clip(r, 1-eps, 1+eps))) with r = exp(logp - logp_old), advantages normalised per minibatch,
           + vf_coef * mse(returns, V) + ent_coef * (-mean entropy); Adam, gradient-norm clip
           (defaults of config/cfg.yaml:66-86: lr 3e-4, 10 epochs, clip 0.2, gamma 0.99, lambda 0.95)
      a2c  one step on the whole buffer: -mean(A logp) + vf_coef * mse + ent_coef * (-mean entropy); RMSprop
           (alpha 0.99, eps 1e-5), no advantage normalisation, lambda 1 (config/cfg.yaml:31-61)

    A gSDE policy (ActorCritic(use_sde=True)) needs nothing else here: evaluate_actions carries its distribution.  SB3's PPO
    calls reset_noise(batch_size) before every minibatch (agents/ppo_mpc.py:243-244), but the loss never reads the
    exploration matrices - log_prob and entropy depend only on the mean and on latent^2 @ exp(log_std)^2 - so those draws
    cannot change the loss; they only renew matrices that the next rollout start redraws anyway.
    """

    def __init__(self, collector, learning_rate: float | None = None, n_epochs: int = 10,
                 batch_size: int = 256, clip_range: float = 0.2, ent_coef: float = 0.0, vf_coef: float = 0.5,
                 max_grad_norm: float = 0.5, normalize_advantage: bool | None = None, seed: int = 0):
        self.col = collector
        self.algorithm = collector.algorithm
        pol = collector.policy
        if self.algorithm == "ppo":
            self.opt = torch.optim.Adam(pol.parameters(), lr=3e-4 if learning_rate is None else learning_rate, eps=1e-5)
            self.normalize_advantage = True if normalize_advantage is None else normalize_advantage
        else:
            self.opt = torch.optim.RMSprop(pol.parameters(), lr=7e-4 if learning_rate is None else learning_rate,
                                           alpha=0.99, eps=1e-5)
            self.normalize_advantage = False if normalize_advantage is None else normalize_advantage
        self.n_epochs, self.batch_size, self.clip_range = int(n_epochs), int(batch_size), float(clip_range)
        self.ent_coef, self.vf_coef, self.max_grad_norm = float(ent_coef), float(vf_coef), float(max_grad_norm)
        self.gen = torch.Generator(device=collector.env.device)
        self.gen.manual_seed(int(seed))
        self.n_updates = 0

    def _flat(self):
        return self.col.flat_buffer()

    def _loss(self, obs, actions, old_logp, adv, ret):
        values, logp, entropy = self.col.policy.evaluate_actions(obs, actions)
        if self.normalize_advantage and adv.numel() > 1:
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        if self.algorithm == "ppo":
            ratio = torch.exp(logp - old_logp)
            pg = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1.0 - self.clip_range, 1.0 + self.clip_range)).mean()
        else:
            pg = -(adv * logp).mean()
        vl = torch.nn.functional.mse_loss(ret, values)
        el = -entropy.mean()
        return pg + self.ent_coef * el + self.vf_coef * vl, pg, vl, el

    def train(self):
        """One update from the collector's (full) buffer; returns the mean losses."""
        pol = self.col.policy
        pol.train()
        obs, actions, old_logp, adv, ret = self._flat()
        n = obs.shape[0]
        stats = []
        if self.algorithm == "ppo":
            for _ in range(self.n_epochs):
                perm = torch.randperm(n, generator=self.gen, device=obs.device)
                for lo in range(0, n, self.batch_size):
                    idx = perm[lo:lo + self.batch_size]
                    loss, pg, vl, el = self._loss(obs[idx], actions[idx], old_logp[idx], adv[idx], ret[idx])
                    self.opt.zero_grad()
                    loss.backward()
                    torch.nn.utils.clip_grad_norm_(pol.parameters(), self.max_grad_norm)
                    self.opt.step()
                    stats.append(torch.stack([loss.detach(), pg.detach(), vl.detach(), el.detach()]))
                self.n_updates += 1
        else:
            loss, pg, vl, el = self._loss(obs, actions, old_logp, adv, ret)
            self.opt.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(pol.parameters(), self.max_grad_norm)
            self.opt.step()
            stats.append(torch.stack([loss.detach(), pg.detach(), vl.detach(), el.detach()]))
            self.n_updates += 1
        m = torch.stack(stats).mean(dim=0).tolist()
        return dict(loss=m[0], policy_loss=m[1], value_loss=m[2], entropy_loss=m[3])

    def learn(self, total_timesteps: int):
        """collect_rollouts / train until `total_timesteps` environment steps were taken (BaseAlgorithm.learn)."""
        log = []
        while self.col.num_timesteps < total_timesteps:
            roll = self.col.collect_rollouts()
            upd = self.train()
            log.append(dict(roll, **upd, timesteps=self.col.num_timesteps,
                            mean_reward=self.col.mean_reward()))
        return log


class _PolicyAgent:
    """What MPCRLAgent and PPOAgent share: an ActorCritic policy and an engine, SB3 checkpoints, the policy's output, and the
    closed-loop evaluation's contract (evaluate.evaluate_agent) - `act_batch_torch` with the state it keeps between calls and
    `restart_actions`.  A subclass says whether the fused policy step can run (`_fusable`) and in which mode (`_mode`), which
    buffers its state needs besides (`_act_buffers`), and how the action becomes what the environment gets (`_act`)."""

    DETERMINISTIC = False          # policy_output's default, the one of the reference's predict
    HAS_PLAN = True                # act_batch_torch(plan=True) returns the MPC's planned trajectory

    @classmethod
    def from_sb3(cls, path, engine=None, device="cpu", **kw):
        """Load an SB3 checkpoint (ActorCritic.load_sb3; what ActorCritic.save_sb3 writes) and wrap it -> (agent, meta)."""
        pol, meta = ActorCritic.load_sb3(path, device=device)
        return cls(pol, engine, **cls._sb3_settings(meta, kw)), meta

    @staticmethod
    def _sb3_settings(meta, kw):
        return kw

    @torch.no_grad()
    def policy_output(self, obs, deterministic: bool | None = None, generator=None):
        self.policy.eval()
        obs = torch.as_tensor(obs, dtype=torch.float32, device=self.policy.log_std.device)
        deterministic = self.DETERMINISTIC if deterministic is None else deterministic
        actions, _, _ = self.policy(obs, deterministic=deterministic, generator=generator)
        return actions

    @torch.no_grad()
    def act_batch_torch(self, obs, deterministic: bool = False, seed: int = 0, env_offset: int = 0, plan: bool = False):
        """obs float32 device tensor [B, 10, 8] -> dict(act [B, 2] f64, status, iters, step, generator): the policy, then the
        subclass's `_act`; plan=True: also the MPC's plan_U, plan_X and plan_order (engine.predict_batch_torch), on the fused
        and the unfused path alike - ValueError for an agent without an MPC (PPOAgent).  Enqueue-only, the same output tensors every call.  With `_fusable` and the observation on a GPU
        the policy is one launch (FusedPolicy, the collector's kernels), otherwise ActorCritic.act.
          deterministic  the mean: the fused kernel reads all-zero noise, `step` is None and no generator is returned
          stochastic     fused: noise keyed by (seed, env_offset + b, step), `step` the int64 [1] counter the caller
                         advances once per step (mpc_episode_stats does); torch: drawn from `generator` (seeded by seed)
          gSDE           one exploration matrix per environment for the whole evaluation (what reset_noise(B) draws, never
                         resampled, agents/ppo_mpc.py:627-628): fused, keyed by (seed, env_offset + b, epoch 0); torch, drawn
                         once from a generator seeded by seed
        restart_actions() puts the counters / matrices back to their start."""
        if plan and not self.HAS_PLAN:
            raise ValueError(f"{type(self).__name__} has no plan: there is no MPC between the policy and the controls")
        key = (int(obs.shape[0]), obs.device, bool(deterministic), int(seed), int(env_offset))
        st = getattr(self, "_act_state", None)
        if st is None or st["key"] != key:
            st = self._act_init(key)
        actions = None
        if st["fused"]:
            st["policy_step"].launch(obs)
        else:
            actions, _, _ = self.policy.act(obs, generator=st["gen"], noise=st["noise"])
        draws = not st["fused"] and not deterministic and not self.policy.use_sde
        return dict(self._act(st, obs, actions, plan), step=st["step"], generator=st["gen"] if draws else None)

    def _fused_policy(self, key):
        B, dev, deterministic, seed, env_offset = key
        return FusedPolicy(self.policy, B, dev, self.engine._lib, self._mode, seed=seed, env_offset=env_offset,
                           deterministic=deterministic)

    def _act_init(self, key):
        B, dev, deterministic, seed, _ = key
        pol = self.policy
        pol.eval()
        pol.refresh_fused()
        A, H = pol.action_dim, pol.pi[0].out_features
        z = lambda *sh, dt=torch.float32: torch.zeros(sh, dtype=dt, device=dev)
        st = dict(key=key, fused=dev.type == "cuda" and self._fusable(), out=None, step=None, gen=None, noise=None)
        if st["fused"]:
            st["policy_step"] = self._fused_policy(key)
            st["fg"] = st["policy_step"].tensors
            if not pol.use_sde:                # None when deterministic: the kernel reads the all-zero noise instead
                st["step"] = st["fg"]["step"]
        elif deterministic:
            st["noise"] = z(B, H, A) if pol.use_sde else z(B, A)
        else:
            st["gen"] = torch.Generator(device=dev)
            st["gen"].manual_seed(seed)
            if pol.use_sde:
                st["noise"] = z(B, H, A, dt=pol.log_std.dtype).normal_(generator=st["gen"])
        self._act_buffers(st, B, dev)
        self._act_state = st
        return st

    @torch.no_grad()
    def restart_actions(self):
        """Put the evaluation's noise counter, generator and exploration matrices back to where act_batch_torch started them
        (in place: a captured graph reads them at their addresses)."""
        st = getattr(self, "_act_state", None)
        if st is None:
            return
        self.policy.refresh_fused()
        if st["step"] is not None:
            st["step"].zero_()
        if st["gen"] is not None:
            st["gen"].manual_seed(st["key"][3])
            if self.policy.use_sde:
                st["noise"].normal_(generator=st["gen"])


class MPCRLAgent(_PolicyAgent):
    """The reference's `trainer.predict(obs)` (trainers/trainer.py:342-368) for a batch of observations: the policy forward,
    then the MPC with its output - version "v0" hands action 0 to the MPC as the reference speed, "v1" actions 0..2 as the
    cost weights.  Like the reference the policy output is stochastic and NOT clipped, whatever the algorithm.

    gSDE policies: the reference draws ONE exploration matrix when it loads a checkpoint (agents/ppo_mpc.py:627-628) and
    predict never resamples, so every later prediction explores with that same matrix.  reset_noise() draws it per
    environment (one matrix per row of the batch, kept until the next reset_noise()); without it the policy's single matrix
    serves every row, as in the reference."""

    def __init__(self, policy: ActorCritic, engine, version: str = "v0", algorithm: str = "ppo",
                 default_weights=(1.0, 1.0, 1.0), collision_cost: bool = False):
        if version not in ("v0", "v1") or algorithm not in ("ppo", "a2c"):
            raise ValueError("version must be v0|v1 and algorithm ppo|a2c")
        if version == "v1" and policy.action_dim < 3:
            raise ValueError("v1 needs an action of at least 3 components (speed, control, input_diff weights)")
        self.policy, self.engine, self.version, self.algorithm = policy, engine, version, algorithm
        self._mode = version
        self.default_weights = tuple(float(w) for w in default_weights)
        self.collision_cost = bool(collision_cost)

    @staticmethod
    def _sb3_settings(meta, kw):
        """version / algorithm from the checkpoint unless given"""
        return dict(dict(version=meta["version"] or "v0", algorithm=meta["algorithm"] or "ppo"), **kw)

    @torch.no_grad()
    def reset_noise(self, n: int, generator=None):
        self.policy.reset_noise(n, generator=generator)

    def _weights(self, B, dev):
        return torch.tensor(self.default_weights, dtype=torch.float64, device=dev).repeat(B, 1).contiguous()

    @torch.no_grad()
    def predict_batch(self, obs_batch, deterministic: bool = False, generator=None):
        """obs_batch [B, 10, 8] -> dict(act [B, 2], status, iters, rl_action [B, A]).  A torch tensor on a GPU goes through
        engine.predict_batch_torch (zero-copy, synchronised before returning); anything else through engine.predict_batch."""
        actions = self.policy_output(obs_batch, deterministic, generator)
        weights, ref_speed = mpc_inputs(actions, self.version, self._weights(actions.shape[0], actions.device))
        if actions.is_cuda and hasattr(self.engine, "predict_batch_torch"):
            obs = torch.as_tensor(obs_batch, dtype=torch.float32, device=actions.device).contiguous()
            out = self.engine.predict_batch_torch(obs, weights, ref_speed, collision_cost=self.collision_cost, sync=True)
        else:
            out = self.engine.predict_batch(np.asarray(torch.as_tensor(obs_batch, dtype=torch.float32).cpu()),
                                            weights.cpu().numpy(), None if ref_speed is None else ref_speed.cpu().numpy(),
                                            collision_cost=self.collision_cost)
        return dict(out, rl_action=actions)

    # ---- closed-loop evaluation (_PolicyAgent.act_batch_torch): the MPC through engine.predict_batch_torch with the policy's
    #      action mapped like mpc_inputs and unclipped (trainer.predict)
    def _fusable(self):
        return fits_fused_policy(self.policy, self.engine) and hasattr(self.engine, "predict_batch_torch")

    def _act_buffers(self, st, B, dev):
        st["w"] = self._weights(B, dev)

    def _act(self, st, obs, actions, plan=False):
        if actions is None:                    # the fused launch left the MPC's inputs in its buffers
            fg = st["fg"]
            weights, ref_speed = (fg["w"], None) if self.version == "v1" else (st["w"], fg["rs"])
        else:
            weights, ref_speed = mpc_inputs(actions, self.version, st["w"])
        st["out"] = self.engine.predict_batch_torch(obs, weights, ref_speed, collision_cost=self.collision_cost, out=st["out"],
                                                    **(dict(plan=True) if plan else {}))
        return st["out"]

    def predict(self, obs, deterministic: bool = False, generator=None):
        """One observation [10, 8] -> the MPC action [2] (trainer.predict)."""
        out = self.predict_batch(torch.as_tensor(obs, dtype=torch.float32)[None], deterministic, generator)
        act = out["act"][0]
        return act.cpu().numpy() if isinstance(act, torch.Tensor) else act


class PPOAgent(_PolicyAgent):
    """The reference's end-to-end baseline (agents/ppo_agent.py `PPOAgent`, the `ppo` model of main/model_comparison.py): an SB3
    MlpPolicy whose two outputs are the vehicle's controls, with no MPC in between.  The environment's action type
    (highway-env's ContinuousAction) clips the action to [-1, 1] and scales it onto the acceleration / steering ranges
    (map_control); here that mapping is part of the agent, because the batched environments take physical controls.
    Gaussian policies with action_dim 2 only.  `engine` (an MPCEngine) is used for its library alone - the fused policy step
    mpc_policy_control on a GPU; None runs the policy in torch, on any device."""

    DETERMINISTIC = True           # agents/ppo_agent.py's default
    HAS_PLAN = False               # no MPC, hence no planned trajectory
    _mode = "direct"

    def __init__(self, policy: ActorCritic, engine=None):
        _check_direct_policy(policy)
        self.policy, self.engine = policy, engine

    def predict(self, obs, deterministic: bool = True, generator=None):
        """One observation [10, 8] -> the normalised action [2] float32 clipped to [-1, 1], what SB3's `model.predict`
        returns and the reference hands to env.step (agents/ppo_agent.py; deterministic=True is its default)."""
        actions = self.policy_output(torch.as_tensor(obs, dtype=torch.float32)[None], deterministic, generator)
        return torch.clamp(actions[0], -1.0, 1.0).cpu().numpy()

    @torch.no_grad()
    def predict_batch(self, obs_batch, deterministic: bool = True, generator=None):
        """obs_batch [B, 10, 8] -> dict(act [B, 2] f64 physical controls, rl_action [B, 2] the unclipped action, status and
        iters [B] int32 zeros: there is no solve)."""
        actions = self.policy_output(obs_batch, deterministic, generator)
        zi = lambda: torch.zeros(actions.shape[0], dtype=torch.int32, device=actions.device)
        return dict(act=map_control(actions), rl_action=actions, status=zi(), iters=zi())

    # ---- closed-loop evaluation (_PolicyAgent.act_batch_torch): act = the controls, written by the fused launch itself or by
    #      map_control; status and iters stay zero
    def _fusable(self):
        return fits_fused_policy(self.policy, self.engine)

    def _act_buffers(self, st, B, dev):
        zi = lambda: torch.zeros(B, dtype=torch.int32, device=dev)
        st["scale"] = control_scale(dev)
        st["out"] = dict(act=st["fg"]["ctrl"] if st["fused"] else torch.zeros((B, 2), dtype=torch.float64, device=dev),
                         status=zi(), iters=zi())

    def _act(self, st, obs, actions, plan=False):
        if actions is not None:
            map_control(actions, out=st["out"]["act"], scale=st["scale"])
        return st["out"]
