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


@dataclass
class EvalResult:
    """records: dict of numpy arrays [B, Q] (steps, success, collision, truncated, avg_speed, return, unsolved, max_iters);
    steps: policy steps the batch took; env_steps = steps * B; seconds: host clock around the stepping loop (it ends in a
    synchronise)."""
    records: dict
    dt: float
    steps: int
    env_steps: int
    seconds: float

    @property
    def travel_time(self):
        return self.records["steps"] * self.dt                        # model_comparison.py:89

    def summary(self) -> dict:
        """model_comparison.py:195-199 over the B Q episodes (rates in %, means over episodes, the average speed as the mean of
        the per-episode means), plus mean_return, unsolved_frac (unsolved solves / steps of the recorded episodes), episodes,
        env_steps, seconds and env_steps_per_s."""
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
                   use_graph: bool | None = None, poll_every: int = 16, seed: int = 0, on_step=None) -> EvalResult:
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
    if on_step is not None:
        on_step(dict(reset=True, ego=env.ego))
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
    return EvalResult(records=stats.records(), dt=float(env.dt), steps=n, env_steps=n * B, seconds=seconds)


def compare(agents: dict, make_env, episodes_per_env: int = 1, **kw) -> dict:
    """Evaluate every agent on a fresh environment from make_env() (same seed: the HIP environment keys its draws by seed and
    environment id, so every agent meets the same initial episodes) -> {name: summary}."""
    return {name: evaluate_agent(agent, make_env(), episodes_per_env, **kw).summary() for name, agent in agents.items()}
