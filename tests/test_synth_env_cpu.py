"""The fused environment step (mpc-rl_for_avs_amd/csrc/mpc_synth_env.hpp, the kernel behind `mpc_synth_env_step`)
compiled for the host, against the torch implementation in rollout.SyntheticIntersectionEnv that it replaces on the GPU:
the deterministic part of a step (vehicle models, crash / arrival / truncation, reward, the sorted observation) must agree
statement for statement; the random part (respawn, reset) is checked through its distributions."""
import ctypes
import glob
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import BUILD_DIR, HOST_CXXFLAGS, ROOT


def load_synth_lib():
    out = os.path.join(BUILD_DIR, "libcpu_synth_env.so")
    src = os.path.join(ROOT, "tests", "cpu_synth_env_harness.cpp")
    deps = [src] + glob.glob(os.path.join(ROOT, "mpc-rl_for_avs_amd", "csrc", "*.hpp"))
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(BUILD_DIR, exist_ok=True)
        subprocess.run(["g++"] + HOST_CXXFLAGS + ["-o", out, src], check=True)
    return ctypes.CDLL(out)


@pytest.fixture(scope="module")
def lib():
    return load_synth_lib()


class HostEnv:
    """The harness behind the interface of the torch class (numpy state)."""

    def __init__(self, lib, B, K, seed=0, spawn_probability=0.3, env_offset=0):
        from mpc_rl_for_avs_amd.reference_path import reference_states
        self.lib, self.B, self.K, self.seed, self.sp, self.off = lib, B, K, seed, spawn_probability, env_offset
        Ks = max(K, 1)
        self.ref = np.ascontiguousarray(reference_states(0.1)[:, :2])
        self.ego = np.zeros((B, 4)); self.opos = np.zeros((B, Ks, 2)); self.ospeed = np.zeros((B, Ks))
        self.ohead = np.zeros((B, Ks)); self.oactive = np.zeros((B, Ks), np.uint8); self.t = np.zeros(B, np.int32)
        self.ctr = np.zeros(B, np.int64)
        self.obs = np.zeros((B, 10, 8), np.float32); self.tobs = np.zeros((B, 10, 8), np.float32)
        self.reward = np.zeros(B, np.float32)
        self.flags = {k: np.zeros(B, np.uint8) for k in ("done", "truncated", "crashed", "arrived")}

    def _call(self, action, reset_all):
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        f = self.flags
        rc = self.lib.synth_env_step(self.B, self.K, ctypes.c_double(0.1), ctypes.c_double(self.sp), ctypes.c_uint64(self.seed),
                                     self.off, p(self.ref), self.ref.shape[0], p(action), p(self.ego), p(self.opos),
                                     p(self.ospeed), p(self.ohead), p(self.oactive), p(self.t), p(self.ctr), p(self.obs),
                                     p(self.tobs), p(self.reward), p(f["done"]), p(f["truncated"]), p(f["crashed"]),
                                     p(f["arrived"]), 1 if reset_all else 0)
        assert rc == 0

    def reset(self):
        self._call(None, True)
        return self.obs

    def step(self, action):
        self._call(np.ascontiguousarray(action, dtype=np.float64), False)
        return self.obs, self.reward, self.flags["done"].astype(bool)


def _copy_state(src, dst):
    """host harness state -> torch environment"""
    dst.ego.copy_(torch.from_numpy(src.ego)); dst.opos.copy_(torch.from_numpy(src.opos))
    dst.ospeed.copy_(torch.from_numpy(src.ospeed)); dst.ohead.copy_(torch.from_numpy(src.ohead))
    dst.oactive.copy_(torch.from_numpy(src.oactive.astype(bool))); dst.t.copy_(torch.from_numpy(src.t))


@pytest.mark.parametrize("K", [0, 1, 4, 9])
def test_deterministic_part_equals_the_torch_environment(lib, K):
    from mpc_rl_for_avs_amd import rollout
    B = 64
    h = HostEnv(lib, B, K, seed=3, spawn_probability=0.0)        # vehicles that leave stay away: no random draw in a step
    obs = h.reset().copy()
    t = rollout.SyntheticIntersectionEnv(B, device="cpu", seed=0, n_others=K, spawn_probability=0.0, backend="torch")
    _copy_state(h, t)
    assert np.array_equal(t.observe().numpy(), obs)             # same sorted float32 observation of the same state
    # a quarter of the egos start on the exit straight, a few metres before the end of the route: arrivals
    h.ego[: B // 4] = np.stack([h.ref[70, 0] + np.linspace(0.0, 4.0, B // 4), np.full(B // 4, h.ref[70, 1]),
                                np.full(B // 4, -np.pi), np.full(B // 4, 10.0)], axis=1)
    _copy_state(h, t)
    rng = np.random.default_rng(K)
    alive = np.ones(B, bool)
    n_crash = n_arrive = 0
    for step in range(120):
        act = np.stack([rng.uniform(-6, 6, B), rng.uniform(-1.0, 1.0, B)], axis=1)
        act[:, 1] *= 0.05                                        # mostly straight: some episodes reach the crossing traffic
        act[: B // 4] = 0.0                                      # the ones on the exit straight just roll on
        o_h, r_h, d_h = h.step(act)
        o_t, r_t, d_t, info = t.step(torch.from_numpy(act))
        a = alive
        assert np.array_equal(d_h[a], d_t.numpy()[a]), step
        assert np.array_equal(h.flags["crashed"].astype(bool)[a], info["crashed"].numpy()[a])
        assert np.array_equal(h.flags["arrived"].astype(bool)[a], info["arrived"].numpy()[a])
        assert np.array_equal(h.flags["truncated"].astype(bool)[a], info["truncated"].numpy()[a])
        assert np.allclose(r_h[a], r_t.numpy()[a], rtol=0, atol=1e-4)
        assert np.allclose(h.tobs[a], info["terminal_obs"].numpy()[a], rtol=0, atol=1e-5)
        n_crash += int(h.flags["crashed"].astype(bool)[a].sum())
        n_arrive += int(h.flags["arrived"].astype(bool)[a].sum())
        alive = alive & ~d_h                                     # after a reset the two draw different episodes
        keep = alive
        assert np.allclose(h.ego[keep], t.ego.numpy()[keep], rtol=0, atol=1e-9)
        assert np.allclose(h.opos[keep], t.opos.numpy()[keep], rtol=0, atol=1e-9)
        assert np.array_equal(o_h[keep], o_t.numpy()[keep]) or np.allclose(o_h[keep], o_t.numpy()[keep], rtol=0, atol=1e-5)
    assert n_arrive >= B // 4 - 2 and (~alive).sum() >= B // 4 - 2   # episodes did end, on both sides alike
    if K >= 4:
        assert n_crash >= 1


def test_truncation_after_200_steps(lib):
    h = HostEnv(lib, 8, 0, seed=1)
    h.reset()
    brake = np.tile([-5.0, 0.0], (8, 1))                          # stands still on the approach lane: never arrives
    for step in range(200):
        _, _, d = h.step(brake)
        assert d.all() == (step == 199)
    assert h.flags["truncated"].all() and not h.flags["crashed"].any() and (h.t == 0).all()
    assert np.allclose(h.ego[:, 3], 10.0) and np.all(np.abs(h.ego[:, 1] - 45.0) <= 5.0)   # fresh episodes


def test_random_part_distributions_and_streams(lib):
    B, K = 4096, 9
    h = HostEnv(lib, B, K, seed=11)
    obs = h.reset().copy()
    assert np.all(h.ego[:, 0] == 2.0) and np.all(h.ego[:, 3] == 10.0) and np.allclose(h.ego[:, 2], -np.pi / 2)
    y = h.ego[:, 1]
    assert y.min() >= 40.0 and y.max() <= 50.0 and abs(y.mean() - 45.0) < 0.2 and abs(y.std() - 10 / 12 ** 0.5) < 0.1
    sp = h.ospeed.ravel()
    assert abs(sp.mean() - 8.0) < 0.05 and abs(sp.std() - 1.0) < 0.05 and sp.min() >= 0.0
    lanes = np.round(h.ohead.ravel() / (np.pi / 2)).astype(int) % 4
    assert np.all(np.abs(np.bincount(lanes, minlength=4) / lanes.size - 0.25) < 0.02)
    d = np.maximum(np.abs(h.opos[..., 0]), np.abs(h.opos[..., 1])).ravel()
    assert d.min() >= 5.0 and d.max() <= 60.0 and abs(d.mean() - 32.5) < 1.0
    # lane geometry: right-hand traffic, 2 m off the axis, heading towards the centre
    x, yy, hh = h.opos[..., 0].ravel(), h.opos[..., 1].ravel(), h.ohead.ravel()
    assert np.all(np.abs(np.where(np.abs(np.cos(hh)) > 0.5, np.abs(yy), np.abs(x)) - 2.0) < 1e-9)
    assert np.all(x * np.cos(hh) + yy * np.sin(hh) < 0.0)
    # the observation is sorted by distance, ego first, float32
    assert np.all(obs[:, :, 0] == 1.0)
    dist = np.hypot(obs[:, 1:, 1] - obs[:, :1, 1], obs[:, 1:, 2] - obs[:, :1, 2])
    assert np.all(np.diff(dist, axis=1) >= -1e-4)
    # streams: another seed, another offset and the next episode of the same environment all differ; same key repeats
    h2 = HostEnv(lib, B, K, seed=12); h2.reset()
    h3 = HostEnv(lib, B, K, seed=11, env_offset=B); h3.reset()
    h4 = HostEnv(lib, B, K, seed=11); h4.reset()
    assert np.array_equal(h4.ego, h.ego) and np.array_equal(h4.opos, h.opos)
    assert (h2.ego[:, 1] != h.ego[:, 1]).mean() > 0.99 and (h3.ego[:, 1] != h.ego[:, 1]).mean() > 0.99
    first = h.ego[:, 1].copy()
    h.reset()
    assert (h.ego[:, 1] != first).mean() > 0.99
    # respawn: with probability 0.3 per step a vehicle that left comes back 40 - 60 m out
    h5 = HostEnv(lib, 2048, 4, seed=5, spawn_probability=0.3)
    h5.reset()
    h5.oactive[:] = 0
    h5.ego[:, :2] = (300.0, 300.0)          # far from the lanes: a vehicle respawned next to the ego would end the episode
    h5.step(np.zeros((2048, 2)))
    assert not h5.flags["done"].any()
    frac = h5.oactive.mean()
    assert abs(frac - 0.3) < 0.02
    back = h5.oactive.astype(bool)
    dd = np.maximum(np.abs(h5.opos[..., 0]), np.abs(h5.opos[..., 1]))[back]
    assert dd.min() >= 40.0 and dd.max() <= 60.0


def test_zero_rows_for_absent_vehicles(lib):
    h = HostEnv(lib, 4, 3, seed=2, spawn_probability=0.0)
    h.reset()
    h.oactive[:, 1] = 0
    obs, _, _ = h.step(np.zeros((4, 2)))
    assert np.all(obs[:, 1:3, 0] == 1.0) and np.all(obs[:, 3:] == 0.0)
