"""TEST INFRASTRUCTURE - routes and observations that drive the device preamble (csrc/mpc_preamble.hpp, mpc_preamble_wave.hpp)
into its long-table, fast-ego, many-row and same-lane corners (tests/test_preamble_cpu.py, tests/test_preamble_gpu.py)."""
import numpy as np


def route(M, spacing=0.7, v=10.0, v_fast=30.0):
    """A straight-arc-straight route like the reference's, M points `spacing` metres apart: x = 2 exactly on the first 40 %,
    a quarter turn of radius ~15 m, then the exit straight.  Reference speed v, v_fast on every seventh point."""
    s_ = np.arange(M) * spacing
    th = np.clip((s_ - 0.4 * s_[-1]) / 15.0, 0.0, np.pi / 2)
    x = 2.0 - np.concatenate([[0.0], np.cumsum(spacing * np.sin(th[:-1]))])
    y = 50.0 - np.concatenate([[0.0], np.cumsum(spacing * np.cos(th[:-1]))])
    return np.stack([x, y, np.full(M, v) + (v_fast - v) * (np.arange(M) % 7 == 0), -np.pi / 2 - th], axis=1)


def observations(rng, ref, B, rows, nv_max=None):
    """obs [B, rows, 8] float32: egos on the route at 0 - 31 m/s (half of them above 20), up to nv_max other vehicles in
    random (non-contiguous) rows: crossing traffic, same-lane traffic exactly on the x = 2 straight (collinear paths),
    crawling vehicles at 0 / 0.002 / 0.004 m/s."""
    M = len(ref)
    x, y = ref[:, 0], ref[:, 1]
    obs = np.zeros((B, rows, 8), np.float32)
    i = rng.integers(0, M, B)
    obs[:, 0, 0] = 1.0
    obs[:, 0, 1] = x[i] + rng.uniform(-0.4, 0.4, B)
    obs[:, 0, 2] = y[i] + rng.uniform(-0.4, 0.4, B)
    sp = np.where(rng.uniform(size=B) < 0.5, rng.uniform(20.0, 31.0, B), rng.uniform(0.0, 12.0, B))
    hd = ref[i, 3] + rng.uniform(-0.1, 0.1, B)
    obs[:, 0, 3], obs[:, 0, 4], obs[:, 0, 5] = sp * np.cos(hd), sp * np.sin(hd), hd
    obs[:, 0, 6], obs[:, 0, 7] = np.sin(hd), np.cos(hd)
    if rows < 2:
        return obs
    nv_max = rows - 1 if nv_max is None else nv_max
    straight = np.nonzero(x == 2.0)[0]
    for b in range(B):
        n = rng.integers(0, nv_max + 1)
        for j in rng.choice(np.arange(1, rows), size=n, replace=False):      # any rows: gaps between present ones
            r = rng.uniform()
            v = rng.uniform(0.0, 12.0)
            if rng.uniform() < 0.2:
                v = rng.choice([0.0, 0.002, 0.004])
            if r < 0.3 and len(straight) > 1:               # same lane, on the straight: x = 2 exactly, either direction
                k = straight[rng.integers(0, len(straight))]
                a = -np.pi / 2 if rng.uniform() < 0.5 else np.pi / 2
                px, py, vx, vy = 2.0, y[k] + rng.uniform(-3.0, 3.0), 0.0, v * np.sin(a)
            else:                                          # crossing traffic, or along the route next to it
                k = rng.integers(0, M)
                side = rng.uniform(-25.0, 25.0)
                a = ref[k, 3] + np.pi / 2 if r < 0.8 else ref[k, 3]
                px, py = x[k] + side * np.cos(a), y[k] + side * np.sin(a)
                s = np.sign(side) if side != 0 else 1.0
                vx, vy = -v * np.cos(a) * s, -v * np.sin(a) * s
                a = a + (np.pi if side > 0 else 0.0)
            obs[b, j] = (1.0, px, py, vx, vy, a, np.sin(a), np.cos(a))
    return obs
