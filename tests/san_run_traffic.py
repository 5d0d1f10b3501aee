"""Child process of tests/test_traffic_env_cpu.py (run with libasan preloaded and MPC_TEST_SANITIZE=1), next to tests/san_run.py:
the host build of the reactive-traffic step (mpc_synth_traffic.hpp) compiled with AddressSanitizer and
UndefinedBehaviorSanitizer, for no traffic, one vehicle and the most the observation holds, resets and respawns included.
Any sanitizer report aborts the process; the parent asserts on the exit code."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle"), HERE]
assert os.environ.get("MPC_TEST_SANITIZE") == "1"

import test_traffic_env_cpu as tt  # noqa: E402

lib = tt.load_traffic_lib()
rng = np.random.default_rng(0)
ended = respawned = 0
for K in (0, 1, 9):
    he = tt.TrafficHostEnv(lib, 33, K, seed=K, spawn_probability=0.5)
    he.reset()
    for _ in range(220):
        before = he.oactive.astype(bool).copy()
        _, _, done = he.step(np.stack([rng.uniform(-6, 6, 33), rng.uniform(-0.1, 0.1, 33)], axis=1))
        ended += int(done.sum())
        respawned += int((he.oactive.astype(bool) & ~before & ~done[:, None]).sum())
assert ended >= 99 and respawned >= 10, (ended, respawned)
x, y, h = tt.host_pose(lib, np.repeat(np.arange(12, dtype=np.int32), 5), np.tile([0.0, 50.0, 60.0, 70.0, 140.0], 12))
assert np.isfinite(x).all() and np.isfinite(y).all() and np.isfinite(h).all()
print(f"sanitized traffic run ok: {ended} episodes ended, {respawned} respawns")
