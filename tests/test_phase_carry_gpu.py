"""The phase carry of the latency builds on the device.  dispatch_solve (csrc/mpc_engine.hip) launches the latency build of a
fixed horizon - the only builds with CTX::kCarry - for a batch of up to four waves per SIMD, and the throughput build, which
forms every value where it is used, with MPC_FLAG_THROUGHPUT.  Same inputs through both, with the criteria of
test_parity_gpu.py::test_both_builds_of_the_solve_kernel_agree: statuses equal on >= 99.8 % of the instances, actions equal to
1e-6 on >= 99.9 % of those both call solved, which are at least 80 % of the batch.  Then the latency build against the host
emulation of the same switch (tests/cpu_wave_carry_harness.cpp): the same statuses and iteration counts, the actions to the
1e-4 of the kernel-against-host comparisons of test_parity_gpu.py."""
import numpy as np
import pytest

from conftest import converged, rel_u0_err
from test_phase_carry_cpu import host_solve, load_carry_lib

pytestmark = pytest.mark.gpu

TOL = 1e-4      # test_parity_gpu.TOL


@pytest.fixture(scope="module")
def engines():
    from mpc_rl_for_avs_amd import engine
    made = {}

    def get(N):
        if N not in made:
            made[N] = engine.MPCEngine(horizon=N, max_iter=100)
        return made[N]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def inputs():
    from mpc_rl_for_avs_amd import synth
    made = {}

    def get(N, V):
        if (N, V) not in made:
            made[(N, V)] = synth.solver_inputs(130, V, seed=21, N=N)
        return made[(N, V)]
    return get


def _device(e, inp, B, cc, V, throughput):
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a[:B]), dtype=dt, device=dev)
    o = e.solve_batch_torch(state=t(inp["state"], torch.float64), ego_index=t(inp["ego_index"], torch.int32),
                            weights=t(inp["weights"], torch.float64), is_collide=t(inp["is_collide"], torch.uint8),
                            vref=t(inp["vref"], torch.float64), others=t(inp["others"], torch.float64) if V > 0 else None,
                            collision_cost=cc, sync=True, throughput=throughput)
    return {k: v.cpu().numpy() for k, v in o.items()}


@pytest.mark.parametrize("B", [64, 130])
@pytest.mark.parametrize("V", [0, 1, 8])
@pytest.mark.parametrize("N", [20, 16])
@pytest.mark.parametrize("cc", [True, False])
def test_latency_build_against_throughput_build(engines, inputs, cc, N, V, B):
    a = _device(engines(N), inputs(N, V), B, cc, V, False)
    b = _device(engines(N), inputs(N, V), B, cc, V, True)
    same = a["status"] == b["status"]
    print("statuses equal on", same.mean())
    assert same.mean() >= 0.998, np.nonzero(~same)[0]
    ok = same & converged(a["status"])
    assert ok.sum() >= 0.8 * len(same)          # the comparison below is not empty
    err = rel_u0_err(a["u0"], b["u0"])[ok]
    print("largest action difference", err.max(), "iterations up to", a["iters"].max())
    assert (err <= 1e-6).mean() >= 0.999, err.max()


def test_latency_build_against_the_host_emulation(engines, inputs, ref_table):
    """The 64 instances of the comparison above (horizon 20, eight vehicles, collision cost on) on the device and in the host
    build with CTX::kCarry."""
    inp = {k: (v[:64] if isinstance(v, np.ndarray) else v) for k, v in inputs(20, 8).items()}
    got = _device(engines(20), inp, 64, True, 8, False)
    want = host_solve(load_carry_lib().wave_solve_batch_carry, ref_table, inp, True)
    err = rel_u0_err(got["u0"], want["u0"])
    solved = converged(want["status"])
    print("status differs at", np.nonzero(got["status"] != want["status"])[0], "iterations differ at",
          np.nonzero(got["iters"] != want["iters"])[0], "largest action difference (solved)", err[solved].max(),
          "solved", int(solved.sum()), "iterations up to", want["iters"].max())
    assert np.array_equal(got["status"], want["status"])
    assert np.array_equal(got["iters"], want["iters"])
    print("largest action difference (all)", err.max())
    assert solved.sum() >= 0.8 * 64 and (err <= TOL).all()
