"""The warm start of the solve kernel's source, host build, against the warm-started oracle at every horizon the GPU matrix
uses (test_warm_start_gpu.py), and the two conditions on the shared inputs that give those tests their power: warm and cold
starts take different iteration counts on a large share of instances, and the oracle's own iteration count hardly moves
when the ego state moves by one unit in the last place (warm_cases.SENSITIVITY, from which the equal-iteration bar follows)."""
import numpy as np
import pytest

import warm_cases as wc


@pytest.fixture(scope="module", autouse=True)
def _clear_cases():
    yield
    wc.clear_cases()


@pytest.mark.parametrize("N", wc.CPU_N)
@pytest.mark.parametrize("cc", [False, True])
def test_host_build_warm_start_matches_oracle(cpu_wave, oracle, ref_table, cc, N):
    B = wc.batch_of(N)
    inp, u_init, cold, want = wc.warm_case(oracle, ref_table, N, cc, B)
    # the mix is what it says: clamped rows outside the bounds, NaN rows, and the strides do not collide
    assert np.isnan(u_init[wc.NAN_ROWS]).all() and np.isfinite(np.delete(u_init, np.s_[5::24], axis=0)).all()
    assert (np.abs(u_init[2::12]) > wc.U_HI).any()
    # conditions on the inputs
    share = wc.warm_changes_iterations(cold, want, N)
    if N < 63:                                   # (a certificate of 400+ active bounds takes seconds per instance)
        wc.oracle_certifies(ref_table, inp, cc, N, want)
    s = wc.sensitivity(oracle, ref_table, inp, cc, N, u_init, want)
    assert s <= wc.SENSITIVITY[(N, cc, B)] + 1e-12, (s, wc.SENSITIVITY[(N, cc, B)])
    # the host build of mpc_wave.hpp from the same initial controls
    got = cpu_wave(ref_table, dict(inp, others=inp.get("others") if cc else None), N=N, collision_cost=cc, max_iter=100,
                   u_init=u_init)
    m = wc.warm_gates(oracle, ref_table, inp, u_init, cc, N, got, want, fractions=B == 256)
    print(f"[warm host] cc={cc} N={N} B={B}: warm != cold iters {share:.3f}, s {s:.4f}, {m}")


@pytest.mark.parametrize("N", [63, 64])
@pytest.mark.parametrize("cc", [False, True])
def test_long_horizon_inputs_of_the_gpu_matrix(oracle, ref_table, cc, N):
    """The GPU matrix runs N = 63 and 64 at B = 256, the host build above at 96: both conditions for those inputs too (the
    oracle alone; the GPU matrix's equal-iteration bar at these horizons follows from THIS sensitivity, that of its own
    inputs)."""
    inp, u_init, cold, want = wc.warm_case(oracle, ref_table, N, cc, 256)
    wc.warm_changes_iterations(cold, want, N)
    s = wc.sensitivity(oracle, ref_table, inp, cc, N, u_init, want)
    assert s <= wc.SENSITIVITY[(N, cc, 256)] + 1e-12, (s, wc.SENSITIVITY[(N, cc, 256)])


def test_memory_model_follows_the_rules():
    """WarmMemory on its own: cold at first, every row's controls recorded, valid only where solved, forgotten by resets,
    kept by environments a shorter step does not reach, advanced with the last stage repeated."""
    N = 3
    mem = wc.WarmMemory(N)
    mem.reach(4)
    assert not mem.valid.any()
    U = np.arange(4 * N * 2, dtype=float).reshape(4, N, 2)
    mem.record(U, np.array([0, 1, 5, 3], np.int32))
    assert mem.valid.tolist() == [True, False, True, False] and np.array_equal(mem.U_prev, U)
    assert np.array_equal(mem.u_init(np.array([2])), U[2:3][:, [1, 2, 2]])
    mem.record(U[:2] + 100.0, np.array([2, 6], np.int32))               # a shorter step: rows 2, 3 untouched
    assert mem.valid.tolist() == [False, True, True, False] and np.array_equal(mem.U_prev[2:], U[2:])
    mem.forget(np.array([1]))
    assert mem.valid.tolist() == [False, False, True, False]
    mem.reach(6)                                                        # growth: old rows kept, new ones cold
    assert mem.valid.tolist() == [False, False, True, False, False, False] and np.array_equal(mem.U_prev[2], U[2])
    mem.forget()
    assert not mem.valid.any()
