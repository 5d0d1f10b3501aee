"""The solve kernel's source, host build, iterate by iterate against the oracle: both sides stopped at the iteration caps
0, 1, 2, 3, 5, 8, 13 and compared on EVERY instance of a batch of 256 (iterate_cases.check_capped) - status and iteration
count equal, the controls within 256 x the oracle's own worst response to a last-place move of the ego states.  No fraction
gates: an answer that stops at the cap is compared like any other, a wrong step shows at the cap behind it, and one
instance is enough to fail.  Horizons on both sides of every path of the solver (N = 1, 2; the compiled 16 and 20; 31 - 33
around the line search's split; 63 and 64 where lane 0 holds two nodes), collision cost off and on; the warm start; a batch
with an infeasible start; the progress guard.  test_iterates_gpu.py runs the same checks on every device build.

What the ladder found when it was written: instance 85 of the N = 64 collision-cost case left the oracle's path in the
FIRST iteration.  The sweep's value function Pxx lost its symmetry to rounding, A'Pxx A handed the antisymmetric part on
from stage to stage (the gains of stage 0 off by 2e-5 relative), and the iterate was 2.8e-4 from the oracle's at cap 8,
4262 x the worst spread, on a path that later rejoined the oracle's.  The oracle symmetrises Pxx at every stage; above the
compiled horizons (from 21 stages) sweep4 now does the same, and the instance is at 6.3e-8 (profiles/iterate_ladder.txt).
No instance is excluded from any bar."""
import numpy as np
import pytest

import iterate_cases as ic

CPU_N = (1, 2, 16, 20, 31, 32, 33, 63, 64)
WARM_N = 20


@pytest.fixture(scope="module", autouse=True)
def _clear_cases():
    yield
    ic.clear_cases()


def _host(cpu_wave, ref_table, c, cap):
    inp, u_init = ic.case_inputs(c)
    return cpu_wave(ref_table, inp, N=c.N, collision_cost=c.cc, tol=1e-8, max_iter=cap, u_init=u_init,
                    stall_window=c.stall_window)


def _ladder_step(cpu_wave, oracle, ref_table, c, cap):
    inp, _ = ic.case_inputs(c)
    want = ic.oracle_ladder(oracle, ref_table, c, cap)
    worst, _ = ic.oracle_spread(oracle, ref_table, c, cap)
    got = _host(cpu_wave, ref_table, c, cap)
    dU = np.abs(got["U"] - want["U"])[want["status"] != 3]
    print(ic.line(c, "host", cap, float(dU.max()) if dU.size else 0.0, worst))
    ic.check_capped(got, want, inp["state"], cap, ic.bar(oracle, ref_table, c, cap))
    return got, want


@pytest.mark.parametrize("cap", ic.CAPS)
@pytest.mark.parametrize("N", CPU_N)
@pytest.mark.parametrize("cc", [False, True])
def test_host_build_iterates_match_oracle(cpu_wave, oracle, ref_table, cc, N, cap):
    _ladder_step(cpu_wave, oracle, ref_table, ic.case(N, cc), cap)


@pytest.mark.parametrize("cap", ic.CAPS)
@pytest.mark.parametrize("cc", [False, True])
def test_host_build_warm_iterates_match_oracle(cpu_wave, oracle, ref_table, cc, cap):
    """Started from controls uniform in +-(6, 1.2): clamped on both sides, so cap 0 returns the clamped controls, bit for
    bit; a start whose rollout leaves the state bounds falls back to the cold one on both sides."""
    c = ic.case(WARM_N, cc, warm=True)
    got, _ = _ladder_step(cpu_wave, oracle, ref_table, c, cap)
    _, u_init = ic.case_inputs(c)
    if cap == 0:
        m = 1e-3 * 2.0 * ic.U_HI                                              # 0.1 % of the range inside the bounds
        clamped = np.clip(u_init, -ic.U_HI + m, ic.U_HI - m)
        kept = (np.abs(got["U"] - clamped) <= 1e-15).reshape(c.B, -1).all(axis=1)
        cold = (got["U"][:, 1:] == 0.0).reshape(c.B, -1).all(axis=1)          # (a_0 may be the standing vehicle's push)
        assert (kept | cold).all() and kept.mean() >= 0.5, (kept.mean(), cold.mean())


@pytest.mark.parametrize("cap", ic.CAPS)
def test_infeasible_start_inside_a_batch(cpu_wave, oracle, ref_table, cap):
    """One instance of the batch starts with its speed outside the bounds: status 3 and no iteration on both sides at every
    cap, its U and X as the oracle leaves them (check_capped), its neighbours untouched by it."""
    c = ic.case(20, True, infeasible=True)
    got, want = _ladder_step(cpu_wave, oracle, ref_table, c, cap)
    assert want["status"][ic.BAD_ROW] == 3 and got["iters"][ic.BAD_ROW] == 0
    assert (want["status"] == 3).sum() == 1
    plain = ic.oracle_ladder(oracle, ref_table, ic.case(20, True), cap)
    rest = np.arange(c.B) != ic.BAD_ROW
    assert ic.bits_equal(want["U"][rest], plain["U"][rest])


@pytest.mark.parametrize("cap", ic.CAPS)
def test_stall_window_inside_the_ladder(cpu_wave, oracle, ref_table, cap):
    """mpc_config.stall_window = 4 on both sides: an instance whose KKT error has not halved within four iterations ends with
    status 4 at the same iteration as in the oracle.  At cap 13 the guard has fired on a share of the batch, at caps up to 3
    it cannot have."""
    c = ic.case(20, True, stall_window=4)
    _, want = _ladder_step(cpu_wave, oracle, ref_table, c, cap)
    stalled = want["status"] == 4
    if cap <= 3:
        assert not stalled.any()
    if cap == 13:
        assert stalled.sum() >= 8 and (want["iters"][stalled] < 13).any(), int(stalled.sum())
