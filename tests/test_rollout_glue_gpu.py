"""mpc_rollout_record and mpc_rollout_finish launched directly on device tensors, over the case lists of
tests/rollout_glue_cases.py (the host build runs the same lists in tests/test_rollout_glue_cases_cpu.py): what exists only in the
__global__ wrappers of csrc/mpc_engine.hip - the "last workgroup to finish" ticket that advances the buffer position, the
atomics on the counters, the `inside` predicate read from device memory, the 256-thread stride over T, the LDS split and the two
barriers around the serial scan - against RolloutBuffer on the CPU.  The record is copies and the finish is float32 operation by
operation in torch's order, so every comparison is of bit patterns; every array a kernel writes lies between guard margins."""
import ctypes

import pytest

import rollout_glue_cases as rc

pytestmark = pytest.mark.gpu


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev():
    import torch
    return torch.device("cuda", 0)


def _lib():
    from mpc_rl_for_avs_amd import engine
    return engine.load_library()


def _stream(dev):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _record(case, st, inp, step_counter=True):
    """one mpc_rollout_record launch on the current stream; no synchronisation"""
    B, A, keep, T = case
    dev = st["row"].device
    lib = _lib()
    r = lib.mpc_rollout_record(
        dev.index, T, B, A, rc.cols_of(A, keep), keep, _p(st["row"]), _p(st["mpc_actions"]), _p(st["pos"]), _p(st["ticket"]),
        _p(st["last_obs"]), _p(st["last_starts"]), _p(inp["actions"]), _p(inp["values"]), _p(inp["log_probs"]), _p(inp["mpc_act"]),
        _p(inp["mpc_status"]), _p(inp["new_obs"]), _p(inp["reward"]), _p(inp["done"]), _p(inp["terminal_obs"]) if keep else None,
        _p(inp["truncated"]) if keep else None, _p(inp["crashed"]), _p(inp["arrived"]), _p(st["counts"]), _p(st["dones_out"]),
        _p(st["step_counter"]) if step_counter else None, _stream(dev))
    assert r == 0, lib.mpc_last_error()


def _finish(case, st, gamma, lam):
    T, B, A, mode = case
    dev = st["row"].device
    lib = _lib()
    r = lib.mpc_rollout_finish(dev.index, T, B, A, st["row"].shape[2], st["keep"], _p(st["row"]), _p(st["last_values"]),
                               _p(st["dones"]), _p(st["terminal_values"]), gamma, lam, _p(st["advantages"]), _p(st["returns"]),
                               _stream(dev))
    assert r == 0, lib.mpc_last_error()


def _records_back_to_back(case, st, steps, step_counter=True, plant=True):
    """`steps` launches on one stream with no host synchronisation in between (every input is on the device before the first)"""
    import torch
    dev = st["row"].device
    inputs = [rc.record_inputs(case, s, dev, plant=plant) for s in range(steps)]
    torch.cuda.synchronize(dev)
    for inp in inputs:
        _record(case, st, inp, step_counter)
    torch.cuda.synchronize(dev)


@pytest.mark.parametrize("case", rc.RECORD_CASES, ids=rc.record_id)
def test_record_kernel_writes_the_torch_row_bit_for_bit(case):
    """T launches and two past the end of the buffer: rows and MPC actions as bit patterns (the two refused steps changed
    neither), the carry-over of the final launch (it happens when the row is refused too), position T + 2, ticket back at 0, the
    step counter advanced by T + 2, the exact episode counts over all T + 2 steps, two refusals, every guard intact."""
    steps = case[3] + rc.PAST_END
    st, intact = rc.record_state(case, _dev())
    _records_back_to_back(case, st, steps)
    want = rc.record_reference(case, steps)
    assert want["counts"][4] == rc.PAST_END and want["pos"] == steps
    rc.check_record(st, intact, want)


def test_record_kernel_from_a_negative_position():
    """position preset to -1: refused, counted, the position advances to 0 and the next launch writes row 0"""
    case = (3, 3, 1, 4)
    st, intact = rc.record_state(case, _dev(), pos0=-1)
    _records_back_to_back(case, st, 3)
    want = rc.record_reference(case, 3, pos0=-1)
    assert want["counts"][4] == 1 and want["pos"] == 2 and want["row"][:2].abs().nan_to_num().sum() > 0
    rc.check_record(st, intact, want)


def test_record_kernel_without_a_step_counter():
    case = (257, 3, 1, 4)
    steps = case[3] + rc.PAST_END
    st, intact = rc.record_state(case, _dev())
    _records_back_to_back(case, st, steps, step_counter=False)
    rc.check_record(st, intact, rc.record_reference(case, steps), step_counter=False)


def test_record_kernel_replayed_as_a_graph_equals_eager_launches():
    """The single record launch captured on a side stream (one kernel node, no parallel branches) after two warm-up launches
    whose effects are undone, replayed T + 1 times with its inputs refreshed in place: buffer, carry-over, counters and position
    bit-identical to T + 1 eager launches on the same inputs (and so to the torch reference)."""
    import torch
    case = rc.GRAPH_CASE
    steps = case[3] + 1
    dev = _dev()
    eager, eager_intact = rc.record_state(case, dev)
    _records_back_to_back(case, eager, steps)

    st, intact = rc.record_state(case, dev)
    fresh = {k: v.clone() for k, v in st.items()}
    static = rc.record_inputs(case, 0, dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):
            _record(case, st, static)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        _record(case, st, static)
    torch.cuda.synchronize(dev)
    for k, v in fresh.items():                       # position, ticket, counters, buffer, carry-over: as before the warm-up
        st[k].copy_(v)
    for s in range(steps):
        for k, v in rc.record_inputs(case, s, dev).items():
            static[k].copy_(v)
        g.replay()
    torch.cuda.synchronize(dev)
    for k in rc.RECORD_STATE + ("pos", "ticket", "step_counter"):
        assert rc.same_bits(st[k], eager[k]), k
    rc.check_record(st, intact, rc.record_reference(case, steps))
    for name, f in eager_intact.items():
        f(name)


@pytest.mark.parametrize("case", rc.FINISH_CASES, ids=rc.finish_id)
def test_finish_kernel_is_the_torch_gae_bit_for_bit(case):
    """row (only the reward column changes, and only with the bootstrap on), advantages and returns equal to
    bootstrap_truncated + compute_returns_and_advantage on the CPU for four (gamma, lambda) pairs; guards intact."""
    import torch
    st, intact = rc.finish_state(case, _dev())
    for gamma, lam in rc.GAMMA_LAMBDA:
        st["row"].copy_(st["row0"])
        st["advantages"].zero_()
        st["returns"].zero_()
        _finish(case, st, gamma, lam)
        torch.cuda.synchronize()
        rc.check_finish(case, gamma, st, intact, rc.finish_reference(case, gamma, lam))


@pytest.mark.parametrize("case", rc.NONFINITE_CASES, ids=rc.finish_id)
def test_a_non_finite_value_stays_in_its_environment(case):
    """(T, B, A) = (300, 6, 2): an infinite reward in environment 0, a NaN value in 1, rewards that overflow in the recurrence
    in 2 - equal to the reference with NaNs at equal positions, environments 3 ... 5 finite and bit-identical.  (The three pairs
    with gamma > 0: with gamma = 0 the recurrence adds nothing up and environment 2 would stay finite.)"""
    import torch
    st, intact = rc.finish_state(case, _dev(), nonfinite=True)
    for gamma, lam in rc.GAMMA_LAMBDA[:3]:
        st["row"].copy_(st["row0"])
        _finish(case, st, gamma, lam)
        torch.cuda.synchronize()
        rc.check_nonfinite(st, intact, rc.finish_reference(case, gamma, lam, True))


def test_record_then_finish_is_add_then_gae():
    """T record launches, then one finish on the buffer and the dones they left, against add x T + bootstrap + GAE on the CPU:
    a disagreement of the two kernels about the row layout, which each could pass alone, shows here."""
    import torch
    want_rec, want = rc.coupled_reference()
    case = rc.COUPLED_CASE
    B, A, keep, T = case
    st, intact = rc.record_state(case, _dev())
    _records_back_to_back(case, st, T, plant=False)
    rc.check_record(st, intact, want_rec)
    fin = rc.coupled_finish_state(st, _dev())
    _finish((T, B, A, "bootstrap"), fin, *rc.GAMMA_LAMBDA[0])
    torch.cuda.synchronize()
    assert torch.equal(st["row"].cpu(), want["row"]) and not torch.equal(want["row"], want_rec["row"])
    assert torch.equal(fin["advantages"].cpu(), want["advantages"]) and torch.equal(fin["returns"].cpu(), want["returns"])
    for name, f in list(intact.items()) + list(fin["intact"].items()):
        f(name)
