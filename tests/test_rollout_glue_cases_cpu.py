"""The case lists of tests/rollout_glue_cases.py through the HOST build of csrc/mpc_rollout_glue.hpp (glue_host.load():
glue_rollout_record, glue_rollout_finish) against the torch references: pins the case generator, the references and the guard
before tests/test_rollout_glue_gpu.py runs the same lists through the device entry points."""
import ctypes

import pytest
import torch

import glue_host
import rollout_glue_cases as rc


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _record(case, st, inp, step_counter=True):
    B, A, keep, T = case
    r = glue_host.load().glue_rollout_record(
        T, B, A, rc.cols_of(A, keep), keep, _p(st["row"]), _p(st["mpc_actions"]), _p(st["pos"]), _p(st["last_obs"]),
        _p(st["last_starts"]), _p(inp["actions"]), _p(inp["values"]), _p(inp["log_probs"]), _p(inp["mpc_act"]),
        _p(inp["mpc_status"]), _p(inp["new_obs"]), _p(inp["reward"]), _p(inp["done"]), _p(inp["terminal_obs"]) if keep else None,
        _p(inp["truncated"]) if keep else None, _p(inp["crashed"]), _p(inp["arrived"]), _p(st["counts"]), _p(st["dones_out"]),
        _p(st["step_counter"]) if step_counter else None)
    assert r == 0


def _finish(case, st, gamma, lam):
    T, B, A, mode = case
    r = glue_host.load().glue_rollout_finish(T, B, A, st["row"].shape[2], st["keep"], _p(st["row"]), _p(st["last_values"]),
                                             _p(st["dones"]), _p(st["terminal_values"]), gamma, lam, _p(st["advantages"]),
                                             _p(st["returns"]))
    assert r == 0


def test_the_guard_sees_a_write_on_either_side():
    v, intact = rc.guarded((3, 5, 7), torch.float32, "cpu")
    assert v.shape == (3, 5, 7) and v.data_ptr() % 16 == 0 and not v.any()
    v.fill_(1.0)
    intact()
    flat = torch.as_strided(v, (1,), (1,), v.storage_offset() - 4)           # one element in front, as float32
    flat.fill_(1.0)
    with pytest.raises(AssertionError, match="in front"):
        intact()
    flat.view(torch.uint8).fill_(rc.SENTINEL)
    intact()
    torch.as_strided(v, (1,), (1,), v.storage_offset() + v.numel()).fill_(0.0)
    with pytest.raises(AssertionError, match="behind"):
        intact()
    small, _ = rc.guarded((5,), torch.int64, "cpu")                          # a margin is never shorter than 256 elements
    assert small.untyped_storage().nbytes() >= (256 + 5 + 256) * 8


def test_every_record_step_plants_the_special_values_and_both_kinds_of_status():
    for case in rc.RECORD_CASES:
        seen = set()
        for step in range(case[3] + rc.PAST_END):
            inp = rc.record_inputs(case, step)
            again = rc.record_inputs(case, step)
            assert all(rc.same_bits(inp[k], again[k]) for k in inp)          # deterministic per (case, step)
            f32 = torch.cat([inp[k].reshape(-1) for k in ("actions", "values", "log_probs", "new_obs", "reward", "terminal_obs")])
            for x in (f32, inp["mpc_act"].reshape(-1)):
                assert torch.isnan(x).any() and ((x == 0) & torch.signbit(x)).any()
            assert (f32 == float("inf")).any() and (f32 == float("-inf")).any()
            assert not (inp["crashed"] & ~inp["done"]).any() and not (inp["arrived"] & ~inp["done"]).any()
            seen |= set(rc.solved(inp["mpc_status"]).tolist())
        assert seen == {True, False} or case[0] == 1


@pytest.mark.parametrize("case", rc.RECORD_CASES, ids=rc.record_id)
def test_record_code_writes_the_torch_row_bit_for_bit(case):
    """T steps and two past the end of the buffer through record_thread on the host: buffer, carry-over, counters, position as
    the torch statement has them, the guards intact."""
    steps = case[3] + rc.PAST_END
    st, intact = rc.record_state(case, "cpu")
    for s in range(steps):
        _record(case, st, rc.record_inputs(case, s))
    want = rc.record_reference(case, steps)
    assert want["counts"][4] == rc.PAST_END and want["pos"] == steps
    rc.check_record(st, intact, want)


def test_record_code_from_a_negative_position_and_without_a_step_counter():
    case = (3, 3, 1, 4)
    st, intact = rc.record_state(case, "cpu", pos0=-1)
    for s in range(3):
        _record(case, st, rc.record_inputs(case, s))
    want = rc.record_reference(case, 3, pos0=-1)                              # refused, counted; the next launch writes row 0
    assert want["counts"][4] == 1 and want["pos"] == 2 and want["row"][:2].abs().nan_to_num().sum() > 0
    rc.check_record(st, intact, want)
    st, intact = rc.record_state(case, "cpu")
    for s in range(6):
        _record(case, st, rc.record_inputs(case, s), step_counter=False)
    rc.check_record(st, intact, rc.record_reference(case, 6), step_counter=False)


@pytest.mark.parametrize("case", rc.FINISH_CASES, ids=rc.finish_id)
def test_finish_code_is_the_torch_gae_bit_for_bit(case):
    st, intact = rc.finish_state(case, "cpu")
    for gamma, lam in rc.GAMMA_LAMBDA:
        st["row"].copy_(st["row0"])
        st["advantages"].zero_()
        st["returns"].zero_()
        _finish(case, st, gamma, lam)
        rc.check_finish(case, gamma, st, intact, rc.finish_reference(case, gamma, lam))


@pytest.mark.parametrize("case", rc.NONFINITE_CASES, ids=rc.finish_id)
def test_a_non_finite_value_stays_in_its_environment_on_the_host(case):
    st, intact = rc.finish_state(case, "cpu", nonfinite=True)
    for gamma, lam in rc.GAMMA_LAMBDA[:3]:
        st["row"].copy_(st["row0"])
        _finish(case, st, gamma, lam)
        rc.check_nonfinite(st, intact, rc.finish_reference(case, gamma, lam, True))


def test_record_then_finish_code_is_add_then_gae():
    want_rec, want = rc.coupled_reference()
    case = rc.COUPLED_CASE
    B, A, keep, T = case
    st, intact = rc.record_state(case, "cpu")
    for s in range(T):
        _record(case, st, rc.record_inputs(case, s, plant=False))
    rc.check_record(st, intact, want_rec)
    fin = rc.coupled_finish_state(st, "cpu")
    _finish((T, B, A, "bootstrap"), fin, *rc.GAMMA_LAMBDA[0])
    assert torch.equal(st["row"], want["row"]) and not torch.equal(want["row"], want_rec["row"])
    assert torch.equal(fin["advantages"], want["advantages"]) and torch.equal(fin["returns"], want["returns"])
    for name, f in list(intact.items()) + list(fin["intact"].items()):
        f(name)
