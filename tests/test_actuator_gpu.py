"""The actuator model of the closed-loop evaluation on the GPU: the mpc_actuate kernel against its host build on the command
streams of tests/test_actuator_cpu.py (applied, the state, age, ctr, the counts and the sums, bit for bit), the library's
refusals, the captured evaluation step against the eager one, and the default actuator against an evaluation without one."""
import ctypes

import numpy as np
import pytest

from test_actuator_cpu import PARAMS, assert_runs_equal, command_stream, run_class, run_host
from test_evaluate_cpu import CFG, Env

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda", 0)


@pytest.mark.parametrize("delay", [0, 1, 7])
@pytest.mark.parametrize("B", [1, 31, 32, 33, 97])           # one lane pair; either side of a full wave; a ragged fourth wave
def test_kernel_is_the_host_build_bit_for_bit(B, delay):
    import torch
    kw = dict(PARAMS["all"], delay=delay)                     # every feature on; the stream has a reset launch in the middle
    steps = command_stream(B, seed=100 + B)
    got = run_class(steps, B, kw, device=_dev(), backend="hip")
    torch.cuda.synchronize(_dev())
    assert_runs_equal(got, run_host(steps, B, kw), "kernel vs host build")


@pytest.mark.parametrize("name", ["off", "all"])
def test_kernel_with_applied_aliasing_command_is_the_host_build(name):
    B = 97
    steps = command_stream(B, seed=100 + B)
    got = run_class(steps, B, PARAMS[name], device=_dev(), backend="hip", alias=True)
    assert_runs_equal(got, run_host(steps, B, PARAMS[name]), "kernel, aliased, vs host build")


def test_kernel_refuses_invalid_arguments():
    import torch
    from mpc_rl_for_avs_amd import engine
    lib = engine.load_library()
    dev = _dev()
    B = 4
    z = lambda *sh, dt: torch.zeros(sh, dtype=dt, device=dev)
    cmd, out, done = z(B, 2, dt=torch.float64), z(B, 2, dt=torch.float64), z(B, dt=torch.uint8)
    state, sums = z(10, B, 2, dt=torch.float64), z(2, B, 2, dt=torch.float64)
    age, ctr, counts = z(B, dt=torch.int32), z(B, dt=torch.int64), z(5, B, dt=torch.int64)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    inf, nan = float("inf"), float("nan")
    pair = lambda v: (ctypes.c_double * 2)(*v)

    def call(B=B, reset=0, cmd=cmd, done=done, out=out, state=state, age=age, ctr=ctr, counts=counts, sums=sums, params=True,
             size=None, **q):
        q = dict(dict(delay=0, dt=0.1, p_hold=0.0, gain=(1, 1), offset=(0, 0), sigma=(0, 0), alpha=(1, 1), rate=(inf, inf),
                      lo=(-inf, -inf), hi=(inf, inf), seed=0, env_offset=0), **q)
        par = engine.ActuatorParams(struct_size=ctypes.sizeof(engine.ActuatorParams) if size is None else size, reserved=0,
                                    **{k: pair(v) if isinstance(v, tuple) else v for k, v in q.items()})
        return lib.mpc_actuate(0, B, reset, ctypes.byref(par) if params else None, p(cmd), p(done), p(out), p(state), p(age),
                               p(ctr), p(counts), p(sums), stream)

    assert call(reset=1, cmd=None, done=None, out=None) == 0 and call() == 0
    assert call(B=0) == 0 and call(done=None) == 0 and call(out=cmd) == 0                # applied may be command
    assert call(delay=7, p_hold=1.0, alpha=(1e-6, 1.0), rate=(1e-9, inf), lo=(0.0, -inf), hi=(0.0, inf)) == 0
    for kw, word in ((dict(B=-1), b"B"), (dict(delay=-1), b"delay"), (dict(delay=8), b"delay"), (dict(dt=0.0), b"dt"),
                     (dict(dt=nan), b"dt"), (dict(p_hold=-0.1), b"p_hold"), (dict(p_hold=1.5), b"p_hold"),
                     (dict(p_hold=nan), b"p_hold"), (dict(gain=(nan, 1.0)), b"gain"), (dict(offset=(0.0, inf)), b"offset"),
                     (dict(sigma=(-1.0, 0.0)), b"sigma"), (dict(sigma=(0.0, nan)), b"sigma"), (dict(alpha=(0.0, 1.0)), b"alpha"),
                     (dict(alpha=(1.0, 1.5)), b"alpha"), (dict(alpha=(nan, 1.0)), b"alpha"), (dict(rate=(0.0, 1.0)), b"rate"),
                     (dict(rate=(1.0, nan)), b"rate"), (dict(lo=(1.0, 0.0), hi=(0.0, 1.0)), b"lo"), (dict(lo=(nan, 0.0)), b"lo"),
                     (dict(hi=(0.0, nan)), b"hi"), (dict(params=False), b"params"), (dict(size=8), b"struct_size"),
                     (dict(cmd=None), b"command"), (dict(out=None), b"applied"), (dict(state=None), b"state_f64"),
                     (dict(age=None), b"age"), (dict(ctr=None), b"ctr"), (dict(counts=None), b"counts"), (dict(sums=None), b"sums"),
                     (dict(reset=1, state=None), b"state_f64")):
        assert call(**kw) == -1, kw                                # MPC_ERR_INVALID_ARG
        text = lib.mpc_last_error()
        assert b"mpc_actuate" in text and word in text, (kw, text)
    torch.cuda.synchronize(dev)
    assert counts[0].cpu().tolist() == [4] * B                     # the four launches after the reset; a refused call launches nothing
    assert call() == 0
    torch.cuda.synchronize(dev)
    assert counts[0].cpu().tolist() == [5] * B and ctr.cpu().tolist() == [5] * B


def _pure():
    from mpc_rl_for_avs_amd.engine import MPCEngine
    from mpc_rl_for_avs_amd.pure_mpc import PureMPC_Agent
    return PureMPC_Agent(Env(), dict(CFG), engine=MPCEngine(horizon=20, device=0), collision_cost=False)


def _eval(agent, B, **kw):
    from mpc_rl_for_avs_amd import evaluate, rollout
    env = rollout.SyntheticIntersectionEnv(B, device=_dev(), seed=7, n_others=4, traffic="idm")
    return evaluate.evaluate_agent(agent, env, episodes_per_env=1, seed=7, metrics=True, **kw)


def _assert_same(a, b):
    assert set(a) == set(b)
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), k


def _assert_same_totals(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


@pytest.fixture(scope="module")
def agent():
    return _pure()


@pytest.fixture(scope="module")
def plain(agent):
    return _eval(agent, 64, use_graph=True)


def test_graph_and_eager_evaluations_are_bit_identical(agent, plain):
    kw = dict(actuation=dict(delay=1, tau=(0.1, 0.2)))
    g = _eval(agent, 64, use_graph=True, **kw)
    e = _eval(agent, 64, use_graph=False, **kw)
    _assert_same(g.records, e.records)
    _assert_same(g.drive, e.drive)
    _assert_same_totals(g.actuation, e.actuation)
    t = g.actuation
    print("actuation totals:", t)
    assert g.steps == e.steps and t["steps"] == g.env_steps and t["mean_abs_dev"].min() > 0 and t["held"] == t["nonfinite"] == 0
    again = _eval(agent, 64, use_graph=True, **kw)                 # the same seed twice: the same bytes
    _assert_same(g.records, again.records)
    _assert_same(g.drive, again.drive)
    _assert_same_totals(g.actuation, again.actuation)
    assert g.records["return"].tobytes() != plain.records["return"].tobytes()            # and the model acted


def test_the_default_actuation_is_the_evaluation_without_one(agent, plain):
    res = _eval(agent, 64, use_graph=True, actuation=dict())
    _assert_same(res.records, plain.records)
    _assert_same(res.drive, plain.drive)
    t = res.actuation
    assert res.steps == plain.steps and plain.actuation is None and t["steps"] == res.env_steps
    assert t["held"] == t["rate_limited"] == t["saturated"] == t["nonfinite"] == 0 and not t["max_abs_dev"].any()
