"""The perception model of the closed-loop evaluation on the GPU: the mpc_perceive kernel against its host build on the streams
of tests/test_perception_cpu.py (observation, classes, counts and counter, bit for bit), its argument checks, the captured
evaluation step against the eager one, an evaluation with every parameter off against one without a perception model, and an
eager evaluation replayed by the plain-Python restatement of the model."""
import ctypes

import numpy as np
import pytest

import perception_host as ph
from test_evaluate_cpu import CFG, Env
from test_perception_cpu import ALL_ON, KEY, assert_runs_equal, random_stream, run_class, run_host

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda", 0)


@pytest.mark.parametrize("name,params", [("off", dict(KEY)), ("all", ALL_ON)])
@pytest.mark.parametrize("R,S", [(1, 0), (2, 1), (10, 4), (17, 8)])
@pytest.mark.parametrize("B", [1, 3, 5, 257])               # a lone environment, partial groups, more than one block
def test_kernel_is_the_host_build_bit_for_bit(B, R, S, name, params):
    import torch
    occ, steps = random_stream(B, R, S, seed=1000 * B + R)
    got = run_class(occ, steps, B, R, params, device=_dev(), backend="hip")
    torch.cuda.synchronize(_dev())
    assert_runs_equal(got, run_host(occ, steps, B, R, params), "kernel vs host build")


def test_kernel_refuses_invalid_arguments():
    import torch
    from mpc_rl_for_avs_amd import engine
    lib = engine.load_library()
    dev = _dev()
    B, R, S = 4, 10, 2
    z = lambda *sh, dt: torch.zeros(sh, dtype=dt, device=dev)
    true, seen, occ = z(B, R, 8, dt=torch.float32), z(B, R, 8, dt=torch.float32), z(S, 4, 2, dt=torch.float64)
    cls, counts, ctr = z(B, R, dt=torch.uint8), z(5, B, dt=torch.int64), z(B, dt=torch.int64)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    size = ctypes.sizeof(engine.PerceptionParams)
    good = dict(struct_size=size, occlusion=1, min_points=1, env_offset=0, range=float("inf"), p_drop=0.0, sigma_pos=0.0,
                sigma_vel=0.0, sigma_head=0.0, seed=1)

    def call(B=B, R=R, S=S, reset=0, params=True, true=true, occ=occ, seen=seen, cls=cls, counts=counts, ctr=ctr, **fields):
        q = engine.PerceptionParams(**dict(good, **fields))
        return lib.mpc_perceive(0, B, R, S, reset, ctypes.byref(q) if params else None, p(true), p(occ), p(seen), p(cls),
                                p(counts), p(ctr), stream)

    assert call(reset=1) == 0 and call() == 0
    assert call(B=0) == 0 and call(cls=None) == 0 and call(S=0, occ=None) == 0
    nan = float("nan")
    for kw in (dict(B=-1), dict(R=0), dict(R=18), dict(S=-1), dict(S=9), dict(occ=None), dict(params=False), dict(true=None),
               dict(seen=None), dict(counts=None), dict(ctr=None), dict(seen=true), dict(struct_size=size - 8),
               dict(struct_size=0), dict(min_points=0), dict(min_points=6), dict(p_drop=-0.01), dict(p_drop=1.01),
               dict(p_drop=nan), dict(sigma_pos=-1.0), dict(sigma_pos=nan), dict(sigma_vel=-1.0), dict(sigma_vel=nan),
               dict(sigma_head=-1.0), dict(sigma_head=nan), dict(range=nan), dict(range=0.0), dict(range=-1.0)):
        assert call(**kw) == -1, kw                                # MPC_ERR_INVALID_ARG
        assert b"mpc_perceive" in lib.mpc_last_error(), kw
    torch.cuda.synchronize(dev)
    assert ctr.cpu().tolist() == [4] * B                           # the four launches above; a refused call launches nothing
    assert call() == 0
    torch.cuda.synchronize(dev)
    assert ctr.cpu().tolist() == [5] * B


def _real():
    from mpc_rl_for_avs_amd import evaluate
    return dict(range=40.0, occlusion=True, occluders=evaluate.corner_buildings(), p_drop=0.05, sigma_pos=0.2, sigma_vel=0.3,
                sigma_head=0.02, seed=7)


def _pure():
    from mpc_rl_for_avs_amd.engine import MPCEngine
    from mpc_rl_for_avs_amd.pure_mpc import PureMPC_Agent
    return PureMPC_Agent(Env(), dict(CFG), engine=MPCEngine(horizon=20, device=0), collision_cost=False)


def _eval(agent, B, traffic, **kw):
    from mpc_rl_for_avs_amd import evaluate, rollout
    env = rollout.SyntheticIntersectionEnv(B, device=_dev(), seed=7, n_others=4, traffic=traffic)
    return evaluate.evaluate_agent(agent, env, episodes_per_env=1, seed=7, metrics=True, **kw), env


def _assert_same(a, b):
    assert set(a) == set(b)
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), k


@pytest.mark.parametrize("traffic", ["constant", "idm"])
def test_graph_and_eager_evaluations_are_bit_identical(traffic):
    agent = _pure()
    g, _ = _eval(agent, 64, traffic, use_graph=True, perception=_real())
    e, _ = _eval(agent, 64, traffic, use_graph=False, perception=_real())
    _assert_same(g.records, e.records)
    _assert_same(g.drive, e.drive)
    assert g.steps == e.steps and g.perception == e.perception
    p = g.perception
    print("perception totals:", p)
    assert p["occluded"] >= 1 and p["seen"] >= 1
    assert p["present"] == p["seen"] + p["out_of_range"] + p["occluded"] + p["dropped"]


@pytest.mark.parametrize("traffic", ["constant", "idm"])
def test_every_parameter_off_is_the_evaluation_without_perception(traffic):
    agent = _pure()
    base, _ = _eval(agent, 64, traffic)
    off, _ = _eval(agent, 64, traffic, perception={})
    _assert_same(base.records, off.records)
    _assert_same(base.drive, off.drive)
    assert base.perception is None and off.perception["present"] == off.perception["seen"] > 0


@pytest.mark.parametrize("traffic", ["constant", "idm"])
def test_eager_evaluation_is_reproduced_by_the_plain_python_restatement(traffic):
    import torch
    from mpc_rl_for_avs_amd import rollout
    B = 16
    seen = []
    take = lambda d: {k: (v.cpu().numpy().copy() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
    real = _real()
    res, env = _eval(_pure(), B, traffic, use_graph=False, perception=dict(real), on_step=lambda d: seen.append(take(d)))
    steps = [dict(obs=s["obs"], reset=bool(s.get("reset"))) for s in seen]
    kw = {k: v for k, v in real.items() if k != "occluders"}
    outs, counts, ctr = ph.replay(steps, B, rollout.VEHICLES_COUNT, real["occluders"],
                                  env_offset=int(getattr(env, "env_offset", 0)), **kw)
    for k, (s, (want_seen, want_cls)) in enumerate(zip(seen, outs)):
        assert s["seen"].tobytes() == want_seen.tobytes() and np.array_equal(s["row_class"], want_cls), k
    assert res.perception == dict(zip(ph.COUNTS, counts.sum(axis=1).tolist())) and (ctr == res.steps + 1).all()
