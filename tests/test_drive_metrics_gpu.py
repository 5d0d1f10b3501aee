"""Safety and comfort metrics of the closed-loop evaluation on the GPU: the mpc_drive_metrics kernel against its host build
on the streams of tests/test_drive_metrics_cpu.py (state and records, bit for bit), its argument checks, the captured
evaluation step against the eager one, and an eager evaluation replayed by the plain-Python restatement of the metrics."""
import ctypes

import numpy as np
import pytest

import drive_metrics_host as dmh
from test_drive_metrics_cpu import DT, PLANES, assert_planes_equal, random_stream, run_host
from test_evaluate_cpu import CFG, Env

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda", 0)


@pytest.mark.parametrize("B", [1, 3, 5, 257])              # a lone environment, partial waves, more than one block
@pytest.mark.parametrize("R,M,Q", [(1, 1, 1), (10, 17, 3), (17, 128, 2), (10, 18, 1)])
def test_kernel_is_the_host_build_bit_for_bit(B, R, M, Q):
    import torch
    from mpc_rl_for_avs_amd import evaluate
    dev = _dev()
    ref, steps = random_stream(B, R, M, Q, seed=1000 * B + R)
    h = run_host(ref, steps, B, R, Q)
    d = evaluate.DriveMetrics(B, Q, dev, "hip", ref, DT, R)
    for s in steps:
        t = {k: torch.as_tensor(v).to(dev) for k, v in s.items() if k != "reset"}
        if s.get("reset"):
            d.update(None, t["obs"], None, None, reset=True)
        else:
            d.update(t["terminal_obs"], t["obs"], t["act"], t["done"])
    torch.cuda.synchronize(dev)
    assert_planes_equal({n: getattr(d, n).cpu().numpy() for n in PLANES}, h, "kernel vs host build")


def test_kernel_refuses_invalid_arguments():
    import torch
    from mpc_rl_for_avs_amd import engine
    lib = engine.load_library()
    dev = _dev()
    B, R, Q, M = 4, 10, 2, 5
    z = lambda *sh, dt: torch.zeros(sh, dtype=dt, device=dev)
    tobs, obs, act, done = z(B, R, 8, dt=torch.float32), z(B, R, 8, dt=torch.float32), z(B, 2, dt=torch.float64), z(B, dt=torch.uint8)
    ref = z(M, 2, dt=torch.float64)
    si, sf = z(5, B, dt=torch.int32), z(17, B, dt=torch.float64)
    ri, rf = z(4, B, Q, dt=torch.int32), z(10, B, Q, dt=torch.float64)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(B=B, R=R, Q=Q, M=M, reset=0, dt=0.1, tobs=tobs, obs=obs, act=act, done=done, ref=ref, si=si, sf=sf, ri=ri, rf=rf):
        return lib.mpc_drive_metrics(0, B, R, Q, M, reset, dt, p(tobs), p(obs), p(act), p(done), p(ref), p(si), p(sf), p(ri),
                                     p(rf), stream)

    assert call(reset=1) == 0 and call() == 0
    assert call(reset=1, tobs=None, act=None, done=None) == 0    # a reset launch needs obs only
    assert call(B=0) == 0
    for kw in (dict(B=-1), dict(Q=0), dict(R=0), dict(R=18), dict(M=0), dict(M=129), dict(dt=0.0), dict(dt=-0.1),
               dict(si=None), dict(sf=None), dict(ri=None), dict(rf=None), dict(obs=None), dict(ref=None),
               dict(obs=None, reset=1), dict(tobs=None), dict(act=None), dict(done=None)):
        assert call(**kw) == -1, kw                                # MPC_ERR_INVALID_ARG
        assert b"mpc_drive_metrics" in lib.mpc_last_error(), kw
    torch.cuda.synchronize(dev)


def _pure():
    from mpc_rl_for_avs_amd.engine import MPCEngine
    from mpc_rl_for_avs_amd.pure_mpc import PureMPC_Agent
    return PureMPC_Agent(Env(), dict(CFG), engine=MPCEngine(horizon=20, device=0), collision_cost=False)


def _eval(agent, B, traffic, **kw):
    from mpc_rl_for_avs_amd import evaluate, rollout
    env = rollout.SyntheticIntersectionEnv(B, device=_dev(), seed=7, n_others=4, traffic=traffic)
    return evaluate.evaluate_agent(agent, env, episodes_per_env=1, seed=7, metrics=True, **kw), env


def _assert_drive_equal(got, want):
    from mpc_rl_for_avs_amd import evaluate
    for k in evaluate.DRIVE_I32 + evaluate.DRIVE_F64:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8)), k


@pytest.mark.parametrize("traffic", ["constant", "idm"])
def test_graph_and_eager_evaluations_give_the_same_metrics(traffic):
    agent = _pure()
    g, _ = _eval(agent, 64, traffic, use_graph=True)
    e, _ = _eval(agent, 64, traffic, use_graph=False)
    _assert_drive_equal(g.drive, e.drive)
    assert np.array_equal(g.drive["steps"], g.records["steps"]) and g.steps == e.steps
    assert np.isfinite(g.drive["min_box_gap"]).any()               # the ego met traffic


@pytest.mark.parametrize("traffic", ["constant", "idm"])
def test_eager_evaluation_is_reproduced_by_the_plain_python_restatement(traffic):
    import torch
    from mpc_rl_for_avs_amd import evaluate, rollout
    B = 16
    seen = []
    take = lambda d: {k: (v.cpu().numpy().copy() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
    res, env = _eval(_pure(), B, traffic, use_graph=False, on_step=lambda d: seen.append(take(d)))
    want = dmh.replay(seen, B, 1, env.ref_xy.cpu().numpy(), env.dt, rollout.VEHICLES_COUNT)
    _assert_drive_equal(res.drive, evaluate.records_from_planes(want["rec_i32"], want["rec_f64"], evaluate.DRIVE_I32,
                                                                  evaluate.DRIVE_F64))
    assert np.array_equal(res.drive["steps"], res.records["steps"])
