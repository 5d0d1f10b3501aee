"""Closed-loop evaluation on the GPU: the mpc_episode_stats kernel against its host build on the streams of
tests/test_evaluate_cpu.py (bit for bit) and its argument checks; the captured evaluation step against the eager one; one
evaluation of 256 environments against two shards of 128; every agent kind run to completion, its records reproduced from
the eager path's per-step inputs by the plain-Python restatement of the reference's bookkeeping."""
import ctypes

import numpy as np
import pytest

import episode_stats_host as esh
import sde_host
import test_evaluate_cpu as tec
from test_evaluate_cpu import CFG, Env, _assert_records_equal, _expected_recorded, random_stream

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda", 0)


@pytest.mark.parametrize("B", [1, 63, 257])
@pytest.mark.parametrize("Q", [1, 3])
def test_kernel_is_the_host_build_bit_for_bit(B, Q):
    import torch
    from mpc_rl_for_avs_amd import evaluate, rollout
    dev = _dev()
    T = Q * rollout.EPISODE_STEPS + 60
    steps = random_stream(B, T, Q, seed=100 * B + Q, reset_at=30)
    h = esh.HostStats(B, Q)
    s = evaluate.EpisodeStats(B, Q, dev, "hip")
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    for st in steps:
        h.update(st, reset=bool(st.get("reset")))
        t = {k: torch.as_tensor(v).to(dev) for k, v in st.items() if k != "reset"}
        if st.get("reset"):
            s.update(t["ego"], reset=True, step_counter=ctr)
        else:
            s.update(**t, step_counter=ctr)
    torch.cuda.synchronize(dev)
    for name in ("state_i32", "state_f64", "rec_i32", "rec_f64", "recorded"):
        g, w = getattr(s, name).cpu().numpy(), np.ascontiguousarray(getattr(h, name))
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), name
    assert int(ctr[0]) == T
    assert int(s.recorded[0]) == _expected_recorded(steps, B, Q)
    _assert_records_equal(s.records(), esh.replay(steps, B, Q))


def test_kernel_refuses_invalid_arguments():
    import torch
    from mpc_rl_for_avs_amd import engine
    lib = engine.load_library()
    dev = _dev()
    B, Q = 4, 2
    z = lambda *sh, dt: torch.zeros(sh, dtype=dt, device=dev)
    ego, si, sf = z(B, 4, dt=torch.float64), z(5, B, dt=torch.int32), z(3, B, dt=torch.float64)
    ri, rf, rec = z(6, B, Q, dt=torch.int32), z(2, B, Q, dt=torch.float64), z(1, dt=torch.int64)
    u8, f32, i32 = z(B, dt=torch.uint8), z(B, dt=torch.float32), z(B, dt=torch.int32)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(B=B, Q=Q, reset=0, ego=ego, done=u8, recorded=rec, si=si):
        return lib.mpc_episode_stats(0, B, Q, reset, p(done), p(u8), p(u8), p(u8), p(f32), p(ego), p(i32), p(i32), p(si), p(sf),
                                     p(ri), p(rf), p(recorded), None, stream)

    assert call() == 0 and call(reset=1, done=None) == 0       # a reset launch needs no step inputs
    for kw in (dict(B=-1), dict(Q=0), dict(ego=None), dict(recorded=None), dict(si=None), dict(done=None)):
        assert call(**kw) == -1, kw                              # MPC_ERR_INVALID_ARG
        assert b"mpc_episode_stats" in lib.mpc_last_error()
    torch.cuda.synchronize(dev)


def _pure(collision_cost=True, engine=None):
    from mpc_rl_for_avs_amd.engine import MPCEngine
    from mpc_rl_for_avs_amd.pure_mpc import PureMPC_Agent
    return PureMPC_Agent(Env(), dict(CFG), engine=engine or MPCEngine(horizon=20, device=0), collision_cost=collision_cost)


def _mpcrl(name, tmp_path, engine=None):
    from mpc_rl_for_avs_amd import rollout
    from mpc_rl_for_avs_amd.engine import MPCEngine
    agent, meta = rollout.MPCRLAgent.from_sb3(sde_host.sb3_zip(tmp_path, name), engine or MPCEngine(horizon=20, device=0),
                                              device=_dev())
    return agent, meta


def _env(B, seed=7, env_offset=0):
    from mpc_rl_for_avs_amd import rollout
    return rollout.SyntheticIntersectionEnv(B, device=_dev(), seed=seed, n_others=4, env_offset=env_offset)


def _eval(agent, B, Q, seed=7, env_offset=0, **kw):
    from mpc_rl_for_avs_amd import evaluate
    return evaluate.evaluate_agent(agent, _env(B, seed, env_offset), episodes_per_env=Q, seed=seed, **kw)


def test_graph_and_eager_evaluations_record_the_same_episodes():
    agent = _pure(collision_cost=True)
    g = _eval(agent, 256, 2, use_graph=True)
    e = _eval(agent, 256, 2, use_graph=False)
    _assert_records_equal(g.records, e.records)
    assert g.steps == e.steps


def test_all_features_in_one_evaluation_graph_eager_and_single_feature_runs_agree():
    from mpc_rl_for_avs_amd import evaluate, rollout
    from episode_trace_host import same_bits
    agent = _pure(collision_cost=False)

    def run(use_graph=True, **features):
        env = rollout.SyntheticIntersectionEnv(tec.ALL_B, device=_dev(), seed=1, n_others=4, traffic="idm")
        features = {k: dict(v) if isinstance(v, dict) else v for k, v in features.items()}
        return evaluate.evaluate_agent(agent, env, episodes_per_env=tec.ALL_Q, seed=1, use_graph=use_graph,
                                       perception=tec.all_features_perception(), **features)

    g = tec.assert_features_do_not_disturb_one_another(run)          # the graph run against four single-feature graph runs
    e = run(use_graph=False, **tec.ALL_FEATURES)
    assert g.steps == e.steps <= 400 and g.traces.counts == e.traces.counts and g.perception == e.perception
    planes = lambda t: dict(t.index, scene=t.scene, seen=t.seen, action=t.action, reward=t.reward, frame_i32=t.frame_i32)
    for name, a, b in (("records", g.records, e.records), ("drive", g.drive, e.drive),
                       ("interaction", g.interaction, e.interaction), ("traces", planes(g.traces), planes(e.traces))):
        assert list(a) == list(b), name
        for k in a:
            assert same_bits(a[k], b[k]), (name, k)


def _shards(make_agent, Q=1, **kw):
    whole = _eval(make_agent(), 256, Q, **kw)
    parts = [_eval(make_agent(), 128, Q, env_offset=off, **kw) for off in (0, 128)]
    for k, v in whole.records.items():
        joined = np.concatenate([p.records[k] for p in parts], axis=0)
        if v.dtype == np.float64:
            assert np.array_equal(v.view(np.int64), joined.view(np.int64)), k
        else:
            assert np.array_equal(v, joined), k


def test_shards_record_the_episodes_of_the_whole_batch_pure_mpc():
    _shards(lambda: _pure(collision_cost=True))


def test_shards_record_the_episodes_of_the_whole_batch_stochastic_gsde_policy(tmp_path):
    def make():
        agent, meta = _mpcrl("ppo_v0", tmp_path)
        assert meta["use_sde"]
        return agent
    _shards(make, deterministic=False)


def _check_valid(res, B, Q):
    from mpc_rl_for_avs_amd import rollout
    r = res.records
    assert r["steps"].shape == (B, Q)
    assert (r["steps"] >= 1).all() and (r["steps"] <= rollout.EPISODE_STEPS).all()
    assert (r["steps"][r["truncated"]] == rollout.EPISODE_STEPS).all()
    assert not (r["truncated"] & r["success"]).any()
    assert (r["avg_speed"] >= 0).all() and (r["avg_speed"] <= 30).all()
    assert res.steps <= Q * rollout.EPISODE_STEPS
    s = res.summary()
    assert s["episodes"] == B * Q and 0 <= s["unsolved_frac"] <= 1 and s["env_steps_per_s"] > 0


def _eager_replay(agent, B, **kw):
    import torch
    seen = []
    take = lambda d: {k: (v.cpu().numpy().copy() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
    res = _eval(agent, B, 1, use_graph=False, on_step=lambda d: seen.append(take(d)), **kw)
    _assert_records_equal(res.records, esh.replay(seen, B, 1))
    return res


AGENTS = ["pure_mpc", "pure_mpc_collision", "ltv"] + [f"{n}:{d}" for n in sde_host.NAMES for d in ("det", "sto")]


@pytest.mark.parametrize("kind", AGENTS)
def test_every_agent_kind_runs_to_completion(kind, tmp_path):
    from mpc_rl_for_avs_amd.pure_mpc_linear import IterativeLinearMPC_Agent
    B, kw = 256, {}
    if kind.startswith("pure_mpc"):
        agent = _pure(collision_cost=kind.endswith("collision"))
    elif kind == "ltv":
        agent = IterativeLinearMPC_Agent(Env, dict(horizon=20, render=False))
    else:
        name, d = kind.split(":")
        agent, _ = _mpcrl(name, tmp_path)
        kw["deterministic"] = d == "det"
    res = _eval(agent, B, 1, **kw)
    _check_valid(res, B, 1)
    _check_valid(_eager_replay(agent, B, **kw), B, 1)
