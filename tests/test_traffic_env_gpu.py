"""`mpc_synth_env_step_idm` on the GPU (traffic="idm"): the kernel against its host build (same seed, same episodes), against the
torch ops on the device, inside a captured rollout step and a closed-loop evaluation; and the default environment untouched."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hostlib():
    from test_traffic_env_cpu import load_traffic_lib
    return load_traffic_lib()


@pytest.mark.parametrize("K, B", [(0, 5), (1, 66), (4, 256), (9, 131)])
def test_kernel_equals_its_host_build(hostlib, K, B):
    """No traffic, one vehicle, four, the most the observation holds; batch sizes that leave the last wave partly empty."""
    import torch
    from mpc_rl_for_avs_amd import rollout
    from test_traffic_env_cpu import TrafficHostEnv
    dev = torch.device("cuda:0")
    g = rollout.SyntheticIntersectionEnv(B, device=dev, seed=21, n_others=K, spawn_probability=0.3, traffic="idm")
    assert g.backend == "hip"
    h = TrafficHostEnv(hostlib, B, K, seed=21, spawn_probability=0.3)
    assert np.allclose(g.reset().cpu().numpy(), h.reset(), rtol=0, atol=1e-5)
    assert np.array_equal(g.oactive.cpu().numpy(), h.oactive.astype(bool)) and np.array_equal(g.oroute.cpu().numpy(), h.oroute)
    rng = np.random.default_rng(0)
    ended = braked_for_ego = 0
    respawned_turns = set()
    for step in range(150):
        act = np.stack([rng.uniform(-3, 5, B), 0.03 * rng.uniform(-1, 1, B)], axis=1)
        before = h.oactive.astype(bool).copy()
        o_g, r_g, d_g, info = g.step(torch.as_tensor(act, device=dev))
        o_h, r_h, d_h = h.step(act)
        assert np.array_equal(d_g.cpu().numpy(), d_h), step
        for k in ("crashed", "arrived", "truncated"):
            assert np.array_equal(info[k].cpu().numpy(), h.flags[k].astype(bool)), (step, k)
        assert np.array_equal(g.oactive.cpu().numpy(), h.oactive.astype(bool)), step
        assert np.array_equal(g.oroute.cpu().numpy(), h.oroute), step
        assert np.allclose(r_g.cpu().numpy(), r_h, rtol=0, atol=1e-4)
        assert np.allclose(o_g.cpu().numpy(), o_h, rtol=0, atol=1e-4)
        assert np.allclose(info["terminal_obs"].cpu().numpy(), h.tobs, rtol=0, atol=1e-4)
        for n in ("ego", "oprog", "ospeed"):
            assert np.allclose(getattr(g, n).cpu().numpy(), getattr(h, n), rtol=0, atol=1e-8), (step, n)
        ended += int(d_h.sum())
        braked_for_ego += int(((h.leader == -1) & (h.accel < 0.0)).any(axis=1).sum())
        new = h.oactive.astype(bool) & ~before & ~d_h[:, None]
        respawned_turns |= set((h.oroute[new] % 3).tolist())
    assert np.array_equal(g.rng_counter.cpu().numpy(), h.ctr)
    # what the comparison covered: the two larger cases each see 20 ended episodes; 66 environments with one vehicle end fewer
    # in 150 steps, there every turn type and the braking still have to occur
    if K >= 1:
        assert ended >= (20 if B >= 128 else 1) and respawned_turns == {0, 1, 2} and braked_for_ego >= 1, \
            (ended, respawned_turns, braked_for_ego)


def test_kernel_equals_the_torch_ops_on_the_device():
    import torch
    from mpc_rl_for_avs_amd import rollout
    B, K = 256, 4
    dev = torch.device("cuda:0")
    gt = rollout.SyntheticIntersectionEnv(B, device=dev, seed=5, n_others=K, spawn_probability=0.0, backend="torch", traffic="idm")
    gh = rollout.SyntheticIntersectionEnv(B, device=dev, seed=5, n_others=K, spawn_probability=0.0, backend="hip", traffic="idm")
    gh.reset()
    for n in ("ego", "opos", "ospeed", "ohead", "oactive", "oroute", "oprog", "otarget", "t"):
        getattr(gt, n).copy_(getattr(gh, n))
    rng = np.random.default_rng(0)
    alive = torch.ones(B, dtype=torch.bool, device=dev)
    for step in range(60):
        act = torch.as_tensor(np.stack([rng.uniform(-3, 5, B), 0.03 * rng.uniform(-1, 1, B)], axis=1), device=dev)
        o1, r1, d1, i1 = gt.step(act)
        o2, r2, d2, i2 = gh.step(act)
        assert torch.equal(d1[alive], d2[alive]), step
        for k in ("crashed", "arrived", "truncated"):
            assert torch.equal(i1[k][alive], i2[k][alive]), (step, k)
        assert torch.allclose(i1["terminal_obs"][alive], i2["terminal_obs"][alive], rtol=0, atol=1e-4)
        alive = alive & ~d2
        assert torch.allclose(gt.ego[alive], gh.ego[alive], rtol=0, atol=1e-9)
    assert int((~alive).sum()) >= 5


def test_captured_step_equals_the_eager_step_and_evaluation_completes():
    import torch
    from mpc_rl_for_avs_amd import engine, evaluate, rollout
    from mpc_rl_for_avs_amd.pure_mpc import PureMPC_Agent
    dev = torch.device("cuda:0")
    B, K, T = 64, 3, 8
    out = []
    for use_graph in (False, True):
        torch.manual_seed(7)
        pol = rollout.ActorCritic(1).to(dev)
        eng = engine.MPCEngine(horizon=20, max_iter=100, device=0)
        env = rollout.SyntheticIntersectionEnv(B, device=dev, seed=3, n_others=K, traffic="idm")
        col = rollout.BatchedCollector(env, pol, eng, version="v0", algorithm="ppo", n_steps=T, collision_cost=False, seed=1,
                                       use_graph=use_graph)
        assert (col._graph is not None) == use_graph, col.graph_fallback_reason
        col.collect_rollouts()
        torch.cuda.synchronize()
        state = {n: getattr(env, n).clone() for n in ("ego", "opos", "ospeed", "ohead", "oactive", "oroute", "oprog", "otarget",
                                                      "t", "rng_counter")}
        out.append((col.buffer._row.clone(), state))
        eng.close()
    assert torch.equal(out[0][0], out[1][0])
    for n, a in out[0][1].items():
        assert torch.equal(a, out[1][1][n]), n

    class Env:
        config = {"simulation_frequency": 30, "policy_frequency": 10, "observation": {"vehicles_count": 10}}

    agent = PureMPC_Agent(Env(), dict(horizon=20, render=False, weight_speed=1, weight_control=1, weight_input_diff=1),
                          collision_cost=False)
    env = rollout.SyntheticIntersectionEnv(64, device=dev, seed=0, n_others=4, traffic="idm")
    res = evaluate.evaluate_agent(agent, env, episodes_per_env=1)
    assert res.summary()["episodes"] == 64          # every environment's episode was recorded


def test_default_environment_is_the_constant_traffic_environment():
    import torch
    from mpc_rl_for_avs_amd import rollout
    dev = torch.device("cuda:0")
    B, K = 131, 4
    a = rollout.SyntheticIntersectionEnv(B, device=dev, seed=9, n_others=K, traffic="constant")
    b = rollout.SyntheticIntersectionEnv(B, device=dev, seed=9, n_others=K)
    assert b.traffic == "constant" and not hasattr(b, "oroute")
    assert torch.equal(a.reset(), b.reset())
    rng = np.random.default_rng(1)
    for step in range(50):
        act = torch.as_tensor(np.stack([rng.uniform(-3, 5, B), 0.03 * rng.uniform(-1, 1, B)], axis=1), device=dev)
        oa, ra, da, ia = a.step(act)
        ob, rb, db, ib = b.step(act)
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db)
        for k in ("terminal_obs", "truncated", "crashed", "arrived"):
            assert torch.equal(ia[k], ib[k]), (step, k)
        for n in ("ego", "opos", "ospeed", "ohead", "oactive", "t", "rng_counter"):
            assert torch.equal(getattr(a, n), getattr(b, n)), (step, n)
