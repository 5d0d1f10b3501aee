"""The end-to-end PPO baseline (the reference's fourth model, agents/ppo_agent.py) without a GPU: the per-thread code of
mpc_policy_control_kernel<E> compiled for the host (tests/cpu_policy_control_harness.cpp) against the host build of
mpc_policy_act bit for bit, at every tile size and across every tile boundary; the controls' saturation; rollout.PPOAgent and
BatchedCollector(version="direct") on the torch CPU environment with no engine; the save_sb3 / load_sb3 round trip."""
import numpy as np
import pytest
import torch

import glue_host
import policy_control_host as pch
import policy_ref as pr

BATCHES = (1, 2, 3, 7, 8, 9, 15, 16, 17, 33)        # across every tile boundary of E <= 16
ENV_OFFSET = 1000


@pytest.mark.parametrize("hidden", [8, 64, 128])
def test_tiled_kernel_code_equals_the_per_environment_code(hidden):
    """policy_control for E = 1, 2, 4, 8, 16 against glue_host.policy_act (A = 2, v0): actions, values, log-probabilities and
    the written-back noise bit for bit, handed-in noise and the kernel's own draws (steps 0 and 5, environment offset 1000);
    control is numpy's 5 * clip and (pi / 4) * clip of the returned actions."""
    pol = pr.make_policy(hidden, 2, 0.0, use_sde=False, seed=hidden + 1)
    for B in BATCHES:
        obs = pr.make_obs(B, seed=hidden + B)
        given = np.random.default_rng(hidden * 100 + B).standard_normal((B, 2)).astype(np.float32)
        for draw in (None, (77, ENV_OFFSET, 0), (77, ENV_OFFSET, 5)):
            want = glue_host.policy_act(pol, obs, given.copy(), "v0", True, draw=draw)
            if draw is None:
                assert np.array_equal(want["noise"], given)
            else:
                assert not np.array_equal(want["noise"], given)
            for tile in pch.TILES:
                got = pch.policy_control(pol, obs, given, tile, draw=draw)
                for k in ("actions", "values", "log_probs", "noise"):
                    assert np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), (k, B, tile, draw)
                assert np.array_equal(got["control"], pch.numpy_control(got["actions"])), (B, tile, draw)
                assert np.array_equal(got["control"], pch.map_control(got["actions"]))
    # the steps draw different noise, and the offset shifts the stream by environments
    a = glue_host.policy_act(pol, pr.make_obs(4, seed=1), np.zeros((4, 2), np.float32), "v0", True, draw=(77, ENV_OFFSET, 0))["noise"]
    b = pch.policy_control(pol, pr.make_obs(4, seed=1), np.zeros((4, 2), np.float32), 4, draw=(77, ENV_OFFSET + 1, 0))["noise"]
    assert np.array_equal(a[1:], b[:3])


def _saturated_policy(signs):
    """Zero action head with biases +-3: with zero noise the action is the bias itself."""
    pol = pr.make_policy(64, 2, 0.0, use_sde=False, seed=5)
    with torch.no_grad():
        pol.action_net.weight.zero_()
        pol.action_net.bias.copy_(torch.tensor([3.0 * signs[0], 3.0 * signs[1]]))
    return pol


@pytest.mark.parametrize("signs", [(1, -1), (-1, 1)])
def test_saturated_actions_give_the_range_ends_and_stay_unclipped(signs):
    pol = _saturated_policy(signs)
    B = 5
    obs = pr.make_obs(B, seed=2)
    want = np.tile(np.array([5.0 * signs[0], (np.pi / 4) * signs[1]]), (B, 1))
    for tile in pch.TILES:
        got = pch.policy_control(pol, obs, np.zeros((B, 2), np.float32), tile)
        assert np.array_equal(got["actions"], np.tile(np.float32([3.0 * signs[0], 3.0 * signs[1]]), (B, 1)))
        assert np.array_equal(got["control"], want)
    from mpc_rl_for_avs_amd import rollout
    pol.refresh_fused()
    a, _, _ = pol.act(torch.from_numpy(obs), noise=torch.zeros(B, 2))
    assert np.array_equal(rollout.map_control(a).numpy(), want) and np.array_equal(a.numpy(), got["actions"])
    # inside the range the mapping is linear, and the bounds themselves are kept
    inside = np.float32([[0.5, -0.25], [1.0, -1.0], [-1.0, 1.0], [0.0, 0.0]])
    assert np.array_equal(pch.map_control(inside), pch.numpy_control(inside))
    assert np.array_equal(rollout.map_control(torch.from_numpy(inside)).numpy(), pch.numpy_control(inside))
    assert np.array_equal(pch.map_control(inside)[1], [5.0, -np.pi / 4])


def test_ppo_agent_on_the_cpu_environment_without_an_engine():
    from mpc_rl_for_avs_amd import evaluate, rollout
    pol = pr.make_policy(64, 2, -0.5, use_sde=False, seed=9)
    agent = rollout.PPOAgent(pol)
    assert agent.engine is None
    B = 8
    obs = torch.from_numpy(pr.make_obs(B, seed=4))
    out = agent.act_batch_torch(obs, deterministic=True)
    pol.refresh_fused()
    mean, _, _ = pol.act(obs, noise=torch.zeros(B, 2))
    assert torch.equal(out["act"], rollout.map_control(mean)) and out["act"].dtype == torch.float64
    with torch.no_grad():
        fwd, _, _ = pol(obs, deterministic=True)
    assert torch.allclose(out["act"], rollout.map_control(fwd), atol=1e-5, rtol=0)
    for k in ("status", "iters"):
        assert out[k].dtype == torch.int32 and out[k].shape == (B,) and not out[k].any()
    again = agent.act_batch_torch(obs, deterministic=True)
    assert again["act"].data_ptr() == out["act"].data_ptr()              # the same output tensors on every call
    # stochastic: seeded, restartable, and different from the mean
    s1 = agent.act_batch_torch(obs, deterministic=False, seed=3)["act"].clone()
    s2 = agent.act_batch_torch(obs, deterministic=False, seed=3)["act"].clone()
    agent.restart_actions()
    s3 = agent.act_batch_torch(obs, deterministic=False, seed=3)["act"].clone()
    assert torch.equal(s1, s3) and not torch.equal(s1, s2) and not torch.equal(s1, out["act"])
    # predict: SB3's - one observation, the clipped normalised action, deterministic by default
    with torch.no_grad():
        pol.action_net.bias.add_(torch.tensor([2.0, 0.0]))              # component 0 beyond the Box bound
    a = agent.predict(obs[0].numpy())
    with torch.no_grad():
        fwd, _, _ = pol(obs[:1], deterministic=True)
    assert a.dtype == np.float32 and a.shape == (2,) and a[0] == 1.0 and float(fwd[0, 0]) > 1.0
    assert np.array_equal(a, np.clip(fwd[0].numpy(), -1.0, 1.0))
    pb = agent.predict_batch(obs)
    assert torch.equal(pb["act"], rollout.map_control(pb["rl_action"])) and float(pb["rl_action"][0, 0]) > 1.0
    assert pb["act"].dtype == torch.float64 and not pb["status"].any() and not pb["iters"].any()
    assert pb["status"].dtype == torch.int32 and pb["iters"].dtype == torch.int32
    # closed loop: 8 environments x 1 episode, records for each, no solve anywhere
    env = rollout.SyntheticIntersectionEnv(B, device="cpu", seed=21, n_others=4, backend="torch")
    res = evaluate.evaluate_agent(agent, env, episodes_per_env=1, use_graph=False, poll_every=5, seed=1)
    rec = res.records
    assert rec["steps"].shape == (B, 1) and (rec["steps"] >= 1).all()
    assert not rec["unsolved"].any() and not rec["max_iters"].any()
    assert set(res.summary()) >= {"success_rate", "collision_rate"}
    # policies the baseline cannot be: another action width, gSDE
    with pytest.raises(ValueError, match="action_dim 2"):
        rollout.PPOAgent(rollout.ActorCritic(1))
    with pytest.raises(ValueError, match="gSDE"):
        rollout.PPOAgent(rollout.ActorCritic(2, use_sde=True))


def test_direct_collector_and_trainer_on_the_cpu():
    from mpc_rl_for_avs_amd import rollout
    B, T = 5, 8
    pol = pr.make_policy(64, 2, -0.5, use_sde=False, seed=12)
    env = rollout.SyntheticIntersectionEnv(B, device="cpu", seed=3, n_others=4, backend="torch")
    col = rollout.BatchedCollector(env, pol, None, version="direct", algorithm="ppo", n_steps=T, seed=4)
    assert not col.fused_glue and col._graph is None
    rows = []
    for _ in range(2):
        stats = col.collect_rollouts()
        b = col.buffer
        assert b.pos == T and stats["steps"] == B * T and stats["mpc_unconverged"] == 0
        assert torch.isfinite(b._row).all() and torch.isfinite(b.advantages).all()
        assert torch.equal(b.mpc_actions, rollout.map_control(b.actions.reshape(-1, 2)).reshape(T, B, 2))
        assert b.actions.abs().max() > 0 and b.obs.abs().sum() > 0
        assert set(col.last_mpc) == {"act", "status", "iters"} and not col.last_mpc["status"].any()
        assert torch.equal(col.last_mpc["act"], b.mpc_actions[-1])
        rows.append(b.actions.clone())
    assert not torch.equal(rows[0], rows[1])
    before = [q.detach().clone() for q in pol.parameters()]
    trainer = rollout.OnPolicyTrainer(col, n_epochs=2, batch_size=16, seed=1)
    log = trainer.learn(col.num_timesteps + 2 * B * T)
    assert len(log) == 2 and all(np.isfinite([r["loss"], r["policy_loss"], r["value_loss"], r["entropy_loss"]]).all() for r in log)
    assert any(not torch.equal(q, w) for q, w in zip(pol.parameters(), before))
    # a2c keeps its meaning (no truncation bootstrap), and the controls are clipped all the same
    col2 = rollout.BatchedCollector(env, pol, None, version="direct", algorithm="a2c", n_steps=T, seed=4)
    col2.collect_rollouts()
    assert col2.buffer.terminal_obs is None
    assert torch.equal(col2.buffer.mpc_actions, rollout.map_control(col2.buffer.actions.reshape(-1, 2)).reshape(T, B, 2))
    assert col2.buffer.mpc_actions[..., 0].abs().max() <= 5.0 and col2.buffer.mpc_actions[..., 1].abs().max() <= np.pi / 4


@pytest.mark.parametrize("kw", [dict(collision_cost=True), dict(warm_start=True), dict(reset_mpc_on_done=True),
                                dict(gather_actions=True), dict(throughput=True), "action_dim", "sde"],
                         ids=lambda k: k if isinstance(k, str) else next(iter(k)))
def test_direct_collector_refuses_what_belongs_to_the_mpc(kw):
    from mpc_rl_for_avs_amd import rollout
    env = rollout.SyntheticIntersectionEnv(3, device="cpu", seed=3, n_others=4, backend="torch")
    pol = rollout.ActorCritic(3 if kw == "action_dim" else 2, use_sde=kw == "sde")
    with pytest.raises(ValueError):
        rollout.BatchedCollector(env, pol, None, version="direct", n_steps=2, **(kw if isinstance(kw, dict) else {}))


@pytest.mark.parametrize("algorithm,version", [("ppo", None), ("a2c", "v0"), (None, "v1")])
def test_checkpoint_round_trip(tmp_path, algorithm, version):
    from mpc_rl_for_avs_amd import rollout
    A = 3 if version == "v1" else 2
    pol = pr.make_policy(40, A, -0.3, use_sde=False, seed=17)
    path = str(tmp_path / "baseline.zip")
    pol.save_sb3(path, version=version, algorithm=algorithm, n_steps=2048)
    back, meta = rollout.ActorCritic.load_sb3(path)
    own, got = pol.state_dict(), back.state_dict()
    assert set(own) == set(got)
    for k in own:
        assert own[k].dtype == got[k].dtype and torch.equal(own[k], got[k]), k
    assert meta == dict(version=version, use_sde=False, sde_sample_freq=-1, action_dim=A, algorithm=algorithm)
    if A == 2:
        agent, meta2 = rollout.PPOAgent.from_sb3(path)
        assert meta2 == meta
        obs = torch.from_numpy(pr.make_obs(6, seed=8))
        orig = rollout.PPOAgent(pol)
        for det in (True, False):
            assert torch.equal(agent.act_batch_torch(obs, deterministic=det, seed=5)["act"],
                               orig.act_batch_torch(obs, deterministic=det, seed=5)["act"])
        assert np.array_equal(agent.predict(obs[0]), orig.predict(obs[0]))
    # a gSDE policy keeps its flag and its sample frequency through the file
    sde = pr.make_policy(8, 1, 0.0, use_sde=True, seed=2)
    sde.save_sb3(path, version="v0", algorithm="ppo", sde_sample_freq=4)
    back, meta = rollout.ActorCritic.load_sb3(path)
    assert meta["use_sde"] and meta["sde_sample_freq"] == 4 and torch.equal(back.log_std, sde.log_std)
