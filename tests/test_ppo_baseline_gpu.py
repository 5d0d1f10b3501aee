"""The end-to-end PPO baseline on the GPU: mpc_policy_control against mpc_policy_act on the same device tensors bit for bit
(every tile boundary, noise handed in and drawn, canaries behind the outputs) and against the float64 statement of
tests/policy_ref.py; the arguments it refuses; the fused BatchedCollector(version="direct") rollout against the torch step fed
the kernel's noise, and its graph replay against its eager run; evaluate_agent / compare with rollout.PPOAgent."""
import ctypes

import numpy as np
import pytest

import policy_control_host as pch
import policy_ref as pr
from test_evaluate_cpu import CFG, Env, _assert_records_equal

pytestmark = pytest.mark.gpu

ENV_OFFSET = 1000
PAD = 16                    # canary rows behind every output
CANARY = -12345.5
BATCHES = (1, 2, 3, 7, 8, 9, 15, 16, 17, 33, 4099)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _launch_both(lib, pol, obs, noise=None, draw=None, tile=None):
    """mpc_policy_act (A = 2, v0, clip) and mpc_policy_control (the shipped tile, or mpc_policy_control_tile) on the same
    observation / weight tensors; outputs have PAD canary rows.  noise [B, 2] is read, or draw = (seed, step) drawn."""
    import torch
    dev, B = obs.device, obs.shape[0]
    f = pol._fz
    H2 = f["b1"].numel()
    full = lambda *sh, dt=torch.float32: torch.full(sh, CANARY, dtype=dt, device=dev)
    step = None if draw is None else torch.tensor([draw[1]], dtype=torch.int64, device=dev)
    seed = 0 if draw is None else draw[0]
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    outs = []
    for which in ("act", "control"):
        o = dict(actions=full(B + PAD, 2), values=full(B + PAD), log_probs=full(B + PAD), noise=full(B + PAD, 2),
                 ref_speed=full(B + PAD, dt=torch.float64), control=full(B + PAD, 2, dt=torch.float64))
        if draw is None:
            o["noise"][:B] = noise
        weights = (_p(f["w1"]), _p(f["b1"]), _p(f["w2"]), _p(f["b2"]), _p(f["wh"]), _p(f["bh"]), _p(f["std"]), _p(f["c0"]))
        if which == "act":
            rc = lib.mpc_policy_act(dev.index, B, 2, H2, _p(obs), *weights, _p(o["noise"]), seed, ENV_OFFSET, _p(step), 0, 1,
                                    _p(o["actions"]), _p(o["values"]), _p(o["log_probs"]), None, _p(o["ref_speed"]), stream)
        else:
            args = (dev.index, B, H2, _p(obs), *weights, _p(o["noise"]), seed, ENV_OFFSET, _p(step), _p(o["actions"]),
                    _p(o["values"]), _p(o["log_probs"]), _p(o["control"]), stream)
            rc = lib.mpc_policy_control(*args) if tile is None else lib.mpc_policy_control_tile(tile, *args)
        assert rc == 0, lib.mpc_last_error()
        torch.cuda.synchronize(dev)
        outs.append({k: v.cpu().numpy() for k, v in o.items()})
    return outs


@pytest.mark.parametrize("hidden", [8, 64, 128])
def test_policy_control_equals_policy_act_bit_for_bit(hidden):
    import torch
    from mpc_rl_for_avs_amd import engine
    dev = torch.device("cuda", 0)
    lib = engine.load_library()
    pol = pr.make_policy(hidden, 2, 0.0, use_sde=False, seed=hidden + 1).to(dev)
    f = pr.fused_weights(pol)
    worst = {}
    for B in BATCHES:
        obs = pr.make_obs(B, seed=hidden + B)
        obs_d = torch.from_numpy(obs).to(dev)
        given = np.random.default_rng(hidden * 100 + B).standard_normal((B, 2)).astype(np.float32)
        # the shipped tile in every noise mode; every other tile of the library once per batch size
        for draw, tile in ((None, None), ((77, 0), None), ((77, 5), None)) + tuple((None, t) for t in pch.TILES):
            act, ctl = _launch_both(lib, pol, obs_d, noise=torch.from_numpy(given).to(dev), draw=draw, tile=tile)
            for k in ("actions", "values", "log_probs", "noise"):
                assert np.array_equal(ctl[k][:B].view(np.int32), act[k][:B].view(np.int32)), (k, B, draw, tile)
            assert np.array_equal(ctl["control"][:B], pch.numpy_control(ctl["actions"][:B])), (B, draw, tile)
            for k in ("actions", "values", "log_probs", "noise", "control"):          # nothing written behind row B
                assert (ctl[k][B:] == CANARY).all(), (k, B, draw, tile)
            if draw is None:
                assert np.array_equal(ctl["noise"][:B], given)                       # handed-in noise is read, not overwritten
            want = pr.gaussian(f, obs.reshape(B, -1), ctl["noise"][:B], 2)
            for k in ("actions", "values", "log_probs"):
                r, e = pr.check(ctl[k][:B], want, k)
                worst[k] = max(worst.get(k, (0.0, 0.0)), (r, e))
    print(f"[policy_control H{hidden}] worst err/bar (err) against float64: " +
          ", ".join(f"{k} {r:.3f} ({e:.2e})" for k, (r, e) in worst.items()))


def test_saturated_controls_on_the_device():
    import torch
    from mpc_rl_for_avs_amd import engine
    dev = torch.device("cuda", 0)
    lib = engine.load_library()
    pol = pr.make_policy(64, 2, 0.0, use_sde=False, seed=5)
    with torch.no_grad():
        pol.action_net.weight.zero_()
        pol.action_net.bias.copy_(torch.tensor([3.0, -3.0]))
    pol = pol.to(dev)
    pol.refresh_fused()
    B = 9
    obs_d = torch.from_numpy(pr.make_obs(B, seed=2)).to(dev)
    _, ctl = _launch_both(lib, pol, obs_d, noise=torch.zeros(B, 2, device=dev))
    assert np.array_equal(ctl["actions"][:B], np.tile(np.float32([3.0, -3.0]), (B, 1)))
    assert np.array_equal(ctl["control"][:B], np.tile([5.0, -np.pi / 4], (B, 1)))


def test_refused_arguments_leave_no_error_behind():
    """Odd 2H, 2H > 256, a null pointer, a negative batch and an unknown tile are MPC_ERR_INVALID_ARG before any launch; B = 0
    is accepted without one.  Afterwards the device has no pending error: a synchronise succeeds and a valid launch computes."""
    import torch
    from mpc_rl_for_avs_amd import engine
    dev = torch.device("cuda", 0)
    lib = engine.load_library()
    x = torch.zeros(1 << 16, device=dev)
    q = ctypes.c_void_p(x.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    base = [dev.index, 2, 128] + [q] * 10 + [0, 0, None, q, q, q, q, st]
    assert lib.mpc_policy_control(*(base[:1] + [0] + base[2:])) == 0                # B == 0: nothing to do
    for i, bad in ((2, 127), (2, 129), (2, 258), (2, 0), (1, -1), (3, None), (8, None), (12, None), (16, None), (19, None)):
        args = list(base)
        args[i] = bad
        assert lib.mpc_policy_control(*args) == -1, (i, bad)
        assert b"mpc_policy_control" in lib.mpc_last_error()
    for tile in (0, 3, 32):
        assert lib.mpc_policy_control_tile(tile, *base) == -1
    torch.cuda.synchronize(dev)                                                     # raises if an error were pending
    pol = pr.make_policy(8, 2, 0.0, use_sde=False, seed=1).to(dev)
    pol.refresh_fused()
    obs_d = torch.from_numpy(pr.make_obs(4, seed=1)).to(dev)
    act, ctl = _launch_both(lib, pol, obs_d, noise=torch.zeros(4, 2, device=dev))
    assert np.array_equal(ctl["actions"][:4], act["actions"][:4]) and np.isfinite(ctl["control"][:4]).all()


def _direct_collector(fused, use_graph, B=37, T=8):
    import torch
    from mpc_rl_for_avs_amd import engine, rollout
    dev = torch.device("cuda", 0)
    torch.manual_seed(11)
    pol = rollout.ActorCritic(2).to(dev)
    with torch.no_grad():
        pol.log_std.fill_(-1.0)
    eng = engine.MPCEngine(horizon=20, max_iter=100)
    env = rollout.SyntheticIntersectionEnv(B, device=dev, seed=9, n_others=4)
    col = rollout.BatchedCollector(env, pol, eng, version="direct", algorithm="ppo", n_steps=T, seed=4, use_graph=use_graph,
                                   fused_glue=fused)
    assert col.fused_glue == fused and (col._graph is not None) == use_graph
    return col, eng


def _snapshot(col, stats):
    b = col.buffer
    return dict(stats=stats, row=b._row.clone(), obs=b.obs.clone(), actions=b.actions.clone(), values=b.values.clone(),
                logp=b.log_probs.clone(), rewards=b.rewards.clone(), starts=b.episode_starts.clone(), mpc=b.mpc_actions.clone(),
                adv=b.advantages.clone(), ret=b.returns.clone(), dones=col._roll["dones"].clone(), last=col._last_obs.clone())


def test_fused_direct_rollout_equals_the_torch_step_and_its_graph_replay():
    """37 environments, 2 rollouts of 8 steps.  Fused (mpc_policy_control + environment + mpc_rollout_record) against the torch
    step fed the noise the kernel drew: actions and values to 2e-5, log-probabilities to 1e-4 (the bars of
    tests/test_policy_shapes_gpu.py for this comparison: the float32 sums of three small matrix products in another order);
    the controls are those actions times 5 and pi / 4, so 1e-4; rewards (smooth in the state) to 1e-4; episode starts and
    dones equal.  The graph-replayed fused rollouts equal the eager fused ones bit for bit."""
    import torch
    T, R = 8, 2
    col, eng = _direct_collector(True, False)
    eager, noises = [], []
    for _ in range(R):
        col._begin_rollout()
        for _ in range(T):
            col._step()
            noises.append(col._fg["noise"].clone())
        col._finish_rollout()
        eager.append(_snapshot(col, col._rollout_stats(T)))
    assert int(col._fg["step"]) == R * T and not torch.equal(noises[0], noises[1])
    assert col.last_mpc["act"].data_ptr() == col._fg["ctrl"].data_ptr() and not col.last_mpc["status"].any()
    eng.close()
    col, eng = _direct_collector(True, True)
    for r in range(R):
        g = _snapshot(col, col.collect_rollouts())
        assert g["stats"] == eager[r]["stats"] and g["stats"]["mpc_unconverged"] == 0
        for k in ("row", "mpc", "adv", "ret", "dones", "last"):
            assert torch.equal(g[k], eager[r][k]), (r, k)
    eng.close()
    col, eng = _direct_collector(False, False)
    col.noise_feed = [x.clone() for x in noises]
    for r in range(R):
        t, f = _snapshot(col, col.collect_rollouts()), eager[r]
        d = {k: float((f[k] - t[k]).abs().max()) for k in ("actions", "values", "logp", "mpc", "rewards", "obs")}
        print(f"[direct rollout {r}] max |fused - torch|: " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()))
        assert torch.equal(f["obs"][0], t["obs"][0]) or r > 0
        assert d["actions"] <= 2e-5 and d["values"] <= 2e-5 and d["logp"] <= 1e-4
        assert d["mpc"] <= 1e-4 and d["rewards"] <= 1e-4
        assert torch.equal(f["starts"], t["starts"]) and torch.equal(f["dones"], t["dones"])
        assert torch.equal(f["mpc"], col.buffer.mpc_actions.new_tensor(pch.numpy_control(f["actions"].reshape(-1, 2).cpu().numpy())
                                                                       ).reshape(f["mpc"].shape))
        assert f["stats"]["episodes"] == t["stats"]["episodes"] and f["stats"]["crashed"] == t["stats"]["crashed"]
        assert torch.isfinite(f["adv"]).all() and torch.isfinite(t["adv"]).all()
    assert not col.noise_feed
    eng.close()


def _agent(seed=3):
    import torch
    from mpc_rl_for_avs_amd import rollout
    from mpc_rl_for_avs_amd.engine import MPCEngine
    pol = pr.make_policy(64, 2, -1.0, use_sde=False, seed=seed).to(torch.device("cuda", 0))
    return rollout.PPOAgent(pol, MPCEngine(horizon=20, device=0))


def _eval(agent, B, seed=7, **kw):
    import torch
    from mpc_rl_for_avs_amd import evaluate, rollout
    env = rollout.SyntheticIntersectionEnv(B, device=torch.device("cuda", 0), seed=seed, n_others=4)
    return evaluate.evaluate_agent(agent, env, episodes_per_env=1, seed=seed, **kw)


@pytest.mark.parametrize("deterministic", [False, True], ids=["stochastic", "deterministic"])
def test_evaluate_ppo_agent_graph_equals_eager_and_repeats(deterministic):
    agent = _agent()
    g = _eval(agent, 64, use_graph=True, deterministic=deterministic)
    e = _eval(agent, 64, use_graph=False, deterministic=deterministic)
    again = _eval(agent, 64, use_graph=True, deterministic=deterministic)
    _assert_records_equal(g.records, e.records)
    _assert_records_equal(g.records, again.records)
    assert g.steps == e.steps and g.records["steps"].shape == (64, 1)
    assert not g.records["unsolved"].any() and not g.records["max_iters"].any()
    assert agent._act_state["fused"]
    other = _eval(agent, 64, use_graph=True, deterministic=not deterministic)
    assert not all(np.array_equal(other.records[k], g.records[k]) for k in ("steps", "avg_speed", "return"))
    agent.engine.close()


def test_compare_puts_the_baseline_beside_pure_mpc():
    import torch
    from mpc_rl_for_avs_amd import evaluate, rollout
    from mpc_rl_for_avs_amd.engine import MPCEngine
    from mpc_rl_for_avs_amd.pure_mpc import PureMPC_Agent
    agents = {"pure_mpc": PureMPC_Agent(Env(), dict(CFG), engine=MPCEngine(horizon=20, device=0), collision_cost=False),
              "ppo": _agent()}
    make_env = lambda: rollout.SyntheticIntersectionEnv(32, device=torch.device("cuda", 0), seed=5, n_others=4)
    out = evaluate.compare(agents, make_env, episodes_per_env=1, seed=5)
    assert set(out) == {"pure_mpc", "ppo"} and set(out["pure_mpc"]) == set(out["ppo"])
    assert out["ppo"]["episodes"] == 32 and out["ppo"]["unsolved_frac"] == 0.0
    agents["ppo"].engine.close()
