"""gSDE exploration (ActorCritic(use_sde=True), stable-baselines3's StateDependentNoiseDistribution) and SB3 checkpoints on
the CPU: the torch distribution against an independent float64 numpy statement of its formulas, its gradients, the host
build of the fused kernel's code (csrc/mpc_rollout_glue.hpp, mpc_policy_act_sde) against ActorCritic.act, the kernel's
counter-based draws, ActorCritic.load_sb3 on checkpoints rebuilt from tests/golden/sb3_policies.npz, and MPCRLAgent."""
import math
import os
import zipfile

import numpy as np
import pytest
import torch

import sde_host
from mpc_rl_for_avs_amd import rollout

REFERENCE_WEIGHTS = "/root/reference/weights"


def _obs(B, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((B, 10, 8), generator=g) * 3.0


def _sde_policy(A, seed, log_std_init=-0.5):
    torch.manual_seed(seed)
    pol = rollout.ActorCritic(A, use_sde=True, log_std_init=log_std_init)
    with torch.no_grad():
        pol.log_std.add_(0.3 * torch.randn(pol.log_std.shape))      # not all equal: every (h, a) entry matters
    return pol


def _numpy_sde(pol, obs, actions=None, Z=None):
    """The formulas of StateDependentNoiseDistribution (full_std, no expln, epsilon 1e-6) in float64 numpy, from the
    parameters alone."""
    P = {k: v.detach().double().numpy() for k, v in pol.state_dict().items()}
    x = obs.reshape(obs.shape[0], -1).double().numpy()
    lat = np.tanh(np.tanh(x @ P["pi.0.weight"].T + P["pi.0.bias"]) @ P["pi.2.weight"].T + P["pi.2.bias"])
    mean = lat @ P["action_net.weight"].T + P["action_net.bias"]
    std_m = np.exp(P["log_std"])
    var = (lat ** 2) @ (std_m ** 2)
    scale = np.sqrt(var + 1e-6)
    out = dict(mean=mean, scale=scale, entropy=(0.5 + 0.5 * np.log(2 * np.pi) + np.log(scale)).sum(axis=1))
    if Z is not None:
        E = std_m[None] * np.asarray(Z, np.float64)
        out["sample"] = mean + np.einsum("bh,bha->ba", lat, E)
    if actions is not None:
        a = np.asarray(actions, np.float64)
        out["log_prob"] = (-(a - mean) ** 2 / (2 * scale ** 2) - np.log(scale) - 0.5 * np.log(2 * np.pi)).sum(axis=1)
    return out


@pytest.mark.parametrize("A", [1, 3, 4])
def test_sde_distribution_against_numpy(A):
    B = 40
    pol = _sde_policy(A, seed=3 + A)
    assert tuple(pol.log_std.shape) == (64, A)
    obs = _obs(B, 17)
    Z = torch.randn((B, 64, A), generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        d, latent_d = pol._dist(obs)
        sample = d.mean + pol._sde_sample_noise(latent_d, pol.log_std.exp(), Z)
        _, logp, ent = pol.evaluate_actions(obs, sample)
    ref = _numpy_sde(pol, obs, actions=sample.double().numpy(), Z=Z.numpy())
    rel = lambda got, want: np.abs(np.asarray(got, np.float64) - want).max() / max(1.0, np.abs(want).max())
    assert rel(d.mean.numpy(), ref["mean"]) < 1e-5
    assert rel(d.stddev.numpy(), ref["scale"]) < 1e-5
    assert rel(sample.numpy(), ref["sample"]) < 1e-5
    assert rel(logp.numpy(), ref["log_prob"]) < 1e-5
    assert rel(ent.numpy(), ref["entropy"]) < 1e-5
    # the state-dependent variance really varies with the state
    assert float(d.stddev.std(dim=0).max()) > 1e-3
    # forward(): per-environment matrices when n == B, the single matrix otherwise (get_noise), mean when deterministic
    with torch.no_grad():
        pol.reset_noise(B, generator=torch.Generator().manual_seed(1))
        a, v, lp = pol(obs)
        want = _numpy_sde(pol, obs, Z=pol.sde_noise.numpy())["sample"]
        assert rel(a.numpy(), want) < 1e-5
        a1, _, _ = pol(obs[:7])
        want1 = _numpy_sde(pol, obs[:7], Z=pol.sde_noise_single.expand(7, -1, -1).numpy())["sample"]
        assert rel(a1.numpy(), want1) < 1e-5
        am, _, _ = pol(obs, deterministic=True)
        assert torch.equal(am, d.mean)
        # act(): the fused weights give the same function
        pol.refresh_fused()
        fa, fv, flp = pol.act(obs, noise=Z)
        assert rel(fa.numpy(), ref["sample"]) < 1e-5
        assert rel(flp.numpy(), ref["log_prob"]) < 1e-4
        assert torch.allclose(fv, pol.predict_values(obs), atol=1e-5)


def test_sde_gradients():
    """log_std learns only through the variance; the variance never passes a gradient into the policy tower."""
    B, A = 32, 3
    pol = _sde_policy(A, seed=8)
    obs = _obs(B, 2)
    with torch.no_grad():
        pol.reset_noise(B)
        actions, _, _ = pol(obs)
    _, logp, ent = pol.evaluate_actions(obs, actions)
    loss = -(logp.mean()) - 0.01 * ent.mean()
    loss.backward()
    assert pol.log_std.grad is not None and float(pol.log_std.grad.abs().max()) > 0
    # the standard deviation alone: gradient to log_std, none to pi
    pol.zero_grad()
    d, _ = pol._dist(obs)
    grads = torch.autograd.grad(d.stddev.sum(), [pol.log_std] + list(pol.pi.parameters()) + list(pol.action_net.parameters()),
                                allow_unused=True)
    assert grads[0] is not None and float(grads[0].abs().max()) > 0
    assert all(g is None for g in grads[1:])
    # finite differences of the loss in log_std (float64)
    pd = _sde_policy(A, seed=8).double()
    obs64, act64 = obs.double(), actions.double()

    def f(ls):
        with torch.no_grad():
            pd.log_std.copy_(ls)
        _, lp, en = pd.evaluate_actions(obs64, act64)
        return -(lp.mean()) - 0.01 * en.mean()

    base = pd.log_std.detach().clone()
    pd.zero_grad()
    f(base).backward()
    g = pd.log_std.grad.clone()
    eps = 1e-6
    for (h, a) in [(0, 0), (5, 2), (63, 1), (31, 0)]:
        up, dn = base.clone(), base.clone()
        up[h, a] += eps
        dn[h, a] -= eps
        with torch.no_grad():
            fd = (f(up) - f(dn)).item() / (2 * eps)
        assert abs(fd - g[h, a].item()) <= 1e-6 + 1e-5 * abs(fd), (h, a, fd, g[h, a].item())


@pytest.mark.parametrize("version,clip,A", [("v0", True, 1), ("v0", False, 1), ("v1", True, 4), ("v1", False, 3)])
def test_host_build_of_the_kernel_is_the_torch_step(version, clip, A):
    B = 64
    pol = _sde_policy(A, seed=11, log_std_init=0.0)
    obs = _obs(B, 21)
    Z = torch.randn((B, 64, A), generator=torch.Generator().manual_seed(9))
    o = sde_host.policy_act_sde(pol, obs.numpy(), Z.numpy(), version=version, clip=clip)
    pol.refresh_fused()
    a, v, lp = pol.act(obs, noise=Z)
    assert np.allclose(o["actions"], a.numpy(), atol=2e-5, rtol=0)
    assert np.allclose(o["values"], v.numpy(), atol=2e-5, rtol=0)
    assert np.allclose(o["log_probs"], lp.numpy(), atol=1e-4, rtol=1e-5)
    c = torch.clamp(a, -1.0, 1.0) if clip else a
    assert float(a.abs().max()) > 1.0                       # the clip is exercised
    if version == "v1":
        assert np.allclose(o["weights"], c[:, :3].double().numpy(), atol=2e-5)
    else:
        assert np.allclose(o["ref_speed"], c[:, 0].double().numpy(), atol=2e-5)
    # drawn in the kernel's code: the Z it returns reproduce the same step through torch
    d = sde_host.policy_act_sde(pol, obs.numpy(), None, version=version, clip=clip, draw=(5, 100, 7, 3, -1))
    a2, _, lp2 = pol.act(obs, noise=torch.from_numpy(d["Z"]))
    assert np.allclose(d["actions"], a2.numpy(), atol=2e-5) and np.allclose(d["log_probs"], lp2.numpy(), atol=1e-4, rtol=1e-5)
    for b in (0, 17, 63):
        assert np.array_equal(d["Z"][b], sde_host.sde_noise(5, 100 + b, 7, 64, A))


def test_counter_based_exploration_draws():
    H, A = 64, 8
    z = sde_host.sde_noise(1, 0, 0, H, A)
    assert np.array_equal(z, sde_host.sde_noise(1, 0, 0, H, A))                  # deterministic
    for other in (sde_host.sde_noise(1, 1, 0, H, A), sde_host.sde_noise(1, 0, 1, H, A), sde_host.sde_noise(2, 0, 0, H, A)):
        assert not np.allclose(other, z)                                          # env id, epoch, seed
        assert abs(np.corrcoef(other.ravel(), z.ravel())[0, 1]) < 0.15
    allz = np.concatenate([sde_host.sde_noise(7, e, ep, H, A).ravel() for e in range(50) for ep in range(4)])
    assert allz.size == 102400
    assert abs(allz.mean()) < 0.01 and abs(allz.var() - 1.0) < 0.02
    assert abs((allz ** 4).mean() - 3.0) < 0.1                                   # Gaussian tails
    # sde_sample_freq = k: the matrix changes exactly every k steps of the rollout; -1: never within a rollout
    for k in (1, 3, 5):
        mats = [sde_host.sde_noise(3, 9, 40, 8, 2, step=t, freq=k) for t in range(16)]
        for t in range(1, 16):
            assert np.array_equal(mats[t], mats[t - 1]) == (t % k != 0), (k, t)
    assert all(np.array_equal(sde_host.sde_noise(3, 9, 40, 8, 2, step=t), sde_host.sde_noise(3, 9, 40, 8, 2)) for t in range(10))


def _load(tmp_path, name):
    return rollout.ActorCritic.load_sb3(sde_host.sb3_zip(tmp_path, name))


@pytest.mark.parametrize("name,use_sde,A,version", [("ppo_v0", True, 1, "v0"), ("a2c_v0", False, 1, "v0"),
                                                    ("ppo_v1", True, 4, "v1")])
def test_load_sb3(tmp_path, name, use_sde, A, version):
    pol, meta = _load(tmp_path, name)
    sd, data = sde_host.fixture(name)
    assert meta["use_sde"] == use_sde == pol.use_sde and meta["action_dim"] == A == pol.action_dim
    assert meta["version"] == version and meta["sde_sample_freq"] == -1
    assert meta["algorithm"] == name[:3]
    own = pol.state_dict()
    for k, name_ in rollout.ActorCritic._SB3_KEYS.items():
        assert np.array_equal(own[name_].numpy(), sd[k]), k
    if name == "ppo_v0":
        obs = _obs(16, 4)
        with torch.no_grad():
            a, _, _ = pol(obs, deterministic=True)
        assert np.allclose(a.double().numpy(), _numpy_sde(pol, obs)["mean"], atol=1e-5, rtol=1e-5)


def test_load_sb3_refuses_malformed_checkpoints(tmp_path):
    sd, data = sde_host.fixture("ppo_v0")
    bad = dict(sd, log_std=np.zeros(1, np.float32))                  # use_sde but a DiagGaussian log_std
    with pytest.raises(ValueError, match="log_std"):
        rollout.ActorCritic.load_sb3(sde_host.write_sb3_zip(tmp_path / "a.zip", bad, data))
    with pytest.raises(ValueError, match="policy.pth"):
        rollout.ActorCritic.load_sb3(sde_host.write_sb3_zip(tmp_path / "b.zip", sd, data, with_policy=False))
    wrong = dict(sd)
    wrong["action_net.bias"] = np.zeros(2, np.float32)
    with pytest.raises(ValueError, match="action_net.bias"):
        rollout.ActorCritic.load_sb3(sde_host.write_sb3_zip(tmp_path / "c.zip", wrong, data))
    extra = dict(sd, **{"features_extractor.weight": np.zeros(3, np.float32)})
    with pytest.raises(ValueError, match="unexpected"):
        rollout.ActorCritic.load_sb3(sde_host.write_sb3_zip(tmp_path / "d.zip", extra, data))
    (tmp_path / "e.zip").write_bytes(b"not a zip")
    with pytest.raises(ValueError, match="zip"):
        rollout.ActorCritic.load_sb3(str(tmp_path / "e.zip"))
    # the pickled fields are never unpickled: a payload that would raise on unpickling loads fine
    poisoned = dict(data, policy_class={":type:": "x", ":serialized:": "gARjYnVpbHRpbnMKZXZhbApxAC4="})
    pol, meta = rollout.ActorCritic.load_sb3(sde_host.write_sb3_zip(tmp_path / "f.zip", sd, poisoned))
    assert meta["use_sde"]


@pytest.mark.skipif(not os.path.isdir(REFERENCE_WEIGHTS), reason="the reference's checkpoints are not on this machine")
def test_load_sb3_on_the_reference_checkpoints():
    for rel, use_sde, A in (("v0/test_ppo_v0.zip", True, 1), ("v0/test_ppo_v0_128000.zip", True, 1),
                            ("v0/test_ppo_v0_128_linux.zip", True, 1), ("v0/test_a2c_v0.zip", False, 1),
                            ("v1/test_ppo_v1.zip", True, 4)):
        path = os.path.join(REFERENCE_WEIGHTS, rel)
        assert zipfile.is_zipfile(path)
        pol, meta = rollout.ActorCritic.load_sb3(path)
        assert meta["use_sde"] == use_sde and meta["action_dim"] == A
    pol, _ = rollout.ActorCritic.load_sb3(os.path.join(REFERENCE_WEIGHTS, "v0/test_ppo_v0.zip"))
    sd, _ = sde_host.fixture("ppo_v0")
    assert np.array_equal(pol.log_std.detach().numpy(), sd["log_std"])


class _HeadActorCritic(torch.nn.Module):
    """ActorCritic as it was before gSDE (the state-independent Gaussian), restated to pin the default."""

    def __init__(self, action_dim, obs_dim=80, hidden=64):
        super().__init__()
        mk = lambda: torch.nn.Sequential(torch.nn.Linear(obs_dim, hidden), torch.nn.Tanh(),
                                         torch.nn.Linear(hidden, hidden), torch.nn.Tanh())
        self.pi, self.vf = mk(), mk()
        self.action_net = torch.nn.Linear(hidden, action_dim)
        self.value_net = torch.nn.Linear(hidden, 1)
        self.log_std = torch.nn.Parameter(torch.zeros(action_dim))

    def forward(self, obs, generator=None):
        mean = self.action_net(self.pi(obs.flatten(1)))
        d = torch.distributions.Normal(mean, self.log_std.exp().expand_as(mean))
        a = d.mean + d.stddev * torch.randn(mean.shape, generator=generator)
        return a, self.value_net(self.vf(obs.flatten(1)))[:, 0], d.log_prob(a).sum(dim=1), d.entropy().sum(dim=1)


def test_default_policy_is_unchanged():
    torch.manual_seed(123)
    new = rollout.ActorCritic(1)
    after_new = torch.randn(3)
    torch.manual_seed(123)
    old = _HeadActorCritic(1)
    after_old = torch.randn(3)
    assert torch.equal(after_new, after_old)               # construction draws the same random numbers
    assert not new.use_sde and tuple(new.log_std.shape) == (1,)
    for (k1, v1), (k2, v2) in zip(new.state_dict().items(), old.state_dict().items()):
        assert k1 == k2 and torch.equal(v1, v2)
    obs = _obs(20, 6)
    with torch.no_grad():
        a, v, lp = new(obs, generator=torch.Generator().manual_seed(4))
        a0, v0, lp0, ent0 = old(obs, generator=torch.Generator().manual_seed(4))
        assert torch.equal(a, a0) and torch.equal(v, v0) and torch.equal(lp, lp0)
        _, lpe, ent = new.evaluate_actions(obs, a)
        assert torch.equal(lpe, lp0) and torch.equal(ent, ent0)
        new.refresh_fused()
        assert set(new._fz) == {"w1", "b1", "w2", "b2", "wh", "bh", "std", "c0"}
    with pytest.raises(RuntimeError):
        new.reset_noise(4)


class _StubEngine:
    def __init__(self):
        self.calls = []

    def predict_batch_torch(self, obs, weights, ref_speed=None, collision_cost=False, out=None, sync=False, warm_start=False):
        self.calls.append(dict(weights=weights.clone(), ref_speed=None if ref_speed is None else ref_speed.clone()))
        B = obs.shape[0]
        return dict(act=torch.zeros((B, 2), dtype=torch.float64), status=torch.zeros(B, dtype=torch.int32),
                    iters=torch.zeros(B, dtype=torch.int32))

    def predict_batch(self, obs, weights, ref_speed=None, collision_cost=False):
        self.calls.append(dict(weights=torch.as_tensor(weights), ref_speed=None if ref_speed is None else torch.as_tensor(ref_speed)))
        B = obs.shape[0]
        return dict(act=np.full((B, 2), 0.25), status=np.zeros(B, np.int32), iters=np.zeros(B, np.int32))

    def reset_env_mask_torch(self, done, warm_only=False):
        pass


@pytest.mark.parametrize("freq", [-1, 2])
def test_collector_with_sde_on_the_cpu(freq):
    """The torch step of BatchedCollector with a gSDE policy: one matrix per environment, redrawn at the rollout start and
    every sde_sample_freq steps; the buffer's log-probabilities are those of evaluate_actions."""
    torch.manual_seed(0)
    pol = rollout.ActorCritic(1, use_sde=True, log_std_init=-1.0)
    env = rollout.SyntheticIntersectionEnv(8, seed=1, n_others=2)
    col = rollout.BatchedCollector(env, pol, _StubEngine(), version="v0", algorithm="ppo", n_steps=6, use_graph=False,
                                   sde_sample_freq=freq)
    assert col.use_sde and not col.fused_glue and col.sde_noise.shape == (8, 64, 1)
    seen = []
    orig = col._sde_resample

    def spy():
        orig()
        seen.append((col.buffer.pos, col.sde_noise.clone()))
    col._sde_resample = spy
    col.collect_rollouts()
    first = col.sde_noise.clone()
    assert [p for p, _ in seen] == ([0] if freq < 0 else [0, 2, 4])
    b = col.buffer
    with torch.no_grad():
        _, lp, _ = pol.evaluate_actions(b.obs.reshape(-1, 10, 8), b.actions.reshape(-1, 1))
    assert torch.allclose(lp, b.log_probs.reshape(-1), atol=1e-4)
    col.collect_rollouts()
    assert not torch.equal(first, col.sde_noise)          # the next rollout explores with new matrices
    tr = rollout.OnPolicyTrainer(col, n_epochs=1, batch_size=16)
    before = pol.log_std.detach().clone()
    tr.train()
    assert not torch.equal(before, pol.log_std.detach())


@pytest.mark.parametrize("version,A", [("v0", 1), ("v1", 4)])
def test_mpcrl_agent_predicts_like_the_reference_trainer(tmp_path, version, A):
    name = "ppo_v0" if version == "v0" else "ppo_v1"
    eng = _StubEngine()
    agent, meta = rollout.MPCRLAgent.from_sb3(sde_host.sb3_zip(tmp_path, name), eng)
    assert agent.version == version and agent.algorithm == "ppo" and agent.policy.action_dim == A
    obs = _obs(12, 8)
    out = agent.predict_batch(obs, deterministic=True)
    with torch.no_grad():
        mean, _, _ = agent.policy(obs, deterministic=True)
    call = eng.calls[-1]
    if version == "v0":
        assert torch.equal(call["ref_speed"], mean[:, 0].double())       # unclipped, as the reference hands it on
        assert torch.equal(call["weights"], torch.ones((12, 3), dtype=torch.float64))
    else:
        assert call["ref_speed"] is None and torch.equal(call["weights"], mean[:, :3].double())
    assert out["act"].shape == (12, 2)
    # stochastic: the reference's one matrix for every prediction; reset_noise(n) one per environment
    g = lambda: torch.Generator().manual_seed(0)
    a1 = agent.predict_batch(obs)["rl_action"]
    a2 = agent.predict_batch(obs)["rl_action"]
    assert torch.equal(a1, a2) and not torch.equal(a1, mean)
    agent.reset_noise(12, generator=g())
    a3 = agent.predict_batch(obs)["rl_action"]
    want = _numpy_sde(agent.policy, obs, Z=agent.policy.sde_noise.numpy())["sample"]
    assert np.allclose(a3.double().numpy(), want, atol=1e-5)
    single = agent.predict(obs[0].numpy())
    assert single.shape == (2,) and np.all(single == 0.25)


def test_fused_entry_point_refuses_bad_arguments():
    """mpc_policy_act_sde validates before it touches the device (no GPU needed): sizes, null pointers, and exactly one
    source of the exploration matrices."""
    import ctypes
    from mpc_rl_for_avs_amd import engine
    lib = engine.load_library()
    q = ctypes.c_void_p(64)           # never dereferenced: every call below is refused, or has B == 0
    base = [0, 4, 1, 128] + [q] * 8 + [q, 0, 0, None, None, -1, 0, 1, q, q, q, None, q, None]
    assert lib.mpc_policy_act_sde(*(base[:1] + [0] + base[2:])) == 0          # B == 0: nothing to do
    for i, bad in ((2, 9), (2, 0), (3, 258), (3, 127), (3, 0), (1, -1), (4, None), (11, None), (20, None), (24, None)):
        args = list(base)
        args[i] = bad
        assert lib.mpc_policy_act_sde(*args) == -1, (i, bad)
        assert b"mpc_policy_act_sde" in lib.mpc_last_error()
    both = list(base)
    both[15] = q                      # Z AND an epoch
    assert lib.mpc_policy_act_sde(*both) == -1
    neither = list(base)
    neither[12] = None
    assert lib.mpc_policy_act_sde(*neither) == -1
    v1_short = list(base)
    v1_short[18], v1_short[23] = 1, q                       # v1 with one action component
    assert lib.mpc_policy_act_sde(*v1_short) == -1
