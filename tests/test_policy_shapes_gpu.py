"""mpc_policy_act / mpc_policy_act_sde on the device at every hidden size and action width the ABI accepts a corner of,
against the float64 statement of tests/policy_ref.py (the cases and bars of tests/test_policy_shapes_cpu.py); the kernels'
own counter-based draws against the host build's; fused BatchedCollector rollouts at hidden 128 and 32 against the torch
step; the sizes the entry points and the collector refuse."""
import ctypes

import numpy as np
import pytest

import glue_host
import policy_ref as pr
import sde_host

pytestmark = pytest.mark.gpu

ENV_OFFSET = 1000


def _launch(lib, pol, obs, noise=None, Z=None, draw=None, version="v0", clip=True, env_offset=ENV_OFFSET):
    """One mpc_policy_act (use_sde False) or mpc_policy_act_sde launch on device tensors -> dict of host numpy arrays.
    Gaussian: noise [B, A] read, or draw = (seed, step) drawn and written back (o["noise"]).  gSDE: Z [B, H, A] read, or
    draw = (seed, epoch, step, freq)."""
    import torch
    dev = obs.device
    f, A, B = pol._fz, pol.action_dim, obs.shape[0]
    H2 = f["b1"].numel()
    z = lambda *sh, dt=torch.float32: torch.zeros(sh, dtype=dt, device=dev)
    o = dict(act=z(B, A), val=z(B), logp=z(B), w=torch.full((B, 3), float("nan"), dtype=torch.float64, device=dev),
             rs=torch.full((B,), float("nan"), dtype=torch.float64, device=dev))
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    i64 = lambda v: torch.tensor([v], dtype=torch.int64, device=dev)
    v1 = version == "v1"
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    if pol.use_sde:
        ep = None if draw is None else i64(draw[1])
        st = None if draw is None else i64(draw[2])
        rc = lib.mpc_policy_act_sde(dev.index, B, A, H2, p(obs), p(f["w1"]), p(f["b1"]), p(f["w2"]), p(f["b2"]), p(f["wh"]),
                                    p(f["bh"]), p(f["std"]), p(Z), 0 if draw is None else draw[0], env_offset, p(ep), p(st),
                                    -1 if draw is None else draw[3], 1 if v1 else 0, 1 if clip else 0, p(o["act"]), p(o["val"]),
                                    p(o["logp"]), p(o["w"]) if v1 else None, None if v1 else p(o["rs"]), stream)
    else:
        nz = noise.clone() if draw is None else torch.full((B, A), float("nan"), device=dev)
        rc = lib.mpc_policy_act(dev.index, B, A, H2, p(obs), p(f["w1"]), p(f["b1"]), p(f["w2"]), p(f["b2"]), p(f["wh"]),
                                p(f["bh"]), p(f["std"]), p(f["c0"]), p(nz), 0 if draw is None else draw[0], env_offset,
                                None if draw is None else p(i64(draw[1])), 1 if v1 else 0, 1 if clip else 0, p(o["act"]),
                                p(o["val"]), p(o["logp"]), p(o["w"]) if v1 else None, None if v1 else p(o["rs"]), stream)
        o["noise"] = nz
    assert rc == 0, lib.mpc_last_error()
    torch.cuda.synchronize(dev)
    out = {k: v.cpu().numpy() for k, v in o.items()}
    return dict(actions=out["act"], values=out["val"], log_probs=out["logp"], weights=out["w"], ref_speed=out["rs"],
                noise=out.get("noise"))


def _check_against_float64(got, want, version, clip, worst):
    for k in ("actions", "values", "log_probs"):
        r, e = pr.check(got[k], want, k)
        worst[k] = max(worst.get(k, (0.0, 0.0)), (r, e))
    w, rs = pr.map_action(got["actions"], version, clip)
    if version == "v1":
        assert np.array_equal(got["weights"], w) and np.isnan(got["ref_speed"]).all()
    else:
        assert np.array_equal(got["ref_speed"], rs) and np.isnan(got["weights"]).all()


def _ulps(a, b):
    """|a - b| in float32 units in the last place (same-sign finite values)."""
    ia, ib = np.asarray(a, np.float32).view(np.int32).astype(np.int64), np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    assert np.array_equal(np.signbit(a), np.signbit(b))
    return np.abs(ia - ib)


# the kernels' Box-Muller draws (double log / sqrt / cos, rounded to float32) against the host build's (glibc): measured on an
# MI355X, 0 ulp in every case below (the Gaussian noise written back at 4 steps, the gSDE matrices through a probe policy at
# 2 (freq, step) pairs, 4099 environments each), so bit equality is required; two libms could differ by one float32 ulp at
# most, which a change of either would show here
MAX_DRAW_ULPS = 0


@pytest.mark.parametrize("use_sde", [False, True], ids=["gaussian", "sde"])
@pytest.mark.parametrize("case", pr.CASES, ids=pr.case_id)
def test_policy_step_on_the_device_against_float64(case, use_sde):
    import torch
    from mpc_rl_for_avs_amd import engine
    dev = torch.device("cuda", 0)
    lib = engine.load_library()
    H, A, version, clip, log_std = case
    pol = pr.make_policy(H, A, log_std, use_sde=use_sde, seed=H * 10 + A + 2).to(dev)
    f = pr.fused_weights(pol)
    worst = {}
    for B in (1, 3, 4099):
        obs = pr.make_obs(B, seed=H + A + B)
        obs_d = torch.from_numpy(obs).to(dev)
        rng = np.random.default_rng(H * A + B)
        if use_sde:
            Z = rng.standard_normal((B, H, A)).astype(np.float32)
            got = _launch(lib, pol, obs_d, Z=torch.from_numpy(Z).to(dev), version=version, clip=clip)
            want = pr.sde(f, obs.reshape(B, -1), Z, A, kernel_actions=got["actions"])
        else:
            noise = rng.standard_normal((B, A)).astype(np.float32)
            got = _launch(lib, pol, obs_d, noise=torch.from_numpy(noise).to(dev), version=version, clip=clip)
            assert np.array_equal(got["noise"], noise)                  # handed-in noise is read, not overwritten
            want = pr.gaussian(f, obs.reshape(B, -1), noise, A)
        _check_against_float64(got, want, version, clip, worst)
    print(f"[policy {pr.case_id(case)} {'sde' if use_sde else 'gaussian'}] worst err/bar (err): " +
          ", ".join(f"{k} {r:.3f} ({e:.2e})" for k, (r, e) in worst.items()))


@pytest.mark.parametrize("case", [pr.CASES[i] for i in (0, 4, 8, 10)], ids=pr.case_id)
def test_drawn_noise_equals_the_host_draws(case):
    """The kernels' own draws for (seed, global environment env_offset + b, step / epoch): the Gaussian noise written back
    against policy_noise of the host build, and gSDE steps across epochs (sde_sample_freq -1 and 3) against the same kernel
    fed the host build's matrices."""
    import torch
    from mpc_rl_for_avs_amd import engine
    dev = torch.device("cuda", 0)
    lib = engine.load_library()
    H, A, version, clip, log_std = case
    B, seed = 4099, 0xFEEDFACECAFE1234
    obs = pr.make_obs(B, seed=11)
    obs_d = torch.from_numpy(obs).to(dev)
    pol = pr.make_policy(H, A, log_std, use_sde=False, seed=3).to(dev)
    pol.refresh_fused()
    worst = 0
    for step in (0, 1, 7, 123456789):
        got = _launch(lib, pol, obs_d, draw=(seed, step), version=version, clip=clip)
        host = glue_host.policy_act(pol, obs, np.zeros((B, A), np.float32), version, clip, draw=(seed, ENV_OFFSET, step))
        worst = max(worst, int(_ulps(got["noise"], host["noise"]).max()))
        # the sample is the one the read path makes of the written-back noise
        again = _launch(lib, pol, obs_d, noise=torch.from_numpy(got["noise"]).to(dev), version=version, clip=clip)
        assert np.array_equal(again["actions"], got["actions"]) and np.array_equal(again["log_probs"], got["log_probs"])
    print(f"[draws {pr.case_id(case)}] gaussian noise: max {worst} ulp device vs host")
    assert worst <= MAX_DRAW_ULPS
    pol = pr.make_policy(H, A, log_std, use_sde=True, seed=4).to(dev)
    f = pr.fused_weights(pol)
    n_equal = n_rows = 0
    for freq in (-1, 3):
        for step in range(7):
            epoch = 5
            got = _launch(lib, pol, obs_d, draw=(seed, epoch, step, freq), version=version, clip=clip)
            Z = np.stack([sde_host.sde_noise(seed, ENV_OFFSET + b, epoch, H, A, step=step, freq=freq) for b in range(B)])
            read = _launch(lib, pol, obs_d, Z=torch.from_numpy(Z).to(dev), version=version, clip=clip)
            same = (got["actions"] == read["actions"]).all(axis=1) & (got["log_probs"] == read["log_probs"])
            n_equal, n_rows = n_equal + int(same.sum()), n_rows + B
            # where a draw differs by an ulp the step is still the float64 step of the host's matrices
            want = pr.sde(f, obs.reshape(B, -1), Z, A, kernel_actions=got["actions"])
            pr.check(got["actions"], want, "actions")
            pr.check(got["log_probs"], want, "log_probs")
            assert np.array_equal(got["values"], read["values"])
    print(f"[draws {pr.case_id(case)}] gsde: {n_equal}/{n_rows} steps bit-equal to the host build's matrices")
    if MAX_DRAW_ULPS == 0 or worst == 0:
        assert n_equal == n_rows
    # the exploration matrices themselves, entry by entry: the kernel never writes Z out, so a probe policy makes the action
    # equal to row h of it (below); first fed the host's matrices (the probe is exact), then drawing its own
    worst_z = 0
    for freq, step in ((-1, 0), (3, 5)):
        Z = np.stack([sde_host.sde_noise(seed, ENV_OFFSET + b, 5, H, A, step=step, freq=freq) for b in range(B)])
        Zd = torch.from_numpy(Z).to(dev)
        for h in range(H):
            probe = _sde_row_probe(H, A, h, dev)
            read = _launch(lib, probe, obs_d, Z=Zd, version=version, clip=clip)
            assert np.array_equal(read["actions"], Z[:, h]), h
            got = _launch(lib, probe, obs_d, draw=(seed, 5, step, freq), version=version, clip=clip)
            worst_z = max(worst_z, int(_ulps(got["actions"], Z[:, h]).max()))
    print(f"[draws {pr.case_id(case)}] gsde Z: max {worst_z} ulp device vs host ({2 * B * H * A} entries)")
    assert worst_z <= MAX_DRAW_ULPS


def _sde_row_probe(H, A, h, dev):
    """ActorCritic(use_sde=True) whose action is row h of the exploration matrix Z, exactly: zero action head (mean 0),
    std = exp(0) = 1 (E = Z), layer-2 weights of the policy tower zero and its biases 100 at unit h, 0 elsewhere, so that the
    latent is (tanhf(100) = 1 at h, tanhf(0) = 0 elsewhere) whatever the observation, and latent @ E = Z[h] with exact sums."""
    import torch
    from mpc_rl_for_avs_amd import rollout
    pol = rollout.ActorCritic(A, hidden=H, use_sde=True)
    with torch.no_grad():
        pol.action_net.weight.zero_()
        pol.action_net.bias.zero_()
        pol.log_std.zero_()
        pol.pi[2].weight.zero_()
        pol.pi[2].bias.zero_()
        pol.pi[2].bias[h] = 100.0
    pol = pol.to(dev)
    pol.refresh_fused()
    return pol


@pytest.mark.parametrize("use_sde", [False, True], ids=["gaussian", "sde"])
@pytest.mark.parametrize("hidden,A,version,algorithm", [(128, 5, "v1", "ppo"), (32, 1, "v0", "a2c")])
def test_fused_rollout_at_other_hidden_sizes(hidden, A, version, algorithm, use_sde):
    """A short graph-captured fused BatchedCollector rollout with ActorCritic(A, hidden): its step 0 is the torch step fed
    the same draws, to the bars of test_predict_gpu.py::test_fused_glue_step_equals_the_torch_step."""
    import torch
    from mpc_rl_for_avs_amd import engine, rollout
    dev = torch.device("cuda", 0)
    B, T, seed = 64, 4, 29
    torch.manual_seed(hidden + A)
    pol = rollout.ActorCritic(A, hidden=hidden, use_sde=use_sde, log_std_init=-1.0).to(dev)
    eng = engine.MPCEngine(horizon=20, max_iter=100)
    env = rollout.SyntheticIntersectionEnv(B, device=dev, seed=6, n_others=4)
    col = rollout.BatchedCollector(env, pol, eng, version=version, algorithm=algorithm, n_steps=T, seed=seed,
                                   sde_sample_freq=2 if use_sde else -1)
    assert col.fused_glue and col._graph is not None and col.use_sde == use_sde
    obs0 = col._last_obs.clone()
    col.collect_rollouts()
    b = col.buffer
    assert torch.equal(b.obs[0], obs0)
    if use_sde:
        # the first rollout draws from epoch 0 + its span (ceil(T / sde_sample_freq) epochs), step 0 from the first of them
        assert col._sde_span == 2
        Z = torch.from_numpy(np.stack([sde_host.sde_noise(seed, e, 2, hidden, A) for e in range(B)])).to(dev)
        a, v, lp = pol.act(obs0, noise=Z)
    else:
        noise = glue_host.policy_act(pol, obs0.cpu().numpy(), np.zeros((B, A), np.float32), version, algorithm == "ppo",
                                     draw=(seed, 0, 0))["noise"]
        a, v, lp = pol.act(obs0, noise=torch.from_numpy(noise).to(dev))
    assert torch.allclose(b.actions[0], a, atol=2e-5) and torch.allclose(b.values[0], v, atol=2e-5)
    assert torch.allclose(b.log_probs[0], lp, atol=1e-4)
    assert torch.isfinite(b.actions).all() and torch.isfinite(b.advantages).all()
    eng.close()


def test_refused_sizes():
    """2H = 258, odd 2H and A = 9 are MPC_ERR_INVALID_ARG for both entry points (before any launch); a fused collector of an
    ActorCritic with hidden 129 is refused."""
    import torch
    from mpc_rl_for_avs_amd import engine, rollout
    dev = torch.device("cuda", 0)
    lib = engine.load_library()
    x = torch.zeros(4096, device=dev)
    q = ctypes.c_void_p(x.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    gauss = [dev.index, 2, 4, 128] + [q] * 9 + [q, 0, 0, None, 1, 1, q, q, q, q, None, st]
    sde = [dev.index, 2, 4, 128] + [q] * 8 + [q, 0, 0, None, None, -1, 1, 1, q, q, q, q, None, st]
    for fn, base in ((lib.mpc_policy_act, gauss), (lib.mpc_policy_act_sde, sde)):
        for i, bad in ((3, 258), (3, 127), (3, 129), (2, 9)):
            args = list(base)
            args[i] = bad
            assert fn(*args) == -1, (fn, i, bad)
    torch.cuda.synchronize(dev)
    eng = engine.MPCEngine(horizon=20, max_iter=100)
    env = rollout.SyntheticIntersectionEnv(8, device=dev, seed=1, n_others=4)
    for use_sde in (False, True):
        pol = rollout.ActorCritic(1, hidden=129, use_sde=use_sde).to(dev)
        with pytest.raises(ValueError, match="hidden <= 128"):
            rollout.BatchedCollector(env, pol, eng, n_steps=2, fused_glue=True)
    eng.close()
