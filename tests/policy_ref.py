"""TEST INFRASTRUCTURE - a plain float64 statement of the fused policy step (csrc/mpc_rollout_glue.hpp: mpc_policy_act,
mpc_policy_act_sde) and the error bars its float32 kernels are held to.

Error model.  The kernels accumulate every output in index order with one rounding per fused multiply-add, so a sum of n
terms t_k carries an error of at most n u sum |t_k| (u = 2^-24, Higham's gamma_n to first order).  Through the network:

    layer 1   s1 = b1 + x . w1        80 terms      d_s1 <= 81 u S1,                   S1 = |b1| + sum |x_i w1_ij|
              h1 = tanhf(s1)                        d_h1 <= (1 - h1^2) d_s1 + T u      (T: tanhf's error, in units of u)
    layer 2   s2 = b2 + h1 . w2       H terms       d_s2 <= (H + 1) u S2 + sum |w2_ij| d_h1_i
              h2 = tanhf(s2)                        d_h2 <= (1 - h2^2) d_s2 + T u
    heads     out = bh + h2 . wh      H terms       d_out <= (H + 1) u S3 + sum |wh_io| d_h2_i

which is the (80 + H) u growth through two tanh layers, scaled per output by the magnitudes it sums instead of a constant
1 + |ref| (pre-activations of observations in metres are sums of terms far larger than their result).  A sample adds one
rounding of |action|; gSDE's noise and variance are H-term sums with bars of the same form; the Gaussian log-probability is
a sum of A squares.  Every bar is that first-order bound times SAFETY (second-order terms, the float64 reference's own
rounding) plus a floor of 4 u (1 + |ref|).

Log-probabilities.  gSDE: the float64 log-density is evaluated at the kernel's OWN action.  The kernel forms d = action - mean
in float32, which cancels: against a reference that samples with exact noise the comparison would measure that cancellation
rather than the kernel.  The kernel's mean still differs from the float64 mean by d_mean, which moves the density by
|d| d_mean / scale^2 per component; that term is part of the bar.  Gaussian: the kernel's log-probability is
-|noise|^2 / 2 - c0, a function of the noise alone (the density at the exact sample mean + std * noise), and the reference
is that density in float64.  Evaluating it at the kernel's action instead would divide the action's rounding by std: at
log_std = -20 that is 10^9 standard deviations of nothing the kernel got wrong."""
import math

import numpy as np

U32 = 2.0 ** -24          # unit roundoff of float32
TANH_ULPS = 4.0           # tanhf's error bound in units of U32 (glibc and the device libm are within 2 ulp)
SAFETY = 2.0
LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)
SDE_EPSILON = 1e-6


def fused_weights(pol):
    """ActorCritic._fz as float32 numpy arrays (what the kernels read)."""
    pol.refresh_fused()
    return {k: np.ascontiguousarray(v.detach().cpu().numpy(), np.float32) for k, v in pol._fz.items()}


def forward(f, obs, A):
    """The fused network in float64, with its float32 error bars: obs [B, 80] -> dict(mean [B, A], value [B], latent
    [B, H], and bars mean_bar, value_bar, latent_bar)."""
    x = np.asarray(obs, np.float64).reshape(len(obs), -1)
    w1, b1, w2, b2, wh, bh = (f[k].astype(np.float64) for k in ("w1", "b1", "w2", "b2", "wh", "bh"))
    H2 = b1.size
    H = H2 // 2
    s1 = x @ w1 + b1
    h1 = np.tanh(s1)
    e1 = (1.0 - h1 ** 2) * (81 * U32 * (np.abs(x) @ np.abs(w1) + np.abs(b1))) + TANH_ULPS * U32
    s2 = h1 @ w2 + b2
    h2 = np.tanh(s2)
    # w2 is block diagonal: |h1| @ |w2| sums H terms per unit, the zero blocks add nothing
    e2 = (1.0 - h2 ** 2) * ((H + 1) * U32 * (np.abs(h1) @ np.abs(w2) + np.abs(b2)) + e1 @ np.abs(w2)) + TANH_ULPS * U32
    out = h2 @ wh + bh
    eo = (H + 1) * U32 * (np.abs(h2) @ np.abs(wh) + np.abs(bh)) + e2 @ np.abs(wh)
    return dict(mean=out[:, :A], value=out[:, A], latent=h2[:, :H], mean_bar=eo[:, :A], value_bar=eo[:, A],
                latent_bar=e2[:, :H])


def bar(first_order, ref):
    return SAFETY * first_order + 4 * U32 * (1.0 + np.abs(ref))


def map_action(act, version, clip):
    """(mpc_weights [B, 3] or None, mpc_ref_speed [B] or None) of float32 actions, as the kernels map them."""
    a = np.asarray(act, np.float32)
    c = np.clip(a, np.float32(-1.0), np.float32(1.0)) if clip else a
    c = c.astype(np.float64)
    return (c[:, :3], None) if version == "v1" else (None, c[:, 0])


def gaussian(f, obs, noise, A):
    """mpc_policy_act in float64 for the handed-in noise [B, A]: dict(actions, values, log_probs) and their bars."""
    r = forward(f, obs, A)
    n = np.asarray(noise, np.float64)
    std = f["std"].astype(np.float64)
    act = r["mean"] + std * n
    log_std = np.log(std)
    logp = -0.5 * (n * n).sum(axis=1) - log_std.sum() - A * LOG_SQRT_2PI
    # c0 is stored in float32 (its distance from the float64 constant is the input's, not the kernel's); A + 2 roundings of
    # the sum of squares, its halving and the subtraction
    c0 = float(f["c0"].reshape(-1)[0])
    logp_first = (A + 2) * U32 * (0.5 * (n * n).sum(axis=1) + abs(c0)) + abs(c0 - (log_std.sum() + A * LOG_SQRT_2PI))
    return dict(actions=act, values=r["value"], log_probs=logp,
                actions_bar=bar(r["mean_bar"] + U32 * np.abs(act), act), values_bar=bar(r["value_bar"], r["value"]),
                log_probs_bar=bar(logp_first, logp))


def sde(f, obs, Z, A, kernel_actions=None):
    """mpc_policy_act_sde in float64 for the handed-in exploration matrices Z [B, H, A]: dict(actions, values, log_probs)
    and their bars.  The log-probability is the float64 density evaluated at `kernel_actions` (the kernel's own output; the
    reference's exact sample when None)."""
    r = forward(f, obs, A)
    std = f["std"].astype(np.float64)                            # [H, A]
    Zd = np.asarray(Z, np.float64)
    E = std[None] * Zd                                           # [B, H, A]
    lat, lat_bar = r["latent"], r["latent_bar"]
    H = lat.shape[1]
    noise = np.einsum("bh,bha->ba", lat, E)
    var = (lat ** 2) @ (std ** 2)
    # E's entries are rounded once (sde_row); the sums carry H roundings of their terms and the latent's own error
    noise_first = (H + 2) * U32 * np.einsum("bh,bha->ba", np.abs(lat), np.abs(E)) + np.einsum("bh,bha->ba", lat_bar, np.abs(E))
    var_first = (H + 3) * U32 * var + (2 * np.abs(lat) * lat_bar) @ (std ** 2)
    act = r["mean"] + noise
    act_first = r["mean_bar"] + noise_first + U32 * np.abs(act)
    at = act if kernel_actions is None else np.asarray(kernel_actions, np.float64)
    scale2 = var + SDE_EPSILON
    d = at - r["mean"]
    logp = (-(d * d) / (2.0 * scale2) - 0.5 * np.log(scale2) - LOG_SQRT_2PI).sum(axis=1)
    # the kernel's d is (its action) - (its mean): against the float64 mean it is off by the mean's error; its scale by the
    # variance's; logf, sqrtf and the divisions round once each (a few u of every term)
    dd = np.abs(d)
    logp_first = (dd * r["mean_bar"] / scale2 + (d * d / (2 * scale2) + 0.5) * var_first / scale2 +
                  8 * U32 * (d * d / (2 * scale2) + np.abs(0.5 * np.log(scale2)) + LOG_SQRT_2PI)).sum(axis=1)
    return dict(actions=act, values=r["value"], log_probs=logp, noise=noise, variance=var,
                actions_bar=bar(act_first, act), values_bar=bar(r["value_bar"], r["value"]), log_probs_bar=bar(logp_first, logp))


def check(got, want, name):
    """Asserts |got - want| <= bar elementwise; returns the worst ratio error / bar (for the record of measured errors)."""
    g = np.asarray(got, np.float64)
    w, b = want[name], want[name + "_bar"]
    err = np.abs(g - w)
    ratio = err / b
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    assert np.all(np.isfinite(g)) and np.all(ratio <= 1.0), \
        f"{name}: |err| {err[i]:.3e} > bar {b[i]:.3e} at {i} (got {g[i]!r}, float64 {w[i]!r})"
    return float(ratio.max()), float(err.max())


# ---- the cases both policy-shape test files run -------------------------------------------------------------------------
# (hidden, action_dim, version, clip, log_std): every hidden size of the ABI's corners (1, a non-multiple of 8, one wave,
# more than one wave of layer threads, the ABI's largest 128) against every action width, v0 / v1, clip on / off and
# log_std -20 / 0 / 2
CASES = [(1, 1, "v0", True, 0.0), (1, 8, "v1", False, 2.0), (8, 2, "v0", False, -20.0), (8, 5, "v1", True, 0.0),
         (40, 3, "v1", True, 2.0), (40, 1, "v0", False, -20.0), (64, 5, "v1", False, 0.0), (64, 2, "v0", True, 2.0),
         (100, 8, "v1", True, -20.0), (100, 3, "v0", False, 2.0), (128, 8, "v1", False, 2.0), (128, 1, "v0", True, 0.0),
         (128, 3, "v1", True, -20.0)]


def case_id(c):
    return f"H{c[0]}-A{c[1]}-{c[2]}-{'clip' if c[3] else 'noclip'}-ls{c[4]:g}"


def make_policy(H, A, log_std, use_sde, seed):
    """ActorCritic(A, hidden=H) with torch's initialisation, biases moved off zero and log_std around `log_std`."""
    import torch
    from mpc_rl_for_avs_amd import rollout
    torch.manual_seed(seed)
    pol = rollout.ActorCritic(A, hidden=H, use_sde=use_sde)
    with torch.no_grad():
        for m in (pol.pi[0], pol.pi[2], pol.vf[0], pol.vf[2], pol.action_net, pol.value_net):
            m.bias.uniform_(-0.5, 0.5)
        pol.log_std.copy_(log_std + 0.2 * torch.rand(pol.log_std.shape) - 0.1)
    return pol


def make_obs(B, seed):
    """obs [B, 10, 8] float32: simulator-like observations with all ten rows present (every one of the 80 inputs, and so
    every row of w1, takes part), every fifth scaled x40 (pre-activations deep in tanh saturation), one all-zero
    (the biases alone)."""
    from mpc_rl_for_avs_amd import synth
    obs = synth.make_obs_batch(B, 9, seed=seed)
    obs[::5] *= np.float32(40.0)
    obs[min(3, B - 1)] = 0.0
    return obs


def boundary_policy(pol, version):
    """Action components 0 .. 2 of `pol` with zero weights and biases exactly on and beyond the Box(-1, 1) bounds: with zero
    noise the kernel's action is the bias itself (its sums add exact zeros), so the clip and the mapping onto the MPC's
    inputs are hit at the boundary."""
    import torch
    with torch.no_grad():
        k = 3 if version == "v1" else 1
        pol.action_net.weight[:k] = 0.0
        vals = [1.0, -1.0, float(np.nextafter(np.float32(-1.0), np.float32(-2.0)))] if version == "v1" else [1.0]
        pol.action_net.bias[:k] = torch.tensor(vals[:k])
    return pol
