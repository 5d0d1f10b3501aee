// Host build of the gSDE policy step of mpc-rl_for_avs_amd/csrc/mpc_rollout_glue.hpp for tests only (-m "not gpu"): the per-thread
// code of mpc_policy_act_sde looped over environments and threads on the CPU, against ActorCritic(use_sde=True).act in
// tests/test_sde_cpu.py.  Never loaded by the product.
#include <cmath>
#include <cstdint>
#include <vector>

#include "../mpc-rl_for_avs_amd/csrc/mpc_rollout_glue.hpp"

// sde_noise [B][H][A] read (sde_epoch == nullptr) or, with sde_epoch given, drawn as the kernel draws it and left in sde_noise
extern "C" int glue_policy_act_sde(int B, int A, int H2, const float *obs, const float *w1, const float *b1, const float *w2,
                                   const float *b2, const float *wh, const float *bh, const float *sde_std, float *sde_noise,
                                   uint64_t noise_seed, int env_offset, const int64_t *sde_epoch, const int64_t *sde_step,
                                   int sde_sample_freq, int version_v1, int clip, float *actions, float *values, float *log_probs,
                                   double *mpc_weights, double *mpc_ref_speed) {
    namespace glue = mpc::glue;
    if (A < 1 || A > glue::kMaxAction || H2 < 2 || H2 > glue::kMaxHidden2 || (H2 & 1)) return 1;
    const glue::PolicyWeights W{w1, b1, w2, b2, wh, bh, sde_std, nullptr};
    const int H = H2 / 2;
    std::vector<float> h1((size_t)H2), h2((size_t)H2), head((size_t)A + 1), e((size_t)H * A), sums(2 * (size_t)A);
    for (int b = 0; b < B; ++b) {
        const float *x = obs + (size_t)b * glue::kObsDim;
        for (int j = 0; j < H; ++j) {                                   // the kernel: thread j < H
            float *z = sde_noise + ((size_t)b * H + j) * A;
            if (sde_epoch) {
                const long long ep = glue::sde_draw_epoch(*sde_epoch, sde_step ? *sde_step : 0, sde_sample_freq);
                for (int a = 0; a < A; ++a) z[a] = glue::sde_noise(noise_seed, env_offset + b, ep, j * A + a);
            }
            glue::sde_row(W.std, A, j, z, e.data() + (size_t)j * A);
        }
        for (int j = 0; j < H2; ++j) h1[(size_t)j] = glue::layer1_unit(W, H2, x, j);
        for (int j = 0; j < H2; ++j) h2[(size_t)j] = glue::layer2_unit(W, H2, h1.data(), j);
        for (int o = 0; o <= A; ++o) head[(size_t)o] = glue::head_unit(W, H2, A, h2.data(), o);
        for (int o = 0; o < 2 * A; ++o) sums[(size_t)o] = glue::sde_sum(W.std, H, A, h2.data(), e.data(), o);
        glue::finish_action_sde(A, head.data(), sums.data(), version_v1, clip, nullptr, actions + (size_t)b * A, values + b,
                                log_probs + b, version_v1 && mpc_weights ? mpc_weights + (size_t)b * 3 : nullptr,
                                !version_v1 && mpc_ref_speed ? mpc_ref_speed + b : nullptr);
    }
    return 0;
}

// the kernel's counter-based draws alone: out [n] = Z entries k = 0 .. n - 1 of environment `env` at the epoch a step draws from
extern "C" void glue_sde_noise(uint64_t seed, int env, int64_t epoch, int64_t step, int freq, int n, float *out) {
    const long long ep = mpc::glue::sde_draw_epoch(epoch, step, freq);
    for (int k = 0; k < n; ++k) out[k] = mpc::glue::sde_noise(seed, env, ep, k);
}
