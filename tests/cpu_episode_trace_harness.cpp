// Host build of mpc-rl_for_avs_amd/csrc/mpc_episode_trace.hpp for tests only (-m "not gpu"): the two launches of
// mpc_episode_trace on the CPU, with the argument list of the entry point minus device and stream and the entry point's
// argument checks.  The claim is a plain loop in index order; the frame launch is the header's step_env per environment with
// one lane and no barrier.  Against a plain-Python restatement of the model and the evaluator's numpy path
// (tests/test_episode_trace_cpu.py).  Never loaded by the product.  tests/episode_trace_san_main.cpp includes this file.
#include <cstdint>

#include "../mpc-rl_for_avs_amd/csrc/mpc_episode_trace.hpp"

namespace {
struct NoBarrier {
    void operator()(int) const {}
};
}  // namespace

extern "C" int episode_trace_step(int B, int R, int Q, int W, int C, int keep, int reset, const float *terminal_obs,
                                  const float *obs, const float *seen, const double *action, const float *reward,
                                  const uint8_t *done, const uint8_t *truncated, const uint8_t *crashed, const uint8_t *arrived,
                                  const int32_t *status, const int32_t *iters, int32_t *state_i32, float *ring_scene,
                                  float *ring_seen, double *ring_act, float *ring_reward, int32_t *ring_i32, int32_t *slot,
                                  float *kept_scene, float *kept_seen, double *kept_act, float *kept_reward, int32_t *kept_i32,
                                  int32_t *index, int64_t *counts) {
    namespace tr = mpc::trace;
    if (B < 0 || R < 1 || R > tr::kMaxRows || Q < 1 || W < 1 || W > tr::kMaxWindow || C < 1 || keep < 1 || keep > 31) return -1;
    if (!state_i32 || !ring_scene || !ring_act || !ring_reward || !ring_i32 || !slot || !kept_scene || !kept_act ||
        !kept_reward || !kept_i32 || !index || !counts)
        return -1;
    if (!obs) return -1;
    if (!reset && (!terminal_obs || !action || !reward || !done || !truncated || !crashed || !arrived || !status || !iters))
        return -1;
    if ((ring_seen != nullptr) != (kept_seen != nullptr) || (!reset && (seen != nullptr) != (ring_seen != nullptr))) return -1;
    if (B == 0) return 0;
    const tr::Recorder rec{B, R, Q, W, C, keep, state_i32, ring_scene, ring_seen, ring_act, ring_reward, ring_i32, slot,
                           kept_scene, kept_seen, kept_act, kept_reward, kept_i32, index, counts};
    const tr::StepInputs in{terminal_obs, obs, seen, action, reward, done, truncated, crashed, arrived, status, iters};
    if (reset) {
        for (int f = 0; f < tr::kCounts; ++f) counts[f] = 0;
    } else {                                                 // the claim
        const int64_t kept_before = counts[tr::kKept];
        int64_t matched = 0;
        for (int b = 0; b < B; ++b) {
            const bool sel = tr::ends_selected(rec, in, b);
            slot[b] = sel ? tr::slot_of(kept_before, matched, C) : -1;
            matched += sel ? 1 : 0;
        }
        tr::advance_counts(counts, matched, C);
    }
    for (int b = 0; b < B; ++b) tr::step_env(rec, in, b, reset != 0, 0, 1, NoBarrier{});
    return 0;
}
