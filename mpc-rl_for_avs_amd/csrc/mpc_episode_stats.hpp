// mpc_episode_stats.hpp - per-episode accounting of a closed-loop evaluation (the reference's model comparison,
// main/model_comparison.py:40-100, for B environments stepped together).  One launch per policy step, after the environment's
// step (mpc_synth_env_step), one thread per environment; the update of one environment is `episode_update` below, shared by
// the kernel (mpc_episode_stats in mpc_engine.hip) and its host build (tests/cpu_episode_stats_harness.cpp).
//
// Running state of environment b (device memory, planar):
//   state_i32 [5][B]  steps of the current episode, crashed on any step (0 / 1), unsolved solves (not MPC_STATUS_IS_SOLVED),
//                     the largest iteration count, the episode ordinal j (saturates at the quota Q)
//   state_f64 [3][B]  sum of the speeds before each step, return (sum of the f32 rewards in f64), carry_speed
// Records, one slot [b][j] per episode of environment b (j < Q), each written by exactly one thread:
//   rec_i32 [6][B][Q] steps, success (arrived, :78), collision (crashed on any step, :75), truncated, unsolved, max_iters
//   rec_f64 [2][B][Q] average speed (speed sum / steps, :90), return
//
// The speed summed at step t is the ego speed BEFORE that step (:61 reads it before env.step).  After an auto-reset `ego`
// already holds the next episode, so every launch ends by storing ego[b][3] in carry_speed and the next launch adds that.
// A reset launch (after env.reset()) only initialises the running state and carry_speed.  Sums are sequential per
// environment in f64, so the kernel, the host build and a plain-Python restatement agree bit for bit.
#pragma once

#include <stdint.h>

#include "mpc_core.hpp"

namespace mpc {
namespace stats {

enum { kSteps = 0, kCrashed = 1, kUnsolved = 2, kMaxIters = 3, kOrdinal = 4, kStateI32 = 5 };
enum { kSpeedSum = 0, kReturn = 1, kCarrySpeed = 2, kStateF64 = 3 };
enum { kRecSteps = 0, kRecSuccess = 1, kRecCollision = 2, kRecTruncated = 3, kRecUnsolved = 4, kRecMaxIters = 5, kRecI32 = 6 };
enum { kRecAvgSpeed = 0, kRecReturn = 1, kRecF64 = 2 };

struct StepInputs {              // one policy step of B environments
    const uint8_t *done, *truncated, *crashed, *arrived;   // [B] the environment's step outputs
    const float *reward;                                   // [B]
    const double *ego;                                     // [B][4] x, y, heading, speed AFTER the step (and auto-reset)
    const int32_t *status, *iters;                         // [B] the MPC solve of this step
};

struct Accounts {
    int B, Q;
    int32_t *state_i32;          // [5][B]
    double *state_f64;           // [3][B]
    int32_t *rec_i32;            // [6][B][Q]
    double *rec_f64;             // [2][B][Q]
};

MPC_HD bool solved(int32_t st) { return st == 0 || (st >= 5 && st <= 7); }   // MPC_STATUS_IS_SOLVED

// environment b; returns true when this step wrote a record (the caller counts it)
MPC_HD bool episode_update(const Accounts &a, const StepInputs &in, int b, bool reset) {
    const size_t B = (size_t)a.B;
    int32_t *si = a.state_i32 + b;          // field f of environment b at si[f * B]
    double *sf = a.state_f64 + b;
    const double speed = in.ego[(size_t)b * 4 + 3];
    bool wrote = false;
    if (reset) {
        for (int f = 0; f < kStateI32; ++f) si[f * B] = 0;
        sf[kSpeedSum * B] = 0.0;
        sf[kReturn * B] = 0.0;
    } else {
        const int32_t steps = si[kSteps * B] + 1;
        const int32_t crashed = (si[kCrashed * B] || in.crashed[b]) ? 1 : 0;
        const int32_t unsolved = si[kUnsolved * B] + (solved(in.status[b]) ? 0 : 1);
        const int32_t it = in.iters[b], mi = si[kMaxIters * B] > it ? si[kMaxIters * B] : it;
        const double speed_sum = sf[kSpeedSum * B] + sf[kCarrySpeed * B];
        const double ret = sf[kReturn * B] + (double)in.reward[b];
        const int32_t j = si[kOrdinal * B];
        if (in.done[b]) {
            if (j < a.Q) {
                const size_t r = (size_t)b * a.Q + j, BQ = B * a.Q;
                a.rec_i32[kRecSteps * BQ + r] = steps;
                a.rec_i32[kRecSuccess * BQ + r] = in.arrived[b] ? 1 : 0;
                a.rec_i32[kRecCollision * BQ + r] = crashed;
                a.rec_i32[kRecTruncated * BQ + r] = in.truncated[b] ? 1 : 0;
                a.rec_i32[kRecUnsolved * BQ + r] = unsolved;
                a.rec_i32[kRecMaxIters * BQ + r] = mi;
                a.rec_f64[kRecAvgSpeed * BQ + r] = speed_sum / (double)steps;
                a.rec_f64[kRecReturn * BQ + r] = ret;
                wrote = true;
            }
            for (int f = 0; f < kOrdinal; ++f) si[f * B] = 0;
            si[kOrdinal * B] = j < a.Q ? j + 1 : j;          // j == Q: idle, steps with the batch, writes nothing
            sf[kSpeedSum * B] = 0.0;
            sf[kReturn * B] = 0.0;
        } else {
            si[kSteps * B] = steps;
            si[kCrashed * B] = crashed;
            si[kUnsolved * B] = unsolved;
            si[kMaxIters * B] = mi;
            sf[kSpeedSum * B] = speed_sum;
            sf[kReturn * B] = ret;
        }
    }
    sf[kCarrySpeed * B] = speed;             // the speed before the next step
    return wrote;
}

}  // namespace stats
}  // namespace mpc
