// mpc_actuator.hpp - an actuator model between the agent and the plant of a closed-loop evaluation: what happens between
// "the agent commanded (a, delta)" and "the vehicle applied (a', delta')".  Transport delay, lost commands, calibration error,
// noise, first-order lag, rate limits and saturation.  One launch per policy step between the agent's action and the
// environment's step; the update of one environment is written once for the kernel (mpc_actuate_kernel in mpc_engine.hip,
// one lane per (environment, channel) pair) and its host build (tests/cpu_actuator_harness.cpp, actuate_env below, serially).
// Both are put together from the same per-channel functions.
//
// CHANNELS: c = 0 acceleration [m/s^2], c = 1 steering [rad].
//   command  [B][2] f64  the agent's output
//   applied  [B][2] f64  what the environment is handed (may alias command: a channel's command is read before it is written)
//   done_prev [B] u8     the environment's episode ended on the PREVIOUS step: this command is the first of a new episode
//                        (NULL: never)
//
// PARAMETERS (Params; the value that switches each off): delay 0..7 whole policy steps (0); p_hold in [0, 1] (0); gain[c] (1)
// and offset[c] (0), finite; sigma[c] >= 0, finite (0); alpha[c] in (0, 1] (1; alpha = dt / (tau + dt) for a lag of time
// constant tau); rate[c] > 0 per second (+inf); lo[c] <= hi[c] (-inf, +inf); dt > 0; seed, env_offset.  `refusal` below is the
// check, written so that NaN fails every comparison.
//
// STATE per environment: age (i32) the commands received in this episode; ctr (i64) the draw counter, which only a reset launch
// sets back; ring[8][c] the last eight commands; last[c] what reached the actuator in the previous step; prev[c] what was
// applied in the previous step.  state_f64 [10][B][2] = ring 0..7, last, prev (the lane of (b, c) reads consecutive addresses);
// age [B]; ctr [B]; counts [5][B] i64 (planar) = steps, held, rate_limited, saturated, nonfinite; sums [2][B][2] f64 = the sum
// and the maximum of |applied - command|.
//
// ARITHMETIC: f64 throughout; only + - * /, fabs, comparisons and integer operations, no exp, log or trigonometry, no
// contraction (the pragma in every function).  So the kernel, the host build, the evaluator's CPU path and a plain-Python
// restatement agree bit for bit.  The generator is mpc::env::Rng.
//
// THE UPDATE of environment b, in evaluation order, for both channels.  `cmd` is the value after step 2.
//   1 clear      when done_prev != NULL && done_prev[b] != 0: age = 0, and the ring, last and prev become +0.0.
//   2 command    u = command[b][c]; when !(u - u == 0.0) (NaN or +-inf): u = 0.0 and the environment counts one nonfinite step
//                (at most one per step, whichever channel triggers it).
//   3 delay      ring[age & 7][c] = u; delayed = age >= delay ? ring[(age - delay) & 7][c] : +0.0.
//   4 hold       draws: Rng r(seed ^ kSalt, env_offset + b, ctr); kSalt keeps them apart from the environment's and the
//                perception model's draws, which use the same seed and counter values.  When p_hold > 0 and r.u01(0) < p_hold:
//                delayed = last[c] - one draw per environment, for both channels - and the environment counts one held step.
//                Then last[c] = delayed.
//   5 calibrate  v = delayed when gain[c] == 1 && offset[c] == 0, else v = gain[c] * delayed + offset[c] (a product, then a
//                sum).  When sigma[c] != 0: v = v + sigma[c] * n(1 + 4 c), with
//                n(k) = ((u(k) + u(k+1)) + (u(k+2) + u(k+3)) - 2.0) * 1.7320508075688772, u(k) = r.u01(k): a sum of four
//                uniforms scaled to unit variance, support +-3.4642 (the formula of sense::unit_noise, restated here).
//   6 lag        y = v when alpha[c] == 1, else y = prev[c] + alpha[c] * (v - prev[c]).
//   7 rate       only when rate[c] is finite: m = rate[c] * dt, d = y - prev[c]; d > m gives y = prev[c] + m, d < -m gives
//                y = prev[c] - m; either counts rate_limited, once per environment per step.
//   8 saturate   y < lo[c] gives y = lo[c]; y > hi[c] gives y = hi[c]; either counts saturated, once per environment per step.
//   9 commit     prev[c] = y, applied[b][c] = y; sums[0][b][c] += fabs(y - cmd); sums[1][b][c] = max(itself, fabs(y - cmd));
//                after both channels age += 1, ctr += 1, steps += 1.
//
// IDENTITY: with every parameter off, applied is command bit for bit for every finite command, -0.0 included: no step
// computes anything, each one copies.
//
// A launch with reset != 0 clears the state, age, ctr, the counts and the sums of every environment, reads no command and writes
// no applied: command, done_prev and applied may all be NULL in such a launch.
#pragma once

#include <stdint.h>

#include "mpc_core.hpp"
#include "mpc_synth_env.hpp"

namespace mpc {
namespace act {

constexpr uint64_t kSalt = 0x9FB21C651E98DF25ull;        // odd; xor-ed into the seed of every draw of this header
constexpr double kUnitScale = 1.7320508075688772;        // sqrt(3): four uniforms have variance 4 / 12
constexpr int kChannels = 2, kRing = 8, kMaxDelay = 7, kLast = 8, kPrev = 9, kPlanes = 10, kSums = 2;

enum { kCntSteps = 0, kCntHeld = 1, kCntRateLimited = 2, kCntSaturated = 3, kCntNonfinite = 4, kCounts = 5 };

struct Params {
    double dt, p_hold;
    double gain[kChannels], offset[kChannels], sigma[kChannels], alpha[kChannels], rate[kChannels], lo[kChannels],
        hi[kChannels];
    uint64_t seed;
    int32_t delay, env_offset;
};

struct Buffers {
    int B;
    const double *command;       // [B][2]
    const uint8_t *done_prev;    // [B] or NULL
    double *applied;             // [B][2]
    double *state;               // [10][B][2]
    int32_t *age;                // [B]
    int64_t *ctr;                // [B]
    int64_t *counts;             // [5][B]
    double *sums;                // [2][B][2]
};

// the parameters of one channel: a select, so that a lane's channel never indexes the kernel's argument
struct Channel {
    double gain, offset, sigma, alpha, rate, lo, hi;
};

MPC_HD Channel channel(const Params &P, int c) {
    return c == 0 ? Channel{P.gain[0], P.offset[0], P.sigma[0], P.alpha[0], P.rate[0], P.lo[0], P.hi[0]}
                  : Channel{P.gain[1], P.offset[1], P.sigma[1], P.alpha[1], P.rate[1], P.lo[1], P.hi[1]};
}

// element (b, c) of plane p of a [.][B][2] array
MPC_HD size_t at(int p, int B, int b, int c) { return ((size_t)p * (size_t)B + (size_t)b) * kChannels + (size_t)c; }

MPC_HD bool is_finite(double x) {
#pragma clang fp contract(off)
    return x - x == 0.0;
}

// why the library and the host build refuse P (each comparison written so that NaN fails it); nullptr when they accept it
inline const char *refusal(const Params &P) {
    if (P.delay < 0 || P.delay > kMaxDelay) return "0 <= delay <= 7";
    if (!(P.dt > 0.0)) return "dt > 0, not NaN";
    if (!(P.p_hold >= 0.0 && P.p_hold <= 1.0)) return "0 <= p_hold <= 1, not NaN";
    for (int c = 0; c < kChannels; ++c) {
        if (!is_finite(P.gain[c]) || !is_finite(P.offset[c])) return "gain and offset finite";
        if (!(P.sigma[c] >= 0.0) || !is_finite(P.sigma[c])) return "sigma >= 0 and finite";
        if (!(P.alpha[c] > 0.0 && P.alpha[c] <= 1.0)) return "0 < alpha <= 1, not NaN";
        if (!(P.rate[c] > 0.0)) return "rate > 0, not NaN (+inf: no limit)";
        if (!(P.lo[c] <= P.hi[c])) return "lo <= hi, neither NaN";
    }
    return nullptr;
}

MPC_HD double unit_noise(const env::Rng &r, int k) {
#pragma clang fp contract(off)
    return ((r.u01(k) + r.u01(k + 1)) + (r.u01(k + 2) + r.u01(k + 3)) - 2.0) * kUnitScale;
}

// step 4's draw: one per environment
MPC_HD bool hold_draw(const Params &P, const env::Rng &r) {
#pragma clang fp contract(off)
    return P.p_hold > 0.0 && r.u01(0) < P.p_hold;
}

// steps 5 - 8 of channel c: what the actuator makes of `delayed`, the value that reached it, from `prev`, what it applied last
MPC_HD double shape(const Channel &q, double dt, const env::Rng &r, int c, double delayed, double prev, bool &rate_limited,
                    bool &saturated) {
#pragma clang fp contract(off)
    double v = delayed;                                                      // 5
    if (!(q.gain == 1.0 && q.offset == 0.0)) {
        const double g = q.gain * delayed;
        v = g + q.offset;
    }
    if (q.sigma != 0.0) {
        const double e = q.sigma * unit_noise(r, 1 + 4 * c);
        v = v + e;
    }
    double y = v;                                                            // 6
    if (q.alpha != 1.0) {
        const double w = v - prev;
        const double s = q.alpha * w;
        y = prev + s;
    }
    rate_limited = false;                                                    // 7
    if (is_finite(q.rate)) {
        const double m = q.rate * dt, d = y - prev;
        if (d > m) y = prev + m, rate_limited = true;
        if (d < -m) y = prev - m, rate_limited = true;
    }
    saturated = false;                                                       // 8
    if (y < q.lo) y = q.lo, saturated = true;
    if (y > q.hi) y = q.hi, saturated = true;
    return y;
}

// step 9's deviation
MPC_HD double deviation(double y, double cmd) {
#pragma clang fp contract(off)
    return fabs(y - cmd);
}

// a reset launch, one environment
MPC_HD void reset_env(const Buffers &buf, int b) {
    const int B = buf.B;
    for (int c = 0; c < kChannels; ++c) {
        for (int p = 0; p < kPlanes; ++p) buf.state[at(p, B, b, c)] = 0.0;
        for (int p = 0; p < kSums; ++p) buf.sums[at(p, B, b, c)] = 0.0;
    }
    buf.age[b] = 0;
    buf.ctr[b] = 0;
    for (int f = 0; f < kCounts; ++f) buf.counts[(size_t)f * B + b] = 0;
}

// one environment, serially: the host build, and the statement the kernel's two lanes split between them
MPC_HD void actuate_env(const Params &P, const Buffers &buf, int b, bool reset) {
#pragma clang fp contract(off)
    if (reset) {
        reset_env(buf, b);
        return;
    }
    const int B = buf.B;
    const bool clear = buf.done_prev != nullptr && buf.done_prev[b] != 0;    // 1
    const int32_t age = clear ? 0 : buf.age[b];
    const int64_t ctr = buf.ctr[b];
    const env::Rng r(P.seed ^ kSalt, P.env_offset + b, ctr);
    const bool held = hold_draw(P, r);                                       // 4: the one draw
    bool nonfinite = false, rate_limited = false, saturated = false;
    for (int c = 0; c < kChannels; ++c) {
        if (clear)
            for (int p = 0; p < kPlanes; ++p) buf.state[at(p, B, b, c)] = 0.0;
        double u = buf.command[at(0, B, b, c)];                              // 2
        if (!is_finite(u)) u = 0.0, nonfinite = true;
        buf.state[at(age & (kRing - 1), B, b, c)] = u;                       // 3
        double delayed = age >= P.delay ? buf.state[at((age - P.delay) & (kRing - 1), B, b, c)] : 0.0;
        if (held) delayed = buf.state[at(kLast, B, b, c)];                   // 4
        buf.state[at(kLast, B, b, c)] = delayed;
        bool limited, clipped;
        const double y = shape(channel(P, c), P.dt, r, c, delayed, buf.state[at(kPrev, B, b, c)], limited, clipped);   // 5 - 8
        rate_limited = rate_limited || limited;
        saturated = saturated || clipped;
        buf.state[at(kPrev, B, b, c)] = y;                                   // 9
        buf.applied[at(0, B, b, c)] = y;
        const double dev = deviation(y, u);
        const double top = buf.sums[at(1, B, b, c)];
        buf.sums[at(0, B, b, c)] = buf.sums[at(0, B, b, c)] + dev;
        buf.sums[at(1, B, b, c)] = dev > top ? dev : top;
    }
    buf.age[b] = age + 1;
    buf.ctr[b] = ctr + 1;
    const int64_t n[kCounts] = {1, held ? 1 : 0, rate_limited ? 1 : 0, saturated ? 1 : 0, nonfinite ? 1 : 0};
    for (int f = 0; f < kCounts; ++f) buf.counts[(size_t)f * B + b] += n[f];
}

}  // namespace act
}  // namespace mpc
