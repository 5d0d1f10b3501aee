// mpc_compensate.hpp - delay compensation in front of the agent of a closed-loop evaluation: the agent's command takes effect
// `steps` policy steps after the scene it was computed from (mpc_actuator.hpp's transport delay), so the agent is handed the
// scene predicted to that moment instead.  The compensator remembers the commands still in flight, rolls the ego through
// them with the plant's own step (env::step_ego) behind the NOMINAL actuator (act::shape with gain 1, offset 0, sigma 0: lag,
// rate limit and saturation, no errors), and moves the other vehicles on with their observed velocity.  One launch per policy
// step after the scene has been sensed; the update of one environment is written once for the kernel (mpc_compensate_kernel
// in mpc_engine.hip, sixteen lanes per environment, lane l row l + 1, the ego's part by every lane) and its host build
// (tests/cpu_compensate_harness.cpp, compensate_env below, serially).  Both are put together from the same functions.
//
// OBSERVATION ONLY: reads the observation and the agent's own commands, never the simulator's or the actuator's state.
//   obs     [B][R][8] f32  presence, x, y, vx, vy, heading, sin_h, cos_h (mpc_synth_env.hpp); row 0 the ego; a row i >= 1 is
//                          PRESENT when its presence != 0.  Inputs are finite.  1 <= R <= 17.
//   command [B][2] f64     the agent's command of the step that just ran (not read in a reset launch, nor where done is set)
//   done    [B] u8         the environment's episode ended on this step, obs is the first scene of a new one (NULL: never)
//   out     [B][R][8] f32  the scene the agent acts on (must not alias obs)
//   pred    [B][4] f64     the predicted ego x, y, heading, speed (may be NULL)
//
// PARAMETERS (Params): steps 0..7 whole policy steps to look ahead (d below); latency >= 0 whole policy steps by which the
// scene handed in is old (L below; mpc_latency.hpp), steps + latency <= 7; dt > 0; per channel (0 acceleration, 1 steering) the
// nominal actuator's alpha in (0, 1], rate > 0 per second (+inf: no limit), lo <= hi.  `refusal` below is the check, written
// so that NaN fails every comparison.  mpc_compensate is latency 0; mpc_compensate_stale takes it as an argument.
//
// STATE per environment: ring [8][B][2] f64 the last eight commands (the compensator's own memory); prev [B][2] f64 the nominal
// applied action of the step before the scene shown; age [B] i32 the commands pushed in this episode; pring [8][B][2] f64 the
// predicted (x, y) of the last eight launches; counts [B] i64 the predictions scored; sums [2][B] f64 the sum and the maximum
// of the prediction error [m].
//
// ARITHMETIC: f64 on the f32 inputs widened exactly.  Steps 1, 2, 6, 7 and the counts use only + - *, comparisons and integer
// operations without contraction (the pragma), so they agree bit for bit between the kernel, the host build, the evaluator's
// CPU path and a plain-Python restatement.  The ego's rollout goes through sqrt, sin, cos, tan and atan (env::step_ego, the
// plant's function as it stands), whose last bits belong to the library: pred, the ego's row, pring and the sums agree to
// rounding.
//
// THE STALE SCENE.  Let d = steps, L = latency, n the age after the push, s = min(L, n) and m = n - s: the scene shown is the
// episode's scene after m steps (the latency stage shows the episode's first scene until L steps have passed).  With L = 0,
// s = 0 and m = n, and every statement below is the one it was before the latency existed.
//
// THE UPDATE of environment b, in evaluation order.  c runs over both channels.
//   1 clear    when reset or done[b]: the ring, prev and pring become +0.0 and age 0; no command is pushed (it belonged to the
//              old episode).  A reset launch also zeroes counts and sums.
//   2 push     otherwise, with age0 the age before: u = command[b][c]; when !(u - u == 0.0) (NaN or +-inf): u = 0.0 (the
//              actuator's step 2).  ring[age0 & 7][c] = u.  prev advances only when the scene did: when age0 >= L,
//              j = age0 - L - d, delayed = j >= 0 ? ring[j & 7][c] : +0.0 and prev[c] = shape(delayed, prev[c]) - act::shape,
//              steps 5 - 8 of mpc_actuator.hpp with gain 1, offset 0, sigma 0: the nominal applied action of the step
//              before the scene; otherwise prev is unchanged, which is +0.0 since the clear.  Then age = age0 + 1.
//   3 score    only when d + L > 0 and age >= d + L: (px, py) = pring[(age - d - L) & 7] - the prediction of launch n' targets
//              step n' + d, and the scene of that step arrives at launch n' + d + L; dx = px - x0, dy = py - y0 against row
//              0's (x, y) widened; e = sqrt(dx * dx + dy * dy); counts += 1, sums[0] += e, sums[1] = e > sums[1] ? e : sums[1].
//   4 rollout  from row 0: x = obs[1], y = obs[2], th = obs[5], sp = sqrt(vx * vx + vy * vy) of obs[3], obs[4] (|v|, as the
//              preamble reads the speed); p = prev.  d + s steps: for k = 0 .. d + s - 1: i = age - s - d + k;
//              p[c] = shape(i >= 0 ? ring[i & 7][c] : +0.0, p[c]) (i == age - 1 is the command just pushed);
//              (x, y, th, sp) = env::step_ego((x, y, th, sp), p, dt) - the plant's own function: its clamps and its speed
//              limits are part of the prediction.  pring[age & 7] = (x, y); pred[b] = (x, y, th, sp) when given.
//   5 ego row  out row 0, by the formulas of env::observe: 1, (float)x, (float)y, (float)(sp * cos th), (float)(sp * sin th),
//              (float)th, (float)sin th, (float)cos th.
//   6 others   h = (double)(d + s) * dt, formed once per environment.  Every present row i >= 1: x' = (float)(x + vx * h),
//              y' = (float)(y + vy * h) (a product, then a sum, in f64, narrowed once); presence becomes 1, velocity and the
//              three heading values are copied.
//   7 order    kx = x' - ex, ky = y' - ey, key = kx * kx + ky * ky with (ex, ey) the f32 values just written to row 0, all
//              widened.  The present rows become rows 1, 2, ... by ascending key, ties to the lower input row; the remaining
//              rows are +0.0f in all eight columns.  So "others sorted by distance, present rows contiguous" holds for what
//              the agent gets.
//   8 identity with d + L == 0 (launch arguments, hence the same for every environment) steps 5 - 7 are replaced by a copy:
//              every row of obs goes to the same row of out, bit for bit, whatever its order.  Nothing is scored; the ring,
//              prev, age, pring and pred are kept as above (the rollout has no step, so pred is the observed ego).  With
//              d + L > 0 an environment whose own look-ahead d + s is 0 is still written by the formulas of steps 5 - 7.
//
// With the delay, alpha, rate and limits of a noise-free actuator model (no gain, offset, noise or hold) `prev` at launch n
// reproduces that actuator's applied action of step n - 1 - L bit for bit, and the predicted ego is the plant's state after
// n + d steps of the episode, to the rounding of the f32 observation.
//
// TWO BUILDS.  Every function that depends on the latency takes a template constant kStale: with kStale false the latency is the
// constant 0 (`if constexpr`), which is the code mpc_compensate has always launched; with kStale true P.latency is read.
#pragma once

#include <math.h>
#include <stdint.h>

#include "mpc_actuator.hpp"
#include "mpc_core.hpp"
#include "mpc_synth_env.hpp"

namespace mpc {
namespace comp {

constexpr int kCols = 8, kMaxRows = 17, kChannels = 2, kRing = 8, kMaxSteps = 7, kSums = 2;

struct Params {
    double dt;
    double alpha[kChannels], rate[kChannels], lo[kChannels], hi[kChannels];
    int32_t steps;
    int32_t latency;             // trailing: an aggregate initialiser that stops at steps leaves it 0
};

struct Buffers {
    int B, R;
    const float *obs;            // [B][R][8]
    const double *command;       // [B][2] or NULL in a reset launch
    const uint8_t *done;         // [B] or NULL
    float *out;                  // [B][R][8]
    double *pred;                // [B][4] or NULL
    double *ring;                // [8][B][2]
    double *prev;                // [B][2]
    int32_t *age;                // [B]
    double *pring;               // [8][B][2]
    int64_t *counts;             // [B]
    double *sums;                // [2][B]
};

// why the library and the host build refuse P (each comparison written so that NaN fails it); nullptr when they accept it
inline const char *refusal(const Params &P) {
    if (P.steps < 0 || P.steps > kMaxSteps) return "0 <= steps <= 7";
    if (P.latency < 0 || P.latency > kMaxSteps - P.steps) return "0 <= latency, steps + latency <= 7";
    if (!(P.dt > 0.0)) return "dt > 0, not NaN";
    for (int c = 0; c < kChannels; ++c) {
        if (!(P.alpha[c] > 0.0 && P.alpha[c] <= 1.0)) return "0 < alpha <= 1, not NaN";
        if (!(P.rate[c] > 0.0)) return "rate > 0, not NaN (+inf: no limit)";
        if (!(P.lo[c] <= P.hi[c])) return "lo <= hi, neither NaN";
    }
    return nullptr;
}

// the nominal actuator of channel c: no calibration error, no noise (a select, so that nothing indexes the kernel's argument)
MPC_HD act::Channel nominal(const Params &P, int c) {
    return c == 0 ? act::Channel{1.0, 0.0, 0.0, P.alpha[0], P.rate[0], P.lo[0], P.hi[0]}
                  : act::Channel{1.0, 0.0, 0.0, P.alpha[1], P.rate[1], P.lo[1], P.hi[1]};
}

// act::shape of the nominal actuator; sigma is 0, so no draw is made and the generator's key does not matter
MPC_HD double shape(const Params &P, int c, double delayed, double prev) {
    bool rate_limited, saturated;
    return act::shape(nominal(P, c), P.dt, env::Rng(0, 0, 0), c, delayed, prev, rate_limited, saturated);
}

// step 3's error
MPC_HD double miss(double px, double py, float x0, float y0) {
#pragma clang fp contract(off)
    const double dx = px - (double)x0, dy = py - (double)y0;
    const double a = dx * dx, c = dy * dy;
    return sqrt(a + c);
}

// step 4's speed
MPC_HD double speed(float vx, float vy) {
#pragma clang fp contract(off)
    const double a = (double)vx * (double)vx, c = (double)vy * (double)vy;
    return sqrt(a + c);
}

// steps 1 - 4 of environment b: the predicted ego, and in `ahead` its look-ahead d + s.  Every load comes before every store,
// and the command just pushed is taken from its register, so the lanes of a group may all call this and one of them, `write`,
// keep the state.  kStale false: the latency is the constant 0.
template <bool kStale>
MPC_HD env::Ego predict_ego(const Params &P, const Buffers &buf, int b, bool reset, bool write, int &ahead) {
#pragma clang fp contract(off)
    const int B = buf.B, steps = P.steps;
    int L = 0;
    if constexpr (kStale) L = P.latency;
    const int back = steps + L;                                  // how far the push and the score reach back
    const float *row0 = buf.obs + (size_t)b * buf.R * kCols;
    const bool clear = reset || (buf.done != nullptr && buf.done[b] != 0);                   // 1
    const int32_t age0 = clear ? 0 : buf.age[b];
    int32_t age = age0;
    double u0 = 0.0, u1 = 0.0, prev0 = 0.0, prev1 = 0.0;
    if (!clear) {                                                                            // 2
        u0 = buf.command[act::at(0, B, b, 0)];
        u1 = buf.command[act::at(0, B, b, 1)];
        u0 = act::is_finite(u0) ? u0 : 0.0;
        u1 = act::is_finite(u1) ? u1 : 0.0;
        double d0 = u0, d1 = u1;                             // back == 0: the slot just pushed
        if (back > 0) {
            const int slot = (age0 - back) & (kRing - 1);    // another slot than the one pushed
            const double r0 = buf.ring[act::at(slot, B, b, 0)], r1 = buf.ring[act::at(slot, B, b, 1)];
            d0 = age0 >= back ? r0 : 0.0;
            d1 = age0 >= back ? r1 : 0.0;
        }
        if constexpr (kStale) {                              // while the scene has not moved, neither does prev
            const double q0 = buf.prev[act::at(0, B, b, 0)], q1 = buf.prev[act::at(0, B, b, 1)];
            const double y0 = shape(P, 0, d0, q0), y1 = shape(P, 1, d1, q1);
            prev0 = age0 >= L ? y0 : q0;
            prev1 = age0 >= L ? y1 : q1;
        } else {
            prev0 = shape(P, 0, d0, buf.prev[act::at(0, B, b, 0)]);
            prev1 = shape(P, 1, d1, buf.prev[act::at(0, B, b, 1)]);
        }
        age = age0 + 1;
    }
    const bool scored = back > 0 && age >= back;                                             // 3 (never after a clear)
    double err = 0.0;
    if (scored) {
        const int slot = (age - back) & (kRing - 1);
        err = miss(buf.pring[act::at(slot, B, b, 0)], buf.pring[act::at(slot, B, b, 1)], row0[1], row0[2]);
    }
    int old = 0;                                             // s: how many steps old the scene shown is
    if constexpr (kStale) old = L < age ? L : age;
    ahead = steps + old;
    env::Ego e;                                                                              // 4
    e.x = (double)row0[1], e.y = (double)row0[2], e.th = (double)row0[5], e.sp = speed(row0[3], row0[4]);
    double p[kChannels] = {prev0, prev1};
    for (int k = 0; k < ahead; ++k) {
        const int i = age - ahead + k;                       // i == age - 1 is the command just pushed (only without a clear)
        const int slot = i & (kRing - 1);
        const double r0 = buf.ring[act::at(slot, B, b, 0)], r1 = buf.ring[act::at(slot, B, b, 1)];
        const double d0 = i < 0 ? 0.0 : (i == age - 1 ? u0 : r0), d1 = i < 0 ? 0.0 : (i == age - 1 ? u1 : r1);
        p[0] = shape(P, 0, d0, p[0]);
        p[1] = shape(P, 1, d1, p[1]);
        e = env::step_ego(e, p, P.dt);
    }
    if (!write) return e;
    const int mine = age & (kRing - 1);                      // the slot of this launch's prediction
    if (clear) {
        for (int s = 0; s < kRing; ++s)
            for (int c = 0; c < kChannels; ++c) {
                buf.ring[act::at(s, B, b, c)] = 0.0;
                if (s != mine) buf.pring[act::at(s, B, b, c)] = 0.0;
            }
        if (reset) {
            buf.counts[b] = 0;
            buf.sums[b] = 0.0;
            buf.sums[(size_t)B + b] = 0.0;
        }
    } else {
        buf.ring[act::at(age0 & (kRing - 1), B, b, 0)] = u0;
        buf.ring[act::at(age0 & (kRing - 1), B, b, 1)] = u1;
    }
    buf.prev[act::at(0, B, b, 0)] = prev0;
    buf.prev[act::at(0, B, b, 1)] = prev1;
    buf.age[b] = age;
    if (scored) {
        const double top = buf.sums[(size_t)B + b];
        buf.counts[b] = buf.counts[b] + 1;
        buf.sums[b] = buf.sums[b] + err;
        buf.sums[(size_t)B + b] = err > top ? err : top;
    }
    buf.pring[act::at(mine, B, b, 0)] = e.x;
    buf.pring[act::at(mine, B, b, 1)] = e.y;
    if (buf.pred != nullptr) env::store_ego(buf.pred + (size_t)b * 4, e);
    return e;
}

// step 5
MPC_HD void ego_row(const env::Ego &e, float *row) {
    const double s = sin(e.th), c = cos(e.th);
    row[0] = 1.0f;
    row[1] = (float)e.x;
    row[2] = (float)e.y;
    row[3] = (float)(e.sp * c);
    row[4] = (float)(e.sp * s);
    row[5] = (float)e.th;
    row[6] = (float)s;
    row[7] = (float)c;
}

// step 6: one coordinate of a present row, h = (d + s) * dt
MPC_HD float advance(float x, float v, double h) {
#pragma clang fp contract(off)
    const double s = (double)v * h;
    const double n = (double)x + s;
    return (float)n;
}

// step 7: the ordering key of a moved row about the ego's written position
MPC_HD double order_key(float x, float y, float ex, float ey) {
#pragma clang fp contract(off)
    const double kx = (double)x - (double)ex, ky = (double)y - (double)ey;
    const double a = kx * kx, c = ky * ky;
    return a + c;
}

// (key_a, row a) orders before (key_b, row b)
MPC_HD bool before(double key_a, int a, double key_b, int b) { return key_a < key_b || (key_a == key_b && a < b); }

// one environment, serially: the host build, and the statement the kernel's lanes split between them
template <bool kStale = false>
MPC_HD void compensate_env(const Params &P, const Buffers &buf, int b, bool reset) {
#pragma clang fp contract(off)
    const int R = buf.R;
    const float *in = buf.obs + (size_t)b * R * kCols;
    float *out = buf.out + (size_t)b * R * kCols;
    int ahead;
    const env::Ego e = predict_ego<kStale>(P, buf, b, reset, true, ahead);   // 1 - 4
    int back = P.steps;
    if constexpr (kStale) back = P.steps + P.latency;
    if (back == 0) {                                                         // 8
        for (int i = 0; i < R * kCols; ++i) out[i] = in[i];
        return;
    }
    ego_row(e, out);                                                         // 5
    const double h = (double)ahead * P.dt;
    float moved[kMaxRows][kCols];
    double key[kMaxRows];
    bool present[kMaxRows];
    for (int i = 1; i < R; ++i) {                                            // 6
        const float *row = in + i * kCols;
        present[i] = row[0] != 0.0f;
        moved[i][0] = 1.0f;
        moved[i][1] = advance(row[1], row[3], h);
        moved[i][2] = advance(row[2], row[4], h);
        for (int c = 3; c < kCols; ++c) moved[i][c] = row[c];
        key[i] = order_key(moved[i][1], moved[i][2], out[1], out[2]);
    }
    for (int i = 1; i < R; ++i)                                              // 7
        for (int c = 0; c < kCols; ++c) out[i * kCols + c] = 0.0f;
    for (int i = 1; i < R; ++i) {
        if (!present[i]) continue;
        int rank = 0;
        for (int j = 1; j < R; ++j) rank += (present[j] && before(key[j], j, key[i], i)) ? 1 : 0;
        for (int c = 0; c < kCols; ++c) out[(1 + rank) * kCols + c] = moved[i][c];
    }
}

}  // namespace comp
}  // namespace mpc
