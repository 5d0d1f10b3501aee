// mpc_latency.hpp - sensing latency in front of the agent's pipeline of a closed-loop evaluation: the frame a planner gets is
// a few policy steps old.  The stage hands on the TRUE scene of `steps` policy steps ago, so the perception model and the
// tracker behind it see the old frame from where the ego was then, and what they say of a row (row_class, row_slot) keeps
// describing what the agent gets.  One launch per policy step, in front of mpc_perceive and mpc_track_rows; the update of one
// environment is written once for the kernel (mpc_delay_scene_kernel in mpc_engine.hip, the tracker's mapping: sixteen lanes
// per environment, lane l row l + 1, lane 0 also row 0 and the state) and its host build (tests/cpu_latency_harness.cpp,
// delay_env below, serially).  Both are put together from the same functions.
//
//   obs     [B][R][8] f32  the true scene of this step (mpc_synth_env.hpp's columns; row 0 the ego).  1 <= R <= 17.
//   done    [B] u8         the environment's episode ended on this step, obs is the first scene of a new one (NULL: never)
//   out     [B][R][8] f32  the scene handed on (must not alias obs)
//   stale   [B] i32        the age, in steps, of the frame handed out (may be NULL)
//
// PARAMETER: steps 0..7 whole policy steps of latency.  `refusal` below is the check.
//
// STATE per environment: frames [8][B][R][8] f32 the last eight scenes; age [B] i32 the frames pushed in this episode;
// counts [B] i64 the launches; sums [3][B] f64 the sum of stale, the sum and the maximum of the ego lag [m] - the distance
// between row 0 of obs and row 0 of out.
//
// ARITHMETIC: the frames are copied bit for bit, whatever they hold.  stale, age, counts and sums[0] are integers (sums[0] a
// sum of small integers in f64, exact).  The ego lag is f64 on the f32 positions widened exactly, products and sum without
// contraction (the pragma), then sqrt, whose last bit belongs to the library: sums[1] and sums[2] agree to rounding.
//
// THE UPDATE of environment b, in evaluation order.
//   1 clear    when reset or done[b]: age = 0.  An old episode's frame is never shown in the new one: a slot is read only if
//              it was written in this episode (step 3 reaches back at most `age` frames).  A reset launch also zeroes counts
//              and sums.
//   2 push     frames[age & 7] = obs, every row.
//   3 select   s = min(steps, age); out = frames[(age - s) & 7] bit for bit, every row, whatever its order; with s == 0 that
//              is obs itself.  stale[b] = s when given.  So the first `steps` steps of an episode show the episode's first
//              scene, growing older.
//   4 score    counts += 1; sums[0] += s; dx = x0 - ox, dy = y0 - oy with (x0, y0) of obs row 0 and (ox, oy) of out row 0,
//              all widened; e = sqrt(dx * dx + dy * dy); sums[1] += e, sums[2] = e > sums[2] ? e : sums[2].
//   5 advance  age += 1.
#pragma once

#include <math.h>
#include <stdint.h>

#include "mpc_core.hpp"

namespace mpc {
namespace lat {

constexpr int kCols = 8, kMaxRows = 17, kRing = 8, kMaxSteps = 7, kSums = 3;

struct Buffers {
    int B, R;
    const float *obs;            // [B][R][8]
    const uint8_t *done;         // [B] or NULL
    float *out;                  // [B][R][8]
    int32_t *stale;              // [B] or NULL
    float *frames;               // [8][B][R][8]
    int32_t *age;                // [B]
    int64_t *counts;             // [B]
    double *sums;                // [3][B]
};

// why the library and the host build refuse the sizes or the latency; nullptr when they accept them
inline const char *refusal(int B, int R, int steps) {
    if (B < 0 || R < 1 || R > kMaxRows) return "B >= 0, 1 <= R <= 17";
    if (steps < 0 || steps > kMaxSteps) return "0 <= steps <= 7";
    return nullptr;
}

// steps 1 and 3 of environment b, as far as they need the state: what is pushed where and what is shown
struct Pick {
    int32_t age;                 // the frames of this episode before this launch
    int32_t s;                   // the age of the frame shown
    int push, show;              // the slots written and shown; the same slot exactly when s == 0
};

// the one load of age; every lane of a group may call this before lane 0 stores
MPC_HD Pick select(const Buffers &buf, int steps, int b, bool reset) {
    const bool clear = reset || (buf.done != nullptr && buf.done[b] != 0);                   // 1
    Pick p;
    p.age = clear ? 0 : buf.age[b];
    p.s = steps < p.age ? steps : p.age;                                                     // 3
    p.push = p.age & (kRing - 1);
    p.show = (p.age - p.s) & (kRing - 1);
    return p;
}

MPC_HD size_t at(const Buffers &buf, int slot, int b, int row) {
    return (((size_t)slot * (size_t)buf.B + (size_t)b) * (size_t)buf.R + (size_t)row) * kCols;
}

// steps 2 and 3 of one row: its loads, then its stores; `fresh` and `shown` get the row of obs and the row handed out
MPC_HD void move_row(const Buffers &buf, const Pick &p, int b, int row, float *fresh, float *shown) {
    const float *in = buf.obs + ((size_t)b * buf.R + row) * kCols;
    const float *old = buf.frames + at(buf, p.show, b, row);
    for (int c = 0; c < kCols; ++c) fresh[c] = in[c];
    for (int c = 0; c < kCols; ++c) shown[c] = p.s == 0 ? fresh[c] : old[c];                 // s > 0: another slot than push
    float *keep = buf.frames + at(buf, p.push, b, row);
    float *out = buf.out + ((size_t)b * buf.R + row) * kCols;
    for (int c = 0; c < kCols; ++c) keep[c] = fresh[c];
    for (int c = 0; c < kCols; ++c) out[c] = shown[c];
}

// step 4's ego lag
MPC_HD double lag(float x0, float y0, float ox, float oy) {
#pragma clang fp contract(off)
    const double dx = (double)x0 - (double)ox, dy = (double)y0 - (double)oy;
    const double a = dx * dx, c = dy * dy;
    return sqrt(a + c);
}

// steps 3 (stale), 4 and 5: the state's owner alone, after row 0 was moved
MPC_HD void keep_state(const Buffers &buf, const Pick &p, int b, bool reset, const float *fresh0, const float *shown0) {
#pragma clang fp contract(off)
    const size_t B = (size_t)buf.B;
    const double e = lag(fresh0[1], fresh0[2], shown0[1], shown0[2]);
    const int64_t n = reset ? 0 : buf.counts[b];
    const double stale = reset ? 0.0 : buf.sums[b], sum = reset ? 0.0 : buf.sums[B + b], top = reset ? 0.0 : buf.sums[2 * B + b];
    if (buf.stale != nullptr) buf.stale[b] = p.s;
    buf.counts[b] = n + 1;
    buf.sums[b] = stale + (double)p.s;
    buf.sums[B + b] = sum + e;
    buf.sums[2 * B + b] = e > top ? e : top;
    buf.age[b] = p.age + 1;                                                                   // 5
}

// one environment, serially: the host build, and the statement the kernel's lanes split between them
MPC_HD void delay_env(const Buffers &buf, int steps, int b, bool reset) {
    const Pick p = select(buf, steps, b, reset);
    float fresh[kCols], shown[kCols], fresh0[kCols], shown0[kCols];
    move_row(buf, p, b, 0, fresh0, shown0);
    for (int i = 1; i < buf.R; ++i) move_row(buf, p, b, i, fresh, shown);
    keep_state(buf, p, b, reset, fresh0, shown0);
}

}  // namespace lat
}  // namespace mpc
