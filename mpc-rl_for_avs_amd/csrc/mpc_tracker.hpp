// mpc_tracker.hpp - a tracker between the perception model (or the true observation) and the agent of a closed-loop
// evaluation: it keeps a vehicle that vanishes from the observation for a few steps (occlusion, dropout), moves it on with
// its last velocity, smooths the noise, and gives every output row an identity (the slot behind it).  One launch per policy
// step after the perception model's; the update of one environment is written once for the kernel (mpc_track_kernel in
// mpc_engine.hip, sixteen lanes per environment, lane l both row l + 1 and slot l) and its host build
// (tests/cpu_tracker_harness.cpp, track_env below, serially).  Both are put together from the same per-slot functions.
//
// OBSERVATION ONLY: reads the measured observation, never the simulator's state.
//   meas [B][R][8] f32  presence, x, y, vx, vy, heading, sin_h, cos_h (mpc_synth_env.hpp); row 0 the ego; a row i >= 1 is
//                       PRESENT when its presence != 0.  Inputs are finite.
//   out  [B][R][8] f32  the observation the agent acts on (must not alias meas)
//   done [B] u8         the environment's episode ended on this step (NULL: never); `reset`: every environment starts anew
//
// SLOTS AND STATE: 16 track slots per environment whatever R is.  track_f64 [B][16][7] = x, y, vx, vy, heading, sin_h,
// cos_h; track_i32 [B][16][3] = alive, age, miss.
//
// PARAMETERS (Params): dt > 0; gate >= 0 [m] (+inf allowed; gate2 = gate * gate is formed once by the caller); coast 0..200
// launches a track survives unmeasured; alpha_pos, alpha_vel in (0, 1] the gains.
//
// ARITHMETIC: f64 on the f32 inputs widened exactly; only + - *, comparisons and integer operations, no contraction (the
// pragma in every function).  So the kernel, the host build, the evaluator's CPU path and a plain-Python restatement agree bit
// for bit.
//
// THE UPDATE of one environment, in evaluation order.  (mx, my, mvx, mvy, mh, ms, mc) = columns 1..7 of a row.
//   1 clear      when reset or done: the ten values of every slot become 0 (the frame that follows a done is the first scene
//                of a new episode).
//   2 predict    every alive slot: x = x + vx * dt, y = y + vy * dt (a product, then a sum).
//   3 associate  greedy, in row order i = 1 .. R - 1, present rows only.  Among the slots that are alive and not yet claimed
//                in this launch: dx = mx - x, dy = my - y, d = dx * dx + dy * dy; a slot is eligible when d <= gate2; the row
//                claims the eligible slot with the smallest d, a tie goes to the lowest slot; a row that finds none is
//                unassociated.  Rows arrive sorted by distance to the ego, so the nearest vehicles choose first.
//   4 update     a claimed slot from its row: x = x + alpha_pos * (mx - x), likewise y; vx = vx + alpha_vel * (mvx - vx),
//                likewise vy; a gain that is exactly 1 copies the measurement instead; heading, sin_h, cos_h are always copied
//                (no angle arithmetic); miss = 0, age += 1.
//   5 coast      an alive slot that was not claimed: miss += 1; when miss > coast it expires: its ten values become 0.
//   6 births     the k-th unassociated row, in row order, takes the k-th candidate slot.  Candidates: the slots that are not
//                alive, ascending, followed by the alive slots that were not claimed, ascending (taking one of those EVICTS a
//                coasting track).  There are always enough: 16 - claimed >= unassociated because R - 1 <= 16.  The slot gets
//                the row's seven values, alive = 1, age = 1, miss = 0.
//   7 output     row 0 copied from meas.  The alive slots ordered by kx = x - ex, ky = y - ey, key = kx * kx + ky * ky (ex, ey
//                of meas row 0), ties to the lowest slot; the first R - 1 become rows 1, 2, ... as 1.0f, (float)x, (float)y,
//                (float)vx, (float)vy and the three heading values, each narrowed once; every remaining row +0.0f in all
//                eight columns.  Present rows of the output are contiguous.  row_slot [B][R] u8 (may be NULL): the slot behind
//                each output row, 255 for row 0 and empty rows;  row_miss [B][R] u8 (may be NULL): that slot's miss (0 when
//                the row was measured in this launch, 0 for row 0 and empty rows).
//   8 counts     counts [7][B] i64 (planar) += measured (present rows), matched, born, coasted (output rows with miss > 0),
//                expired, evicted, cut (alive slots that did not fit into R - 1 rows).  A reset launch zeroes them first, then
//                tracks the frame like any other launch.
//
// With coast = 0 and both gains 1 every slot that is not measured expires and the output is the present input rows, bit for
// bit, in the order of `key`.  With coasting on, a vehicle hidden for k <= coast launches stays in the observation at its last
// velocity and keeps its slot when it reappears within the gate.
#pragma once

#include <stdint.h>

#include "mpc_core.hpp"

namespace mpc {
namespace track {

constexpr int kCols = 8, kMaxRows = 17, kSlots = 16, kF64 = 7, kI32 = 3, kMaxCoast = 200, kNoSlot = 255;

enum { kCntMeasured = 0, kCntMatched = 1, kCntBorn = 2, kCntCoasted = 3, kCntExpired = 4, kCntEvicted = 5, kCntCut = 6,
       kCounts = 7 };

struct Params {
    double dt, gate2, alpha_pos, alpha_vel;
    int32_t coast;
};

struct Buffers {
    int B, R;
    const float *meas;           // [B][R][8]
    const uint8_t *done;         // [B] or NULL
    float *out;                  // [B][R][8]
    uint8_t *row_slot;           // [B][R] or NULL
    uint8_t *row_miss;           // [B][R] or NULL
    double *track_f64;           // [B][16][7]
    int32_t *track_i32;          // [B][16][3]
    int64_t *counts;             // [7][B]
};

struct Slot {
    double x, y, vx, vy, heading, sin_h, cos_h;
    int32_t alive, age, miss;
};

MPC_HD Slot empty_slot() { return Slot{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0}; }

MPC_HD Slot load_slot(const Buffers &buf, int b, int s) {
    const double *f = buf.track_f64 + ((size_t)b * kSlots + s) * kF64;
    const int32_t *n = buf.track_i32 + ((size_t)b * kSlots + s) * kI32;
    return Slot{f[0], f[1], f[2], f[3], f[4], f[5], f[6], n[0], n[1], n[2]};
}

MPC_HD void store_slot(const Buffers &buf, int b, int s, const Slot &t) {
    double *f = buf.track_f64 + ((size_t)b * kSlots + s) * kF64;
    int32_t *n = buf.track_i32 + ((size_t)b * kSlots + s) * kI32;
    f[0] = t.x, f[1] = t.y, f[2] = t.vx, f[3] = t.vy, f[4] = t.heading, f[5] = t.sin_h, f[6] = t.cos_h;
    n[0] = t.alive, n[1] = t.age, n[2] = t.miss;
}

// step 2
MPC_HD void predict(const Params &P, Slot &t) {
#pragma clang fp contract(off)
    if (t.alive == 0) return;
    const double sx = t.vx * P.dt, sy = t.vy * P.dt;
    t.x = t.x + sx;
    t.y = t.y + sy;
}

// step 3: the squared distance of the measurement (mx, my) to the slot's predicted position
MPC_HD double dist2(const Slot &t, float mx, float my) {
#pragma clang fp contract(off)
    const double dx = (double)mx - t.x, dy = (double)my - t.y;
    const double a = dx * dx, c = dy * dy;
    return a + c;
}

MPC_HD double blend(double a, double alpha, double m) {
#pragma clang fp contract(off)
    if (alpha == 1.0) return m;
    const double r = m - a;
    const double g = alpha * r;
    return a + g;
}

// step 4: a claimed slot from columns 1..7 of its row
MPC_HD void update(const Params &P, Slot &t, float mx, float my, float mvx, float mvy, float mh, float ms, float mc) {
    t.x = blend(t.x, P.alpha_pos, (double)mx);
    t.y = blend(t.y, P.alpha_pos, (double)my);
    t.vx = blend(t.vx, P.alpha_vel, (double)mvx);
    t.vy = blend(t.vy, P.alpha_vel, (double)mvy);
    t.heading = mh, t.sin_h = ms, t.cos_h = mc;
    t.miss = 0;
    t.age += 1;
}

// step 5: an alive slot that was not claimed; true when it expires
MPC_HD bool coast(const Params &P, Slot &t) {
    t.miss += 1;
    if (t.miss <= P.coast) return false;
    t = empty_slot();
    return true;
}

// step 6
MPC_HD Slot born(float mx, float my, float mvx, float mvy, float mh, float ms, float mc) {
    return Slot{(double)mx, (double)my, (double)mvx, (double)mvy, (double)mh, (double)ms, (double)mc, 1, 1, 0};
}

// step 7: the ordering key of a slot for the ego at (ex, ey)
MPC_HD double order_key(const Slot &t, float ex, float ey) {
#pragma clang fp contract(off)
    const double kx = t.x - (double)ex, ky = t.y - (double)ey;
    const double a = kx * kx, c = ky * ky;
    return a + c;
}

// (key_a, slot a) orders before (key_b, slot b)
MPC_HD bool before(double key_a, int a, double key_b, int b) { return key_a < key_b || (key_a == key_b && a < b); }

MPC_HD void write_row(float *row, const Slot &t) {
    row[0] = 1.0f;
    row[1] = (float)t.x, row[2] = (float)t.y, row[3] = (float)t.vx, row[4] = (float)t.vy;
    row[5] = (float)t.heading, row[6] = (float)t.sin_h, row[7] = (float)t.cos_h;
}

// one environment, serially: the host build, and the statement the kernel's lanes split between them
MPC_HD void track_env(const Params &P, const Buffers &buf, int b, bool reset) {
    const int R = buf.R;
    const size_t B = (size_t)buf.B;
    const float *in = buf.meas + (size_t)b * R * kCols;
    float *out = buf.out + (size_t)b * R * kCols;
    const bool clear = reset || (buf.done && buf.done[b] != 0);
    Slot t[kSlots];
    bool claimed[kSlots], unassociated[kMaxRows];
    int64_t n[kCounts] = {0, 0, 0, 0, 0, 0, 0};
    for (int s = 0; s < kSlots; ++s) {
        t[s] = clear ? empty_slot() : load_slot(buf, b, s);                 // 1
        predict(P, t[s]);                                                    // 2
        claimed[s] = false;
    }
    for (int i = 1; i < R; ++i) {                                            // 3, 4
        const float *row = in + i * kCols;
        unassociated[i] = false;
        if (row[0] == 0.0f) continue;
        n[kCntMeasured] += 1;
        int best = -1;
        double best_d = 0.0;
        for (int s = 0; s < kSlots; ++s) {
            if (t[s].alive == 0 || claimed[s]) continue;
            const double d = dist2(t[s], row[1], row[2]);
            if (d <= P.gate2 && (best < 0 || d < best_d)) best = s, best_d = d;
        }
        if (best < 0) {
            unassociated[i] = true;
            continue;
        }
        claimed[best] = true;
        update(P, t[best], row[1], row[2], row[3], row[4], row[5], row[6], row[7]);
        n[kCntMatched] += 1;
    }
    for (int s = 0; s < kSlots; ++s)                                         // 5
        if (t[s].alive != 0 && !claimed[s]) n[kCntExpired] += coast(P, t[s]) ? 1 : 0;
    int cand[kSlots], n_cand = 0;                                            // 6
    for (int s = 0; s < kSlots; ++s)
        if (t[s].alive == 0) cand[n_cand++] = s;
    for (int s = 0; s < kSlots; ++s)
        if (t[s].alive != 0 && !claimed[s]) cand[n_cand++] = s;
    int k = 0;
    for (int i = 1; i < R; ++i) {
        if (!unassociated[i]) continue;
        const float *row = in + i * kCols;
        const int s = cand[k++];
        n[kCntEvicted] += t[s].alive != 0;
        t[s] = born(row[1], row[2], row[3], row[4], row[5], row[6], row[7]);
        n[kCntBorn] += 1;
    }
    for (int c = 0; c < kCols; ++c) out[c] = in[c];                          // 7
    for (int i = 1; i < R; ++i)
        for (int c = 0; c < kCols; ++c) out[i * kCols + c] = 0.0f;
    for (int i = 0; i < R; ++i) {
        if (buf.row_slot) buf.row_slot[(size_t)b * R + i] = (uint8_t)kNoSlot;
        if (buf.row_miss) buf.row_miss[(size_t)b * R + i] = 0;
    }
    double key[kSlots];
    for (int s = 0; s < kSlots; ++s) key[s] = order_key(t[s], in[1], in[2]);
    for (int s = 0; s < kSlots; ++s) {
        if (t[s].alive == 0) continue;
        int rank = 0;
        for (int u = 0; u < kSlots; ++u) rank += (t[u].alive != 0 && before(key[u], u, key[s], s)) ? 1 : 0;
        if (rank >= R - 1) {
            n[kCntCut] += 1;
            continue;
        }
        write_row(out + (1 + rank) * kCols, t[s]);
        if (buf.row_slot) buf.row_slot[(size_t)b * R + 1 + rank] = (uint8_t)s;
        if (buf.row_miss) buf.row_miss[(size_t)b * R + 1 + rank] = (uint8_t)t[s].miss;
        n[kCntCoasted] += t[s].miss > 0;
    }
    for (int s = 0; s < kSlots; ++s) store_slot(buf, b, s, t[s]);
    for (int f = 0; f < kCounts; ++f) buf.counts[f * B + b] = (reset ? 0 : buf.counts[f * B + b]) + n[f];      // 8
}

}  // namespace track
}  // namespace mpc
