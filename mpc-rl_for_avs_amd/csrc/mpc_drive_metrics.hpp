// mpc_drive_metrics.hpp - safety and comfort metrics of a closed-loop evaluation, per episode, next to mpc_episode_stats.hpp:
// how close the ego got, how long it was on a collision course, how hard it braked and jerked, how well it kept its route.
// One launch per policy step after the environment's step; the update of one environment is written once for the kernel
// (mpc_drive_metrics_kernel in mpc_engine.hip, sixteen lanes per environment) and its host build
// (tests/cpu_drive_metrics_harness.cpp).  The thresholds below are this project's, not the reference's.
//
// OBSERVATION ONLY: the update reads what an observer of the environment sees, never the simulator's state, so it serves any
// environment with the reference's observation layout.  Inputs of a step:
//   terminal_obs [B][R][8] f32  the scene after the step, before the auto-reset: presence, x, y, vx, vy, heading, sin_h, cos_h;
//                               row 0 is the ego; a row i >= 1 counts when its presence != 0
//   obs          [B][R][8] f32  what the next step starts from (= terminal_obs unless done)
//   action       [B][2]   f64   acceleration, steering as handed to the environment (commanded, not clamped)
//   done         [B]      u8    the episode ended on this step
//   ref_xy       [M][2]   f64   the ego's route;  dt the step length
//
// ARITHMETIC: f64 on the f32 inputs widened exactly; only + - * / sqrt fabs and comparisons, no contraction (the pragma in
// every function: the device compiler contracts a * b + c by default), rotations by the observation's own sin_h / cos_h.  So
// the kernel, the host build, the evaluator's torch ops and a plain-Python restatement agree bit for bit.  min(a, b) is
// `b < a ? b : a`, max(a, b) is `b > a ? b : a`; nothing that is min- or max-reduced is NaN or -0.0 (finite inputs), "nothing
// there" is +inf for a minimum and 0 for a maximum.  A minimum of square roots is taken as the square root of the minimum
// (sqrt is monotone and correctly rounded: the same bits).
//
// THE FORMULAS, in evaluation order (sums left to right).  p = (x, y), vel = (vx, vy), h = (cos_h, sin_h) of terminal_obs row 0;
// q, w, g the same of a present row i >= 1; n = (-h.y, h.x), m = (-g.y, g.x); r = q - p.
//   seg2(x; e0, d)   squared distance of the point x to the segment e0 + t d, 0 <= t <= 1:
//                    s = x - e0;  dd = d.x d.x + d.y d.y;  t = 0, and if dd > 0: t = (s.x d.x + s.y d.y) / dd, t = 0 if t < 0,
//                    t = 1 if t > 1;  c = s - t d (each component: s - t * d);  seg2 = c.x c.x + c.y c.y
//   centre gap       sqrt(r.x r.x + r.y r.y)                     (the quantity of the environment's crash test)
//   box gap          between the 5.0 x 2.0 rectangles centred at p and q with axes h and g.  L = 2.5 h, W = 1.0 n (per
//                    component); corners A0 = (p + L) + W, A1 = (p - L) + W, A2 = (p - L) - W, A3 = (p + L) - W, likewise B
//                    from q, 2.5 g, 1.0 m; edge k runs from corner k to corner (k + 1) % 4, d = its end - its start.
//                    Separating axes a = h, n, g, m (unnormalised), in that order; a separates when
//                    fabs(r.x a.x + r.y a.y) > 2.5 fabs(h.a) + 1.0 fabs(n.a) + 2.5 fabs(g.a) + 1.0 fabs(m.a)
//                    (u.a = u.x a.x + u.y a.y).  No axis separates: 0.  Otherwise sqrt of the minimum of
//                    seg2(Ai; Bk, dBk) and seg2(Bi; Ak, dAk) over i, k = 0..3.
//   ttc              constant velocities, u = w - vel, D = kCrashDistance: rr = r.x r.x + r.y r.y;  0 if rr <= D D;  else
//                    a = u.x u.x + u.y u.y, b = r.x u.x + r.y u.y, c = rr - D D, disc = b b - a c;  +inf if a == 0 or b >= 0 or
//                    disc < 0;  else (-b - sqrt(disc)) / a
//   each of the three: minimum over the present rows (+inf when there is none)
//   xte              sqrt of the minimum over i = 0 .. max(M - 1, 1) - 1 of seg2(p; ref[i], ref[min(i + 1, M - 1)] - ref[i])
//                    (M == 1: the distance to the single point)
//   acceleration     ax = (vx - cvx) / dt, ay = (vy - cvy) / dt (c*: the carried values from before the step);
//                    a_lon = ax ccos + ay csin, a_lat = ay ccos - ax csin: the heading before the step
//   jerk             from the second step of an episode on: jx = (ax - cax) / dt, jy = (ay - cay) / dt, j2 = jx jx + jy jy,
//                    jerk = sqrt(j2);  steering rate, likewise: fabs(steer - csteer) / dt
//
// Running state of environment b (planar, like mpc_episode_stats):
//   state_i32 [5][B]   steps, ttc_steps (ttc < kTtcThreshold), close_steps (box gap < kCloseGap), hard_brake_steps
//                      (a_lon < -kHardBrake), episode ordinal j (saturates at the quota Q)
//   state_f64 [17][B]  min centre gap, min box gap, min ttc, max |a_lon|, max |a_lat|, sum of j2, max jerk, max steering
//                      rate, sum of xte, max xte;  then the carries vx, vy, cos_h, sin_h, ax, ay, steer
// Records, slot [b][j] for j < Q with the quota and ordinal rule of mpc_episode_stats (both see the same `done`, so slot
// [b][j] of both describes the same episode):
//   rec_i32 [4][B][Q]  steps, ttc_steps, close_steps, hard_brake_steps
//   rec_f64 [10][B][Q] min_centre_gap, min_box_gap, min_ttc, max_abs_alon, max_abs_alat, rms_jerk = sqrt(sum j2 / (steps - 1))
//                      (0 when steps < 2), max_jerk, max_steer_rate, mean_xte = sum / steps, max_xte
// Every launch ends by storing the carries: vx, vy, cos_h, sin_h of `obs` row 0 (after a done they belong to the new episode)
// and this step's ax, ay, steer.  A reset launch initialises the running state, and the carries from `obs` alone (ax, ay,
// steer = 0).
#pragma once

#include <stdint.h>

#include "mpc_core.hpp"

namespace mpc {
namespace drive {

constexpr double kHalfLength = 2.5, kHalfWidth = 1.0;    // the 5.0 m x 2.0 m vehicle
constexpr double kCrashDistance = 2.5;                   // the environment's crash test (mpc_synth_env.hpp)
constexpr double kTtcThreshold = 2.0;                    // s: a step with ttc below it is a step on a collision course
constexpr double kCloseGap = 1.0;                        // m, box gap: a near miss
constexpr double kHardBrake = 3.0;                       // m/s^2: a_lon < -kHardBrake
constexpr double kInf = __builtin_huge_val();
constexpr int kCols = 8, kMaxRows = 17, kMaxRoute = 128; // observation columns, MPC_MAX_OTHERS + 1, route points

enum { kSteps = 0, kTtcSteps = 1, kCloseSteps = 2, kHardBrakeSteps = 3, kOrdinal = 4, kStateI32 = 5 };
enum { kMinCentre = 0, kMinBox = 1, kMinTtc = 2, kMaxAlon = 3, kMaxAlat = 4, kJerkSum = 5, kMaxJerk = 6, kMaxSteerRate = 7,
       kXteSum = 8, kMaxXte = 9, kCarryVx = 10, kCarryVy = 11, kCarryCos = 12, kCarrySin = 13, kCarryAx = 14, kCarryAy = 15,
       kCarrySteer = 16, kStateF64 = 17 };
enum { kRecSteps = 0, kRecTtcSteps = 1, kRecCloseSteps = 2, kRecHardBrakeSteps = 3, kRecI32 = 4 };
enum { kRecMinCentre = 0, kRecMinBox = 1, kRecMinTtc = 2, kRecMaxAlon = 3, kRecMaxAlat = 4, kRecRmsJerk = 5, kRecMaxJerk = 6,
       kRecMaxSteerRate = 7, kRecMeanXte = 8, kRecMaxXte = 9, kRecF64 = 10 };

struct StepInputs {              // one policy step of B environments
    int R, M;
    double dt;
    const float *terminal_obs, *obs;     // [B][R][8]
    const double *action;                // [B][2]
    const uint8_t *done;                 // [B]
    const double *ref_xy;                // [M][2]
};

struct Accounts {
    int B, Q;
    int32_t *state_i32;          // [5][B]
    double *state_f64;           // [17][B]
    int32_t *rec_i32;            // [4][B][Q]
    double *rec_f64;             // [10][B][Q]
};

struct Gaps {                    // what the rows and the route contribute to one step of one environment
    double centre, box, ttc, xte2;       // minima; xte2 is the squared cross-track error
};

MPC_HD double min2(double a, double b) { return b < a ? b : a; }
MPC_HD double max2(double a, double b) { return b > a ? b : a; }

MPC_HD double seg2(double x, double y, double e0x, double e0y, double dx, double dy) {
#pragma clang fp contract(off)
    const double sx = x - e0x, sy = y - e0y;
    const double dd = dx * dx + dy * dy;
    double t = 0.0;
    if (dd > 0.0) {
        t = (sx * dx + sy * dy) / dd;
        t = t < 0.0 ? 0.0 : t;
        t = t > 1.0 ? 1.0 : t;
    }
    const double cx = sx - t * dx, cy = sy - t * dy;
    return cx * cx + cy * cy;
}

MPC_HD void corners(double px, double py, double hx, double hy, double *cx, double *cy) {
#pragma clang fp contract(off)
    const double lx = kHalfLength * hx, ly = kHalfLength * hy;
    const double wx = kHalfWidth * -hy, wy = kHalfWidth * hx;
    const double fx = px + lx, fy = py + ly, bx = px - lx, by = py - ly;
    cx[0] = fx + wx; cy[0] = fy + wy;
    cx[1] = bx + wx; cy[1] = by + wy;
    cx[2] = bx - wx; cy[2] = by - wy;
    cx[3] = fx - wx; cy[3] = fy - wy;
}

MPC_HD bool separates(double rx, double ry, double hx, double hy, double gx, double gy, double ax, double ay) {
#pragma clang fp contract(off)
    const double nx = -hy, ny = hx, mx = -gy, my = gx;
    const double reach = kHalfLength * fabs(hx * ax + hy * ay) + kHalfWidth * fabs(nx * ax + ny * ay) +
                         kHalfLength * fabs(gx * ax + gy * ay) + kHalfWidth * fabs(mx * ax + my * ay);
    return fabs(rx * ax + ry * ay) > reach;
}

// min over the corners of (c) of the squared distance to the edges of (e)
MPC_HD double corners_to_edges2(const double *cx, const double *cy, const double *ex, const double *ey) {
#pragma clang fp contract(off)
    double best = kInf;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int k1 = (k + 1) & 3;
        const double dx = ex[k1] - ex[k], dy = ey[k1] - ey[k];
#pragma unroll
        for (int i = 0; i < 4; ++i) best = min2(best, seg2(cx[i], cy[i], ex[k], ey[k], dx, dy));
    }
    return best;
}

MPC_HD double box_gap(double px, double py, double hx, double hy, double qx, double qy, double gx, double gy) {
#pragma clang fp contract(off)
    const double rx = qx - px, ry = qy - py;
    const bool apart = separates(rx, ry, hx, hy, gx, gy, hx, hy) || separates(rx, ry, hx, hy, gx, gy, -hy, hx) ||
                       separates(rx, ry, hx, hy, gx, gy, gx, gy) || separates(rx, ry, hx, hy, gx, gy, -gy, gx);
    if (!apart) return 0.0;
    double ax[4], ay[4], bx[4], by[4];
    corners(px, py, hx, hy, ax, ay);
    corners(qx, qy, gx, gy, bx, by);
    return sqrt(min2(corners_to_edges2(ax, ay, bx, by), corners_to_edges2(bx, by, ax, ay)));
}

MPC_HD double time_to_collision(double rx, double ry, double ux, double uy) {
#pragma clang fp contract(off)
    const double rr = rx * rx + ry * ry, d2 = kCrashDistance * kCrashDistance;
    if (rr <= d2) return 0.0;
    const double a = ux * ux + uy * uy, b = rx * ux + ry * uy, c = rr - d2;
    const double disc = b * b - a * c;
    if (a == 0.0 || b >= 0.0 || disc < 0.0) return kInf;
    return (-b - sqrt(disc)) / a;
}

// observation row `row` (>= 1) against the ego row of the same scene, folded into g
MPC_HD void fold_row(const float *ego, const float *row, Gaps &g) {
#pragma clang fp contract(off)
    if (row[0] == 0.0f) return;
    const double px = ego[1], py = ego[2], vx = ego[3], vy = ego[4], hy = ego[6], hx = ego[7];
    const double qx = row[1], qy = row[2], wx = row[3], wy = row[4], gy = row[6], gx = row[7];
    const double rx = qx - px, ry = qy - py;
    g.centre = min2(g.centre, sqrt(rx * rx + ry * ry));
    g.box = min2(g.box, box_gap(px, py, hx, hy, qx, qy, gx, gy));
    g.ttc = min2(g.ttc, time_to_collision(rx, ry, wx - vx, wy - vy));
}

// route segment i (0 <= i < max(M - 1, 1)) against the ego of the scene
MPC_HD void fold_segment(const float *ego, const double *ref_xy, int M, int i, Gaps &g) {
#pragma clang fp contract(off)
    const int i1 = i + 1 < M ? i + 1 : M - 1;
    const double e0x = ref_xy[2 * i], e0y = ref_xy[2 * i + 1];
    g.xte2 = min2(g.xte2, seg2(ego[1], ego[2], e0x, e0y, ref_xy[2 * i1] - e0x, ref_xy[2 * i1 + 1] - e0y));
}

// the sequential part, environment b: g holds the step's minima over rows and segments (unused on a reset launch)
MPC_HD void episode_update(const Accounts &a, const StepInputs &in, int b, bool reset, const Gaps &g) {
#pragma clang fp contract(off)
    const size_t B = (size_t)a.B;
    int32_t *si = a.state_i32 + b;          // field f of environment b at si[f * B]
    double *sf = a.state_f64 + b;
    const float *next = in.obs + (size_t)b * in.R * kCols;
    double ax = 0.0, ay = 0.0, steer = 0.0;
    bool clear = reset;
    int32_t ordinal = 0;
    if (!reset) {
        const float *ego = in.terminal_obs + (size_t)b * in.R * kCols;
        const double dt = in.dt;
        const int32_t steps = si[kSteps * B] + 1;
        ax = ((double)ego[3] - sf[kCarryVx * B]) / dt;
        ay = ((double)ego[4] - sf[kCarryVy * B]) / dt;
        steer = in.action[(size_t)b * 2 + 1];
        const double ccos = sf[kCarryCos * B], csin = sf[kCarrySin * B];
        const double alon = ax * ccos + ay * csin, alat = ay * ccos - ax * csin;
        const double xte = sqrt(g.xte2);
        const int32_t ttc_steps = si[kTtcSteps * B] + (g.ttc < kTtcThreshold ? 1 : 0);
        const int32_t close_steps = si[kCloseSteps * B] + (g.box < kCloseGap ? 1 : 0);
        const int32_t brake_steps = si[kHardBrakeSteps * B] + (alon < -kHardBrake ? 1 : 0);
        const double min_centre = min2(sf[kMinCentre * B], g.centre), min_box = min2(sf[kMinBox * B], g.box);
        const double min_ttc = min2(sf[kMinTtc * B], g.ttc);
        const double max_alon = max2(sf[kMaxAlon * B], fabs(alon)), max_alat = max2(sf[kMaxAlat * B], fabs(alat));
        double jerk_sum = sf[kJerkSum * B], max_jerk = sf[kMaxJerk * B], max_rate = sf[kMaxSteerRate * B];
        if (steps >= 2) {
            const double jx = (ax - sf[kCarryAx * B]) / dt, jy = (ay - sf[kCarryAy * B]) / dt;
            const double j2 = jx * jx + jy * jy;
            jerk_sum = jerk_sum + j2;
            max_jerk = max2(max_jerk, sqrt(j2));
            max_rate = max2(max_rate, fabs(steer - sf[kCarrySteer * B]) / dt);
        }
        const double xte_sum = sf[kXteSum * B] + xte, max_xte = max2(sf[kMaxXte * B], xte);
        const int32_t j = si[kOrdinal * B];
        ordinal = j;
        if (in.done[b]) {
            if (j < a.Q) {
                const size_t r = (size_t)b * a.Q + j, BQ = B * a.Q;
                a.rec_i32[kRecSteps * BQ + r] = steps;
                a.rec_i32[kRecTtcSteps * BQ + r] = ttc_steps;
                a.rec_i32[kRecCloseSteps * BQ + r] = close_steps;
                a.rec_i32[kRecHardBrakeSteps * BQ + r] = brake_steps;
                a.rec_f64[kRecMinCentre * BQ + r] = min_centre;
                a.rec_f64[kRecMinBox * BQ + r] = min_box;
                a.rec_f64[kRecMinTtc * BQ + r] = min_ttc;
                a.rec_f64[kRecMaxAlon * BQ + r] = max_alon;
                a.rec_f64[kRecMaxAlat * BQ + r] = max_alat;
                a.rec_f64[kRecRmsJerk * BQ + r] = steps >= 2 ? sqrt(jerk_sum / (double)(steps - 1)) : 0.0;
                a.rec_f64[kRecMaxJerk * BQ + r] = max_jerk;
                a.rec_f64[kRecMaxSteerRate * BQ + r] = max_rate;
                a.rec_f64[kRecMeanXte * BQ + r] = xte_sum / (double)steps;
                a.rec_f64[kRecMaxXte * BQ + r] = max_xte;
                ordinal = j + 1;                 // j == Q: idle, steps with the batch, writes nothing
            }
            clear = true;
        } else {
            si[kSteps * B] = steps;
            si[kTtcSteps * B] = ttc_steps;
            si[kCloseSteps * B] = close_steps;
            si[kHardBrakeSteps * B] = brake_steps;
            sf[kMinCentre * B] = min_centre;
            sf[kMinBox * B] = min_box;
            sf[kMinTtc * B] = min_ttc;
            sf[kMaxAlon * B] = max_alon;
            sf[kMaxAlat * B] = max_alat;
            sf[kJerkSum * B] = jerk_sum;
            sf[kMaxJerk * B] = max_jerk;
            sf[kMaxSteerRate * B] = max_rate;
            sf[kXteSum * B] = xte_sum;
            sf[kMaxXte * B] = max_xte;
        }
    }
    if (clear) {
        for (int f = 0; f < kOrdinal; ++f) si[f * B] = 0;
        si[kOrdinal * B] = ordinal;
        for (int f = kMinCentre; f <= kMinTtc; ++f) sf[f * B] = kInf;
        for (int f = kMaxAlon; f <= kMaxXte; ++f) sf[f * B] = 0.0;
    }
    sf[kCarryVx * B] = next[3];
    sf[kCarryVy * B] = next[4];
    sf[kCarryCos * B] = next[7];
    sf[kCarrySin * B] = next[6];
    sf[kCarryAx * B] = ax;
    sf[kCarryAy * B] = ay;
    sf[kCarrySteer * B] = steer;
}

// one environment, serially: the host build, and the statement the kernel's lanes split between them
MPC_HD void update_env(const Accounts &a, const StepInputs &in, int b, bool reset) {
    Gaps g{kInf, kInf, kInf, kInf};
    if (!reset) {
        const float *ego = in.terminal_obs + (size_t)b * in.R * kCols;
        for (int i = 1; i < in.R; ++i) fold_row(ego, ego + i * kCols, g);
        const int nseg = in.M > 1 ? in.M - 1 : 1;
        for (int i = 0; i < nseg; ++i) fold_segment(ego, in.ref_xy, in.M, i, g);
    }
    episode_update(a, in, b, reset, g);
}

}  // namespace drive
}  // namespace mpc
