// mpc_plan.hpp - the MPC's plan next to what happened, in a closed-loop evaluation: the planned trajectory X / U that
// mpc_predict_batch_plan / mpc_ltv_predict_batch_plan hand out is scored per episode (mpc_plan_metrics, beside
// mpc_drive_metrics.hpp) and kept, step by step, for the episodes the trace recorder keeps (mpc_plan_trace, the companion of
// mpc_episode_trace.hpp).  The update of one environment is written once for the kernels (mpc_plan_metrics_kernel, sixteen
// lanes per environment, and mpc_plan_trace_kernel, one workgroup per environment, in mpc_engine.hip), their host build
// (tests/cpu_plan_harness.cpp) and, statement by statement, the evaluator's numpy path (evaluate.PlanMetrics).
//
// ---- mpc_plan_metrics ---------------------------------------------------------------------------------------------------
// Inputs of step t (t = 0, 1, .. counts the steps of the episode) of environment b:
//   plan_X [B][N+1][4] f64, plan_U [B][N][2] f64, status [B] i32   the step's solve; the plan is VALID iff
//                              MPC_STATUS_IS_SOLVED(status).  An invalid plan is counted (steps, not plans_valid) and its
//                              numbers are used nowhere.
//   order                      the state order of plan_X: 0 NLP (x, y, theta, v), 1 LTV (x, y, v, yaw).  Both keep x, y in
//                              columns 0 and 1, which is all the update reads; the argument is checked and otherwise unused.
//   acted [B][R][8] f32        the observation the agent acted on: presence, x, y, vx, vy, heading, sin_h, cos_h; row 0 the ego
//   terminal_obs [B][R][8] f32 the scene after the step, before the auto-reset
//   done [B] u8, dt [s], gap [m], leads[4] (each 1..N, or 0 = unused; Lmax = the largest)
//
// ARITHMETIC: f64 on the f32 inputs widened exactly; only + - * / sqrt fabs and comparisons, no contraction (the pragma in
// every function).  min(a, b) is `b < a ? b : a`, max(a, b) is `b > a ? b : a`; a valid plan and an observation are finite, so
// nothing that is min- or max-reduced is NaN; "nothing there" is +inf for a minimum.  The minimum of square roots is taken as
// the square root of the minimum.
//
// THE UPDATE, in evaluation order.
//   1 clearance   only with a valid plan: over the stages k = 1..N and the rows j = 1..R-1 of `acted` with presence != 0:
//                 kd = (double)k * dt; qx = x_j + kd * vx_j; qy = y_j + kd * vy_j (a product, then a sum); ex = X[k][0] - qx;
//                 ey = X[k][1] - qy; d2 = ex * ex + ey * ey.  c = sqrt(min d2), +inf when there is no pair.
//                 min_plan_gap = min(itself, c); conflict_steps += c < gap.
//   2 counts      steps += 1; plans_valid += valid.
//   3 append      ring entry t mod Lmax: xy[i] = X[leads[i]][0..1] for every used lead i (an unused lead's pair is not
//                 written), valid = the plan's validity.
//   4 lead error  o = terminal_obs row 0 (x, y).  For every used lead i with h = leads[i] <= t + 1: p = t + 1 - h, the entry
//                 p mod Lmax (h <= Lmax, so it is still there; h = Lmax with Lmax = 1 reads the entry just written).  When
//                 that entry is valid: ex = o.x - xy[i][0]; ey = o.y - xy[i][1]; e = sqrt(ex * ex + ey * ey); lead_n[i] += 1;
//                 lead_sum[i] += e; lead_max[i] = max(itself, e).  The plan made at step p said where the ego would be after
//                 h steps, which is the scene after step p + h - 1 = t.
//   5 replanning  when t >= 1 and this plan and the previous one are valid: for c = 0 (acceleration), 1 (steering):
//                 j = fabs(U[0][c] - prev_u[c]); replan_sum[c] += j; replan_max[c] = max(itself, j); replan_n += 1 (once).
//                 Then prev_u = U[min(1, N - 1)], prev_valid = valid: what the plan intends for the NEXT step.
//   6 done[b]     if the ordinal j < Q: write slot [b][j] (means are sum / n, 0 when n == 0) and j += 1.  Then the running
//                 state returns to its start (below) and every ring entry's validity becomes 0 (the pairs stay: an entry is
//                 read only when it is valid and its plan belongs to this episode, h <= t + 1).
//
// Running state of environment b (planar):
//   state_i32 [10][B]  steps, plans_valid, conflict_steps, prev_valid, the ordinal j (saturates at Q: such an environment
//                      keeps updating its state and writes no record), lead_n[4], replan_n
//   state_f64 [15][B]  min_plan_gap (+inf at the start), replan_sum[2], replan_max[2], lead_sum[4], lead_max[4], prev_u[2]
//   ring_xy [B][Lmax][4][2] f64, ring_valid [B][Lmax] i32
// Records, slot [b][j] for j < Q with the quota and ordinal rule of mpc_episode_stats (the same `done`, the same slot):
//   rec_i32 [8][B][Q]   steps, plans_valid, plan_conflict_steps, replan_n, lead_n[4]
//   rec_f64 [13][B][Q]  min_plan_gap, replan_accel_mean, replan_steer_mean, replan_accel_max, replan_steer_max,
//                       lead_mean[4], lead_max[4]
// A reset launch puts the running state of every environment (the ordinal included) at its start and clears the validity of
// the ring; it reads no step input.
//
// ---- mpc_plan_trace -----------------------------------------------------------------------------------------------------
// Launched right after mpc_episode_trace on the same stream for the same step, it reads that call's work array slot [B] (the
// slot of the store an episode that ends on this step was given, else -1; mpc_episode_trace leaves it alone until its next
// call) and `done`, and keeps the plans of the last W steps of the current episode: ring_X [B][W][N+1][4], ring_U [B][W][N][2]
// f64, frame t at index t mod W.  When done[b] and 0 <= slot[b] < C the last L = min(T, W) frames go, chronologically, to
// kept_X [C][W][N+1][4] / kept_U [C][W][N][2] at that slot: kept frame i is the plan that produced the recorder's action
// frame i.  state_i32 [2][B] = steps of the current episode, the ordinal j (the recorder's rule: an environment with j >= Q
// writes nothing; done advances j).  A reset launch clears both.  The order, the capacity and the selection are the
// recorder's.  Every ring and store index is reduced to its range before use.
#pragma once

#include <stdint.h>

#include "mpc_core.hpp"
#include "mpc_episode_trace.hpp"

namespace mpc {
namespace plan {

constexpr double kInf = __builtin_huge_val();
constexpr int kCols = 8, kMaxRows = 17, kLeads = 4, kMaxHorizon = 64;    // observation columns, MPC_MAX_OTHERS + 1, MPC_MAX_HORIZON

enum { kSteps = 0, kPlansValid = 1, kConflictSteps = 2, kPrevValid = 3, kOrdinal = 4, kLeadN = 5, kReplanN = 9, kStateI32 = 10 };
enum { kMinGap = 0, kReplanSum = 1, kReplanMax = 3, kLeadSum = 5, kLeadMax = 9, kPrevU = 13, kStateF64 = 15 };
enum { kRecSteps = 0, kRecPlansValid = 1, kRecConflictSteps = 2, kRecReplanN = 3, kRecLeadN = 4, kRecI32 = 8 };
enum { kRecMinGap = 0, kRecReplanMean = 1, kRecReplanMax = 3, kRecLeadMean = 5, kRecLeadMax = 9, kRecF64 = 13 };
enum { kTraceSteps = 0, kTraceOrdinal = 1, kTraceStateI32 = 2 };

struct StepInputs {              // one policy step of B environments
    int N, R, order;
    double dt, gap;
    int32_t leads[kLeads];
    const double *plan_X, *plan_U;       // [B][N + 1][4], [B][N][2]
    const int32_t *status;               // [B]
    const float *acted, *terminal_obs;   // [B][R][8]
    const uint8_t *done;                 // [B]
};

struct Accounts {
    int B, Q, Lmax;
    int32_t *state_i32;          // [10][B]
    double *state_f64;           // [15][B]
    double *ring_xy;             // [B][Lmax][4][2]
    int32_t *ring_valid;         // [B][Lmax]
    int32_t *rec_i32;            // [8][B][Q]
    double *rec_f64;             // [13][B][Q]
};

MPC_HD double min2(double a, double b) { return b < a ? b : a; }
MPC_HD double max2(double a, double b) { return b > a ? b : a; }
MPC_HD constexpr bool solved(int32_t st) { return st == 0 || (st >= 5 && st <= 7); }   // MPC_STATUS_IS_SOLVED (checked in mpc_engine.hip)

inline int max_lead(const int32_t *leads) {
    int m = 0;
    for (int i = 0; i < kLeads; ++i) m = leads[i] > m ? leads[i] : m;
    return m;
}

// why the library and the host build refuse the sizes and parameters of a launch, one rule at a time (each comparison written
// so that NaN fails it); nullptr when they accept them
inline const char *refusal(int B, int N, int R, int Q, int order, double dt, double gap, const int32_t *leads) {
    if (B < 0) return "B >= 0";
    if (N < 1 || N > kMaxHorizon) return "1 <= N <= MPC_MAX_HORIZON";
    if (R < 1 || R > kMaxRows) return "1 <= R <= MPC_MAX_OTHERS + 1";
    if (Q < 1) return "Q >= 1";
    if (!(dt > 0.0)) return "dt > 0, not NaN";
    if (!(gap >= 0.0)) return "gap >= 0, not NaN";
    for (int i = 0; i < kLeads; ++i)
        if (leads[i] < 0 || leads[i] > N) return "every lead in 0 .. N";
    if (max_lead(leads) == 0) return "at least one lead used";
    if (order < 0 || order > 1) return "order 0 (NLP) or 1 (LTV)";
    return nullptr;
}

// step 1: pair i of the N (R - 1) (stage, row) pairs of environment b folded into the squared clearance d2
MPC_HD double fold_pair(const StepInputs &in, int b, int i, double d2) {
#pragma clang fp contract(off)
    const int rows = in.R - 1, k = 1 + i / rows, j = 1 + i % rows;
    const float *row = in.acted + ((size_t)b * in.R + j) * kCols;
    if (row[0] == 0.0f) return d2;
    const double *x = in.plan_X + ((size_t)b * (in.N + 1) + k) * 4;
    const double kd = (double)k * in.dt;
    const double qx = (double)row[1] + kd * (double)row[3], qy = (double)row[2] + kd * (double)row[4];
    const double ex = x[0] - qx, ey = x[1] - qy;
    return min2(d2, ex * ex + ey * ey);
}

// lane-strided over the pairs: the kernel passes its lane of sixteen, the host build (0, 1); +inf with an invalid plan
MPC_HD double fold_pairs(const StepInputs &in, int b, int lane, int lanes) {
    double d2 = kInf;
    if (!solved(in.status[b])) return d2;
    const int pairs = in.N * (in.R - 1);
    for (int i = lane; i < pairs; i += lanes) d2 = fold_pair(in, b, i, d2);
    return d2;
}

MPC_HD void start_state(const Accounts &a, int b, int32_t ordinal) {
    const size_t B = (size_t)a.B;
    for (int f = 0; f < kStateI32; ++f) a.state_i32[f * B + b] = f == kOrdinal ? ordinal : 0;
    for (int f = 0; f < kStateF64; ++f) a.state_f64[f * B + b] = f == kMinGap ? kInf : 0.0;
    for (int e = 0; e < a.Lmax; ++e) a.ring_valid[(size_t)b * a.Lmax + e] = 0;
}

// steps 1 (its end) to 6, environment b: d2 holds the step's squared clearance over all pairs (unused on a reset launch)
MPC_HD void episode_update(const Accounts &a, const StepInputs &in, int b, bool reset, double d2) {
#pragma clang fp contract(off)
    if (reset) {
        start_state(a, b, 0);
        return;
    }
    const size_t B = (size_t)a.B;
    int32_t *si = a.state_i32 + b;          // field f of environment b at si[f * B]
    double *sf = a.state_f64 + b;
    const unsigned L = (unsigned)a.Lmax;
    double *ring = a.ring_xy + (size_t)b * L * kLeads * 2;
    int32_t *ring_valid = a.ring_valid + (size_t)b * L;
    const double *X = in.plan_X + (size_t)b * (in.N + 1) * 4, *U = in.plan_U + (size_t)b * in.N * 2;
    const float *ego = in.terminal_obs + (size_t)b * in.R * kCols;
    const bool valid = solved(in.status[b]);
    const int32_t t = si[kSteps * B];
    if (valid) {                                                             // 1
        const double c = sqrt(d2);
        sf[kMinGap * B] = min2(sf[kMinGap * B], c);
        si[kConflictSteps * B] += c < in.gap ? 1 : 0;
    }
    si[kSteps * B] = t + 1;                                                  // 2
    si[kPlansValid * B] += valid ? 1 : 0;
    const unsigned at = (unsigned)t % L;                                     // 3
#pragma unroll
    for (int i = 0; i < kLeads; ++i)
        if (in.leads[i] > 0) {
            ring[(at * kLeads + i) * 2 + 0] = X[in.leads[i] * 4 + 0];
            ring[(at * kLeads + i) * 2 + 1] = X[in.leads[i] * 4 + 1];
        }
    ring_valid[at] = valid ? 1 : 0;
    const double ox = ego[1], oy = ego[2];                                   // 4
#pragma unroll
    for (int i = 0; i < kLeads; ++i) {
        const int32_t h = in.leads[i];
        if (h < 1 || h > t + 1) continue;
        const unsigned p = (unsigned)(t + 1 - h) % L;
        if (ring_valid[p] == 0) continue;
        const double ex = ox - ring[(p * kLeads + i) * 2 + 0], ey = oy - ring[(p * kLeads + i) * 2 + 1];
        const double e = sqrt(ex * ex + ey * ey);
        si[(kLeadN + i) * B] += 1;
        sf[(kLeadSum + i) * B] = sf[(kLeadSum + i) * B] + e;
        sf[(kLeadMax + i) * B] = max2(sf[(kLeadMax + i) * B], e);
    }
    if (t >= 1 && valid && si[kPrevValid * B] != 0) {                        // 5
        for (int c = 0; c < 2; ++c) {
            const double j = fabs(U[c] - sf[(kPrevU + c) * B]);
            sf[(kReplanSum + c) * B] = sf[(kReplanSum + c) * B] + j;
            sf[(kReplanMax + c) * B] = max2(sf[(kReplanMax + c) * B], j);
        }
        si[kReplanN * B] += 1;
    }
    const int next = in.N > 1 ? 1 : 0;
    sf[(kPrevU + 0) * B] = U[next * 2 + 0];
    sf[(kPrevU + 1) * B] = U[next * 2 + 1];
    si[kPrevValid * B] = valid ? 1 : 0;
    if (in.done[b]) {                                                        // 6
        int32_t j = si[kOrdinal * B];
        if (j < a.Q) {
            const size_t r = (size_t)b * a.Q + j, BQ = B * a.Q;
            const int32_t rn = si[kReplanN * B];
            a.rec_i32[kRecSteps * BQ + r] = si[kSteps * B];
            a.rec_i32[kRecPlansValid * BQ + r] = si[kPlansValid * B];
            a.rec_i32[kRecConflictSteps * BQ + r] = si[kConflictSteps * B];
            a.rec_i32[kRecReplanN * BQ + r] = rn;
            a.rec_f64[kRecMinGap * BQ + r] = sf[kMinGap * B];
            for (int c = 0; c < 2; ++c) {
                a.rec_f64[(kRecReplanMean + c) * BQ + r] = rn > 0 ? sf[(kReplanSum + c) * B] / (double)rn : 0.0;
                a.rec_f64[(kRecReplanMax + c) * BQ + r] = sf[(kReplanMax + c) * B];
            }
            for (int i = 0; i < kLeads; ++i) {
                const int32_t n = si[(kLeadN + i) * B];
                a.rec_i32[(kRecLeadN + i) * BQ + r] = n;
                a.rec_f64[(kRecLeadMean + i) * BQ + r] = n > 0 ? sf[(kLeadSum + i) * B] / (double)n : 0.0;
                a.rec_f64[(kRecLeadMax + i) * BQ + r] = sf[(kLeadMax + i) * B];
            }
            j += 1;                          // j == Q: steps with the batch, writes no record
        }
        start_state(a, b, j);
    }
}

// one environment, serially: the host build, and the statement the kernel's lanes split between them
MPC_HD void update_env(const Accounts &a, const StepInputs &in, int b, bool reset) {
    episode_update(a, in, b, reset, reset ? kInf : fold_pairs(in, b, 0, 1));
}

// ---- the plan planes of the kept episodes ---------------------------------------------------------------------------------

struct TraceInputs {
    const double *plan_X, *plan_U;       // [B][N + 1][4], [B][N][2]
    const uint8_t *done;                 // [B]
    const int32_t *slot;                 // [B], mpc_episode_trace's work array of the same step
};

struct TraceStore {
    int B, N, Q, W, C;
    int32_t *state_i32;                  // [2][B]
    double *ring_X, *ring_U;             // [B][W][N + 1][4], [B][W][N][2]
    double *kept_X, *kept_U;             // [C][W][N + 1][4], [C][W][N][2]
};

// What one launch does for environment b.  `at(0)` is called between the append and the copy: the kernel passes a workgroup
// barrier (the copy reads what other lanes appended; every lane has read the running state by then, so lane 0 may write it
// afterwards), the host build nothing.
template <class Barrier>
MPC_HD void trace_env(const TraceStore &r, const TraceInputs &in, int b, bool reset, int lane, int lanes, Barrier at) {
    const size_t B = (size_t)r.B, W = (size_t)r.W, ux = ((size_t)r.N + 1) * 4, uu = (size_t)r.N * 2;
    int32_t *si = r.state_i32 + b;
    if (reset) {
        if (lane == 0) si[kTraceSteps * B] = 0, si[kTraceOrdinal * B] = 0;
        return;
    }
    const int32_t j = si[kTraceOrdinal * B];
    if (j >= r.Q) return;                                    // the quota is recorded: writes nothing
    const int32_t t = si[kTraceSteps * B], s = in.slot[b];
    const bool done = in.done[b] != 0;
    const size_t f = (size_t)b * W + trace::wrap(t, r.W);
    for (size_t e = lane; e < ux; e += lanes) r.ring_X[f * ux + e] = in.plan_X[(size_t)b * ux + e];
    for (size_t e = lane; e < uu; e += lanes) r.ring_U[f * uu + e] = in.plan_U[(size_t)b * uu + e];
    at(0);
    if (done && s >= 0 && s < r.C) {
        const int32_t T = t + 1, L = T < r.W ? T : r.W;
        const unsigned f0 = trace::wrap(T - L, r.W);
        trace::copy_ring(r.kept_X + (size_t)s * W * ux, r.ring_X + (size_t)b * W * ux, ux, f0, (unsigned)L, (unsigned)r.W, lane,
                         lanes);
        trace::copy_ring(r.kept_U + (size_t)s * W * uu, r.ring_U + (size_t)b * W * uu, uu, f0, (unsigned)L, (unsigned)r.W, lane,
                         lanes);
    }
    if (lane == 0) {
        si[kTraceSteps * B] = done ? 0 : t + 1;
        if (done) si[kTraceOrdinal * B] = j + 1;
    }
}

}  // namespace plan
}  // namespace mpc
