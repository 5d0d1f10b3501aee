// mpc_interaction.hpp - interaction metrics of a closed-loop evaluation, per episode, next to mpc_episode_stats.hpp and
// mpc_drive_metrics.hpp: what the ego does to the reactive traffic (traffic = "idm").  How often another vehicle yields to the
// ego, how hard the ego makes it brake, how much speed that costs the traffic, and the post-encroachment time where a traffic
// route crosses the ego's.  One launch per policy step after the environment's step; the update of one environment is
// written once for the kernel (mpc_interaction_kernel in mpc_engine.hip, sixteen lanes per environment) and its host build
// (tests/cpu_interaction_harness.cpp).  kPetCritical below is this project's threshold, kHardBrake the drive metrics'.
//
// ENVIRONMENT BOUND: the update reads the simulator's slots (ego, opos, ospeed, ohead, oactive, oroute, oprog, otarget of
// mpc_synth_env_step_idm), not the observation, whose rows are sorted by distance and so are not a vehicle from one step to
// the next.  Leader, circle rule and acceleration are mpc::env's own functions (mpc_synth_traffic.hpp); nothing is restated.
//
// WHICH STATES ARE FOLDED.  A launch comes after the environment's step and auto-reset.  Not done: the environment's current
// state is folded.  done: the record is written from the states folded so far, the running state is cleared, and the current
// (fresh) state is folded as state 0 of the next episode.  A reset launch clears and folds the fresh state.  An episode's
// account therefore covers the states s_0 .. s_{T-1} in which the agent and the traffic made their decisions - exactly the
// states step_env_idm computed accelerations from; `steps` = T.  THE TERMINAL STATE IS NOT FOLDED: nobody decides in it.
//
// ARITHMETIC: f64 without contraction (the pragma in every function).  cos and sin are the build's own, so the kernel, the
// host build and the evaluator's numpy path agree to rounding of those two, not bit for bit.  min2 / max2 are the drive
// metrics'; "nothing there" is +inf for a minimum and 0 for a maximum.
//
// THE FORMULAS, in evaluation order (sums left to right), for the state with index n within its episode (n = steps so far):
//  (a) yielding and forced braking - a pure function of the state.  For every active vehicle j:
//      lead_j   best of env::offer_leader over the ego (c = -1) and then the other active vehicles k ascending
//      alt_j    the same with the ego never offered
//      who[j]   lead_j.who (-2 for an inactive vehicle)
//      circle rule (env::walk_leaders, K steps from p = who[j] along who[]): closed && lowest == j -> lead_j = nobody
//      a_with   env::idm_acceleration(ospeed, otarget, ohead, lead_j)
//      yields   lead_j.who == -1 after the circle rule (the ego is never part of a circle, so the rule leaves it alone)
//      a_free   for a yielding vehicle: the walk from p = alt_j.who along the same who[] (only j's leader is replaced, and a
//               walk from j never reads who[j]); closed && lowest == j -> alt_j = nobody; idm_acceleration(..., alt_j)
//      imposed  a_free - a_with for a yielding vehicle, else 0;  hard: yields and a_with < -kHardBrake
//      n_yield = vehicles that yield;  forced = max(0, max over yielding j of -a_with);  hard_mask: bit j where hard
//      deficit = (sum over j = 0 .. K-1 ascending of imposed_j) * dt   [m/s]: the speed the ego took from the traffic
//  (b) post-encroachment time at crossing conflicts - uses slot identity.  conflict [12][2] = (sigma_c, s_c) per traffic
//      route: arc length along the ego's polyline and along the route where they cross; sigma_c < 0: no crossing conflict.
//      sigma    the ego's arc length: over the segments i = 0 .. max(M - 1, 1) - 1 of ref_xy (end point min(i + 1, M - 1)),
//               d2_i = drive::seg2(ego; ref[i], d_i); the first of the nearest wins;  t as in seg2 (0 if dd == 0, else
//               (s.d) / dd clamped to [0, 1]);  sigma = (sqrt(dd_0) + ... + sqrt(dd_{i-1}), left to right from 0.0) + t * sqrt(dd_i)
//      pass     a quantity going from prev (state n - 1) to cur (state n) passes c when prev < c <= cur, at
//               tau = (double)(n - 1) + (c - prev) / (cur - prev), in units of the state index; n >= 1 only
//      ego      for every route r with sigma_c >= 0 and t_e[r] not set: if sigma passes sigma_c, t_e[r] = tau (the first
//               pass of an episode is kept)
//      slot j   holds the same vehicle as in the previously folded state iff it is active, the carried oroute equals its
//               oroute (the carry is -1 for a slot that was inactive or cleared) and oprog >= the carried oprog.  Otherwise
//               t_v[j] is cleared and no pass is evaluated for it in this state.  The same vehicle with t_v[j] not set and a
//               route r with sigma_c >= 0: if oprog passes s_c, t_v[j] = tau
//      pet      for slot j ascending, r its route: when t_e[r] and t_v[j] are both set and one of them was set in this state
//               (the second of the two passes), pet = fabs(t_e[r] - t_v[j]) * dt once: conflicts += 1, pet_critical += 1 if
//               pet < kPetCritical, ego_first += 1 if t_e[r] < t_v[j], min_pet = min2(min_pet, pet).  The vehicle is the one
//               still in the slot.  "Not set" is a negative time (-1.0); a set one is > 0.
//  then: steps += 1, yield_steps += n_yield > 0, forced_brake_steps += hard_mask != 0, forced_brake_events += bits set in
//  hard_mask and not in the previous state's (0 after a clear), max_forced_decel = max2(., forced), speed_deficit += deficit,
//  and the carries: sigma, hard_mask, per slot oprog and oroute (-1 when inactive).
//
// Running state of environment b (planar [field][B], like the sister kernels):
//   state_i32 [9 + S][B]    steps, yield_steps, forced_brake_steps, forced_brake_events, conflicts, pet_critical, ego_first,
//                           episode ordinal j (saturates at the quota Q), previous hard_mask;  then S = kSlots (9) carried oroute
//   state_f64 [16 + 2 S][B] max_forced_decel, speed_deficit, min_pet, carried sigma;  t_e[12];  t_v[S];  carried oprog[S]
// Records, slot [b][j] for j < Q with the quota and ordinal rule of mpc_episode_stats (all three accounts see the same `done`,
// so slot [b][j] of all three describes the same episode):
//   rec_i32 [7][B][Q]  steps, yield_steps, forced_brake_steps, forced_brake_events, conflicts, pet_critical, ego_first
//   rec_f64 [3][B][Q]  max_forced_decel, speed_deficit, min_pet (+inf when no conflict was evaluated)
// A new episode clears every counter, the previous mask and all pass times and carries.
#pragma once

#include <stdint.h>

#include "mpc_drive_metrics.hpp"
#include "mpc_synth_traffic.hpp"

namespace mpc {
namespace interact {

constexpr double kPetCritical = 1.5;                      // s: this project's threshold for a critical post-encroachment time
constexpr double kHardBrake = drive::kHardBrake;          // m/s^2: a yielding vehicle braking harder than this is forced
constexpr double kInf = drive::kInf;
constexpr double kUnset = -1.0;                           // a pass time that is not set
constexpr int kRoutes = 12, kSlots = env::kMaxOthers, kMaxRoute = drive::kMaxRoute;

enum { kSteps = 0, kYieldSteps = 1, kForcedSteps = 2, kForcedEvents = 3, kConflicts = 4, kPetCriticalN = 5, kEgoFirst = 6,
       kOrdinal = 7, kPrevMask = 8, kCarryRoute = 9, kStateI32 = 9 + kSlots };
enum { kMaxForced = 0, kDeficit = 1, kMinPet = 2, kCarrySigma = 3, kTe = 4, kTv = 4 + kRoutes, kCarryProg = 4 + kRoutes + kSlots,
       kStateF64 = 4 + kRoutes + 2 * kSlots };
enum { kRecI32 = 7, kRecF64 = 3 };

struct StepInputs {              // the environment after a step: the state arrays of mpc_synth_env_step_idm
    int K, M;
    double dt;
    const double *ego;           // [B][4]
    const double *opos;          // [B][max(K, 1)][2]
    const double *ospeed, *ohead;        // [B][max(K, 1)]
    const uint8_t *oactive;
    const int32_t *oroute;
    const double *oprog, *otarget;
    const uint8_t *done;         // [B]
    const double *ref_xy;        // [M][2]
    const double *conflict;      // [12][2]
};

struct Accounts {
    int B, Q;
    int32_t *state_i32;          // [9 + kSlots][B]
    double *state_f64;           // [16 + 2 kSlots][B]
    int32_t *rec_i32;            // [7][B][Q]
    double *rec_f64;             // [3][B][Q]
};

struct Decision {                // part (a) for one vehicle
    int who;                     // whom it follows after the circle rule (-3 inactive)
    double a_with, imposed;
    bool yields, hard;
};

struct Proj {                    // the nearest segment so far
    double d2;
    int idx;
};

struct Pets {                    // what the slots contribute to one state
    int conflicts, critical, ego_first;
    double min_pet;
};

// one walk of the circle rule from vehicle j whose leader is `first`; who_of(p) is read through `who` [K]
MPC_HD bool drives_free(int j, int K, int first, const int *who) {
    int p = first, lowest = j;
    bool closed = false;
    for (int n = 0; n < K; ++n) env::walk_leaders(j, p >= 0 ? who[p] : -2, p, lowest, closed);
    return closed && lowest == j;
}

// the decision of an active vehicle from its two leaders after the circle rule (alt only matters when it yields)
MPC_HD Decision decide(double v, double v0, double h, const env::Leader &lead, const env::Leader &alt) {
#pragma clang fp contract(off)
    Decision d;
    d.who = lead.who;
    d.a_with = env::idm_acceleration(v, v0, h, lead);
    d.yields = lead.who == -1;
    d.imposed = 0.0;
    if (d.yields) d.imposed = env::idm_acceleration(v, v0, h, alt) - d.a_with;
    d.hard = d.yields && d.a_with < -kHardBrake;
    return d;
}

MPC_HD Decision inactive_decision() {
    Decision d;
    d.who = -3;
    d.a_with = 0.0;
    d.imposed = 0.0;
    d.yields = false;
    d.hard = false;
    return d;
}

// segment i of the route against the point: keeps the first of the nearest when i ascends
MPC_HD void fold_proj(const double *ref_xy, int M, int i, double x, double y, Proj &p) {
#pragma clang fp contract(off)
    const int i1 = i + 1 < M ? i + 1 : M - 1;
    const double e0x = ref_xy[2 * i], e0y = ref_xy[2 * i + 1];
    const double d2 = drive::seg2(x, y, e0x, e0y, ref_xy[2 * i1] - e0x, ref_xy[2 * i1 + 1] - e0y);
    if (d2 < p.d2) {
        p.d2 = d2;
        p.idx = i;
    }
}

// arc length of the projection onto segment idx
MPC_HD double sigma_at(const double *ref_xy, int M, int idx, double x, double y) {
#pragma clang fp contract(off)
    double before = 0.0;
    for (int i = 0; i < idx; ++i) {
        const int i1 = i + 1 < M ? i + 1 : M - 1;
        const double dx = ref_xy[2 * i1] - ref_xy[2 * i], dy = ref_xy[2 * i1 + 1] - ref_xy[2 * i + 1];
        before = before + sqrt(dx * dx + dy * dy);
    }
    const int i1 = idx + 1 < M ? idx + 1 : M - 1;
    const double e0x = ref_xy[2 * idx], e0y = ref_xy[2 * idx + 1];
    const double dx = ref_xy[2 * i1] - e0x, dy = ref_xy[2 * i1 + 1] - e0y;
    const double sx = x - e0x, sy = y - e0y;
    const double dd = dx * dx + dy * dy;
    double t = 0.0;
    if (dd > 0.0) {
        t = (sx * dx + sy * dy) / dd;
        t = t < 0.0 ? 0.0 : t;
        t = t > 1.0 ? 1.0 : t;
    }
    return before + t * sqrt(dd);
}

// (b) indexes the conflict table by the route: a slot whose route is not one of the twelve counts as empty there
MPC_HD bool valid_route(int route) { return route >= 0 && route < kRoutes; }

MPC_HD bool passes(double prev, double c, double cur) { return prev < c && c <= cur; }

MPC_HD double pass_time(int n, double prev, double c, double cur) {
#pragma clang fp contract(off)
    return (double)(n - 1) + (c - prev) / (cur - prev);
}

// the ego's pass time of route r after state n: te as carried (kUnset after a clear); `fresh` whether it was set here
MPC_HD double ego_pass(int n, double sigma_c, double te, double sigma_prev, double sigma, bool &fresh) {
    fresh = n >= 1 && sigma_c >= 0.0 && te < 0.0 && passes(sigma_prev, sigma_c, sigma);
    return fresh ? pass_time(n, sigma_prev, sigma_c, sigma) : te;
}

// slot j's pass time after state n: tv, croute, cprog as carried; `fresh` whether it was set here
MPC_HD double slot_pass(int n, bool active, int route, double prog, int croute, double cprog, double tv,
                        const double *conflict, bool &fresh) {
    fresh = false;
    const bool same = n >= 1 && active && croute == route && prog >= cprog;
    if (!same) return kUnset;
    const double sigma_c = conflict[2 * route], s_c = conflict[2 * route + 1];
    fresh = sigma_c >= 0.0 && tv < 0.0 && passes(cprog, s_c, prog);
    return fresh ? pass_time(n, cprog, s_c, prog) : tv;
}

// the post-encroachment time of a slot whose pair completed in this state, folded into p
MPC_HD void fold_pet(double te, double tv, bool te_fresh, bool tv_fresh, double dt, Pets &p) {
#pragma clang fp contract(off)
    if (!(te >= 0.0 && tv >= 0.0 && (te_fresh || tv_fresh))) return;
    const double pet = fabs(te - tv) * dt;
    p.conflicts += 1;
    p.critical += pet < kPetCritical ? 1 : 0;
    p.ego_first += te < tv ? 1 : 0;
    p.min_pet = drive::min2(p.min_pet, pet);
}

struct Running {                 // the counters of an episode
    int32_t steps, yield_steps, forced_steps, forced_events, conflicts, critical, ego_first, prev_mask;
    double max_forced, deficit, min_pet;
};

MPC_HD Running cleared() {
    Running r;
    r.steps = r.yield_steps = r.forced_steps = r.forced_events = r.conflicts = r.critical = r.ego_first = r.prev_mask = 0;
    r.max_forced = 0.0;
    r.deficit = 0.0;
    r.min_pet = kInf;
    return r;
}

// The head of the sequential part, environment b: whether this launch starts an episode; when the last one ended, its record
// is written first.  Returns the counters the fold continues from; `ordinal` is the one to store.
MPC_HD Running open_episode(const Accounts &a, const StepInputs &in, int b, bool reset, bool &fresh, int32_t &ordinal) {
    const size_t B = (size_t)a.B;
    const int32_t *si = a.state_i32 + b;
    const double *sf = a.state_f64 + b;
    fresh = reset || in.done[b] != 0;
    ordinal = reset ? 0 : si[kOrdinal * B];
    if (!fresh) {
        Running r;
        r.steps = si[kSteps * B];
        r.yield_steps = si[kYieldSteps * B];
        r.forced_steps = si[kForcedSteps * B];
        r.forced_events = si[kForcedEvents * B];
        r.conflicts = si[kConflicts * B];
        r.critical = si[kPetCriticalN * B];
        r.ego_first = si[kEgoFirst * B];
        r.prev_mask = si[kPrevMask * B];
        r.max_forced = sf[kMaxForced * B];
        r.deficit = sf[kDeficit * B];
        r.min_pet = sf[kMinPet * B];
        return r;
    }
    if (!reset && ordinal < a.Q) {
        const size_t r = (size_t)b * a.Q + ordinal, BQ = B * a.Q;
        for (int f = 0; f < kRecI32; ++f) a.rec_i32[f * BQ + r] = si[f * B];     // the first seven fields, in record order
        for (int f = 0; f < kRecF64; ++f) a.rec_f64[f * BQ + r] = sf[f * B];
        ordinal += 1;                    // ordinal == Q: idle, steps with the batch, writes nothing
    }
    return cleared();
}

// The tail of the sequential part: the state's contributions folded into r and stored.  n_yield, forced, hard_mask and
// imposed_sum are part (a) of this state, p part (b), sigma the ego's arc length.
MPC_HD void close_state(const Accounts &a, int b, double dt, Running r, int32_t ordinal, int n_yield, double forced,
                        int32_t hard_mask, double imposed_sum, const Pets &p, double sigma) {
#pragma clang fp contract(off)
    const size_t B = (size_t)a.B;
    int32_t *si = a.state_i32 + b;
    double *sf = a.state_f64 + b;
    si[kSteps * B] = r.steps + 1;
    si[kYieldSteps * B] = r.yield_steps + (n_yield > 0 ? 1 : 0);
    si[kForcedSteps * B] = r.forced_steps + (hard_mask != 0 ? 1 : 0);
    si[kForcedEvents * B] = r.forced_events + __builtin_popcount((unsigned)(hard_mask & ~r.prev_mask));
    si[kConflicts * B] = r.conflicts + p.conflicts;
    si[kPetCriticalN * B] = r.critical + p.critical;
    si[kEgoFirst * B] = r.ego_first + p.ego_first;
    si[kOrdinal * B] = ordinal;
    si[kPrevMask * B] = hard_mask;
    sf[kMaxForced * B] = drive::max2(r.max_forced, forced);
    sf[kDeficit * B] = r.deficit + imposed_sum * dt;
    sf[kMinPet * B] = drive::min2(r.min_pet, p.min_pet);
    sf[kCarrySigma * B] = sigma;
}

// one environment, serially: the host build, and the statement the kernel's lanes split between them.  decisions (optional,
// [K]): part (a) per vehicle, a diagnostic for the tests.
MPC_HD void update_env(const Accounts &a, const StepInputs &in, int b, bool reset, Decision *decisions = nullptr) {
#pragma clang fp contract(off)
    const size_t B = (size_t)a.B;
    const int K = in.K, Ks = K > 0 ? K : 1;
    const size_t vo = (size_t)b * Ks;
    int32_t *si = a.state_i32 + b;
    double *sf = a.state_f64 + b;
    bool fresh;
    int32_t ordinal;
    const Running run = open_episode(a, in, b, reset, fresh, ordinal);
    const int n = run.steps;
    const env::Ego e = env::load_ego(in.ego + (size_t)b * 4);
    // ---- (a)
    env::Leader lead[kSlots], alt[kSlots];
    int who[kSlots];
    for (int j = 0; j < K; ++j) {
        lead[j] = alt[j] = env::no_leader();
        who[j] = -2;
        if (!in.oactive[vo + j]) continue;
        const double xj = in.opos[2 * (vo + j)], yj = in.opos[2 * (vo + j) + 1], hj = in.ohead[vo + j];
        const double cj = cos(hj), sj = sin(hj);
        env::offer_leader(lead[j], j, xj, yj, hj, cj, sj, -1, e.x, e.y, e.th, e.sp);
        for (int k = 0; k < K; ++k)
            if (k != j && in.oactive[vo + k]) {
                const double kx = in.opos[2 * (vo + k)], ky = in.opos[2 * (vo + k) + 1];
                env::offer_leader(lead[j], j, xj, yj, hj, cj, sj, k, kx, ky, in.ohead[vo + k], in.ospeed[vo + k]);
                env::offer_leader(alt[j], j, xj, yj, hj, cj, sj, k, kx, ky, in.ohead[vo + k], in.ospeed[vo + k]);
            }
        who[j] = lead[j].who;
    }
    int n_yield = 0;
    int32_t hard_mask = 0;
    double forced = 0.0, imposed_sum = 0.0;
    for (int j = 0; j < K; ++j) {
        Decision d = inactive_decision();
        if (in.oactive[vo + j]) {
            if (drives_free(j, K, who[j], who)) lead[j] = env::no_leader();
            if (lead[j].who == -1 && drives_free(j, K, alt[j].who, who)) alt[j] = env::no_leader();
            d = decide(in.ospeed[vo + j], in.otarget[vo + j], in.ohead[vo + j], lead[j], alt[j]);
        }
        n_yield += d.yields ? 1 : 0;
        if (d.yields) forced = drive::max2(forced, -d.a_with);
        hard_mask |= d.hard ? (1 << j) : 0;
        imposed_sum = imposed_sum + d.imposed;
        if (decisions) decisions[j] = d;
    }
    // ---- (b)
    Proj pr{kInf, 0};
    const int nseg = in.M > 1 ? in.M - 1 : 1;
    for (int i = 0; i < nseg; ++i) fold_proj(in.ref_xy, in.M, i, e.x, e.y, pr);
    const double sigma = sigma_at(in.ref_xy, in.M, pr.idx, e.x, e.y);
    const double sigma_prev = sf[kCarrySigma * B];
    double te[kRoutes];
    bool te_fresh[kRoutes];
    for (int r = 0; r < kRoutes; ++r) {
        te[r] = ego_pass(n, in.conflict[2 * r], fresh ? kUnset : sf[(kTe + r) * B], sigma_prev, sigma, te_fresh[r]);
        sf[(kTe + r) * B] = te[r];
    }
    Pets p{0, 0, 0, kInf};
    for (int j = 0; j < kSlots; ++j) {
        const bool active = j < K && in.oactive[vo + j] != 0 && valid_route(in.oroute[vo + j]);
        const int route = active ? in.oroute[vo + j] : -1;
        const double prog = active ? in.oprog[vo + j] : 0.0;
        bool tv_fresh = false;
        double tv = kUnset;
        if (!fresh) tv = slot_pass(n, active, route, prog, si[(kCarryRoute + j) * B], sf[(kCarryProg + j) * B], sf[(kTv + j) * B],
                                   in.conflict, tv_fresh);
        if (active) fold_pet(te[route], tv, te_fresh[route], tv_fresh, in.dt, p);
        sf[(kTv + j) * B] = tv;
        sf[(kCarryProg + j) * B] = prog;
        si[(kCarryRoute + j) * B] = route;
    }
    close_state(a, b, in.dt, run, ordinal, n_yield, forced, hard_mask, imposed_sum, p, sigma);
}

}  // namespace interact
}  // namespace mpc
