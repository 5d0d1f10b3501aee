// mpc_order.hpp - the launch-order tiers of a batch (mpc_engine.hip: mpc_order_kernel), as host-and-device functions so the
// CPU suite can call them (tests/cpu_order_harness.cpp); tools/seat_model.py restates them in numpy.
//
// tier_of() returns 0 = the seat tier (only where `seats` is set), 1..4 = the four tiers every ordered launch has had since
// round 6.  Every comparison is written so that a NaN / inf input compares false and the instance falls through to a later
// tier.
#pragma once

#include "mpc_core.hpp"

namespace mpc {
namespace order {

constexpr double kStanding = 0.1, kNear = 15.0, kTurn = 0.05;
constexpr int kBehind = 5;
// the seat tier: chosen with tools/seat_model.py on the seeds 8 - 23 (profiles/seat_tier_model.txt)
constexpr double kSeatSpeed = 4.0, kSeatClose = 5.0;
constexpr double kSeatStill = 1e-300;   // squared relative speed below which the two do not move against each other

// Squared distance at the time-aligned closest approach within [0, T] between the ego going straight on at its heading and
// speed (unit heading ce, se) and a vehicle o = (x, y, speed, heading) at its observed constant velocity.  The relative
// motion is linear, the squared distance a quadratic in time: its minimum clipped to the horizon, one reciprocal, no loop
// over the nodes.  (NaN anywhere ends as NaN: the clip passes it on.)
MPC_HD double closest_approach2(const double *x, double ce, double se, const double *o, double T) {
    const double px = o[0] - x[0], py = o[1] - x[1];
    const double wx = o[2] * cos(o[3]) - x[3] * ce, wy = o[2] * sin(o[3]) - x[3] * se;
    const double ww = wx * wx + wy * wy, pw = px * wx + py * wy;
    double t = ww > kSeatStill ? -pw * (1.0 / ww) : 0.0;      // (no relative motion: the distance now; the reciprocal stays finite)
    t = t < 0.0 ? 0.0 : (t > T ? T : t);
    const double qx = px + wx * t, qy = py + wy * t;
    return qx * qx + qy * qy;
}

// The seat tier.  The latency build holds two waves per SIMD, launch positions p and p + (number of SIMDs) share one, and
// the one that started first runs at nearly the lone-wave rate while its mate gets the rest: the first tier should hold the
// likely cap-runners AND fit the first 1024 positions, which tier 1 (about 1600 of 4096) does not.  Standing ego as in tier
// 1; otherwise no predicted collision, an ego that moves (speed >= kSeatSpeed) and a vehicle whose closest approach is below
// kSeatClose.  `others_i` = this instance's [nv][4].
MPC_HD bool first_seat(bool collide, const double *x, const double *others_i, int nv, double T) {
    if (x[3] < kStanding) return true;
    if (collide || !(x[3] >= kSeatSpeed)) return false;
    const double ce = cos(x[2]), se = sin(x[2]);
    bool hit = false;
    for (int j = 0; j < nv; ++j) hit = hit || closest_approach2(x, ce, se, others_i + (size_t)j * 4, T) < kSeatClose * kSeatClose;
    return hit;
}

// Tiers 1..4 are those of every ordered launch (see mpc_order_kernel): 1 = standing ego, or no predicted collision and
// (collision cost off or a vehicle within kNear); 2 = the other instances without a predicted collision; 3 = a predicted
// collision while the route turns; 4 = the rest.  With `seats` (one batch of the latency build with the collision cost on)
// the members of first_seat() leave them for tier 0.  T = horizon x dt.
MPC_HD int tier_of(const uint8_t *is_collide, const double *state, const double *others, int V, const int32_t *nveh,
                   const int32_t *ego, const double *ref5, int M, int N, int i, bool seats, double T) {
    const double *x = state + (size_t)i * 4;
    const bool collide = is_collide[i] != 0;
    const bool have = others && V > 0;
    const int nv = have ? (nveh ? (nveh[i] < 0 ? 0 : (nveh[i] > V ? V : nveh[i])) : V) : 0;
    if (seats && have && first_seat(collide, x, others + (size_t)i * V * 4, nv, T)) return 0;
    if (x[3] < kStanding) return 1;
    if (collide) {
        const int e0 = ego_row0(ego[i], M);
        const int a = e0 - kBehind < 0 ? 0 : (e0 - kBehind > M - 1 ? M - 1 : e0 - kBehind);
        const int b = e0 + N < 0 ? 0 : (e0 + N > M - 1 ? M - 1 : e0 + N);
        const double d = ref5[(size_t)b * REF_COLS + R_H] - ref5[(size_t)a * REF_COLS + R_H];
        return fabs(remainder(d, 6.283185307179586)) > kTurn ? 3 : 4;      // (NaN compares false: tier 4)
    }
    if (!have) return 1;
    bool near = false;
    for (int j = 0; j < nv; ++j) {
        const double *o = others + ((size_t)i * V + j) * 4;
        const double dx = o[0] - x[0], dy = o[1] - x[1];
        near = near || dx * dx + dy * dy < kNear * kNear;
    }
    return near ? 1 : 2;
}

}  // namespace order
}  // namespace mpc
