// mpc_synth_traffic.hpp - reactive traffic for the synthetic intersection environment (traffic = "idm"): every other vehicle
// follows one of twelve routes through the junction (four entries x straight / left / right), keeps its distance with the
// Intelligent Driver Model and brakes for whatever stands in the corridor in front of it, the ego included.  Written once for
// device and host (MPC_HD) like mpc_synth_env.hpp, whose constant-velocity step, draw slots and observation stay as they
// are: this header only adds.  The kernel in mpc_engine.hip (mpc_synth_env_idm_kernel) runs lane j of a 16-lane group as
// vehicle j with the functions below; step_env_idm at the end is the same step for ONE environment as a serial statement,
// the host-side reference of the tests (tests/cpu_traffic_env_harness.cpp).
//
// State per vehicle next to opos / ospeed / ohead / oactive (which stay what the observation is built from):
//   oroute  int32  3 * entry + turn; entry = approach lane 0..3 of env::spawn_other, turn 0 straight, 1 left, 2 right
//   oprog   f64    arc length s along the route
//   otarget f64    desired speed v0
// A vehicle integrates s and its speed only; position and heading are pose(route, s), so it cannot drift off its lane.
//
// A step is synchronous: every vehicle chooses its acceleration from the state BEFORE the step (the ego's and the other
// vehicles'), so the result does not depend on the order the vehicles are visited in - lane j of the kernel decides alone.
//
// The IDM constants below are this project's; highway-env is not available to compare with, so they are NOT checked
// against its IDMVehicle.
//
// contract(off): the host build is compiled with -ffp-contract=off, the device compiler contracts a * b + c by default.
// The corridor test and the spawn rule compare such expressions with thresholds, so both builds round them alike.
#pragma once

#include "mpc_synth_env.hpp"

namespace mpc {
namespace env {

constexpr double kIdmAccel = 3.0;          // a_max
constexpr double kIdmDecel = 5.0;          // b, comfortable deceleration
constexpr double kIdmMinGap = 5.0;         // s0
constexpr double kIdmHeadway = 1.5;        // T
constexpr double kVehicleLength = 5.0;
constexpr double kIdmTwoSqrtAB = 7.745966692414834;   // 2 sqrt(a_max b)
constexpr double kIdmAccelLo = -6.0, kIdmAccelHi = 3.0;
constexpr double kCorridorLength = 40.0, kCorridorHalfWidth = 2.0;
constexpr double kSpawnClearance = 10.0;
constexpr double kApproachLength = 50.0;   // the junction is entered 10 m from the centre
constexpr double kRadiusRight = 8.0, kRadiusLeft = 12.0;
constexpr double kTargetSpeedFloor = 1.0;
// one more uniform draw per vehicle (the turn), from slots the constant-velocity step never reads
constexpr int kSlotTurnRespawn = 128, kSlotTurnReset = 144;

// an angle in (-3 pi, 3 pi] to (-pi, pi]
MPC_HD double wrap_pi(double a) {
    a = a > kPiE ? a - 2.0 * kPiE : a;
    a = a <= -kPiE ? a + 2.0 * kPiE : a;
    return a;
}

MPC_HD double lane_heading(int entry) { return entry == 0 ? 0.0 : (entry == 1 ? kPiE / 2 : (entry == 2 ? kPiE : -kPiE / 2)); }

// position and heading at arc length s of a route.  d = direction of the entry heading h, n = its left-hand normal in these
// coordinates (y down): d = (cos h, sin h), n = (-sin h, cos h), exact for the four entries.
MPC_HD void pose(int route, double s, double &x, double &y, double &h) {
#pragma clang fp contract(off)
    const int entry = route / 3, turn = route - 3 * entry;
    const double dx = entry == 0 ? 1.0 : (entry == 2 ? -1.0 : 0.0), dy = entry == 1 ? 1.0 : (entry == 3 ? -1.0 : 0.0);
    const double nx = -dy, ny = dx;
    const double h0 = lane_heading(entry);
    const double u = s - kApproachLength;
    if (turn == 0 || u <= 0.0) {               // approach, and the straight route all the way
        const double a = s - 60.0;
        x = a * dx + 2.0 * nx;
        y = a * dy + 2.0 * ny;
        h = h0;
        return;
    }
    if (turn == 2) {                           // right: radius 8 about -10 d + 10 n, ends at -2 d + 10 n heading h + pi/2
        const double len = kRadiusRight * (kPiE / 2);
        if (u <= len) {
            const double phi = u / kRadiusRight, c = cos(phi), sn = sin(phi);
            x = (-10.0 * dx + 10.0 * nx) + kRadiusRight * (-nx * c + dx * sn);
            y = (-10.0 * dy + 10.0 * ny) + kRadiusRight * (-ny * c + dy * sn);
            h = wrap_pi(h0 + phi);
        } else {
            const double r = u - len;
            x = (-2.0 * dx + 10.0 * nx) + r * nx;
            y = (-2.0 * dy + 10.0 * ny) + r * ny;
            h = wrap_pi(h0 + kPiE / 2);
        }
        return;
    }
    const double len = kRadiusLeft * (kPiE / 2);   // left: radius 12 about -10 d - 10 n, ends at 2 d - 10 n heading h - pi/2
    if (u <= len) {
        const double phi = u / kRadiusLeft, c = cos(phi), sn = sin(phi);
        x = (-10.0 * dx - 10.0 * nx) + kRadiusLeft * (nx * c + dx * sn);
        y = (-10.0 * dy - 10.0 * ny) + kRadiusLeft * (ny * c + dy * sn);
        h = wrap_pi(h0 - phi);
    } else {
        const double r = u - len;
        x = (2.0 * dx - 10.0 * nx) - r * nx;
        y = (2.0 * dy - 10.0 * ny) - r * ny;
        h = wrap_pi(h0 - kPiE / 2);
    }
}

// the nearest counted candidate in vehicle j's corridor so far: who = -2 nobody, -1 the ego, k another vehicle
struct Leader {
    double ell, head, speed;
    int who;
};
MPC_HD Leader no_leader() {
    Leader l;
    l.ell = INFINITY;
    l.head = 0.0;
    l.speed = 0.0;
    l.who = -2;
    return l;
}

// Offer candidate c (centre cx, cy, heading ch, speed cv) to vehicle j at (xj, yj) with heading hj = atan2(sj, cj).  In the
// corridor: 0 < longitudinal offset <= 40 and |lateral offset| <= 2 in j's body frame.  The ego (c = -1) counts whenever it
// is there; another vehicle counts if it drives roughly j's way (car-following) or has the lower slot index (crossing
// traffic yields by index), and only from one vehicle length ahead: the other vehicles do not collide with each other, and
// one whose centre is nearer than that overlaps j (routes merge) rather than leads it - counted, its gap of zero froze
// whole queues at the merges, each vehicle waiting until the one it overlapped was 10 m away.
MPC_HD void offer_leader(Leader &best, int j, double xj, double yj, double hj, double cj, double sj, int c, double cx, double cy,
                         double ch, double cv) {
#pragma clang fp contract(off)
    const double ex = cx - xj, ey = cy - yj;
    const double ell = ex * cj + ey * sj;
    const double w = ey * cj - ex * sj;
    const bool inside = ell > 0.0 && ell <= kCorridorLength && fabs(w) <= kCorridorHalfWidth;
    const bool counts = c < 0 || (ell > kVehicleLength && (c < j || fabs(wrap_pi(ch - hj)) < kPiE / 4));
    if (inside && counts && ell < best.ell) {
        best.ell = ell;
        best.head = ch;
        best.speed = cv;
        best.who = c;
    }
}

// Who waits for whom is a map j -> leader(j), and it can close into a circle of standing vehicles in two ways the corridor
// rule allows: two vehicles merging onto one exit lane at a small angle are each just ahead of the other, and a chain can mix
// following with yielding (a turning vehicle's straight corridor sweeps over a lane it never enters).  One step of the walk
// along that map from vehicle j: `p` is where the walk stands, `lowest` the lowest index met, `closed` whether it came back
// to j.  After K steps (a circle has at most K members) the vehicle with closed && lowest == j - the lowest index of its
// circle - drives as on a free road for this step, so every circle has one member that moves: the relation that remains is
// acyclic, decided by index.  leader_of_p is leader(p), < 0 where p follows the ego or nobody.
MPC_HD void walk_leaders(int j, int leader_of_p, int &p, int &lowest, bool &closed) {
    if (p < 0 || closed) return;
    if (p == j) {
        closed = true;
        return;
    }
    lowest = p < lowest ? p : lowest;
    p = leader_of_p;
}

// IDM acceleration of a vehicle with speed v, desired speed v0 and heading hj behind `lead`, clamped to [-6, 3]
MPC_HD double idm_acceleration(double v, double v0, double hj, const Leader &lead) {
#pragma clang fp contract(off)
    const double r = v / v0, r2 = r * r;
    double interaction = 0.0;
    if (lead.who != -2) {
        double gap = lead.ell - kVehicleLength;
        gap = gap < 0.1 ? 0.1 : gap;
        const double dv = v - lead.speed * cos(lead.head - hj);
        double dyn = v * kIdmHeadway + v * dv / kIdmTwoSqrtAB;
        dyn = dyn < 0.0 ? 0.0 : dyn;
        const double q = (kIdmMinGap + dyn) / gap;
        interaction = q * q;
    }
    const double a = kIdmAccel * (1.0 - r2 * r2 - interaction);
    return a < kIdmAccelLo ? kIdmAccelLo : (a > kIdmAccelHi ? kIdmAccelHi : a);
}

// explicit Euler in the ego's order: the arc length advances with the speed before the step
MPC_HD void advance(double a, double dt, double &s, double &v) {
#pragma clang fp contract(off)
    s = s + v * dt;
    const double nv = v + a * dt;
    v = nv < 0.0 ? 0.0 : (nv > 30.0 ? 30.0 : nv);
}

// a vehicle drawn with env::spawn_other's slots s .. s + 3 plus the turn from `turn_slot`: the entry lane is recovered from
// the same draw spawn_other makes, the distance d from the centre gives s = 60 - d
struct Drawn {
    int route;
    double s, speed, target, x, y, h;
};
MPC_HD Drawn draw_vehicle(const Rng &r, int slot, int turn_slot, double dlo, double dhi) {
#pragma clang fp contract(off)
    Drawn o;
    int lane = (int)(r.u01(slot) * 4.0);
    lane = lane > 3 ? 3 : lane;
    int turn = (int)(r.u01(turn_slot) * 3.0);
    turn = turn > 2 ? 2 : turn;
    o.route = 3 * lane + turn;
    const double d = dlo + (dhi - dlo) * r.u01(slot + 1);
    o.s = 60.0 - d;
    double sp = 8.0 + r.normal(slot + 2);
    sp = sp < 0.0 ? 0.0 : sp;
    o.speed = sp;
    o.target = sp < kTargetSpeedFloor ? kTargetSpeedFloor : sp;
    pose(o.route, o.s, o.x, o.y, o.h);
    return o;
}

// spawn rule: a drawn vehicle is not placed when its centre is within 10 m of the given one
MPC_HD bool too_close(double ax, double ay, double bx, double by) {
#pragma clang fp contract(off)
    const double ex = ax - bx, ey = ay - by;
    return ex * ex + ey * ey < kSpawnClearance * kSpawnClearance;
}

struct TrafficView {
    int32_t *oroute;   // [K]
    double *oprog;     // [K]
    double *otarget;   // [K]
};

// fresh episode: the ego as env::reset_env draws it; vehicle j is placed unless a lower-index vehicle was drawn within 10 m
// (whether that one was placed or not, so j decides from the draws alone)
MPC_HD void reset_env_idm(const View &v, const TrafficView &tv, int K, const Rng &r) {
    store_ego(v.ego, fresh_ego(r));
    double qx[kMaxOthers], qy[kMaxOthers];
    for (int j = 0; j < K; ++j) {
        const Drawn o = draw_vehicle(r, kSlotReset + 4 * j, kSlotTurnReset + j, 5.0, 60.0);
        qx[j] = o.x;
        qy[j] = o.y;
        bool placed = true;
        for (int k = 0; k < j; ++k) placed = placed && !too_close(o.x, o.y, qx[k], qy[k]);
        v.opos[2 * j] = o.x;
        v.opos[2 * j + 1] = o.y;
        v.ospeed[j] = o.speed;
        v.ohead[j] = o.h;
        v.oactive[j] = placed ? 1 : 0;
        tv.oroute[j] = o.route;
        tv.oprog[j] = o.s;
        tv.otarget[j] = o.target;
    }
    *v.t = 0;
}

// one policy step with reactive traffic; everything that concerns the ego, the reward, the termination and the observation
// is env::step_env's, through the same functions.  leader_out / accel_out (optional, [K]): whom each vehicle that drove this
// step followed (-2 nobody, -1 the ego, k vehicle k; -3 for a vehicle that was not active) and the acceleration it chose -
// diagnostics for the tests.
MPC_HD StepOut step_env_idm(const View &v, const TrafficView &tv, int K, double dt, double spawn_probability, uint64_t seed,
                            int env_id, const double *ref_xy, int M, const double *action, float *terminal_obs, float *obs,
                            int32_t *leader_out, double *accel_out) {
    const Rng r(seed, env_id, *v.ctr);
    *v.ctr += 1;
    const Ego e0 = load_ego(v.ego), e = step_ego(e0, action, dt);
    store_ego(v.ego, e);
    // ---- accelerations from the state before the step
    double acc[kMaxOthers];
    Leader leads[kMaxOthers];
    int who[kMaxOthers];
    for (int j = 0; j < K; ++j) {
        leads[j] = no_leader();
        who[j] = -2;
        if (!v.oactive[j]) continue;
        const double xj = v.opos[2 * j], yj = v.opos[2 * j + 1], hj = v.ohead[j], cj = cos(hj), sj = sin(hj);
        Leader lead = no_leader();
        offer_leader(lead, j, xj, yj, hj, cj, sj, -1, e0.x, e0.y, e0.th, e0.sp);
        for (int k = 0; k < K; ++k)
            if (k != j && v.oactive[k])
                offer_leader(lead, j, xj, yj, hj, cj, sj, k, v.opos[2 * k], v.opos[2 * k + 1], v.ohead[k], v.ospeed[k]);
        leads[j] = lead;
        who[j] = lead.who;
    }
    for (int j = 0; j < K; ++j) {
        acc[j] = 0.0;
        if (leader_out) leader_out[j] = -3;
        if (accel_out) accel_out[j] = 0.0;
        if (!v.oactive[j]) continue;
        int p = who[j], lowest = j;
        bool closed = false;
        for (int n = 0; n < K; ++n) walk_leaders(j, p >= 0 ? who[p] : -2, p, lowest, closed);
        if (closed && lowest == j) leads[j] = no_leader();
        acc[j] = idm_acceleration(v.ospeed[j], tv.otarget[j], v.ohead[j], leads[j]);
        if (leader_out) leader_out[j] = leads[j].who;
        if (accel_out) accel_out[j] = acc[j];
    }
    // ---- move; a vehicle that left (or was away) draws its respawn
    bool stays[kMaxOthers], drew[kMaxOthers];
    Drawn cand[kMaxOthers];
    for (int j = 0; j < K; ++j) {
        bool gone = true;
        if (v.oactive[j]) {
            advance(acc[j], dt, tv.oprog[j], v.ospeed[j]);
            pose(tv.oroute[j], tv.oprog[j], v.opos[2 * j], v.opos[2 * j + 1], v.ohead[j]);
            gone = left_the_map(v.opos[2 * j], v.opos[2 * j + 1]);
        }
        stays[j] = !gone;
        drew[j] = gone && r.u01(kSlotRespawn + 5 * j) < spawn_probability;
        if (drew[j]) cand[j] = draw_vehicle(r, kSlotRespawn + 5 * j + 1, kSlotTurnRespawn + j, 40.0, 60.0);
    }
    // ---- spawn rule: clear of every lower-index vehicle that stays or was drawn, and of every higher-index one that stays
    bool crashed = false;
    for (int j = 0; j < K; ++j) {
        if (!stays[j]) {
            bool placed = drew[j];
            for (int k = 0; k < K && placed; ++k) {
                if (k == j) continue;
                if (stays[k]) placed = !too_close(cand[j].x, cand[j].y, v.opos[2 * k], v.opos[2 * k + 1]);
                else if (k < j && drew[k]) placed = !too_close(cand[j].x, cand[j].y, cand[k].x, cand[k].y);
            }
            if (placed) {
                tv.oroute[j] = cand[j].route;
                tv.oprog[j] = cand[j].s;
                tv.otarget[j] = cand[j].target;
            }
            v.oactive[j] = placed ? 1 : 0;
        }
    }
    for (int j = 0; j < K; ++j) {       // (after the rule: it reads the positions of the vehicles that stay)
        if (!stays[j] && v.oactive[j]) {
            v.opos[2 * j] = cand[j].x;
            v.opos[2 * j + 1] = cand[j].y;
            v.ospeed[j] = cand[j].speed;
            v.ohead[j] = cand[j].h;
        }
        crashed = crashed || (v.oactive[j] && hits_ego(v.opos[2 * j], v.opos[2 * j + 1], e.x, e.y));
    }
    const Nearest n = nearest_route_point(ref_xy, M, 0, 1, e.x, e.y);
    *v.t += 1;
    const StepOut o = score_step(n.d, n.idx, M, crashed, e.sp, *v.t);
    observe(v, K, terminal_obs);
    if (o.done) {
        reset_env_idm(v, tv, K, r);
        observe(v, K, obs);
    } else {
        for (int i = 0; i < kRows * kCols; ++i) obs[i] = terminal_obs[i];
    }
    return o;
}

}  // namespace env
}  // namespace mpc
