// mpc_perception.hpp - a perception model between the environment and the agent of a closed-loop evaluation: what the ego
// sees of the true scene.  Limited range, occlusion by other vehicles and by static buildings, random dropout and bounded
// measurement noise.  One launch per policy step after the environment's step; the update of one environment is written once
// for the kernel (mpc_perceive_kernel in mpc_engine.hip, sixteen lanes per environment, a lane per row) and its host build
// (tests/cpu_perception_harness.cpp, perceive_env below, serially).
//
// OBSERVATION ONLY: reads the true observation, never the simulator's state.
//   obs_true [B][R][8] f32  presence, x, y, vx, vy, heading, sin_h, cos_h (mpc_synth_env.hpp); row 0 the ego; a row i >= 1 is
//                           PRESENT when its presence != 0
//   obs_seen [B][R][8] f32  the observation the agent acts on (must not alias obs_true)
//   occluders [S][4][2] f64 S <= 8 convex quadrilaterals by their corners in order (static: buildings); NULL when S == 0
//
// ARITHMETIC: f64 on the f32 inputs widened exactly; only + - * / sqrt, comparisons and integer operations, no contraction
// (the pragma in every function).  So the kernel, the host build, the evaluator's CPU path and a plain-Python restatement
// agree bit for bit.  The rectangle of a vehicle is mpc::drive::corners (5.0 m x 2.0 m), the generator is mpc::env::Rng.
//
// PARAMETERS (Params; the value that switches each off):  range [m] (+inf), occlusion 0 / 1 (0), min_points 1..5 (1),
// p_drop in [0, 1] (0), sigma_pos [m], sigma_vel [m/s], sigma_head [rad] (0), seed, env_offset.
//
// THE UPDATE of environment b, in evaluation order.  p = (x, y) of row 0; q, (cos_h, sin_h) of a row i >= 1.
//   range      r = q - p;  dd = r.x r.x + r.y r.y;  out of range when dd > range * range
//   occlusion  (only when occlusion != 0)  the five sample points of row i: s0 = q, s1..s4 = corners(q, (cos_h, sin_h)).
//              Occluding edges: the four edges (corner k to corner (k + 1) % 4) of the rectangle of every PRESENT row j >= 1,
//              j != i - a vehicle that is itself out of range or dropped still blocks the view - and of every static
//              occluder.  The ego's rectangle occludes nothing.  With cross(a, b) = a.x b.y - a.y b.x and, for the edge
//              e0 -> e1 and the sample point s,
//                d1 = cross(e1 - e0, p - e0)   d2 = cross(e1 - e0, s - e0)   d3 = cross(s - p, e0 - p)   d4 = cross(s - p, e1 - p)
//              the sight line p -> s STRICTLY crosses the edge when
//                ((d1 > 0 && d2 < 0) || (d1 < 0 && d2 > 0)) && ((d3 > 0 && d4 < 0) || (d3 < 0 && d4 > 0));
//              touching, grazing a corner and collinear overlap do not hide.  A point is hidden when its sight line crosses
//              any edge; the row is occluded when fewer than min_points of its five points are not hidden.
//   draws      Rng r(seed ^ kSalt, env_offset + b, ctr[b]); kSalt keeps them apart from the environment's own draws, which
//              use the same seed and counter values.  u(k) = r.u01(k).  The slots of row i start at 32 i: +0 dropout;
//              +1..+4, +5..+8, +9..+12, +13..+16, +17..+20 the four uniforms of x, y, vx, vy, heading.
//              n(k) = ((u(k) + u(k+1)) + (u(k+2) + u(k+3)) - 2.0) * 1.7320508075688772: a sum of four uniforms scaled to
//              unit variance, support +-3.46; no log, no cos, so the same bits everywhere.
//   dropout    dropped when u(32 i) < p_drop
//   class      of row i, by priority: 0 absent, 2 out of range, 3 occluded, 4 dropped, 1 seen.  Row 0 has class 1.
//   noise      on a seen row:  x' = x + sigma_pos n(+1), y' = y + sigma_pos n(+5);  vx' = vx + sigma_vel n(+9),
//              vy' = vy + sigma_vel n(+13);  eps = sigma_head n(+17): heading' = heading + eps, c1 = cos_h - eps sin_h,
//              s1 = sin_h + eps cos_h, nrm = sqrt(c1 c1 + s1 s1), cos_h' = c1 / nrm, sin_h' = s1 / nrm (both unchanged when
//              nrm == 0).  A group (position, velocity, heading) whose sigma is exactly 0 is copied, not recomputed: with
//              every parameter off the output is the input bit for bit.  Each result is narrowed to f32 once; the presence
//              column is copied.
//   output     row 0 copied; the seen rows compacted to rows 1, 2, ... in their input order; every remaining row +0.0f in
//              all eight columns.  Present rows of the output are contiguous whatever the input.  Rows are NOT re-sorted:
//              the input's order by true distance is kept - a perception stack that ranks by its own (noisy) estimates is
//              not modelled.
//   accounting row_class [B][R] u8 (may be NULL): the class of every INPUT row;  counts [5][B] i64 (planar) += rows >= 1 that
//              were present, seen, out of range, occluded, dropped;  ctr [B] i64 += 1, last.  A reset launch first sets
//              ctr[b] = 0 and the five counts of b to 0, then perceives obs_true like any other launch (the reset observation
//              is seen through the same model).
#pragma once

#include <stdint.h>

#include "mpc_core.hpp"
#include "mpc_drive_metrics.hpp"
#include "mpc_synth_env.hpp"

namespace mpc {
namespace sense {

constexpr uint64_t kSalt = 0xC2B2AE3D27D4EB4Full;        // odd; xor-ed into the seed of every draw of this header
constexpr double kUnitScale = 1.7320508075688772;        // sqrt(3): four uniforms have variance 4 / 12
constexpr int kCols = 8, kMaxRows = 17, kMaxOccluders = 8, kPoints = 5, kRowSlots = 32;

enum { kAbsent = 0, kSeen = 1, kOutOfRange = 2, kOccluded = 3, kDropped = 4 };                    // row_class
enum { kCntPresent = 0, kCntSeen = 1, kCntOutOfRange = 2, kCntOccluded = 3, kCntDropped = 4, kCounts = 5 };

struct Params {
    double range, p_drop, sigma_pos, sigma_vel, sigma_head;
    uint64_t seed;
    int32_t occlusion, min_points, env_offset;
};

struct Buffers {
    int B, R, S;
    const float *obs_true;       // [B][R][8]
    const double *occluders;     // [S][4][2]
    float *obs_seen;             // [B][R][8]
    uint8_t *row_class;          // [B][R] or NULL
    int64_t *counts;             // [5][B]
    int64_t *ctr;                // [B]
};

MPC_HD double cross2(double ax, double ay, double bx, double by) {
#pragma clang fp contract(off)
    return ax * by - ay * bx;
}

// the sample points of a row: its centre, then the corners of its rectangle
MPC_HD void sample_points(const float *row, double *sx, double *sy) {
#pragma clang fp contract(off)
    sx[0] = row[1];
    sy[0] = row[2];
    drive::corners(row[1], row[2], row[7], row[6], sx + 1, sy + 1);
}

// bit t set: the sight line p -> s_t strictly crosses an edge of the quadrilateral (qx, qy)
MPC_HD unsigned hidden_points(double px, double py, const double *sx, const double *sy, const double *qx, const double *qy) {
#pragma clang fp contract(off)
    unsigned hidden = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int k1 = (k + 1) & 3;
        const double e0x = qx[k], e0y = qy[k], e1x = qx[k1], e1y = qy[k1];
        const double ex = e1x - e0x, ey = e1y - e0y;
        const double d1 = cross2(ex, ey, px - e0x, py - e0y);
#pragma unroll
        for (int t = 0; t < kPoints; ++t) {
            const double d2 = cross2(ex, ey, sx[t] - e0x, sy[t] - e0y);
            const double rx = sx[t] - px, ry = sy[t] - py;
            const double d3 = cross2(rx, ry, e0x - px, e0y - py), d4 = cross2(rx, ry, e1x - px, e1y - py);
            const bool crossing = ((d1 > 0.0 && d2 < 0.0) || (d1 < 0.0 && d2 > 0.0)) &&
                                  ((d3 > 0.0 && d4 < 0.0) || (d3 < 0.0 && d4 > 0.0));
            hidden |= crossing ? 1u << t : 0u;
        }
    }
    return hidden;
}

MPC_HD unsigned hidden_by_static(double px, double py, const double *sx, const double *sy, const double *occluders, int S) {
    unsigned hidden = 0;
    for (int s = 0; s < S; ++s) {
        double qx[4], qy[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            qx[k] = occluders[s * 8 + 2 * k];
            qy[k] = occluders[s * 8 + 2 * k + 1];
        }
        hidden |= hidden_points(px, py, sx, sy, qx, qy);
    }
    return hidden;
}

MPC_HD double unit_noise(const env::Rng &r, int k) {
#pragma clang fp contract(off)
    return ((r.u01(k) + r.u01(k + 1)) + (r.u01(k + 2) + r.u01(k + 3)) - 2.0) * kUnitScale;
}

// class of row i >= 1 (`hidden`: the union of hidden_points over its occluding edges; unused unless P.occlusion)
MPC_HD int classify(const Params &P, const env::Rng &r, int i, const float *ego, const float *row, unsigned hidden) {
#pragma clang fp contract(off)
    if (row[0] == 0.0f) return kAbsent;
    const double rx = (double)row[1] - (double)ego[1], ry = (double)row[2] - (double)ego[2];
    const double dd = rx * rx + ry * ry;
    if (dd > P.range * P.range) return kOutOfRange;
    if (P.occlusion != 0) {
        int visible = 0;
        for (int t = 0; t < kPoints; ++t) visible += (hidden >> t & 1u) ? 0 : 1;
        if (visible < P.min_points) return kOccluded;
    }
    if (r.u01(kRowSlots * i) < P.p_drop) return kDropped;
    return kSeen;
}

// the seen row i as the agent gets it
MPC_HD void noisy_row(const Params &P, const env::Rng &r, int i, const float *row, float *out) {
#pragma clang fp contract(off)
    const int k = kRowSlots * i;
    for (int c = 0; c < kCols; ++c) out[c] = row[c];
    if (P.sigma_pos != 0.0) {
        out[1] = (float)((double)row[1] + P.sigma_pos * unit_noise(r, k + 1));
        out[2] = (float)((double)row[2] + P.sigma_pos * unit_noise(r, k + 5));
    }
    if (P.sigma_vel != 0.0) {
        out[3] = (float)((double)row[3] + P.sigma_vel * unit_noise(r, k + 9));
        out[4] = (float)((double)row[4] + P.sigma_vel * unit_noise(r, k + 13));
    }
    if (P.sigma_head != 0.0) {
        const double eps = P.sigma_head * unit_noise(r, k + 17);
        const double sh = row[6], ch = row[7];
        const double c1 = ch - eps * sh, s1 = sh + eps * ch;
        const double nrm = sqrt(c1 * c1 + s1 * s1);
        out[5] = (float)((double)row[5] + eps);
        if (nrm != 0.0) {
            out[6] = (float)(s1 / nrm);
            out[7] = (float)(c1 / nrm);
        }
    }
}

// one environment, serially: the host build, and the statement the kernel's lanes split between them
MPC_HD void perceive_env(const Params &P, const Buffers &buf, int b, bool reset) {
    const int R = buf.R;
    const size_t B = (size_t)buf.B;
    const float *in = buf.obs_true + (size_t)b * R * kCols;
    float *out = buf.obs_seen + (size_t)b * R * kCols;
    const int64_t c = reset ? 0 : buf.ctr[b];
    const env::Rng r(P.seed ^ kSalt, P.env_offset + b, c);
    const double px = in[1], py = in[2];
    int64_t n[kCounts] = {0, 0, 0, 0, 0};
    for (int col = 0; col < kCols; ++col) out[col] = in[col];
    if (buf.row_class) buf.row_class[(size_t)b * R] = kSeen;
    int next = 1;
    for (int i = 1; i < R; ++i) {
        const float *row = in + i * kCols;
        unsigned hidden = 0;
        if (P.occlusion != 0) {
            double sx[kPoints], sy[kPoints];
            sample_points(row, sx, sy);
            for (int j = 1; j < R; ++j) {
                const float *other = in + j * kCols;
                if (j == i || other[0] == 0.0f) continue;
                double qx[4], qy[4];
                drive::corners(other[1], other[2], other[7], other[6], qx, qy);
                hidden |= hidden_points(px, py, sx, sy, qx, qy);
            }
            hidden |= hidden_by_static(px, py, sx, sy, buf.occluders, buf.S);
        }
        const int cls = classify(P, r, i, in, row, hidden);
        if (buf.row_class) buf.row_class[(size_t)b * R + i] = (uint8_t)cls;
        n[kCntPresent] += cls != kAbsent;
        n[kCntSeen] += cls == kSeen;
        n[kCntOutOfRange] += cls == kOutOfRange;
        n[kCntOccluded] += cls == kOccluded;
        n[kCntDropped] += cls == kDropped;
        if (cls == kSeen) noisy_row(P, r, i, row, out + (next++) * kCols);
    }
    for (int i = next; i < R; ++i)
        for (int col = 0; col < kCols; ++col) out[i * kCols + col] = 0.0f;
    for (int f = 0; f < kCounts; ++f) buf.counts[f * B + b] = (reset ? 0 : buf.counts[f * B + b]) + n[f];
    buf.ctr[b] = c + 1;
}

}  // namespace sense
}  // namespace mpc
