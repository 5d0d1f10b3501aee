// mpc_synth_lanes.hpp - the device side of the synthetic environment's step that its two kernels in mpc_engine.hip share
// (mpc_synth_env_rows_kernel, constant-velocity traffic; mpc_synth_env_idm_kernel, reactive traffic).
//
// SIXTEEN lanes per environment (four environments per wave of a 64-thread block): lane j of a group owns vehicle j (model
// step, respawn draws, crash test, its row of the observation - its place among the rows by counting the vehicles that are
// nearer, which is the stable insertion sort of env::observe), the 85 route points of the lane-centring term are scanned 16
// at a time with a min-reduction over the group (lowest index among equal distances, as the serial scan keeps the first),
// what concerns the ego alone is computed by every lane of the group.  Statement by statement the arithmetic of
// env::step_env / env::step_env_idm, whose host builds are the reference of the tests; one thread per environment spent
// 30 us per step on 256 environments - a chain of ~2000 dependent operations in 4 of the GPU's 1024 SIMDs.
//
// Every shuffle and barrier below sits in control flow that is uniform over the wave: a lane without a vehicle, or a group
// past the end of the batch, computes along and writes nothing.
#pragma once

#include <hip/hip_runtime.h>

#include "mpc_synth_traffic.hpp"

namespace mpc {
namespace env {

constexpr int kMaxRoutePoints = 128;   // what a block stages in LDS; the launch rejects a longer route

// who this lane is: lane q of group g steps vehicle j of environment b with the generator r
struct LaneGroup {
    int q, g, b, j;
    bool live, mine;    // live: the group has an environment; mine: the lane has a vehicle
    size_t vo;          // vehicle j's place in the [B][max(K, 1)] arrays
    int64_t c0;         // the environment's step counter before this step
    Rng r;
};
__device__ inline LaneGroup lane_group(int B, int K, uint64_t seed, int env_offset, const int64_t *ctr) {
    const int q = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int b_ = blockIdx.x * 4 + g;
    const bool live = b_ < B;              // a group past the end computes on the last environment and writes nothing
    const int b = live ? b_ : B - 1;
    const int Ks = K > 0 ? K : 1;
    const bool mine = q < K;
    const int j = mine ? q : 0;
    const int64_t c0 = ctr[b];
    return LaneGroup{q, g, b, j, live, mine, (size_t)b * Ks + j, c0, Rng(seed, env_offset + b, c0)};
}

// the route into LDS, by the whole block
__device__ inline void stage_route(double *s_ref, const double *ref_xy, int M) {
    for (int i = threadIdx.x; i < 2 * M; i += blockDim.x) s_ref[i] = ref_xy[i];
    __syncthreads();
}

__device__ inline bool group_any(bool flag, int g) {
    const unsigned long long flags = __ballot(flag);
    return ((flags >> (16 * g)) & 0xffffull) != 0;
}

// nearest route point to the ego: the first of the nearest, as the serial scan
__device__ inline Nearest group_nearest_route_point(const double *s_ref, int M, int q, double ex, double ey) {
    Nearest n = nearest_route_point(s_ref, M, q, 16, ex, ey);
    for (int off = 8; off >= 1; off >>= 1) {
        const double od = __shfl_xor(n.d, off, 16);
        const int oi = __shfl_xor(n.idx, off, 16);
        const bool take = od < n.d || (od == n.d && oi < n.idx);
        n.d = take ? od : n.d;
        n.idx = take ? oi : n.idx;
    }
    return n;
}

// the observation of one environment by its group: lane q's vehicle (px, py, ps, ph, active) takes the row after the vehicles
// that are nearer to the ego, lane 15 writes the ego's row; built in s_obs and copied to out
__device__ inline void synth_observe_rows(int q, int K, const Ego &e, double px, double py, double ps, double ph, bool active,
                                          float *s_obs, float *out, bool live) {
    const double x = e.x, y = e.y, th = e.th, sp = e.sp;
    for (int i = q; i < kRows * kCols; i += 16) s_obs[i] = 0.0f;
    const double dx = px - x, dy = py - y;
    const double d = active ? sqrt(dx * dx + dy * dy) : INFINITY;
    int rank = 0;
    for (int k = 0; k < K; ++k) {
        const double dk = __shfl(d, k, 16);
        const int ak = __shfl((int)active, k, 16);
        rank += (ak && (dk < d || (dk == d && k < q))) ? 1 : 0;
    }
    __syncthreads();
    if (q == 15) {
        const double s = sin(th), c = cos(th);
        s_obs[0] = 1.0f;
        s_obs[1] = (float)x;
        s_obs[2] = (float)y;
        s_obs[3] = (float)(sp * c);
        s_obs[4] = (float)(sp * s);
        s_obs[5] = (float)th;
        s_obs[6] = (float)s;
        s_obs[7] = (float)c;
    }
    if (active) {
        float *row = s_obs + (1 + rank) * kCols;
        const double sh = sin(ph), ch = cos(ph);
        row[0] = 1.0f;
        row[1] = (float)px;
        row[2] = (float)py;
        row[3] = (float)(ps * ch);
        row[4] = (float)(ps * sh);
        row[5] = (float)ph;
        row[6] = (float)sh;
        row[7] = (float)ch;
    }
    __syncthreads();
    if (live)
        for (int i = q; i < kRows * kCols; i += 16) out[i] = s_obs[i];
}

// spawn rule of the reactive traffic for lane q from what lane k offers (its position, whether it stays, whether it was drawn
// this step): clear of every lower-index vehicle that stays or was drawn, and of every higher-index one that stays
__device__ inline bool synth_spawn_clear(int q, int K, double cx, double cy, double sx, double sy, bool stays, bool drew) {
    bool clear = true;
    for (int k = 0; k < K; ++k) {
        const double kx = __shfl(sx, k, 16), ky = __shfl(sy, k, 16);
        const int kst = __shfl((int)stays, k, 16), kdr = __shfl((int)drew, k, 16);
        const bool blocks = k != q && (kst || (k < q && kdr)) && too_close(cx, cy, kx, ky);
        clear = clear && !blocks;
    }
    return clear;
}

// write-back of the state every traffic model has: vehicle j by its lane, the ego and the counters by lane 0
__device__ inline void store_state(const LaneGroup &G, const Ego &e, double px, double py, double ps, double ph, bool act,
                                   int t_next, double *ego, double *opos, double *ospeed, double *ohead, uint8_t *oactive,
                                   int32_t *t, int64_t *ctr) {
    if (G.live && G.mine) {
        opos[2 * G.vo] = px;
        opos[2 * G.vo + 1] = py;
        ospeed[G.vo] = ps;
        ohead[G.vo] = ph;
        oactive[G.vo] = act ? 1 : 0;
    }
    if (G.live && G.q == 0) {
        store_ego(ego + (size_t)G.b * 4, e);
        t[G.b] = t_next;
        ctr[G.b] = G.c0 + 1;
    }
}

__device__ inline void store_outputs(const LaneGroup &G, const StepOut &o, float *reward, uint8_t *done, uint8_t *truncated,
                                     uint8_t *crashed, uint8_t *arrived) {
    if (G.live && G.q == 0) {
        reward[G.b] = o.reward;
        done[G.b] = o.done;
        truncated[G.b] = o.truncated;
        crashed[G.b] = o.crashed;
        arrived[G.b] = o.arrived;
    }
}

}  // namespace env
}  // namespace mpc
