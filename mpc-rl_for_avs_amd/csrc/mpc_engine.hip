// mpc_engine.hip - gfx950 kernels and the C ABI (include/mpc_mi355x.h) of the batched MPC solve engine.
//
// Kernels (all: workgroup = one wave64, no inter-workgroup communication, HBM touched only for inputs / outputs):
//   mpc_solve_wave_kernel   one wave per MPC instance (mpc_wave.hpp + mpc_wave_dev.hpp): stage-parallel phases,
//                           Riccati stage on the FP64 matrix cores, all line-search step lengths at once;
//                           per-instance state (46-54 doubles per stage + trial areas, 14 KB at N = 20) in LDS
//   mpc_preamble_kernel     observation -> problem data (mpc_preamble_wave.hpp), one wave per environment
//   mpc_env_reset_kernel    episode boundaries of the per-environment detector state
// Host side: argument checks, staging of host-pointer calls through one device buffer on the caller's stream,
// per-handle device state (reference table, environment records, preamble outputs).
#include <hip/hip_runtime.h>

#include <atomic>
#include <cassert>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/mpc_mi355x.h"
#include "mpc_core.hpp"
#include "mpc_ltv.hpp"
#include "mpc_wave.hpp"
#include "mpc_wave_dev.hpp"
#include "mpc_preamble.hpp"
#include "mpc_preamble_wave.hpp"
#include "mpc_synth_lanes.hpp"
#include "mpc_rollout_glue.hpp"
#include "mpc_drive_metrics.hpp"
#include "mpc_perception.hpp"
#include "mpc_tracker.hpp"
#include "mpc_actuator.hpp"
#include "mpc_compensate.hpp"
#include "mpc_latency.hpp"
#include "mpc_interaction.hpp"
#include "mpc_episode_stats.hpp"
#include "mpc_episode_trace.hpp"
#include "mpc_plan.hpp"
#include "mpc_order.hpp"

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(MPC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));          \
    } while (0)

constexpr int kBlock = 64;  // one wave64 per workgroup
constexpr int kMaxDevices = 64;
// Waves per SIMD the wave-cooperative kernel is compiled for.  Since round 5 an instance needs 13.5 KB of LDS at N = 20 with
// the collision cost and 8 vehicles (the linearisation table and the PQ / PB table of the row-cooperative rollout,
// mpc_wave.hpp), i.e. 12 instances per CU: the throughput build is compiled for 3 waves per SIMD (166 registers, no scratch),
// which is what LDS admits anyway.  (Rounds 2 - 4: 9.9 KB, 128 registers, 4 per SIMD.)
constexpr int kWaveOcc = 3, kWaveOccGeneric = 3;
// ... except the runtime-horizon build WITH the collision cost: at 3 waves per SIMD (168 registers) it spilled two vector
// registers to scratch memory (12 B per lane, round 5); compiled for 2 waves per SIMD it has none (round 6)
constexpr int kWaveOccGenericCC = 2;
// The build for batches that do not keep the SIMDs deep in work (WaveOpsT<RELAX>, mpc_wave_dev.hpp): occupancy 2, up to 256
// registers, fresh() / opaque() the identity (everything hoisted): less time per iteration for a wave that has its SIMD to
// itself.  Used up to FOUR waves per SIMD of batch depth (B <= 4096 on 256 CUs: every BASELINE configuration): two are
// resident, the rest of a 4096 batch is dispatched as slots free, which also balances the SIMDs better than static residents,
// and the stragglers a batch ends with run at the lone-wave rate.
constexpr int kWaveOccLat = 2, kLatDepth = 4;
constexpr int kRelaxLat = 7;
// The latency builds of the fixed horizons are limited to two waves per SIMD by their registers: eight workgroups per CU, which
// leaves LDS over.  They get the spare region of mpc_wave.hpp (CTX::kSpareLds) for values that are otherwise recomputed.  Every
// other build - throughput (LDS is what limits it), runtime horizon, mpc_eval_kernel - keeps the common layout.
constexpr bool wave_spare_lds(int NC, int OCC, int RELAX) { return NC > 0 && OCC == kWaveOccLat && RELAX == kRelaxLat; }
// The same builds have registers to spare below their limit of 256: they keep same-lane values between neighbouring
// stage-parallel phases in registers (CTX::kCarry, the phase carry of mpc_wave.hpp).  No other build does.
constexpr bool wave_phase_carry(int NC, int OCC, int RELAX) { return wave_spare_lds(NC, OCC, RELAX); }

// ---------------------------------------------------------------------------------------------------
// wave-cooperative kernel: ONE wave64 per instance (mpc_wave.hpp); workgroup = 1 wave, grid = B
// ---------------------------------------------------------------------------------------------------
template <int NC, int RELAX = 0, bool SPARE = false, bool CARRY = false>
struct WaveCtx : mpc::wave::WaveOpsT<RELAX> {
    static constexpr int kN = NC;
    static constexpr bool kSpareLds = SPARE;
    static constexpr bool kCarry = CARRY;
    const double *table;  // [M][REF_COLS] in global memory (wave-uniform index in the serial parts -> scalar loads)
    int e0, M;
    __device__ __forceinline__ WaveCtx(mpc::wave::lds_double_t *l, const double *t, int e, int m)
        : mpc::wave::WaveOpsT<RELAX>{l}, table(t), e0(mpc::ego_row0(e, m)), M(m) {}
    __device__ __forceinline__ void tick(int) const {}  // section timing hook, used by tools/ubench only
    __device__ __forceinline__ double ref(int k, int c) const {
        int idx = e0 + k;
        idx = idx > M - 1 ? M - 1 : idx;
        idx = idx < 0 ? 0 : idx;
        return table[idx * mpc::REF_COLS + c];
    }
    __device__ __forceinline__ double refv(int k) const {   // speed column, stored behind the [M][REF_COLS] block
        int idx = e0 + k;
        idx = idx > M - 1 ? M - 1 : idx;
        idx = idx < 0 ? 0 : idx;
        return table[M * mpc::REF_COLS + idx];
    }
};

// inputs of instance b -> LDS: reference speeds (lane k = stage k) and other vehicles (lane j = vehicle j, advanced per stage by
// speed x dt along the heading: agents/archive/pure_mpc.py:190-191)
template <bool CC, class CTX>
__device__ __forceinline__ void stage_problem(CTX &ctx, const mpc::SolveParams &P, int b, int lane, int N, int SL,
                                              const double *__restrict__ ref5, int M, const double *__restrict__ vref,
                                              const double *__restrict__ others, int Vin) {
    const int OTH = SL * (N + 1) + mpc::wave::SC_SIZE;
    for (int node = lane; node <= N; node += kBlock) {
        double rv;
        if (vref) {
            rv = vref[(size_t)b * (N + 1) + node];
        } else {
            int idx = ctx.e0 + node;
            idx = idx > M - 1 ? M - 1 : idx;
            idx = idx < 0 ? 0 : idx;
            rv = ref5[M * mpc::REF_COLS + idx];
        }
        ctx.st(node * SL + mpc::wave::W_RV, rv);
    }
    if (CC && lane < P.V) {
        const double *ov = others + ((size_t)b * Vin + lane) * 4;
        const double sp = ov[2] * P.dt, hh = ov[3];
        ctx.st(OTH + lane * 4 + 0, ov[0]);
        ctx.st(OTH + lane * 4 + 1, ov[1]);
        ctx.st(OTH + lane * 4 + 2, sp * cos(hh));
        ctx.st(OTH + lane * 4 + 3, sp * sin(hh));
    }
}

template <bool CC, int NC, int OCC, int RELAX>
__global__ __launch_bounds__(kBlock, OCC) void mpc_solve_wave_kernel(
    mpc::SolveParams P, int B, const double *__restrict__ ref5, int M, const double *__restrict__ state,
    const int32_t *__restrict__ ego_index, const double *__restrict__ vref, const double *__restrict__ weights,
    const uint8_t *__restrict__ is_collide, const double *__restrict__ others, int Vin,
    const int32_t *__restrict__ nveh, double w_collision, const double *u_init, int u_shift, uint8_t *u_valid,
    double *__restrict__ u0_out, double *U_out, double *__restrict__ X_out, int32_t *__restrict__ status_out,
    int32_t *__restrict__ iters_out, const int32_t *__restrict__ order) {
    extern __shared__ double smem[];
    const int N = NC > 0 ? NC : P.N;
    if ((int)blockIdx.x >= B) return;            // grid = B workgroups of one wave
    // which instance this workgroup solves: workgroups start in the order of their index, and a batch that does not fit
    // the GPU at once ends with whatever started last (mpc_order_kernel below)
    const int b = order ? order[blockIdx.x] : (int)blockIdx.x;
    if (nveh) P.V = min(P.V, max(0, nveh[b]));   // vehicles actually present in this instance
    const int lane = threadIdx.x;
    constexpr int SL = mpc::wave::stage_slots(CC);
    using Ctx = WaveCtx<NC, RELAX, wave_spare_lds(NC, OCC, RELAX), wave_phase_carry(NC, OCC, RELAX)>;
    Ctx ctx((mpc::wave::lds_double_t *)smem, ref5, ego_index[b], M);
    stage_problem<CC>(ctx, P, b, lane, N, SL, ref5, M, vref, others, Vin);
    __syncthreads();
    double x0[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) x0[i] = state[(size_t)b * 4 + i];
    const bool collide = is_collide[b] != 0;
    const double ws_ = collide ? 100.0 : weights[(size_t)b * 3 + 0];  // agents/pure_mpc.py:143-147
    const double wcoll = (CC && collide) ? 3000.0 * w_collision : 0.0;
    mpc::wave::Solver<CC, Ctx> solver(P, ctx, x0, ws_, weights[(size_t)b * 3 + 1], weights[(size_t)b * 3 + 2], wcoll);
    int status, iters, cur;
    double kkt;
    // opt-in warm start: initial controls u_init[b][min(k + u_shift, N-1)] (u_shift = 1: the previous solution of this
    // environment advanced by one stage), where u_valid (if given) says that there is one.  u_init may alias U_out: it
    // is read here, before the solve, and written after it by the same wave.
    const bool warm = u_init != nullptr && (u_valid == nullptr || u_valid[b] != 0);
    if (warm && lane < N) {
        const int src = min(lane + u_shift, N - 1);
        ctx.st(lane * SL + mpc::wave::W_U + 0, mpc::warm_clamp(u_init[((size_t)b * N + src) * 2 + 0], 0));
        ctx.st(lane * SL + mpc::wave::W_U + 1, mpc::warm_clamp(u_init[((size_t)b * N + src) * 2 + 1], 1));
    }
    __syncthreads();
    solver.solve(status, iters, cur, kkt, warm);
    __syncthreads();
    const int CB = cur * 6;
    // only a converged solve may seed the next warm start
    if (P.strict_kink && (status == MPC_STATUS_CONVERGED_ON_KINK || status == MPC_STATUS_ACCEPTABLE_ON_KINK))
        status = MPC_STATUS_KINK_UNSOLVED;      // MPC_FLAG_STRICT_DISCONTINUITY: same iterate, reported as the reference's IPOPT would
    if (lane == 0 && u_valid && U_out) u_valid[b] = MPC_STATUS_IS_SOLVED(status) ? 1 : 0;
    if (lane < 2) u0_out[(size_t)b * 2 + lane] = ctx.ld(CB + mpc::wave::W_U + lane);
    if (U_out && lane < N) {
        U_out[((size_t)b * N + lane) * 2 + 0] = ctx.ld(lane * SL + CB + mpc::wave::W_U + 0);
        U_out[((size_t)b * N + lane) * 2 + 1] = ctx.ld(lane * SL + CB + mpc::wave::W_U + 1);
    }
    if (X_out)
        for (int node = lane; node <= N; node += kBlock)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                X_out[((size_t)b * (N + 1) + node) * 4 + i] = ctx.ld(node * SL + CB + mpc::wave::W_X + i);
    if (lane == 0) {
        if (status_out) status_out[b] = status;
        if (iters_out) iters_out[b] = iters;
    }
}

// X of the instances that ended with MPC_STATUS_INFEASIBLE_START: the solve kernel's start rollout stops at the first node
// outside the bounds and leaves the rows behind it as they were; one thread per instance rolls the returned controls out
// to the end (mpc::infeasible_start_rollout).  A kernel of its own, enqueued behind the solve when U, X and status are all
// asked for: any line added to the solve kernel itself moves the register allocation of its compiled-horizon builds.
__global__ __launch_bounds__(256) void mpc_infeasible_start_kernel(int B, int N, double dt, const double *__restrict__ state,
                                                                   const double *__restrict__ U,
                                                                   const int32_t *__restrict__ status, double *__restrict__ X) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B || status[b] != MPC_STATUS_INFEASIBLE_START) return;
    mpc::infeasible_start_rollout(state + (size_t)b * 4, U + (size_t)b * N * 2, N, dt, X + (size_t)b * (N + 1) * 4);
}

// one wave that ends `ticks` of the constant 100 MHz clock after it started (mpc_streams_overlap): the clock advances whatever
// the wave does, so the loop ends
__global__ __launch_bounds__(64) void mpc_timer_kernel(long long ticks) {
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}

// Launch order of a batch.  The hardware starts workgroups in index order, a SIMD's issue arbiter favours its oldest wave,
// and a batch lasts as long as its slowest instance - so the instances likely to be slow should be the first to start, and
// there should be no more of them than the GPU holds at once (2048 waves of the latency build).  The cheap predictors this NLP
// offers (oracle iteration counts of eight draws of 4096, profiles/r04_launch_order.txt): instances WITH a predicted collision
// are easy (w_s = 100, agents/pure_mpc.py:143-147, makes the speed term dominate: 99th percentile 26 - 29 iterations against
// 45 - 50 without; of the instances with >= 50 iterations 90 - 100 % have is_collide = 0) unless the ego stands still (speed on
// its bound 0: every exception found); and with the collision cost on, an instance without a vehicle within 15 m of the ego is
// the easy live objective in all but name (no instance with >= 70 iterations had its nearest vehicle farther away, unless it
// stood still).  Tiers, each in its original order (a stable partition): 1 = standing ego, or no predicted collision
// and (collision cost off or a vehicle within kNear); 2 = the other instances without a predicted collision; 3 = a predicted
// collision while the route turns; 4 = the rest; tier 0 is the seat tier below.  (Tier 4, round 6: with a predicted collision the instances that still need
// >= 60 iterations - 3 to 6 of 65 536, one or two of them at the cap - sit where the reference heading changes between five rows
// behind the ego and the end of the look-ahead, 15 of 16 over four draws; started last, one of them alone is 13 % of a bulk
// launch.  The straight-route half of what was one tier, 28 % of a batch with a maximum of 41 - 58 iterations, now ends the launch:
// 65 536 instances 21.2 -> 19.6 ms in the occupancy model that reproduced the three-tier measurements to 0.2 ms.)
// (Round 5 also built "what the same environment needed one step ago" as the first key for the closed loop; measured neutral to
// negative - profiles/r05_launch_order_prev.txt, docs/NOT_ADOPTED.md - and removed in round 6 together with its per-environment
// record and the environment variable that switched it on.)
// (The tier functions live in mpc_order.hpp, host and device: tests/test_order_tiers_cpu.py calls them on the CPU.)
//
// The seat tier (tier 0, `seats`): the latency build holds two waves per SIMD, and workgroups p and p + 1024 share one
// (tools/ubench/seat_probe.hip, profiles/seat_probe.txt: on 930 - 1024 of the 1024 SIMDs, the rest at a distance of 768;
// the lower index is the one that runs near the lone rate, x 1.06 - 1.08 against x 1.29 - 1.31 for its mate on an FP64 chain).
// The first of the tiers above holds 1550 - 1700 of 4096, so a third of it sits in the younger seats, where a cap-runner
// runs beside a mate of its own tier at the leftover rate.  Where ONE batch of the latency build is solved with the collision
// cost on, a narrower tier goes in front (mpc::order::first_seat: standing ego, or no predicted collision, a moving ego and a
// vehicle whose closest approach within the horizon is below 5 m): 950 - 1074 of 4096 (seeds 0 - 23) with the recall of the wider tier on
// the instances with >= 60 iterations (tools/seat_model.py, profiles/seat_tier_model.txt).  Bulk launches, launches without
// vehicles and the live objective keep the four tiers: with tier 0 empty the order is the one they always had.
// Measured against the four tiers alone (profiles/seat_tier.txt, builds alternating, five fresh processes each): the headline batch
// 3.731 - 3.739 -> 3.556 - 3.572 ms (-4.5 %), results equal array for array; seeds 0 - 7 mean -2.9 %, seed 6 +1.8 %; caps 40 / 60
// not slower / -7 %.
// The seat tier's closest approach costs two FP64 sin / cos and a reciprocal per vehicle: computed inside the one workgroup of
// mpc_order_kernel it made that kernel 61 us on the headline batch (one CU, issue-bound; the parent's took 19), so where the seat
// tier applies the tiers are written by this kernel first, one wave per 64 instances over as many CUs: 8.7 us, and the order
// kernel behind it 7.7 us (rocprofv3 kernel trace, profiles/seat_tier.txt).
__global__ __launch_bounds__(64) void mpc_tier_kernel(int B, const uint8_t *__restrict__ is_collide,
                                                      const double *__restrict__ state, const double *__restrict__ others, int V,
                                                      const int32_t *__restrict__ nveh, const int32_t *__restrict__ ego,
                                                      const double *__restrict__ ref5, int M, int N, double T,
                                                      int32_t *__restrict__ tier) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < B) tier[i] = mpc::order::tier_of(is_collide, state, others, V, nveh, ego, ref5, M, N, i, true, T);
}
// `tiers_given`: mpc_tier_kernel has filled `tier` (the seat tier applies); otherwise the four tiers are computed here, as ever.
__global__ __launch_bounds__(1024) void mpc_order_kernel(int B, const uint8_t *__restrict__ is_collide,
                                                         const double *__restrict__ state, const double *__restrict__ others,
                                                         int V, const int32_t *__restrict__ nveh, const int32_t *__restrict__ ego,
                                                         const double *__restrict__ ref5, int M, int N, int tiers_given,
                                                         int32_t *__restrict__ order, int32_t *tier) {
    __shared__ int s_c0[1024], s_c1[1024], s_c2[1024], s_c3[1024];
    const int t = threadIdx.x, chunk = (B + 1023) / 1024, lo = min(B, t * chunk), hi = min(B, lo + chunk);
    // tiers first, every thread an interleaved share (neighbouring threads read neighbouring instances), kept in scratch
    if (!tiers_given)
        for (int i = t; i < B; i += 1024)
            tier[i] = mpc::order::tier_of(is_collide, state, others, V, nveh, ego, ref5, M, N, i, false, 0.0);
    __syncthreads();
    int n0 = 0, n1 = 0, n2 = 0, n3 = 0;
    for (int i = lo; i < hi; ++i) {
        const int k = tier[i];
        n0 += k == 0;
        n1 += k == 1;
        n2 += k == 2;
        n3 += k == 3;
    }
    s_c0[t] = n0;
    s_c1[t] = n1;
    s_c2[t] = n2;
    s_c3[t] = n3;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {          // inclusive scans of the tier counts
        const int v0 = t >= d ? s_c0[t - d] : 0, v1 = t >= d ? s_c1[t - d] : 0, v2 = t >= d ? s_c2[t - d] : 0,
                  v3 = t >= d ? s_c3[t - d] : 0;
        __syncthreads();
        s_c0[t] += v0;
        s_c1[t] += v1;
        s_c2[t] += v2;
        s_c3[t] += v3;
        __syncthreads();
    }
    const int tot0 = s_c0[1023], tot1 = s_c1[1023], tot2 = s_c2[1023], tot3 = s_c3[1023];
    const int b0 = s_c0[t] - n0, b1 = s_c1[t] - n1, b2 = s_c2[t] - n2, b3 = s_c3[t] - n3;   // members of tiers 0..3 before this chunk
    int p0 = b0, p1 = tot0 + b1, p2 = tot0 + tot1 + b2, p3 = tot0 + tot1 + tot2 + b3,
        p4 = tot0 + tot1 + tot2 + tot3 + (lo - b0 - b1 - b2 - b3);
    for (int i = lo; i < hi; ++i) {
        const int k = tier[i];
        if (k == 0) order[p0++] = i;
        else if (k == 1) order[p1++] = i;
        else if (k == 2) order[p2++] = i;
        else if (k == 3) order[p3++] = i;
        else order[p4++] = i;
    }
}

// diagnostics (mpc_eval_nlp): the NLP's objective and model step at given points, through Solver::evaluate() of the build
// for runtime horizons (the same class template as every solve kernel); one wave per point
template <bool CC>
__global__ __launch_bounds__(kBlock) void mpc_eval_kernel(mpc::SolveParams P, int B, const double *__restrict__ ref5, int M,
                                                          const int32_t *__restrict__ ego_index, const double *__restrict__ vref,
                                                          const double *__restrict__ weights, const uint8_t *__restrict__ is_collide,
                                                          const double *__restrict__ others, int Vin, double w_collision,
                                                          const double *__restrict__ X, const double *__restrict__ U,
                                                          double *__restrict__ f_out, double *__restrict__ xnext_out) {
    extern __shared__ double smem[];
    const int N = P.N, b = blockIdx.x, lane = threadIdx.x;
    if (b >= B) return;
    constexpr int SL = mpc::wave::stage_slots(CC);
    WaveCtx<0, 0> ctx((mpc::wave::lds_double_t *)smem, ref5, ego_index[b], M);
    stage_problem<CC>(ctx, P, b, lane, N, SL, ref5, M, vref, others, Vin);
    for (int node = lane; node <= N; node += kBlock) {
        for (int i = 0; i < 4; ++i) ctx.st(node * SL + mpc::wave::W_X + i, X[((size_t)b * (N + 1) + node) * 4 + i]);
        if (node < N)
            for (int i = 0; i < 2; ++i) ctx.st(node * SL + mpc::wave::W_U + i, U[((size_t)b * N + node) * 2 + i]);
    }
    __syncthreads();
    double x0[4];
    for (int i = 0; i < 4; ++i) x0[i] = X[(size_t)b * (N + 1) * 4 + i];
    const bool collide = is_collide[b] != 0;
    const double ws_ = collide ? 100.0 : weights[(size_t)b * 3 + 0];
    const double wcoll = (CC && collide) ? 3000.0 * w_collision : 0.0;
    mpc::wave::Solver<CC, WaveCtx<0, 0>> solver(P, ctx, x0, ws_, weights[(size_t)b * 3 + 1], weights[(size_t)b * 3 + 2], wcoll);
    mpc::wave::PerLane<double> xn[4];
    const double f = solver.evaluate(xn);
    if (lane == 0) f_out[b] = f;
    if (lane < N)
        for (int i = 0; i < 4; ++i) xnext_out[((size_t)b * N + lane) * 4 + i] = xn[i].at(lane);
}

// ---------------------------------------------------------------------------------------------------
// iterative-linear MPC (mpc_ltv.hpp; reference agents/pure_mpc_linear.py): ONE wave64 per instance, grid = B.
// The ego state comes either from `state` ([B][4] x, y, v, yaw) or straight from the observation (`obs`, row 0 parsed
// as agents/base_agent.py:96-102 does).  U holds the stored control profile (oa, od) on entry and, where the QP was
// solved, the new one on exit; elsewhere it is left alone and the action is (0, 0) (pure_mpc_linear.py:193-196).
// ---------------------------------------------------------------------------------------------------
// Two builds, as for the solve kernel: OCC 3 (<= 168 registers, nothing spilled; LDS admits 12 instances per CU at N = 20
// anyway) keeps the role tables and uniform constants out of registers by recomputing them (opaque / fresh); OCC 2 with
// both relaxed lets the compiler hoist them - 5 % less time per solve when the batch leaves the SIMDs that empty.
template <int OCC, int RELAX>
__global__ __launch_bounds__(kBlock, OCC) void mpc_ltv_kernel(
    mpc::ltv::LtvParams P, int B, const double *__restrict__ ref5, int M, const double *__restrict__ state,
    const float *__restrict__ obs, int rows, double *U, double *__restrict__ u0_out, double *__restrict__ X_out,
    int32_t *__restrict__ status_out, int32_t *__restrict__ iters_out, int32_t *__restrict__ target_out) {
    namespace ltv = mpc::ltv;
    extern __shared__ double smem[];
    const int N = P.N;
    const int b = blockIdx.x;
    if (b >= B) return;
    const int lane = threadIdx.x;
    double x0[4];   // x, y, yaw, v
    if (obs) {
        const float *ob = obs + (size_t)b * rows * mpc::pre::kObsCols;
        x0[0] = (double)ob[1];
        x0[1] = (double)ob[2];
        x0[2] = (double)mpc::pre::normalize_angle_f32(ob[5]);
        x0[3] = (double)mpc::pre::speed_f32(ob[3], ob[4]);
    } else {
        x0[0] = state[(size_t)b * 4 + 0];
        x0[1] = state[(size_t)b * 4 + 1];
        x0[2] = state[(size_t)b * 4 + 3];
        x0[3] = state[(size_t)b * 4 + 2];
    }
    WaveCtx<0, RELAX> ctx((mpc::wave::lds_double_t *)smem, ref5, 0, M);
    // nearest reference point, first minimum of the squared distance (calc_nearest_index_in_direction, :38-60);
    // products and sum rounded separately like the Python expression
    {
        double best = INFINITY;
        int bidx = 0;
        for (int i = lane; i < M; i += kBlock) {
            const double dx = ref5[i * mpc::REF_COLS + mpc::R_X] - x0[0], dy = ref5[i * mpc::REF_COLS + mpc::R_Y] - x0[1];
            const double d = mpc::pre::f64add(mpc::pre::f64mul(dx, dx), mpc::pre::f64mul(dy, dy));
            if (d < best) {
                best = d;
                bidx = i;
            }
        }
        mpc::wave::PerLane<double> pv, pi;
        pv.v = best;
        const double m = ctx.wave_min(pv);
        pi.v = best == m ? (double)bidx : 1e9;
        ctx.e0 = (int)ctx.wave_min(pi);
    }
    if (lane < N) {
        ctx.st(lane * ltv::L_SLOTS + ltv::L_U + 0, U[((size_t)b * N + lane) * 2 + 0]);
        ctx.st(lane * ltv::L_SLOTS + ltv::L_U + 1, U[((size_t)b * N + lane) * 2 + 1]);
    }
    __syncthreads();
    ltv::Solver<WaveCtx<0, RELAX>> solver(P, ctx, x0);
    // the loop of :189: every pass re-simulates the profile the previous one stored and solves the QP linearised
    // about it; the first pass that fails ends the call with the action (0, 0) and the profile stored so far
    int status = ltv::ST_MAX_ITER, iters = 0;
    bool ok = false;
#pragma unroll 1
    for (int pass = 0; pass < P.passes; ++pass) {
        int it = 0;
        solver.solve(status, it);
        iters += it;
        __syncthreads();
        ok = status == ltv::ST_CONVERGED;
        if (!ok) break;
        const int ul = ctx.opaque(lane);   // the row address is formed here, not carried in registers through the solve
        if (ul < N) {
            U[((size_t)b * N + ul) * 2 + 0] = ctx.ld(ul * ltv::L_SLOTS + ltv::L_U + 0);
            U[((size_t)b * N + ul) * 2 + 1] = ctx.ld(ul * ltv::L_SLOTS + ltv::L_U + 1);
        }
    }
    if (lane < 2) u0_out[(size_t)b * 2 + lane] = ok ? ctx.ld(ltv::L_U + lane) : 0.0;
    if (X_out && status != ltv::ST_INFEASIBLE)
        for (int node = lane; node <= N; node += kBlock) {
            double *o = X_out + ((size_t)b * (N + 1) + node) * 4;
            o[0] = ctx.ld(node * ltv::L_SLOTS + ltv::L_X + 0);
            o[1] = ctx.ld(node * ltv::L_SLOTS + ltv::L_X + 1);
            o[2] = ctx.ld(node * ltv::L_SLOTS + ltv::L_X + 3);
            o[3] = ctx.ld(node * ltv::L_SLOTS + ltv::L_X + 2);
        }
    if (lane == 0) {
        if (status_out) status_out[b] = status;
        if (iters_out) iters_out[b] = iters;
        if (target_out) target_out[b] = ctx.e0;
    }
}

// ---------------------------------------------------------------------------------------------------
// observation -> problem data: ONE wave per environment (mpc_preamble_wave.hpp says which lanes do what).  Workgroup = one
// wave, grid = B, 20 KB of LDS (predicted paths, running arc lengths - later the sorted nodes and middles of collinear stretches -, crossing candidates), nothing in scratch.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock, 2) void mpc_preamble_kernel(
    int B, const float *__restrict__ obs, int rows, const double *__restrict__ ref5, int M, int N, double dt,
    const double *__restrict__ ref_speed, mpc::pre::EnvState *__restrict__ env, double *__restrict__ state,
    int32_t *__restrict__ ego_index, double *__restrict__ vref, uint8_t *__restrict__ is_collide,
    double *__restrict__ others, int Vslots, int32_t *__restrict__ nveh, int advance, double *__restrict__ dbg_ego,
    int32_t *__restrict__ dbg_len, float *__restrict__ dbg_agents) {
    namespace pre = mpc::pre;
    __shared__ double s_words[pre::preamble_wave_lds_doubles()];
    __shared__ int32_t s_conf[pre::kMaxOthers];
    __shared__ pre::P2 s_cpt[pre::kMaxOthers];
    const int b = blockIdx.x;
    if (b >= B) return;
    WaveCtx<0, 3> ctx((mpc::wave::lds_double_t *)s_words, ref5, 0, M);
    const pre::RefTable R{ref5, M};
    constexpr size_t P = pre::kPredHorizon + 1;
    const pre::PreDiag diag{dbg_len ? dbg_ego + (size_t)b * P * 2 : nullptr, dbg_len ? dbg_len + b : nullptr,
                            dbg_len ? dbg_agents + (size_t)b * Vslots * P * 2 : nullptr, Vslots};
    pre::preamble_env_wave(ctx, obs + (size_t)b * rows * pre::kObsCols, rows, R, N, dt, ref_speed ? ref_speed + b : nullptr,
                           env[b], state + (size_t)b * 4, ego_index[b], vref + (size_t)b * (N + 1), is_collide[b],
                           others + (size_t)b * Vslots * 4, Vslots, nveh[b], advance != 0, s_conf, s_cpt, diag);
}

__global__ void mpc_env_reset_kernel(int n, const int32_t *__restrict__ ids, const uint8_t *__restrict__ mask,
                                     mpc::pre::EnvState *__restrict__ env, uint8_t *__restrict__ warm_valid, int cap,
                                     int warm_only, double *__restrict__ ltv_u, int ltv_row) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = ids ? ids[i] : i;
    if (b < 0 || b >= cap) return;
    if (mask && !mask[i]) return;
    if (!warm_only) env[b] = mpc::pre::EnvState{};
    warm_valid[b] = 0;
    if (ltv_u)                      // stored profile of the iterative-linear agent: oa = od = None -> zeros
        for (int i = 0; i < ltv_row; ++i) ltv_u[(size_t)b * ltv_row + i] = 0.0;
}

// ---------------------------------------------------------------------------------------------------
// synthetic intersection environment (mpc_synth_env.hpp): step + terminal observation + auto-reset + next observation in ONE
// launch (the torch implementation of the same step is ~100 small kernels)
// ---------------------------------------------------------------------------------------------------
// The lane-group pieces the two kernels share (who a lane is, route staging, nearest route point, observation, write-back)
// are in mpc_synth_lanes.hpp; each kernel below reads top to bottom as the steps of its traffic model.
__global__ __launch_bounds__(64) void mpc_synth_env_rows_kernel(
    int B, int K, double dt, double spawn_probability, uint64_t seed, int env_offset, const double *__restrict__ ref_xy,
    int M, const double *__restrict__ action, double *__restrict__ ego, double *__restrict__ opos,
    double *__restrict__ ospeed, double *__restrict__ ohead, uint8_t *__restrict__ oactive, int32_t *__restrict__ t,
    int64_t *__restrict__ ctr, float *__restrict__ obs, float *__restrict__ terminal_obs, float *__restrict__ reward,
    uint8_t *__restrict__ done, uint8_t *__restrict__ truncated, uint8_t *__restrict__ crashed,
    uint8_t *__restrict__ arrived, int reset_all) {
    namespace env = mpc::env;
    constexpr int kObs = env::kRows * env::kCols;
    __shared__ double s_ref[2 * env::kMaxRoutePoints];
    __shared__ float s_obs[4][kObs];
    env::stage_route(s_ref, ref_xy, M);
    const env::LaneGroup G = env::lane_group(B, K, seed, env_offset, ctr);
    const int q = G.q, j = G.j;
    float *o = obs + (size_t)G.b * kObs;
    double px = 0.0, py = 0.0, ps = 0.0, ph = 0.0;
    if (reset_all) {
        if (G.mine) env::spawn_other(G.r, env::kSlotReset + 4 * j, 5.0, 60.0, px, py, ps, ph);
        const env::Ego e = env::fresh_ego(G.r);
        env::synth_observe_rows(q, K, e, px, py, ps, ph, G.mine, s_obs[G.g], o, G.live);
        env::store_state(G, e, px, py, ps, ph, G.mine, 0, ego, opos, ospeed, ohead, oactive, t, ctr);
        return;
    }
    // ---- ego
    env::Ego e = env::step_ego(env::load_ego(ego + (size_t)G.b * 4), action + (size_t)G.b * 2, dt);
    // ---- vehicle j
    bool act = false, hit = false;
    if (G.mine) {
        px = opos[2 * G.vo]; py = opos[2 * G.vo + 1]; ps = ospeed[G.vo]; ph = ohead[G.vo];
        act = oactive[G.vo] != 0;
        hit = env::step_other(G.r, j, dt, spawn_probability, e.x, e.y, px, py, ps, ph, act);
    }
    const bool crash = env::group_any(hit, G.g);
    // ---- reward and termination
    const env::Nearest n = env::group_nearest_route_point(s_ref, M, q, e.x, e.y);
    const int tn = t[G.b] + 1;
    const env::StepOut so = env::score_step(n.d, n.idx, M, crash, e.sp, tn);
    env::synth_observe_rows(q, K, e, px, py, ps, ph, act, s_obs[G.g], terminal_obs + (size_t)G.b * kObs, G.live);
    if (so.done) {      // uniform over the group
        e = env::fresh_ego(G.r);
        if (G.mine) env::spawn_other(G.r, env::kSlotReset + 4 * j, 5.0, 60.0, px, py, ps, ph);
        act = G.mine;
    }
    // (a group that goes on rebuilds the same observation: the four groups of a wave stay in step for the barriers inside)
    env::synth_observe_rows(q, K, e, px, py, ps, ph, act, s_obs[G.g], o, G.live);
    env::store_state(G, e, px, py, ps, ph, act, so.done ? 0 : tn, ego, opos, ospeed, ohead, oactive, t, ctr);
    env::store_outputs(G, so, reward, done, truncated, crashed, arrived);
}

// ---- the same step with reactive traffic (mpc_synth_traffic.hpp; traffic = "idm"), with the same mapping: lane j of a 16-lane
// group owns vehicle j.  Its corridor scan and the spawn rule are loops over k < K of group shuffles of what lane k holds, the
// shape of the rank count in synth_observe_rows; every shuffle sits in control flow that is uniform over the wave (a lane
// without a vehicle, or a group whose episode goes on, computes along and discards), and all four groups reach every barrier.
__global__ __launch_bounds__(64) void mpc_synth_env_idm_kernel(
    int B, int K, double dt, double spawn_probability, uint64_t seed, int env_offset, const double *__restrict__ ref_xy,
    int M, const double *__restrict__ action, double *__restrict__ ego, double *__restrict__ opos,
    double *__restrict__ ospeed, double *__restrict__ ohead, uint8_t *__restrict__ oactive, int32_t *__restrict__ oroute,
    double *__restrict__ oprog, double *__restrict__ otarget, int32_t *__restrict__ t, int64_t *__restrict__ ctr,
    float *__restrict__ obs, float *__restrict__ terminal_obs, float *__restrict__ reward, uint8_t *__restrict__ done,
    uint8_t *__restrict__ truncated, uint8_t *__restrict__ crashed, uint8_t *__restrict__ arrived, int reset_all) {
    namespace env = mpc::env;
    constexpr int kObs = env::kRows * env::kCols;
    __shared__ double s_ref[2 * env::kMaxRoutePoints];
    __shared__ float s_obs[4][kObs];
    env::stage_route(s_ref, ref_xy, M);
    const env::LaneGroup G = env::lane_group(B, K, seed, env_offset, ctr);
    const int q = G.q, j = G.j;
    const size_t vo = G.vo;
    double px = 0.0, py = 0.0, ps = 0.0, ph = 0.0, prog = 0.0, target = 1.0;
    int route = 0;
    bool act = false;
    env::Ego e = {};
    env::StepOut so = {};
    so.done = 1;        // a reset launch: every episode starts afresh
    int tn = 0;
    if (!reset_all) {
        // ---- ego
        const env::Ego e0 = env::load_ego(ego + (size_t)G.b * 4);
        e = env::step_ego(e0, action + (size_t)G.b * 2, dt);
        // ---- vehicle j: its leader among the ego and the others as they were before the step
        if (G.mine) {
            px = opos[2 * vo]; py = opos[2 * vo + 1]; ps = ospeed[vo]; ph = ohead[vo];
            act = oactive[vo] != 0;
            route = oroute[vo]; prog = oprog[vo]; target = otarget[vo];
        }
        const double cj = cos(ph), sj = sin(ph);
        env::Leader lead = env::no_leader();
        env::offer_leader(lead, q, px, py, ph, cj, sj, -1, e0.x, e0.y, e0.th, e0.sp);
        for (int k = 0; k < K; ++k) {
            const double kx = __shfl(px, k, 16), ky = __shfl(py, k, 16), kh = __shfl(ph, k, 16), kv = __shfl(ps, k, 16);
            const int ka = __shfl((int)act, k, 16);
            if (k != q && ka) env::offer_leader(lead, q, px, py, ph, cj, sj, k, kx, ky, kh, kv);
        }
        // a circle of vehicles waiting for each other: its lowest index drives free (env::walk_leaders)
        const int who = G.mine && act ? lead.who : -2;
        int wp = who, lowest = q;
        bool closed = false;
        for (int n = 0; n < K; ++n) {
            const int next = __shfl(who, wp >= 0 ? wp : 0, 16);
            env::walk_leaders(q, wp >= 0 ? next : -2, wp, lowest, closed);
        }
        if (closed && lowest == q) lead = env::no_leader();
        // ---- it moves; one that left (or was away) draws its respawn and is placed where the spawn rule allows
        bool stays = false, drew = false;
        env::Drawn cand = {};
        if (G.mine) {
            if (act) {
                const double acc = env::idm_acceleration(ps, target, ph, lead);
                env::advance(acc, dt, prog, ps);
                env::pose(route, prog, px, py, ph);
                stays = !env::left_the_map(px, py);
            }
            drew = !stays && G.r.u01(env::kSlotRespawn + 5 * j) < spawn_probability;
            if (drew) cand = env::draw_vehicle(G.r, env::kSlotRespawn + 5 * j + 1, env::kSlotTurnRespawn + j, 40.0, 60.0);
        }
        const bool clear = env::synth_spawn_clear(q, K, cand.x, cand.y, stays ? px : cand.x, stays ? py : cand.y, stays, drew);
        bool hit = false;
        if (G.mine) {
            if (!stays) {
                act = drew && clear;
                if (act) {
                    px = cand.x; py = cand.y; ps = cand.speed; ph = cand.h;
                    route = cand.route; prog = cand.s; target = cand.target;
                }
            }
            hit = act && env::hits_ego(px, py, e.x, e.y);
        }
        const bool crash = env::group_any(hit, G.g);
        // ---- reward and termination
        const env::Nearest n = env::group_nearest_route_point(s_ref, M, q, e.x, e.y);
        tn = t[G.b] + 1;
        so = env::score_step(n.d, n.idx, M, crash, e.sp, tn);
        env::synth_observe_rows(q, K, e, px, py, ps, ph, act, s_obs[G.g], terminal_obs + (size_t)G.b * kObs, G.live);
    }
    // ---- fresh episode (every group of a reset launch, the groups whose episode ended otherwise; uniform over a group)
    const bool fin = so.done;
    env::Drawn fresh = {};
    if (fin && G.mine) fresh = env::draw_vehicle(G.r, env::kSlotReset + 4 * j, env::kSlotTurnReset + j, 5.0, 60.0);
    const bool placed = env::synth_spawn_clear(q, K, fresh.x, fresh.y, fresh.x, fresh.y, false, fin && G.mine);
    if (fin) {
        e = env::fresh_ego(G.r);
        if (G.mine) {
            px = fresh.x; py = fresh.y; ps = fresh.speed; ph = fresh.h;
            route = fresh.route; prog = fresh.s; target = fresh.target;
            act = placed;
        }
    }
    // (a group that goes on rebuilds the same observation: the four groups of a wave stay in step for the barriers inside)
    env::synth_observe_rows(q, K, e, px, py, ps, ph, act, s_obs[G.g], obs + (size_t)G.b * kObs, G.live);
    env::store_state(G, e, px, py, ps, ph, act, fin ? 0 : tn, ego, opos, ospeed, ohead, oactive, t, ctr);
    if (G.live && G.mine) {
        oroute[vo] = route;
        oprog[vo] = prog;
        otarget[vo] = target;
    }
    if (!reset_all) env::store_outputs(G, so, reward, done, truncated, crashed, arrived);
}

// ---------------------------------------------------------------------------------------------------
// rollout glue (mpc_rollout_glue.hpp): the policy forward + sample + MPC inputs, and the buffer row / carry-over /
// counters of a step.  One workgroup per environment.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(mpc::glue::kMaxHidden2) void mpc_policy_act_kernel(
    int B, int A, int H2, const float *__restrict__ obs, mpc::glue::PolicyWeights W, float *noise,
    unsigned long long noise_seed, int env_offset, const long long *__restrict__ noise_step,
    int version_v1, int clip, float *__restrict__ actions, float *__restrict__ values, float *__restrict__ log_probs,
    double *__restrict__ mpc_weights, double *__restrict__ mpc_ref_speed) {
    namespace glue = mpc::glue;
    __shared__ float s_x[glue::kObsDim];
    __shared__ float s_h1[glue::kMaxHidden2], s_h2[glue::kMaxHidden2];
    __shared__ float s_head[glue::kMaxAction + 1];
    const int b = blockIdx.x, j = threadIdx.x;
    if (b >= B) return;
    if (j < glue::kObsDim) s_x[j] = obs[(size_t)b * glue::kObsDim + j];
    // the sample's noise: drawn here (and left in `noise` for the caller to see) or handed in
    if (noise_step && j < A) noise[(size_t)b * A + j] = glue::policy_noise(noise_seed, env_offset + b, *noise_step, j);
    __syncthreads();
    if (j < H2) s_h1[j] = glue::layer1_unit(W, H2, s_x, j);
    __syncthreads();
    if (j < H2) s_h2[j] = glue::layer2_unit(W, H2, s_h1, j);
    __syncthreads();
    if (j <= A) s_head[j] = glue::head_unit(W, H2, A, s_h2, j);
    __syncthreads();
    if (j == 0)
        glue::finish_action(W, A, s_head, noise + (size_t)b * A, version_v1, clip, nullptr, actions + (size_t)b * A, values + b,
                            log_probs + b, mpc_weights ? mpc_weights + (size_t)b * 3 : nullptr,
                            mpc_ref_speed ? mpc_ref_speed + b : nullptr);
}

// the gSDE form of the same step (mpc_rollout_glue.hpp): thread h < H also holds row h of the environment's exploration matrix
// E = std * Z in LDS (Z drawn here, A Box-Muller draws per thread, or read from the caller); after layer 2 the H policy units
// are the latent, and threads 64 .. 64 + 2A (the second wave, next to the heads on the first) reduce the noise latent @ E and
// the variance latent^2 @ std^2 in index order
__global__ __launch_bounds__(mpc::glue::kMaxHidden2) void mpc_policy_act_sde_kernel(
    int B, int A, int H2, const float *__restrict__ obs, mpc::glue::PolicyWeights W, const float *__restrict__ sde_noise,
    unsigned long long noise_seed, int env_offset, const long long *__restrict__ sde_epoch,
    const long long *__restrict__ sde_step, int sde_sample_freq, int version_v1, int clip, float *__restrict__ actions,
    float *__restrict__ values, float *__restrict__ log_probs, double *__restrict__ mpc_weights,
    double *__restrict__ mpc_ref_speed) {
    namespace glue = mpc::glue;
    __shared__ float s_x[glue::kObsDim];
    __shared__ float s_h1[glue::kMaxHidden2], s_h2[glue::kMaxHidden2];
    __shared__ float s_head[glue::kMaxAction + 1];
    __shared__ float s_e[glue::kMaxHidden2 / 2 * glue::kMaxAction];
    __shared__ float s_sum[2 * glue::kMaxAction];
    const int b = blockIdx.x, j = threadIdx.x, H = H2 / 2;
    if (b >= B) return;
    if (j < glue::kObsDim) s_x[j] = obs[(size_t)b * glue::kObsDim + j];
    if (j < H) {
        float z[glue::kMaxAction];
        if (sde_noise) {
            for (int a = 0; a < A; ++a) z[a] = sde_noise[((size_t)b * H + j) * A + a];
        } else {
            const long long e = glue::sde_draw_epoch(*sde_epoch, sde_step ? *sde_step : 0, sde_sample_freq);
            for (int a = 0; a < A; ++a) z[a] = glue::sde_noise(noise_seed, env_offset + b, e, j * A + a);
        }
        glue::sde_row(W.std, A, j, z, s_e + j * A);
    }
    __syncthreads();
    if (j < H2) s_h1[j] = glue::layer1_unit(W, H2, s_x, j);
    __syncthreads();
    if (j < H2) s_h2[j] = glue::layer2_unit(W, H2, s_h1, j);
    __syncthreads();
    if (j <= A) s_head[j] = glue::head_unit(W, H2, A, s_h2, j);
    if (j >= 64 && j < 64 + 2 * A) s_sum[j - 64] = glue::sde_sum(W.std, H, A, s_h2, s_e, j - 64);
    __syncthreads();
    if (j == 0)
        glue::finish_action_sde(A, s_head, s_sum, version_v1, clip, nullptr, actions + (size_t)b * A, values + b, log_probs + b,
                                mpc_weights ? mpc_weights + (size_t)b * 3 : nullptr, mpc_ref_speed ? mpc_ref_speed + b : nullptr);
}

// the end-to-end baseline's step (agents/ppo_agent.py: the policy's two outputs are the controls, no MPC): the network of
// mpc_policy_act_kernel at A = 2 for a tile of E consecutive environments per workgroup.  Without a solve behind it the forward
// IS the step, and at one workgroup per environment every workgroup reads all weights again; here thread j holds unit j of
// all E environments, loads each weight once and feeds E running sums from LDS (inputs interleaved [i][E], read as a
// broadcast).  Each sum is accumulated as mpc_policy_act_kernel accumulates it, so the outputs agree bit for bit.
// LDS (dynamic): x [80][E] | h1 [2H][E] | h2 [2H][E] | heads [3][E].  An environment the last tile lacks reads environment
// B - 1 and writes nothing; every thread reaches every barrier.
template <int E>
__global__ __launch_bounds__(mpc::glue::kMaxHidden2) void mpc_policy_control_kernel(
    int B, int H2, const float *__restrict__ obs, mpc::glue::PolicyWeights W, float *noise, unsigned long long noise_seed,
    int env_offset, const long long *__restrict__ noise_step, float *__restrict__ actions, float *__restrict__ values,
    float *__restrict__ log_probs, double *__restrict__ control) {
    namespace glue = mpc::glue;
    constexpr int O = glue::kObsDim;
    extern __shared__ float s_tile[];
    float *s_x = s_tile, *s_h1 = s_x + O * E, *s_h2 = s_h1 + H2 * E, *s_head = s_h2 + H2 * E;
    const int b0 = blockIdx.x * E, j = threadIdx.x;
    glue::stage_tile<E>(obs, B, b0, j, (int)blockDim.x, s_x);
    // thread e < E finishes environment b0 + e; its noise stays in registers: drawn here (and left in `noise`) or handed in
    const bool mine = j < E && b0 + j < B;
    float z[2] = {0.0f, 0.0f};
    if (mine) {
        const int b = b0 + j;
        if (noise_step) {
            for (int a = 0; a < 2; ++a) z[a] = noise[(size_t)b * 2 + a] = glue::policy_noise(noise_seed, env_offset + b, *noise_step, a);
        } else {
            for (int a = 0; a < 2; ++a) z[a] = noise[(size_t)b * 2 + a];
        }
    }
    __syncthreads();
    if (j < H2) glue::layer1_tile<E>(W, H2, s_x, j, s_h1 + j * E);
    __syncthreads();
    if (j < H2) glue::layer2_tile<E>(W, H2, s_h1, j, s_h2 + j * E);
    __syncthreads();
    if (j <= 2) glue::head_tile<E>(W, H2, 2, s_h2, j, s_head + j * E);
    __syncthreads();
    if (mine) {
        const int b = b0 + j;
        float out4[4];
        double u[2];
        glue::finish_control<E>(W, s_head, j, z, out4, u);
        actions[(size_t)b * 2 + 0] = out4[0];
        actions[(size_t)b * 2 + 1] = out4[1];
        values[b] = out4[2];
        log_probs[b] = out4[3];
        control[(size_t)b * 2 + 0] = u[0];
        control[(size_t)b * 2 + 1] = u[1];
    }
}

template <int E>
static void launch_policy_control(hipStream_t stream, int B, int H2, const float *obs, const mpc::glue::PolicyWeights &W, float *noise,
                                  uint64_t noise_seed, int env_offset, const int64_t *noise_step, float *actions, float *values,
                                  float *log_probs, double *control) {
    const int threads = (H2 + 63) / 64 * 64;
    const size_t lds = (size_t)(mpc::glue::kObsDim + 2 * H2 + 3) * E * sizeof(float);
    hipLaunchKernelGGL(mpc_policy_control_kernel<E>, dim3((unsigned)((B + E - 1) / E)), dim3((unsigned)threads), lds, stream, B, H2, obs,
                       W, noise, (unsigned long long)noise_seed, env_offset, reinterpret_cast<const long long *>(noise_step), actions,
                       values, log_probs, control);
}

__global__ __launch_bounds__(128) void mpc_rollout_record_kernel(mpc::glue::RecordArgs R, int T, long long *__restrict__ pos_dev,
                                                                 int32_t *__restrict__ ticket,
                                                                 unsigned long long *__restrict__ counts,
                                                                 long long *__restrict__ step_counter) {
    const int b = blockIdx.x, j = threadIdx.x;
    if (b >= R.B) return;
    const long long pos = *pos_dev;
    // a step past the end of the buffer writes no row (the torch path raises there): refused and counted
    const bool inside = pos >= 0 && pos < (long long)T;
    const int bits = mpc::glue::record_thread(R, pos, b, j, inside);
    if (!inside && b == 0 && j == 0) atomicAdd(counts + 4, 1ull);
    if (bits & 1) atomicAdd(counts + 0, 1ull);
    if (bits & 2) atomicAdd(counts + 1, 1ull);
    if (bits & 4) atomicAdd(counts + 2, 1ull);
    if (bits & 8) atomicAdd(counts + 3, 1ull);
    // the last workgroup to finish advances the buffer position (every workgroup has read it by then)
    __syncthreads();
    if (j == 0) {
        __threadfence();
        if (atomicAdd(ticket, 1) == R.B - 1) {
            *ticket = 0;
            *pos_dev = pos + 1;
            if (step_counter) *step_counter += 1;      // policy steps taken so far: keys the next step's noise
        }
    }
}

// per-episode accounting of a closed-loop evaluation (mpc_episode_stats.hpp): one thread per environment; each record slot
// has one writer, `recorded` counts the finished episodes that wrote one (one atomic add each)
__global__ __launch_bounds__(256) void mpc_episode_stats_kernel(mpc::stats::Accounts acc, mpc::stats::StepInputs in, int reset,
                                                                unsigned long long *__restrict__ recorded,
                                                                long long *__restrict__ step_counter) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= acc.B) return;
    if (mpc::stats::episode_update(acc, in, b, reset != 0)) atomicAdd(recorded, 1ull);
    if (b == 0) {
        if (reset) *recorded = 0ull;                      // a reset launch writes no record: no add races with this
        else if (step_counter) *step_counter += 1;        // policy steps taken so far: keys mpc_policy_act's next noise
    }
}

// safety and comfort metrics of a closed-loop evaluation (mpc_drive_metrics.hpp): sixteen lanes per environment, four
// environments per wave, the mapping of the two environment kernels.  Lane l of a group owns observation row l + 1 (R <= 17)
// and the route segments l, l + 16, ...; four group minima by shuffles, then lane 0 does the sequential update and the one
// record write.  Every shuffle sits in wave-uniform control flow: a lane without a row, and a group past the end (it reads
// the last environment), carry +inf and write nothing.  No LDS, no atomics.
__global__ __launch_bounds__(64) void mpc_drive_metrics_kernel(mpc::drive::Accounts acc, mpc::drive::StepInputs in, int reset) {
    namespace drive = mpc::drive;
    const int l = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int b_ = blockIdx.x * 4 + g;
    const bool live = b_ < acc.B;
    const int b = live ? b_ : acc.B - 1;
    drive::Gaps m{drive::kInf, drive::kInf, drive::kInf, drive::kInf};
    if (!reset) {
        const float *ego = in.terminal_obs + (size_t)b * in.R * drive::kCols;
        if (l < in.R - 1) drive::fold_row(ego, ego + (l + 1) * drive::kCols, m);
        const int nseg = in.M > 1 ? in.M - 1 : 1;
        for (int i = l; i < nseg; i += 16) drive::fold_segment(ego, in.ref_xy, in.M, i, m);
    }
    for (int off = 8; off >= 1; off >>= 1) {
        m.centre = drive::min2(m.centre, __shfl_xor(m.centre, off, 16));
        m.box = drive::min2(m.box, __shfl_xor(m.box, off, 16));
        m.ttc = drive::min2(m.ttc, __shfl_xor(m.ttc, off, 16));
        m.xte2 = drive::min2(m.xte2, __shfl_xor(m.xte2, off, 16));
    }
    if (live && l == 0) drive::episode_update(acc, in, b, reset != 0, m);
}

// interaction metrics of a closed-loop evaluation (mpc_interaction.hpp): sixteen lanes per environment, four environments per
// wave, the mapping of mpc_synth_env_idm_kernel.  Lane j of a group is vehicle j: its two leaders (with and without the ego)
// from a loop over k < K of group shuffles, both walks of the circle rule by shuffles of who[], its decision; the group's
// counts are slices of two ballots, the largest deceleration a shuffle maximum, the imposed accelerations summed in index
// order from shuffles.  The route is staged in LDS as in the environment kernels; its segments are strided over the lanes and
// the (distance, index) minimum taken by shuffles (first of the nearest).  Lane r < 12 keeps the ego's pass time of route r,
// lane j < 9 its slot's pass time and carries, lane 0 does the sequential part and writes the counters and the record.
// Every shuffle, ballot and barrier sits in wave-uniform control flow: a lane without a vehicle decides nothing, a group
// past the end reads the last environment; only stores are predicated.  The running state is read by every lane of a group
// before a lane of the same wave writes it.  No atomics.
__global__ __launch_bounds__(64) void mpc_interaction_kernel(mpc::interact::Accounts acc, mpc::interact::StepInputs in, int reset) {
    namespace ia = mpc::interact;
    namespace env = mpc::env;
    namespace drive = mpc::drive;
    __shared__ double s_ref[2 * env::kMaxRoutePoints];
    env::stage_route(s_ref, in.ref_xy, in.M);
    const int q = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int b_ = blockIdx.x * 4 + g;
    const bool live = b_ < acc.B;
    const int b = live ? b_ : acc.B - 1;
    const size_t B = (size_t)acc.B;
    const int K = in.K, Ks = K > 0 ? K : 1;
    const bool mine = q < K;
    const size_t vo = (size_t)b * Ks + (mine ? q : 0);
    int32_t *si = acc.state_i32 + b;
    double *sf = acc.state_f64 + b;
    const bool fresh = reset || in.done[b] != 0;
    const int n = fresh ? 0 : si[ia::kSteps * B];
    const env::Ego e = env::load_ego(in.ego + (size_t)b * 4);
    // ---- (a) vehicle q
    double px = 0.0, py = 0.0, ps = 0.0, ph = 0.0, prog = 0.0, target = 1.0;
    int route = -1;
    bool act = false;
    if (mine) {
        px = in.opos[2 * vo]; py = in.opos[2 * vo + 1]; ps = in.ospeed[vo]; ph = in.ohead[vo];
        act = in.oactive[vo] != 0;
        route = in.oroute[vo]; prog = in.oprog[vo]; target = in.otarget[vo];
    }
    const double cj = cos(ph), sj = sin(ph);
    env::Leader lead = env::no_leader(), alt = env::no_leader();
    env::offer_leader(lead, q, px, py, ph, cj, sj, -1, e.x, e.y, e.th, e.sp);
    for (int k = 0; k < K; ++k) {
        const double kx = __shfl(px, k, 16), ky = __shfl(py, k, 16), kh = __shfl(ph, k, 16), kv = __shfl(ps, k, 16);
        const int ka = __shfl((int)act, k, 16);
        if (k != q && ka) {
            env::offer_leader(lead, q, px, py, ph, cj, sj, k, kx, ky, kh, kv);
            env::offer_leader(alt, q, px, py, ph, cj, sj, k, kx, ky, kh, kv);
        }
    }
    const int who = act ? lead.who : -2;
    int wp = who, lowest = q, ap = act ? alt.who : -2, alowest = q;
    bool closed = false, aclosed = false;
    for (int i = 0; i < K; ++i) {
        const int next = __shfl(who, wp >= 0 ? wp : 0, 16), anext = __shfl(who, ap >= 0 ? ap : 0, 16);
        env::walk_leaders(q, wp >= 0 ? next : -2, wp, lowest, closed);
        env::walk_leaders(q, ap >= 0 ? anext : -2, ap, alowest, aclosed);
    }
    if (closed && lowest == q) lead = env::no_leader();
    if (aclosed && alowest == q) alt = env::no_leader();
    ia::Decision d = ia::inactive_decision();
    if (act) d = ia::decide(ps, target, ph, lead, alt);
    const int n_yield = __popcll((__ballot(d.yields) >> (16 * g)) & 0xffffull);
    const int32_t hard_mask = (int32_t)((__ballot(d.hard) >> (16 * g)) & 0xffffull);
    double forced = d.yields ? drive::max2(0.0, -d.a_with) : 0.0;
    for (int off = 8; off >= 1; off >>= 1) forced = drive::max2(forced, __shfl_xor(forced, off, 16));
    double imposed_sum = 0.0;
    for (int k = 0; k < K; ++k) imposed_sum = imposed_sum + __shfl(d.imposed, k, 16);
    // ---- (b) the ego's arc length, the pass times, the post-encroachment times
    ia::Proj pr{ia::kInf, 0};
    const int nseg = in.M > 1 ? in.M - 1 : 1;
    for (int i = q; i < nseg; i += 16) ia::fold_proj(s_ref, in.M, i, e.x, e.y, pr);
    double near_d2 = pr.d2;
    int near_idx = pr.idx;
    for (int off = 8; off >= 1; off >>= 1) {       // the smaller distance, the lower index among equal ones
        const double od = __shfl_xor(near_d2, off, 16);
        const int oi = __shfl_xor(near_idx, off, 16);
        const bool take = od < near_d2 || (od == near_d2 && oi < near_idx);
        near_d2 = take ? od : near_d2;
        near_idx = take ? oi : near_idx;
    }
    const double sigma = ia::sigma_at(s_ref, in.M, near_idx, e.x, e.y);
    const int r = q < ia::kRoutes ? q : 0;
    bool te_fresh = false, tv_fresh = false;
    const double te = ia::ego_pass(n, in.conflict[2 * r], fresh ? ia::kUnset : sf[(ia::kTe + r) * B], sf[ia::kCarrySigma * B],
                                   sigma, te_fresh);
    const int s = q < ia::kSlots ? q : 0;
    const bool in_slot = act && q < ia::kSlots && ia::valid_route(route);
    const int sroute = in_slot ? route : -1;
    const double sprog = in_slot ? prog : 0.0;
    double tv = ia::kUnset;
    if (!fresh) tv = ia::slot_pass(n, in_slot, sroute, sprog, si[(ia::kCarryRoute + s) * B], sf[(ia::kCarryProg + s) * B],
                                   sf[(ia::kTv + s) * B], in.conflict, tv_fresh);
    const double te_r = __shfl(te, in_slot ? sroute : 0, 16);
    const int te_r_fresh = __shfl((int)te_fresh, in_slot ? sroute : 0, 16);
    ia::Pets p{0, 0, 0, ia::kInf};
    if (in_slot) ia::fold_pet(te_r, tv, te_r_fresh != 0, tv_fresh, in.dt, p);
    for (int off = 8; off >= 1; off >>= 1) {
        p.conflicts += __shfl_xor(p.conflicts, off, 16);
        p.critical += __shfl_xor(p.critical, off, 16);
        p.ego_first += __shfl_xor(p.ego_first, off, 16);
        p.min_pet = drive::min2(p.min_pet, __shfl_xor(p.min_pet, off, 16));
    }
    // ---- the sequential part (it reads the counters before it writes them), then the lanes' own fields
    if (live && q == 0) {
        bool f;
        int32_t ordinal;
        const ia::Running run = ia::open_episode(acc, in, b, reset != 0, f, ordinal);
        ia::close_state(acc, b, in.dt, run, ordinal, n_yield, forced, hard_mask, imposed_sum, p, sigma);
    }
    if (live && q < ia::kRoutes) sf[(ia::kTe + q) * B] = te;
    if (live && q < ia::kSlots) {
        sf[(ia::kTv + q) * B] = tv;
        sf[(ia::kCarryProg + q) * B] = sprog;
        si[(ia::kCarryRoute + q) * B] = sroute;
    }
}

// episode trace recorder of a closed-loop evaluation (mpc_episode_trace.hpp), launch 1 of 2 - the claim: which of the episodes
// that end on this step get which slot of the store.  ONE workgroup of sixteen waves walks the B environments in index order
// in passes of 1024: each lane asks the header's ends_selected() of its environment (the running state is the one before the
// step: the frame kernel changes it afterwards, in stream order), a wave ranks its lanes with a 64-bit ballot and a popcount
// of the bits below the lane, the waves' totals go through LDS and every lane adds up the waves before its own; the matched
// so far is carried in a register that every lane keeps alike.  Slots are therefore handed out in environment order, with no
// atomics, and the order is part of the result.  Lane 0 advances the counts after the last pass; every lane read the kept
// count before the first barrier.  A reset launch clears the counts.  Ballot and barriers sit in uniform control flow.
constexpr int kTraceClaimThreads = 1024, kTraceFrameThreads = 256;
__global__ __launch_bounds__(kTraceClaimThreads) void mpc_episode_trace_claim_kernel(mpc::trace::Recorder rec,
                                                                                      mpc::trace::StepInputs in, int reset) {
    namespace tr = mpc::trace;
    __shared__ int s_total[kTraceClaimThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (reset) {
        if (tid < tr::kCounts) rec.counts[tid] = 0;
        return;
    }
    const long long kept_before = rec.counts[tr::kKept];
    long long matched = 0;
    for (int base = 0; base < rec.B; base += kTraceClaimThreads) {
        const int b = base + tid;
        const bool sel = b < rec.B && tr::ends_selected(rec, in, b);
        const unsigned long long mask = __ballot(sel);
        const int below = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) s_total[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < kTraceClaimThreads / 64; ++w) {
            const int c = s_total[w];
            total += c;
            before += w < wave ? c : 0;
        }
        if (b < rec.B) rec.slot[b] = sel ? tr::slot_of(kept_before, matched + before + below, rec.C) : -1;
        matched += total;
        __syncthreads();                                   // the next pass overwrites s_total
    }
    if (tid == 0) tr::advance_counts(rec.counts, matched, rec.C);
}

// launch 2 of 2 - frame and commit: one workgroup per environment, FOUR waves.  The append is small (a scene is 2 R <= 34
// chunks of 16 bytes, one per lane, and lane 0 writes the scalars), so one wave would do for it; the four are there for the
// copy of an episode that ends with a slot, up to (2 W + 1) scenes of the rings to the store, as lane-strided 16-byte loads
// and stores with 256 of them in flight per pass instead of 64.  The frame appended in this launch is read back by other
// lanes during that copy: there is a WORKGROUP BARRIER between append and copy (the copy reads the rings only, one code
// path), and a second one before s_0 of the next episode overwrites ring entry 0, which the copy may have read, and before
// lane 0 writes the running state that every lane read at the start.  Both barriers sit in uniform control flow: every
// condition before them depends on the environment alone.  No atomics, no LDS.
struct TraceBarrier {
    __device__ __forceinline__ void operator()(int) const { __syncthreads(); }
};
__global__ __launch_bounds__(kTraceFrameThreads) void mpc_episode_trace_frame_kernel(mpc::trace::Recorder rec,
                                                                                      mpc::trace::StepInputs in, int reset) {
    mpc::trace::step_env(rec, in, (int)blockIdx.x, reset != 0, (int)threadIdx.x, kTraceFrameThreads, TraceBarrier{});
}

// perception model of a closed-loop evaluation (mpc_perception.hpp): sixteen lanes per environment, four environments per
// wave, the mapping of mpc_drive_metrics_kernel.  Lane l of a group owns observation row l + 1 (R <= 17): it forms the row's
// rectangle once, the lanes hand their rectangles round inside the group by shuffles (no second read of global memory), the
// static occluders are read at wave-uniform addresses, and the compaction rank of a seen row is a popcount of the group's
// slice of the ballot below the lane: no LDS, no atomics, no serial scan.  Every shuffle and ballot sits in wave-uniform
// control flow: a lane without a row counts as absent, a group past the end reads the last environment; only stores are
// predicated.  ctr[b] is read by every lane of the group before lane 0 of the same wave writes it.
__global__ __launch_bounds__(64) void mpc_perceive_kernel(mpc::sense::Params P, mpc::sense::Buffers buf, int reset) {
    namespace sense = mpc::sense;
    const int l = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int b_ = blockIdx.x * 4 + g;
    const bool live = b_ < buf.B;
    const int b = live ? b_ : buf.B - 1;
    const int R = buf.R, i = l + 1;
    const bool has = i < R;
    const float *in = buf.obs_true + (size_t)b * R * sense::kCols;
    float row[sense::kCols], ego[sense::kCols];
#pragma unroll
    for (int c = 0; c < sense::kCols; ++c) {
        ego[c] = in[c];
        row[c] = in[(has ? i : 0) * sense::kCols + c];
    }
    if (!has) row[0] = 0.0f;                                  // no row: absent
    const bool present = row[0] != 0.0f;
    const double px = ego[1], py = ego[2];
    double sx[sense::kPoints], sy[sense::kPoints];            // the centre, then the rectangle this lane also lends out
    sense::sample_points(row, sx, sy);
    unsigned hidden = 0;
    if (P.occlusion != 0) {
        for (int j = 0; j < R - 1; ++j) {
            double qx[4], qy[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                qx[k] = __shfl(sx[k + 1], j, 16);
                qy[k] = __shfl(sy[k + 1], j, 16);
            }
            const int blocks = __shfl((int)present, j, 16);
            const unsigned h = sense::hidden_points(px, py, sx, sy, qx, qy);
            hidden |= (blocks && j != l) ? h : 0u;
        }
        hidden |= sense::hidden_by_static(px, py, sx, sy, buf.occluders, buf.S);
    }
    const int64_t c = reset ? 0 : buf.ctr[b];
    const mpc::env::Rng r(P.seed ^ sense::kSalt, P.env_offset + b, c);
    const int cls = sense::classify(P, r, i, ego, row, hidden);
    const int shift = g * 16;
    const unsigned seen_mask = (unsigned)(__ballot(cls == sense::kSeen) >> shift) & 0xFFFFu;
    const unsigned present_mask = (unsigned)(__ballot(cls != sense::kAbsent) >> shift) & 0xFFFFu;
    const unsigned range_mask = (unsigned)(__ballot(cls == sense::kOutOfRange) >> shift) & 0xFFFFu;
    const unsigned occluded_mask = (unsigned)(__ballot(cls == sense::kOccluded) >> shift) & 0xFFFFu;
    const unsigned dropped_mask = (unsigned)(__ballot(cls == sense::kDropped) >> shift) & 0xFFFFu;
    const int rank = (int)__popc(seen_mask & ((1u << l) - 1u)), n_seen = (int)__popc(seen_mask);
    if (!live) return;                                        // nothing but stores below
    float *out = buf.obs_seen + (size_t)b * R * sense::kCols;
    if (cls == sense::kSeen) {
        float o[sense::kCols];
        sense::noisy_row(P, r, i, row, o);
#pragma unroll
        for (int k = 0; k < sense::kCols; ++k) out[(1 + rank) * sense::kCols + k] = o[k];
    }
    if (has && l >= n_seen) {
#pragma unroll
        for (int k = 0; k < sense::kCols; ++k) out[i * sense::kCols + k] = 0.0f;
    }
    if (has && buf.row_class) buf.row_class[(size_t)b * R + i] = (uint8_t)cls;
    if (l == 0) {
#pragma unroll
        for (int k = 0; k < sense::kCols; ++k) out[k] = ego[k];
        if (buf.row_class) buf.row_class[(size_t)b * R] = (uint8_t)sense::kSeen;
        const size_t B = (size_t)buf.B;
        const int n[sense::kCounts] = {(int)__popc(present_mask), n_seen, (int)__popc(range_mask),
                                       (int)__popc(occluded_mask), (int)__popc(dropped_mask)};
#pragma unroll
        for (int f = 0; f < sense::kCounts; ++f) buf.counts[f * B + b] = (reset ? 0 : buf.counts[f * B + b]) + n[f];
        buf.ctr[b] = c + 1;
    }
}

// tracker of a closed-loop evaluation (mpc_tracker.hpp): the mapping of mpc_perceive_kernel, sixteen lanes per environment,
// four environments per wave.  Lane l of a group is BOTH measurement row l + 1 (R <= 17) and track slot l.  The association
// is a loop over the rows (R is wave-uniform): the row's position is broadcast inside the group, every lane forms the
// distance of its slot, and the group takes the lexicographic minimum of (d, slot) by four xor-shuffles - that order is
// total, so the tree gives the serial loop's answer, ties to the lowest slot - and the winning lane marks itself claimed.  A
// slot then fetches the row it was updated or born from with one lane-indexed shuffle per column.  Birth slots come from
// popcounts of the group's slices of the ballots (free slots, then coasting ones, against the unassociated rows), the output
// rank of a slot from a count of smaller (key, slot) over sixteen broadcasts: no LDS, no atomics, no serial scan.  Every
// shuffle and ballot sits in wave-uniform control flow: a lane without a row counts as absent, a group past the end reads
// the last environment; only stores are predicated.  Each slot's state is read and written by its own lane alone; the
// counts by lane 0.
__global__ __launch_bounds__(64) void mpc_track_kernel(mpc::track::Params P, mpc::track::Buffers buf, int reset) {
    namespace track = mpc::track;
    const int l = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int b_ = blockIdx.x * 4 + g;
    const bool live = b_ < buf.B;
    const int b = live ? b_ : buf.B - 1;
    const int R = buf.R, i = l + 1;
    const bool has = i < R;
    const int shift = g * 16;
    const unsigned below = (1u << l) - 1u;
    const float *in = buf.meas + (size_t)b * R * track::kCols;
    float row[track::kCols];
#pragma unroll
    for (int c = 0; c < track::kCols; ++c) row[c] = in[(has ? i : 0) * track::kCols + c];
    const float ex = in[1], ey = in[2];
    const bool present = has && row[0] != 0.0f;              // no row: absent
    const bool clear = reset != 0 || (buf.done != nullptr && buf.done[b] != 0);
    track::Slot t = clear ? track::empty_slot() : track::load_slot(buf, b, l);          // 1
    track::predict(P, t);                                                                // 2
    bool claimed = false, associated = false;
    int source = l;                                          // the lane whose row this slot is updated or born from
    for (int j = 0; j < R - 1; ++j) {                        // 3
        const float mx = __shfl(row[1], j, 16), my = __shfl(row[2], j, 16);
        const int there = __shfl((int)present, j, 16);
        const double d = track::dist2(t, mx, my);
        const bool eligible = there != 0 && t.alive != 0 && !claimed && d <= P.gate2;
        double best_d = eligible ? d : __builtin_huge_val();                             // d is finite: inputs are
        int best = eligible ? l : track::kSlots;
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) {
            const double od = __shfl_xor(best_d, m, 16);
            const int os = __shfl_xor(best, m, 16);
            const bool take = track::before(od, os, best_d, best);
            best_d = take ? od : best_d;
            best = take ? os : best;
        }
        if (best == l) claimed = true, source = j;
        if (j == l) associated = best < track::kSlots;
    }
    const bool was_alive = t.alive != 0;
    bool expired = false;
    if (was_alive && !claimed) expired = track::coast(P, t);                             // 5 (4 follows with 6)
    const unsigned measured_mask = (unsigned)(__ballot(present) >> shift) & 0xFFFFu;
    const unsigned claimed_mask = (unsigned)(__ballot(claimed) >> shift) & 0xFFFFu;
    const unsigned expired_mask = (unsigned)(__ballot(expired) >> shift) & 0xFFFFu;
    const unsigned unassoc_mask = (unsigned)(__ballot(present && !associated) >> shift) & 0xFFFFu;
    const unsigned free_mask = (unsigned)(__ballot(t.alive == 0) >> shift) & 0xFFFFu;
    const unsigned coasting_mask = (unsigned)(__ballot(t.alive != 0 && !claimed) >> shift) & 0xFFFFu;
    const int n_unassoc = (int)__popc(unassoc_mask);
    const int candidate = t.alive == 0 ? (int)__popc(free_mask & below)                  // 6: this slot's place in the queue
                          : !claimed   ? (int)__popc(free_mask) + (int)__popc(coasting_mask & below)
                                       : track::kSlots;
    const bool birth = candidate < n_unassoc;
    const bool evicted = birth && t.alive != 0;
    if (birth) {
#pragma unroll
        for (int r = 0; r < 16; ++r)                         // the candidate-th unassociated row
            if ((unassoc_mask >> r & 1u) != 0 && (int)__popc(unassoc_mask & ((1u << r) - 1u)) == candidate) source = r;
    }
    float m[track::kCols];
#pragma unroll
    for (int c = 1; c < track::kCols; ++c) m[c] = __shfl(row[c], source, 16);
    if (claimed) track::update(P, t, m[1], m[2], m[3], m[4], m[5], m[6], m[7]);          // 4
    if (birth) t = track::born(m[1], m[2], m[3], m[4], m[5], m[6], m[7]);
    const unsigned evicted_mask = (unsigned)(__ballot(evicted) >> shift) & 0xFFFFu;
    const unsigned alive_mask = (unsigned)(__ballot(t.alive != 0) >> shift) & 0xFFFFu;
    const double key = track::order_key(t, ex, ey);                                      // 7
    int rank = 0;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const double other = __shfl(key, s, 16);
        rank += ((alive_mask >> s & 1u) != 0 && track::before(other, s, key, l)) ? 1 : 0;
    }
    const bool shown = t.alive != 0 && rank < R - 1;
    const unsigned coasted_mask = (unsigned)(__ballot(shown && t.miss > 0) >> shift) & 0xFFFFu;
    const int n_alive = (int)__popc(alive_mask);
    const int n_shown = n_alive < R - 1 ? n_alive : R - 1;
    if (!live) return;                                        // nothing but stores below
    float *out = buf.out + (size_t)b * R * track::kCols;
    uint8_t *row_slot = buf.row_slot ? buf.row_slot + (size_t)b * R : nullptr;
    uint8_t *row_miss = buf.row_miss ? buf.row_miss + (size_t)b * R : nullptr;
    if (shown) {
        float o[track::kCols];
        track::write_row(o, t);
#pragma unroll
        for (int c = 0; c < track::kCols; ++c) out[(1 + rank) * track::kCols + c] = o[c];
        if (row_slot) row_slot[1 + rank] = (uint8_t)l;
        if (row_miss) row_miss[1 + rank] = (uint8_t)t.miss;
    }
    if (has && l >= n_shown) {
#pragma unroll
        for (int c = 0; c < track::kCols; ++c) out[i * track::kCols + c] = 0.0f;
        if (row_slot) row_slot[i] = (uint8_t)track::kNoSlot;
        if (row_miss) row_miss[i] = 0;
    }
    track::store_slot(buf, b, l, t);
    if (l == 0) {
#pragma unroll
        for (int c = 0; c < track::kCols; ++c) out[c] = in[c];
        if (row_slot) row_slot[0] = (uint8_t)track::kNoSlot;
        if (row_miss) row_miss[0] = 0;
        const size_t B = (size_t)buf.B;
        const int n[track::kCounts] = {(int)__popc(measured_mask), (int)__popc(claimed_mask), n_unassoc,
                                       (int)__popc(coasted_mask), (int)__popc(expired_mask), (int)__popc(evicted_mask),
                                       n_alive - n_shown};
#pragma unroll
        for (int f = 0; f < track::kCounts; ++f) buf.counts[f * B + b] = (reset ? 0 : buf.counts[f * B + b]) + n[f];
    }
}

// actuator model of a closed-loop evaluation (mpc_actuator.hpp): one lane per (environment, channel) pair, 32 environments
// per wave - lane l is environment blockIdx.x * 32 + (l >> 1) and channel l & 1, so the loads and stores of command, applied,
// the sums and every plane of the [.][B][2] state are consecutive addresses across the wave.  The ring stays in memory: a lane
// stores its command into slot age & 7 and loads slot (age - delay) & 7, which is another slot whenever delay > 0; nothing is
// indexed in registers.  What both channels of an environment share goes through __shfl_xor(., 1) in wave-uniform control
// flow: the hold draw (the even lane's) and the OR of the nonfinite, rate_limited and saturated flags.  A lane past the end
// computes on the last environment; only its stores are predicated.  The even lane writes age, ctr and the counts.  No LDS, no
// atomics, no scratch.
__global__ __launch_bounds__(64) void mpc_actuate_kernel(mpc::act::Params P, mpc::act::Buffers buf, int reset) {
#pragma clang fp contract(off)
    namespace act = mpc::act;
    const int l = threadIdx.x, c = l & 1;
    const int b_ = blockIdx.x * 32 + (l >> 1);
    const bool live = b_ < buf.B;
    const int B = buf.B, b = live ? b_ : B - 1;
    if (reset != 0) {                                        // wave-uniform
        if (!live) return;
#pragma unroll
        for (int p = 0; p < act::kPlanes; ++p) buf.state[act::at(p, B, b, c)] = 0.0;
#pragma unroll
        for (int p = 0; p < act::kSums; ++p) buf.sums[act::at(p, B, b, c)] = 0.0;
        if (c == 0) {
            buf.age[b] = 0;
            buf.ctr[b] = 0;
#pragma unroll
            for (int f = 0; f < act::kCounts; ++f) buf.counts[(size_t)f * B + b] = 0;
        }
        return;
    }
    const bool clear = buf.done_prev != nullptr && buf.done_prev[b] != 0;                // 1
    const int age = clear ? 0 : buf.age[b];
    const int64_t ctr = buf.ctr[b];
    double u = buf.command[act::at(0, B, b, c)];                                         // 2
    const bool nonfinite = !act::is_finite(u);
    u = nonfinite ? 0.0 : u;
    const int slot = age & (act::kRing - 1);                                             // 3
    double delayed = u;
    if (P.delay > 0) {                                       // wave-uniform; the slot read is not the slot written below
        const double old = buf.state[act::at((age - P.delay) & (act::kRing - 1), B, b, c)];
        delayed = age >= P.delay ? old : 0.0;                // after a clear age is 0: nothing stale is used
    }
    const double last = clear ? 0.0 : buf.state[act::at(act::kLast, B, b, c)];
    const double prev = clear ? 0.0 : buf.state[act::at(act::kPrev, B, b, c)];
    const mpc::env::Rng r(P.seed ^ act::kSalt, P.env_offset + b, ctr);
    const int drawn = act::hold_draw(P, r) ? 1 : 0;                                      // 4
    const int partner = __shfl_xor(drawn, 1);
    const bool held = (c == 0 ? drawn : partner) != 0;       // the even lane's draw, for both channels
    delayed = held ? last : delayed;
    bool rate_limited, saturated;
    const double y = act::shape(act::channel(P, c), P.dt, r, c, delayed, prev, rate_limited, saturated);   // 5 - 8
    const int mine = (nonfinite ? 1 : 0) | (rate_limited ? 2 : 0) | (saturated ? 4 : 0);
    const int flags = mine | __shfl_xor(mine, 1);
    if (!live) return;                                       // nothing but stores below
#pragma unroll
    for (int k = 0; k < act::kRing; ++k) {
        if (k == slot)
            buf.state[act::at(k, B, b, c)] = u;
        else if (clear)
            buf.state[act::at(k, B, b, c)] = 0.0;
    }
    buf.state[act::at(act::kLast, B, b, c)] = delayed;
    buf.state[act::at(act::kPrev, B, b, c)] = y;                                         // 9
    buf.applied[act::at(0, B, b, c)] = y;
    const double dev = act::deviation(y, u);
    const double top = buf.sums[act::at(1, B, b, c)];
    buf.sums[act::at(0, B, b, c)] = buf.sums[act::at(0, B, b, c)] + dev;
    buf.sums[act::at(1, B, b, c)] = dev > top ? dev : top;
    if (c == 0) {
        buf.age[b] = age + 1;
        buf.ctr[b] = ctr + 1;
        const int n[act::kCounts] = {1, held ? 1 : 0, (flags >> 1) & 1, (flags >> 2) & 1, flags & 1};
#pragma unroll
        for (int f = 0; f < act::kCounts; ++f) buf.counts[(size_t)f * B + b] += n[f];
    }
}

// the plan against what happened (mpc_plan.hpp, mpc_plan_metrics): sixteen lanes per environment, four environments per wave,
// the mapping of mpc_drive_metrics_kernel.  The N (R - 1) pairs of a planned stage and an observed vehicle are strided over
// the sixteen lanes of a group, the group's minimum of the squared distances is taken by shuffles, then lane 0 does the
// sequential update, the ring and the one record write.  The shuffles sit in wave-uniform control flow: a group with an invalid
// plan, a lane without a pair, and a group past the end (it folds nothing) carry +inf; a group past the end writes nothing.
// No LDS, no atomics.
static_assert(mpc::plan::kMaxRows == MPC_MAX_OTHERS + 1 && mpc::plan::kMaxHorizon == MPC_MAX_HORIZON,
              "mpc_plan.hpp restates the public header's limits");
static_assert(mpc::plan::solved(0) == MPC_STATUS_IS_SOLVED(0) && mpc::plan::solved(1) == MPC_STATUS_IS_SOLVED(1) &&
                  mpc::plan::solved(4) == MPC_STATUS_IS_SOLVED(4) && mpc::plan::solved(5) == MPC_STATUS_IS_SOLVED(5) &&
                  mpc::plan::solved(7) == MPC_STATUS_IS_SOLVED(7) && mpc::plan::solved(8) == MPC_STATUS_IS_SOLVED(8),
              "mpc_plan.hpp restates MPC_STATUS_IS_SOLVED");
__global__ __launch_bounds__(64) void mpc_plan_metrics_kernel(mpc::plan::Accounts acc, mpc::plan::StepInputs in, int reset) {
    namespace plan = mpc::plan;
    const int l = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int b_ = blockIdx.x * 4 + g;
    const bool live = b_ < acc.B;
    const int b = live ? b_ : acc.B - 1;
    double d2 = plan::kInf;
    if (!reset && live) d2 = plan::fold_pairs(in, b, l, 16);
    for (int off = 8; off >= 1; off >>= 1) d2 = plan::min2(d2, __shfl_xor(d2, off, 16));
    if (live && l == 0) plan::episode_update(acc, in, b, reset != 0, d2);
}

// the plan planes of the kept episodes (mpc_plan.hpp, mpc_plan_trace): one workgroup of four waves per environment, the shape
// of mpc_episode_trace_frame_kernel, whose slot [B] it reads.  The append is (N + 1) 4 + 2 N doubles, one per lane; the copy of
// an episode that ends with a slot is lane-strided and coalesced, 256 loads in flight per pass.  ONE workgroup barrier between
// append and copy, in uniform control flow (the conditions before it depend on the environment alone): the copy reads what
// other lanes appended, and lane 0 writes the running state only after every lane has read it.  No atomics, no LDS.
__global__ __launch_bounds__(kTraceFrameThreads) void mpc_plan_trace_kernel(mpc::plan::TraceStore store,
                                                                             mpc::plan::TraceInputs in, int reset) {
    mpc::plan::trace_env(store, in, (int)blockIdx.x, reset != 0, (int)threadIdx.x, kTraceFrameThreads, TraceBarrier{});
}

// delay compensation of a closed-loop evaluation (mpc_compensate.hpp): the mapping of mpc_track_kernel, sixteen lanes per
// environment, four environments per wave, lane l row l + 1 of the observation (R <= 17).  The ego's part - push, score and the
// rollout through the commands in flight - is computed by every lane of the group (the environment kernels' convention), so
// nothing is broadcast; lane 0 alone writes the state, row 0 and pred.  The rings stay in memory and are indexed by address:
// every load of comp::predict_ego comes before its stores, and the command just pushed is used from its register.  A present
// row's place is the count of rows with a smaller (key, row) over fifteen 16-wide shuffles (an absent row's key is +inf: a
// present row's is finite), which is the stable sort; an absent row takes a zero row behind them, found from the group's
// slice of one ballot.  Every shuffle and the ballot sit in wave-uniform control flow (P.steps and R are launch arguments): a
// lane without a row counts as absent, a group past the end computes on the last environment; only stores are predicated.  No
// LDS, no atomics, no scratch.
// TWO BUILDS on a template constant: <false> is mpc_compensate's, the latency the constant 0; <true> is mpc_compensate_stale's,
// for a scene that is P.latency steps old.  There the rollout's trip count, steps + min(latency, age), differs between the four
// environments of a wave, so nothing inside comp::predict_ego may shuffle - and nothing does: every shuffle and the ballot
// come after it, where control flow is uniform again (P.steps + P.latency is a launch argument too).  A run-time flag instead
// of the constant would be one kernel less and a different register allocation for the latency-0 path.
template <bool kStale>
__global__ __launch_bounds__(64) void mpc_compensate_kernel(mpc::comp::Params P, mpc::comp::Buffers buf, int reset) {
#pragma clang fp contract(off)
    namespace comp = mpc::comp;
    const int l = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int b_ = blockIdx.x * 4 + g;
    const bool live = b_ < buf.B;
    const int b = live ? b_ : buf.B - 1;
    const int R = buf.R, i = l + 1;
    const bool has = i < R;
    const float *in = buf.obs + (size_t)b * R * comp::kCols;
    float row[comp::kCols];
#pragma unroll
    for (int c = 0; c < comp::kCols; ++c) row[c] = in[(has ? i : 0) * comp::kCols + c];
    int ahead;
    const mpc::env::Ego e = comp::predict_ego<kStale>(P, buf, b, reset != 0, live && l == 0, ahead);    // 1 - 4
    int back = P.steps;
    if constexpr (kStale) back = P.steps + P.latency;
    float *out = buf.out + (size_t)b * R * comp::kCols;
    if (back == 0) {                                         // 8, wave-uniform: every row in place
        if (!live) return;
        if (has) {
#pragma unroll
            for (int c = 0; c < comp::kCols; ++c) out[i * comp::kCols + c] = row[c];
        }
        if (l == 0) {
#pragma unroll
            for (int c = 0; c < comp::kCols; ++c) out[c] = in[c];
        }
        return;
    }
    float ego[comp::kCols];
    comp::ego_row(e, ego);                                                               // 5
    const double h = (double)ahead * P.dt;
    const bool present = has && row[0] != 0.0f;              // no row: absent
    const float nx = comp::advance(row[1], row[3], h), ny = comp::advance(row[2], row[4], h);        // 6
    const double key = present ? comp::order_key(nx, ny, ego[1], ego[2]) : __builtin_huge_val();     // 7
    int rank = 0;
#pragma unroll
    for (int s = 1; s < 16; ++s) {
        const int o = (l + s) & 15;
        const double other = __shfl(key, o, 16);
        rank += comp::before(other, o, key, l) ? 1 : 0;
    }
    const unsigned present_mask = (unsigned)(__ballot(present) >> (g * 16)) & 0xFFFFu;
    const int zero_row = 1 + (int)__popc(present_mask) + (int)__popc(~present_mask & ((1u << l) - 1u));
    if (!live) return;                                        // nothing but stores below
    if (present) {
        float *o = out + (1 + rank) * comp::kCols;
        o[0] = 1.0f, o[1] = nx, o[2] = ny;
#pragma unroll
        for (int c = 3; c < comp::kCols; ++c) o[c] = row[c];
    } else if (has) {
#pragma unroll
        for (int c = 0; c < comp::kCols; ++c) out[zero_row * comp::kCols + c] = 0.0f;
    }
    if (l == 0) {
#pragma unroll
        for (int c = 0; c < comp::kCols; ++c) out[c] = ego[c];
    }
}


// sensing latency of a closed-loop evaluation (mpc_latency.hpp): the mapping of mpc_track_kernel, sixteen lanes per
// environment, four environments per wave.  Lane l moves row l + 1 (R <= 17), lane 0 also row 0, and lane 0 alone keeps the
// state.  All lanes of an environment sit in one wave and every one of them loads age (lat::select) before lane 0 stores it.
// The frames stay in memory and are indexed by address; the slot shown is another than the slot pushed whenever it is read.  A
// group past the end works on the last environment and stores nothing.  No shuffles, no LDS, no atomics, no scratch.
__global__ __launch_bounds__(64) void mpc_delay_scene_kernel(mpc::lat::Buffers buf, int steps, int reset) {
    namespace lat = mpc::lat;
    const int l = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int b_ = blockIdx.x * 4 + g;
    const bool live = b_ < buf.B;
    const int b = live ? b_ : buf.B - 1;
    const int i = l + 1;
    const lat::Pick p = lat::select(buf, steps, b, reset != 0);                          // 1, 3
    if (!live) return;                                        // nothing but stores below
    float fresh[lat::kCols], shown[lat::kCols];
    if (i < buf.R) lat::move_row(buf, p, b, i, fresh, shown);                            // 2, 3
    if (l == 0) {
        lat::move_row(buf, p, b, 0, fresh, shown);
        lat::keep_state(buf, p, b, reset != 0, fresh, shown);                            // 4, 5
    }
}

// end of a rollout (mpc_rollout_glue.hpp: truncation bootstrap + GAE): one workgroup per environment; thread t computes the
// terms of step t (strided over T), thread 0 runs the reversed recurrence over the LDS copies, all threads store
__global__ __launch_bounds__(256) void mpc_rollout_finish_kernel(mpc::glue::GaeArgs g) {
    extern __shared__ float gae_lds[];           // [T] delta -> advantage, [T] coefficient
    const int b = blockIdx.x;
    float *delta = gae_lds, *coef = gae_lds + g.T;
    for (int t = threadIdx.x; t < g.T; t += blockDim.x) mpc::glue::gae_terms(g, b, t, delta + t, coef + t);
    __syncthreads();
    if (threadIdx.x == 0) {
        float gae = 0.0f;
        for (int t = g.T - 1; t >= 0; --t) {
            gae = mpc::glue::gae_step(delta[t], coef[t], gae);
            delta[t] = gae;
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < g.T; t += blockDim.x) mpc::glue::gae_store(g, b, t, delta[t]);
}

// device memory the handle owns: released when the handle is deleted (mpc_destroy), so a buffer added to mpc_handle is
// freed without a second edit
template <class T>
struct DevPtr {
    T *p = nullptr;
    DevPtr() = default;
    DevPtr(const DevPtr &) = delete;
    DevPtr &operator=(const DevPtr &) = delete;
    ~DevPtr() { if (p) (void)hipFree(p); }
    operator T *() const { return p; }
};

// ... one that is grown on demand and reused across calls (grow() below)
struct GrowBuf : DevPtr<void> {
    size_t bytes = 0;
};

}  // namespace

struct mpc_handle {
    mpc_config cfg;
    int device = 0;
    DevPtr<double> d_ref;  // [M][REF_COLS] x y heading sin cos, followed by the speed column [M]
    int M = 0;
    int num_cu = 256;
    size_t lds_per_cu = 160 * 1024;
    GrowBuf stage;  // staging of host-pointer calls (Staging below)
    // observation-level path (mpc_predict_batch): per-environment detector state and the problem data the
    // preamble kernel writes for the solve kernel
    DevPtr<mpc::pre::EnvState> d_env;
    GrowBuf ids;   // scratch of mpc_reset_env_state (int32)
    int env_cap = 0;
    DevPtr<double> d_warm;         // [env_cap][N][2] last control sequence per environment (MPC_FLAG_WARM_START)
    DevPtr<uint8_t> d_warm_valid;  // [env_cap] 1 = d_warm holds a solution of the current episode
    DevPtr<double> d_ltv_u;        // [env_cap][N][2] stored profile (oa, od) of the iterative-linear agent per environment
    GrowBuf pre;
    int pre_B = 0, pre_V = 0;   // shape of the last preamble output (for mpc_get_last_inputs)
    double *p_state = nullptr, *p_vref = nullptr, *p_others = nullptr;   // segments of `pre`
    int32_t *p_ego = nullptr, *p_nveh = nullptr;
    uint8_t *p_coll = nullptr;
    // diagnostics (mpc_set_diagnostics): polylines of the last preamble launch
    bool diag = false;
    GrowBuf diag_buf;
    int diag_B = 0, diag_V = 0;
    double *g_ego = nullptr;   // segments of `diag_buf`
    int32_t *g_len = nullptr;
    float *g_agents = nullptr;
    // launch order of a batch (mpc_order_kernel): allocated once, by mpc_create
    DevPtr<int32_t> d_order;
    int order_cap = 0;
};

namespace {

size_t round_up(size_t v, size_t m) { return (v + m - 1) / m * m; }

// next 16-byte aligned segment of a packed device allocation: returns its offset and advances `off`
size_t carve(size_t &off, size_t bytes) {
    const size_t o = off;
    off += round_up(bytes, 16);
    return o;
}

// Refusal of anything that frees or moves device memory while `stream` is being captured: the graph keeps addresses.
// `remedy` is the call site's message (each tells the user a different way out).
int refuse_in_capture(hipStream_t stream, const char *remedy) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (stream && hipStreamIsCapturing(stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
        return fail(MPC_ERR_INVALID_ARG, remedy);
    return MPC_OK;
}

// Grow a handle-owned buffer to at least `bytes` (contents are not kept).  The old buffer may still be in use by enqueued
// (MPC_FLAG_NO_SYNC) work of any stream, and a captured graph holds its address: never inside a capture, and only once the
// device is idle.  `remedy` = nullptr: the caller is synchronous by contract (host pointers) and cannot be captured.
// On failure the buffer is left empty.
int grow(GrowBuf &b, size_t bytes, hipStream_t stream, const char *remedy) {
    if (b.bytes >= bytes) return MPC_OK;
    if (int rc = remedy ? refuse_in_capture(stream, remedy) : MPC_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    void *old = b.p;
    b.p = nullptr;
    b.bytes = 0;
    if (old) HIP_TRY(hipFree(old));
    HIP_TRY(hipMalloc(&b.p, bytes));
    b.bytes = bytes;
    return MPC_OK;
}

// Host-pointer calls: every argument is copied through ONE handle-owned device buffer on the caller's stream.  An entry
// point states each argument once - pointer, bytes, direction - gets its device view from ptr(), and ends with finish().
// With device pointers (`dev`) every method hands the caller's pointer through and nothing is copied.  Two host-pointer
// calls on one handle share the buffer; the synchronise at the end of the first is what serialises them.
class Staging {
  public:
    Staging(mpc_handle *h, hipStream_t stream, bool dev) : h_(h), stream_(stream), dev_(dev) {}
    // Each states one argument and returns its ticket for ptr().  A null `host` takes no room and stays null, or with
    // kReserve gets a segment that is not copied: the kernel has a place to write even if the caller does not want the result.
    enum IfNull { kSkip, kReserve };
    template <class T>
    struct Arg { int i; };
    template <class T>
    Arg<const T> in(const T *host, size_t bytes, IfNull n = kSkip) { return {add(const_cast<T *>(host), bytes, kIn, n)}; }
    template <class T>
    Arg<T> out(T *host, size_t bytes, IfNull n = kSkip) { return {add(host, bytes, kOut, n)}; }
    template <class T>
    Arg<T> inout(T *host, size_t bytes, IfNull n = kSkip) { return {add(host, bytes, kIn | kOut, n)}; }

    // size the buffer, enqueue the host-to-device copies; ptr() is valid from here on
    int commit() {
        if (dev_) return MPC_OK;
        if (int rc = grow(h_->stage, off_, stream_, nullptr)) return rc;
        for (int i = 0; i < n_; ++i)
            if (seg_[i].staged && (seg_[i].dir & kIn) && seg_[i].host)
                HIP_TRY(hipMemcpyAsync(device(seg_[i]), seg_[i].host, seg_[i].bytes, hipMemcpyHostToDevice, stream_));
        return MPC_OK;
    }
    // the device view of an argument: its segment, or the caller's own pointer (device pointers, null)
    template <class T>
    T *ptr(Arg<T> a) const {
        const Seg &s = seg_[a.i];
        return static_cast<T *>(s.staged ? device(s) : s.host);
    }
    // the one synchronisation rule: host pointers always, device pointers unless MPC_FLAG_NO_SYNC
    int sync(uint32_t flags) {
        if (!dev_ || !(flags & MPC_FLAG_NO_SYNC)) HIP_TRY(hipStreamSynchronize(stream_));
        return MPC_OK;
    }
    // enqueue the device-to-host copies, then sync()
    int finish(uint32_t flags) {
        for (int i = 0; i < n_; ++i)
            if (seg_[i].staged && (seg_[i].dir & kOut) && seg_[i].host)
                HIP_TRY(hipMemcpyAsync(seg_[i].host, device(seg_[i]), seg_[i].bytes, hipMemcpyDeviceToHost, stream_));
        return sync(flags);
    }

  private:
    enum { kIn = 1, kOut = 2, kMaxSeg = 12 };
    struct Seg {
        void *host;
        size_t off, bytes;
        int dir;
        bool staged;
    };
    int add(void *host, size_t bytes, int dir, IfNull n) {
        assert(n_ < kMaxSeg);
        const bool staged = !dev_ && (host || n == kReserve);
        seg_[n_] = Seg{host, staged ? carve(off_, bytes) : 0, bytes, dir, staged};
        return n_++;
    }
    void *device(const Seg &s) const { return static_cast<char *>(h_->stage.p) + s.off; }

    mpc_handle *h_;
    hipStream_t stream_;
    bool dev_;
    Seg seg_[kMaxSeg];
    int n_ = 0;
    size_t off_ = 0;
};

// The dynamic-LDS limit of a kernel is raised once per (kernel, device), to the largest size asked for so far: the
// attribute call is not a stream operation and must stay out of a stream capture (hipGraph) of the launch, so only the
// first use of a size has to happen outside one.  One cache per kernel; zero-initialised (static); concurrent callers at
// worst both set the attribute.
using LdsLimits = std::atomic<size_t>[kMaxDevices];
int raise_lds_limit(const void *kernel, int device, size_t bytes, LdsLimits &cache) {
    if (device < kMaxDevices && cache[device].load(std::memory_order_acquire) >= bytes) return MPC_OK;
    HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    if (device < kMaxDevices) {
        size_t cur = cache[device].load(std::memory_order_relaxed);
        while (cur < bytes && !cache[device].compare_exchange_weak(cur, bytes, std::memory_order_release)) {}
    }
    return MPC_OK;
}

template <bool CC, int NC, int OCC, int RELAX>
int launch_wave(const mpc_handle *h, const mpc::SolveParams &P, int B, int V, hipStream_t stream,
                const double *d_state, const int32_t *d_ego, const double *d_vref, const double *d_weights,
                const uint8_t *d_coll, const double *d_others, const int32_t *d_nveh, const double *d_uinit, int u_shift,
                uint8_t *d_uvalid, double *d_u0, double *d_U, double *d_X, int32_t *d_status, int32_t *d_iters,
                const int32_t *d_order) {
    auto kern = mpc_solve_wave_kernel<CC, NC, OCC, RELAX>;
    const size_t lds = (size_t)mpc::wave::lds_doubles(CC, P.N, P.V, wave_spare_lds(NC, OCC, RELAX)) * sizeof(double);
    static LdsLimits lds_set;
    if (int rc = raise_lds_limit(reinterpret_cast<const void *>(kern), h->device, lds, lds_set)) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(kBlock), lds, stream, P, B, h->d_ref, h->M, d_state, d_ego,
                       d_vref, d_weights, d_coll, d_others, V, d_nveh, h->cfg.w_collision, d_uinit, u_shift, d_uvalid,
                       d_u0, d_U, d_X, d_status, d_iters, d_order);
    HIP_TRY(hipGetLastError());
    return MPC_OK;
}

// Launch of the solve kernel for B instances whose data already sits in device memory (shared by mpc_solve_batch and
// mpc_predict_batch).  d_nveh: vehicles present per instance or nullptr (= V for all).
mpc::SolveParams solve_params(const mpc_handle *h, int Vuse) {
    mpc::SolveParams P;
    P.N = h->cfg.horizon;
    P.V = Vuse;
    P.max_iter = h->cfg.max_iter;
    P.dt = h->cfg.dt;
    P.tol = h->cfg.tol;
    P.mu_init = 0.1;
    P.w_distance = h->cfg.w_distance;
    P.stall_window = h->cfg.stall_window;
    P.strict_kink = 0;
    return P;
}

int dispatch_solve(const mpc_handle *h, int B, bool cc, int V, uint32_t flags, hipStream_t stream, const double *d_state,
                   const int32_t *d_ego, const double *d_vref, const double *d_weights, const uint8_t *d_coll,
                   const double *d_others, const int32_t *d_nveh, const double *d_uinit, int u_shift, uint8_t *d_uvalid,
                   double *d_u0, double *d_U, double *d_X, int32_t *d_status, int32_t *d_iters) {
    const int N = h->cfg.horizon;
    const int Vuse = cc ? V : 0;
    mpc::SolveParams P = solve_params(h, Vuse);
    P.strict_kink = (flags & MPC_FLAG_STRICT_DISCONTINUITY) ? 1 : 0;
    const bool throughput = (flags & MPC_FLAG_THROUGHPUT) != 0;

    static_assert(MPC_MAX_HORIZON <= mpc::wave::kMaxHorizon, "lane k = stage k needs the horizon to fit a wave");
    const bool lat = !throughput && B <= kLatDepth * (4 * h->num_cu);      // which build: see kWaveOccLat above
    const bool spare = lat && (N == 20 || N == 16);                        // (wave_spare_lds of the build launched below)
    const size_t wlds = (size_t)mpc::wave::lds_doubles(cc, N, Vuse, spare) * sizeof(double);
    if (wlds > h->lds_per_cu)
        return fail(MPC_ERR_INVALID_ARG, "horizon / vehicle count too large for the LDS workspace of one instance");
    int rc;
#define MPC_LAUNCH_W(CCV, NCV, OCCV, RLX)                                                                              \
    rc = launch_wave<CCV, NCV, OCCV, RLX>(h, P, (int)B, (int)V, stream, d_state, d_ego, d_vref, d_weights, d_coll, \
                                          d_others, d_nveh, d_uinit, u_shift, d_uvalid, d_u0, d_U, d_X, d_status, d_iters, d_order)
    // which build: by how deep the batch fills the SIMDs (see kWaveOccLat above)
    const int simds = 4 * h->num_cu;
    // launch order (mpc_order_kernel): pays as soon as waves share a SIMD.  Not with MPC_FLAG_THROUGHPUT: batches in flight on
    // several streams may share this handle, and the order buffer is the handle's.  Until round 5 only up to 8 waves per SIMD
    // ("beyond that the order changed nothing" - measured with round 4's kernel); a bulk launch ends with whatever started
    // last running alone, up to 100 iterations x 28 us = 13 % of a launch of 65 536, and the tiers start 85 - 90 % of the
    // instances with >= 60 iterations in the first 40 % of the launch: 21.2 / 21.3 / 21.4 / 22.2 -> 20.3 / 19.8 / 20.6 / 22.6 ms
    // on four draws (profiles/r06_bulk_order.txt; tools/sim_schedule.py's occupancy model predicts each to 0.2 ms)
    const int32_t *d_order = nullptr;
    if (!throughput && B > simds && h->d_order && h->order_cap >= B) {
        // the seat tier in front (see mpc_order_kernel): only where the latency build (a compiled horizon, `spare`) solves this
        // one batch two waves per SIMD, with vehicles and the collision cost
        const int seats = spare && cc && d_others && Vuse > 0 ? 1 : 0;
        int32_t *d_tier = h->d_order + h->order_cap;
        if (seats) {
            hipLaunchKernelGGL(mpc_tier_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, stream, (int)B, d_coll, d_state,
                               d_others, (int)Vuse, d_nveh, d_ego, h->d_ref, h->M, N, N * h->cfg.dt, d_tier);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(mpc_order_kernel, dim3(1), dim3(1024), 0, stream, (int)B, d_coll, d_state, cc ? d_others : nullptr,
                           (int)Vuse, d_nveh, d_ego, h->d_ref, h->M, N, seats, h->d_order, d_tier);
        HIP_TRY(hipGetLastError());
        d_order = h->d_order;
    }
#define MPC_LAUNCH_N(CCV, NCV)                                          \
    if (lat) MPC_LAUNCH_W(CCV, NCV, kWaveOccLat, kRelaxLat);            \
    else MPC_LAUNCH_W(CCV, NCV, kWaveOcc, 0)
    if (cc) {
        if (N == 20) { MPC_LAUNCH_N(true, 20); }       /* BASELINE horizon */
        else if (N == 16) { MPC_LAUNCH_N(true, 16); }  /* reference cfg.yaml default */
        else MPC_LAUNCH_W(true, 0, kWaveOccGenericCC, 0);
    } else {
        if (N == 20) { MPC_LAUNCH_N(false, 20); }
        else if (N == 16) { MPC_LAUNCH_N(false, 16); }
        else MPC_LAUNCH_W(false, 0, kWaveOccGeneric, 0);
    }
#undef MPC_LAUNCH_N
#undef MPC_LAUNCH_W
    if (rc == MPC_OK && d_X && d_U && d_status) {
        hipLaunchKernelGGL(mpc_infeasible_start_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, (int)B, N,
                           h->cfg.dt, d_state, d_U, d_status, d_X);
        HIP_TRY(hipGetLastError());
    }
    return rc;
}

}  // namespace

extern "C" {

int mpc_version(void) { return MPC_ABI_VERSION; }

const char *mpc_last_error(void) { return g_last_error.c_str(); }

void mpc_default_config(mpc_config *cfg) {
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (int32_t)sizeof(mpc_config);
    cfg->horizon = 20;
    cfg->dt = 0.1;
    cfg->max_iter = 100;
    cfg->device = 0;
    cfg->tol = 1e-8;
    cfg->w_distance = 10.0;
    cfg->w_collision = 1.0;
    cfg->ltv_passes = 1;
}

int mpc_default_config_sized(mpc_config *cfg, int32_t size) {
    if (!cfg) return fail(MPC_ERR_INVALID_ARG, "mpc_default_config_sized: null argument");
    if (size != (int32_t)sizeof(mpc_config))
        return fail(MPC_ERR_INVALID_ARG, "mpc_default_config_sized: the caller's mpc_config has " + std::to_string(size) +
                                         " bytes, this library's has " + std::to_string(sizeof(mpc_config)));
    mpc_default_config(cfg);
    return MPC_OK;
}

int mpc_create(const mpc_config *cfg, mpc_handle **out) {
    if (!cfg || !out) return fail(MPC_ERR_INVALID_ARG, "mpc_create: null argument");
    if (cfg->struct_size != (int32_t)sizeof(mpc_config))
        return fail(MPC_ERR_INVALID_ARG, "mpc_create: mpc_config.struct_size mismatch");
    if (cfg->horizon < 1 || cfg->horizon > MPC_MAX_HORIZON)
        return fail(MPC_ERR_INVALID_ARG, "mpc_create: horizon out of range");
    if (!(cfg->dt > 0.0) || cfg->max_iter < 0 || !(cfg->tol > 0.0))
        return fail(MPC_ERR_INVALID_ARG, "mpc_create: dt, max_iter and tol must be positive");
    if (cfg->ltv_passes < 1 || cfg->ltv_passes > 16 || cfg->stall_window < 0)
        return fail(MPC_ERR_INVALID_ARG, "mpc_create: ltv_passes must be 1..16 and stall_window non-negative");
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(MPC_ERR_NO_DEVICE,
                    std::string("mpc_create: no HIP device available (the engine has no CPU path): ") +
                        (e != hipSuccess ? hipGetErrorString(e) : "device count is 0"));
    if (cfg->device < 0 || cfg->device >= count) return fail(MPC_ERR_INVALID_ARG, "mpc_create: bad device ordinal");
    HIP_TRY(hipSetDevice(cfg->device));
    mpc_handle *h = new (std::nothrow) mpc_handle();
    if (!h) return fail(MPC_ERR_HIP, "mpc_create: out of host memory");
    h->cfg = *cfg;
    h->device = cfg->device;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess) {
            if (prop.multiProcessorCount > 0) h->num_cu = prop.multiProcessorCount;
            if (prop.maxSharedMemoryPerMultiProcessor > 0) h->lds_per_cu = prop.maxSharedMemoryPerMultiProcessor;
        }
    }
    {
        // the buffer of the launch order is allocated ONCE, here, for the largest batch that is ever ordered (64 waves per SIMD:
        // 512 KB on an MI355X) and never moves: a captured hipGraph keeps its address in two kernels (ADVICE r4 - until round 4
        // it was grown on demand, and a later, larger call on the same handle would have left such a graph replaying against
        // freed memory)
        const int cap = 64 * 4 * h->num_cu;       // dispatch_solve orders batches of up to 64 waves per SIMD (65 536 instances)
        if (hipMalloc(reinterpret_cast<void **>(&h->d_order.p), (size_t)cap * 2 * sizeof(int32_t)) == hipSuccess)
            h->order_cap = cap;
        else
            h->d_order.p = nullptr;               // (unordered launches are correct, only slower)
    }
    *out = h;
    g_last_error.clear();
    return MPC_OK;
}

void mpc_destroy(mpc_handle *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    delete h;      // every DevPtr / GrowBuf member frees its memory
}

int mpc_set_reference(mpc_handle *h, const double *ref, int32_t M) {
    if (!h || !ref || M < 1 || M > 4096) return fail(MPC_ERR_INVALID_ARG, "mpc_set_reference: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    std::string buf((size_t)M * (mpc::REF_COLS + 1) * sizeof(double), '\0');
    double *r6 = reinterpret_cast<double *>(&buf[0]);
    for (int i = 0; i < M; ++i) {
        r6[i * mpc::REF_COLS + mpc::R_X] = ref[i * 4 + 0];
        r6[i * mpc::REF_COLS + mpc::R_Y] = ref[i * 4 + 1];
        r6[i * mpc::REF_COLS + mpc::R_H] = ref[i * 4 + 3];
        r6[i * mpc::REF_COLS + mpc::R_SIN] = sin(ref[i * 4 + 3]);
        r6[i * mpc::REF_COLS + mpc::R_COS] = cos(ref[i * 4 + 3]);
        r6[M * mpc::REF_COLS + i] = ref[i * 4 + 2];
    }
    if (h->d_ref) HIP_TRY(hipFree(h->d_ref));
    h->d_ref.p = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&h->d_ref.p), buf.size()));
    HIP_TRY(hipMemcpy(h->d_ref, r6, buf.size(), hipMemcpyHostToDevice));
    h->M = M;
    return MPC_OK;
}

int64_t mpc_workspace_bytes(const mpc_handle *h, int32_t B, int32_t V) {
    if (!h || B < 0 || V < 0 || V > MPC_MAX_OTHERS) return -1;
    // the layout every build of the solve kernel shares since round 5 (mpc_wave.hpp: lds_doubles) - what limits the residency
    // of the throughput build; the spare region of the latency builds (wave_spare_lds) is LDS that would lie idle and is not
    // counted.  The workspace is per instance, so B is checked and otherwise unused by design
    const int N = h->cfg.horizon;
    return (int64_t)mpc::wave::lds_doubles(V > 0, N, V) * (int64_t)sizeof(double);
}

int mpc_solve_batch(mpc_handle *h, int32_t B, const double *state, const int32_t *ego_index, const double *vref,
                    const double *weights, const uint8_t *is_collide, const double *others, int32_t V,
                    uint32_t flags, double *u0, double *U, double *X, int32_t *status, int32_t *iters,
                    void *stream_) {
    if (!h) return fail(MPC_ERR_INVALID_ARG, "mpc_solve_batch: null handle");
    if (B < 0 || !state || !ego_index || !weights || !is_collide || !u0)
        return fail(MPC_ERR_INVALID_ARG, "mpc_solve_batch: null required pointer or negative batch");
    if (V < 0 || V > MPC_MAX_OTHERS) return fail(MPC_ERR_INVALID_ARG, "mpc_solve_batch: V out of range");
    const bool cc = (flags & MPC_FLAG_COLLISION_COST) != 0;
    if (cc && V > 0 && !others) return fail(MPC_ERR_INVALID_ARG, "mpc_solve_batch: collision cost needs `others`");
    if (!h->d_ref) return fail(MPC_ERR_NO_REFERENCE, "mpc_solve_batch: call mpc_set_reference first");
    if (B == 0) return MPC_OK;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int N = h->cfg.horizon;
    const size_t N1 = (size_t)N + 1;

    const bool dev = (flags & MPC_FLAG_DEVICE_PTRS) != 0, warm = (flags & MPC_FLAG_WARM_START) != 0;
    if (warm && !U) return fail(MPC_ERR_INVALID_ARG, "mpc_solve_batch: MPC_FLAG_WARM_START needs U (initial controls in, solution out)");

    Staging st(h, stream, dev);
    const auto s_state = st.in(state, (size_t)B * 4 * 8);
    const auto s_ego = st.in(ego_index, (size_t)B * 4);
    const auto s_w = st.in(weights, (size_t)B * 3 * 8);
    const auto s_c = st.in(is_collide, (size_t)B);
    const auto s_vref = st.in(vref, (size_t)B * N1 * 8);                                     // optional
    const auto s_oth = st.in(cc && V > 0 ? others : nullptr, (size_t)B * V * 4 * 8);
    const auto s_u0 = st.out(u0, (size_t)B * 2 * 8);
    const auto s_U = warm ? st.inout(U, (size_t)B * N * 2 * 8) : st.out(U, (size_t)B * N * 2 * 8);   // optional unless warm
    const auto s_X = st.out(X, (size_t)B * N1 * 4 * 8);                                      // optional
    const auto s_st = st.out(status, (size_t)B * 4, Staging::kReserve);
    const auto s_it = st.out(iters, (size_t)B * 4, Staging::kReserve);
    if (int rc = st.commit()) return rc;

    double *d_U = st.ptr(s_U);
    if (int rc = dispatch_solve(h, B, cc, V, flags, stream, st.ptr(s_state), st.ptr(s_ego), st.ptr(s_vref), st.ptr(s_w),
                                st.ptr(s_c), st.ptr(s_oth), nullptr, warm ? d_U : nullptr, 0, nullptr, st.ptr(s_u0), d_U,
                                st.ptr(s_X), st.ptr(s_st), st.ptr(s_it)))
        return rc;
    return st.finish(flags);
}

// grow the per-environment state array to at least B records (new records start as fresh episodes).  The old buffers
// are released, so this must not happen while earlier work may still use them: not inside a stream capture (a captured
// graph has the addresses baked in - size the handle first with mpc_reserve_envs), and only after the device is idle.
static int ensure_env(mpc_handle *h, int B, hipStream_t stream) {
    if (B <= h->env_cap) return MPC_OK;
    if (int rc = refuse_in_capture(stream, "per-environment buffers must grow, which is not possible inside a stream capture: "
                                           "call mpc_reserve_envs before capturing"))
        return rc;
    int cap = h->env_cap > 0 ? h->env_cap : 256;
    while (cap < B) cap *= 2;
    const size_t wrow = (size_t)h->cfg.horizon * 2 * sizeof(double);
    constexpr int NB = 4;
    void *nb[NB] = {nullptr, nullptr, nullptr, nullptr};
    const size_t bytes[NB] = {(size_t)cap * sizeof(mpc::pre::EnvState), (size_t)cap * wrow, (size_t)cap, (size_t)cap * wrow};
    void *old[NB] = {h->d_env.p, h->d_warm.p, h->d_warm_valid.p, h->d_ltv_u.p};
    const size_t old_bytes[NB] = {(size_t)h->env_cap * sizeof(mpc::pre::EnvState), (size_t)h->env_cap * wrow,
                                  (size_t)h->env_cap, (size_t)h->env_cap * wrow};
    hipError_t e = hipDeviceSynchronize();       // in-flight MPC_FLAG_NO_SYNC work on any stream still uses the old buffers
    for (int i = 0; i < NB && e == hipSuccess; ++i) {
        e = hipMalloc(&nb[i], bytes[i]);
        if (e == hipSuccess) e = hipMemset(nb[i], 0, bytes[i]);
        if (e == hipSuccess && old[i]) e = hipMemcpy(nb[i], old[i], old_bytes[i], hipMemcpyDeviceToDevice);
    }
    if (e != hipSuccess) {
        for (int i = 0; i < NB; ++i)
            if (nb[i]) (void)hipFree(nb[i]);
        return fail(MPC_ERR_HIP, std::string("ensure_env: ") + hipGetErrorString(e));
    }
    for (int i = 0; i < NB; ++i)
        if (old[i]) (void)hipFree(old[i]);
    h->d_env.p = static_cast<mpc::pre::EnvState *>(nb[0]);
    h->d_warm.p = static_cast<double *>(nb[1]);
    h->d_warm_valid.p = static_cast<uint8_t *>(nb[2]);
    h->d_ltv_u.p = static_cast<double *>(nb[3]);
    h->env_cap = cap;
    return MPC_OK;
}

int mpc_reserve_envs(mpc_handle *h, int32_t B) {
    if (!h || B < 0) return fail(MPC_ERR_INVALID_ARG, "mpc_reserve_envs: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    return ensure_env(h, B, nullptr);
}

int mpc_predict_batch(mpc_handle *h, int32_t B, const float *obs, int32_t vehicles_count, const double *weights,
                      const double *ref_speed, uint32_t flags, double *act, int32_t *status, int32_t *iters,
                      void *stream_) {
    return mpc_predict_batch_plan(h, B, obs, vehicles_count, weights, ref_speed, flags, act, nullptr, nullptr, status, iters,
                                  stream_);
}

// the one body of the observation-level entry; U / X: the plan the solve ended with, or NULL (the launches, and every bit of
// act / status / iters and of the handle's memory, are the same either way)
int mpc_predict_batch_plan(mpc_handle *h, int32_t B, const float *obs, int32_t vehicles_count, const double *weights,
                           const double *ref_speed, uint32_t flags, double *act, double *U, double *X, int32_t *status,
                           int32_t *iters, void *stream_) {
    if (!h) return fail(MPC_ERR_INVALID_ARG, "mpc_predict_batch: null handle");
    const bool detect_only = (flags & MPC_FLAG_DETECT_ONLY) != 0, detected = (flags & MPC_FLAG_DETECTED) != 0;
    if (detect_only && detected)
        return fail(MPC_ERR_INVALID_ARG, "mpc_predict_batch: MPC_FLAG_DETECT_ONLY and MPC_FLAG_DETECTED exclude each other");
    if (B < 0 || !obs || (!detect_only && (!weights || !act)))
        return fail(MPC_ERR_INVALID_ARG, "mpc_predict_batch: null required pointer or negative batch");
    if (vehicles_count < 1 || vehicles_count > MPC_MAX_OTHERS + 1)
        return fail(MPC_ERR_INVALID_ARG, "mpc_predict_batch: vehicles_count out of range");
    if (!h->d_ref) return fail(MPC_ERR_NO_REFERENCE, "mpc_predict_batch: call mpc_set_reference first");
    if (B == 0) return MPC_OK;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int N = h->cfg.horizon, rows = vehicles_count, V = vehicles_count - 1;
    const size_t N1 = (size_t)N + 1;
    const bool cc = (flags & MPC_FLAG_COLLISION_COST) != 0 && V > 0;
    const bool dev = (flags & MPC_FLAG_DEVICE_PTRS) != 0;
    if (int rc = ensure_env(h, B, stream)) return rc;

    // problem-data buffers written by the preamble kernel
    {
        size_t off = 0;
        auto seg = [&](size_t bytes) { return carve(off, bytes); };
        const size_t o_state = seg((size_t)B * 4 * 8), o_vref = seg((size_t)B * N1 * 8);
        const size_t o_oth = seg((size_t)B * (V > 0 ? V : 1) * 4 * 8), o_ego = seg((size_t)B * 4);
        const size_t o_nv = seg((size_t)B * 4), o_c = seg((size_t)B);
        if (int rc = grow(h->pre, off, stream, "mpc_predict_batch: the problem-data buffer must grow, which is not possible "
                                               "inside a stream capture: run one step of this size before capturing"))
            return rc;
        char *pb = static_cast<char *>(h->pre.p);
        h->p_state = reinterpret_cast<double *>(pb + o_state);
        h->p_vref = reinterpret_cast<double *>(pb + o_vref);
        h->p_others = reinterpret_cast<double *>(pb + o_oth);
        h->p_ego = reinterpret_cast<int32_t *>(pb + o_ego);
        h->p_nveh = reinterpret_cast<int32_t *>(pb + o_nv);
        h->p_coll = reinterpret_cast<uint8_t *>(pb + o_c);
        h->pre_B = B;
        h->pre_V = V;
    }

    Staging st(h, stream, dev);
    const auto s_obs = st.in(obs, (size_t)B * rows * mpc::pre::kObsCols * 4);
    const auto s_w = st.in(weights, (size_t)B * 3 * 8, Staging::kReserve);        // null with MPC_FLAG_DETECT_ONLY, like act
    const auto s_rs = st.in(ref_speed, (size_t)B * 8);                            // optional
    const auto s_act = st.out(act, (size_t)B * 2 * 8, Staging::kReserve);
    const auto s_U = st.out(detect_only ? nullptr : U, (size_t)B * N * 2 * 8);                // optional
    const auto s_X = st.out(detect_only ? nullptr : X, (size_t)B * N1 * 4 * 8);               // optional
    const auto s_st = st.out(status, (size_t)B * 4, Staging::kReserve);
    const auto s_it = st.out(iters, (size_t)B * 4, Staging::kReserve);
    if (int rc = st.commit()) return rc;

    if (h->diag) {
        size_t off = 0;
        const size_t P = mpc::pre::kPredHorizon + 1, Vs = (size_t)(V > 0 ? V : 1);
        const size_t o_ego = carve(off, (size_t)B * P * 2 * 8), o_len = carve(off, (size_t)B * 4);
        const size_t o_ag = carve(off, (size_t)B * Vs * P * 2 * 4);
        if (int rc = grow(h->diag_buf, off, stream, "mpc_predict_batch: diagnostics buffers cannot grow inside a stream capture"))
            return rc;
        char *db = static_cast<char *>(h->diag_buf.p);
        h->g_ego = reinterpret_cast<double *>(db + o_ego);
        h->g_len = reinterpret_cast<int32_t *>(db + o_len);
        h->g_agents = reinterpret_cast<float *>(db + o_ag);
        h->diag_B = B;
        h->diag_V = (int)Vs;
        HIP_TRY(hipMemsetAsync(h->diag_buf.p, 0, off, stream));
    }
    hipLaunchKernelGGL(mpc_preamble_kernel, dim3((unsigned)B), dim3(kBlock), 0, stream,
                       (int)B, st.ptr(s_obs), rows, h->d_ref, h->M, N, h->cfg.dt, st.ptr(s_rs), h->d_env,
                       h->p_state, h->p_ego, h->p_vref, h->p_coll, h->p_others, V > 0 ? V : 1, h->p_nveh, detected ? 0 : 1,
                       h->diag ? h->g_ego : nullptr, h->diag ? h->g_len : nullptr, h->diag ? h->g_agents : nullptr);
    HIP_TRY(hipGetLastError());
    const bool warm = (flags & MPC_FLAG_WARM_START) != 0;
    if (detect_only) {
        // _check_collision on its own (agents/pure_mpc.py:552-676): the records are advanced, nothing is solved and
        // nothing is copied back
        return st.sync(flags);
    }
    if (int rc = dispatch_solve(h, B, cc, V, flags, stream, h->p_state, h->p_ego, h->p_vref, st.ptr(s_w), h->p_coll,
                                h->p_others, h->p_nveh, warm ? h->d_warm : nullptr, 1, warm ? h->d_warm_valid : nullptr,
                                st.ptr(s_act), warm ? h->d_warm : st.ptr(s_U), st.ptr(s_X), st.ptr(s_st), st.ptr(s_it)))
        return rc;
    // with a warm start the kernel's U_out is the handle's memory, which stays what it is: the plan's U is a copy of it
    if (warm && st.ptr(s_U))
        HIP_TRY(hipMemcpyAsync(st.ptr(s_U), h->d_warm, (size_t)B * N * 2 * 8, hipMemcpyDeviceToDevice, stream));
    return st.finish(flags);
}

// ---- iterative-linear MPC (reference agents/pure_mpc_linear.py) ---------------------------------------------
// the two builds of mpc_ltv_kernel: waves per SIMD, and what the latency build may keep in registers (fresh / opaque the
// identity, residuals kept: mpc_ltv.hpp relax_bits).  Measured on one box (tools/gpu_ltv_ab.py, round 4): recomputed residuals
// cost a lone wave 2 %.
constexpr int kLtvOcc = 3, kLtvOccLat = 2, kLtvRelaxLat = 1 | 2 | 8;
// ... used up to FOUR waves per SIMD of batch depth, like the solve kernel's (round 6: with the 4x4 factorisation a lone wave is 15 %
// faster than in round 5 and a batch of 4096 takes 1.50 ms in this build against 1.61 ms in the other, 16 384 the same in both)
constexpr int kLtvLatDepth = 4;
static int launch_ltv(mpc_handle *h, int B, hipStream_t stream, const double *d_state, const float *d_obs, int rows,
                      double *d_U, double *d_u0, double *d_X, int32_t *d_status, int32_t *d_iters, int32_t *d_target) {
    mpc::ltv::LtvParams P;
    P.N = h->cfg.horizon;
    P.max_iter = h->cfg.max_iter;
    P.passes = h->cfg.ltv_passes;
    P.dt = h->cfg.dt;
    const size_t lds = (size_t)mpc::ltv::lds_doubles(P.N) * sizeof(double);
    // both builds on first use, whichever is launched: a later capture may launch the other
    static LdsLimits lds_set, lds_set_lat;
    const void *thr = reinterpret_cast<const void *>(mpc_ltv_kernel<kLtvOcc, 0>);
    const void *lat = reinterpret_cast<const void *>(mpc_ltv_kernel<kLtvOccLat, kLtvRelaxLat>);
    if (int rc = raise_lds_limit(thr, h->device, lds, lds_set)) return rc;
    if (int rc = raise_lds_limit(lat, h->device, lds, lds_set_lat)) return rc;
    // which build: by how deep the batch fills the SIMDs
    if (B <= kLtvLatDepth * 4 * h->num_cu)
        hipLaunchKernelGGL((mpc_ltv_kernel<kLtvOccLat, kLtvRelaxLat>), dim3((unsigned)B), dim3(kBlock), lds, stream, P, B,
                           h->d_ref, h->M, d_state, d_obs, rows, d_U, d_u0, d_X, d_status, d_iters, d_target);
    else
        hipLaunchKernelGGL((mpc_ltv_kernel<kLtvOcc, 0>), dim3((unsigned)B), dim3(kBlock), lds, stream, P, B, h->d_ref, h->M,
                           d_state, d_obs, rows, d_U, d_u0, d_X, d_status, d_iters, d_target);
    HIP_TRY(hipGetLastError());
    return MPC_OK;
}

int mpc_ltv_solve_batch(mpc_handle *h, int32_t B, const double *state, uint32_t flags, double *u0, double *U, double *X,
                        int32_t *status, int32_t *iters, int32_t *target_index, void *stream_) {
    if (!h) return fail(MPC_ERR_INVALID_ARG, "mpc_ltv_solve_batch: null handle");
    if (B < 0 || !state || !u0 || !U)
        return fail(MPC_ERR_INVALID_ARG, "mpc_ltv_solve_batch: null required pointer or negative batch");
    if (!h->d_ref) return fail(MPC_ERR_NO_REFERENCE, "mpc_ltv_solve_batch: call mpc_set_reference first");
    if (B == 0) return MPC_OK;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int N = h->cfg.horizon;
    const size_t N1 = (size_t)N + 1;
    const bool dev = (flags & MPC_FLAG_DEVICE_PTRS) != 0;
    Staging st(h, stream, dev);
    const auto s_state = st.in(state, (size_t)B * 4 * 8);
    const auto s_u0 = st.out(u0, (size_t)B * 2 * 8);
    const auto s_U = st.inout(U, (size_t)B * N * 2 * 8);            // stored profile in, new profile out
    const auto s_X = st.out(X, (size_t)B * N1 * 4 * 8);             // optional
    const auto s_st = st.out(status, (size_t)B * 4, Staging::kReserve);
    const auto s_it = st.out(iters, (size_t)B * 4, Staging::kReserve);
    const auto s_tg = st.out(target_index, (size_t)B * 4, Staging::kReserve);
    if (int rc = st.commit()) return rc;
    if (int rc = launch_ltv(h, B, stream, st.ptr(s_state), nullptr, 0, st.ptr(s_U), st.ptr(s_u0), st.ptr(s_X), st.ptr(s_st),
                            st.ptr(s_it), st.ptr(s_tg)))
        return rc;
    return st.finish(flags);
}

int mpc_ltv_predict_batch(mpc_handle *h, int32_t B, const float *obs, int32_t vehicles_count, uint32_t flags, double *act,
                          int32_t *status, int32_t *iters, void *stream_) {
    return mpc_ltv_predict_batch_plan(h, B, obs, vehicles_count, flags, act, nullptr, nullptr, status, iters, stream_);
}

// the one body of that entry; U / X: the plan, or NULL (the same launch and the same bits either way)
int mpc_ltv_predict_batch_plan(mpc_handle *h, int32_t B, const float *obs, int32_t vehicles_count, uint32_t flags, double *act,
                               double *U, double *X, int32_t *status, int32_t *iters, void *stream_) {
    if (!h) return fail(MPC_ERR_INVALID_ARG, "mpc_ltv_predict_batch: null handle");
    if (B < 0 || !obs || !act)
        return fail(MPC_ERR_INVALID_ARG, "mpc_ltv_predict_batch: null required pointer or negative batch");
    if (vehicles_count < 1 || vehicles_count > MPC_MAX_OTHERS + 1)
        return fail(MPC_ERR_INVALID_ARG, "mpc_ltv_predict_batch: vehicles_count out of range");
    if (!h->d_ref) return fail(MPC_ERR_NO_REFERENCE, "mpc_ltv_predict_batch: call mpc_set_reference first");
    if (B == 0) return MPC_OK;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int rows = vehicles_count, N = h->cfg.horizon;
    const bool dev = (flags & MPC_FLAG_DEVICE_PTRS) != 0;
    if (int rc = ensure_env(h, B, stream)) return rc;
    Staging st(h, stream, dev);
    const auto s_obs = st.in(obs, (size_t)B * rows * mpc::pre::kObsCols * 4);
    const auto s_act = st.out(act, (size_t)B * 2 * 8);
    const auto s_U = st.out(U, (size_t)B * N * 2 * 8);                        // optional
    const auto s_X = st.inout(X, (size_t)B * ((size_t)N + 1) * 4 * 8);        // optional; in: the kernel skips some rows
    const auto s_st = st.out(status, (size_t)B * 4, Staging::kReserve);
    const auto s_it = st.out(iters, (size_t)B * 4, Staging::kReserve);
    if (int rc = st.commit()) return rc;
    if (int rc = launch_ltv(h, B, stream, nullptr, st.ptr(s_obs), rows, h->d_ltv_u, st.ptr(s_act), st.ptr(s_X), st.ptr(s_st),
                            st.ptr(s_it), nullptr))
        return rc;
    // the kernel's U is the stored profile, which stays what it is: the plan's U is a copy of it
    if (st.ptr(s_U))
        HIP_TRY(hipMemcpyAsync(st.ptr(s_U), h->d_ltv_u, (size_t)B * N * 2 * 8, hipMemcpyDeviceToDevice, stream));
    return st.finish(flags);
}

int mpc_reset_env_state(mpc_handle *h, const int32_t *env_ids, int32_t n, void *stream_) {
    if (!h) return fail(MPC_ERR_INVALID_ARG, "mpc_reset_env_state: null handle");
    if (!h->d_env) return MPC_OK;   // nothing allocated yet: every environment is fresh
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (!env_ids || n < 0) {
        HIP_TRY(hipMemsetAsync(h->d_env, 0, (size_t)h->env_cap * sizeof(mpc::pre::EnvState), stream));
        HIP_TRY(hipMemsetAsync(h->d_warm_valid, 0, (size_t)h->env_cap, stream));
        HIP_TRY(hipMemsetAsync(h->d_ltv_u, 0, (size_t)h->env_cap * h->cfg.horizon * 2 * sizeof(double), stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return MPC_OK;
    }
    if (n == 0) return MPC_OK;
    size_t cap = 256;                           // handle-owned, grow-only (no allocation per call)
    while (cap < (size_t)n) cap *= 2;
    if (int rc = grow(h->ids, cap * 4, stream, nullptr)) return rc;      // (this call is synchronous: never captured)
    int32_t *d_ids = static_cast<int32_t *>(h->ids.p);
    hipError_t e = hipMemcpyAsync(d_ids, env_ids, (size_t)n * 4, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(mpc_env_reset_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (int)n, d_ids,
                           (const uint8_t *)nullptr, h->d_env, h->d_warm_valid, h->env_cap, 0, h->d_ltv_u, h->cfg.horizon * 2);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(MPC_ERR_HIP, std::string("mpc_reset_env_state: ") + hipGetErrorString(e));
    return MPC_OK;
}

int mpc_reset_env_mask(mpc_handle *h, int32_t B, const uint8_t *done, uint32_t flags, void *stream_) {
    if (!h || B < 0 || !done) return fail(MPC_ERR_INVALID_ARG, "mpc_reset_env_mask: bad argument");
    if (!h->d_env || B == 0) return MPC_OK;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    Staging st(h, stream, (flags & MPC_FLAG_DEVICE_PTRS) != 0);
    const auto s_done = st.in(done, (size_t)B);
    if (int rc = st.commit()) return rc;
    const int n = B < h->env_cap ? B : h->env_cap;
    hipLaunchKernelGGL(mpc_env_reset_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n,
                       (const int32_t *)nullptr, st.ptr(s_done), h->d_env, h->d_warm_valid, h->env_cap,
                       (flags & MPC_FLAG_WARM_START) ? 1 : 0, (flags & MPC_FLAG_WARM_START) ? nullptr : h->d_ltv_u,
                       h->cfg.horizon * 2);
    HIP_TRY(hipGetLastError());
    return st.finish(flags);
}

int mpc_get_env_state(mpc_handle *h, int32_t B, int32_t *is_collide, int32_t *ego_index, int32_t *collision_memory,
                      int32_t *stop_index, int32_t *conflict_index, double *conflict_points) {
    if (!h || B < 0) return fail(MPC_ERR_INVALID_ARG, "mpc_get_env_state: bad argument");
    if (B == 0) return MPC_OK;
    if (!h->d_env || B > h->env_cap) return fail(MPC_ERR_INVALID_ARG, "mpc_get_env_state: no such environments");
    HIP_TRY(hipSetDevice(h->device));
    std::vector<mpc::pre::EnvState> host((size_t)B);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(host.data(), h->d_env, (size_t)B * sizeof(mpc::pre::EnvState), hipMemcpyDeviceToHost));
    for (int b = 0; b < B; ++b) {
        const mpc::pre::EnvState &s = host[(size_t)b];
        if (is_collide) is_collide[b] = s.is_collide;
        if (ego_index) ego_index[b] = s.ego_index;
        if (collision_memory) collision_memory[b] = s.collision_memory;
        if (stop_index) stop_index[b] = s.stop_index1 - 1;
        if (conflict_index)
            for (int j = 0; j < MPC_MAX_OTHERS; ++j)
                conflict_index[(size_t)b * MPC_MAX_OTHERS + j] = j < s.n_conflict ? s.conflict[j] : -1;
        if (conflict_points)
            for (int j = 0; j < MPC_MAX_OTHERS; ++j) {
                const bool hit = j < s.n_conflict && s.conflict[j] >= 0;
                conflict_points[((size_t)b * MPC_MAX_OTHERS + j) * 2 + 0] = hit ? s.conflict_pt[j][0] : NAN;
                conflict_points[((size_t)b * MPC_MAX_OTHERS + j) * 2 + 1] = hit ? s.conflict_pt[j][1] : NAN;
            }
    }
    return MPC_OK;
}

int64_t mpc_env_state_bytes(void) { return (int64_t)sizeof(mpc::pre::EnvState); }

int mpc_save_env_state(mpc_handle *h, int32_t B, void *records) {
    if (!h || B < 0 || (!records && B > 0)) return fail(MPC_ERR_INVALID_ARG, "mpc_save_env_state: bad argument");
    if (B == 0) return MPC_OK;
    if (!h->d_env || B > h->env_cap) return fail(MPC_ERR_INVALID_ARG, "mpc_save_env_state: no such environments");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(records, h->d_env, (size_t)B * sizeof(mpc::pre::EnvState), hipMemcpyDeviceToHost));
    return MPC_OK;
}

int mpc_set_env_state(mpc_handle *h, int32_t B, const void *records) {
    if (!h || B < 0 || (!records && B > 0)) return fail(MPC_ERR_INVALID_ARG, "mpc_set_env_state: bad argument");
    if (B == 0) return MPC_OK;
    // the records are opaque to the caller but not trusted: the device code uses the counts as loop bounds and the
    // indices as subscripts of the reference table
    if (!h->d_ref) return fail(MPC_ERR_NO_REFERENCE, "mpc_set_env_state: call mpc_set_reference first (indices are checked against it)");
    {
        const auto *rec = static_cast<const mpc::pre::EnvState *>(records);
        const int M = h->M, K = mpc::pre::kMaxOthers;
        for (int b = 0; b < B; ++b) {
            const mpc::pre::EnvState &s = rec[b];
            bool ok = s.collision_memory >= 0 && s.collision_memory <= 10 && (s.has_memorized == 0 || s.has_memorized == 1) &&
                      s.n_memorized >= 0 && s.n_memorized <= K && s.n_conflict >= 0 && s.n_conflict <= K &&
                      (s.is_collide == 0 || s.is_collide == 1) && s.ego_index >= 0 && s.ego_index < M &&
                      s.stop_index1 >= 0 && s.stop_index1 <= M && s.last_valid_stop1 >= 0 && s.last_valid_stop1 <= M;
            for (int j = 0; ok && j < K; ++j)
                ok = s.conflict[j] >= -1 && s.conflict[j] < M && s.memorized[j] >= -1 && s.memorized[j] < M;
            if (!ok) return fail(MPC_ERR_INVALID_ARG, "mpc_set_env_state: record " + std::to_string(b) + " is not a valid detector state");
        }
    }
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    if (int rc = ensure_env(h, B, nullptr)) return rc;
    HIP_TRY(hipMemcpy(h->d_env, records, (size_t)B * sizeof(mpc::pre::EnvState), hipMemcpyHostToDevice));
    // a restored environment is not the episode whose controls the handle remembers: no warm start, no stored LTV profile
    HIP_TRY(hipMemset(h->d_warm_valid, 0, (size_t)B));
    HIP_TRY(hipMemset(h->d_ltv_u, 0, (size_t)B * h->cfg.horizon * 2 * sizeof(double)));
    return MPC_OK;
}

int mpc_streams_overlap(int32_t device, void *stream_a, void *stream_b, int32_t *overlap) {
    if (!overlap) return fail(MPC_ERR_INVALID_ARG, "mpc_streams_overlap: null output pointer");
    HIP_TRY(hipSetDevice(device));
    hipStream_t sa = static_cast<hipStream_t>(stream_a), sb = static_cast<hipStream_t>(stream_b);
    if (sa == sb) {
        *overlap = 0;
        return MPC_OK;
    }
    const long long ticks = 30000;       // of the 100 MHz constant clock: 0.3 ms, long against a launch, short against anything else
    auto timed = [&](bool both, double &ms) -> int {
        HIP_TRY(hipStreamSynchronize(sa));
        HIP_TRY(hipStreamSynchronize(sb));
        const auto t0 = std::chrono::steady_clock::now();
        hipLaunchKernelGGL(mpc_timer_kernel, dim3(1), dim3(64), 0, sa, ticks);
        if (both) hipLaunchKernelGGL(mpc_timer_kernel, dim3(1), dim3(64), 0, sb, ticks);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(sa));
        HIP_TRY(hipStreamSynchronize(sb));
        ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return MPC_OK;
    };
    double one = 0.0, two = 0.0, warm = 0.0;
    if (int rc = timed(true, warm)) return rc;       // first launch of the kernel on these streams: code load, queue wake-up
    if (int rc = timed(false, one)) return rc;
    if (int rc = timed(true, two)) return rc;
    *overlap = two < 1.5 * one ? 1 : 0;
    return MPC_OK;
}

// argument checks and launch geometry of the two entry points of the synthetic environment: sixteen lanes per environment,
// four environments per block; *blocks = 0 where there is nothing to launch
static int synth_env_launch_shape(const std::string &who, int32_t device, int32_t B, int32_t K, double dt, int32_t M,
                                  bool state_ok, bool outputs_ok, unsigned *blocks) {
    *blocks = 0;
    if (B < 0 || K < 0 || K > mpc::env::kMaxOthers || !(dt > 0.0) || M < 1) return fail(MPC_ERR_INVALID_ARG, who + ": bad size");
    if (!state_ok) return fail(MPC_ERR_INVALID_ARG, who + ": null state pointer");
    if (!outputs_ok) return fail(MPC_ERR_INVALID_ARG, who + ": null output pointer");
    if (B == 0) return MPC_OK;
    HIP_TRY(hipSetDevice(device));
    if (M > mpc::env::kMaxRoutePoints) return fail(MPC_ERR_INVALID_ARG, who + ": at most 15 other vehicles and 128 route points");
    *blocks = (unsigned)((B + 3) / 4);
    return MPC_OK;
}

int mpc_synth_env_step(int32_t device, int32_t B, int32_t K, double dt, double spawn_probability, uint64_t seed,
                       int32_t env_offset, const double *ref_xy, int32_t M, const double *action, double *ego, double *opos,
                       double *ospeed, double *ohead, uint8_t *oactive, int32_t *t, int64_t *rng_counter, float *obs,
                       float *terminal_obs, float *reward, uint8_t *done, uint8_t *truncated, uint8_t *crashed,
                       uint8_t *arrived, int32_t reset_all, void *stream_) {
    unsigned blocks;
    const int rc = synth_env_launch_shape(
        "mpc_synth_env_step", device, B, K, dt, M, ref_xy && ego && opos && ospeed && ohead && oactive && t && rng_counter && obs,
        reset_all || (action && terminal_obs && reward && done && truncated && crashed && arrived), &blocks);
    if (rc || !blocks) return rc;
    hipLaunchKernelGGL(mpc_synth_env_rows_kernel, dim3(blocks), dim3(64), 0, reinterpret_cast<hipStream_t>(stream_),
                       (int)B, (int)K, dt, spawn_probability, seed, (int)env_offset, ref_xy, (int)M, action, ego, opos, ospeed,
                       ohead, oactive, t, rng_counter, obs, terminal_obs, reward, done, truncated, crashed, arrived,
                       (int)reset_all);
    HIP_TRY(hipGetLastError());
    return MPC_OK;
}

int mpc_synth_env_step_idm(int32_t device, int32_t B, int32_t K, double dt, double spawn_probability, uint64_t seed,
                           int32_t env_offset, const double *ref_xy, int32_t M, const double *action, double *ego, double *opos,
                           double *ospeed, double *ohead, uint8_t *oactive, int32_t *oroute, double *oprog, double *otarget,
                           int32_t *t, int64_t *rng_counter, float *obs, float *terminal_obs, float *reward, uint8_t *done,
                           uint8_t *truncated, uint8_t *crashed, uint8_t *arrived, int32_t reset_all, void *stream_) {
    unsigned blocks;
    const int rc = synth_env_launch_shape(
        "mpc_synth_env_step_idm", device, B, K, dt, M,
        ref_xy && ego && opos && ospeed && ohead && oactive && oroute && oprog && otarget && t && rng_counter && obs,
        reset_all || (action && terminal_obs && reward && done && truncated && crashed && arrived), &blocks);
    if (rc || !blocks) return rc;
    hipLaunchKernelGGL(mpc_synth_env_idm_kernel, dim3(blocks), dim3(64), 0, reinterpret_cast<hipStream_t>(stream_),
                       (int)B, (int)K, dt, spawn_probability, seed, (int)env_offset, ref_xy, (int)M, action, ego, opos, ospeed,
                       ohead, oactive, oroute, oprog, otarget, t, rng_counter, obs, terminal_obs, reward, done, truncated,
                       crashed, arrived, (int)reset_all);
    HIP_TRY(hipGetLastError());
    return MPC_OK;
}

int mpc_policy_act(int32_t device, int32_t B, int32_t A, int32_t H2, const float *obs, const float *w1, const float *b1,
                   const float *w2, const float *b2, const float *wh, const float *bh, const float *std_, const float *c0,
                   float *noise, uint64_t noise_seed, int32_t env_offset, const int64_t *noise_step, int32_t version_v1,
                   int32_t clip, float *actions, float *values, float *log_probs, double *mpc_weights, double *mpc_ref_speed,
                   void *stream_) {
    if (B < 0 || A < 1 || A > mpc::glue::kMaxAction || H2 < 2 || H2 > mpc::glue::kMaxHidden2 || (H2 & 1))
        return fail(MPC_ERR_INVALID_ARG, "mpc_policy_act: bad size (action_dim 1..8, 2 x hidden <= 256)");
    if (!obs || !w1 || !b1 || !w2 || !b2 || !wh || !bh || !std_ || !c0 || !noise || !actions || !values || !log_probs)
        return fail(MPC_ERR_INVALID_ARG, "mpc_policy_act: null pointer");
    if (version_v1 ? (!mpc_weights || A < 3) : !mpc_ref_speed)
        return fail(MPC_ERR_INVALID_ARG, "mpc_policy_act: v1 needs mpc_weights and >= 3 action components, v0 needs mpc_ref_speed");
    if (B == 0) return MPC_OK;
    HIP_TRY(hipSetDevice(device));
    const mpc::glue::PolicyWeights W{w1, b1, w2, b2, wh, bh, std_, c0};
    const int threads = H2 > mpc::glue::kObsDim ? H2 : mpc::glue::kObsDim;
    hipLaunchKernelGGL(mpc_policy_act_kernel, dim3((unsigned)B), dim3((unsigned)((threads + 63) / 64 * 64)), 0,
                       reinterpret_cast<hipStream_t>(stream_), (int)B, (int)A, (int)H2, obs, W, noise, (unsigned long long)noise_seed,
                       (int)env_offset, reinterpret_cast<const long long *>(noise_step), (int)version_v1, (int)clip,
                       actions, values, log_probs, version_v1 ? mpc_weights : nullptr, version_v1 ? nullptr : mpc_ref_speed);
    HIP_TRY(hipGetLastError());
    return MPC_OK;
}

int mpc_policy_act_sde(int32_t device, int32_t B, int32_t A, int32_t H2, const float *obs, const float *w1, const float *b1,
                       const float *w2, const float *b2, const float *wh, const float *bh, const float *sde_std,
                       const float *sde_noise, uint64_t noise_seed, int32_t env_offset, const int64_t *sde_epoch,
                       const int64_t *sde_step, int32_t sde_sample_freq, int32_t version_v1, int32_t clip, float *actions,
                       float *values, float *log_probs, double *mpc_weights, double *mpc_ref_speed, void *stream_) {
    if (B < 0 || A < 1 || A > mpc::glue::kMaxAction || H2 < 2 || H2 > mpc::glue::kMaxHidden2 || (H2 & 1))
        return fail(MPC_ERR_INVALID_ARG, "mpc_policy_act_sde: bad size (action_dim 1..8, 2 x hidden <= 256)");
    if (!obs || !w1 || !b1 || !w2 || !b2 || !wh || !bh || !sde_std || !actions || !values || !log_probs)
        return fail(MPC_ERR_INVALID_ARG, "mpc_policy_act_sde: null pointer");
    if (!sde_noise == !sde_epoch)
        return fail(MPC_ERR_INVALID_ARG, "mpc_policy_act_sde: exactly one of sde_noise (read) and sde_epoch (drawn)");
    if (version_v1 ? (!mpc_weights || A < 3) : !mpc_ref_speed)
        return fail(MPC_ERR_INVALID_ARG, "mpc_policy_act_sde: v1 needs mpc_weights and >= 3 action components, v0 needs mpc_ref_speed");
    if (B == 0) return MPC_OK;
    HIP_TRY(hipSetDevice(device));
    const mpc::glue::PolicyWeights W{w1, b1, w2, b2, wh, bh, sde_std, nullptr};
    // at least two waves: the second reduces the noise and the variance while the first computes the heads
    const int threads = H2 > 128 ? H2 : 128;
    hipLaunchKernelGGL(mpc_policy_act_sde_kernel, dim3((unsigned)B), dim3((unsigned)((threads + 63) / 64 * 64)), 0,
                       reinterpret_cast<hipStream_t>(stream_), (int)B, (int)A, (int)H2, obs, W, sde_noise,
                       (unsigned long long)noise_seed, (int)env_offset, reinterpret_cast<const long long *>(sde_epoch),
                       reinterpret_cast<const long long *>(sde_step), (int)sde_sample_freq, (int)version_v1, (int)clip,
                       actions, values, log_probs, version_v1 ? mpc_weights : nullptr, version_v1 ? nullptr : mpc_ref_speed);
    HIP_TRY(hipGetLastError());
    return MPC_OK;
}

int mpc_policy_control_tile(int32_t tile, int32_t device, int32_t B, int32_t H2, const float *obs, const float *w1, const float *b1,
                            const float *w2, const float *b2, const float *wh, const float *bh, const float *std_, const float *c0,
                            float *noise, uint64_t noise_seed, int32_t env_offset, const int64_t *noise_step, float *actions,
                            float *values, float *log_probs, double *control, void *stream_) {
    if (B < 0 || H2 < 2 || H2 > mpc::glue::kMaxHidden2 || (H2 & 1))
        return fail(MPC_ERR_INVALID_ARG, "mpc_policy_control: bad size (2 x hidden even and <= 256)");
    if (tile != 1 && tile != 2 && tile != 4 && tile != 8 && tile != 16)
        return fail(MPC_ERR_INVALID_ARG, "mpc_policy_control_tile: tile must be 1, 2, 4, 8 or 16");
    if (!obs || !w1 || !b1 || !w2 || !b2 || !wh || !bh || !std_ || !c0 || !noise || !actions || !values || !log_probs || !control)
        return fail(MPC_ERR_INVALID_ARG, "mpc_policy_control: null pointer");
    if (B == 0) return MPC_OK;
    HIP_TRY(hipSetDevice(device));
    const mpc::glue::PolicyWeights W{w1, b1, w2, b2, wh, bh, std_, c0};
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
#define MPC_CONTROL_TILE(E) \
    case E: launch_policy_control<E>(stream, B, H2, obs, W, noise, noise_seed, env_offset, noise_step, actions, values, log_probs, control); break
    switch (tile) {
        MPC_CONTROL_TILE(1);
        MPC_CONTROL_TILE(2);
        MPC_CONTROL_TILE(4);
        MPC_CONTROL_TILE(8);
        MPC_CONTROL_TILE(16);
    }
#undef MPC_CONTROL_TILE
    HIP_TRY(hipGetLastError());
    return MPC_OK;
}

int mpc_policy_control(int32_t device, int32_t B, int32_t H2, const float *obs, const float *w1, const float *b1, const float *w2,
                       const float *b2, const float *wh, const float *bh, const float *std_, const float *c0, float *noise,
                       uint64_t noise_seed, int32_t env_offset, const int64_t *noise_step, float *actions, float *values,
                       float *log_probs, double *control, void *stream_) {
    // the tile pays once its workgroups still fill the GPU (measured: DESIGN.md 5.2); the bits are the same either way
    return mpc_policy_control_tile(B >= MPC_POLICY_CONTROL_TILE_FROM ? MPC_POLICY_CONTROL_TILE : 1, device, B, H2, obs, w1, b1, w2, b2, wh, bh, std_, c0, noise, noise_seed,
                                   env_offset, noise_step, actions, values, log_probs, control, stream_);
}

int mpc_rollout_record(int32_t device, int32_t T, int32_t B, int32_t A, int32_t cols, int32_t keep_terminal, float *row,
                       double *mpc_actions_buf, int64_t *pos_dev, int32_t *ticket, float *last_obs, float *last_starts,
                       const float *actions, const float *values, const float *log_probs, const double *mpc_act,
                       const int32_t *mpc_status, const float *new_obs, const float *reward, const uint8_t *done,
                       const float *terminal_obs, const uint8_t *truncated, const uint8_t *crashed, const uint8_t *arrived,
                       int64_t *counts, uint8_t *dones_out, int64_t *step_counter, void *stream_) {
    constexpr int O = mpc::glue::kObsDim;
    if (T < 1 || B < 0 || A < 1 || A > mpc::glue::kMaxAction || cols != O + A + 4 + (keep_terminal ? O + 1 : 0))
        return fail(MPC_ERR_INVALID_ARG, "mpc_rollout_record: bad size / row layout");
    if (!row || !mpc_actions_buf || !pos_dev || !ticket || !last_obs || !last_starts || !actions || !values || !log_probs ||
        !mpc_act || !mpc_status || !new_obs || !reward || !done || !crashed || !arrived || !counts || !dones_out ||
        (keep_terminal && (!terminal_obs || !truncated)))
        return fail(MPC_ERR_INVALID_ARG, "mpc_rollout_record: null pointer");
    if (B == 0) return MPC_OK;
    HIP_TRY(hipSetDevice(device));
    const mpc::glue::RecordArgs R{(int)B, (int)A, (int)cols, (int)keep_terminal, row, mpc_actions_buf, last_obs, last_starts, actions,
                                 values, log_probs, mpc_act, mpc_status, new_obs, reward, done, terminal_obs, truncated, crashed,
                                 arrived, dones_out};
    hipLaunchKernelGGL(mpc_rollout_record_kernel, dim3((unsigned)B), dim3(128), 0, reinterpret_cast<hipStream_t>(stream_), R, (int)T,
                       reinterpret_cast<long long *>(pos_dev), ticket, reinterpret_cast<unsigned long long *>(counts),
                       reinterpret_cast<long long *>(step_counter));
    HIP_TRY(hipGetLastError());
    return MPC_OK;
}

int mpc_rollout_finish(int32_t device, int32_t T, int32_t B, int32_t A, int32_t cols, int32_t keep_terminal, float *row,
                       const float *last_values, const uint8_t *dones, const float *terminal_values, double gamma,
                       double gae_lambda, float *advantages, float *returns, void *stream_) {
    constexpr int O = mpc::glue::kObsDim;
    if (T < 1 || T > 8192 || B < 0 || A < 1 || A > mpc::glue::kMaxAction || cols != O + A + 4 + (keep_terminal ? O + 1 : 0))
        return fail(MPC_ERR_INVALID_ARG, "mpc_rollout_finish: bad size / row layout (1 <= T <= 8192)");
    if (!row || !last_values || !dones || !advantages || !returns)
        return fail(MPC_ERR_INVALID_ARG, "mpc_rollout_finish: null pointer");
    if (B == 0) return MPC_OK;
    HIP_TRY(hipSetDevice(device));
    const mpc::glue::GaeArgs g{(int)T, (int)B, (int)A, (int)cols, (int)keep_terminal, row, last_values, dones, terminal_values,
                              (float)gamma, (float)(gamma * gae_lambda), advantages, returns};
    hipLaunchKernelGGL(mpc_rollout_finish_kernel, dim3((unsigned)B), dim3(256), (size_t)T * 2 * sizeof(float),
                       reinterpret_cast<hipStream_t>(stream_), g);
    HIP_TRY(hipGetLastError());
    return MPC_OK;
}

int mpc_episode_stats(int32_t device, int32_t B, int32_t Q, int32_t reset, const uint8_t *done, const uint8_t *truncated,
                      const uint8_t *crashed, const uint8_t *arrived, const float *reward, const double *ego,
                      const int32_t *status, const int32_t *iters, int32_t *state_i32, double *state_f64, int32_t *rec_i32,
                      double *rec_f64, int64_t *recorded, int64_t *step_counter, void *stream_) {
    if (B < 0 || Q < 1) return fail(MPC_ERR_INVALID_ARG, "mpc_episode_stats: bad size (B >= 0, Q >= 1)");
    if (!ego || !state_i32 || !state_f64 || !rec_i32 || !rec_f64 || !recorded)
        return fail(MPC_ERR_INVALID_ARG, "mpc_episode_stats: null state / record pointer");
    if (!reset && (!done || !truncated || !crashed || !arrived || !reward || !status || !iters))
        return fail(MPC_ERR_INVALID_ARG, "mpc_episode_stats: null step-input pointer");
    if (B == 0) return MPC_OK;
    HIP_TRY(hipSetDevice(device));
    const mpc::stats::Accounts acc{(int)B, (int)Q, state_i32, state_f64, rec_i32, rec_f64};
    const mpc::stats::StepInputs in{done, truncated, crashed, arrived, reward, ego, status, iters};
    hipLaunchKernelGGL(mpc_episode_stats_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream_), acc, in, (int)reset,
                       reinterpret_cast<unsigned long long *>(recorded), reinterpret_cast<long long *>(step_counter));
    HIP_TRY(hipGetLastError());
    return MPC_OK;
}

int mpc_drive_metrics(int32_t device, int32_t B, int32_t R, int32_t Q, int32_t M, int32_t reset, double dt,
                      const float *terminal_obs, const float *obs, const double *action, const uint8_t *done,
                      const double *ref_xy, int32_t *state_i32, double *state_f64, int32_t *rec_i32, double *rec_f64,
                      void *stream_) {
    if (B < 0 || Q < 1 || R < 1 || R > MPC_MAX_OTHERS + 1 || M < 1 || M > mpc::drive::kMaxRoute || !(dt > 0.0))
        return fail(MPC_ERR_INVALID_ARG, "mpc_drive_metrics: bad size (B >= 0, Q >= 1, 1 <= R <= 17, 1 <= M <= 128, dt > 0)");
    if (!obs || !ref_xy || !state_i32 || !state_f64 || !rec_i32 || !rec_f64)
        return fail(MPC_ERR_INVALID_ARG, "mpc_drive_metrics: null obs / ref_xy / state / record pointer");
    if (!reset && (!terminal_obs || !action || !done))
        return fail(MPC_ERR_INVALID_ARG, "mpc_drive_metrics: null step-input pointer");
    if (B == 0) return MPC_OK;
    HIP_TRY(hipSetDevice(device));
    const mpc::drive::Accounts acc{(int)B, (int)Q, state_i32, state_f64, rec_i32, rec_f64};
    const mpc::drive::StepInputs in{(int)R, (int)M, dt, terminal_obs, obs, action, done, ref_xy};
    hipLaunchKernelGGL(mpc_drive_metrics_kernel, dim3((unsigned)((B + 3) / 4)), dim3(64), 0,
                       reinterpret_cast<hipStream_t>(stream_), acc, in, (int)reset);
    HIP_TRY(hipGetLastError());
    return MPC_OK;
}

int mpc_interaction_metrics(int32_t device, int32_t B, int32_t K, int32_t Q, int32_t M, int32_t reset, double dt,
                            const double *ego, const double *opos, const double *ospeed, const double *ohead,
                            const uint8_t *oactive, const int32_t *oroute, const double *oprog, const double *otarget,
                            const uint8_t *done, const double *ref_xy, const double *conflict, int32_t *state_i32,
                            double *state_f64, int32_t *rec_i32, double *rec_f64, void *stream_) {
    if (B < 0 || Q < 1 || K < 1 || K > mpc::env::kMaxOthers || M < 1 || M > mpc::interact::kMaxRoute || !(dt > 0.0))
        return fail(MPC_ERR_INVALID_ARG,
                    "mpc_interaction_metrics: bad size (B >= 0, Q >= 1, 1 <= K <= 9, 1 <= M <= 128, dt > 0)");
    if (!ego || !opos || !ospeed || !ohead || !oactive || !oroute || !oprog || !otarget)
        return fail(MPC_ERR_INVALID_ARG, "mpc_interaction_metrics: null environment state pointer");
    if (!ref_xy || !conflict || !state_i32 || !state_f64 || !rec_i32 || !rec_f64)
        return fail(MPC_ERR_INVALID_ARG, "mpc_interaction_metrics: null ref_xy / conflict / state / record pointer");
    if (!reset && !done) return fail(MPC_ERR_INVALID_ARG, "mpc_interaction_metrics: null done of a non-reset launch");
    if (B == 0) return MPC_OK;
    HIP_TRY(hipSetDevice(device));
    const mpc::interact::Accounts acc{(int)B, (int)Q, state_i32, state_f64, rec_i32, rec_f64};
    const mpc::interact::StepInputs in{(int)K, (int)M, dt, ego, opos, ospeed, ohead, oactive, oroute, oprog, otarget, done,
                                       ref_xy, conflict};
    hipLaunchKernelGGL(mpc_interaction_kernel, dim3((unsigned)((B + 3) / 4)), dim3(64), 0,
                       reinterpret_cast<hipStream_t>(stream_), acc, in, (int)reset);
    HIP_TRY(hipGetLastError());
    return MPC_OK;
}

int mpc_episode_trace(int32_t device, int32_t B, int32_t R, int32_t Q, int32_t W, int32_t C, int32_t keep, int32_t reset,
                      const float *terminal_obs, const float *obs, const float *seen, const double *action,
                      const float *reward, const uint8_t *done, const uint8_t *truncated, const uint8_t *crashed,
                      const uint8_t *arrived, const int32_t *status, const int32_t *iters, int32_t *state_i32,
                      float *ring_scene, float *ring_seen, double *ring_act, float *ring_reward, int32_t *ring_i32,
                      int32_t *slot, float *kept_scene, float *kept_seen, double *kept_act, float *kept_reward,
                      int32_t *kept_i32, int32_t *index, int64_t *counts, void *stream_) {
    namespace tr = mpc::trace;
    if (B < 0 || R < 1 || R > MPC_MAX_OTHERS + 1 || Q < 1 || W < 1 || W > tr::kMaxWindow || C < 1 || keep < 1 || keep > 31)
        return fail(MPC_ERR_INVALID_ARG, "mpc_episode_trace: bad size (B >= 0, 1 <= R <= 17, Q >= 1, 1 <= W <= 4096, C >= 1, "
                                         "1 <= keep <= 31)");
    if (!state_i32 || !ring_scene || !ring_act || !ring_reward || !ring_i32 || !slot || !kept_scene || !kept_act ||
        !kept_reward || !kept_i32 || !index || !counts)
        return fail(MPC_ERR_INVALID_ARG, "mpc_episode_trace: null state / ring / slot / store / index / counts pointer");
    if (!obs) return fail(MPC_ERR_INVALID_ARG, "mpc_episode_trace: null obs");
    if (!reset && (!terminal_obs || !action || !reward || !done || !truncated || !crashed || !arrived || !status || !iters))
        return fail(MPC_ERR_INVALID_ARG, "mpc_episode_trace: null step-input pointer of a non-reset launch");
    if ((ring_seen != nullptr) != (kept_seen != nullptr) || (!reset && (seen != nullptr) != (ring_seen != nullptr)))
        return fail(MPC_ERR_INVALID_ARG, "mpc_episode_trace: seen, ring_seen and kept_seen must all be given or all be NULL");
    for (const void *p : {(const void *)terminal_obs, (const void *)obs, (const void *)seen, (const void *)ring_scene,
                          (const void *)ring_seen, (const void *)kept_scene, (const void *)kept_seen})
        if (((uintptr_t)p & 15) != 0)
            return fail(MPC_ERR_INVALID_ARG, "mpc_episode_trace: the observation, ring and store planes of scenes must be "
                                             "16-byte aligned");
    if (B == 0) return MPC_OK;
    HIP_TRY(hipSetDevice(device));
    const tr::Recorder rec{(int)B, (int)R, (int)Q, (int)W, (int)C, (int)keep, state_i32, ring_scene, ring_seen, ring_act,
                           ring_reward, ring_i32, slot, kept_scene, kept_seen, kept_act, kept_reward, kept_i32, index, counts};
    const tr::StepInputs in{terminal_obs, obs, seen, action, reward, done, truncated, crashed, arrived, status, iters};
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(mpc_episode_trace_claim_kernel, dim3(1), dim3(kTraceClaimThreads), 0, stream, rec, in, (int)reset);
    hipLaunchKernelGGL(mpc_episode_trace_frame_kernel, dim3((unsigned)B), dim3(kTraceFrameThreads), 0, stream, rec, in,
                       (int)reset);
    HIP_TRY(hipGetLastError());
    return MPC_OK;
}

int mpc_perceive(int32_t device, int32_t B, int32_t R, int32_t S, int32_t reset, const mpc_perception *params,
                 const float *obs_true, const double *occluders, float *obs_seen, uint8_t *row_class, int64_t *counts,
                 int64_t *ctr, void *stream_) {
    if (B < 0 || R < 1 || R > MPC_MAX_OTHERS + 1 || S < 0 || S > mpc::sense::kMaxOccluders)
        return fail(MPC_ERR_INVALID_ARG, "mpc_perceive: bad size (B >= 0, 1 <= R <= 17, 0 <= S <= 8)");
    if (!params || !obs_true || !obs_seen || !counts || !ctr || (S > 0 && !occluders))
        return fail(MPC_ERR_INVALID_ARG, "mpc_perceive: null params / obs_true / obs_seen / counts / ctr / occluders pointer");
    if (obs_seen == obs_true) return fail(MPC_ERR_INVALID_ARG, "mpc_perceive: obs_seen must not be obs_true");
    if (params->struct_size != (int32_t)sizeof(mpc_perception))
        return fail(MPC_ERR_INVALID_ARG, "mpc_perceive: mpc_perception.struct_size mismatch");
    const mpc_perception &p = *params;
    if (p.min_points < 1 || p.min_points > mpc::sense::kPoints || !(p.p_drop >= 0.0 && p.p_drop <= 1.0) ||
        !(p.sigma_pos >= 0.0) || !(p.sigma_vel >= 0.0) || !(p.sigma_head >= 0.0) || !(p.range > 0.0))
        return fail(MPC_ERR_INVALID_ARG, "mpc_perceive: bad parameter (1 <= min_points <= 5, 0 <= p_drop <= 1, sigma >= 0, "
                                         "range > 0; none NaN)");
    if (B == 0) return MPC_OK;
    HIP_TRY(hipSetDevice(device));
    const mpc::sense::Params P{p.range, p.p_drop, p.sigma_pos, p.sigma_vel, p.sigma_head, p.seed, p.occlusion, p.min_points,
                               p.env_offset};
    const mpc::sense::Buffers buf{(int)B, (int)R, (int)S, obs_true, occluders, obs_seen, row_class, counts, ctr};
    hipLaunchKernelGGL(mpc_perceive_kernel, dim3((unsigned)((B + 3) / 4)), dim3(64), 0,
                       reinterpret_cast<hipStream_t>(stream_), P, buf, (int)reset);
    HIP_TRY(hipGetLastError());
    return MPC_OK;
}

int mpc_track_rows(int32_t device, int32_t B, int32_t R, int32_t reset, double dt, double gate, int32_t coast,
                   double alpha_pos, double alpha_vel, const float *obs_meas, const uint8_t *done, float *obs_out,
                   uint8_t *row_slot, uint8_t *row_miss, double *track_f64, int32_t *track_i32, int64_t *counts,
                   void *stream_) {
    if (B < 0 || R < 1 || R > mpc::track::kMaxRows)
        return fail(MPC_ERR_INVALID_ARG, "mpc_track_rows: bad size (B >= 0, 1 <= R <= 17)");
    if (!(dt > 0.0) || !(gate >= 0.0))
        return fail(MPC_ERR_INVALID_ARG, "mpc_track_rows: bad parameter (dt > 0, gate >= 0; neither NaN)");
    if (coast < 0 || coast > mpc::track::kMaxCoast)
        return fail(MPC_ERR_INVALID_ARG, "mpc_track_rows: bad parameter (0 <= coast <= 200)");
    if (!(alpha_pos > 0.0 && alpha_pos <= 1.0) || !(alpha_vel > 0.0 && alpha_vel <= 1.0))
        return fail(MPC_ERR_INVALID_ARG, "mpc_track_rows: bad parameter (0 < alpha_pos <= 1, 0 < alpha_vel <= 1; neither NaN)");
    if (!obs_meas || !obs_out || !track_f64 || !track_i32 || !counts)
        return fail(MPC_ERR_INVALID_ARG, "mpc_track_rows: null obs_meas / obs_out / track_f64 / track_i32 / counts pointer");
    if (obs_out == obs_meas) return fail(MPC_ERR_INVALID_ARG, "mpc_track_rows: obs_out must not be obs_meas");
    if (B == 0) return MPC_OK;
    HIP_TRY(hipSetDevice(device));
    const mpc::track::Params P{dt, gate * gate, alpha_pos, alpha_vel, coast};
    const mpc::track::Buffers buf{(int)B, (int)R, obs_meas, done, obs_out, row_slot, row_miss, track_f64, track_i32, counts};
    hipLaunchKernelGGL(mpc_track_kernel, dim3((unsigned)((B + 3) / 4)), dim3(64), 0, reinterpret_cast<hipStream_t>(stream_),
                       P, buf, (int)reset);
    HIP_TRY(hipGetLastError());
    return MPC_OK;
}

int mpc_actuate(int32_t device, int32_t B, int32_t reset, const mpc_actuator *params, const double *command,
                const uint8_t *done_prev, double *applied, double *state_f64, int32_t *age, int64_t *ctr, int64_t *counts,
                double *sums, void *stream_) {
    namespace act = mpc::act;
    if (B < 0) return fail(MPC_ERR_INVALID_ARG, "mpc_actuate: bad size (B >= 0)");
    if (!params || !state_f64 || !age || !ctr || !counts || !sums)
        return fail(MPC_ERR_INVALID_ARG, "mpc_actuate: null params / state_f64 / age / ctr / counts / sums pointer");
    if (reset == 0 && (!command || !applied))
        return fail(MPC_ERR_INVALID_ARG, "mpc_actuate: null command / applied pointer in a launch without reset");
    if (params->struct_size != (int32_t)sizeof(mpc_actuator))
        return fail(MPC_ERR_INVALID_ARG, "mpc_actuate: mpc_actuator.struct_size mismatch");
    const mpc_actuator &p = *params;
    const act::Params P{p.dt, p.p_hold, {p.gain[0], p.gain[1]}, {p.offset[0], p.offset[1]}, {p.sigma[0], p.sigma[1]},
                        {p.alpha[0], p.alpha[1]}, {p.rate[0], p.rate[1]}, {p.lo[0], p.lo[1]}, {p.hi[0], p.hi[1]}, p.seed,
                        p.delay, p.env_offset};
    if (const char *why = act::refusal(P))
        return fail(MPC_ERR_INVALID_ARG, std::string("mpc_actuate: bad parameter (") + why + ")");
    if (B == 0) return MPC_OK;
    HIP_TRY(hipSetDevice(device));
    const act::Buffers buf{(int)B, command, done_prev, applied, state_f64, age, ctr, counts, sums};
    hipLaunchKernelGGL(mpc_actuate_kernel, dim3((unsigned)((B + 31) / 32)), dim3(64), 0, reinterpret_cast<hipStream_t>(stream_),
                       P, buf, (int)reset);
    HIP_TRY(hipGetLastError());
    return MPC_OK;
}

int mpc_compensate(int32_t device, int32_t B, int32_t R, int32_t reset, const mpc_compensator *params, const float *obs,
                   const double *command, const uint8_t *done, float *out, double *pred, double *ring, double *prev,
                   int32_t *age, double *pring, int64_t *counts, double *sums, void *stream_) {
    namespace comp = mpc::comp;
    if (B < 0 || R < 1 || R > comp::kMaxRows)
        return fail(MPC_ERR_INVALID_ARG, "mpc_compensate: bad size (B >= 0, 1 <= R <= 17)");
    if (!params || !obs || !out || !ring || !prev || !age || !pring || !counts || !sums)
        return fail(MPC_ERR_INVALID_ARG,
                    "mpc_compensate: null params / obs / out / ring / prev / age / pring / counts / sums pointer");
    if (reset == 0 && !command)
        return fail(MPC_ERR_INVALID_ARG, "mpc_compensate: null command pointer in a launch without reset");
    if (out == obs) return fail(MPC_ERR_INVALID_ARG, "mpc_compensate: out must not be obs");
    if (params->struct_size != (int32_t)sizeof(mpc_compensator))
        return fail(MPC_ERR_INVALID_ARG, "mpc_compensate: mpc_compensator.struct_size mismatch");
    const mpc_compensator &p = *params;
    const comp::Params P{p.dt, {p.alpha[0], p.alpha[1]}, {p.rate[0], p.rate[1]}, {p.lo[0], p.lo[1]}, {p.hi[0], p.hi[1]}, p.steps};
    if (const char *why = comp::refusal(P))
        return fail(MPC_ERR_INVALID_ARG, std::string("mpc_compensate: bad parameter (") + why + ")");
    if (B == 0) return MPC_OK;
    HIP_TRY(hipSetDevice(device));
    const comp::Buffers buf{(int)B, (int)R, obs, command, done, out, pred, ring, prev, age, pring, counts, sums};
    hipLaunchKernelGGL(mpc_compensate_kernel<false>, dim3((unsigned)((B + 3) / 4)), dim3(64), 0,
                       reinterpret_cast<hipStream_t>(stream_), P, buf, (int)reset);
    HIP_TRY(hipGetLastError());
    return MPC_OK;
}

int mpc_compensate_stale(int32_t device, int32_t B, int32_t R, int32_t reset, const mpc_compensator *params, int32_t latency,
                         const float *obs, const double *command, const uint8_t *done, float *out, double *pred, double *ring,
                         double *prev, int32_t *age, double *pring, int64_t *counts, double *sums, void *stream_) {
    namespace comp = mpc::comp;
    if (B < 0 || R < 1 || R > comp::kMaxRows)
        return fail(MPC_ERR_INVALID_ARG, "mpc_compensate_stale: bad size (B >= 0, 1 <= R <= 17)");
    if (!params || !obs || !out || !ring || !prev || !age || !pring || !counts || !sums)
        return fail(MPC_ERR_INVALID_ARG,
                    "mpc_compensate_stale: null params / obs / out / ring / prev / age / pring / counts / sums pointer");
    if (reset == 0 && !command)
        return fail(MPC_ERR_INVALID_ARG, "mpc_compensate_stale: null command pointer in a launch without reset");
    if (out == obs) return fail(MPC_ERR_INVALID_ARG, "mpc_compensate_stale: out must not be obs");
    if (params->struct_size != (int32_t)sizeof(mpc_compensator))
        return fail(MPC_ERR_INVALID_ARG, "mpc_compensate_stale: mpc_compensator.struct_size mismatch");
    const mpc_compensator &p = *params;
    const comp::Params P{p.dt, {p.alpha[0], p.alpha[1]}, {p.rate[0], p.rate[1]}, {p.lo[0], p.lo[1]}, {p.hi[0], p.hi[1]}, p.steps,
                         latency};
    if (const char *why = comp::refusal(P))
        return fail(MPC_ERR_INVALID_ARG, std::string("mpc_compensate_stale: bad parameter (") + why + ")");
    if (B == 0) return MPC_OK;
    HIP_TRY(hipSetDevice(device));
    const comp::Buffers buf{(int)B, (int)R, obs, command, done, out, pred, ring, prev, age, pring, counts, sums};
    hipLaunchKernelGGL(mpc_compensate_kernel<true>, dim3((unsigned)((B + 3) / 4)), dim3(64), 0,
                       reinterpret_cast<hipStream_t>(stream_), P, buf, (int)reset);
    HIP_TRY(hipGetLastError());
    return MPC_OK;
}

int mpc_delay_scene(int32_t device, int32_t B, int32_t R, int32_t reset, int32_t steps, const float *obs, const uint8_t *done,
                    float *out, int32_t *stale, float *frames, int32_t *age, int64_t *counts, double *sums, void *stream_) {
    namespace lat = mpc::lat;
    if (const char *why = lat::refusal((int)B, (int)R, (int)steps))
        return fail(MPC_ERR_INVALID_ARG, std::string("mpc_delay_scene: bad argument (") + why + ")");
    if (!obs || !out || !frames || !age || !counts || !sums)
        return fail(MPC_ERR_INVALID_ARG, "mpc_delay_scene: null obs / out / frames / age / counts / sums pointer");
    if (out == obs) return fail(MPC_ERR_INVALID_ARG, "mpc_delay_scene: out must not be obs");
    if (B == 0) return MPC_OK;
    HIP_TRY(hipSetDevice(device));
    const lat::Buffers buf{(int)B, (int)R, obs, done, out, stale, frames, age, counts, sums};
    hipLaunchKernelGGL(mpc_delay_scene_kernel, dim3((unsigned)((B + 3) / 4)), dim3(64), 0,
                       reinterpret_cast<hipStream_t>(stream_), buf, (int)steps, (int)reset);
    HIP_TRY(hipGetLastError());
    return MPC_OK;
}

int mpc_plan_metrics(int32_t device, int32_t B, int32_t N, int32_t R, int32_t Q, int32_t reset, int32_t order, double dt,
                     double gap, int32_t lead0, int32_t lead1, int32_t lead2, int32_t lead3, const double *plan_X,
                     const double *plan_U, const int32_t *status, const float *acted, const float *terminal_obs,
                     const uint8_t *done, int32_t *state_i32, double *state_f64, double *ring_xy, int32_t *ring_valid,
                     int32_t *rec_i32, double *rec_f64, void *stream_) {
    namespace plan = mpc::plan;
    const int32_t leads[plan::kLeads] = {lead0, lead1, lead2, lead3};
    if (const char *why = plan::refusal(B, N, R, Q, order, dt, gap, leads))
        return fail(MPC_ERR_INVALID_ARG, std::string("mpc_plan_metrics: bad argument (") + why + ")");
    if (!state_i32 || !state_f64 || !ring_xy || !ring_valid || !rec_i32 || !rec_f64)
        return fail(MPC_ERR_INVALID_ARG, "mpc_plan_metrics: null state / ring / record pointer");
    if (!reset && (!plan_X || !plan_U || !status || !acted || !terminal_obs || !done))
        return fail(MPC_ERR_INVALID_ARG, "mpc_plan_metrics: null step-input pointer of a non-reset launch");
    if (B == 0) return MPC_OK;
    HIP_TRY(hipSetDevice(device));
    const plan::Accounts acc{(int)B, (int)Q, plan::max_lead(leads), state_i32, state_f64, ring_xy, ring_valid, rec_i32, rec_f64};
    const plan::StepInputs in{(int)N, (int)R, (int)order, dt, gap, {lead0, lead1, lead2, lead3}, plan_X, plan_U, status, acted,
                              terminal_obs, done};
    hipLaunchKernelGGL(mpc_plan_metrics_kernel, dim3((unsigned)((B + 3) / 4)), dim3(64), 0,
                       reinterpret_cast<hipStream_t>(stream_), acc, in, (int)reset);
    HIP_TRY(hipGetLastError());
    return MPC_OK;
}

int mpc_plan_trace(int32_t device, int32_t B, int32_t N, int32_t Q, int32_t W, int32_t C, int32_t reset, const double *plan_X,
                   const double *plan_U, const uint8_t *done, const int32_t *slot, int32_t *state_i32, double *ring_X,
                   double *ring_U, double *kept_X, double *kept_U, void *stream_) {
    namespace plan = mpc::plan;
    if (B < 0 || N < 1 || N > MPC_MAX_HORIZON || Q < 1 || W < 1 || W > mpc::trace::kMaxWindow || C < 1)
        return fail(MPC_ERR_INVALID_ARG, "mpc_plan_trace: bad size (B >= 0, 1 <= N <= 64, Q >= 1, 1 <= W <= 4096, C >= 1)");
    if (!state_i32 || !ring_X || !ring_U || !kept_X || !kept_U)
        return fail(MPC_ERR_INVALID_ARG, "mpc_plan_trace: null state / ring / store pointer");
    if (!reset && (!plan_X || !plan_U || !done || !slot))
        return fail(MPC_ERR_INVALID_ARG, "mpc_plan_trace: null step-input pointer of a non-reset launch");
    if (B == 0) return MPC_OK;
    HIP_TRY(hipSetDevice(device));
    const plan::TraceStore store{(int)B, (int)N, (int)Q, (int)W, (int)C, state_i32, ring_X, ring_U, kept_X, kept_U};
    const plan::TraceInputs in{plan_X, plan_U, done, slot};
    hipLaunchKernelGGL(mpc_plan_trace_kernel, dim3((unsigned)B), dim3(kTraceFrameThreads), 0,
                       reinterpret_cast<hipStream_t>(stream_), store, in, (int)reset);
    HIP_TRY(hipGetLastError());
    return MPC_OK;
}

int mpc_eval_nlp(mpc_handle *h, int32_t B, const int32_t *ego_index, const double *vref, const double *weights,
                 const uint8_t *is_collide, const double *others, int32_t V, uint32_t flags, const double *X, const double *U,
                 double *f, double *x_next) {
    if (!h) return fail(MPC_ERR_INVALID_ARG, "mpc_eval_nlp: null handle");
    if (B < 0 || !ego_index || !weights || !is_collide || !X || !U || !f || !x_next)
        return fail(MPC_ERR_INVALID_ARG, "mpc_eval_nlp: null required pointer or negative batch");
    if (V < 0 || V > MPC_MAX_OTHERS) return fail(MPC_ERR_INVALID_ARG, "mpc_eval_nlp: V out of range");
    const bool cc = (flags & MPC_FLAG_COLLISION_COST) != 0;
    if (flags & ~(uint32_t)MPC_FLAG_COLLISION_COST) return fail(MPC_ERR_INVALID_ARG, "mpc_eval_nlp: only MPC_FLAG_COLLISION_COST (host pointers, synchronous)");
    if (cc && V > 0 && !others) return fail(MPC_ERR_INVALID_ARG, "mpc_eval_nlp: collision cost needs `others`");
    if (!h->d_ref) return fail(MPC_ERR_NO_REFERENCE, "mpc_eval_nlp: call mpc_set_reference first");
    if (B == 0) return MPC_OK;
    HIP_TRY(hipSetDevice(h->device));
    const int N = h->cfg.horizon;
    const size_t N1 = (size_t)N + 1;
    hipStream_t stream = nullptr;
    Staging st(h, stream, false);                  // host pointers only, on the null stream
    const auto s_ego = st.in(ego_index, (size_t)B * 4);
    const auto s_w = st.in(weights, (size_t)B * 3 * 8);
    const auto s_c = st.in(is_collide, (size_t)B);
    const auto s_vref = st.in(vref, (size_t)B * N1 * 8);                                     // optional
    const auto s_oth = st.in(cc && V > 0 ? others : nullptr, (size_t)B * V * 4 * 8);
    const auto s_X = st.in(X, (size_t)B * N1 * 4 * 8);
    const auto s_U = st.in(U, (size_t)B * N * 2 * 8);
    const auto s_f = st.out(f, (size_t)B * 8);
    const auto s_xn = st.out(x_next, (size_t)B * N * 4 * 8);
    if (int rc = st.commit()) return rc;
    mpc::SolveParams P = solve_params(h, cc ? V : 0);
    const size_t lds = (size_t)mpc::wave::lds_doubles(cc, N, P.V) * sizeof(double);
    auto kern = cc ? mpc_eval_kernel<true> : mpc_eval_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(kBlock), lds, stream, P, (int)B, h->d_ref.p, h->M, st.ptr(s_ego),
                       st.ptr(s_vref), st.ptr(s_w), st.ptr(s_c), st.ptr(s_oth), cc ? (int)V : 0, h->cfg.w_collision,
                       st.ptr(s_X), st.ptr(s_U), st.ptr(s_f), st.ptr(s_xn));
    HIP_TRY(hipGetLastError());
    return st.finish(0);
}

int mpc_set_diagnostics(mpc_handle *h, int32_t on) {
    if (!h) return fail(MPC_ERR_INVALID_ARG, "mpc_set_diagnostics: null handle");
    h->diag = on != 0;
    if (!h->diag) h->diag_B = 0;
    return MPC_OK;
}

int mpc_get_last_paths(mpc_handle *h, int32_t B, double *ego_path, int32_t *ego_len, float *agent_paths) {
    if (!h || B < 0) return fail(MPC_ERR_INVALID_ARG, "mpc_get_last_paths: bad argument");
    if (B == 0) return MPC_OK;
    if (!h->diag || !h->diag_buf || B > h->diag_B)
        return fail(MPC_ERR_INVALID_ARG, "mpc_get_last_paths: no diagnostics of that size (mpc_set_diagnostics, then mpc_predict_batch)");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t P = mpc::pre::kPredHorizon + 1;
    if (ego_path) HIP_TRY(hipMemcpy(ego_path, h->g_ego, (size_t)B * P * 2 * 8, hipMemcpyDeviceToHost));
    if (ego_len) HIP_TRY(hipMemcpy(ego_len, h->g_len, (size_t)B * 4, hipMemcpyDeviceToHost));
    if (agent_paths) HIP_TRY(hipMemcpy(agent_paths, h->g_agents, (size_t)B * h->diag_V * P * 2 * 4, hipMemcpyDeviceToHost));
    return MPC_OK;
}

int mpc_get_last_inputs(mpc_handle *h, int32_t B, double *state, int32_t *ego_index, double *vref,
                        uint8_t *is_collide, double *others, int32_t *nveh) {
    if (!h || B < 0) return fail(MPC_ERR_INVALID_ARG, "mpc_get_last_inputs: bad argument");
    if (B == 0) return MPC_OK;
    if (!h->pre || B > h->pre_B) return fail(MPC_ERR_INVALID_ARG, "mpc_get_last_inputs: no preamble output of that size");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t N1 = (size_t)h->cfg.horizon + 1, V = (size_t)(h->pre_V > 0 ? h->pre_V : 1);
    if (state) HIP_TRY(hipMemcpy(state, h->p_state, (size_t)B * 4 * 8, hipMemcpyDeviceToHost));
    if (ego_index) HIP_TRY(hipMemcpy(ego_index, h->p_ego, (size_t)B * 4, hipMemcpyDeviceToHost));
    if (vref) HIP_TRY(hipMemcpy(vref, h->p_vref, (size_t)B * N1 * 8, hipMemcpyDeviceToHost));
    if (is_collide) HIP_TRY(hipMemcpy(is_collide, h->p_coll, (size_t)B, hipMemcpyDeviceToHost));
    if (others) HIP_TRY(hipMemcpy(others, h->p_others, (size_t)B * V * 4 * 8, hipMemcpyDeviceToHost));
    if (nveh) HIP_TRY(hipMemcpy(nveh, h->p_nveh, (size_t)B * 4, hipMemcpyDeviceToHost));
    return MPC_OK;
}

int mpc_get_launch_order(mpc_handle *h, int32_t B, int32_t *order, int32_t *tier) {
    if (!h || B < 0) return fail(MPC_ERR_INVALID_ARG, "mpc_get_launch_order: bad argument");
    if (B == 0) return MPC_OK;
    if (!h->d_order || B > h->order_cap) return fail(MPC_ERR_INVALID_ARG, "mpc_get_launch_order: no launch order of that size");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    if (order) HIP_TRY(hipMemcpy(order, h->d_order, (size_t)B * 4, hipMemcpyDeviceToHost));
    if (tier) HIP_TRY(hipMemcpy(tier, h->d_order + h->order_cap, (size_t)B * 4, hipMemcpyDeviceToHost));
    return MPC_OK;
}

}  // extern "C"
