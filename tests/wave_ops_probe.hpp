// TEST INFRASTRUCTURE - every primitive of the CTX interface of mpc-rl_for_avs_amd/csrc/mpc_wave.hpp, one at a time, written
// once against that interface the way the solver is: tests/dev_wave_ops.hip runs it on mpc::wave::WaveOpsT<RELAX> (one wave
// per input set), tests/cpu_wave_ops_harness.cpp on HostCtx (tests/host_wave_ctx.hpp).  tests/test_wave_ops_gpu.py compares the
// two bit for bit; tests/wave_ops_cases.py states every result once more in plain numpy.  Never loaded by the product.
//
// An input set is kIn[OP] rows of 64 doubles, a result kOut[OP] rows of 64 doubles (every lane's value; integers travel as
// doubles, which hold them exactly).  No operation here multiplies and adds in one expression: the device build contracts
// such an expression into a fused multiply-add and the host build (-ffp-contract=off) does not.
#pragma once

#include "../mpc-rl_for_avs_amd/csrc/mpc_wave.hpp"

namespace probe {

enum : int {
    OP_MFMA = 0,      // a, b, c -> c + a x b (four 4x4x4 blocks)
    OP_LANE_GET,      // p, (lane index in word 0) -> p of lanes 0, 5, 16, 31, 32, 47, 63 and of the given lane
    OP_ROW_BCAST,     // p -> row_bcast<0..15>
    OP_ROW_BCAST2,    // p -> row_bcast2<0..7>
    OP_IDENT,         // p, (uniform value in word 0), integers -> uni, fresh, keep, hide, opaque, opaque_shared
    OP_BIT_SELECT,    // masks (0 / -1), a, b -> bit_select with the mask plain and behind hide()
    OP_BCAST_BALLOT,  // integers, (lane index in word 0) -> wave_bcast of lanes 0, 21, 63 and the given one, ballot low / high half
    OP_REDUCE,        // p -> wave_sum, wave_max, wave_min
    OP_SUFFIX_SUM,    // p -> wave_suffix_sum
    OP_SUM2,          // p -> wave_sum2 lo, hi
    OP_MAX_RATIO,     // n, d -> wave_max_ratio n, d
    OP_LDS_ROUNDS,    // p -> eight dependent store / phase / load-another-lane's-word / phase rounds
    OP_COUNT
};
constexpr int kRounds = 8;
constexpr int kIn[OP_COUNT] = {3, 2, 1, 1, 3, 3, 2, 1, 1, 1, 2, 1};
constexpr int kOut[OP_COUNT] = {1, 8, 16, 8, 6, 2, 6, 3, 1, 2, 2, 1};
constexpr int kL = mpc::wave::kLanes;

template <int J, class CTX>
MPC_HD void bcast_all(CTX &c, mpc::wave::PerLane<double> &P, double *out) {
    mpc::wave::PerLane<double> D;
    c.template row_bcast<J>(D, P);
    c.lanes([&](int lane) { out[J * kL + lane] = D.at(lane); });
    if constexpr (J + 1 < 16) bcast_all<J + 1>(c, P, out);
}
template <int J, class CTX>
MPC_HD void bcast2_all(CTX &c, mpc::wave::PerLane<double> &P, double *out) {
    mpc::wave::PerLane<double> D;
    c.template row_bcast2<J>(D, P);
    c.lanes([&](int lane) { out[J * kL + lane] = D.at(lane); });
    if constexpr (J + 1 < 8) bcast2_all<J + 1>(c, P, out);
}

// in: kIn[OP] x 64 doubles of one set, out: kOut[OP] x 64.  c.L: at least 64 words.
template <int OP, class CTX>
MPC_HD void wave_op(CTX &c, const double *in, double *out) {
    using mpc::wave::PerLane;
    auto load = [&](PerLane<double> &P, int row) { c.lanes([&](int lane) { P.at(lane) = in[row * kL + lane]; }); };
    auto loadi = [&](PerLane<int> &P, int row) { c.lanes([&](int lane) { P.at(lane) = (int)in[row * kL + lane]; }); };
    auto all = [&](int row, double v) { c.lanes([&](int lane) { out[row * kL + lane] = v; }); };
    if constexpr (OP == OP_MFMA) {
        PerLane<double> A, B, C;
        load(A, 0);
        load(B, 1);
        load(C, 2);
        c.mfma(A, B, C);
        c.lanes([&](int lane) { out[lane] = C.at(lane); });
    } else if constexpr (OP == OP_LANE_GET) {
        PerLane<double> P;
        load(P, 0);
        const int given = (int)in[kL];
        all(0, c.lane_get(P, 0));
        all(1, c.lane_get(P, 5));
        all(2, c.lane_get(P, 16));
        all(3, c.lane_get(P, 31));
        all(4, c.lane_get(P, 32));
        all(5, c.lane_get(P, 47));
        all(6, c.lane_get(P, 63));
        all(7, c.lane_get(P, given));
    } else if constexpr (OP == OP_ROW_BCAST) {
        PerLane<double> P;
        load(P, 0);
        bcast_all<0>(c, P, out);
    } else if constexpr (OP == OP_ROW_BCAST2) {
        PerLane<double> P;
        load(P, 0);
        bcast2_all<0>(c, P, out);
    } else if constexpr (OP == OP_IDENT) {
        PerLane<double> P;
        PerLane<int> Q;
        load(P, 0);
        loadi(Q, 2);
        const double u = in[kL];
        c.template set_priority<1>();
        all(0, c.uni(u));
        c.sched_fence();
        all(1, c.fresh(u));
        c.template set_priority<0>();
        c.lanes([&](int lane) {
            out[2 * kL + lane] = c.keep(P.at(lane));
            out[3 * kL + lane] = (double)c.hide(Q.at(lane));
            out[4 * kL + lane] = (double)c.opaque(Q.at(lane));
            out[5 * kL + lane] = (double)c.opaque_shared(Q.at(lane));
        });
    } else if constexpr (OP == OP_BIT_SELECT) {
        PerLane<int> M;
        PerLane<double> A, B;
        loadi(M, 0);
        load(A, 1);
        load(B, 2);
        c.lanes([&](int lane) {
            out[lane] = c.bit_select(M.at(lane), A.at(lane), B.at(lane));
            out[kL + lane] = c.bit_select(c.hide(M.at(lane)), A.at(lane), B.at(lane));
        });
    } else if constexpr (OP == OP_BCAST_BALLOT) {
        PerLane<int> Q;
        loadi(Q, 0);
        const int given = (int)in[kL];
        all(0, (double)c.wave_bcast(Q, 0));
        all(1, (double)c.wave_bcast(Q, 21));
        all(2, (double)c.wave_bcast(Q, 63));
        all(3, (double)c.wave_bcast(Q, given));
        const unsigned long long m = c.ballot(Q);
        all(4, (double)(unsigned)(m & 0xffffffffull));
        all(5, (double)(unsigned)(m >> 32));
    } else if constexpr (OP == OP_REDUCE) {
        PerLane<double> P;          // (the host model reduces in place: loaded again for every reduction)
        load(P, 0);
        all(0, c.wave_sum(P));
        load(P, 0);
        all(1, c.wave_max(P));
        load(P, 0);
        all(2, c.wave_min(P));
    } else if constexpr (OP == OP_SUFFIX_SUM) {
        PerLane<double> P;
        load(P, 0);
        c.wave_suffix_sum(P);
        c.lanes([&](int lane) { out[lane] = P.at(lane); });
    } else if constexpr (OP == OP_SUM2) {
        PerLane<double> P;
        load(P, 0);
        double lo, hi;
        c.wave_sum2(P, lo, hi);
        all(0, lo);
        all(1, hi);
    } else if constexpr (OP == OP_MAX_RATIO) {
        PerLane<double> N, D;
        load(N, 0);
        load(D, 1);
        double rn, rd;
        c.wave_max_ratio(N, D, rn, rd);
        all(0, rn);
        all(1, rd);
    } else if constexpr (OP == OP_LDS_ROUNDS) {
        // round r: every lane stores its value to its own word; the phase ends; every lane adds another lane's word to its value
        // (63 - lane in even rounds, lane ^ 17 in odd ones); the phase ends, and the next round overwrites the words.  A load
        // moved above the end of the storing phase reads the previous round's word, a store moved above the end of the loading
        // phase overwrites a word another lane has yet to read: either changes the sums.
        PerLane<double> V;
        load(V, 0);
        for (int r = 0; r < kRounds; ++r) {
            c.phase([&](int lane) { c.st(lane, V.at(lane)); });
            c.phase([&](int lane) { V.at(lane) = V.at(lane) + c.ld((r & 1) ? (lane ^ 17) : (kL - 1 - lane)); });
        }
        c.lanes([&](int lane) { out[lane] = V.at(lane); });
    }
}

// ---- lean FP64 math of mpc_core.hpp, one point per call: fn, inputs x[0..1] -> outputs y[0..3] -------------------------
enum : int { FN_RCP = 0, FN_RSQ, FN_FRCP, FN_FRSQRT, FN_SINCOS_HALF, FN_SINCOS_DELTA_THETA, FN_ATAN_B, FN_LOG_POS, FN_DYN_EVAL, FN_COUNT };
constexpr int kFnIn[FN_COUNT] = {1, 1, 1, 1, 1, 2, 1, 1, 2};
constexpr int kFnOut[FN_COUNT] = {1, 1, 1, 1, 2, 4, 1, 1, 4};

}  // namespace probe
