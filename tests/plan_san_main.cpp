// Stand-alone program for a sanitizer run of the host build of csrc/mpc_plan.hpp (tests/test_plan_cpu.py compiles it with
// -fsanitize=address,undefined and runs it as a child process; nothing is loaded into Python): the shapes of the CPU test,
// 30 launches per shape from a simple LCG with a reset launch (NULL step inputs) in the middle, exactly sized heap buffers so
// that any access past a stage, a row, a ring entry, a record slot or a batch is reported, episodes that end at every age
// from 1 on, invalid plans among them, absent rows, a quota the environments pass, and the plan trace driven by slots of -1,
// of the store's range and beyond it.
#include <cstdio>
#include <vector>

#include "cpu_plan_harness.cpp"

namespace {

uint64_t g_state = 0x853C49E6748FEA9Bull;

double lcg() {          // [0, 1)
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) * (1.0 / 9007199254740992.0);
}

int run(int B, int N, int R, const int32_t *leads) {
    const int Q = 2, W = 3, C = 2;
    int Lmax = 0;
    for (int i = 0; i < 4; ++i) Lmax = leads[i] > Lmax ? leads[i] : Lmax;
    std::vector<double> X((size_t)B * (N + 1) * 4), U((size_t)B * N * 2), sf((size_t)15 * B), ring((size_t)B * Lmax * 8),
        rf((size_t)13 * B * Q), ring_X((size_t)B * W * (N + 1) * 4), ring_U((size_t)B * W * N * 2),
        kept_X((size_t)C * W * (N + 1) * 4), kept_U((size_t)C * W * N * 2);
    std::vector<float> acted((size_t)B * R * 8), terminal((size_t)B * R * 8);
    std::vector<int32_t> status((size_t)B), si((size_t)10 * B), ring_valid((size_t)B * Lmax), ri((size_t)8 * B * Q), slot((size_t)B),
        ti((size_t)2 * B);
    std::vector<uint8_t> done((size_t)B);
    const char *why = nullptr;
    for (int step = 0; step < 30; ++step) {
        if (step == 0 || step == 14) {
            if (plan_metrics_step(B, N, R, Q, 1, step ? 1 : 0, 0.1, 2.5, leads, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                  si.data(), sf.data(), ring.data(), ring_valid.data(), ri.data(), rf.data(), &why) != 0)
                return 1;
            if (plan_trace_step(B, N, Q, W, C, 1, nullptr, nullptr, nullptr, nullptr, ti.data(), ring_X.data(), ring_U.data(),
                                kept_X.data(), kept_U.data()) != 0)
                return 2;
        }
        for (auto &v : X) v = 40.0 * lcg() - 20.0;
        for (auto &v : U) v = 2.0 * lcg() - 1.0;
        for (auto &v : acted) v = (float)(20.0 * lcg() - 10.0);
        for (auto &v : terminal) v = (float)(20.0 * lcg() - 10.0);
        for (int b = 0; b < B; ++b) {
            for (int j = 0; j < R; ++j) acted[((size_t)b * R + j) * 8] = lcg() < 0.25 ? 0.0f : 1.0f;
            status[b] = lcg() < 0.2 ? 1 + (step + b) % 4 : (step % 2 ? 0 : 5 + b % 3);
            done[b] = (step + b) % (1 + b % 5) == 0 ? 1 : 0;         // environment 0 ends every step, 4 every fifth
            slot[b] = done[b] ? (step + b) % (C + 2) - 1 : -1;       // -1, 0 .. C - 1, and C: past the store
        }
        if (plan_metrics_step(B, N, R, Q, 0, step % 2, 0.1, 2.5, leads, X.data(), U.data(), status.data(), acted.data(),
                              terminal.data(), done.data(), si.data(), sf.data(), ring.data(), ring_valid.data(), ri.data(),
                              rf.data(), &why) != 0)
            return 3;
        if (plan_trace_step(B, N, Q, W, C, 0, X.data(), U.data(), done.data(), slot.data(), ti.data(), ring_X.data(),
                            ring_U.data(), kept_X.data(), kept_U.data()) != 0)
            return 4;
        for (int b = 0; b < B; ++b) {
            if (si[(size_t)4 * B + b] < 0 || si[(size_t)4 * B + b] > Q || ti[(size_t)B + b] < 0) return 5;   // the ordinals
            if (!(sf[b] >= 0.0)) return 6;                                                                 // min_plan_gap, never NaN
        }
    }
    return 0;
}

}  // namespace

int main() {
    const int sizes[3] = {1, 5, 33}, horizons[3] = {1, 2, 20}, rows[4] = {1, 2, 10, 17};
    const int32_t first[4] = {1, 0, 0, 0}, spread[4] = {1, 5, 10, 20};
    for (int B : sizes)
        for (int N : horizons)
            for (int R : rows)
                for (int set = 0; set < (N == 20 ? 2 : 1); ++set) {
                    const int rc = run(B, N, R, set ? spread : first);
                    if (rc != 0) {
                        std::printf("plan_san_main: B=%d N=%d R=%d leads=%d failed (%d)\n", B, N, R, set, rc);
                        return 1;
                    }
                }
    std::printf("plan_san_main: ok\n");
    return 0;
}
