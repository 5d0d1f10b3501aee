// Stand-alone program for a sanitizer run of the host builds of csrc/mpc_latency.hpp and of the latency-aware build of
// csrc/mpc_compensate.hpp (tests/test_latency_cpu.py compiles it with -fsanitize=address,undefined and runs it as a child
// process; nothing is loaded into Python).  The true scenes of a small batch go through the latency stage and from there into
// the compensator, 25 launches per setting from a simple LCG, in exactly sized heap buffers so that any access past a row, a
// ring slot, a frame or a batch is reported: every latency 0..7 on its own, every (look-ahead, latency) with a sum of at most
// 7, done on some launches (also on consecutive ones) and NULL on others, stale and pred on some launches and NULL on others, a
// reset launch in the middle, one NaN command.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "cpu_latency_harness.cpp"

namespace {

const double inf = std::numeric_limits<double>::infinity();
uint64_t g_state = 0x853C49E6748FEA9Bull;

double lcg() {          // [0, 1)
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) * (1.0 / 9007199254740992.0);
}

// d < 0: the latency stage alone
int run(int B, int R, int d, int L, const double *par) {
    const size_t scene = (size_t)B * R * 8;
    std::vector<float> obs(scene), late(scene), out(scene), frames((size_t)8 * scene);
    std::vector<std::vector<float>> history;
    std::vector<double> command((size_t)B * 2), pred((size_t)B * 4), ring((size_t)8 * B * 2), prev((size_t)B * 2),
        pring((size_t)8 * B * 2), sums((size_t)2 * B), lsums((size_t)3 * B);
    std::vector<uint8_t> done((size_t)B);
    std::vector<int32_t> age((size_t)B), lage((size_t)B), stale((size_t)B), first((size_t)B);
    std::vector<int64_t> counts((size_t)B), lcounts((size_t)B);
    for (int launch = 0; launch < 25; ++launch) {
        const bool reset = launch == 0 || launch == 12;
        for (int b = 0; b < B; ++b) {
            float *e = obs.data() + (size_t)b * R * 8;
            const double th = 6.0 * lcg() - 3.0, sp = 30.0 * lcg();
            e[0] = 1.0f, e[1] = (float)(100.0 * lcg() - 50.0), e[2] = (float)(100.0 * lcg() - 50.0);
            e[3] = (float)(sp * std::cos(th)), e[4] = (float)(sp * std::sin(th));
            e[5] = (float)th, e[6] = (float)std::sin(th), e[7] = (float)std::cos(th);
            for (int i = 1; i < R; ++i) {
                float *r = e + i * 8;
                r[0] = lcg() < 0.7 ? 1.0f : 0.0f;
                for (int c = 1; c < 8; ++c) r[c] = (float)(120.0 * lcg() - 60.0);
            }
            done[b] = (launch % 7 == 3 && b % 2 == 0) || (launch % 7 == 4 && b % 2 == 0) || (launch % 5 == 4 && b % 3 == 1) ? 1 : 0;
            command[(size_t)b * 2] = 16.0 * lcg() - 8.0;
            command[(size_t)b * 2 + 1] = 3.0 * lcg() - 1.5;
        }
        if (launch == 5) command[(size_t)(B - 1) * 2] = std::nan("");
        const bool with_done = !(reset || launch % 4 == 0);
        history.push_back(obs);
        for (size_t k = 0; k < scene; ++k) late[k] = out[k] = std::nanf("");
        int rc = latency_step(B, R, reset ? 1 : 0, L, obs.data(), with_done ? done.data() : nullptr, late.data(),
                              launch % 3 == 2 ? nullptr : stale.data(), frames.data(), lage.data(), lcounts.data(), lsums.data());
        if (rc != 0) return 1;
        for (int b = 0; b < B; ++b) {
            if (reset || (with_done && done[b])) first[b] = launch;
            const int s = launch - first[b] < L ? launch - first[b] : L;
            if (launch % 3 != 2 && stale[b] != s) return 2;
            if (lage[b] != launch - first[b] + 1) return 3;
            const float *want = history[(size_t)(launch - s)].data() + (size_t)b * R * 8;      // never older than the episode
            if (std::memcmp(late.data() + (size_t)b * R * 8, want, (size_t)R * 8 * sizeof(float)) != 0) return 4;
        }
        if (d < 0) continue;
        rc = compensate_stale_step(B, R, reset ? 1 : 0, par, d, L, late.data(), reset ? nullptr : command.data(),
                                   with_done ? done.data() : nullptr, out.data(), launch % 3 == 1 ? nullptr : pred.data(),
                                   ring.data(), prev.data(), age.data(), pring.data(), counts.data(), sums.data());
        if (rc != 0) return 5;
        for (int b = 0; b < B; ++b) {
            if (age[b] != launch - first[b] || counts[b] < 0 || counts[b] > launch) return 6;
            int present_in = 0, present_out = 0;
            for (int i = 1; i < R; ++i) {
                present_in += late[((size_t)b * R + i) * 8] != 0.0f;
                present_out += out[((size_t)b * R + i) * 8] != 0.0f;
            }
            if (present_in != present_out) return 7;
            for (int k = 0; k < R * 8; ++k)
                if (!(out[(size_t)b * R * 8 + k] == out[(size_t)b * R * 8 + k])) return 8;       // every element written, no NaN
            for (int c = 0; c < 2; ++c) {
                const double y = prev[(size_t)b * 2 + c];
                if (!(y >= par[5 + c] && y <= par[7 + c])) return 9;                              // the nominal limits hold
            }
        }
    }
    return 0;
}

}  // namespace

int main() {
    const int sizes[4][2] = {{1, 1}, {5, 2}, {5, 17}, {3, 10}};
    const double off[9] = {0.1, 1, 1, inf, inf, -inf, -inf, inf, inf};
    const double on[9] = {0.1, 0.5, 0.25, 20.0, 2.0, -5.0, -0.785, 5.0, 0.785};
    for (const auto &s : sizes)
        for (int L = 0; L <= 7; ++L)
            for (int d = -1; d + L <= 7; ++d)
                for (const double *par : {off, on}) {
                    const int rc = run(s[0], s[1], d, L, par);
                    if (rc != 0) {
                        std::printf("latency_san_main: B=%d R=%d steps=%d latency=%d %s failed (%d)\n", s[0], s[1], d, L,
                                    par == on ? "on" : "off", rc);
                        return 1;
                    }
                }
    std::printf("latency_san_main: ok\n");
    return 0;
}
