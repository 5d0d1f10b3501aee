// Stand-alone program for a sanitizer run of the host build of csrc/mpc_compensate.hpp (tests/test_compensate_cpu.py compiles it
// with -fsanitize=address,undefined and runs it as a child process; nothing is loaded into Python): the shapes of the CPU test
// and a ragged one, 25 launches per setting from a simple LCG - scenes with absent rows between present ones, commands beyond
// the limits, +-0.0, one NaN and one inf among them - in exactly sized heap buffers so that any access past a row, a ring slot
// or a batch is reported; every look-ahead 0..7 with the nominal actuator off and on, done on some launches and NULL on
// others, pred on some launches and NULL on others, a reset launch with NULL command and done in the middle.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "cpu_compensate_harness.cpp"

namespace {

const double inf = std::numeric_limits<double>::infinity();
uint64_t g_state = 0x853C49E6748FEA9Bull;

double lcg() {          // [0, 1)
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) * (1.0 / 9007199254740992.0);
}

int run(int B, int R, int steps, const double *par) {
    std::vector<float> obs((size_t)B * R * 8), out((size_t)B * R * 8);
    std::vector<double> command((size_t)B * 2), pred((size_t)B * 4), ring((size_t)8 * B * 2), prev((size_t)B * 2),
        pring((size_t)8 * B * 2), sums((size_t)2 * B);
    std::vector<uint8_t> done((size_t)B);
    std::vector<int32_t> age((size_t)B);
    std::vector<int64_t> counts((size_t)B);
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
            done[b] = (launch % 7 == 3 && b % 2 == 0) || (launch % 5 == 4 && b % 3 == 1) ? 1 : 0;
            command[(size_t)b * 2] = 16.0 * lcg() - 8.0;
            command[(size_t)b * 2 + 1] = 3.0 * lcg() - 1.5;
        }
        if (launch == 2) command[0] = -0.0, command[1] = 0.0;
        if (launch == 5) command[(size_t)(B - 1) * 2] = std::nan("");
        if (launch == 9) command[(size_t)(B - 1) * 2 + 1] = -inf;
        for (size_t k = 0; k < out.size(); ++k) out[k] = std::nanf("");
        const int rc = compensate_step(B, R, reset ? 1 : 0, par, steps, obs.data(), reset ? nullptr : command.data(),
                                       reset || launch % 4 == 0 ? nullptr : done.data(), out.data(),
                                       launch % 3 == 1 ? nullptr : pred.data(), ring.data(), prev.data(), age.data(),
                                       pring.data(), counts.data(), sums.data());
        if (rc != 0) return 1;
        for (int b = 0; b < B; ++b) {
            if (age[b] < 0 || age[b] > launch || counts[b] < 0 || counts[b] > launch) return 2;
            int present_in = 0, present_out = 0;
            bool gap = false;
            for (int i = 1; i < R; ++i) {
                present_in += obs[((size_t)b * R + i) * 8] != 0.0f;
                const bool here = out[((size_t)b * R + i) * 8] != 0.0f;
                if (steps > 0 && here && gap) return 3;          // present rows are contiguous
                gap = gap || !here;
                present_out += here;
            }
            if (present_in != present_out) return 4;
            for (int k = 0; k < R * 8; ++k)
                if (!(out[(size_t)b * R * 8 + k] == out[(size_t)b * R * 8 + k])) return 5;       // every element written, no NaN
            for (int c = 0; c < 2; ++c) {
                const double y = prev[(size_t)b * 2 + c];
                if (!(y >= par[5 + c] && y <= par[7 + c])) return 6;                              // the nominal limits hold
            }
        }
    }
    return 0;
}

}  // namespace

int main() {
    const int sizes[4][2] = {{1, 1}, {5, 10}, {5, 17}, {7, 2}};
    const double off[9] = {0.1, 1, 1, inf, inf, -inf, -inf, inf, inf};
    const double on[9] = {0.1, 0.5, 0.25, 20.0, 2.0, -5.0, -0.785, 5.0, 0.785};
    for (const auto &s : sizes)
        for (int steps = 0; steps <= 7; ++steps)
            for (const double *par : {off, on}) {
                const int rc = run(s[0], s[1], steps, par);
                if (rc != 0) {
                    std::printf("compensate_san_main: B=%d R=%d steps=%d %s failed (%d)\n", s[0], s[1], steps,
                                par == on ? "on" : "off", rc);
                    return 1;
                }
            }
    std::printf("compensate_san_main: ok\n");
    return 0;
}
