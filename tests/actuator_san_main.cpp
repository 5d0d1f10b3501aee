// Stand-alone program for a sanitizer run of the host build of csrc/mpc_actuator.hpp (tests/test_actuator_cpu.py compiles it
// with -fsanitize=address,undefined and runs it as a child process; nothing is loaded into Python): the shapes of the CPU
// test, 25 commands per environment from a simple LCG with +-0.0, values beyond the limits, one NaN and one inf among them,
// exactly sized heap buffers so that any access past a channel, a plane or a batch is reported, every feature alone and all
// together, done_prev on some launches and NULL on others, a reset launch with NULL command and applied in the middle, and
// applied aliasing command on every third launch.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "cpu_actuator_harness.cpp"

namespace {

const double inf = std::numeric_limits<double>::infinity();
uint64_t g_state = 0x853C49E6748FEA9Bull;

double lcg() {          // [0, 1)
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) * (1.0 / 9007199254740992.0);
}

struct Set {
    int delay;
    double par[16];     // dt, p_hold, gain, offset, sigma, alpha, rate, lo, hi
};

int run(int B, const Set &q) {
    std::vector<double> command((size_t)B * 2), applied((size_t)B * 2), state((size_t)10 * B * 2), sums((size_t)2 * B * 2);
    std::vector<uint8_t> done((size_t)B);
    std::vector<int32_t> age((size_t)B);
    std::vector<int64_t> ctr((size_t)B), counts((size_t)5 * B);
    if (actuator_step(B, 1, q.par, 7, q.delay, 3, nullptr, nullptr, nullptr, state.data(), age.data(), ctr.data(),
                      counts.data(), sums.data()) != 0)
        return 1;
    int64_t launches = 0;
    for (int step = 0; step < 25; ++step) {
        if (step == 12) {
            if (actuator_step(B, 1, q.par, 7, q.delay, 3, nullptr, nullptr, nullptr, state.data(), age.data(), ctr.data(),
                              counts.data(), sums.data()) != 0)
                return 2;
            launches = 0;
        }
        for (int b = 0; b < B; ++b) {
            done[b] = (step % 7 == 3 && b % 2 == 0) || (step % 5 == 4 && b % 3 == 1) ? 1 : 0;
            for (int c = 0; c < 2; ++c) command[(size_t)b * 2 + c] = 16.0 * lcg() - 8.0;
        }
        if (step == 2) command[0] = -0.0, command[1] = 0.0;
        if (step == 5) command[(size_t)(B - 1) * 2] = std::nan("");
        if (step == 9) command[(size_t)(B - 1) * 2 + 1] = -inf;
        const bool alias = step % 3 == 2;
        double *out = alias ? command.data() : applied.data();
        if (actuator_step(B, 0, q.par, 7, q.delay, 3, command.data(), step % 4 ? done.data() : nullptr, out, state.data(),
                          age.data(), ctr.data(), counts.data(), sums.data()) != 0)
            return 3;
        launches += 1;
        for (int b = 0; b < B; ++b) {
            if (counts[b] != launches || ctr[b] != launches || age[b] < 1 || age[b] > launches) return 4;
            for (int c = 0; c < 2; ++c) {
                const double y = out[(size_t)b * 2 + c];
                if (!(y >= q.par[12 + c] && y <= q.par[14 + c])) return 5;                  // finite limits hold, NaN never
                if (y != state[((size_t)9 * B + b) * 2 + c]) return 6;                      // prev is what was applied
            }
        }
    }
    return 0;
}

}  // namespace

int main() {
    const int sizes[3] = {1, 5, 33};
    const Set sets[9] = {
        {0, {0.1, 0.0, 1, 1, 0, 0, 0, 0, 1, 1, inf, inf, -inf, -inf, inf, inf}},                  // off
        {3, {0.1, 0.0, 1, 1, 0, 0, 0, 0, 1, 1, inf, inf, -inf, -inf, inf, inf}},                  // delay
        {7, {0.1, 0.3, 1, 1, 0, 0, 0, 0, 1, 1, inf, inf, -inf, -inf, inf, inf}},                  // the longest delay, hold
        {0, {0.1, 0.0, 1.1, 0.9, 0.2, -0.05, 0, 0, 1, 1, inf, inf, -inf, -inf, inf, inf}},        // calibration
        {0, {0.1, 0.0, 1, 1, 0, 0, 0.3, 0.02, 1, 1, inf, inf, -inf, -inf, inf, inf}},             // noise
        {0, {0.1, 0.0, 1, 1, 0, 0, 0, 0, 0.5, 0.25, inf, inf, -inf, -inf, inf, inf}},             // lag
        {0, {0.1, 0.0, 1, 1, 0, 0, 0, 0, 1, 1, 10.0, 1.0, -inf, -inf, inf, inf}},                 // rate limit
        {0, {0.1, 0.0, 1, 1, 0, 0, 0, 0, 1, 1, inf, inf, -5.0, -0.785, 5.0, 0.785}},              // saturation
        {2, {0.1, 0.2, 1.1, 0.9, 0.2, -0.05, 0.3, 0.02, 0.5, 0.25, 10.0, 1.0, -5.0, -0.785, 5.0, 0.785}}};   // all
    for (int B : sizes)
        for (int k = 0; k < 9; ++k) {
            const int rc = run(B, sets[k]);
            if (rc != 0) {
                std::printf("actuator_san_main: B=%d set=%d failed (%d)\n", B, k, rc);
                return 1;
            }
        }
    std::printf("actuator_san_main: ok\n");
    return 0;
}
