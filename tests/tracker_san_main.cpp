// Stand-alone program for a sanitizer run of the host build of csrc/mpc_tracker.hpp (tests/test_tracker_cpu.py compiles it
// with -fsanitize=address,undefined and runs it as a child process; nothing is loaded into Python): the shapes of the CPU
// test, vehicles at constant velocity with jumps from a simple LCG, rows randomly absent, exactly sized heap buffers so that
// any access past a row, a slot or a batch is reported, every parameter set, a reset launch in the middle, done on some
// launches, with and without done, row_slot and row_miss, and at R = 17 sixteen tracks met by sixteen far measurements.
#include <cstdio>
#include <limits>
#include <vector>

#include "cpu_tracker_harness.cpp"

namespace {

uint64_t g_state = 0x853C49E6748FEA9Bull;

double lcg() {          // [0, 1)
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) * (1.0 / 9007199254740992.0);
}

struct Set {
    double gate;
    int coast;
    double alpha_pos, alpha_vel;
};

int run(int B, int R, const Set &q) {
    const double dt = 0.1;
    std::vector<float> obs((size_t)B * R * 8), out((size_t)B * R * 8);
    std::vector<double> pos((size_t)B * R * 2), vel((size_t)B * R * 2), tf((size_t)B * 16 * 7);
    std::vector<uint8_t> done((size_t)B), slot((size_t)B * R), miss((size_t)B * R);
    std::vector<int32_t> ti((size_t)B * 16 * 3);
    std::vector<int64_t> counts((size_t)7 * B);
    for (size_t k = 0; k < pos.size(); ++k) pos[k] = 80.0 * lcg() - 40.0, vel[k] = 20.0 * lcg() - 10.0;
    for (int step = 0; step < 40; ++step) {
        const bool all = step == 30 || step == 31;
        for (int b = 0; b < B; ++b) {
            done[b] = (step % 9 == 8 && b % 2 == 0) ? 1 : 0;
            for (int i = 0; i < R; ++i) {
                const size_t k = ((size_t)b * R + i) * 2;
                if (lcg() < 0.03) pos[k] = 80.0 * lcg() - 40.0, pos[k + 1] = 80.0 * lcg() - 40.0;
                pos[k] += vel[k] * dt, pos[k + 1] += vel[k + 1] * dt;
                float *row = &obs[((size_t)b * R + i) * 8];
                const bool present = i == 0 || all || lcg() < 0.7;
                const double far = step == 31 && i > 0 ? 1000.0 : 0.0;
                const double c = 2.0 * lcg() - 1.0;
                const double v[8] = {1.0, pos[k] + far, pos[k + 1], vel[k], vel[k + 1], 6.0 * lcg() - 3.0, 1.0 - c * c, c};
                for (int j = 0; j < 8; ++j) row[j] = present ? (float)v[j] : 0.0f;
            }
        }
        const bool planes = step % 2 == 0;
        const int rc = tracker_step(B, R, step == 0 || step == 20, dt, q.gate, q.coast, q.alpha_pos, q.alpha_vel, obs.data(),
                                    step % 3 ? done.data() : nullptr, out.data(), planes ? slot.data() : nullptr,
                                    planes ? miss.data() : nullptr, tf.data(), ti.data(), counts.data());
        if (rc != 0) return 1;
        for (int b = 0; b < B; ++b) {
            int alive = 0, rows = 0;
            for (int s = 0; s < 16; ++s) alive += ti[((size_t)b * 16 + s) * 3] != 0;
            for (int i = 1; i < R; ++i) rows += out[((size_t)b * R + i) * 8] != 0.0f;
            if (rows != (alive < R - 1 ? alive : R - 1)) return 2;
            const int64_t *n = &counts[b];                       // measured = matched + born
            if (n[0] != n[(size_t)B] + n[(size_t)2 * B]) return 3;
        }
    }
    return 0;
}

}  // namespace

int main() {
    const double inf = std::numeric_limits<double>::infinity();
    const int shapes[4][2] = {{1, 1}, {3, 2}, {5, 10}, {4, 17}};
    const Set sets[6] = {{3.0, 0, 1.0, 1.0}, {3.0, 3, 1.0, 1.0}, {3.0, 0, 0.5, 0.3}, {0.0, 0, 1.0, 1.0}, {inf, 0, 1.0, 1.0},
                         {3.0, 50, 0.5, 0.3}};
    for (const auto &sh : shapes)
        for (int k = 0; k < 6; ++k) {
            const int rc = run(sh[0], sh[1], sets[k]);
            if (rc != 0) {
                std::printf("tracker_san_main: B=%d R=%d set=%d failed (%d)\n", sh[0], sh[1], k, rc);
                return 1;
            }
        }
    std::printf("tracker_san_main: ok\n");
    return 0;
}
