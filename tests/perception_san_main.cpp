// Stand-alone program for a sanitizer run of the host build of csrc/mpc_perception.hpp (tests/test_perception_cpu.py compiles
// it with -fsanitize=address,undefined and runs it as a child process; nothing is loaded into Python): the shapes of the CPU
// test, scenes from a simple LCG, exactly sized heap buffers so that any access past a row, a batch or the occluder list is
// reported, all features on, a reset launch in the middle, with and without row_class.
#include <cstdio>
#include <limits>
#include <vector>

#include "cpu_perception_harness.cpp"

namespace {

uint64_t g_state = 0x853C49E6748FEA9Bull;

double lcg() {          // [0, 1)
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) * (1.0 / 9007199254740992.0);
}

int run(int B, int R, int S, bool all_on) {
    std::vector<float> obs((size_t)B * R * 8), seen((size_t)B * R * 8);
    std::vector<double> occ((size_t)S * 8);
    std::vector<uint8_t> cls((size_t)B * R);
    std::vector<int64_t> counts((size_t)5 * B), ctr((size_t)B);
    for (int s = 0; s < S; ++s) {
        const double cx = 60.0 * lcg() - 30.0, cy = 60.0 * lcg() - 30.0, w = 2.0 + 10.0 * lcg(), h = 2.0 + 10.0 * lcg();
        const double q[8] = {cx - w, cy - h, cx + w, cy - h, cx + w, cy + h, cx - w, cy + h};
        for (int k = 0; k < 8; ++k) occ[(size_t)s * 8 + k] = q[k];
    }
    const double inf = std::numeric_limits<double>::infinity();
    for (int step = 0; step < 40; ++step) {
        for (int b = 0; b < B; ++b)
            for (int i = 0; i < R; ++i) {
                float *row = &obs[((size_t)b * R + i) * 8];
                const bool present = i == 0 || lcg() < 0.7;
                const double c = 2.0 * lcg() - 1.0, s = (lcg() < 0.5 ? -1.0 : 1.0) * sqrt(1.0 - c * c);
                const double v[8] = {1.0, 80.0 * lcg() - 40.0, 80.0 * lcg() - 40.0, 30.0 * lcg() - 15.0, 30.0 * lcg() - 15.0,
                                     6.0 * lcg() - 3.0, s, c};
                for (int k = 0; k < 8; ++k) row[k] = present ? (float)v[k] : 0.0f;
            }
        const int rc = perception_step(B, R, S, step == 0 || step == 20, all_on ? 30.0 : inf, all_on, all_on ? 2 : 1,
                                       all_on ? 0.2 : 0.0, all_on ? 0.2 : 0.0, all_on ? 0.3 : 0.0, all_on ? 0.02 : 0.0, 99u + step / 64,
                                       3, obs.data(), S ? occ.data() : nullptr, seen.data(), step % 2 ? cls.data() : nullptr,
                                       counts.data(), ctr.data());
        if (rc != 0) return 1;
        for (int b = 0; b < B; ++b) {
            if (ctr[b] != (step < 20 ? step + 1 : step - 19)) return 2;
            const int64_t *n = &counts[b];
            if (n[0] != n[(size_t)B] + n[(size_t)2 * B] + n[(size_t)3 * B] + n[(size_t)4 * B]) return 3;
        }
    }
    return 0;
}

}  // namespace

int main() {
    const int shapes[4][3] = {{1, 1, 0}, {3, 2, 1}, {5, 10, 4}, {4, 17, 8}};
    for (const auto &sh : shapes)
        for (int on = 0; on < 2; ++on) {
            const int rc = run(sh[0], sh[1], sh[2], on != 0);
            if (rc != 0) {
                std::printf("perception_san_main: B=%d R=%d S=%d all_on=%d failed (%d)\n", sh[0], sh[1], sh[2], on, rc);
                return 1;
            }
        }
    std::printf("perception_san_main: ok\n");
    return 0;
}
