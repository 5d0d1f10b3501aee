// Stand-alone program for a sanitizer run of the host build of csrc/mpc_episode_trace.hpp (tests/test_episode_trace_cpu.py
// compiles it with -fsanitize=address,undefined and runs it as a child process; nothing is loaded into Python): small streams
// from a simple LCG into exactly sized heap buffers, so that any access past a ring entry, a store slot or the batch is
// reported - a window of 3 with episodes longer than it, a store of one slot with drops, 17 rows, with and without the seen
// plane, a reset launch in the middle, an environment past its quota.  It also checks the counts' invariant and the index.
#include <cstdio>
#include <vector>

#include "cpu_episode_trace_harness.cpp"

namespace {

uint64_t g_state = 0x853C49E6748FEA9Bull;

double lcg() {          // [0, 1)
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) * (1.0 / 9007199254740992.0);
}

int run(int B, int R, int Q, int W, int C, int keep, bool with_seen) {
    const size_t scene = (size_t)R * 8;
    std::vector<float> terminal(B * scene), obs(B * scene), seen(with_seen ? B * scene : 0), reward(B);
    std::vector<double> action((size_t)B * 2);
    std::vector<uint8_t> done(B), truncated(B), crashed(B), arrived(B);
    std::vector<int32_t> status(B), iters(B), state((size_t)4 * B), slot(B);
    std::vector<float> ring_scene((size_t)B * (W + 1) * scene), ring_seen(with_seen ? (size_t)B * W * scene : 0), ring_reward((size_t)B * W);
    std::vector<double> ring_act((size_t)B * W * 2);
    std::vector<int32_t> ring_i32((size_t)B * W * 3);
    std::vector<float> kept_scene((size_t)C * (W + 1) * scene), kept_seen(with_seen ? (size_t)C * W * scene : 0), kept_reward((size_t)C * W);
    std::vector<double> kept_act((size_t)C * W * 2);
    std::vector<int32_t> kept_i32((size_t)C * W * 3), index((size_t)C * 6);
    std::vector<int64_t> counts(4);
    for (int step = 0; step < 60; ++step) {
        const bool reset = step == 0 || step == 35;
        for (auto *v : {&terminal, &obs, &seen, &reward})
            for (float &x : *v) x = (float)(20.0 * lcg() - 10.0);
        for (double &x : action) x = 2.0 * lcg() - 1.0;
        for (int b = 0; b < B; ++b) {
            done[b] = lcg() < (b % 3 == 0 ? 0.5 : 0.15);     // every third environment ends often: it passes its quota
            truncated[b] = done[b] && lcg() < 0.5;
            arrived[b] = done[b] && lcg() < 0.5;
            crashed[b] = lcg() < 0.1;
            status[b] = (int32_t)(9.0 * lcg());
            iters[b] = (int32_t)(100.0 * lcg());
        }
        const int rc = episode_trace_step(B, R, Q, W, C, keep, reset, reset ? nullptr : terminal.data(), obs.data(),
                                          with_seen && !reset ? seen.data() : nullptr, action.data(), reward.data(), done.data(),
                                          truncated.data(), crashed.data(), arrived.data(), status.data(), iters.data(),
                                          state.data(), ring_scene.data(), with_seen ? ring_seen.data() : nullptr,
                                          ring_act.data(), ring_reward.data(), ring_i32.data(), slot.data(), kept_scene.data(),
                                          with_seen ? kept_seen.data() : nullptr, kept_act.data(), kept_reward.data(),
                                          kept_i32.data(), index.data(), counts.data());
        if (rc != 0) return 1;
        if (counts[0] != counts[1] + counts[2] || counts[1] > C) return 2;
        if (counts[3] != (step < 35 ? step : step - 35)) return 3;
        for (int64_t s = 0; s < counts[1]; ++s) {
            const int32_t *ix = &index[(size_t)s * 6];
            const int32_t L = ix[2] < W ? ix[2] : W;
            if (ix[0] < 0 || ix[0] >= B || ix[1] < 0 || ix[1] >= Q || ix[2] < 1 || ix[3] != ix[2] - L || ix[5] < 1) return 4;
            if (!(kept_i32[((size_t)s * W + (L - 1)) * 3 + 2] & 1)) return 5;      // the last kept frame carries done
        }
    }
    return 0;
}

}  // namespace

int main() {
    // B, R, Q, W, C, keep
    const int shapes[5][6] = {{1, 1, 1, 1, 1, 16}, {5, 17, 2, 3, 1, 16}, {7, 10, 3, 3, 4, 3}, {4, 17, 1, 8, 4, 8}, {9, 2, 2, 5, 18, 4}};
    for (const auto &sh : shapes)
        for (int with_seen = 0; with_seen < 2; ++with_seen) {
            const int rc = run(sh[0], sh[1], sh[2], sh[3], sh[4], sh[5], with_seen != 0);
            if (rc != 0) {
                std::printf("episode_trace_san_main: B=%d R=%d Q=%d W=%d C=%d keep=%d seen=%d failed (%d)\n", sh[0], sh[1], sh[2],
                            sh[3], sh[4], sh[5], with_seen, rc);
                return 1;
            }
        }
    std::printf("episode_trace_san_main: ok\n");
    return 0;
}
