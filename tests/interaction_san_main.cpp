// Stand-alone program for a sanitizer run of the host build of csrc/mpc_interaction.hpp (tests/test_interaction_cpu.py compiles
// it with -fsanitize=address,undefined and runs it as a child process; nothing is loaded into Python): the shapes of the tests
// (B = 1, 5, 17; K = 1, 4, 9; Q = 1, 2; M = 1, 2, 85), streams of states from a simple LCG in which vehicles advance along
// their routes, slots are emptied and refilled and episodes end, a reset launch in the middle, exactly sized heap buffers so
// that any access past a slot, a route, a batch or the conflict table is reported; the forced-braking and the
// post-encroachment scenarios of the tests with their stated answers.
#include <cstdio>
#include <vector>

#include "cpu_interaction_harness.cpp"

namespace {

uint64_t g_state = 0x853C49E6748FEA9Bull;

double lcg() {          // [0, 1)
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) * (1.0 / 9007199254740992.0);
}

struct Scene {
    int B, K;
    std::vector<double> ego, opos, ospeed, ohead, oprog, otarget;
    std::vector<uint8_t> oactive, done;
    std::vector<int32_t> oroute;
    Scene(int B_, int K_)
        : B(B_), K(K_), ego((size_t)B_ * 4), opos((size_t)B_ * K_ * 2), ospeed((size_t)B_ * K_), ohead((size_t)B_ * K_),
          oprog((size_t)B_ * K_), otarget((size_t)B_ * K_), oactive((size_t)B_ * K_), done((size_t)B_),
          oroute((size_t)B_ * K_) {}
    void place(int b, int j, int route, double s, double v, double v0, bool active) {
        const size_t o = (size_t)b * K + j;
        double h;
        mpc::env::pose(route, s, opos[2 * o], opos[2 * o + 1], h);
        ohead[o] = h;
        oroute[o] = route;
        oprog[o] = s;
        ospeed[o] = v;
        otarget[o] = v0;
        oactive[o] = active ? 1 : 0;
    }
};

struct Books {
    std::vector<int32_t> si, ri;
    std::vector<double> sf, rf;
    Books(int B, int Q)
        : si((size_t)ia::kStateI32 * B), ri((size_t)ia::kRecI32 * B * Q), sf((size_t)ia::kStateF64 * B),
          rf((size_t)ia::kRecF64 * B * Q) {}
};

int step(Scene &s, Books &k, int Q, const std::vector<double> &ref, const double *conflict, bool reset, double *margin) {
    return interaction_step(s.B, s.K, Q, (int)(ref.size() / 2), reset, 0.1, s.ego.data(), s.opos.data(), s.ospeed.data(),
                            s.ohead.data(), s.oactive.data(), s.oroute.data(), s.oprog.data(), s.otarget.data(),
                            reset ? nullptr : s.done.data(), ref.data(), conflict, k.si.data(), k.sf.data(),
                            k.ri.data(), k.rf.data(), nullptr, nullptr, margin);
}

int run(int B, int K, int Q, int M) {
    std::vector<double> ref((size_t)M * 2), conflict(24);
    for (int i = 0; i < M; ++i) {         // down x = 2, then bending towards -x
        ref[2 * i] = 2.0 - (i > M / 2 ? 1.5 * (i - M / 2) : 0.0);
        ref[2 * i + 1] = 50.0 - (100.0 / (M > 1 ? M - 1 : 1)) * i;
    }
    for (int r = 0; r < 12; ++r) {
        conflict[2 * r] = r % 3 == 2 ? -1.0 : 20.0 + 3.0 * r;
        conflict[2 * r + 1] = 45.0 + 2.0 * r;
    }
    Scene s(B, K);
    Books k(B, Q);
    std::vector<double> sigma((size_t)B);
    double margin = 1e300;
    for (int n = 0; n <= 60; ++n) {
        for (int b = 0; b < B; ++b) {
            s.done[b] = n > 0 && lcg() < 0.06;
            if (n == 0 || s.done[b]) sigma[b] = 30.0 * lcg();
            else sigma[b] += 2.0 * lcg() - 0.2;
            s.ego[4 * b] = 2.0 + 2.0 * lcg() - 1.0;
            s.ego[4 * b + 1] = 50.0 - sigma[b];
            s.ego[4 * b + 2] = -1.5707963267948966 + 0.2 * lcg();
            s.ego[4 * b + 3] = 12.0 * lcg();
            for (int j = 0; j < K; ++j) {
                const size_t o = (size_t)b * K + j;
                if (n == 0 || s.done[b] || lcg() < 0.05)
                    s.place(b, j, (int)(12.0 * lcg()) % 12, 20.0 + 40.0 * lcg(), 12.0 * lcg(), 4.0 + 8.0 * lcg(), lcg() < 0.8);
                else
                    s.place(b, j, s.oroute[o], s.oprog[o] + 3.0 * lcg() - (lcg() < 0.03 ? 20.0 : 0.0), 12.0 * lcg(), s.otarget[o],
                            s.oactive[o] != 0);
            }
        }
        if (step(s, k, Q, ref, conflict.data(), n == 0 || n == 30, n % 2 ? &margin : nullptr) != 0) return 1;
        for (int b = 0; b < B; ++b) {
            const int32_t *si = &k.si[b];
            if (si[ia::kSteps * (size_t)B] < 1 || si[ia::kOrdinal * (size_t)B] > Q) return 2;
            if (si[ia::kYieldSteps * (size_t)B] > si[ia::kSteps * (size_t)B]) return 3;
            if (si[ia::kPetCriticalN * (size_t)B] > si[ia::kConflicts * (size_t)B]) return 4;
        }
    }
    return 0;
}

// the ego standing at (2, 30), a vehicle on route 9 at s = 10 with speed and target 8: it yields and brakes with 6 m/s^2
int forced_braking() {
    const std::vector<double> ref = {2.0, 50.0, 2.0, -50.0};
    std::vector<double> conflict(24, -1.0);
    Scene s(1, 1);
    Books k(1, 1);
    s.ego = {2.0, 30.0, -1.5707963267948966, 0.0};
    s.place(0, 0, 9, 10.0, 8.0, 8.0, true);
    if (step(s, k, 1, ref, conflict.data(), true, nullptr) != 0) return 1;
    s.done[0] = 1;
    if (step(s, k, 1, ref, conflict.data(), false, nullptr) != 0) return 1;
    const bool ok = k.ri[0] == 1 && k.ri[1] == 1 && k.ri[2] == 1 && k.ri[3] == 1 && k.rf[0] == 6.0 && k.rf[1] == 6.0 * 0.1;
    return ok ? 0 : 5;
}

// the ego passes sigma = 48 between the states 3 and 4, a route-0 vehicle s = 62 between 5 and 6: 2 states = 0.2 s apart
int post_encroachment() {
    const std::vector<double> ref = {2.0, 50.0, 2.0, -50.0};
    std::vector<double> conflict(24, -1.0);
    conflict[0] = 48.0;
    conflict[1] = 62.0;
    Scene s(1, 1);
    Books k(1, 1);
    for (int n = 0; n <= 8; ++n) {
        s.ego = {2.0, 50.0 - (44.5 + n), -1.5707963267948966, 10.0};
        s.place(0, 0, 0, 51.0 + 2.0 * n, 8.0, 8.0, true);
        s.done[0] = n == 8;
        if (step(s, k, 1, ref, conflict.data(), n == 0, nullptr) != 0) return 1;
    }
    const bool ok = k.ri[0] == 8 && k.ri[4] == 1 && k.ri[5] == 1 && k.ri[6] == 1 && k.rf[2] == 2.0 * 0.1;
    return ok ? 0 : 6;
}

}  // namespace

int main() {
    const int shapes[6][4] = {{1, 1, 1, 1}, {1, 9, 2, 2}, {5, 4, 1, 85}, {5, 9, 2, 2}, {17, 1, 2, 85}, {17, 9, 1, 128}};
    for (const auto &sh : shapes) {
        const int rc = run(sh[0], sh[1], sh[2], sh[3]);
        if (rc != 0) {
            std::printf("interaction_san_main: B=%d K=%d Q=%d M=%d failed (%d)\n", sh[0], sh[1], sh[2], sh[3], rc);
            return 1;
        }
    }
    int rc = forced_braking();
    if (rc == 0) rc = post_encroachment();
    if (rc != 0) {
        std::printf("interaction_san_main: scenario failed (%d)\n", rc);
        return 1;
    }
    std::printf("interaction_san_main: ok\n");
    return 0;
}
