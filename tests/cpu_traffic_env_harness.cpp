// Host build of mpc-rl_for_avs_amd/csrc/mpc_synth_traffic.hpp for tests only (-m "not gpu"): the environment step with
// reactive traffic, one loop iteration per environment, with the argument list of mpc_synth_env_step_idm minus device and
// stream, plus two optional diagnostics [B][K']: whom each vehicle followed and the acceleration it chose.
#include <cmath>
#include <cstdint>

#include "../mpc-rl_for_avs_amd/csrc/mpc_synth_traffic.hpp"

extern "C" int traffic_env_step(int B, int K, double dt, double spawn_probability, uint64_t seed, int env_offset,
                                const double *ref_xy, int M, const double *action, double *ego, double *opos, double *ospeed,
                                double *ohead, uint8_t *oactive, int32_t *oroute, double *oprog, double *otarget, int32_t *t,
                                int64_t *ctr, float *obs, float *terminal_obs, float *reward, uint8_t *done, uint8_t *truncated,
                                uint8_t *crashed, uint8_t *arrived, int reset_all, int32_t *leader, double *accel) {
    namespace env = mpc::env;
    if (K < 0 || K > env::kMaxOthers) return -1;
    const int Ks = K > 0 ? K : 1;
    for (int b = 0; b < B; ++b) {
        const size_t vo = (size_t)b * Ks;
        const env::View v{ego + (size_t)b * 4, opos + vo * 2, ospeed + vo, ohead + vo, oactive + vo, t + b, ctr + b};
        const env::TrafficView tv{oroute + vo, oprog + vo, otarget + vo};
        float *o = obs + (size_t)b * env::kRows * env::kCols;
        if (reset_all) {
            const env::Rng r(seed, env_offset + b, *v.ctr);
            *v.ctr += 1;
            env::reset_env_idm(v, tv, K, r);
            env::observe(v, K, o);
            continue;
        }
        const env::StepOut so = env::step_env_idm(v, tv, K, dt, spawn_probability, seed, env_offset + b, ref_xy, M,
                                                  action + (size_t)b * 2, terminal_obs + (size_t)b * env::kRows * env::kCols, o,
                                                  leader ? leader + vo : nullptr, accel ? accel + vo : nullptr);
        reward[b] = so.reward;
        done[b] = so.done;
        truncated[b] = so.truncated;
        crashed[b] = so.crashed;
        arrived[b] = so.arrived;
    }
    return 0;
}

extern "C" void traffic_pose(int n, const int32_t *route, const double *s, double *x, double *y, double *h) {
    for (int i = 0; i < n; ++i) mpc::env::pose(route[i], s[i], x[i], y[i], h[i]);
}
