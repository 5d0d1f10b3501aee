// Host build of mpc-rl_for_avs_amd/csrc/mpc_actuator.hpp for tests only (-m "not gpu"): the per-environment update of the
// mpc_actuate kernel looped over environments on the CPU, against a plain-Python restatement of its statements and the
// evaluator's CPU path (tests/test_actuator_cpu.py).  The argument checks are those of the library.  Compiled with
// -ffp-contract=off.  Never loaded by the product.  tests/actuator_san_main.cpp includes this file.
#include <cstdint>

#include "../mpc-rl_for_avs_amd/csrc/mpc_actuator.hpp"

namespace act = mpc::act;

// par [16] = dt, p_hold, gain[2], offset[2], sigma[2], alpha[2], rate[2], lo[2], hi[2]
extern "C" int actuator_step(int B, int reset, const double *par, uint64_t seed, int delay, int env_offset,
                             const double *command, const uint8_t *done_prev, double *applied, double *state_f64,
                             int32_t *age, int64_t *ctr, int64_t *counts, double *sums) {
    if (B < 0 || !par || !state_f64 || !age || !ctr || !counts || !sums) return -1;
    if (reset == 0 && (!command || !applied)) return -1;
    const act::Params P{par[0],           par[1],           {par[2], par[3]},   {par[4], par[5]},   {par[6], par[7]}, {par[8], par[9]},
                        {par[10], par[11]}, {par[12], par[13]}, {par[14], par[15]}, seed,           delay,            env_offset};
    if (act::refusal(P) != nullptr) return -1;
    const act::Buffers buf{B, command, done_prev, applied, state_f64, age, ctr, counts, sums};
    for (int b = 0; b < B; ++b) act::actuate_env(P, buf, b, reset != 0);
    return 0;
}
