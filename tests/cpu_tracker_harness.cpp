// Host build of mpc-rl_for_avs_amd/csrc/mpc_tracker.hpp for tests only (-m "not gpu"): the per-environment update of the
// mpc_track_rows kernel looped over environments on the CPU, against a plain-Python restatement of its statements and the
// evaluator's CPU path (tests/test_tracker_cpu.py).  The argument checks are those of the library.  Compiled with
// -ffp-contract=off.  Never loaded by the product.  tests/tracker_san_main.cpp includes this file.
#include <cstdint>

#include "../mpc-rl_for_avs_amd/csrc/mpc_tracker.hpp"

namespace track = mpc::track;

extern "C" int tracker_step(int B, int R, int reset, double dt, double gate, int coast, double alpha_pos, double alpha_vel,
                            const float *obs_meas, const uint8_t *done, float *obs_out, uint8_t *row_slot, uint8_t *row_miss,
                            double *track_f64, int32_t *track_i32, int64_t *counts) {
    if (B < 0 || R < 1 || R > track::kMaxRows) return -1;
    if (!(dt > 0.0) || !(gate >= 0.0) || coast < 0 || coast > track::kMaxCoast) return -1;
    if (!(alpha_pos > 0.0 && alpha_pos <= 1.0) || !(alpha_vel > 0.0 && alpha_vel <= 1.0)) return -1;
    if (!obs_meas || !obs_out || obs_out == obs_meas || !track_f64 || !track_i32 || !counts) return -1;
    const track::Params P{dt, gate * gate, alpha_pos, alpha_vel, coast};
    const track::Buffers buf{B, R, obs_meas, done, obs_out, row_slot, row_miss, track_f64, track_i32, counts};
    for (int b = 0; b < B; ++b) track::track_env(P, buf, b, reset != 0);
    return 0;
}
