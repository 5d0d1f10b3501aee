// TEST INFRASTRUCTURE - device probe of mpc-rl_for_avs_amd/csrc/mpc_wave_dev.hpp (WaveOpsT<RELAX>: matrix core, DPP lane
// permutations, reductions, LDS phases) and of the lean FP64 math of mpc_core.hpp, compiled with the product's flags into
// tests/_build/libdev_wave_ops.so.  The operations are those of tests/wave_ops_probe.hpp, which tests/cpu_wave_ops_harness.cpp
// runs on the host model; tests/test_wave_ops_gpu.py compares the two bit for bit, tests/test_device_math_gpu.py the math with
// mpmath.  One workgroup of one wave handles one input set, as one wave handles one MPC instance in the engine.  The entry points
// take device pointers and a stream and only enqueue.  Never loaded by the product.
#include <hip/hip_runtime.h>

#include <utility>

#include "../mpc-rl_for_avs_amd/csrc/mpc_wave_dev.hpp"
#include "wave_ops_probe.hpp"

namespace {

constexpr int kBlock = 64;

template <int RELAX, int OP>
__global__ __launch_bounds__(kBlock) void wave_op_kernel(const double *in, double *out) {
    __shared__ double smem[probe::kL];
    mpc::wave::WaveOpsT<RELAX> c{(mpc::wave::lds_double_t *)smem};
    probe::wave_op<OP>(c, in + (size_t)blockIdx.x * probe::kIn[OP] * probe::kL, out + (size_t)blockIdx.x * probe::kOut[OP] * probe::kL);
}

template <int RELAX, int OP>
void launch_one(int sets, const double *in, double *out, hipStream_t stream) {
    hipLaunchKernelGGL((wave_op_kernel<RELAX, OP>), dim3((unsigned)sets), dim3(kBlock), 0, stream, in, out);
}
template <int RELAX, int... OPS>
int launch_op(int op, int sets, const double *in, double *out, hipStream_t stream, std::integer_sequence<int, OPS...>) {
    bool found = false;
    ((op == OPS ? (found = true, launch_one<RELAX, OPS>(sets, in, out, stream)) : (void)0), ...);
    return found ? (int)hipGetLastError() : -1;
}

// coefficient tables in LDS, read back into registers by every thread, as the solver's trig() / flog() do
__global__ __launch_bounds__(kBlock) void math_kernel(int fn, int n, const double *in, double *out) {
    __shared__ double tab[mpc::kTrigWords + mpc::kLogWords];
    if (threadIdx.x < mpc::kTrigWords) tab[threadIdx.x] = mpc::trig_coef(threadIdx.x);
    else if (threadIdx.x < mpc::kTrigWords + mpc::kLogWords) tab[threadIdx.x] = mpc::log_coef(threadIdx.x - mpc::kTrigWords);
    __syncthreads();
    mpc::TrigCoef K;
    double KL[mpc::kLogWords];
    for (int i = 0; i < 6; ++i) {
        K.s[i] = tab[i];
        K.c[i] = tab[6 + i];
    }
    for (int i = 0; i < mpc::kLogWords; ++i) KL[i] = tab[mpc::kTrigWords + i];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double x0 = in[i], x1 = probe::kFnIn[fn] > 1 ? in[(size_t)n + i] : 0.0;
    double y[4] = {0.0, 0.0, 0.0, 0.0};
    switch (fn) {
        case probe::FN_RCP: y[0] = __builtin_amdgcn_rcp(x0); break;
        case probe::FN_RSQ: y[0] = __builtin_amdgcn_rsq(x0); break;
        case probe::FN_FRCP: y[0] = mpc::frcp(x0); break;
        case probe::FN_FRSQRT: y[0] = mpc::frsqrt(x0); break;
        case probe::FN_SINCOS_HALF: mpc::sincos_half(K, x0, y[0], y[1]); break;
        case probe::FN_SINCOS_DELTA_THETA: mpc::sincos_delta_theta(K, x0, x1, y[0], y[1], y[2], y[3]); break;
        case probe::FN_ATAN_B: y[0] = mpc::atan_b(K, x0); break;
        case probe::FN_LOG_POS: y[0] = mpc::log_pos(KL, x0); break;
        case probe::FN_DYN_EVAL: mpc::dyn_eval(K, x0, x1, y[0], y[1], y[2], y[3]); break;
        default: break;
    }
    for (int k = 0; k < probe::kFnOut[fn]; ++k) out[(size_t)k * n + i] = y[k];
}

}  // namespace

// in [sets][kIn[op]][64], out [sets][kOut[op]][64] doubles on the device.  0, -1 for an unknown op / build, or the HIP error.
extern "C" int dev_wave_op(int relax, int op, int sets, const double *in, double *out, void *stream) {
    if (sets < 1 || !in || !out) return -1;
    const auto ops = std::make_integer_sequence<int, probe::OP_COUNT>{};
    hipStream_t s = (hipStream_t)stream;
    switch (relax) {   // every RELAX the engine instantiates: throughput builds, preamble, solve latency build, LTV latency build
        case 0: return launch_op<0>(op, sets, in, out, s, ops);
        case 3: return launch_op<3>(op, sets, in, out, s, ops);
        case 7: return launch_op<7>(op, sets, in, out, s, ops);
        case 11: return launch_op<11>(op, sets, in, out, s, ops);
        default: return -1;
    }
}
extern "C" int dev_wave_op_shape(int op, int *n_in, int *n_out) {
    if (op < 0 || op >= probe::OP_COUNT) return -1;
    *n_in = probe::kIn[op];
    *n_out = probe::kOut[op];
    return 0;
}

// in [kFnIn[fn]][n], out [kFnOut[fn]][n] doubles on the device, one point per thread
extern "C" int dev_math(int fn, int n, const double *in, double *out, void *stream) {
    if (fn < 0 || fn >= probe::FN_COUNT || n < 1 || !in || !out) return -1;
    hipLaunchKernelGGL(math_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream, fn, n, in, out);
    return (int)hipGetLastError();
}
extern "C" int dev_math_shape(int fn, int *n_in, int *n_out) {
    if (fn < 0 || fn >= probe::FN_COUNT) return -1;
    *n_in = probe::kFnIn[fn];
    *n_out = probe::kFnOut[fn];
    return 0;
}
