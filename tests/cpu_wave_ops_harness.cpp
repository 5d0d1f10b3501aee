// TEST INFRASTRUCTURE - host twin of tests/dev_wave_ops.hip (-m "not gpu"): the operations of tests/wave_ops_probe.hpp on the host
// model of the wave (HostCtx, HostCtxLtvRelaxed of tests/host_wave_ctx.hpp), and the host build of the lean FP64 math of
// mpc_core.hpp that has no device-only branch.  Never loaded by the product.
#include <utility>

#include "host_wave_ctx.hpp"
#include "wave_ops_probe.hpp"

namespace {

template <class CTX, int... OPS>
int run_op(int op, int sets, const double *in, double *out, std::integer_sequence<int, OPS...>) {
    bool found = false;
    for (int s = 0; s < sets; ++s) {
        double L[probe::kL] = {};
        CTX c{{L, nullptr, 0, 0}};
        c.nwords = probe::kL;
        ((op == OPS ? (found = true, probe::wave_op<OPS>(c, in + (size_t)s * probe::kIn[OPS] * probe::kL,
                                                          out + (size_t)s * probe::kOut[OPS] * probe::kL))
                    : (void)0),
         ...);
    }
    return found ? 0 : -1;
}

// (derived like HostCtxLtvRelaxed, so that run_op's nested-brace initialiser - base, then members - fits both)
struct HostCtxPlain : HostCtx {};

}  // namespace

// the entry point of dev_wave_ops.hip on host memory.  Bit 3 of relax selects HostCtxLtvRelaxed, the context of the LTV latency
// build's host harness; it overrides no primitive (kRelax only steers mpc_ltv.hpp), so both run the same model here, and fresh /
// opaque / opaque_shared are the identity in both.
extern "C" int cpu_wave_op(int relax, int op, int sets, const double *in, double *out) {
    if (sets < 1 || !in || !out) return -1;
    const auto ops = std::make_integer_sequence<int, probe::OP_COUNT>{};
    if (relax != 0 && relax != 3 && relax != 7 && relax != 11) return -1;
    return (relax & 8) ? run_op<HostCtxLtvRelaxed>(op, sets, in, out, ops) : run_op<HostCtxPlain>(op, sets, in, out, ops);
}
extern "C" int cpu_wave_op_shape(int op, int *n_in, int *n_out) {
    if (op < 0 || op >= probe::OP_COUNT) return -1;
    *n_in = probe::kIn[op];
    *n_out = probe::kOut[op];
    return 0;
}

// sincos_half, sincos_delta_theta, dyn_eval as the host harnesses of the solvers run them; -2 for the functions whose host branch
// is libm (frcp, frsqrt, atan_b, log_pos) and the raw hardware seeds
extern "C" int cpu_math(int fn, int n, const double *in, double *out) {
    if (fn < 0 || fn >= probe::FN_COUNT || n < 1 || !in || !out) return -1;
    if (fn != probe::FN_SINCOS_HALF && fn != probe::FN_SINCOS_DELTA_THETA && fn != probe::FN_DYN_EVAL) return -2;
    mpc::TrigCoef K;
    for (int i = 0; i < 6; ++i) {
        K.s[i] = mpc::trig_coef(i);
        K.c[i] = mpc::trig_coef(6 + i);
    }
    for (int i = 0; i < n; ++i) {
        const double x0 = in[i], x1 = probe::kFnIn[fn] > 1 ? in[(size_t)n + i] : 0.0;
        double y[4] = {0.0, 0.0, 0.0, 0.0};
        if (fn == probe::FN_SINCOS_HALF) mpc::sincos_half(K, x0, y[0], y[1]);
        else if (fn == probe::FN_SINCOS_DELTA_THETA) mpc::sincos_delta_theta(K, x0, x1, y[0], y[1], y[2], y[3]);
        else mpc::dyn_eval(K, x0, x1, y[0], y[1], y[2], y[3]);
        for (int k = 0; k < probe::kFnOut[fn]; ++k) out[(size_t)k * n + i] = y[k];
    }
    return 0;
}
