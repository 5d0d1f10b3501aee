// TEST INFRASTRUCTURE - the launch-order tiers of csrc/mpc_order.hpp compiled for the host (tests/order_host.py).
#include "../mpc-rl_for_avs_amd/csrc/mpc_order.hpp"

extern "C" {

// tier_of for every instance of a batch; others / nveh may be null
void order_tiers(int B, const uint8_t *is_collide, const double *state, const double *others, int V, const int32_t *nveh,
                 const int32_t *ego, const double *ref5, int M, int N, int seats, double T, int32_t *tier) {
    for (int i = 0; i < B; ++i) tier[i] = mpc::order::tier_of(is_collide, state, others, V, nveh, ego, ref5, M, N, i, seats != 0, T);
}

// first_seat alone, and the squared closest approach per vehicle [B][V]
void order_first_seat(int B, const uint8_t *is_collide, const double *state, const double *others, int V, const int32_t *nveh,
                      double T, uint8_t *first, double *d2) {
    for (int i = 0; i < B; ++i) {
        const double *x = state + (size_t)i * 4;
        const int nv = nveh ? (nveh[i] < 0 ? 0 : (nveh[i] > V ? V : nveh[i])) : V;
        first[i] = mpc::order::first_seat(is_collide[i] != 0, x, others + (size_t)i * V * 4, nv, T) ? 1 : 0;
        for (int j = 0; j < V; ++j)
            d2[(size_t)i * V + j] = mpc::order::closest_approach2(x, cos(x[2]), sin(x[2]), others + ((size_t)i * V + j) * 4, T);
    }
}

}  // extern "C"
