// seat_probe.hip - which workgroups of a batch of 4096 share a SIMD, and which of the two runs at the lone-wave rate?
// Development tool.  One-wave workgroups with the latency build's footprint (two waves per SIMD by registers: 251 VGPRs;
// 16.2 KB of LDS) record HW_ID / XCC_ID, the clock at their start and the ticks a fixed FP64 chain took them.  The host
// groups them by SIMD and looks at the two that were resident from the start of the launch (the "seats"): the distance of
// their workgroup indices, which of them started first, and the time of each against a wave alone on its SIMD (the same
// kernel launched with 1024 workgroups).
//   hipcc --offload-arch=gfx950 -O3 -o tools/ubench/seat_probe tools/ubench/seat_probe.hip && tools/ubench/seat_probe
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <map>
#include <vector>

struct Rec {
    long long start, ticks;
    unsigned hw, xcc;
};

__global__ __launch_bounds__(64, 2) void probe(Rec *out, double *sink, int B, int iters) {
    extern __shared__ double lds[];
    if ((int)blockIdx.x >= B) return;
    asm volatile("v_mov_b32 v250, 0" ::: "v250");        // the footprint: more than 168 registers = two waves per SIMD
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    double a = 1.0 + threadIdx.x * 1e-9, b = 0.5, c = 1.0000001, d = 0.25;
    const long long t0 = wall_clock64();
    for (int i = 0; i < iters; ++i) {                    // two FP64 chains, as tools/ubench/setprio_probe.hip
        a = __builtin_fma(a, c, b);
        d = __builtin_fma(d, c, a * 1e-30);
        a = __builtin_fma(a, 0.999999, -b);
        d = __builtin_fma(d, 0.999999, b);
    }
    const long long t1 = wall_clock64();
    lds[threadIdx.x] = a + d;
    if (threadIdx.x == 0) {
        Rec r;
        r.start = t0;
        r.ticks = t1 - t0;
        r.hw = hw;
        r.xcc = xcc & 0xf;
        out[blockIdx.x] = r;
    }
    if (a + d == 12345.678) sink[0] = lds[63 - threadIdx.x];
}

static unsigned long long simd_of(const Rec &r) {
    const unsigned simd = (r.hw >> 4) & 3, cu = (r.hw >> 8) & 0xf, sh = (r.hw >> 12) & 1, se = (r.hw >> 13) & 7;
    return ((((unsigned long long)r.xcc << 12) | (se << 8) | (sh << 4) | cu) << 2) | simd;
}

static double median(std::vector<double> v) {
    if (v.empty()) return 0.0;
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

int main() {
    const int BMAX = 4096, iters = 60000;
    const size_t lds = 16200 / 8 * 8;
    Rec *d;
    double *sink;
    if (hipMalloc(&d, BMAX * sizeof(Rec)) != hipSuccess || hipMalloc(&sink, sizeof(double)) != hipSuccess) return 1;
    hipFuncSetAttribute(reinterpret_cast<const void *>(probe), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    std::vector<Rec> h(BMAX);
    double lone = 0.0;
    for (int B : {1024, 4096, 4096}) {
        (void)hipMemset(d, 0, BMAX * sizeof(Rec));
        hipLaunchKernelGGL(probe, dim3(B), dim3(64), lds, 0, d, sink, B, iters);
        if (hipDeviceSynchronize() != hipSuccess) return 2;
        (void)hipMemcpy(h.data(), d, B * sizeof(Rec), hipMemcpyDeviceToHost);
        std::map<unsigned long long, std::vector<int>> by_simd;
        for (int b = 0; b < B; ++b) by_simd[simd_of(h[b])].push_back(b);
        std::vector<double> all;
        for (int b = 0; b < B; ++b) all.push_back(h[b].ticks / 100.0);
        printf("B = %d: %zu distinct SIMDs, median time of a workgroup %.1f us\n", B, by_simd.size(), median(all));
        if (B == 1024) {
            lone = median(all);
            continue;
        }
        // the seats: per SIMD the two workgroups that started first
        std::map<int, int> diff;
        std::vector<double> t_low, t_high, gap;
        int pairs = 0, low_first = 0, low_faster = 0, both_below_2048 = 0, low_below_1024 = 0, high_in_second_k = 0, shown = 0;
        for (auto &kv : by_simd) {
            auto &v = kv.second;
            std::sort(v.begin(), v.end(), [&](int x, int y) { return h[x].start < h[y].start; });
            if (v.size() < 2) continue;
            const int first = v[0], second = v[1], lo = std::min(first, second), hi = std::max(first, second);
            ++pairs;
            diff[hi - lo]++;
            low_first += first == lo;
            low_faster += h[lo].ticks < h[hi].ticks;
            both_below_2048 += hi < 2048;
            low_below_1024 += lo < 1024;
            high_in_second_k += hi >= 1024 && hi < 2048;
            t_low.push_back(h[lo].ticks / 100.0);
            t_high.push_back(h[hi].ticks / 100.0);
            gap.push_back((h[hi].start - h[lo].start) / 100.0);
            if (shown++ < 6) {
                printf("   SIMD %05llx:", kv.first);
                for (int b : v) printf("  wg %d (+%.1f us, %.1f us)", b, (h[b].start - h[v[0]].start) / 100.0, h[b].ticks / 100.0);
                printf("\n");
            }
        }
        printf("   seats (first two workgroups of a SIMD by start time), %d SIMDs: both indices below 2048 on %d; lower index below 1024 on %d, "
               "higher index in 1024..2047 on %d\n", pairs, both_below_2048, low_below_1024, high_in_second_k);
        std::vector<std::pair<int, int>> dd;
        for (auto &kv : diff) dd.push_back({kv.second, kv.first});
        std::sort(dd.rbegin(), dd.rend());
        printf("   index distance of the two seats, most frequent:");
        for (size_t i = 0; i < dd.size() && i < 5; ++i) printf("  %d (%d SIMDs)", dd[i].second, dd[i].first);
        printf("\n   the lower index started first on %d SIMDs (median lead %.1f us) and finished its chain faster on %d\n", low_first,
               median(gap), low_faster);
        printf("   chain time: alone on a SIMD %.1f us; lower-index seat median %.1f us (x %.3f); higher-index seat median %.1f us (x %.3f)\n",
               lone, median(t_low), median(t_low) / lone, median(t_high), median(t_high) / lone);
        // the workgroups that start later: by index quarter, the median start and time
        const long long s0 = std::min_element(h.begin(), h.begin() + B, [](const Rec &x, const Rec &y) { return x.start < y.start; })->start;
        for (int q = 0; q < 4; ++q) {
            std::vector<double> st, tk;
            for (int b = q * B / 4; b < (q + 1) * B / 4; ++b) {
                st.push_back((h[b].start - s0) / 100.0);
                tk.push_back(h[b].ticks / 100.0);
            }
            printf("   workgroups %4d..%4d: median start %.1f us after the first, median chain time %.1f us (x %.3f of alone)\n", q * B / 4,
                   (q + 1) * B / 4 - 1, median(st), median(tk), median(tk) / lone);
        }
    }
    (void)hipFree(d);
    (void)hipFree(sink);
    return 0;
}
