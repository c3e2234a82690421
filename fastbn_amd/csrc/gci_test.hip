// gci_test.hip -- batches of Gaussian conditional-independence tests on the device: one test per lane, the
// kernel templated on the conditioning-set size d (0..8) and fully unrolled, so the (d + 2)(d + 3) / 2
// gathered entries of R and their elimination (gci_elim.h, the function the host twin evaluates too) live
// in registers.  R is read-only and small against the cache (n^2 doubles); the gathers of a test are
// independent loads issued together.  The decision |r| <= tau needs no transcendental: tau comes from the
// host (gci.h).  Without an item array, test t is pair t of the complete graph (level 0 of a PC run).
// The decision-margin log is ci_g2.h's: one atomic pair per wave; degenerate tests are counted beside it.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ci_g2.h"
#include "gci_elim.h"
#include "launchers.h"

namespace {

// the row i of pair index t among the pairs (i < j) of n variables in lexicographic order (PairRow,
// pc_internal.h)
__device__ __forceinline__ int pair_row(long long t, int n) {
    long long lo = 0, hi = n - 2;
    while (lo < hi) {
        const long long m = (lo + hi + 1) / 2;
        if (m * n - m * (m + 1) / 2 <= t) lo = m;
        else hi = m - 1;
    }
    return (int)lo;
}

template <int D>
__global__ __launch_bounds__(256) void gci_test(GciTestArgs A) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    unsigned long long mbits = kNoMargin;
    bool near = false, degenerate = false;
    if (t < A.n) {
        int32_t v[2 + D];
        if (A.items) {
#pragma unroll
            for (int k = 0; k < 2 + D; ++k) v[k] = A.items[t * (2 + D) + k];
        } else {
            const int i = pair_row(t, A.nvars);
            v[0] = i;
            v[1] = (int)(t - ((long long)i * A.nvars - (long long)i * (i + 1) / 2)) + i + 1;
        }
        const double r = fbn_gci_partial_r<D>(A.R, A.nvars, v);
        double m;
        const bool ind = fbn_gci_decide(r, A.tau, &m);
        if (A.r) A.r[t] = r;
        A.indep[t] = ind;
        degenerate = m < 0.0;
        if (!degenerate) mbits = fbn_margin_bits(m), near = fbn_margin_near(m);
    }
    const int lane = threadIdx.x & 63;
    fbn_margin_log_wave(A.stats, mbits, near, lane);
    const unsigned long long nd = __popcll(__ballot(degenerate));
    if (lane == 0 && nd) atomicAdd(A.stats + 2, nd);
}

}  // namespace

// d in 0..8, n >= 1; items: device (or mapped host) memory [n][2 + d], or null with d == 0 (n <= nvars
// (nvars - 1) / 2); stats: {min margin bits, near count, degenerate count}
extern "C" hipError_t fbn_gci_test_launch(const GciTestArgs *a, int d, hipStream_t s) {
    if (a->n <= 0) return hipSuccess;
    if (!a->items && (d != 0 || a->n > (long long)a->nvars * (a->nvars - 1) / 2)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a->n + 255) / 256)), block(256);
    switch (d) {
    case 0: hipLaunchKernelGGL(gci_test<0>, grid, block, 0, s, *a); break;
    case 1: hipLaunchKernelGGL(gci_test<1>, grid, block, 0, s, *a); break;
    case 2: hipLaunchKernelGGL(gci_test<2>, grid, block, 0, s, *a); break;
    case 3: hipLaunchKernelGGL(gci_test<3>, grid, block, 0, s, *a); break;
    case 4: hipLaunchKernelGGL(gci_test<4>, grid, block, 0, s, *a); break;
    case 5: hipLaunchKernelGGL(gci_test<5>, grid, block, 0, s, *a); break;
    case 6: hipLaunchKernelGGL(gci_test<6>, grid, block, 0, s, *a); break;
    case 7: hipLaunchKernelGGL(gci_test<7>, grid, block, 0, s, *a); break;
    case 8: hipLaunchKernelGGL(gci_test<8>, grid, block, 0, s, *a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
