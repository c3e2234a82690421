// gscore.hip -- batches of Gaussian family scores on the device (gscore.h, the functions the host twin
// evaluates too): one family per lane, the kernel templated on the parent count p (0..8) and on the score,
// fully unrolled, so the (p + 1)(p + 2) / 2 gathered entries of R and their elimination live in registers
// (p = 8: 126 VGPRs under the log-likelihood score, 218 under BGe with its second elimination, no scratch).
//
// A bucket of one size arrives as fixed-stride records (out_index, child, parents ascending); a lane writes its
// two results at out_index, the family's place in the caller's batch, so the buckets of a mixed batch need no
// gather pass.  Every wave takes one ballot for its degenerate families and at most one atomic.
//
// R is gathered from global memory, as gci_test.hip does: the gathers of a family are independent loads issued
// together, and the kernel is bound by its fp64 divisions and logarithms, not by them.  A variant that first
// staged R's packed upper triangle in LDS on a persistent grid was measured slower and is not kept (DESIGN.md
// 5.20 has the numbers).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "launchers.h"

namespace {

constexpr int kBlock = 256;

template <int P, bool BGE>
__global__ __launch_bounds__(kBlock) void gscore(GscoreArgs A) {
    const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    bool degenerate = false;
    if (t < A.n) {
        const int32_t *rec = A.rec + t * (2 + P);
        int32_t f[1 + P];
#pragma unroll
        for (int k = 0; k < 1 + P; ++k) f[k] = rec[1 + k];
        double ll, sc;
        degenerate = !fbn_gs_family<P, BGE>(FbnGsFull{A.R, A.nvars}, f, A.lss, A.tq, A.C, &ll, &sc);
        const long long o = rec[0];
        A.loglik[o] = ll;
        A.score[o] = sc;
    }
    const unsigned long long nd = __popcll(__ballot(degenerate));
    if ((threadIdx.x & 63) == 0 && nd) atomicAdd(A.degenerate, nd);
}

template <int P>
hipError_t launch_p(const GscoreArgs &a, int bge, hipStream_t s) {
    const dim3 g((unsigned)((a.n + kBlock - 1) / kBlock)), b(kBlock);
    if (bge) hipLaunchKernelGGL((gscore<P, true>), g, b, 0, s, a);
    else hipLaunchKernelGGL((gscore<P, false>), g, b, 0, s, a);
    return hipGetLastError();
}

}  // namespace

// p in 0..8, 1 <= a->n < 2^31; every record's indices lie in their ranges (the caller validated them)
extern "C" hipError_t fbn_gscore_launch(const GscoreArgs *a, int p, int bge, hipStream_t s) {
    if (a->n <= 0) return hipSuccess;
    if (a->n > 0x7fffffffll) return hipErrorInvalidValue;
    switch (p) {
    case 0: return launch_p<0>(*a, bge, s);
    case 1: return launch_p<1>(*a, bge, s);
    case 2: return launch_p<2>(*a, bge, s);
    case 3: return launch_p<3>(*a, bge, s);
    case 4: return launch_p<4>(*a, bge, s);
    case 5: return launch_p<5>(*a, bge, s);
    case 6: return launch_p<6>(*a, bge, s);
    case 7: return launch_p<7>(*a, bge, s);
    case 8: return launch_p<8>(*a, bge, s);
    default: return hipErrorInvalidValue;
    }
}
