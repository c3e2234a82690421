// hc_score.hip -- the family scores of a batch of counted family tables on gfx950.
//
// Input: the zeroed-then-counted 32-bit tables of param_counts.hip (FbnParamFamily descriptors, one
// table per family at tab + tab_off, [value][parent configuration]) and the host-built table L[n] =
// n ln n.  Output: two doubles per family, the log-likelihood and the score (hc_score.h).  Only those
// 16 bytes per family go back to the host; the tables stay on the device.
//
// One wave per family, kHcWaves families per workgroup.  Lane l takes the configurations j = l,
// l + 64, ...: for one value k adjacent lanes read adjacent counters, so a row of the table is one
// coalesced load per 64 configurations; the gather from L is data-dependent (not measured; most
// counters of a sparse table are small, so most gathers would hit the head of L).  The lane partial
// and the fold of the 64 partials are hc_score.h's, the very functions the host twin evaluates, in fp64 additions and subtractions only, so the result
// is the twin's bit for bit whatever batch, chunk or counting path produced the table.  No atomics;
// lane 0 writes the two results with ordinary vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hc_score.h"
#include "launchers.h"
#include "param_counts.h"

namespace {

constexpr int kHcWaves = 4;  // families per workgroup

__global__ __launch_bounds__(kHcWaves * kHcLanes) void hc_score_kernel(HcScoreArgs A) {
    const int lane = threadIdx.x & (kHcLanes - 1);
    const long long f = (long long)blockIdx.x * kHcWaves + (threadIdx.x >> 6);
    if (f >= A.nfam) return;  // uniform per wave
    const FbnParamFamily F = A.fam[f];
    const int q = A.fstr[F.coff];  // the child's key stride = its parent configurations
    const int r = F.cells / q;
    const double ll = fbn_hc_fold_wave(fbn_hc_lane_partial(A.tab + F.tab_off, r, q, lane, A.L));
    if (lane == 0) {
        A.out[2 * f] = ll;
        A.out[2 * f + 1] = ll - A.pen[f];
    }
}

}  // namespace

extern "C" hipError_t fbn_hc_score_launch(const HcScoreArgs *a, hipStream_t stream) {
    if (a->nfam <= 0 || (a->nfam + kHcWaves - 1) / kHcWaves > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hc_score_kernel, dim3((unsigned)((a->nfam + kHcWaves - 1) / kHcWaves)), dim3(kHcWaves * kHcLanes), 0,
                       stream, *a);
    return hipGetLastError();
}
