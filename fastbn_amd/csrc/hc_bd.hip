// hc_bd.hip -- the Bayesian Dirichlet scores (BDeu, K2) of a batch of counted family tables on gfx950.
//
// Input: the counted 32-bit tables and FbnParamFamily descriptors exactly as hc_score.hip receives them,
// plus two FbnBdPrior records per family (hc_bd.h: the Dirichlet parameter of a cell and of a parent
// configuration with their host-computed Stirling constants).  Output: two doubles per family, the
// log-likelihood (hc_score.h's, from the resident n ln n table: the BIC path's bits) and the BD score.
//
// Why not hc_score.hip's split.  There a counter costs one gather and one add, so a wave whose 64 lanes
// mostly idle (q = 1 .. 4: nearly every family of a first sweep) costs nothing worth saving.  Here every
// non-zero counter costs a logarithm with an fp64 division, about two orders of magnitude more, and an idle
// lane is an idle fp64 pipe.  So the work is split by the family's width:
//
//   class c = 0 .. 5: q <= w = 2^c (the least such c).  The family gets a sub-group of w adjacent lanes
//                     of a wave, lane s of it the configuration j = s; 64 / w families share a wave.
//   class 6:          q > 32.  One wave per family, lane l over j = l, l + 64, ... (hc_score.hip's split).
//
// The host bins a chunk's families by class (fbn_hc_bd_bin) into one index list; one launch covers all
// classes, a workgroup finding its class from the table of first workgroups in the argument record.
// Within a value row k the sub-group's lanes read adjacent counters, and adjacent sub-groups read the rows
// of different tables: coalesced per sub-group, as per wave before.  A zero counter costs a compare.
//
// The packed fold gives hc_bd.h's bits.  The header folds 64 partials p[0 .. 63] at the offsets 32, 16, ..,
// 1: p[l] += p[l + off] for l < off, where p[l] = +0.0 for l >= q.  Take a family of class c < 6, so q <= w =
// 2^c.  Claim: before every step with off >= w, p[l] has its original bits for l < w and is +0.0 for l >= w.
// It holds at the start.  Such a step adds to p[l], l < off, the entry p[l + off] with l + off >= w, which
// is +0.0 by the claim; x + (+0.0) = x for every x but -0.0, no partial is -0.0 (hc_bd.h), and +0.0 + +0.0
// = +0.0: the claim holds after the step.  The remaining steps w/2 .. 1 read and write indices below w
// only, starting from the original bits.  The sub-group performs exactly these steps on exactly these
// values: __shfl_down of width w hands lane s < off the value of lane s + off < 2 off <= w of its own
// sub-group, which the step before left correct (induction from off = w/2 down), so its lane 0 ends with
// the header's p[0].  Lanes s >= off hold values that nothing reads.  For w = 1 there is no step.  Class 6
// is the header's fold itself (width 64).  tests/test_gpu_bd.py holds pack = 1 to pack = 0 and to the twin.
//
// No atomics, no LDS (a per-sub-group cache of D(1 .. T, a_cell) was not built: nothing measured asks for
// it); the first lane of a sub-group writes the two results with ordinary vector stores at the family's
// index in the chunk.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hc_bd.h"
#include "launchers.h"
#include "param_counts.h"

namespace {

constexpr int kBdWaves = 4;  // waves per workgroup

// the fold of the partials of a sub-group of 2^C lanes: its first lane returns the header's p[0]
template <int C>
__device__ __forceinline__ double fold_sub(double v) {
#pragma unroll
    for (int off = (1 << C) >> 1; off >= 1; off >>= 1) v += __shfl_down(v, off, 1 << C);
    return v;
}

// one wave of class C: 64 >> C families (C < 6), or one (C == 6); `wave` counts the class's waves
template <int C>
__device__ __forceinline__ void score_wave(const HcBdArgs &A, long long wave, int lane) {
    constexpr int kShift = C < 6 ? C : 6;
    constexpr int kPer = 64 >> kShift;  // families per wave
    const int sub = lane & ((1 << kShift) - 1);
    const long long slot = wave * kPer + (lane >> kShift);
    const bool live = slot < A.cls_count[C];  // uniform per sub-group
    double ll = 0.0, sc = 0.0;
    long long f = 0;
    if (live) {
        f = A.order[A.cls_first[C] + slot];
        const FbnParamFamily F = A.fam[f];
        const int q = A.fstr[F.coff];  // the child's key stride = its parent configurations
        const int r = F.cells / q;
        const uint32_t *tab = A.tab + F.tab_off;
        const FbnBdPrior cell = A.prior[2 * f], cfg = A.prior[2 * f + 1];
        ll = fbn_hc_lane_partial(tab, r, q, sub, A.L);
        sc = fbn_bd_lane_partial(tab, r, q, sub, cell, cfg);
    }
    // every lane of the wave takes part in the shuffles; a sub-group without a family folds zeros
    ll = fold_sub<kShift>(ll);
    sc = fold_sub<kShift>(sc);
    if (live && sub == 0) {
        A.out[2 * f] = ll;
        A.out[2 * f + 1] = sc;
    }
}

__global__ __launch_bounds__(kBdWaves * kHcLanes) void hc_bd_kernel(HcBdArgs A) {
    const int lane = threadIdx.x & (kHcLanes - 1);
    int c = 0;
    while (c < kBdClasses - 1 && (long long)blockIdx.x >= A.cls_block[c + 1]) ++c;  // uniform per workgroup
    const long long wave = ((long long)blockIdx.x - A.cls_block[c]) * kBdWaves + (threadIdx.x >> 6);
    switch (c) {
    case 0: score_wave<0>(A, wave, lane); break;
    case 1: score_wave<1>(A, wave, lane); break;
    case 2: score_wave<2>(A, wave, lane); break;
    case 3: score_wave<3>(A, wave, lane); break;
    case 4: score_wave<4>(A, wave, lane); break;
    case 5: score_wave<5>(A, wave, lane); break;
    default: score_wave<6>(A, wave, lane); break;
    }
}

}  // namespace

// families [0, nfam) with q[f] parent configurations -> order[nfam], their indices sorted by class (stable),
// and the class counts / first entries / first workgroups of `a`; pack == 0: every family in class 6
extern "C" void fbn_hc_bd_bin(const int32_t *q, long long nfam, int pack, int32_t *order, HcBdArgs *a) {
    auto cls = [&](int32_t qq) {
        if (!pack || qq > 32) return kBdClasses - 1;
        int c = 0;
        while ((1 << c) < qq) ++c;
        return c;
    };
    for (int c = 0; c <= kBdClasses; ++c) a->cls_count[c] = a->cls_first[c] = a->cls_block[c] = 0;
    for (long long f = 0; f < nfam; ++f) ++a->cls_count[cls(q[f])];
    for (int c = 0; c < kBdClasses; ++c) {
        const long long per = c < 6 ? 64 >> c : 1;
        const long long waves = (a->cls_count[c] + per - 1) / per;
        a->cls_first[c + 1] = a->cls_first[c] + a->cls_count[c];
        a->cls_block[c + 1] = a->cls_block[c] + (waves + kBdWaves - 1) / kBdWaves;
    }
    long long at[kBdClasses];
    for (int c = 0; c < kBdClasses; ++c) at[c] = a->cls_first[c];
    for (long long f = 0; f < nfam; ++f) order[at[cls(q[f])]++] = (int32_t)f;
    a->nfam = nfam;
}

extern "C" hipError_t fbn_hc_bd_launch(const HcBdArgs *a, hipStream_t stream) {
    const long long blocks = a->cls_block[kBdClasses];
    if (a->nfam <= 0 || blocks <= 0 || blocks > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hc_bd_kernel, dim3((unsigned)blocks), dim3(kBdWaves * kHcLanes), 0, stream, *a);
    return hipGetLastError();
}
