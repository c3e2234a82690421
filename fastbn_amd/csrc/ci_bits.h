// ci_bits.h -- what the bit-sliced CI kernel files (ci_bits_count.hip, ci_bits_gram.hip,
// ci_bits_g2.hip, ci_l1.hip) share: the count record, the pair decode, the XCD work split, the
// completion of a pair table, and the host functions through which one file launches another's
// kernels (a kernel is launched only from the file that defines it).  Internal to libfastbn.
#ifndef FBN_CI_BITS_H
#define FBN_CI_BITS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ci_args.h"

constexpr int kBitsCells = 64;  // count slots per test

// launches of at most this many tests use the four-lane G^2 pass (ci_bits_g2q)
constexpr long long kG2QuadMax = 16384;

namespace fbn {
// ci_bits_g2.hip: G^2, df, p and the decision of a.n tests with d <= 1 conditioning variables from
// their count records; quad: four lanes per test (ci_bits_g2q), else one (ci_bits_g2)
hipError_t CiG2Launch(const CiG2Args &a, int d, bool quad, int num_cu, hipStream_t s);
// ci_bits_g2.hip: g2[t] = G^2 of pair t's level-0 table, every pair of the complete graph over nv variables
hipError_t CiPairG2Launch(const int32_t *pairtab, const int32_t *dims, int nv, double *g2, hipStream_t s);
// ci_bits_count.hip: the derived counting of a's d = 1 tests (a.pairtab read); n_dev != nullptr: the
// test count is read on the device (at most a.n)
hipError_t CiCountDerivedLaunch(const CiBitsArgs &a, const long long *n_dev, hipStream_t s);
}  // namespace fbn

// test t is the (t0 + t)-th pair (x < y) of the complete graph over nv variables in lexicographic
// order (a PC run's level 0, or one rank's range of it), decoded instead of read
__device__ __forceinline__ void pair_of(long long t, int nv, int &x, int &y) {
    const double b = 2.0 * nv - 1.0;
    long long i = (long long)((b - sqrt(b * b - 8.0 * (double)t)) * 0.5);
    auto off = [&](long long r) { return r * nv - r * (r + 1) / 2; };
    if (i < 0) i = 0;
    while (i > 0 && off(i) > t) --i;
    while (i + 1 < nv && off(i + 1) <= t) ++i;
    x = (int)i;
    y = (int)(t - off(i) + i + 1);
}

// XCD-contiguous work split: workgroups are dispatched round-robin over the 8 XCDs (block b on XCD
// b % 8), each with its own L2.  Cutting the n units into 8 contiguous ranges, range j worked by
// XCD j's blocks in order, keeps consecutive units -- an edge's candidate conditioning variables,
// which share the x and y mask rows -- in one L2 at about the same time.  xcd = 0: plain grid stride.
struct XcdSplit {
    long long first, end, stride;
};
__device__ __forceinline__ XcdSplit xcd_split(long long n, int wave, int per_block, int xcd) {
    const long long G = gridDim.x, b = blockIdx.x;
    if (!xcd || G < 8) return {b * per_block + wave, n, G * per_block};
    const long long j = b % 8, nb = (G - j + 7) / 8, i = b / 8;
    return {n * j / 8 + i * per_block + wave, n * (j + 1) / 8, nb * per_block};
}

// The pair table N[a][b] (Counts2D::FillTable, src/CellTable.cpp:430-455) from its leading cells
// lead(a, b), a < DX-1, b < DY-1: the masks of a variable partition the samples, so the last value's
// row and column follow exactly from the per-value sample counts cx / cy of x and y
// (ci_bits_rowcount) -- N[a][DY-1] = cx[a] - sum_b N[a][b], N[DX-1][b] = cy[b] - sum_a N[a][b]
template <int DX, int DY, class Lead>
__device__ __forceinline__ void complete_pair(Lead lead, const int32_t *__restrict__ cx, const int32_t *__restrict__ cy,
                                              int32_t (&full)[DX * DY]) {
    constexpr int MX = DX - 1, MY = DY - 1;
#pragma unroll
    for (int i = 0; i < MX; ++i) {
        int32_t r = cx[i];
#pragma unroll
        for (int j = 0; j < MY; ++j) full[i * DY + j] = lead(i, j), r -= full[i * DY + j];
        full[i * DY + MY] = r;
    }
#pragma unroll
    for (int j = 0; j < DY; ++j) {
        int32_t r = cy[j];
#pragma unroll
        for (int i = 0; i < MX; ++i) r -= full[i * DY + j];
        full[MX * DY + j] = r;
    }
}

#endif
