// ci_g2.h -- the G^2 arithmetic and the independence decision of the CI kernels, written once:
// ci_bits_g2.hip (both G^2 passes), ci_kernels.hip (tree and in-order paths) and pc_small.hip agree
// bit for bit because they evaluate these functions, not copies of them.
//
// The reference (ComputeGSquareXY / XYZ, src/IndependenceTest.cpp:65-155, 295-364) adds the term
// 2 O log(O / (C R / T)) of every cell with nonzero O, R, C, T into one running sum over z -> x -> y,
// adds (max(rows present, 1) - 1)(max(columns present, 1) - 1) per z slice to df, and decides:
// df == 0 is independent (p = 1); otherwise p = 1 - P(df / 2, G^2 / 2) (ci_chisq.h), independent iff
// p > alpha.  With a decision band ([lo, hi] per df 1..nband, then delta at band[2 nband];
// fbn_chisq_band) and no p wanted, G^2 outside [lo, hi] decides without evaluating p, and the
// logged margin |p - alpha| of such a test is delta.  Device-inline; internal to libfastbn.
#ifndef FBN_CI_G2_H
#define FBN_CI_G2_H

#include <hip/hip_runtime.h>

#include "ci_chisq.h"

// the term of a cell whose four operands are known to be nonzero (callers that keep the terms of a
// row independent evaluate it on placeholder operands and drop the result)
__device__ __forceinline__ double fbn_g2_term_nz(long observed, long sum_row, long sum_col, long total) {
    const double expected = (double)sum_col * (double)sum_row / (double)total;
    return 2.0 * observed * log(observed / expected);
}

// the term of any cell: 0 (skipped by the reference) if the cell, its row, its column or its slice is empty
__device__ __forceinline__ double fbn_g2_term(long observed, long sum_row, long sum_col, long total) {
    if (total == 0 || sum_row == 0 || sum_col == 0 || observed == 0) return 0.0;
    return fbn_g2_term_nz(observed, sum_row, sum_col, total);
}

// the adjusted df of one z slice with alx rows and aly columns present
__device__ __forceinline__ int fbn_g2_slice_df(int alx, int aly) {
    return ((alx >= 1 ? alx : 1) - 1) * ((aly >= 1 ? aly : 1) - 1);
}

// The p-value, explicitly out of line: inlined, the incomplete-gamma code triples the registers of
// every kernel that decides (the G^2 passes: 78-124 -> 215-258 VGPRs) for a call most tests skip.
__device__ __noinline__ inline double fbn_g2_pvalue(double g2, int df) { return fbn_chisq_pvalue(g2, df); }

struct G2Decision {
    int ind;        // 1 independent, 0 dependent, -1 undecided (fbn_g2_decide_tree only)
    double p;       // the p-value; alpha +- delta where the band decided
    double margin;  // |p - alpha|; delta itself where the band decided
};

// the reference's decision from the in-order sum g2 (band == nullptr or want_p: p always evaluated)
__device__ __forceinline__ G2Decision fbn_g2_decide(double g2, int df, double alpha, const double *band, int nband,
                                                    bool want_p) {
    if (df == 0) return G2Decision{1, 1.0, fabs(1.0 - alpha)};  // src/IndependenceTest.cpp:140-142, 349-351
    if (!want_p && band && df <= nband && g2 < band[2 * df - 2])
        return G2Decision{1, alpha + band[2 * nband], band[2 * nband]};  // p > alpha + delta
    if (!want_p && band && df <= nband && g2 > band[2 * df - 1])
        return G2Decision{0, alpha - band[2 * nband], band[2 * nband]};  // p < alpha - delta
    const double p = fbn_g2_pvalue(g2, df);
    return G2Decision{p > alpha ? 1 : 0, p, fabs(p - alpha)};
}

// Tree and in-order sums of the same `cells` terms differ by at most (cells + 64) u sum|t| (ga = the
// sum of the terms' magnitudes)
__device__ __forceinline__ double fbn_g2_tree_err(int cells, double ga) { return (cells + 64) * 2.3e-16 * ga; }

// the decision from a tree sum gs of the terms (decision-only batches with a band): a tree sum that
// clears the band by the bound above decides exactly as the in-order sum would; otherwise undecided
// (ind = -1) and the caller sums in order and calls fbn_g2_decide
__device__ __forceinline__ G2Decision fbn_g2_decide_tree(double gs, double ga, int df, int cells, double alpha,
                                                         const double *band, int nband) {
    if (df == 0) return G2Decision{1, 1.0, fabs(1.0 - alpha)};
    if (band && df <= nband) {
        const double err = fbn_g2_tree_err(cells, ga);
        if (gs + err < band[2 * df - 2]) return G2Decision{1, alpha + band[2 * nband], band[2 * nband]};
        if (gs - err > band[2 * df - 1]) return G2Decision{0, alpha - band[2 * nband], band[2 * nband]};
    }
    return G2Decision{-1, 0.0, 0.0};
}

// ---- the decision-margin log: stats[0] = min over tests of the margin as IEEE bits (non-negative
// doubles order like their bit patterns), stats[1] = tests with a margin below 1e-9
constexpr unsigned long long kNoMargin = ~0ull;  // a lane without a test
__device__ __forceinline__ unsigned long long fbn_margin_bits(double m) {
    return (unsigned long long)__double_as_longlong(m);
}
__device__ __forceinline__ bool fbn_margin_near(double m) { return m < 1e-9; }

// one thread logs one test
__device__ __forceinline__ void fbn_margin_log(unsigned long long *stats, double m) {
    atomicMin(stats, fbn_margin_bits(m));
    if (fbn_margin_near(m)) atomicAdd(stats + 1, 1ull);
}

// a whole wave logs its lanes' tests (mbits = kNoMargin, near = false in lanes without one): one
// atomic pair per wave
__device__ __forceinline__ void fbn_margin_log_wave(unsigned long long *stats, unsigned long long mbits, bool near,
                                                    int lane) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long v = __shfl_xor(mbits, o);
        mbits = v < mbits ? v : mbits;
    }
    const unsigned long long nn = __popcll(__ballot(near));
    if (lane == 0) {
        if (mbits != kNoMargin) atomicMin(stats, mbits);
        if (nn) atomicAdd(stats + 1, nn);
    }
}

#endif
