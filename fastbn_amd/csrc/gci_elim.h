// gci_elim.h -- the partial correlation of one Gaussian conditional-independence test, written once: the
// device kernel (gci_test.hip) and the host twin (gci_host.cpp) agree bit for bit because they evaluate
// this function, not copies of it.
//
// A test (x, y | z_0 .. z_{d-1}) reads the (d + 2)(d + 3) / 2 upper entries of the correlation matrix R for
// the variable order (Z.., x, y) into a packed working triangle W.  The d pivots of Z are eliminated
// without square roots (LDL^T): for pivot k, row i > k gets l = W[k][i] / W[k][k], and its entries j >= i
// lose l * W[k][j] -- only entries of the trailing triangle, which the later pivots and the final 2 x 2
// block still need.  The 2 x 2 Schur complement (a c; c b) of (x, y) then gives
//     r = c / sqrt(a b),  clamped to [-1, 1].
// A pivot <= 2^-40 (R_ZZ singular or nearly so; likewise a <= 2^-40 or b <= 2^-40: x or y is a linear
// function of Z within rounding) makes the test degenerate: r = NaN, and every comparison of the decision
// |r| <= tau is then false, so the test counts as dependent.
//
// Only + - * / and sqrt are used, which IEEE-754 rounds correctly, hence identically on both sides.
// Contraction is switched off in the function body (hc_bd.h's way), and the library's translation units
// are built with -ffp-contract=off and without fast-math besides.  D is a template parameter and every
// loop bound a constant, so the device instantiation is fully unrolled and W lives in registers
// (55 doubles at d = 8: DESIGN.md 5.17 lists the compiler's register and scratch figures).
#ifndef FBN_GCI_ELIM_H
#define FBN_GCI_ELIM_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FBN_GCI_HD __host__ __device__
#else
#define FBN_GCI_HD
#endif

#if defined(__clang__)
#define FBN_GCI_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define FBN_GCI_NO_CONTRACT
#if defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif
#endif

constexpr int kGciMaxD = 8;               // conditioning variables per test (pc_search.h's kMaxD)
constexpr double kGciPivotMin = 0x1p-40;  // a pivot at or below it: the test is degenerate

// packed upper triangle of an M x M matrix: entry (i <= j)
template <int M>
FBN_GCI_HD constexpr int fbn_gci_tri(int i, int j) {
    return i * M - i * (i - 1) / 2 + (j - i);
}

// r of the test v = (x, y, z_0 .. z_{D-1}) on R [n][ld]; NaN when degenerate
template <int D>
FBN_GCI_HD inline double fbn_gci_partial_r(const double *__restrict__ R, long long ld, const int32_t *v) {
    FBN_GCI_NO_CONTRACT
    constexpr int M = D + 2;
    // order (Z.., x, y): position k < D is z_k = v[2 + k], position D is x, D + 1 is y
    long long row[M];
#pragma unroll
    for (int k = 0; k < M; ++k) row[k] = (long long)v[k < D ? 2 + k : k - D];
    double W[M * (M + 1) / 2];
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = i; j < M; ++j) W[fbn_gci_tri<M>(i, j)] = R[row[i] * ld + row[j]];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const double piv = W[fbn_gci_tri<M>(k, k)];
        ok = ok && piv > kGciPivotMin;
#pragma unroll
        for (int i = k + 1; i < M; ++i) {
            const double l = W[fbn_gci_tri<M>(k, i)] / piv;
#pragma unroll
            for (int j = i; j < M; ++j) W[fbn_gci_tri<M>(i, j)] = W[fbn_gci_tri<M>(i, j)] - l * W[fbn_gci_tri<M>(k, j)];
        }
    }
    const double a = W[fbn_gci_tri<M>(D, D)], b = W[fbn_gci_tri<M>(D + 1, D + 1)], c = W[fbn_gci_tri<M>(D, D + 1)];
    ok = ok && a > kGciPivotMin && b > kGciPivotMin;
    double r = c / sqrt(a * b);
    r = r > 1.0 ? 1.0 : r;
    r = r < -1.0 ? -1.0 : r;
    return ok ? r : __builtin_nan("");
}

// the decision and its margin: independent iff |r| <= tau (false for a degenerate test, whose margin is
// not logged: *margin = -1)
FBN_GCI_HD inline bool fbn_gci_decide(double r, double tau, double *margin) {
    FBN_GCI_NO_CONTRACT
    const double ar = r < 0.0 ? -r : r;
    const double m = ar - tau;
    *margin = r != r ? -1.0 : (m < 0.0 ? -m : m);
    return ar <= tau;
}

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif

#endif
