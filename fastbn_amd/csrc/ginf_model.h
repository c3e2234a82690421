// ginf_model.h -- exact conditioning of a linear-Gaussian network's joint N(mu, Sigma) on one evidence case,
// written once: the kernel (ginf.hip) and the host twin (ginf_host.cpp) agree bit for bit because they
// evaluate these functions, not copies of them.  include/fastbn.h states the model and the conventions.
//
// With E the observed indices in ascending order (m of them), every number of a case is one recurrence,
//     elim(s, p, q, j, piv) = (s - sum_{k<j} p_k q_k) / piv,       the sum from +0.0 with k ascending:
//   L_ij = elim(Sigma[e_i][e_j], L_i, L_j, j, L_jj)   i > j     the left-looking Cholesky factor of Sigma_EE
//   a_j  = elim(x_{e_j} - mu_{e_j}, a, L_j, j, L_jj)            L a = delta: delta is one more row below L
//   y_i  = elim(Sigma[e_i][u], L_i, y, i, L_ii)                 L y = Sigma_Eu for an unobserved u
// and three running sums of squares or products in the same ascending order: d_j = Sigma[e_j][e_j] - sum_k
// L_jk^2 with L_jj = sqrt(d_j), a . a, and per u y . a and y . y.  A row's sum of squares grows by one term
// whenever the row gains an entry, so whoever owns a row keeps it in a register and the diagonal costs nothing.
//
// Only + - * / sqrt and hc_bd.h's own logarithm are used: IEEE-754 rounds the first five correctly, the
// logarithm is built from them, so both sides round alike.  Contraction is switched off in every function
// below (hc_bd.h's way), and the library is built with -ffp-contract=off and without fast-math besides.
//
// The kernel's LDS plan lives here too, because the handle reports it and sizes the launch with it.
#ifndef FBN_GINF_MODEL_H
#define FBN_GINF_MODEL_H

#include "hc_bd.h"

#define FBN_GINF_HD FBN_HC_HD

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

constexpr int kGinfMaxObs = 128;             // observed variables per case
constexpr int kGinfMaxVars = 8192;           // variables: index lists of 16-bit entries, Sigma of 512 MiB
constexpr double kGinfDegenerate = 0x1p-40;  // d_j <= this * Sigma[e_j][e_j]: the case is degenerate
constexpr double kGinfLn2Pi = 1.8378770664093453;

// packed lower triangle, row-major: entry (i >= j)
FBN_GINF_HD constexpr int fbn_ginf_tri(int i, int j) { return i * (i + 1) / 2 + j; }

// (s - sum_{k<j} p[k sp] q[k sq]) / piv
FBN_GINF_HD inline double fbn_ginf_elim(double s, const double *p, int sp, const double *q, int sq, int j, double piv) {
    FBN_BD_NO_CONTRACT
    double acc = 0.0;
    for (int k = 0; k < j; ++k) acc = acc + p[k * sp] * q[k * sq];
    return (s - acc) / piv;
}

// acc + x y: one more term of a running sum
FBN_GINF_HD inline double fbn_ginf_more(double acc, double x, double y) {
    FBN_BD_NO_CONTRACT
    return acc + x * y;
}

// d_j of a row whose squares sum to sq, and whether it makes the case degenerate (a NaN does)
FBN_GINF_HD inline double fbn_ginf_diag(double sigma_jj, double sq, bool *degenerate) {
    FBN_BD_NO_CONTRACT
    const double d = sigma_jj - sq;
    *degenerate = !(d > kGinfDegenerate * sigma_jj);
    return d;
}

// log p(e) = -(m ln 2 pi + sum_j ln d_j + a . a) / 2; +0.0 without evidence
FBN_GINF_HD inline double fbn_ginf_logp(int m, const double *d, double aa) {
    FBN_BD_NO_CONTRACT
    if (m == 0) return 0.0;
    double s = 0.0;
    for (int j = 0; j < m; ++j) s = s + fbn_bd_ln(d[j]);
    return -0.5 * (((double)m * kGinfLn2Pi + s) + aa);
}

// the posterior of an unobserved u from its prior and the two sums over its y
FBN_GINF_HD inline void fbn_ginf_posterior(double mu_u, double sigma_uu, double ya, double yy, double *mean, double *var) {
    FBN_BD_NO_CONTRACT
    const double v = sigma_uu - yy;
    *mean = mu_u + ya;
    *var = v < 0.0 ? 0.0 : v;
}

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif

// ---- the kernel's LDS plan: what does not depend on m, then L, then the tile's y
// a [128] and d [128] doubles, E [128] and U [n] 16-bit indices, the waves' counts of the prefix sum and two flags
FBN_GINF_HD constexpr int fbn_ginf_lds_fixed(int n) { return 2 * kGinfMaxObs * 8 + kGinfMaxObs * 2 + 64 + 16 + ((2 * n + 7) & ~7); }
FBN_GINF_HD constexpr int fbn_ginf_lds_tri(int m) { return m * (m + 1) / 2 * 8; }
// lanes of a tile of unobserved variables: the largest multiple of 64 up to 256 whose y [m][T] fits beside L
FBN_GINF_HD constexpr int fbn_ginf_tile(int lds_bytes, int n, int m) {
    const int room = (lds_bytes - fbn_ginf_lds_fixed(n) - fbn_ginf_lds_tri(m)) / (8 * (m > 0 ? m : 1)) / 64 * 64;
    return room > 256 ? 256 : room;
}
// the launch's LDS for a batch whose largest case observes m_max: T = 256 there if the CU's 160 KiB allow it
// (a batch without evidence still asks for one row of y, so that fbn_ginf_tile has room to report)
FBN_GINF_HD constexpr int fbn_ginf_lds_bytes(int n, int m_max) {
    const int want = fbn_ginf_lds_fixed(n) + fbn_ginf_lds_tri(m_max) + 8 * (m_max > 0 ? m_max : 1) * 256;
    return want > 160 * 1024 ? 160 * 1024 : want;
}

#endif
