// gscore.h -- the Gaussian family scores of the score-based learners on continuous data, written once: the
// device kernel (gscore.hip) and the host twin (gscore_host.cpp) agree bit for bit because they evaluate
// these functions, not copies of them.
//
// A family is a child v with parents P ascending, p = |P| <= kGciMaxD.  The (p + 1)(p + 2) / 2 upper entries of
// the correlation matrix R over the order (P.., v) are gathered into a packed working triangle and eliminated
// without square roots in gci_elim.h's operation order; the pivots are d_0 .. d_{p-1} and d_p, the child's.
// Every entry is read as R[min][max], the upper triangle.
//
// Gaussian log-likelihood (kGsLL).  With lss[v] = ln(S_vv / N):
//     loglik = Kll - (N / 2) (lss[v] + ln d_p),   Kll = -(N / 2)(ln 2 pi + 1)
//     score  = loglik - pen[p],                   pen[p] = penalty (p + 2)
// BGe (kGsBGE; Kuipers, Moffa & Heckerman 2014, prior mean = sample mean, so the posterior matrix is t I + S).
// The pivots are those of the scaled matrix R + diag(tq), tq[i] = t / S_ii; with h[p] = (c + p + 1) / 2:
//     score = K[p] - (ln(d_0 d_1 .. d_{p-1}) + sum_P lss) / 2 - h[p] (ln d_p + lss[v])
//     K[p]  = -(N/2) ln pi + ln(a_mu / (N + a_mu)) / 2 + lnGamma((c + p + 1) / 2) - lnGamma((c0 + p + 1) / 2)
//             + ((c0 + 2 p + 1) / 2) ln t - (p / 2 + h[p]) ln N
// (ln S_ii = lss[i] + ln N: the ln N terms are folded into K[p], so what the evaluator adds to K[p] is small
// against it and nothing large cancels).  The product of the pivots takes one logarithm instead of p; it
// cannot underflow (each pivot exceeds 2^-40).  The loglik of a BGe call is the Gaussian one above, from a
// first elimination of the unscaled R.
//
// Tables.  Everything that depends on N, n, p or one variable alone is data computed once on the host
// (gscore_host.cpp, in long double, rounded once) and handed to both sides: FbnGsConsts and lss, tq [n].
// The evaluator calls no maths library: + - * / and hc_bd.h's fbn_bd_ln only, contraction off.
//
// Degenerate: a pivot <= kGciPivotMin in either elimination (a parent or the child is a linear function of
// the others within rounding): loglik = score = -inf, and the function returns false so the caller counts it.
#ifndef FBN_GSCORE_H
#define FBN_GSCORE_H

#include "gci_elim.h"
#include "hc_bd.h"

enum { kGsLL = 0, kGsBGE = 1 };

struct FbnGsConsts {
    double K[kGciMaxD + 1], h[kGciMaxD + 1];  // BGe
    double pen[kGciMaxD + 1];                 // log-likelihood score
    double Kll, halfN;
};

// the source of R's entries
struct FbnGsFull {
    const double *R;
    long long ld;
    FBN_GCI_HD double operator()(int a, int b) const {
        const int lo = a < b ? a : b, hi = a < b ? b : a;
        return R[lo * ld + hi];
    }
};

// the pivots of f = (child, parents ascending): *prod = d_0 .. d_{P-1} multiplied in that order (1 when P == 0),
// *dp = the child's; SCALED: add[i] is added to the diagonal first.  False when a pivot is <= kGciPivotMin.
template <int P, bool SCALED, class Get>
FBN_GCI_HD inline bool fbn_gs_pivots(const Get &get, const int32_t *f, const double *add, double *prod, double *dp) {
    FBN_GCI_NO_CONTRACT
    constexpr int M = P + 1;
    int row[M];
#pragma unroll
    for (int k = 0; k < M; ++k) row[k] = f[k < P ? 1 + k : 0];
    double W[M * (M + 1) / 2];
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = i; j < M; ++j) W[fbn_gci_tri<M>(i, j)] = get(row[i], row[j]);
    if (SCALED) {
#pragma unroll
        for (int i = 0; i < M; ++i) W[fbn_gci_tri<M>(i, i)] = W[fbn_gci_tri<M>(i, i)] + add[row[i]];
    }
    bool ok = true;
    double pr = 1.0;
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const double piv = W[fbn_gci_tri<M>(k, k)];
        ok = ok && piv > kGciPivotMin;
        pr = pr * piv;
#pragma unroll
        for (int i = k + 1; i < M; ++i) {
            const double l = W[fbn_gci_tri<M>(k, i)] / piv;
#pragma unroll
            for (int j = i; j < M; ++j) W[fbn_gci_tri<M>(i, j)] = W[fbn_gci_tri<M>(i, j)] - l * W[fbn_gci_tri<M>(k, j)];
        }
    }
    const double d = W[fbn_gci_tri<M>(P, P)];
    *prod = pr;
    *dp = d;
    return ok && d > kGciPivotMin;
}

// loglik and score of f; false (and -inf twice) for a degenerate family
template <int P, bool BGE, class Get>
FBN_GCI_HD inline bool fbn_gs_family(const Get &get, const int32_t *f, const double *lss, const double *tq,
                                     const FbnGsConsts &C, double *loglik, double *score) {
    FBN_GCI_NO_CONTRACT
    double prod, dp;
    bool ok = fbn_gs_pivots<P, false>(get, f, nullptr, &prod, &dp);
    const double lv = lss[f[0]];
    const double ll = C.Kll - C.halfN * (lv + fbn_bd_ln(dp));
    double sc;
    if (BGE) {
        ok = fbn_gs_pivots<P, true>(get, f, tq, &prod, &dp) && ok;
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < P; ++k) acc = acc + lss[f[1 + k]];
        const double lp = P ? fbn_bd_ln(prod) : 0.0;
        sc = (C.K[P] - 0.5 * (lp + acc)) - C.h[P] * (fbn_bd_ln(dp) + lv);
    } else {
        sc = ll - C.pen[P];
    }
    const double ninf = -__builtin_inf();
    *loglik = ok ? ll : ninf;
    *score = ok ? sc : ninf;
    return ok;
}

#endif
