// hc_bd.h -- the Bayesian Dirichlet family score (BDeu, K2) of the score-based learners, written once: the
// device reduction (hc_bd.hip) and the host twin (hc_search.cpp) agree bit for bit because they evaluate
// these functions, not copies of them.
//
// A family is a child with r states and q parent configurations (the full product of the parents' state
// counts); its counts N_jk lie in fbn_param_counts' layout, tab[k * q + j]; N_j = sum_k N_jk.  With
//     D(n, a) = lnGamma(a + n) - lnGamma(a)
//     score   = sum_jk D(N_jk, a_cell) - sum_j D(N_j, a_cfg)
// BDeu(iss): a_cell = iss / (r q), a_cfg = iss / q.  K2: a_cell = 1, a_cfg = r.  Both are formed on the
// host per family (fbn_bd_alphas) and travel with it as two FbnBdPrior records (fbn_bd_prior).
//
// Bit identity.  No log, lgamma or log1p of any library is called: those differ between host and device.
// fbn_bd_ln is an own logarithm (exponent and mantissa split by bit manipulation, then a fixed
// polynomial) and D is built on it from + - * / alone, which IEEE-754 rounds correctly, hence identically,
// on both sides.  Contraction is switched off in every function below, so no compiler forms an FMA that was
// not written (none is); the library's translation units are built with -ffp-contract=off and without
// fast-math besides.
//
// D(n, a), n >= 1 (D(0, a) = +0.0 is never evaluated: a zero counter costs a compare):
//   a < 16, n < kBdDirect:  ln(a (a+1) ... (a+n-1)), one logarithm of a product of at most 15 factors
//                           below 31 (no overflow; each multiply adds 2^-53 relative, nothing cancels).
//                           Below a = 2^-32 the factor a is taken out: ln(a) + ln((a+1) ... (a+n-1)).
//   otherwise:              head + (S(a + n) - s0), S(x) = (x - 1/2) ln x - x + the Stirling series in 1/x
//                           through x^-9 (x >= 16: the first dropped term is below 1.2e-16);
//                           a < 16:  head = D(kBdDirect, a) by the product form, s0 = S(a + kBdDirect)
//                           a >= 16: head = 0, s0 = S(a).
//   head and s0 depend on a alone: FbnBdPrior carries them, computed on the host by these very functions.
// The difference of two S values cancels when n is small against a; what is lost is 2^-53 of the lnGamma
// magnitudes, the unit the twin's error bound is stated in (1e-12 of them: DESIGN.md 5.15).
//
// Summation order, hc_score.h's extended: 64 lane partials, lane l over the configurations j = l, l + 64,
// ... ascending; per configuration the values k ascending (+ D(N_jk, a_cell) for each non-zero counter,
// N_j summed as an integer), then - D(N_j, a_cfg) if N_j is non-zero.  The partials are folded in halves,
// 32, 16, ..., 1 (fbn_hc_fold).  A lane without a configuration contributes +0.0.  No partial is ever
// -0.0: an accumulator that starts at +0.0 can reach -0.0 only as (-0.0) + (-0.0) or (-0.0) - (+0.0).
#ifndef FBN_HC_BD_H
#define FBN_HC_BD_H

#include "hc_score.h"

// Contraction is switched off for this header's functions alone, so including it changes nothing for the
// includer: clang takes the pragma at the head of each function body (it has no push/pop for it on the
// device target), g++ takes it between push_options and pop_options.
#if defined(__clang__)
#define FBN_BD_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define FBN_BD_NO_CONTRACT
#if defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif
#endif

constexpr int kBdDirect = 16;          // counters below it take the product form (a < kBdShift)
constexpr double kBdShift = 16.0;      // the Stirling series is evaluated at x >= kBdShift only
constexpr double kBdSplit = 0x1p-32;   // below it ln(a) is taken on its own
constexpr double kBdIssMin = 1e-100, kBdIssMax = 1e100;  // every a stays a normal number, every S finite

enum { kBdKindBde = 0, kBdKindK2 = 1 };

struct FbnBdPrior {
    double a, head, s0;
};

// ln x for a normal positive x.  x = 2^k m with m in [sqrt(1/2), sqrt(2)), f = m - 1, s = f / (2 + f):
// ln m = 2 s + s^3 (2/3 + 2/5 s^2 + ...) = f - f^2 / 2 + s (f^2 / 2 + R(s^2)), R a degree-7 minimax
// polynomial in s^2 on |s| < 0.1716 (the classic reduction and coefficients of the BSD libm's log, error
// below 1 ulp); k ln 2 is added as a high part with 32 trailing zero bits (k ln2_hi is exact) and a low
// part.  ln 1 = +0.0 exactly.
FBN_HC_HD inline double fbn_bd_ln(double x) {
    FBN_BD_NO_CONTRACT
    constexpr double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
    constexpr double g1 = 6.666666666666735130e-01, g2 = 3.999999999940941908e-01, g3 = 2.857142874366239149e-01,
                     g4 = 2.222219843214978396e-01, g5 = 1.818357216161805012e-01, g6 = 1.531383769920937332e-01,
                     g7 = 1.479819860511658591e-01;
    uint64_t b;
    __builtin_memcpy(&b, &x, 8);
    int k = (int)(b >> 52) - 1023;
    uint64_t m = b & 0x000fffffffffffffull;
    const uint64_t up = (m + 0x00095f6400000000ull) & 0x0010000000000000ull;  // mantissa >= sqrt(2): halve it
    k += (int)(up >> 52);
    m |= up ^ 0x3ff0000000000000ull;
    double v;
    __builtin_memcpy(&v, &m, 8);
    const double f = v - 1.0;
    const double s = f / (2.0 + f);
    const double dk = (double)k;
    const double z = s * s;
    const double w = z * z;
    const double t1 = w * (g2 + w * (g4 + w * g6));
    const double t2 = z * (g1 + w * (g3 + w * (g5 + w * g7)));
    const double R = t2 + t1;
    const double hfsq = 0.5 * f * f;
    return dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f);
}

// S(x), x >= kBdShift: lnGamma(x) - ln(2 pi) / 2 up to the dropped tail of the series
FBN_HC_HD inline double fbn_bd_stirling(double x) {
    FBN_BD_NO_CONTRACT
    constexpr double c0 = 8.3333333333333329e-02, c1 = -2.7777777777777779e-03, c2 = 7.9365079365079365e-04,
                     c3 = -5.9523809523809529e-04, c4 = 8.4175084175084171e-04;  // 1/12, -1/360, 1/1260, -1/1680, 1/1188
    const double u = 1.0 / x;
    const double z = u * u;
    const double tail = u * (c0 + z * (c1 + z * (c2 + z * (c3 + z * c4))));
    return ((x - 0.5) * fbn_bd_ln(x) - x) + tail;
}

// D(n, a) by the product form: a < kBdShift, 1 <= n <= kBdDirect
FBN_HC_HD inline double fbn_bd_direct(uint32_t n, double a) {
    FBN_BD_NO_CONTRACT
    if (a >= kBdSplit) {
        double p = a;
        for (uint32_t i = 1; i < n; ++i) p = p * (a + (double)i);
        return fbn_bd_ln(p);
    }
    const double t = fbn_bd_ln(a);
    if (n == 1u) return t;
    double p = a + 1.0;
    for (uint32_t i = 2; i < n; ++i) p = p * (a + (double)i);
    return t + fbn_bd_ln(p);
}

FBN_HC_HD inline FbnBdPrior fbn_bd_prior(double a) {
    FBN_BD_NO_CONTRACT
    FbnBdPrior P;
    P.a = a;
    if (a < kBdShift) {
        P.head = fbn_bd_direct((uint32_t)kBdDirect, a);
        P.s0 = fbn_bd_stirling(a + (double)kBdDirect);
    } else {
        P.head = 0.0;
        P.s0 = fbn_bd_stirling(a);
    }
    return P;
}

// D(n, a), n >= 1
FBN_HC_HD inline double fbn_bd_term(uint32_t n, const FbnBdPrior &P) {
    FBN_BD_NO_CONTRACT
    if (P.a < kBdShift && n < (uint32_t)kBdDirect) return fbn_bd_direct(n, P.a);
    return P.head + (fbn_bd_stirling(P.a + (double)n) - P.s0);
}

// the two Dirichlet parameters of a family (host only: the divisions of the score's prior)
inline void fbn_bd_alphas(int kind, double iss, int r, int64_t q, double *a_cell, double *a_cfg) {
    FBN_BD_NO_CONTRACT
    if (kind == kBdKindK2) {
        *a_cell = 1.0;
        *a_cfg = (double)r;
    } else {
        *a_cell = iss / ((double)r * (double)q);
        *a_cfg = iss / (double)q;
    }
}

// the partial of `lane` over a family table of r x q counters
FBN_HC_HD inline double fbn_bd_lane_partial(const uint32_t *tab, int r, int q, int lane, const FbnBdPrior &cell,
                                            const FbnBdPrior &cfg) {
    FBN_BD_NO_CONTRACT
    double acc = 0.0;
    for (int j = lane; j < q; j += kHcLanes) {
        uint32_t nj = 0u;
        for (int k = 0; k < r; ++k) {
            const uint32_t n = tab[(int64_t)k * q + j];
            if (n == 0u) continue;
            nj += n;
            acc += fbn_bd_term(n, cell);
        }
        if (nj != 0u) acc -= fbn_bd_term(nj, cfg);
    }
    return acc;
}

// the host evaluation of one family table: the twin of one wave, or one packed sub-group, of hc_bd.hip.
// loglik is hc_score.h's, from the same table L[n] = n ln n, so its bits are the BIC path's.
inline void fbn_bd_family_host(const uint32_t *tab, int r, int q, const double *L, double a_cell, double a_cfg,
                               double *loglik, double *score) {
    FBN_BD_NO_CONTRACT
    const FbnBdPrior cell = fbn_bd_prior(a_cell), cfg = fbn_bd_prior(a_cfg);
    double p[kHcLanes], s[kHcLanes];
    for (int l = 0; l < kHcLanes; ++l) {
        p[l] = fbn_hc_lane_partial(tab, r, q, l, L);
        s[l] = fbn_bd_lane_partial(tab, r, q, l, cell, cfg);
    }
    *loglik = fbn_hc_fold(p);
    *score = fbn_hc_fold(s);
}

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif

#endif
