// exact_lse.h -- the (log-sum-exp, +) arithmetic of the arc-posterior learner, written once: the lattice kernels
// (exact_bma.hip) and the host twin (exact_bma_host.cpp) agree bit for bit because they evaluate these
// functions, not copies of them.  In hc_bd.h's style: no exp, log or log1p of any library is called (those
// differ between host and device), only + - * / and bit manipulation, which IEEE-754 rounds correctly, hence
// identically, on both sides; contraction is switched off in every function, so no FMA is formed.
//
//   fbn_lse_exp(x), x <= 0:   e^x.  k = x / ln 2 rounded to the nearest integer, r = (x - k ln2_hi) - k ln2_lo
//                             with hc_bd.h's split of ln 2 (k ln2_hi is exact: 32 trailing zero bits, |k| <
//                             2^10), |r| <= 0.3466; e^r = 1 + (r + r c / (2 - c)), c = r - r^2 P(r^2), P the
//                             degree-4 minimax polynomial of the BSD libm's exp (error below 1 ulp); the
//                             scaling by 2^k is one multiply by a power of two built from the exponent bits.
//                             Below kLseExpMin = -708 (-inf included) the result is exactly +0.0: every
//                             value returned is a normal number or zero.  e^0 = 1 exactly.
//   fbn_lse_expm(x), x <= 1:  the same evaluation for the posterior p = e^(ls + Gamma - logZ), whose argument
//                             is at most 0 in exact arithmetic and may exceed it by rounding.
//   fbn_lse(a, b):            ln(e^a + e^b) = hi + ln(1 + e^(lo - hi)), hi = a if a >= b else b, lo the other.
//                             hi is returned unchanged when lo is -inf (so lse(-inf, -inf) = -inf and a
//                             sweep pays nothing for an absent operand) or when lo - hi < kLseCut = -37:
//                             e^-37 < 2^-53, half an ulp of 1, so 1 + e^(lo - hi) would round to 1.  The
//                             logarithm is hc_bd.h's fbn_bd_ln of a number in [1, 2].
// The cutoffs and the operand order (hi first) are part of the definition.  No argument is ever NaN or +inf:
// the local scores are finite or -inf and the empty parent set is always finite.
#ifndef FBN_EXACT_LSE_H
#define FBN_EXACT_LSE_H

#include "hc_bd.h"

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

constexpr double kLseExpMin = -708.0;  // below it e^x is +0.0 (e^-708 = 3.3e-308 is still a normal number)
constexpr double kLseCut = -37.0;      // below it e^(lo - hi) is under half an ulp of 1

// e^x for kLseExpMin <= x <= 1
FBN_HC_HD inline double fbn_lse_exp_core(double x) {
    FBN_BD_NO_CONTRACT
    constexpr double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10,
                     inv_ln2 = 1.44269504088896338700e+00;
    constexpr double p1 = 1.66666666666666019037e-01, p2 = -2.77777777770155933842e-03, p3 = 6.61375632143793436117e-05,
                     p4 = -1.65339022054652515390e-06, p5 = 4.13813679705723846039e-08;
    const int k = (int)(x * inv_ln2 + (x < 0.0 ? -0.5 : 0.5));  // truncation: to nearest
    const double dk = (double)k;
    const double hi = x - dk * ln2_hi, lo = dk * ln2_lo;
    const double r = hi - lo;
    const double t = r * r;
    const double c = r - t * (p1 + t * (p2 + t * (p3 + t * (p4 + t * p5))));
    const double y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi);
    const uint64_t sb = (uint64_t)(k + 1023) << 52;  // 2^k, k in -1022 .. 1
    double scale;
    __builtin_memcpy(&scale, &sb, 8);
    return y * scale;
}

FBN_HC_HD inline double fbn_lse_exp(double x) {
    FBN_BD_NO_CONTRACT
    return x < kLseExpMin ? 0.0 : fbn_lse_exp_core(x);
}

FBN_HC_HD inline double fbn_lse_expm(double x) {
    FBN_BD_NO_CONTRACT
    return x < kLseExpMin ? 0.0 : fbn_lse_exp_core(x);
}

FBN_HC_HD inline double fbn_lse(double a, double b) {
    FBN_BD_NO_CONTRACT
    const double hi = a >= b ? a : b, lo = a >= b ? b : a;
    if (lo == -__builtin_inf()) return hi;
    const double d = lo - hi;
    if (d < kLseCut) return hi;
    return hi + fbn_bd_ln(1.0 + fbn_lse_exp(d));
}

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif

#endif
