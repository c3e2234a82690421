// hc_score.h -- the decomposable family score of the hill-climbing learner, written once: the device
// reduction (hc_score.hip) and the host twin (hc_search.cpp) agree bit for bit because they evaluate
// these functions, not copies of them.
//
// A family is a child with r states and a parent set with q joint configurations; its counts N_jk lie
// in fbn_param_counts' layout, tab[k * q + j] (value k, configuration j of the ascending parents, last
// fastest).  With L[n] = n ln n (L[0] = 0), N_j = sum_k N_jk:
//     loglik = sum_jk L[N_jk] - sum_j L[N_j]            score = loglik - pen
// where pen = penalty * (r - 1) * q is formed on the host (fbn_hc_penalty_term) and L is a table of
// N + 1 doubles filled on the host with the C library's log (fbn_hc_fill_table).  Whoever evaluates a
// family only gathers from L and adds or subtracts doubles: no log, no multiply, nothing a compiler
// could contract into an FMA, so one summation order gives one value on either side.
//
// The order: 64 lane partials, lane l over the configurations j = l, l + 64, ... ascending; per
// configuration the values k ascending (+ L[N_jk] each, N_j summed as an integer), then - L[N_j].
// The partials are folded in halves: p[l] += p[l + 32], then + 16, 8, 4, 2, 1 (l below the offset);
// p[0] is the log-likelihood.  A lane without a configuration contributes +0.0.
#ifndef FBN_HC_SCORE_H
#define FBN_HC_SCORE_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FBN_HC_HD __host__ __device__
#else
#define FBN_HC_HD
#endif

constexpr int kHcLanes = 64;
// largest sample count a score table is built for: 8 * (2^24 + 1) bytes = 128 MiB
constexpr int64_t kHcMaxSamples = (int64_t)1 << 24;

// L[0 .. N]
inline void fbn_hc_fill_table(double *L, int64_t N) {
    L[0] = 0.0;
    for (int64_t n = 1; n <= N; ++n) L[n] = (double)n * log((double)n);
}

// the penalty term of a family (host only: the one multiply of the score)
inline double fbn_hc_penalty_term(double penalty, int r, int64_t q) { return penalty * (double)((int64_t)(r - 1) * q); }

// the partial of `lane` over a family table of r x q counters
FBN_HC_HD inline double fbn_hc_lane_partial(const uint32_t *tab, int r, int q, int lane, const double *L) {
    double acc = 0.0;
    for (int j = lane; j < q; j += kHcLanes) {
        uint32_t nj = 0u;
        for (int k = 0; k < r; ++k) {
            const uint32_t n = tab[(int64_t)k * q + j];
            nj += n;
            acc += L[n];
        }
        acc -= L[nj];
    }
    return acc;
}

// the fold of the 64 partials on the host (p is overwritten); returns the log-likelihood
inline double fbn_hc_fold(double *p) {
    for (int off = kHcLanes / 2; off >= 1; off >>= 1)
        for (int l = 0; l < off; ++l) p[l] += p[l + off];
    return p[0];
}

#if defined(__HIPCC__)
// the same fold across the lanes of a wave: lane 0 returns the log-likelihood (the other lanes'
// values are not the fold of anything)
__device__ __forceinline__ double fbn_hc_fold_wave(double v) {
#pragma unroll
    for (int off = kHcLanes / 2; off >= 1; off >>= 1) v += __shfl_down(v, off, kHcLanes);
    return v;
}
#endif

// the host evaluation of one family table: the twin of one wave of hc_score.hip
inline void fbn_hc_family_host(const uint32_t *tab, int r, int q, const double *L, double pen, double *loglik,
                               double *score) {
    double p[kHcLanes];
    for (int l = 0; l < kHcLanes; ++l) p[l] = fbn_hc_lane_partial(tab, r, q, l, L);
    const double ll = fbn_hc_fold(p);
    *loglik = ll;
    *score = ll - pen;
}

#endif
