// exact_bma.h -- what the arc-posterior learner's device path (capi_bma.hip, exact_bma.hip) and its host twin
// (exact_bma_host.cpp) share beyond exact_dp.h (the lattice layout c_v(S), the pass geometry, the candidate
// enumerator) and exact_lse.h (the arithmetic): the tile of the 8-byte transform, the state's size, the
// checks, the structure prior and the result record.  include/fastbn.h states the definitions.
// Internal to libfastbn.
#ifndef FBN_EXACT_BMA_H
#define FBN_EXACT_BMA_H

#include <vector>

#include "exact_dp.h"

// the LDS tile of a transform pass: 2^12 entries of 8 bytes = 32 KiB, five workgroups (20 waves) on a CU's
// 160 KiB: the sweeps are exp / ln chains of dependent fp64 operations, so waves in flight hide their latency
constexpr int kBmaLdsBits = 12;
constexpr int kBmaTileBitsMax = 13;  // 64 KiB: two workgroups per CU, kept for the measurement
constexpr int kBmaDefaultTileBits = 8;  // the best of the sweep at 24 variables

inline int fbn_bma_default_tile_bits(int M) { return M <= kBmaLdsBits ? (M < 1 ? 1 : M) : kBmaDefaultTileBits; }

struct fbn_bma_result {
    fbn_bma_info info{};
    std::vector<double> arc_prob, q_empty;  // [n][n], [n]
};

namespace fbn {

// 16 n 2^(n-1) + 16 2^n, as a double so that any n has a printable value
inline double BmaStateBytes(int n) {
    double b = 1.0;
    for (int i = 0; i < n; ++i) b *= 2.0;
    return 8.0 * n * b + 16.0 * b;
}
// the prior's kind, the variable limit (FBN_ERR_LIMIT names the bytes of this learner's state), then ExactCheck
int BmaCheck(int nvars, const int32_t *dims, const fbn_exact_options &opt, int prior);
// the log structure prior by parent-set size, [n] doubles; empty for prior = 0 (nothing is added)
std::vector<double> BmaSizePrior(int n, int prior);
// n = 1: no lattice; logZ = B[V] = ls_0[{}], q_0[{}] = 1, the 1 x 1 zero matrix
int BmaOneVariable(const int32_t *dims, const fbn_exact_options &opt, const HcScorer &scorer, int prior, fbn_exact_info *xi,
                   fbn_bma_result *res);
// the scorer's counters of the shared enumerator's record into the result's
inline void BmaTakeScoring(const fbn_exact_info &xi, fbn_bma_info *info) {
    info->families_scored = xi.families_scored, info->batches = xi.batches;
    info->score_kernel_ms = xi.score_kernel_ms, info->score_wall_ms = xi.score_wall_ms;
}

}  // namespace fbn

#endif
