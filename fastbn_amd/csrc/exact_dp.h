// exact_dp.h -- what the exact learner's device path (capi_exact.hip, exact_dp.hip) and its host twin
// (exact_host.cpp) share: the index arithmetic of the subset lattices, the pass geometry of the tiled
// subset-max transform, and the host phases that both run (candidate enumeration and scoring through an
// HcScorer, the trace from the sink table).  Internal to libfastbn.
//
// Lattice of variable v: 2^M entries, M = n - 1, entry c_v(S) for S within V \ {v} (bit v squeezed out).
#ifndef FBN_EXACT_DP_H
#define FBN_EXACT_DP_H

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FBN_EXACT_HD __host__ __device__
#else
#define FBN_EXACT_HD
#endif

constexpr int kExactMaxVars = 26;
// the LDS tile of a transform pass: 2^12 entries of 12 bytes = 48 KiB, three workgroups on a CU's 160 KiB
constexpr int kExactLdsBits = 12;
constexpr int kExactTileBitsMax = 13;  // 96 KiB: one workgroup per CU, kept for the measurement
constexpr int kExactDefaultTileBits = 8;
// most workgroups of one transform launch (256 threads each, 2^32 threads a launch): only a tile_bits of
// a few bits on many variables makes blocks small enough to pass it
constexpr uint64_t kExactGridMax = (1ull << 24) - 1;

// c_v(S): S (bit v clear) with bit v squeezed out; and back
FBN_EXACT_HD inline uint32_t fbn_exact_squeeze(uint32_t S, int v) { return ((S >> (v + 1)) << v) | (S & ((1u << v) - 1u)); }
FBN_EXACT_HD inline uint32_t fbn_exact_expand(uint32_t c, int v) { return ((c >> v) << (v + 1)) | (c & ((1u << v) - 1u)); }

// One pass of the tiled transform.  A workgroup holds 2^(lo + hb) entries: local index e = (j << lo) | l
// is the lattice index  l | r_low << lo | j << gpos | r_high << (gpos + hb),  r = the workgroup's number
// within the lattice (r_low = its gpos - lo low bits).  The pass sweeps the local bits [s0, s0 + G).
//   first pass:  lo = G + c, hb = 0, gpos = lo, s0 = 0: a contiguous run holding 2^c tiles of the bits [0, G)
//   later pass:  lo = c, hb = G, gpos = the group's first bit, s0 = c: tiles over the bits [gpos, gpos + G),
//                2^c of them side by side so that a tile row is a contiguous run of 2^c entries
struct ExactPass {
    int gpos, hb, lo, s0, G;
};

// the passes of tile_bits (1 .. kExactTileBitsMax) bits each over M >= 1 bits, the last one ragged.  A
// block fills the LDS tile (2^kExactLdsBits entries, or 2^tile_bits where that is more): the c run bits
// are what the pass's G bits leave of it, at most the bits below the group.  Returns their number.
// lds_bits: the tile of the kernel that runs the passes (exact_bma.hip's entries are 8 bytes, not 12).
inline int fbn_exact_passes(int M, int tile_bits, ExactPass *out, int lds_bits = kExactLdsBits) {
    const int T = tile_bits, lds = T > lds_bits ? T : lds_bits;
    int np = 0;
    for (int g0 = 0; g0 < M; g0 += T, ++np) {
        const int G = M - g0 < T ? M - g0 : T, room = g0 == 0 ? M - G : g0;
        const int c = lds - G < room ? lds - G : room;
        if (g0 == 0) out[np] = ExactPass{G + c, 0, G + c, 0, G};
        else out[np] = ExactPass{g0, G, c, c, G};
    }
    return np;
}

// the default: a lattice that fits one LDS tile is transformed in a single pass
inline int fbn_exact_default_tile_bits(int M) { return M <= kExactLdsBits ? (M < 1 ? 1 : M) : kExactDefaultTileBits; }

#include <functional>

#include "hc_search.h"

namespace fbn {

// 12 n 2^(n-1) + 9 2^n, as a double so that any n has a printable value
inline double ExactStateBytes(int n) {
    double b = 1.0;
    for (int i = 0; i < n; ++i) b *= 2.0;
    return 6.0 * n * b + 9.0 * b;
}
// options, dims and the variable limit; FBN_ERR_LIMIT names the bytes the lattices would take
int ExactCheck(int nvars, const int32_t *dims, const fbn_exact_options &opt);
// phase 1 for variable v: ls[0 .. 2^(n-1)) = -inf, then the candidates' scores, enumerated by size and
// lexicographically within a size, scored through `scorer` in batches.  size_prior (the arc-posterior
// learner's log structure prior, exact_bma.h): a candidate of k parents gets score + size_prior[k]; nullptr
// (the exact search): the score as it is
int ExactLocalScores(int n, const int32_t *dims, const fbn_exact_options &opt, const HcScorer &scorer, int v, double *ls,
                     fbn_exact_info *info, const double *size_prior = nullptr);
// The enumeration phase 1 runs, shared with the sparse family lists of the order sampler (order_mcmc.h): the
// candidates of v by size and lexicographically within a size, as 64-bit masks over the n <= 64 variables, scored
// in batches; sink(mask, score + size_prior[|mask|]) per candidate in that order.  scorer == nullptr: nothing is
// scored and the sink is not called.  count (optional) is advanced by the number of candidates.
int ExactEnumerate(int n, const int32_t *dims, const fbn_exact_options &opt, const HcScorer *scorer, int v, fbn_exact_info *info,
                   const double *size_prior, const std::function<void(uint64_t, double)> &sink, int64_t *count);
// phase 4: the DAG from sink [2^n] and arg_at(v, index) = arg_v[index], the chosen families scored once
// more for the node values; RV = R[V]
int ExactTrace(int n, const int32_t *dims, const fbn_exact_options &opt, const HcScorer &scorer, const uint8_t *sink,
               const std::function<int(int, uint32_t, uint32_t *)> &arg_at, double RV, fbn_exact_info *info,
               fbn_hc_result *res);

}  // namespace fbn

#endif
