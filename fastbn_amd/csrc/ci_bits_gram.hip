// ci_bits_gram.hip -- the row Gram matrix of the bit-sliced store (level 0 of a PC run), gfx950.
//
// A PC run's level 0 needs popcount(r_i & r_j) for every pair of leading mask rows (values 0..d-2
// of every variable; the last value is derived): a Gram matrix of mask rows over the sample bits.
// One wave per task = an 8 x 8 tile of (i, j) row pairs: per 4-word step 16 16-byte loads feed 256
// popcounts, counters in registers, then a butterfly reduction that leaves counter l's wave total
// in lane l (63 shuffles instead of 64 x 6).  Tasks are built on the host (capi_ci.hip CiGram*): one
// block of one wave per task so the task fields and row pointers are wave-uniform (scalar registers).
// ci_bits_gram_pairs then turns the Gram into the pairs' 64-slot count records (ci_bits_g2.hip's input).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ci_bits.h"
#include "ci_wave.h"
#include "launchers.h"

namespace {

// (field 0, the mask row of a retired masked variant, is always -1 and not read)
constexpr int kGramTaskInts = 8;  // mask row (-1: none), i0, ni, j0, nj, out offset (lo, hi), ld

__global__ __launch_bounds__(64) void ci_bits_gram(const uint32_t *__restrict__ bits, long long W,
                                                   const int32_t *__restrict__ rl, const int32_t *__restrict__ tasks,
                                                   long long ntasks, int32_t *__restrict__ out, int xcd) {
    typedef __attribute__((ext_vector_type(4))) unsigned u4;
    const int lane = threadIdx.x;
    // consecutive tiles (the same i-block of rows) on one XCD: the rows stay in that XCD's L2
    const XcdSplit sp = xcd_split(ntasks, 0, 1, xcd);
    for (long long k = sp.first; k < sp.end; k += sp.stride) {
        const int32_t *t = tasks + k * kGramTaskInts;
        const int i0 = t[1], ni = t[2], j0 = t[3], nj = t[4], ld = t[7];
        const long long off = (long long)(uint32_t)t[5] | ((long long)t[6] << 32);
        const uint32_t *pi[8], *pj[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) pi[r] = bits + (size_t)rl[i0 + (r < ni ? r : 0)] * W;
#pragma unroll
        for (int r = 0; r < 8; ++r) pj[r] = bits + (size_t)rl[j0 + (r < nj ? r : 0)] * W;
        uint32_t v[64];
#pragma unroll
        for (int c = 0; c < 64; ++c) v[c] = 0u;
        for (long long w4 = lane; 4 * w4 < W; w4 += 64) {
            u4 xi[8], yj[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) xi[r] = *reinterpret_cast<const u4 *>(pi[r] + 4 * w4);
#pragma unroll
            for (int r = 0; r < 8; ++r) yj[r] = *reinterpret_cast<const u4 *>(pj[r] + 4 * w4);
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int a = 0; a < 8; ++a)
#pragma unroll
                    for (int b = 0; b < 8; ++b) v[a * 8 + b] += __builtin_popcount(xi[a][q] & yj[b][q]);
        }
        // butterfly: at distance o each lane keeps the half of its counters selected by lane bit o
        // and adds its partner's copy of that half; lane l ends with counter l's total
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const bool hi = (lane & o) != 0;
#pragma unroll
            for (int c = 0; c < o; ++c) {
                const uint32_t send = hi ? v[c] : v[c + o], keep = hi ? v[c + o] : v[c];
                v[c] = keep + (uint32_t)__shfl_xor((int)send, o);
            }
        }
        const int a = lane >> 3, b = lane & 7;
        if (a < ni && b < nj) out[off + (long long)a * ld + b] = (int32_t)v[0];
    }
}

// level 0 from the Gram G of all leading rows (ld x ld, lead0[v] = v's first leading row): the
// (x < y) pair table of test t (pair t0 + t of the complete graph), last row / column derived from
// the per-row sample counts (complete_pair); the 64-slot record and, when recording, the pair table
template <int DX, int DY>
__device__ __forceinline__ void gram_pair(const int32_t *__restrict__ G, long long ld, int x, int y,
                                          const int32_t *__restrict__ lead0, const int32_t *__restrict__ cx,
                                          const int32_t *__restrict__ cy, int32_t *__restrict__ out,
                                          int32_t *__restrict__ ptab) {
    int32_t full[DX * DY];
    const int32_t *g = G + (long long)lead0[x] * ld + lead0[y];
    complete_pair<DX, DY>([&](int i, int j) { return g[i * ld + j]; }, cx, cy, full);
#pragma unroll
    for (int c = 0; c < DX * DY; ++c) out[c] = full[c];
    if (ptab)
#pragma unroll
        for (int c = 0; c < DX * DY; ++c) ptab[c] = full[c];
}

__global__ __launch_bounds__(256) void ci_bits_gram_pairs(const int32_t *__restrict__ G, long long ld,
                                                          const int32_t *__restrict__ lead0,
                                                          const int32_t *__restrict__ dims,
                                                          const int32_t *__restrict__ row0,
                                                          const int32_t *__restrict__ rowcnt, long long t0, long long n,
                                                          int nvars, int32_t *__restrict__ counts,
                                                          int32_t *__restrict__ pairtab) {
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n; t += (long long)gridDim.x * 256) {
        int x, y;
        pair_of(t0 + t, nvars, x, y);
        int32_t *out = counts + t * kBitsCells, *ptab = pairtab ? pairtab + 16 * (t0 + t) : nullptr;
        const int32_t *cx = rowcnt + row0[x], *cy = rowcnt + row0[y];
        switch (dims[x] * 8 + dims[y]) {
#define FBN_GP(A, B)                                                                                         \
    case A * 8 + B:                                                                                          \
        gram_pair<A, B>(G, ld, x, y, lead0, cx, cy, out, ptab);                                              \
        break;
            FBN_DIMS_4x4(FBN_GP)
#undef FBN_GP
        default: break;
        }
    }
}

}  // namespace

extern "C" int fbn_ci_gram_task_ints(void) { return kGramTaskInts; }

extern "C" hipError_t fbn_ci_gram(const uint32_t *bits, long long W, const int32_t *rl, const int32_t *tasks,
                                  long long ntasks, int32_t *out, int num_cu, hipStream_t s) {
    const long long cap = (long long)num_cu * 32;
    const dim3 g((unsigned)(ntasks < cap ? ntasks : cap));
    if (ntasks <= 0) return hipSuccess;
    hipLaunchKernelGGL(ci_bits_gram, g, dim3(64), 0, s, bits, W, rl, tasks, ntasks, out, /*xcd*/ 1);
    return hipGetLastError();
}

extern "C" hipError_t fbn_ci_gram_pairs(const int32_t *G, long long ld, const int32_t *lead0, const int32_t *dims,
                                        const int32_t *row0, const int32_t *rowcnt, long long t0, long long n,
                                        int nvars, int32_t *counts, int32_t *pairtab, int num_cu, hipStream_t s) {
    const long long g = (n + 255) / 256, cap = (long long)num_cu * 8;
    if (n > 0)
        hipLaunchKernelGGL(ci_bits_gram_pairs, dim3((unsigned)(g < cap ? g : cap)), dim3(256), 0, s, G, ld, lead0,
                           dims, row0, rowcnt, t0, n, nvars, counts, pairtab);
    return hipGetLastError();
}
