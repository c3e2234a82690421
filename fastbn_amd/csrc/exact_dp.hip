// exact_dp.hip -- the lattice phases of exact score-optimal structure learning on gfx950: the subset-max
// transform of the n local-score lattices and the level-wise sink recursion (include/fastbn.h states the
// definitions and tie rules; exact_host.cpp holds the same phases in plain loops, the twin these kernels
// are held to bit for bit).
//
// Transform.  bps_v[S] = max over T within S of ls_v[T] is M = n - 1 sweeps over 2^M entries: in sweep b an
// index with bit b set takes its partner's (value, arg) if the partner's value is strictly greater.  One
// launch per bit would move every lattice M times through HBM, so a pass takes a group of G consecutive bits:
// a workgroup loads a block of entries that is closed under those bits into LDS (fp64 values, then uint32
// args: 12 bytes an entry, 2^12 entries = 48 KiB, three workgroups to a CU), runs the G sweeps there in
// ascending bit order with a barrier after each, and stores the block back.  Blocks of one pass are disjoint
// and every partner of an entry under the pass's bits lies in its block, so a pass is exactly G plain sweeps;
// groups ascend, so the passes together are the plain M sweeps, args included, for any tile size.
//   first pass: the block is a contiguous run of 2^(G + c) entries, i.e. 2^c tiles over the bits [0, G);
//   later pass: the block is 2^G rows, one per setting of the bits [gpos, gpos + G), each a contiguous run of
//   2^c entries over the bits [0, c): 2^c independent tiles side by side, so that every global access is a run of
//   2^c doubles (c = 4: one 128-byte line) rather than single doubles 2^gpos apart.
// One grid covers all n lattices.  The compare is fp64, the rest integer moves: the operation is a maximum
// (max, +), which the matrix instructions (sum, x) do not compute.  No atomics: blocks are disjoint.
//
// Sink recursion.  R[W] = max over v in W of R[W \ v] + bps_v[c_v(W \ v)], lowest v among equals.  One launch
// per level k over the subsets of popcount k; level k reads level k - 1 only.  Subsets map to threads by a
// popcount filter over the index range: workgroup H holds the 256 subsets W = H << 8 | t and leaves at once
// unless k - popcount(H) is in 0 .. 8; a thread whose popcount(t) is the difference evaluates W.  Each
// candidate is one fp64 add of two gathered doubles; the results leave through ordinary vector stores
// (fp64 and one byte).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "exact_dp.h"
#include "launchers.h"

namespace {

constexpr int kExactThreads = 256;

__global__ __launch_bounds__(kExactThreads) void exact_pass_kernel(ExactPassArgs A) {
    extern __shared__ __align__(16) double exact_lds[];
    const int B = A.lo + A.hb;
    const uint32_t nent = 1u << B;
    double *lval = exact_lds;
    uint32_t *larg = reinterpret_cast<uint32_t *>(exact_lds + nent);
    const int rbits = A.M - B;  // workgroups per lattice = 2^rbits
    const uint32_t v = blockIdx.x >> rbits, r = blockIdx.x & ((1u << rbits) - 1u);
    const int rl = A.gpos - A.lo;
    const uint32_t base = ((r >> rl) << (A.gpos + A.hb)) | ((r & ((1u << rl) - 1u)) << A.lo);
    const uint32_t lomask = (1u << A.lo) - 1u;
    double *gval = A.val + ((size_t)v << A.M);
    uint32_t *garg = A.arg + ((size_t)v << A.M);

    for (uint32_t e = threadIdx.x; e < nent; e += kExactThreads) {
        const uint32_t g = base | ((e >> A.lo) << A.gpos) | (e & lomask);
        lval[e] = gval[g];
        larg[e] = A.init_arg ? g : garg[g];
    }
    __syncthreads();
    for (int b = A.s0; b < A.s0 + A.G; ++b) {
        const uint32_t bit = 1u << b;
        for (uint32_t p = threadIdx.x; p < (nent >> 1); p += kExactThreads) {
            const uint32_t i0 = ((p >> b) << (b + 1)) | (p & (bit - 1u)), i1 = i0 | bit;
            const double x = lval[i0];
            if (x > lval[i1]) {
                lval[i1] = x;
                larg[i1] = larg[i0];
            }
        }
        __syncthreads();
    }
    for (uint32_t e = threadIdx.x; e < nent; e += kExactThreads) {
        const uint32_t g = base | ((e >> A.lo) << A.gpos) | (e & lomask);
        gval[g] = lval[e];
        garg[g] = larg[e];
    }
}

__global__ __launch_bounds__(kExactThreads) void exact_sink_kernel(ExactSinkArgs A) {
    const uint32_t H = blockIdx.x;
    const int need = A.level - __popc(H);
    if (need < 0 || need > 8 || __popc(threadIdx.x) != need) return;
    const uint32_t W = (H << 8) | threadIdx.x;
    if (W >> A.nvars) return;  // fewer than 8 variables
    const int M = A.nvars - 1;
    double best = 0.0;
    int bv = -1;
    for (uint32_t m = W; m; m &= m - 1u) {  // v ascending
        const int v = __ffs(m) - 1;
        const uint32_t Wm = W ^ (1u << v);
        const double cand = A.R[Wm] + A.bps[((size_t)v << M) + fbn_exact_squeeze(Wm, v)];
        if (bv < 0 || cand > best) best = cand, bv = v;
    }
    A.R[W] = best;
    A.sink[W] = (uint8_t)bv;
}

}  // namespace

extern "C" hipError_t fbn_exact_pass_launch(const ExactPassArgs *a, hipStream_t stream) {
    const int B = a->lo + a->hb;
    if (a->nvars < 2 || a->nvars > kExactMaxVars || a->M != a->nvars - 1 || B < 1 || B > kExactTileBitsMax || B > a->M ||
        a->G < 1 || a->s0 + a->G > B || a->gpos < a->lo || a->gpos + a->hb > a->M ||
        ((uint64_t)a->nvars << (a->M - B)) > kExactGridMax)
        return hipErrorInvalidValue;
    const unsigned grid = (unsigned)a->nvars << (a->M - B);
    hipLaunchKernelGGL(exact_pass_kernel, dim3(grid), dim3(kExactThreads), (size_t)12 << B, stream, *a);
    return hipGetLastError();
}

extern "C" hipError_t fbn_exact_sink_launch(const ExactSinkArgs *a, hipStream_t stream) {
    if (a->nvars < 2 || a->nvars > kExactMaxVars || a->level < 0 || a->level > a->nvars) return hipErrorInvalidValue;
    const unsigned grid = a->nvars > 8 ? 1u << (a->nvars - 8) : 1u;
    hipLaunchKernelGGL(exact_sink_kernel, dim3(grid), dim3(kExactThreads), 0, stream, *a);
    return hipGetLastError();
}
