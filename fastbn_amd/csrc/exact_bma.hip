// exact_bma.hip -- the lattice phases of exact arc posteriors on gfx950, in the (log-sum-exp, +) semiring:
// the zeta transforms of the n value lattices in both directions, the level-wise forward and backward
// recursions, and the gather of the arc matrix (include/fastbn.h states the quantities; exact_bma_host.cpp
// holds the same phases in plain loops, the twin these kernels are held to bit for bit; exact_lse.h is the
// arithmetic both evaluate).
//
// Transform.  One kernel serves the three transforms of the method: alpha (subset direction, lse), Gamma
// (superset direction, lse) and q (superset direction, plain sum).  It runs exact_dp.h's pass geometry: a
// workgroup loads a block of entries closed under a group of G bits into LDS, runs the G sweeps there in
// ascending bit order with a barrier after each, and stores the block back; blocks of one pass are disjoint
// and groups ascend, so the passes together are the plain M sweeps and every entry has one evaluation order
// for any tile size.  What differs from the subset-max transform of exact_dp.hip:
//   - an entry is a value alone, 8 bytes: the tile is 2^12 entries = 32 KiB, five workgroups on a CU;
//   - a lattice edge costs an exp and a ln (some 60 dependent fp64 operations and two divides) where the
//     maximum costs a compare, so the kernel is bound by the fp64 pipe, not by HBM.  A thread handles
//     2^B / 512 independent pairs per sweep (8 at the full tile), which the compiler interleaves; the 20 waves
//     a CU holds cover the rest of the latency;
//   - a pair whose partner is -inf is left alone before any arithmetic (under max_parents most of ls is
//     -inf and whole waves skip), and fbn_lse returns the larger operand past its cutoff;
//   - direction, operation and the load are template parameters, so a sweep's inner loop has no switch;
//   - the quantities gamma and p are never stored: the first pass of the Gamma transform forms gamma_v[U] =
//     F[U] + B[V \ U \ v] from the two subset tables as it loads, and the first pass of the q transform forms
//     p = exp((ls + Gamma) - logZ) as it loads.  alpha's first pass reads ls and writes the second lattice, so
//     ls survives for p; everything after lives in that second lattice.
// The semiring is (lse, +), which the matrix instructions (sum, x) do not compute.  No atomics.
//
// Levels.  One launch per subset size k writes F[W] and B[W] of every W of that size: both read level k - 1
// of their own table and the alpha lattices, so one thread forms both and shares the walk over W's members.
// Subsets map to threads by exact_dp.hip's popcount filter; the results leave through ordinary vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "exact_bma.h"
#include "exact_lse.h"
#include "launchers.h"

namespace {

constexpr int kBmaThreads = 256;

template <int DIR, int OP, int LOAD>
__global__ __launch_bounds__(kBmaThreads) void bma_pass_kernel(BmaPassArgs A) {
    extern __shared__ __align__(16) double bma_lds[];
    const int B = A.lo + A.hb;
    const uint32_t nent = 1u << B;
    const int rbits = A.M - B;  // workgroups per lattice = 2^rbits
    const uint32_t v = blockIdx.x >> rbits, r = blockIdx.x & ((1u << rbits) - 1u);
    const int rl = A.gpos - A.lo;
    const uint32_t base = ((r >> rl) << (A.gpos + A.hb)) | ((r & ((1u << rl) - 1u)) << A.lo);
    const uint32_t lomask = (1u << A.lo) - 1u;
    const size_t lat = (size_t)v << A.M;
    double *gx = A.x + lat;
    const double ninf = -__builtin_inf();

    const uint32_t full = (1u << A.nvars) - 1u;
    double logZ = 0.0;
    if (LOAD == kBmaLoadP) logZ = A.F[full];
    for (uint32_t e = threadIdx.x; e < nent; e += kBmaThreads) {
        const uint32_t g = base | ((e >> A.lo) << A.gpos) | (e & lomask);
        double x;
        if (LOAD == kBmaLoadX) {
            x = gx[g];
        } else if (LOAD == kBmaLoadLs) {
            x = A.ls[lat + g];
        } else if (LOAD == kBmaLoadGamma) {
            const uint32_t U = fbn_exact_expand(g, (int)v);
            x = A.F[U] + A.B[full ^ U ^ (1u << v)];
        } else {
            x = fbn_lse_expm((A.ls[lat + g] + gx[g]) - logZ);
        }
        bma_lds[e] = x;
    }
    __syncthreads();
    for (int b = A.s0; b < A.s0 + A.G; ++b) {
        const uint32_t bit = 1u << b;
        for (uint32_t p = threadIdx.x; p < (nent >> 1); p += kBmaThreads) {
            const uint32_t i0 = ((p >> b) << (b + 1)) | (p & (bit - 1u)), i1 = i0 | bit;
            const uint32_t own = DIR == kBmaSubset ? i1 : i0, partner = DIR == kBmaSubset ? i0 : i1;
            const double y = bma_lds[partner];
            if (OP == kBmaLse) {
                if (y != ninf) bma_lds[own] = fbn_lse(bma_lds[own], y);
            } else {
                bma_lds[own] = bma_lds[own] + y;
            }
        }
        __syncthreads();
    }
    for (uint32_t e = threadIdx.x; e < nent; e += kBmaThreads) {
        const uint32_t g = base | ((e >> A.lo) << A.gpos) | (e & lomask);
        gx[g] = bma_lds[e];
    }
}

__global__ __launch_bounds__(kBmaThreads) void bma_level_kernel(BmaLevelArgs A) {
    const uint32_t H = blockIdx.x;
    const int need = A.level - __popc(H);
    if (need < 0 || need > 8 || __popc(threadIdx.x) != need) return;
    const uint32_t W = (H << 8) | threadIdx.x;
    if (W >> A.nvars) return;  // fewer than 8 variables
    const int M = A.nvars - 1;
    const uint32_t rest = ((1u << A.nvars) - 1u) ^ W;  // V \ W
    double f = 0.0, bk = 0.0;
    bool first = true;
    for (uint32_t m = W; m; m &= m - 1u) {  // v ascending
        const int v = __ffs(m) - 1;
        const uint32_t Wm = W ^ (1u << v);
        const double *a = A.alpha + ((size_t)v << M);
        const double tf = A.F[Wm] + a[fbn_exact_squeeze(Wm, v)];
        const double tb = a[fbn_exact_squeeze(rest, v)] + A.B[Wm];
        f = first ? tf : fbn_lse(f, tf);
        bk = first ? tb : fbn_lse(bk, tb);
        first = false;
    }
    A.F[W] = f;
    A.B[W] = bk;
}

__global__ __launch_bounds__(kBmaThreads) void bma_gather_kernel(const double *q, const double *F, const double *B, int n,
                                                                 double *out) {
    const int t = blockIdx.x * kBmaThreads + threadIdx.x, M = n - 1;
    if (t < n * n) {
        const int u = t / n, v = t % n;
        out[t] = u == v ? 0.0 : q[((size_t)v << M) + fbn_exact_squeeze(1u << u, v)];
    } else if (t < n * n + n) {
        out[t] = q[(size_t)(t - n * n) << M];
    } else if (t == n * n + n) {
        out[t] = F[(1u << n) - 1u];
        out[t + 1] = B[(1u << n) - 1u];
    }
}

template <int DIR, int OP, int LOAD>
void LaunchPass(const BmaPassArgs &a, unsigned grid, size_t lds, hipStream_t stream) {
    hipLaunchKernelGGL((bma_pass_kernel<DIR, OP, LOAD>), dim3(grid), dim3(kBmaThreads), lds, stream, a);
}

}  // namespace

extern "C" hipError_t fbn_bma_pass_launch(const BmaPassArgs *a, hipStream_t stream) {
    const int B = a->lo + a->hb;
    if (a->nvars < 2 || a->nvars > kExactMaxVars || a->M != a->nvars - 1 || B < 1 || B > kBmaTileBitsMax || B > a->M ||
        a->lo < 0 || a->hb < 0 || a->G < 1 || a->s0 < 0 || a->s0 + a->G > B || a->gpos < a->lo || a->gpos + a->hb > a->M ||
        ((uint64_t)a->nvars << (a->M - B)) > kExactGridMax || !a->x)
        return hipErrorInvalidValue;
    const unsigned grid = (unsigned)a->nvars << (a->M - B);
    const size_t lds = (size_t)8 << B;
    const int key = a->dir * 100 + a->op * 10 + a->load;
    if (key == kBmaSubset * 100 + kBmaLse * 10 + kBmaLoadLs && a->ls)
        LaunchPass<kBmaSubset, kBmaLse, kBmaLoadLs>(*a, grid, lds, stream);
    else if (key == kBmaSubset * 100 + kBmaLse * 10 + kBmaLoadX)
        LaunchPass<kBmaSubset, kBmaLse, kBmaLoadX>(*a, grid, lds, stream);
    else if (key == kBmaSuperset * 100 + kBmaLse * 10 + kBmaLoadGamma && a->F && a->B)
        LaunchPass<kBmaSuperset, kBmaLse, kBmaLoadGamma>(*a, grid, lds, stream);
    else if (key == kBmaSuperset * 100 + kBmaLse * 10 + kBmaLoadX)
        LaunchPass<kBmaSuperset, kBmaLse, kBmaLoadX>(*a, grid, lds, stream);
    else if (key == kBmaSuperset * 100 + kBmaAdd * 10 + kBmaLoadP && a->ls && a->F)
        LaunchPass<kBmaSuperset, kBmaAdd, kBmaLoadP>(*a, grid, lds, stream);
    else if (key == kBmaSuperset * 100 + kBmaAdd * 10 + kBmaLoadX)
        LaunchPass<kBmaSuperset, kBmaAdd, kBmaLoadX>(*a, grid, lds, stream);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

extern "C" hipError_t fbn_bma_level_launch(const BmaLevelArgs *a, hipStream_t stream) {
    if (a->nvars < 2 || a->nvars > kExactMaxVars || a->level < 0 || a->level > a->nvars) return hipErrorInvalidValue;
    const unsigned grid = a->nvars > 8 ? 1u << (a->nvars - 8) : 1u;
    hipLaunchKernelGGL(bma_level_kernel, dim3(grid), dim3(kBmaThreads), 0, stream, *a);
    return hipGetLastError();
}

extern "C" hipError_t fbn_bma_gather_launch(const double *q, const double *F, const double *B, int nvars, double *out,
                                            hipStream_t stream) {
    if (nvars < 2 || nvars > kExactMaxVars) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)(nvars * nvars + nvars + 1 + kBmaThreads - 1) / kBmaThreads;
    hipLaunchKernelGGL(bma_gather_kernel, dim3(grid), dim3(kBmaThreads), 0, stream, q, F, B, nvars, out);
    return hipGetLastError();
}
