// gibbs.hip -- the Gibbs sampler's kernels on gfx950 (algorithm and the conditional both sides compile:
// gibbs_model.h; host twin: gibbs_host.cpp).  The reference has no counterpart.
//
// gibbs_kernel: 64-thread workgroups, one chain per lane.  A unit of work is (evidence case, chunk of 64
// of its chains); a persistent grid strides over the units, and a wave keeps its unit for the start and
// all burn_in + sweeps passes, so the chains' state never leaves the CU.  The stream is entered once per
// unit (PcgJumpTo to the chain's first position) and stepped once per (pass, variable) from there.
//
// LDS, dynamic, in this order:
//   values  [V][64] bytes            the chains' current assignment, as sample.hip keeps its samples
//   scratch [dmax][64] doubles       the unnormalised conditional of the variable in hand, lane-contiguous:
//                                    a wave's access to one k is two conflict-free 512-byte rows
//   pc      [V][64] int32 (PC)       every node's parent configuration by topological position, written by
//                                    the start pass and moved by (new - old) * stride when a parent changes
//   acc     [sum_dom] doubles (ACC)  the unit's accumulators; else they are the unit's row of A.ws
// Every column [..][lane] is read and written by its lane alone, and entry j of the accumulators by lane
// j % 64 alone, so the passes need no barrier; the only exchanges between lanes are the butterfly of the
// Rao-Blackwell terms (registers) and the transposed write of the last states.
//
// gibbs_finish_kernel adds a case's chunk rows in ascending order, divides by chains * sweeps, zeroes the
// observed variables' rows and writes the label: no atomics, one order.
// gibbs_cond_kernel (fbn_gibbs_debug_conditionals): one complete assignment per lane through the same
// GibbsConditional.
#include <hip/hip_runtime.h>

#include "gibbs_model.h"
#include "launchers.h"

using fbn::GibbsCondArgs;
using fbn::GibbsDeviceArgs;
using fbn::GibbsView;
using fbn::SampleNode;
using fbn::U128;

namespace {

__device__ __forceinline__ GibbsView view_of(const fbn::DeviceModel &M, const int32_t *coff, const int32_t *child) {
    return GibbsView{M.nodes, M.par, M.prob, M.cdf, coff, child, M.V, M.sum_dom};
}

template <bool ACC, bool PC>
__global__ __launch_bounds__(64) void gibbs_kernel(GibbsDeviceArgs A) {
    extern __shared__ __align__(16) uint8_t vals[];
    const int lane = threadIdx.x, V = A.M.V, SD = A.M.sum_dom;
    const GibbsView G = view_of(A.M, A.coff, A.child);
    double *g = reinterpret_cast<double *>(vals + (size_t)V * 64) + lane;
    int32_t *pcl = reinterpret_cast<int32_t *>(vals + (size_t)V * 64 + (size_t)A.dmax * 512);
    double *lacc = reinterpret_cast<double *>(reinterpret_cast<uint8_t *>(pcl) + (PC ? (size_t)V * 256 : 0));
    const int32_t *pc = PC ? pcl + lane : nullptr;
    const uint8_t *x = vals + lane;
    const long long C = A.S, passes = fbn::GibbsPasses(A.burn_in, A.sweeps);
    const uint64_t P = (uint64_t)V * (uint64_t)passes;
    for (long long u = blockIdx.x; u < A.units; u += gridDim.x) {
        const long long c = u / A.chunks, j0 = (u % A.chunks) * 64;
        const bool active = j0 + lane < C;  // a tail lane runs a chain of its own (in bounds) that adds +0.0
        const int8_t *ev = A.ev + c * V;
        double *acc = ACC ? lacc : A.ws + u * SD;
        for (int j = lane; j < SD; j += 64) acc[j] = 0.0;
        U128 s = fbn::PcgJumpTo(A.state, ((uint64_t)(A.case0 + c) * (uint64_t)C + (uint64_t)(j0 + lane)) * P, A.jump);
        for (int t = 0; t < V; ++t) {  // the start: likelihood weighting's draw without the weight
            const SampleNode nd = A.M.nodes[t];
            const int evv = ev[nd.v];
            const int pcv = fbn::GibbsParentConfig(G, nd, x);
            s = fbn::PcgStep(s, A.inc);
            const int q = evv >= 0 ? evv
                                   : fbn::SelectValue(A.M.cdf + nd.toff + (long long)pcv * nd.d, nd.d,
                                                      fbn::PcgDouble(fbn::PcgOutput(s)));
            vals[nd.v * 64 + lane] = (uint8_t)q;
            if (PC) pcl[t * 64 + lane] = pcv;
        }
        for (long long p = 1; p < passes; ++p) {
            const bool counted = p > A.burn_in;
            for (int t = 0; t < V; ++t) {
                const SampleNode nd = A.M.nodes[t];
                s = fbn::PcgStep(s, A.inc);
                if (ev[nd.v] >= 0) continue;  // wave-uniform: the position is consumed, nothing is drawn
                const int xo = vals[nd.v * 64 + lane];
                const double tot = fbn::GibbsConditional(G, t, x, pc, g);
                const int xn = tot == 0.0 ? xo : fbn::GibbsSelect(g, nd.d, fbn::PcgDouble(fbn::PcgOutput(s)), tot);
                if (counted)
                    for (int k = 0; k < nd.d; ++k) {
                        const double sum = fbn::wave_sum(active ? fbn::GibbsTerm(g, k, tot, xo) : 0.0);
                        const int j = nd.moff + k;
                        if ((j & 63) == lane) acc[j] = acc[j] + sum;
                    }
                if (xn != xo) {
                    vals[nd.v * 64 + lane] = (uint8_t)xn;
                    if (PC)
                        for (int e = A.coff[t]; e < A.coff[t + 1]; ++e)
                            pcl[A.child[2 * e] * 64 + lane] += (xn - xo) * A.child[2 * e + 1];
                }
            }
        }
        if (ACC)
            for (int j = lane; j < SD; j += 64) A.ws[u * SD + j] = acc[j];
        // the last states, transposed through LDS: consecutive lanes write consecutive bytes of [chain][V]
        __syncthreads();
        if (A.states) {
            const long long act = C - j0 < 64 ? C - j0 : 64;
            int8_t *out = A.states + (c * C + j0) * V;
            for (long long i = lane; i < act * V; i += 64) out[i] = (int8_t)vals[(i % V) * 64 + i / V];
        }
        __syncthreads();  // before the next unit's start rewrites the values
    }
}

__global__ __launch_bounds__(256) void gibbs_finish_kernel(GibbsDeviceArgs A) {
    const int SD = A.M.sum_dom;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.ncases * SD) return;
    const long long c = i / SD;
    const int j = (int)(i % SD);
    const int8_t *ev = A.ev + c * A.M.V;
    const double denom = (double)(A.S * A.sweeps);
    auto entry = [&](int q) {
        double sum = 0.0;
        for (long long k = 0; k < A.chunks; ++k) sum = sum + A.ws[(c * A.chunks + k) * SD + q];
        return ev[A.M.ent[q] >> 8] >= 0 ? 0.0 : sum / denom;
    };
    A.marg[c * SD + j] = entry(j);
    if (j == 0) {  // the query's row is entries 0 .. d0 - 1: QueryLabel's arg-max over the same values
        int lab = 0;
        double mp = 0.0;
        for (int q = 0; q < A.M.d0; ++q) {
            const double r = entry(q);
            if (r > mp) mp = r, lab = q;
        }
        A.labels[c] = lab;
    }
}

template <bool PC>
__global__ __launch_bounds__(64) void gibbs_cond_kernel(GibbsCondArgs A) {
    extern __shared__ __align__(16) uint8_t vals[];
    const int lane = threadIdx.x, V = A.M.V, SD = A.M.sum_dom;
    const GibbsView G = view_of(A.M, A.coff, A.child);
    double *g = reinterpret_cast<double *>(vals + (size_t)V * 64) + lane;
    int32_t *pcl = reinterpret_cast<int32_t *>(vals + (size_t)V * 64 + (size_t)A.dmax * 512);
    const uint8_t *x = vals + lane;
    const long long i = (long long)blockIdx.x * 64 + lane;
    const long long src = i < A.n ? i : A.n - 1;  // a tail lane repeats the last assignment and stores nothing
    for (int v = 0; v < V; ++v) vals[v * 64 + lane] = (uint8_t)A.states[src * V + v];
    if (PC)
        for (int t = 0; t < V; ++t) pcl[t * 64 + lane] = fbn::GibbsParentConfig(G, A.M.nodes[t], x);
    for (int t = 0; t < V; ++t) {
        const SampleNode nd = A.M.nodes[t];
        const double tot = fbn::GibbsConditional(G, t, x, PC ? pcl + lane : nullptr, g);
        if (i < A.n)
            for (int k = 0; k < nd.d; ++k) A.out[i * SD + nd.moff + k] = fbn::GibbsTerm(g, k, tot, x[nd.v * 64]);
    }
}

}  // namespace

extern "C" hipError_t fbn_gibbs_launch(const GibbsDeviceArgs *a, int lds_acc, size_t lds_bytes, int grid,
                                       hipStream_t stream) {
    const dim3 g((unsigned)grid), b(64);
    if (lds_acc && a->pc_cache) hipLaunchKernelGGL((gibbs_kernel<true, true>), g, b, lds_bytes, stream, *a);
    else if (lds_acc) hipLaunchKernelGGL((gibbs_kernel<true, false>), g, b, lds_bytes, stream, *a);
    else if (a->pc_cache) hipLaunchKernelGGL((gibbs_kernel<false, true>), g, b, lds_bytes, stream, *a);
    else hipLaunchKernelGGL((gibbs_kernel<false, false>), g, b, lds_bytes, stream, *a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const long long n = a->ncases * a->M.sum_dom;
    hipLaunchKernelGGL(gibbs_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, *a);
    return hipGetLastError();
}

extern "C" hipError_t fbn_gibbs_cond_launch(const GibbsCondArgs *a, size_t lds_bytes, hipStream_t stream) {
    const dim3 g((unsigned)((a->n + 63) / 64)), b(64);
    if (a->pc_cache) hipLaunchKernelGGL(gibbs_cond_kernel<true>, g, b, lds_bytes, stream, *a);
    else hipLaunchKernelGGL(gibbs_cond_kernel<false>, g, b, lds_bytes, stream, *a);
    return hipGetLastError();
}
