// lbp.hip -- loopy belief propagation on gfx950 (algorithm and orders: lbp_model.h; host twin:
// lbp_host.cpp).  Replaces the reference's LBP stub (src/main.cpp:136-147).
//
// One evidence case per wave (64-thread workgroups), a persistent grid that strides over the cases.
// The case's two message arrays and one array of unnormalised values, 3 M doubles, live in LDS
// (lbp_kernel<true, .>) or, for a network whose 24 M bytes exceed the LDS budget, in the workgroup's
// slice of a global workspace sized by the grid (lbp_kernel<false, .>).  Lanes take message entries
// (edge, q) in strides of 64, in the model's cost order (a pass of 64 entries lasts as long as its
// heaviest, so entries of similar cost go together).  A half-step is two passes with a barrier between them: every lane
// stores the unnormalised value of its entries, then every lane adds the d values of its entry's
// edge itself, in ascending q, divides, damps and takes |new - old| -- no sum is split over lanes,
// so the bits do not depend on the mapping.  The factor pass walks the table cells of the entry in
// ascending cell index and gathers them from global memory (the tables are L1 / L2 resident); the
// digits of a cell come from exact reciprocal divisions (LbpDiv).  The residual is a maximum: a
// shuffle butterfly.  No floating-point atomics.
#include <hip/hip_runtime.h>

#include "launchers.h"
#include "lbp_model.h"

using fbn::LbpDeviceArgs;
using fbn::LbpEdge;

namespace {

__device__ __forceinline__ double wave_fmax(double x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x = fmax(x, __shfl_xor(x, off, 64));
    return x;
}

// LAMBDA: the run also writes EPIS-BN's importance function (LbpDeviceArgs::lambda); without it the
// kernel is fbn_lbp_run's, instruction for instruction what it was before that output existed
template <bool LDS, bool LAMBDA>
__global__ __launch_bounds__(64) void lbp_kernel(LbpDeviceArgs A) {
    extern __shared__ __align__(16) double lbp_lds[];
    const int lane = threadIdx.x, V = A.V, SD = A.SD, M = A.M;
    double *m = LDS ? lbp_lds : A.ws + (size_t)blockIdx.x * 3 * (size_t)M;
    double *mu = m + M, *raw = mu + M;
    for (long long c = blockIdx.x; c < A.ncases; c += gridDim.x) {
        const int8_t *ev = A.ev + c * V;
        for (int j = lane; j < M; j += 64) {
            const LbpEdge ed = A.edges[A.bin_edge[j]];
            const int q = j - ed.moff, o = ev[ed.x];
            m[j] = 1.0 / (double)ed.d;
            mu[j] = o >= 0 ? (q == o ? 1.0 : 0.0) : 1.0 / (double)ed.d;
        }
        __syncthreads();
        bool bad = false;
        int used = 0;
        double res = 0.0;
        for (int it = 1; it <= A.iters; ++it) {
            double r = 0.0;
            bool b = false;
            for (int half = 0; half < 2; ++half) {
                double *dst = half ? mu : m;
                for (int i = lane; i < M; i += 64) {
                    const int j = A.order[i];  // entries of similar cost share a pass
                    const LbpEdge ed = A.edges[A.bin_edge[j]];
                    if (ev[ed.x] >= 0) continue;
                    const int q = j - ed.moff;
                    if (half) {
                        const int v0 = A.var_off[ed.x];
                        raw[j] = fbn::LbpVarRaw(A.var_moff + v0, A.var_off[ed.x + 1] - v0, ed.moff, m, q);
                    } else {
                        raw[j] = fbn::LbpFactorRaw(ed, A.terms, A.prob, mu, q);
                    }
                }
                __syncthreads();
                for (int j = lane; j < M; j += 64) {
                    const LbpEdge ed = A.edges[A.bin_edge[j]];
                    if (ev[ed.x] >= 0) continue;
                    const double z = fbn::LbpRowSum(raw + ed.moff, ed.d);
                    if (fbn::LbpBadZ(z)) {
                        b = true;
                        continue;
                    }
                    double nw = raw[j] / z;
                    const double old = dst[j];
                    if (!half && A.damping != 0.0) nw = (1.0 - A.damping) * nw + A.damping * old;
                    r = fmax(r, fabs(nw - old));
                    dst[j] = nw;
                }
                __syncthreads();
            }
            res = wave_fmax(r);
            bad = __any(b) != 0;
            used = it;
            if (bad || res <= A.tol) break;
        }
        // beliefs: the unnormalised rows first, then every lane divides by its own row's sum
        for (int j = lane; j < SD; j += 64) {
            const int x = A.marg_var[j];
            const int v0 = A.var_off[x];
            raw[j] = ev[x] >= 0 ? 0.0 : fbn::LbpVarRaw(A.var_moff + v0, A.var_off[x + 1] - v0, -1, m, j - A.marg_off[x]);
        }
        __syncthreads();
        bool b = false;
        for (int j = lane; j < SD; j += 64) {
            const int x = A.marg_var[j];
            if (ev[x] < 0 && fbn::LbpBadZ(fbn::LbpRowSum(raw + A.marg_off[x], A.dom[x]))) b = true;
        }
        bad = bad || __any(b) != 0;
        if (A.marg) {
            double *row = A.marg + c * SD;
            for (int j = lane; j < SD; j += 64) {
                const int x = A.marg_var[j];
                row[j] = bad || ev[x] >= 0 ? 0.0 : raw[j] / fbn::LbpRowSum(raw + A.marg_off[x], A.dom[x]);
            }
        }
        if (lane == 0) {
            int lab = -1;
            if (!bad) {
                lab = 0;
                double mp = 0.0;  // ArgMax, strict '>' from 0 (src/Inference.cpp:92-102), as fbn_jt_run
                if (ev[0] < 0) {
                    const double z = fbn::LbpRowSum(raw, A.d0);
                    for (int q = 0; q < A.d0; ++q) {
                        const double p = raw[q] / z;
                        if (p > mp) mp = p, lab = q;
                    }
                }
            }
            A.labels[c] = lab;
            if (A.stats) {
                A.stats[2 * c] = (double)used;
                A.stats[2 * c + 1] = bad ? INFINITY : res;
            }
        }
        if (A.messages)
            for (int j = lane; j < 2 * M; j += 64) A.messages[(size_t)c * 2 * (size_t)M + j] = m[j];
        if (LAMBDA)  // every variable's message into its own family
            for (int j = lane; j < SD; j += 64) {
                const int x = A.marg_var[j];
                A.lambda[(size_t)c * SD + j] = bad ? 1.0 : mu[A.self_moff[x] + j - A.marg_off[x]];
            }
        __syncthreads();  // the next case's initialisation overwrites what other lanes still read
    }
}

}  // namespace

extern "C" hipError_t fbn_lbp_launch(const LbpDeviceArgs *a, int lds, size_t lds_bytes, int grid, hipStream_t stream) {
    if (lds && a->lambda)
        hipLaunchKernelGGL((lbp_kernel<true, true>), dim3((unsigned)grid), dim3(64), lds_bytes, stream, *a);
    else if (lds)
        hipLaunchKernelGGL((lbp_kernel<true, false>), dim3((unsigned)grid), dim3(64), lds_bytes, stream, *a);
    else if (a->lambda)
        hipLaunchKernelGGL((lbp_kernel<false, true>), dim3((unsigned)grid), dim3(64), 0, stream, *a);
    else
        hipLaunchKernelGGL((lbp_kernel<false, false>), dim3((unsigned)grid), dim3(64), 0, stream, *a);
    return hipGetLastError();
}
