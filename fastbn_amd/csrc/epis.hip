// epis.hip -- EPIS-BN's sampling kernel on gfx950 (algorithm and the draw both sides compile:
// epis_model.h; host twin: epis_host.cpp).  Replaces the reference's EPIS-BN stub (src/main.cpp:123-134).
//
// sample_epis_kernel keeps sample_lw_kernel's shape (sample.hip): one evidence case per 64-thread
// workgroup, its S samples in chunks of 64, one sample per lane, the values drawn so far as bytes
// [V][64] in LDS, the same stream map (i * V + k), scaled weights (m, e), chunk reductions and
// marginal accumulation.  What differs is the draw of an unobserved variable: EpisDraw on the lane's
// table row (global memory, L1 / L2 resident) and the case's lambda row, the output of the LBP launch
// that ran before on the same stream.  The lambda row, sum_dom doubles, is wave-shared and read d times
// per pass by every lane: it sits in LDS behind the values (sample_epis_kernel<true>) when both fit
// the budget, else it is read from global memory (<false>).  EpisDraw recomputes g' in three passes
// over the d states, so no per-lane array exists and nothing goes to scratch.
#include <hip/hip_runtime.h>

#include "epis_model.h"
#include "launchers.h"

using fbn::EpisDeviceArgs;
using fbn::SampleNode;
using fbn::U128;

namespace {

template <bool LDS_LAMBDA>
__global__ __launch_bounds__(64) void sample_epis_kernel(EpisDeviceArgs A) {
    extern __shared__ __align__(16) uint8_t vals[];  // [V][64], then (LDS_LAMBDA) the lambda row [sum_dom]
    const int lane = threadIdx.x, V = A.M.V, SD = A.M.sum_dom;
    const long long c = blockIdx.x;
    const int8_t *ev = A.ev + c * V;
    double *row = A.marg + c * SD;
    const double *lam = A.lam + c * SD;
    if (LDS_LAMBDA) {
        double *l = reinterpret_cast<double *>(vals + V * 64);
        for (int j = lane; j < SD; j += 64) l[j] = lam[j];
        lam = l;
        __syncthreads();
    }
    const long long total = A.ncases * A.S;
    U128 s;
    fbn::WeightState ws;
    for (long long s0 = 0; s0 < A.S; s0 += 64) {
        const bool active = s0 + lane < A.S;  // a tail lane samples (in bounds) with weight 0
        const bool first = s0 == 0;           // this chunk opens the scope of emax and the sums
        if (first)
            s = fbn::PcgJumpTo(A.state, ((uint64_t)(A.case0 + c) * (uint64_t)A.S + (uint64_t)lane) * (uint64_t)V, A.jump);
        else
            s = fbn::Affine(s, A.jm, A.jc);
        double m = 1.0;
        int e = 0;
        for (int k = 0; k < V; ++k) {
            const SampleNode nd = A.M.nodes[k];
            const int evv = ev[nd.v];
            const double *P = A.M.prob + nd.toff + (long long)fbn::parent_config(A.M, nd, vals, lane) * nd.d;
            s = fbn::PcgStep(s, A.inc);
            int q, de;
            if (evv >= 0) {  // clamp, weigh: as likelihood weighting
                q = evv;
                m = frexp(m * P[q], &de);
            } else {
                double fac;
                q = fbn::EpisDraw(P, lam + nd.moff, nd.d, fbn::EpisCutoff(A.eps, nd.d), fbn::PcgDouble(fbn::PcgOutput(s)), &fac);
                m = frexp(m * fac, &de);
            }
            e += de;
            vals[nd.v * 64 + lane] = (uint8_t)q;
            if (A.dv && active) A.dv[(long long)nd.v * total + c * A.S + s0 + lane] = (uint8_t)q;
        }
        double f;
        const double w = fbn::chunk_weights(ws, m, e, active, first, A.dm, A.de, c * A.S + s0 + lane, &f);
        __syncthreads();
        fbn::accumulate_marginals(A.M, vals, row, w, f, first, lane);
        __syncthreads();
    }
    double *st = A.stats ? A.stats + 4 * c : nullptr;
    fbn::finish_case(A.M, ev, row, ws, A.S, A.labels + c, st, lane);
    if (lane == 0 && st) {
        st[2] = A.lbp_stats ? A.lbp_stats[2 * c] : 0.0;
        st[3] = A.lbp_stats ? A.lbp_stats[2 * c + 1] : 0.0;
    }
}

__global__ __launch_bounds__(256) void fill_kernel(double *p, long long n, double x) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = x;
}

}  // namespace

extern "C" hipError_t fbn_epis_launch(const EpisDeviceArgs *a, int lds_lambda, hipStream_t stream) {
    const size_t vbytes = (size_t)a->M.V * 64;
    if (lds_lambda)
        hipLaunchKernelGGL(sample_epis_kernel<true>, dim3((unsigned)a->ncases), dim3(64),
                           vbytes + (size_t)a->M.sum_dom * 8, stream, *a);
    else
        hipLaunchKernelGGL(sample_epis_kernel<false>, dim3((unsigned)a->ncases), dim3(64), vbytes, stream, *a);
    return hipGetLastError();
}

extern "C" hipError_t fbn_epis_fill(double *p, long long n, double x, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, p, n, x);
    return hipGetLastError();
}
