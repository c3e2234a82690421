// ais.hip -- the adaptive samplers' kernel on gfx950: AIS-BN and SIS (algorithm, the draw and the row
// update both sides compile: ais_model.h; host twin: ais_host.cpp).  Replaces the reference's AIS-BN and
// SIS stubs (src/main.cpp:175-186, :149-160).
//
// sample_ais_kernel keeps the sampling kernels' shape (sample.hip, epis.hip): 64-thread workgroups, one
// evidence case at a time per wave, its samples in chunks of 64, one sample per lane, the values drawn
// so far as bytes [V][64] in LDS, the stream map, scaled weights (m, e), chunk reductions and marginal
// accumulation.  What it adds is state that lives across chunks, per case: the importance CPT I and
// the weighted family counts N, `cells` doubles each, in LDS behind the values (<true>) when they fit the
// budget, else in the workgroup's slice of a global workspace (<false>).  That slice is sized by the
// grid, so the grid is persistent and strides over the cases (as lbp.hip); everything a case owns is
// reset when the workgroup takes its next case.
//
// Between chunks of a learning stage the counts take the chunk's weights: lane j owns the learnable
// nodes j, j + 64, ... and walks the 64 samples in order, so every cell is summed in ascending sample
// order by one lane -- no atomics, no cross-lane sum, one order the host twin repeats.  After a stage
// lanes take rows (x, pc) and apply AisUpdateRow.  The stream is entered once per case (PcgJumpTo);
// every later chunk is a fixed number of positions on from the lane's last draw, within a stage (jm, jc)
// or from a learning stage's last chunk to the next stage's first (sm, sc).
#include <hip/hip_runtime.h>

#include "ais_model.h"
#include "launchers.h"

using fbn::AisDeviceArgs;
using fbn::SampleNode;
using fbn::U128;

namespace {

// byte i of eight consecutive samples' values
__device__ __forceinline__ int byte_of(uint2 b, int i) { return (int)(((i < 4 ? b.x : b.y) >> (8 * (i & 3))) & 0xFFu); }

template <bool LDS_STATE>
__global__ __launch_bounds__(64) void sample_ais_kernel(AisDeviceArgs A) {
    // [V][64] values, 64 weights, (LDS_STATE) I [cells], N [cells], then V learnable flags
    extern __shared__ __align__(16) uint8_t vals[];
    const int lane = threadIdx.x, V = A.M.V, SD = A.M.sum_dom;
    const long long cells = A.cells, nupd = A.sch.nupd, T = A.sch.T;
    double *wl = reinterpret_cast<double *>(vals + V * 64);
    double *I = LDS_STATE ? wl + 64 : A.ws + (long long)blockIdx.x * 2 * cells;
    double *N = I + cells;
    uint8_t *lrn = reinterpret_cast<uint8_t *>(LDS_STATE ? N + cells : wl + 64);
    const long long total = A.ncases * T;
    for (long long c = blockIdx.x; c < A.ncases; c += gridDim.x) {
        const int8_t *ev = A.ev + c * V;
        double *row = A.marg + c * SD;
        // per-case state: the ICPT starts as the CPTs; the learnable set is the unobserved variables
        // with an observed descendant, one reverse-topological pass (lane 0; wave-uniform afterwards)
        for (long long j = lane; j < cells; j += 64) I[j] = A.M.prob[j];
        for (int j = lane; j < V; j += 64) lrn[j] = 0;
        __syncthreads();
        if (lane == 0)
            for (int k = V - 1; k >= 0; --k) {
                const SampleNode nd = A.M.nodes[k];
                if (ev[nd.v] >= 0 || lrn[nd.v])
                    for (int j = 0; j < nd.npar; ++j) lrn[A.M.par[2 * (nd.poff + j)]] = 1;
            }
        __syncthreads();
        for (int j = lane; j < V; j += 64) lrn[j] = lrn[j] && ev[j] < 0;
        __syncthreads();
        U128 s;
        fbn::WeightState ws;
        int upd = 0;
        double ess0 = 0.0;
        bool first = true;  // the next chunk opens the scope of emax, the sums and the counts
        long long tbase = 0;
        for (long long st = 0; st <= nupd; ++st) {
            const long long n = st < nupd ? A.sch.l : A.sch.last;
            const bool counted = A.method == 1 || st == nupd, learn = st < nupd;
            if (A.method == 0 || st == 0) {
                first = true, ws.sumw = 0.0, ws.sumw2 = 0.0;
                if (learn) {
                    for (long long j = lane; j < cells; j += 64) N[j] = 0.0;
                    __syncthreads();
                }
            }
            for (long long s0 = 0; s0 < n; s0 += 64) {
                const bool active = s0 + lane < n;  // a tail lane samples (in bounds) with weight 0
                const int act = (int)(n - s0 < 64 ? n - s0 : 64);
                const long long t = tbase + s0 + lane;
                if (t == lane)  // the case's first chunk
                    s = fbn::PcgJumpTo(A.state, ((uint64_t)(A.case0 + c) * (uint64_t)T + (uint64_t)t) * (uint64_t)V,
                                       A.jump);
                else if (s0 == 0)
                    s = fbn::Affine(s, A.sm, A.sc);
                else
                    s = fbn::Affine(s, A.jm, A.jc);
                double m = 1.0;
                int e = 0;
                for (int k = 0; k < V; ++k) {
                    const SampleNode nd = A.M.nodes[k];
                    const int evv = ev[nd.v];
                    const long long r = nd.toff + (long long)fbn::parent_config(A.M, nd, vals, lane) * nd.d;
                    s = fbn::PcgStep(s, A.inc);
                    int q, de;
                    if (evv >= 0) {  // clamp, weigh: as likelihood weighting
                        q = evv;
                        m = frexp(m * A.M.prob[r + q], &de);
                        e += de;
                    } else if (lrn[nd.v]) {
                        double fac;
                        q = fbn::AisDraw(A.M.prob + r, I + r, nd.d, fbn::EpisCutoff(A.eps, nd.d),
                                         fbn::PcgDouble(fbn::PcgOutput(s)), &fac);
                        m = frexp(m * fac, &de);
                        e += de;
                    } else {
                        q = fbn::SelectValue(A.M.cdf + r, nd.d, fbn::PcgDouble(fbn::PcgOutput(s)));
                    }
                    vals[nd.v * 64 + lane] = (uint8_t)q;
                    if (A.dv && active) A.dv[(long long)nd.v * total + c * T + t] = (uint8_t)q;
                }
                double f;
                const double w = fbn::chunk_weights(ws, m, e, active, first, A.dm, A.de, c * T + t, &f);
                wl[lane] = w;
                if (learn && f != 1.0)
                    for (long long j = lane; j < cells; j += 64) N[j] = N[j] * f;
                __syncthreads();
                if (counted) fbn::accumulate_marginals(A.M, vals, row, w, f, first, lane);
                if (learn)
                    for (int k = lane; k < V; k += 64) {  // the counts: a node per lane, samples in order
                        const SampleNode nd = A.M.nodes[k];
                        if (!lrn[nd.v]) continue;
                        for (int l0 = 0; l0 < act; l0 += 8) {  // eight samples' bytes per LDS read, parents read once
                            int pc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                            for (int j = 0; j < nd.npar; ++j) {
                                const int p = A.M.par[2 * (nd.poff + j)], dp = A.M.par[2 * (nd.poff + j) + 1];
                                const uint2 b = *reinterpret_cast<const uint2 *>(vals + p * 64 + l0);
#pragma unroll
                                for (int i = 0; i < 8; ++i) pc[i] = pc[i] * dp + byte_of(b, i);
                            }
                            const uint2 b = *reinterpret_cast<const uint2 *>(vals + nd.v * 64 + l0);
#pragma unroll
                            for (int i = 0; i < 8; ++i)
                                if (l0 + i < act) {
                                    const long long cell = nd.toff + (long long)pc[i] * nd.d + byte_of(b, i);
                                    N[cell] = N[cell] + wl[l0 + i];
                                }
                        }
                    }
                __syncthreads();
                first = false;
            }
            if (st == 0) ess0 = fbn::WeightEss(ws) / (double)n;
            if (learn) {  // update st: a row (x, pc) per lane
                if (ws.sumw > 0.0) ++upd;
                const double eta = A.eta[st];
                for (int k = 0; k < V; ++k) {
                    const SampleNode nd = A.M.nodes[k];
                    if (!lrn[nd.v]) continue;
                    const long long end = k + 1 < V ? A.M.nodes[k + 1].toff : cells;
                    for (long long r = nd.toff + (long long)lane * nd.d; r < end; r += 64ll * nd.d)
                        fbn::AisUpdateRow(I + r, N + r, nd.d, eta);
                }
                __syncthreads();
            }
            tbase += n;
        }
        if (A.di)
            for (long long j = lane; j < cells; j += 64) A.di[c * cells + j] = I[j];
        double *o = A.stats ? A.stats + 4 * c : nullptr;
        // its barrier also stands between the reads of I above and the next case's rewrite of I and the flags
        fbn::finish_case(A.M, ev, row, ws, A.S, A.labels + c, o, lane);
        if (lane == 0 && o) {
            o[2] = (double)upd;
            o[3] = ess0;
        }
    }
}

}  // namespace

extern "C" hipError_t fbn_ais_launch(const AisDeviceArgs *a, int lds_state, size_t lds_bytes, int grid,
                                     hipStream_t stream) {
    if (lds_state)
        hipLaunchKernelGGL(sample_ais_kernel<true>, dim3((unsigned)grid), dim3(64), lds_bytes, stream, *a);
    else
        hipLaunchKernelGGL(sample_ais_kernel<false>, dim3((unsigned)grid), dim3(64), lds_bytes, stream, *a);
    return hipGetLastError();
}
