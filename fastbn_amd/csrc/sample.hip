// sample.hip -- the sampling engine on gfx950: forward (ancestral) sampling, likelihood weighting
// and probabilistic logic sampling, one sample per lane (algorithm, stream maps and the host twin:
// sample_host.cpp).  Replaces the reference's PLS / LW stubs (src/main.cpp:97-121) and, for workload
// generation, its wall-clock seeded SampleSetGenerator.
//
// Both kernels run one wave per workgroup.  The wave keeps the values its 64 samples have drawn so
// far as bytes [V][64] in LDS (64 V bytes: 2.4 KB for ALARM, 66.6 KB for the 1041-variable
// Munin-like network), walks the variables in topological order, forms each lane's parent
// configuration from its own LDS column and gathers its cdf row (or, for an observed variable under
// likelihood weighting, one probability) from the fp64 tables in global memory.  The per-variable
// records and parent lists are wave-uniform reads.  Random numbers: every lane jumps numpy's
// PCG64(seed) to its first stream position with the host's 2^j jump pairs (2 KB, passed in the kernel
// arguments; one 128-bit affine step per set bit, 64-bit halves, __umul64hi), then takes one affine
// step per variable.
//
// sample_lw_kernel: one evidence case per wave, its S samples in chunks of 64.  A sample's weight is
// a scaled pair (m, e), (m, de) = frexp(m * P(v = ev | parents)), e += de, so 520 observed variables
// do not underflow.  Per chunk: emax by a wave max; when it grows the running sums are rescaled by
// the exact power of two; w = ldexp(m, e - emax); sum w and sum w^2 by a shuffle butterfly; the
// marginal sums by entry -- lane j owns entries j, j + 64, ... of the case's output row, reads that
// variable's 64 value bytes from LDS (four 16-byte reads) and adds w of lane l (v_readlane) where
// the byte equals its value, l = 0 .. 63 in order.  The case's output row is the accumulator between
// chunks (always the same lane on the same address).  No floating-point atomics; every sum has one
// fixed order, so runs and batch splits are bit-identical.
#include <hip/hip_runtime.h>

#include "launchers.h"
#include "sample_device.h"

using fbn::parent_config;
using fbn::SampleNode;
using fbn::U128;

namespace {

__global__ __launch_bounds__(64) void sample_forward_kernel(fbn::ForwardDeviceArgs A) {
    extern __shared__ __align__(16) uint8_t vals[];  // [V][64]
    const int lane = threadIdx.x;
    const long long i = (long long)blockIdx.x * 64 + lane;
    const bool active = i < A.n;
    // a tail lane draws sample n - 1 again and stores nothing
    U128 s = fbn::PcgJumpTo(A.state, (uint64_t)(active ? i : A.n - 1), A.jump);
    for (int k = 0; k < A.M.V; ++k) {
        const SampleNode nd = A.M.nodes[k];
        const int pc = parent_config(A.M, nd, vals, lane);
        const double u = fbn::PcgDouble(fbn::PcgOutput(fbn::PcgStep(s, A.inc)));
        s = fbn::Affine(s, A.jm, A.jc);
        const int q = fbn::SelectValue(A.M.cdf + nd.toff + (long long)pc * nd.d, nd.d, u);
        vals[nd.v * 64 + lane] = (uint8_t)q;
        if (active) A.cols[(long long)nd.v * A.n + i] = (uint8_t)q;
    }
}

__global__ __launch_bounds__(64) void sample_lw_kernel(fbn::LwDeviceArgs A) {
    extern __shared__ __align__(16) uint8_t vals[];  // [V][64]
    const int lane = threadIdx.x, V = A.M.V, SD = A.M.sum_dom;
    const long long c = blockIdx.x;
    const int8_t *ev = A.ev + c * V;
    double *row = A.marg + c * SD;
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
            const int pc = parent_config(A.M, nd, vals, lane);
            s = fbn::PcgStep(s, A.inc);
            int q;
            if (evv >= 0 && A.method == 0) {  // likelihood weighting: clamp, weigh
                q = evv;
                int de;
                m = frexp(m * A.M.prob[nd.toff + (long long)pc * nd.d + q], &de);
                e += de;
            } else {
                q = fbn::SelectValue(A.M.cdf + nd.toff + (long long)pc * nd.d, nd.d, fbn::PcgDouble(fbn::PcgOutput(s)));
                if (evv >= 0 && q != evv) m = 0.0;  // logic sampling: reject
            }
            vals[nd.v * 64 + lane] = (uint8_t)q;
            if (A.dv && active) A.dv[(long long)nd.v * total + c * A.S + s0 + lane] = (uint8_t)q;
        }
        double f;
        const double w = fbn::chunk_weights(ws, m, e, active, first, A.dm, A.de, c * A.S + s0 + lane, &f);
        __syncthreads();
        fbn::accumulate_marginals(A.M, vals, row, w, f, first, lane);
        __syncthreads();
    }
    fbn::finish_case(A.M, ev, row, ws, A.S, A.labels + c, A.stats ? A.stats + 2 * c : nullptr, lane);
}

}  // namespace

extern "C" hipError_t fbn_sample_forward_launch(const fbn::ForwardDeviceArgs *a, hipStream_t stream) {
    hipLaunchKernelGGL(sample_forward_kernel, dim3((unsigned)((a->n + 63) / 64)), dim3(64), (size_t)a->M.V * 64, stream,
                       *a);
    return hipGetLastError();
}

extern "C" hipError_t fbn_lw_launch(const fbn::LwDeviceArgs *a, hipStream_t stream) {
    hipLaunchKernelGGL(sample_lw_kernel, dim3((unsigned)a->ncases), dim3(64), (size_t)a->M.V * 64, stream, *a);
    return hipGetLastError();
}
