// sample_device.h -- device code the sampling kernels share (sample.hip, epis.hip, ais.hip; the latter
// two through epis_model.h and ais_model.h, which hold their kernels' arguments): the model's device
// view, the common kernel arguments, the parent configuration of a lane's sample, the wave reductions,
// the chunk tail, the marginal accumulation of one 64-sample chunk and the case tail.  Also included by
// the handles that fill the arguments (capi_sampler.h).  Internal to libfastbn.
#ifndef FBN_SAMPLE_DEVICE_H
#define FBN_SAMPLE_DEVICE_H

#include <hip/hip_runtime.h>

#include <climits>

#include "sample_model.h"

namespace fbn {

struct DeviceModel {
    const SampleNode *nodes;
    const int32_t *par;
    const double *prob, *cdf;
    const int32_t *ent;
    int V, sum_dom, d0;  // d0: states of variable 0, the query
};

__device__ __forceinline__ int parent_config(const DeviceModel &M, const SampleNode &nd, const uint8_t *vals, int lane) {
    int pc = 0;
    for (int j = 0; j < nd.npar; ++j) {
        const int p = M.par[2 * (nd.poff + j)], dp = M.par[2 * (nd.poff + j) + 1];
        pc = pc * dp + vals[p * 64 + lane];
    }
    return pc;
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x = x + __shfl_xor(x, off, 64);
    return x;
}
__device__ __forceinline__ int wave_max(int x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x = max(x, __shfl_xor(x, off, 64));
    return x;
}
__device__ __forceinline__ double read_lane(double x, int l) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// One chunk's marginal sums by entry: lane j owns entries j, j + 64, ... of the case's row, reads
// that variable's 64 value bytes from LDS (four 16-byte reads) and adds w of lane l where the byte
// equals its value, l = 0 .. 63 in order.  first: the row starts from 0.0; else from row[j] * f.
__device__ __forceinline__ void accumulate_marginals(const DeviceModel &M, const uint8_t *vals, double *row, double w,
                                                     double f, bool first, int lane) {
    for (int j = lane; j < M.sum_dom; j += 64) {
        const int en = M.ent[j], q = en & 255;
        double acc = first ? 0.0 : row[j] * f;
        const uint4 *xv = reinterpret_cast<const uint4 *>(vals + (en >> 8) * 64);
#pragma unroll 1  // 16 lanes at a time: unrolled over all 64 the selected terms alone take 128 VGPRs
        for (int t = 0; t < 4; ++t) {
            const uint4 b = xv[t];
            const unsigned wd[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int l = 0; l < 16; ++l)
                acc += (int)((wd[l >> 2] >> (8 * (l & 3))) & 0xFFu) == q ? read_lane(w, 16 * t + l) : 0.0;
        }
        row[j] = acc;
    }
}

// What the case-inference kernels' arguments have in common; LwDeviceArgs (below), EpisDeviceArgs
// (epis_model.h) and AisDeviceArgs (ais_model.h) extend it.  Filled by SamplerHandle (capi_sampler.h).
struct SampleCaseArgs {
    DeviceModel M;
    U128 state, inc, jm, jc;  // the jump of 63 V positions (the same lane's sample in the next chunk)
    uint64_t jump[256];       // this seed's 2^j jump pairs (PcgStream::jump), read from the kernel arguments
    const int8_t *ev;         // [ncases][V], checked
    long long ncases, S, case0;
    int32_t *labels;
    double *marg;   // [ncases][sum_dom]: accumulators, then the result
    double *stats;  // [ncases][2] (likelihood weighting) or [ncases][4], or NULL
    uint8_t *dv;    // debug (all or none): values [V][ncases * draws], mantissas, exponents [ncases * draws]
    double *dm;
    int32_t *de;
};

// sample_lw_kernel's arguments (sample.hip; filled by capi_sample.hip); stats [ncases][2], draws = S
struct LwDeviceArgs : SampleCaseArgs {
    int method;
};
// sample_forward_kernel's
struct ForwardDeviceArgs {
    DeviceModel M;
    U128 state, inc, jm, jc;  // seeded state; the jump of n positions (one variable on)
    uint64_t jump[256];       // this seed's 2^j jump pairs (PcgStream::jump), read from the kernel arguments
    long long n;
    uint8_t *cols;  // [V][n]
};

// The chunk tail: from a lane's sample weight (m, e) -- a tail lane is not active and weighs 0 -- the
// wave's maximum exponent, the rescale factor f of what was summed before (first: this chunk opens the
// scope), the lane's weight w on the new scale, and the two butterfly sums into ws.  di: the sample's
// place in the debug arrays dm, de (all or none).  No barrier inside; every lane of the wave calls it.
__device__ __forceinline__ double chunk_weights(WeightState &ws, double m, int e, bool active, bool first, double *dm,
                                                int32_t *de, long long di, double *f) {
    if (dm && active) {
        dm[di] = m;
        de[di] = e;
    }
    *f = WeightRescale(ws, wave_max(active ? e : INT_MIN), first);
    const double w = active ? ldexp(m, e - ws.emax) : 0.0;
    WeightAdd(ws, *f, wave_sum(w), wave_sum(w * w));
    return w;
}

// The case tail: normalise the row (observed variables and a weightless case: zeros), then on lane 0 the
// query label and the base statistics st[0 .. 2) = log_evidence, ess (st: the case's stats row or NULL).
// Every lane of the workgroup calls it: the barrier orders the row's stores, other lanes', before lane 0
// reads them.
__device__ __forceinline__ void finish_case(const DeviceModel &M, const int8_t *ev, double *row, const WeightState &ws,
                                            long long S, int32_t *label, double *st, int lane) {
    if (ws.sumw > 0.0) {
        for (int j = lane; j < M.sum_dom; j += 64) row[j] = ev[M.ent[j] >> 8] >= 0 ? 0.0 : row[j] / ws.sumw;
    } else {
        for (int j = lane; j < M.sum_dom; j += 64) row[j] = 0.0;
    }
    __syncthreads();
    if (lane == 0) {
        *label = QueryLabel(row, M.d0, ws.sumw);
        if (st) st[0] = WeightLogEvidence(ws, S), st[1] = WeightEss(ws);
    }
}

}  // namespace fbn

#endif
