// sample_device.h -- device code the sampling kernels share (sample.hip, epis.hip): the model's
// device view, the parent configuration of a lane's sample, the wave reductions and the marginal
// accumulation of one 64-sample chunk.  Internal to libfastbn.
#ifndef FBN_SAMPLE_DEVICE_H
#define FBN_SAMPLE_DEVICE_H

#include <hip/hip_runtime.h>

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

// sample_epis_kernel's arguments (epis.hip; filled by capi_epis.hip)
struct EpisDeviceArgs {
    DeviceModel M;
    U128 state, inc, jm, jc;  // the jump of 63 V positions (the same lane's sample in the next chunk)
    uint64_t jump[256];       // this seed's 2^j jump pairs (PcgStream::jump), read from the kernel arguments
    const int8_t *ev;         // [ncases][V], checked
    long long ncases, S, case0;
    double eps;               // < 0: EpisCutoff's defaults
    const double *lam;        // [ncases][sum_dom]
    const double *lbp_stats;  // [ncases][2] or NULL (no pre-propagation: zeros)
    int32_t *labels;
    double *marg;   // [ncases][sum_dom]: accumulators, then the result
    double *stats;  // [ncases][4] or NULL
    uint8_t *dv;    // debug (all or none): values [V][ncases * S], mantissas, exponents [ncases * S]
    double *dm;
    int32_t *de;
};

}  // namespace fbn

#endif
