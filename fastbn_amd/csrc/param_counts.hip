// param_counts.hip -- family counts of every node of a DAG in one launch on gfx950.
//
// A work item is (family, sample slice): one 256-thread workgroup counts the samples [s0, s1) of one
// node's family table counts[q][pc] (q = the node's code, pc = the configuration of its parents in
// ascending index order, last fastest: fbn_network_create's layout), so 37 families x 5,000 samples
// and 1,000 families x 100,000 samples both give thousands of workgroups.  The column store is uint8
// [var][sample]; a thread takes 16 consecutive samples per step and builds their 16 keys column by
// column: per column five aligned dwords (one 16-byte load and the dword after it), funnel-shifted
// by the column's byte misalignment -- column v starts at byte v * N, which is not dword-aligned
// when N % 4 != 0, and a slice may start anywhere -- so there is no separate head loop; the last
// step of a slice masks the samples past s1 (their bytes are loaded, never used as a key).
//
// Two counting paths, chosen by the family's cell count alone (uniform per workgroup):
//   * LDS path (cells <= lds_cells_max <= 8192): sub-histograms in LDS, param_copies(cells) per wave
//     (lane l of wave w adds into copy w * k + l % k; copies at an odd stride), as ci_kernels.hip's
//     sub_lanes -- no cross-wave contention and k-fold fewer same-address conflicts inside a wave,
//     which matters most for the 2- to 16-cell tables of root nodes; one shared table above 2048
//     cells.  Merged once per workgroup: the copies summed per cell, non-zero sums added into the
//     family's global table with device-scope vector atomics.
//   * global path (larger tables): device-scope vector atomics straight into the zeroed global table.
// Accumulators are 32-bit: the caller checks N < 2^31.  Every key is in range because every code of
// column v is < dims[v]: the upload checks that (fbn_ci_cols_check) before any kernel bins with it,
// and this kernel relies on it -- it does not clamp keys.
//
// Reference: the sample loop of ParameterLearning::LearnParamsKnowStructCompData
// (src/ParameterLearning.cpp:40-58) and DiscreteNode::AddInstanceOfVarVal / AddCount
// (src/DiscreteNode.cpp:100-145), one map update per node per sample.  Counts are integers: the same
// in any order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "param_counts.h"

namespace {

// sub-histogram copies per wave for a table of `cells` cells (0: one table shared by the workgroup).
// 4 waves x copies x (cells | 1) ints: at most 4 x 2049 ints = 32.8 KB
__device__ __host__ inline int param_copies(int cells) {
    return cells <= 16 ? 16 : cells <= 256 ? 4 : cells <= 512 ? 2 : cells <= 2048 ? 1 : 0;
}

struct ParamArgs {
    const uint8_t *cols;  // [nvars][N], readable 32 bytes past the end
    long long N;
    const FbnParamFamily *fam;
    const int32_t *fcol, *fstr;
    uint32_t *tab;
    long long slice, nslices;
    int lds_cells_max;
};

__device__ __forceinline__ void add_agent(uint32_t *p, uint32_t v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void add_lds(uint32_t *p, uint32_t v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// the samples [s0, s1) of one family binned through add(key)
template <class Add>
__device__ __forceinline__ void count_slice(const ParamArgs &A, const FbnParamFamily &F, long long s0, long long s1,
                                            int tid, Add add) {
    const long long nunits = (s1 - s0 + kParamUnit - 1) / kParamUnit;
    const int32_t *fcol = A.fcol + F.coff, *fstr = A.fstr + F.coff;
    for (long long u = tid; u < nunits; u += kParamBlock) {
        const long long s = s0 + kParamUnit * u;
        const int valid = (int)(s1 - s < kParamUnit ? s1 - s : kParamUnit);
        int key[kParamUnit];
#pragma unroll
        for (int i = 0; i < kParamUnit; ++i) key[i] = 0;
        for (int j = 0; j < F.ncol; ++j) {
            const unsigned long long byte = (unsigned long long)fcol[j] * (unsigned long long)A.N + (unsigned long long)s;
            const int str = fstr[j];
            // the 16 bytes at `byte` from the five aligned dwords that hold them (the fifth dword is
            // within the 32 readable bytes past the store when the column is the last one)
            const uint32_t *w = reinterpret_cast<const uint32_t *>(A.cols + (byte & ~3ull));
            const int sh = 8 * (int)(byte & 3ull);
            uint32_t d[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) d[q] = w[q];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t x = (uint32_t)((((unsigned long long)d[q + 1] << 32) | d[q]) >> sh);
#pragma unroll
                for (int b = 0; b < 4; ++b) key[4 * q + b] += (int)((x >> (8 * b)) & 0xFFu) * str;
            }
        }
#pragma unroll
        for (int i = 0; i < kParamUnit; ++i)
            if (i < valid) add(key[i]);
    }
}

__global__ __launch_bounds__(kParamBlock) void param_counts_kernel(ParamArgs A) {
    extern __shared__ __align__(16) uint32_t sub[];
    const long long item = blockIdx.x;
    const long long f = item / A.nslices, sl = item % A.nslices;
    const FbnParamFamily F = A.fam[f];
    const long long s0 = sl * A.slice;
    const long long s1 = s0 + A.slice < A.N ? s0 + A.slice : A.N;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint32_t *gtab = A.tab + F.tab_off;
    if (F.cells <= A.lds_cells_max) {  // LDS path
        const int kl = param_copies(F.cells);
        const int nsub = kl ? (kParamBlock / 64) * kl : 1;
        const int sstr = F.cells | 1;
        for (int c = tid; c < nsub * sstr; c += kParamBlock) sub[c] = 0u;
        __syncthreads();
        uint32_t *mine = sub + (kl ? (wv * kl + (lane & (kl - 1))) * sstr : 0);
        count_slice(A, F, s0, s1, tid, [&](int key) { add_lds(mine + key, 1u); });
        __syncthreads();
        for (int c = tid; c < F.cells; c += kParamBlock) {
            uint32_t v = 0u;
            for (int w = 0; w < nsub; ++w) v += sub[w * sstr + c];
            if (v) add_agent(gtab + c, v);
        }
    } else {  // global path
        count_slice(A, F, s0, s1, tid, [&](int key) { add_agent(gtab + key, 1u); });
    }
}

}  // namespace

extern "C" size_t fbn_param_lds_ints(int cells) {
    const int kl = param_copies(cells);
    return (size_t)(kl ? (kParamBlock / 64) * kl : 1) * (size_t)(cells | 1);
}

extern "C" hipError_t fbn_param_launch(const uint8_t *cols, long long N, const FbnParamFamily *fam, long long nfam,
                                       const int32_t *fcol, const int32_t *fstr, uint32_t *tab, long long slice,
                                       long long nslices, int lds_cells_max, size_t lds_bytes, hipStream_t stream) {
    if (nfam <= 0 || nslices <= 0 || slice <= 0 || nfam * nslices > 0x7fffffffll) return hipErrorInvalidValue;
    if (lds_cells_max > kParamLdsCellsMax) lds_cells_max = kParamLdsCellsMax;
    ParamArgs a{cols, N, fam, fcol, fstr, tab, slice, nslices, lds_cells_max};
    hipLaunchKernelGGL(param_counts_kernel, dim3((unsigned)(nfam * nslices)), dim3(kParamBlock), lds_bytes, stream, a);
    return hipGetLastError();
}
