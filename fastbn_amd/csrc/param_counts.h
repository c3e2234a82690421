// param_counts.h -- launch interface of the family-count kernel (param_counts.hip), shared with capi_ci.hip.
#ifndef FBN_PARAM_COUNTS_H
#define FBN_PARAM_COUNTS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

// one family = one node and its parents: columns fcol[coff .. coff + ncol) (the node first, then its
// parents ascending) with key strides fstr[...] (the node: parent configurations; parent j: product
// of the later parents' state counts), its table of `cells` 32-bit counters at tab + tab_off
struct FbnParamFamily {
    long long tab_off;
    int32_t coff, ncol, cells, pad;
};

constexpr int kParamBlock = 256;        // threads per workgroup
constexpr int kParamUnit = 16;          // samples per thread and step (one 16-byte load per column)
constexpr int kParamLdsCellsMax = 8192; // largest table counted in LDS (32 KB)

// the default slice length for nfam families of N samples on num_cu CUs: enough (family, slice) items
// for every CU to hold several workgroups, each slice at least 1024 samples (4 steps of the
// workgroup's 256 threads), a multiple of the 16 samples a thread takes per step
inline long long fbn_param_default_slice(long long N, int num_cu, long long nfam) {
    const long long want = (16ll * num_cu + nfam - 1) / nfam;  // slices per family to aim for
    long long ns = N / 1024 < want ? N / 1024 : want;
    if (ns < 1) ns = 1;
    return ((N + ns - 1) / ns + kParamUnit - 1) / kParamUnit * kParamUnit;
}

// LDS ints a family of `cells` (<= kParamLdsCellsMax) cells needs
extern "C" size_t fbn_param_lds_ints(int cells);
// families [0, nfam) x slices [0, nslices) of `slice` samples, one workgroup each; tab zeroed by the
// caller; cols readable for 32 bytes past its last column (the aligned loads of a misaligned column)
extern "C" hipError_t fbn_param_launch(const uint8_t *cols, long long N, const FbnParamFamily *fam, long long nfam,
                                       const int32_t *fcol, const int32_t *fstr, uint32_t *tab, long long slice,
                                       long long nslices, int lds_cells_max, size_t lds_bytes, hipStream_t stream);

#endif
