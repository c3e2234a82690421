// fbn_device.h -- device plumbing shared by the files that own device memory (capi_*.hip):
// the HIP error macro, the growable buffers, the table upload, the gfx950 device check, the evidence range check.
// Internal to libfastbn.
#ifndef FBN_DEVICE_H
#define FBN_DEVICE_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "fbn_internal.h"
#include "launchers.h"

#define FBN_HIP(call)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (call);                                                                         \
        if (e_ != hipSuccess) return fbn::SetError(FBN_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

// the index of pair (i < j) among the n (n - 1) / 2 pairs of n variables in lexicographic order, for
// the kernels and their callers (the host-only twin with its inverse: fbn::PairIndex, pc_internal.h)
__host__ __device__ inline long long fbn_pair_index(int i, int j, int n) {
    return (long long)i * n - (long long)i * (i + 1) / 2 + (j - i - 1);
}

namespace fbn {

// growable device buffer
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    int ensure(size_t b) {
        if (b <= bytes) return FBN_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        if (b == 0) return FBN_OK;
        hipError_t e = hipMalloc(&p, b);
        if (e != hipSuccess) return SetError(FBN_ERR_NOMEM, "hipMalloc(%zu): %s", b, hipGetErrorString(e));
        bytes = b;
        return FBN_OK;
    }
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    template <class T>
    T *as() const {
        return static_cast<T *>(p);
    }
};

// a host table into b (grown to fit; never empty, so its pointer is always valid)
template <class T>
int Upload(DevBuf &b, const std::vector<T> &v) {
    if (int rc = b.ensure(std::max<size_t>(v.size() * sizeof(T), 16))) return rc;
    if (!v.empty()) FBN_HIP(hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return FBN_OK;
}

inline int CheckDevice(int device, int *num_cu) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return SetError(FBN_ERR_NODEV, "no HIP device visible");
    if (device < 0 || device >= n) return SetError(FBN_ERR_NODEV, "device %d out of range (%d visible)", device, n);
    FBN_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    FBN_HIP(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
        return SetError(FBN_ERR_NODEV, "device %d is %s; libfastbn is built for gfx950 only", device, prop.gcnArchName);
    if (num_cu) *num_cu = prop.multiProcessorCount;
    return FBN_OK;
}

inline int PinnedEnsure(void *&ptr, size_t &have, size_t want) {
    if (want <= have) return FBN_OK;
    if (ptr) (void)hipHostFree(ptr);
    ptr = nullptr;
    have = 0;
    want = std::max<size_t>(want, 1 << 16) * 2;
    hipError_t e = hipHostMalloc(&ptr, want, hipHostMallocDefault);
    if (e != hipSuccess) return SetError(FBN_ERR_NOMEM, "hipHostMalloc(%zu): %s", want, hipGetErrorString(e));
    have = want;
    return FBN_OK;
}

// out-of-domain evidence has no reference meaning (a code >= the node's state count would shift
// bits into the neighbouring digit fields of the kernels' evidence masks): checked on the device
// before any kernel indexes with it; one stream sync (the host loop cost ~1 ns per value).
// d_ev [ncases][V]; d_dom / host_dom: the V state counts; d_word: 8 bytes of device scratch
inline int EvidenceCheckDevice(const int8_t *d_ev, int64_t ncases, int V, const int32_t *d_dom,
                               const int32_t *host_dom, unsigned long long *d_word, hipStream_t s) {
    FBN_HIP(hipMemsetAsync(d_word, 0xFF, 8, s));
    hipError_t e = fbn_jt_evidence_check(d_ev, (long long)ncases * V, V, d_dom, d_word, s);
    if (e != hipSuccess) return SetError(FBN_ERR_HIP, "evidence check: %s", hipGetErrorString(e));
    unsigned long long first = 0;
    FBN_HIP(hipMemcpyAsync(&first, d_word, 8, hipMemcpyDeviceToHost, s));
    FBN_HIP(hipStreamSynchronize(s));
    if (first == ~0ull) return FBN_OK;
    int8_t code = 0;
    FBN_HIP(hipMemcpy(&code, d_ev + first, 1, hipMemcpyDeviceToHost));
    const long long c = (long long)(first / V);
    const int v = (int)(first % V);
    return SetError(FBN_ERR_ARG, "case %lld: evidence %d for node %d (domain %d)", c, (int)code, v, host_dom[v]);
}

}  // namespace fbn

#endif
