// fbn_device.h -- device plumbing shared by the files that own device memory (capi_*.hip):
// the HIP error macro, the growable buffers, the table upload, the gfx950 device check, the grid clamp
// against free memory, the evidence range check, and DeviceHandle, the base of every handle that
// queues work on caller streams (device, timing events, streams seen, create / destroy).
// Internal to libfastbn.
#ifndef FBN_DEVICE_H
#define FBN_DEVICE_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <set>
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

// Declared AFTER the host buffers that asynchronous copies on `s` read or write: an early error return
// then drains the stream before those buffers are destroyed.  The success path synchronises itself and
// calls done().
struct StreamDrain {
    hipStream_t s;
    bool armed = true;
    explicit StreamDrain(hipStream_t st) : s(st) {}
    void done() { armed = false; }
    ~StreamDrain() {
        if (armed) (void)hipStreamSynchronize(s);
    }
    StreamDrain(const StreamDrain &) = delete;
    StreamDrain &operator=(const StreamDrain &) = delete;
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

// the LDS of one CU: what bounds the workgroups resident on it by their LDS use
constexpr int64_t kCuLdsBytes = 160 * 1024;

// A persistent grid whose units (waves or workgroups) each own unit_bytes of workspace, kept within a
// share (num / den) of the free device memory beside the held_bytes the workspace has already; at
// least 1.  A unit of no bytes, or a device that does not report its memory, never clamps.
struct MemShare {
    size_t num, den;
};
constexpr MemShare kMemShare80{8, 10}, kMemShareHalf{1, 2};
inline int64_t ClampGridToFreeMemory(int64_t grid, size_t unit_bytes, size_t held_bytes, MemShare share) {
    size_t free_b = 0, total_b = 0;
    if (unit_bytes == 0 || hipMemGetInfo(&free_b, &total_b) != hipSuccess) return grid;
    const size_t have = free_b / share.den * share.num + held_bytes;
    return std::max<int64_t>(1, std::min<int64_t>(grid, (int64_t)(have / unit_bytes)));
}

// out-of-domain evidence has no reference meaning (a code >= the node's state count would shift
// bits into the neighbouring digit fields of the kernels' evidence masks): checked on the device
// before any kernel indexes with it; one stream sync (the host loop cost ~1 ns per value).
// Attached once to the handle's host state counts (which outlive it); dom is their device copy.
struct EvidenceCheck {
    DevBuf dom, word;  // the V state counts; 8 bytes: the first offending index
    const std::vector<int32_t> *host_dom = nullptr;
    int Attach(const std::vector<int32_t> &h) {
        host_dom = &h;
        if (int rc = Upload(dom, h)) return rc;
        return word.ensure(8);
    }
    // d_ev [ncases][V]
    int Run(const int8_t *d_ev, int64_t ncases, hipStream_t s) const {
        const int V = (int)host_dom->size();
        unsigned long long *d_word = word.as<unsigned long long>();
        FBN_HIP(hipMemsetAsync(d_word, 0xFF, 8, s));
        hipError_t e = fbn_jt_evidence_check(d_ev, (long long)ncases * V, V, dom.as<int32_t>(), d_word, s);
        if (e != hipSuccess) return SetError(FBN_ERR_HIP, "evidence check: %s", hipGetErrorString(e));
        unsigned long long first = 0;
        FBN_HIP(hipMemcpyAsync(&first, d_word, 8, hipMemcpyDeviceToHost, s));
        FBN_HIP(hipStreamSynchronize(s));
        if (first == ~0ull) return FBN_OK;
        int8_t code = 0;
        FBN_HIP(hipMemcpy(&code, d_ev + first, 1, hipMemcpyDeviceToHost));
        const long long c = (long long)(first / V);
        const int v = (int)(first % V);
        return SetError(FBN_ERR_ARG, "case %lld: evidence %d for node %d (domain %d)", c, (int)code, v, (*host_dom)[v]);
    }
};

// The base of a handle that owns device state: its device (-1: a host-only handle), the two events around
// its last kernel, the evidence check, and the caller streams its runs were queued on.  A run returns
// before its kernels end, so every entry that enqueues on a caller's stream notes it, and destroy drains
// the noted streams (not the whole device) before the buffers go.
struct DeviceHandle {
    int device = -1, num_cu = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false, timing = true;  // a timed launch is recorded; launches are timed at all
    std::set<hipStream_t> streams;
    EvidenceCheck evidence;
    ~DeviceHandle() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }

    int Attach(int dev) {
        device = dev;
        if (int rc = CheckDevice(dev, &num_cu)) return rc;
        FBN_HIP(hipEventCreate(&ev0));
        FBN_HIP(hipEventCreate(&ev1));
        return FBN_OK;
    }
    void Note(hipStream_t st) { streams.insert(st); }
    void Drain() {
        if (device < 0) return;
        (void)hipSetDevice(device);
        for (hipStream_t st : streams) (void)hipStreamSynchronize(st);
    }
    // the timed interval of a run: everything enqueued on st between Begin and End
    int Begin(hipStream_t st) {
        if (timing) FBN_HIP(hipEventRecord(ev0, st));
        return FBN_OK;
    }
    int End(hipStream_t st) {
        if (timing) FBN_HIP(hipEventRecord(ev1, st));
        timed = timing;
        return FBN_OK;
    }
    // launch() -> hipError_t between the two events
    template <class Launch>
    int Timed(hipStream_t st, Launch launch) {
        if (int rc = Begin(st)) return rc;
        FBN_HIP(launch());
        return End(st);
    }
    int LastKernelMs(float *ms) const {
        if (!ms || !timed) return SetError(FBN_ERR_ARG, "no timed launch");
        FBN_HIP(hipEventSynchronize(ev1));
        FBN_HIP(hipEventElapsedTime(ms, ev0, ev1));
        return FBN_OK;
    }
};

// the fbn_*_create / fbn_*_destroy entries of a handle H derived from DeviceHandle; init(H *) builds it
template <class H, class Init>
int CreateHandle(const fbn_network *net, H **out, Init init) {
    if (!net || !out) return SetError(FBN_ERR_ARG, "null pointer");
    *out = nullptr;
    H *s = new H;
    if (int rc = init(s)) {
        delete s;
        return rc;
    }
    *out = s;
    return FBN_OK;
}
template <class H>
int DestroyHandle(H *s) {
    if (!s) return FBN_OK;
    s->Drain();
    delete s;
    return FBN_OK;
}

}  // namespace fbn

#endif
