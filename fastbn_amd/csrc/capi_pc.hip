// capi_pc.hip -- the PC-stable entries of include/fastbn.h and the host <-> device seam of the
// PC-stable driver (pc_internal.h): batches, the device-resident levels 0 and 1, the small-graph search.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "capi_state.h"
#include "launchers.h"
#include "pc_internal.h"
#include "pc_small.h"

using fbn::SetError;

extern "C" {

// ------------------------------------------------------------------ PC-stable
int fbn_pc_stable(fbn_ci_ctx *c, double alpha, int depth, int group_size, fbn_pc_result **out) {
    if (!c || !out || depth < 1 || !(alpha >= 0.0 && alpha <= 1.0)) return SetError(FBN_ERR_ARG, "bad argument");
    auto r = std::unique_ptr<fbn_pc_result>(new (std::nothrow) fbn_pc_result());
    if (!r) return SetError(FBN_ERR_NOMEM, "out of memory");
    FBN_HIP(hipSetDevice(c->device));
    const bool timing = fbn::PcTiming();  // diagnostic
    using fbn::Clock;
    using fbn::Ms;
    auto t0 = Clock::now();
    int rc;
    // the device-resident search (small graphs) sets the ctx's margin log itself (and resets it when
    // it falls back to the host levels)
    if (!fbn::CiPCSmallEligible(c, group_size) && (rc = fbn::CiResetMargin(c))) return rc;
    auto t1 = Clock::now();
    if ((rc = fbn::RunPCStable(c, alpha, depth, group_size, r->r))) return rc;
    auto t2 = Clock::now();
    // the run's work is all on the ctx stream
    if (!r->r.margin_done && (rc = fbn::CiReadMargin(c, &r->r.min_margin, &r->r.near_alpha, true))) return rc;
    auto t3 = Clock::now();
    if ((rc = fbn::OrientPC(c->nvars, r->r))) return rc;  // StructLearnByPCStable steps 2-3
    if (timing)
        fprintf(stderr, "pc_stable: margin reset %.2f ms, skeleton %.2f ms, margin read %.2f ms, orientation %.2f ms\n",
                Ms(t0, t1), Ms(t1, t2), Ms(t2, t3), Ms(t3, Clock::now()));
    *out = r.release();
    return FBN_OK;
}
int fbn_pc_num_levels(const fbn_pc_result *r, int *n) {
    if (!r || !n) return SetError(FBN_ERR_ARG, "null pointer");
    *n = (int)r->r.tests_per_level.size();
    return FBN_OK;
}
int fbn_pc_level_tests(const fbn_pc_result *r, int64_t *tests) {
    if (!r || !tests) return SetError(FBN_ERR_ARG, "null pointer");
    std::copy(r->r.tests_per_level.begin(), r->r.tests_per_level.end(), tests);
    return FBN_OK;
}
int fbn_pc_level_launched(const fbn_pc_result *r, int64_t *tests) {
    if (!r || !tests) return SetError(FBN_ERR_ARG, "null pointer");
    std::copy(r->r.launched_per_level.begin(), r->r.launched_per_level.end(), tests);
    return FBN_OK;
}
int fbn_pc_num_edges(const fbn_pc_result *r, int *n) {
    if (!r || !n) return SetError(FBN_ERR_ARG, "null pointer");
    *n = (int)r->r.edges.size();
    return FBN_OK;
}
int fbn_pc_edges(const fbn_pc_result *r, int32_t *pairs) {
    if (!r || !pairs) return SetError(FBN_ERR_ARG, "null pointer");
    for (size_t i = 0; i < r->r.edges.size(); ++i) pairs[2 * i] = r->r.edges[i].first, pairs[2 * i + 1] = r->r.edges[i].second;
    return FBN_OK;
}
static constexpr int32_t kPcRecordMagic = 0x52504246;  // 'FBPR': fbn_pc_result_record layout version 1
int fbn_pc_sepsets(const fbn_pc_result *r, int32_t *buf, int64_t cap, int64_t *len) {
    if (!r) return SetError(FBN_ERR_ARG, "null pointer");
    int64_t k = 0;
    auto put = [&](int32_t v) {
        if (buf && k < cap) buf[k] = v;
        ++k;
    };
    const auto &sm = r->r.sepset;
    for (size_t i = 0, n = sm.sorted_size(); i < n; ++i) {
        const auto key = sm.key(i);
        const auto z = sm.value(i);
        put(key.first);
        put(key.second);
        put((int32_t)z.size());
        for (int v : z) put(v);
    }
    if (len) *len = k;
    return FBN_OK;
}
int fbn_pc_result_record(const fbn_pc_result *r, int32_t *buf, int64_t cap, int64_t *len) {
    if (!r) return SetError(FBN_ERR_ARG, "null pointer");
    int64_t k = 0;
    auto put = [&](int32_t v) {
        if (buf && k < cap) buf[k] = v;
        ++k;
    };
    const auto &R = r->r;
    put(kPcRecordMagic);
    put((int32_t)R.tests_per_level.size());
    for (int64_t t : R.tests_per_level) put((int32_t)(uint32_t)(uint64_t)t), put((int32_t)((uint64_t)t >> 32));
    put((int32_t)R.edges.size());
    for (auto &e : R.edges) put(e.first), put(e.second);
    int64_t slen = 0;
    fbn_pc_sepsets(r, nullptr, 0, &slen);
    put((int32_t)slen);
    if (buf && k + slen <= cap) fbn_pc_sepsets(r, buf + k, slen, nullptr);
    k += slen;
    if (len) *len = k;
    if (buf && k > cap) return SetError(FBN_ERR_LIMIT, "record needs %lld ints (cap %lld)", (long long)k, (long long)cap);
    return FBN_OK;
}
int fbn_pc_small_eligible(const fbn_ci_ctx *c, int group_size, int *eligible) {
    if (!c || !eligible) return SetError(FBN_ERR_ARG, "null pointer");
    *eligible = fbn::CiPCSmallEligible(c, group_size) ? 1 : 0;
    return FBN_OK;
}
int fbn_pc_small_eligible_shape(int nvars, int64_t nsamples, const int32_t *dims, int group_size, int *eligible) {
    if (!eligible || (nvars > 0 && !dims)) return SetError(FBN_ERR_ARG, "null pointer");
    *eligible = fbn::PCSmallShape(nvars, nsamples, dims, group_size) ? 1 : 0;
    return FBN_OK;
}
int fbn_pc_level(fbn_ci_ctx *c, double alpha, int d, int group_size, const int32_t *edges, int64_t nedges,
                 int64_t e_begin, int64_t e_end, uint8_t *removed, int32_t *sepsets, int64_t *counted,
                 int64_t *launched) {
    if (!c || d < 0 || d > 8 || group_size < 1 || group_size > 8 || nedges < 0 || (nedges && !edges) ||
        e_begin < 0 || e_end < e_begin || e_end > nedges || (e_end > e_begin && !removed))
        return SetError(FBN_ERR_ARG, "bad argument");
    fbn::Skeleton sk;
    sk.Reset(c->nvars);
    auto &ev = sk.edges;
    ev.resize((size_t)nedges);
    for (int64_t i = 0; i < nedges; ++i) {
        const int a = edges[2 * i], b = edges[2 * i + 1];
        if (a < 0 || b <= a || b >= c->nvars) return SetError(FBN_ERR_ARG, "edge %lld must be (x < y) in range", (long long)i);
        if (i && !(ev[i - 1] < std::make_pair(a, b))) return SetError(FBN_ERR_ARG, "edges must be in (x, y) lexicographic order");
        ev[i] = {a, b};
    }
    sk.RebuildAdj(false);
    FBN_HIP(hipSetDevice(c->device));
    fbn::PCResultHost scratch;
    fbn::LevelOut out;
    int rc = fbn::RunLevel(c, alpha, d, group_size, sk, (size_t)e_begin, (size_t)e_end, out, scratch);
    if (rc) return rc;
    for (int64_t e = 0; e < e_end - e_begin; ++e) {
        removed[e] = out.removed[e] ? 1 : 0;
        if (sepsets)
            for (int j = 0; j < d; ++j) sepsets[e * d + j] = out.removed[e] ? out.sep[(size_t)e * d + j] : -1;
    }
    if (counted) *counted = out.counted;
    if (launched) *launched = out.launched;
    return FBN_OK;
}
int fbn_pc_orient_skeleton(int nvars, const int32_t *pairs, int nedges, const int32_t *sepsets, int64_t len,
                           fbn_pc_result **out) {
    if (nvars <= 0 || nedges < 0 || (nedges && !pairs) || (len && !sepsets) || !out)
        return SetError(FBN_ERR_ARG, "bad argument");
    auto r = std::unique_ptr<fbn_pc_result>(new (std::nothrow) fbn_pc_result());
    if (!r) return SetError(FBN_ERR_NOMEM, "out of memory");
    for (int i = 0; i < nedges; ++i) {
        const int a = pairs[2 * i], b = pairs[2 * i + 1];
        if (a < 0 || b < 0 || a >= nvars || b >= nvars || a == b) return SetError(FBN_ERR_ARG, "bad edge %d", i);
        r->r.edges.push_back({std::min(a, b), std::max(a, b)});
    }
    for (int64_t k = 0; k < len;) {  // (x, y, m, z_0..z_{m-1}) records, as fbn_pc_sepsets writes them
        if (k + 3 > len || k + 3 + sepsets[k + 2] > len || sepsets[k + 2] < 0) return SetError(FBN_ERR_ARG, "bad sepset list");
        const int x = sepsets[k], y = sepsets[k + 1], m = sepsets[k + 2];
        r->r.sepset.set({std::min(x, y), std::max(x, y)}, sepsets + k + 3, m);
        k += 3 + m;
    }
    int rc = fbn::OrientPC(nvars, r->r);
    if (rc) return rc;
    *out = r.release();
    return FBN_OK;
}
int fbn_pc_num_oriented_edges(const fbn_pc_result *r, int *n) {
    if (!r || !n) return SetError(FBN_ERR_ARG, "null pointer");
    *n = (int)r->r.oriented.size();
    return FBN_OK;
}
int fbn_pc_oriented_edges(const fbn_pc_result *r, int32_t *triples) {
    if (!r || !triples) return SetError(FBN_ERR_ARG, "null pointer");
    for (size_t i = 0; i < r->r.oriented.size(); ++i)
        for (int k = 0; k < 3; ++k) triples[3 * i + k] = r->r.oriented[i][k];
    return FBN_OK;
}
int fbn_shd_bif(const char *bif_path, int nvars, const int32_t *triples, int n, int *shd) {
    if (!bif_path || !shd || n < 0 || (n && !triples)) return SetError(FBN_ERR_ARG, "bad argument");
    std::vector<std::string> names;
    std::vector<std::pair<int, int>> arcs;
    int rc = fbn::LoadBifGraph(bif_path, names, arcs);
    if (rc) return rc;
    if ((int)names.size() != nvars)
        return SetError(FBN_ERR_ARG, "%s has %zu variables, the learned graph %d", bif_path, names.size(), nvars);
    std::vector<std::array<int, 3>> learned(n);
    for (int i = 0; i < n; ++i) {
        learned[i] = {triples[3 * i], triples[3 * i + 1], triples[3 * i + 2] ? 1 : 0};
        if (learned[i][0] < 0 || learned[i][0] >= nvars || learned[i][1] < 0 || learned[i][1] >= nvars)
            return SetError(FBN_ERR_ARG, "edge %d out of range", i);
    }
    int unl = 0;
    return fbn::ComputeSHD(nvars, arcs, learned, shd, &unl);
}
int fbn_pc_shd_bif(const fbn_pc_result *r, const char *bif_path, int *shd) {
    if (!r || !bif_path || !shd) return SetError(FBN_ERR_ARG, "null pointer");
    std::vector<int32_t> t(3 * r->r.oriented.size() + 3);
    for (size_t i = 0; i < r->r.oriented.size(); ++i)
        for (int k = 0; k < 3; ++k) t[3 * i + k] = r->r.oriented[i][k];
    return fbn_shd_bif(bif_path, r->r.num_nodes, t.data(), (int)r->r.oriented.size(), shd);
}
int fbn_pc_device_bytes(const fbn_pc_result *r, int64_t *bytes) {
    if (!r || !bytes) return SetError(FBN_ERR_ARG, "null pointer");
    *bytes = r->r.device_bytes;
    return FBN_OK;
}
int fbn_pc_path(const fbn_pc_result *r, int *path) {
    if (!r || !path) return SetError(FBN_ERR_ARG, "null pointer");
    *path = r->r.path;
    return FBN_OK;
}
int fbn_pc_timing(const fbn_pc_result *r, double *total_s, double *kernel_s) {
    if (!r) return SetError(FBN_ERR_ARG, "null pointer");
    if (total_s) *total_s = r->r.total_s;
    if (kernel_s) *kernel_s = r->r.kernel_s;
    return FBN_OK;
}
int fbn_pc_result_destroy(fbn_pc_result *r) {
    delete r;
    return FBN_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ driver seam
namespace fbn {
void CiCtxShape(const fbn_ci_ctx *c, int *nvars, int64_t *nsamples) {
    *nvars = c->nvars;
    *nsamples = c->N;
}
// batches up to this many item bytes take the zero-copy path of CiBatchLaunch
constexpr size_t kZeroCopyBytes = 256 << 10;
const int32_t *CiCtxDims(const fbn_ci_ctx *c) { return c->dims.data(); }
void CiSetPairMode(fbn_ci_ctx *c, int mode) {
    c->pair_mode = mode;
    if (mode == 1) c->l1mi_covered = 0;  // a new level 0 records from pair 0
    if (mode != 2) c->pairs_recorded = false;
}
int CiBatchLaunch(fbn_ci_ctx *c, int k, const int32_t *items, int64_t n, int d, double alpha, bool want_df,
                  const CiBatchStats *pre) {
    CiSlot &S = c->slot[k];
    S.n = n;
    S.want_df = want_df;
    if (n == 0) return FBN_OK;
    // pinned staging: the copies are true DMA on the ctx stream, one host sync per round
    const size_t ib = (size_t)n * (2 + d) * 4, rb = (size_t)n * 5 + 8;
    int rc;
    if ((rc = PinnedEnsure(S.h_items, S.h_items_bytes, ib))) return rc;
    if ((rc = PinnedEnsure(S.h_res, S.h_res_bytes, rb))) return rc;
    memcpy(S.h_items, items, ib);
    uint8_t *h_ind = static_cast<uint8_t *>(S.h_res);
    int32_t *h_df = reinterpret_cast<int32_t *>(h_ind + (((size_t)n + 3) & ~(size_t)3));
    const int32_t *hi = static_cast<const int32_t *>(S.h_items);
    // small rounds (the latency-bound ones): the kernel reads the items from and writes the
    // decisions to the pinned buffers directly (one launch + one sync per round); large rounds
    // stage through device memory with DMA copies
    S.zc = ib <= kZeroCopyBytes && !fbn::KnobSet("FBN_CI_NO_ZEROCOPY");
    CiBatchReq q;
    q.items = hi, q.n = n, q.d = d, q.alpha = alpha;
    q.k = k;
    q.pre = pre;
    if (S.zc) q.zc_items = hi, q.zc_indep = h_ind, q.zc_df = want_df ? h_df : nullptr;
    if ((rc = CiLaunchDevice(c, q, c->stream))) return rc;
    if (!S.zc) {
        FBN_HIP(hipMemcpyAsync(h_ind, S.indep.p, (size_t)n, hipMemcpyDeviceToHost, c->stream));
        if (want_df) FBN_HIP(hipMemcpyAsync(h_df, S.df.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    }
    FBN_HIP(hipEventRecord(S.done, c->stream));
    return FBN_OK;
}
bool CiAllPairsEligible(const fbn_ci_ctx *c, const CiBatchStats &st) { return CiBitsEligible(c, st.maxdim); }
int CiBatchLaunchAllPairs(fbn_ci_ctx *c, double alpha, const CiBatchStats *pre, int64_t t0, int64_t n,
                          bool copy_flags) {
    CiSlot &S = c->slot[0];
    S.n = n;
    S.want_df = false;
    S.zc = false;
    if (n == 0) return FBN_OK;
    int rc;
    if ((rc = PinnedEnsure(S.h_res, S.h_res_bytes, (size_t)n * 5 + 8))) return rc;
    CiBatchReq q;
    q.n = n, q.d = 0, q.alpha = alpha;
    q.pre = pre;
    q.all_pairs = true, q.pair0 = t0;
    if ((rc = CiLaunchDevice(c, q, c->stream))) return rc;
    if (copy_flags) FBN_HIP(hipMemcpyAsync(S.h_res, S.indep.p, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    FBN_HIP(hipEventRecord(S.done, c->stream));
    return FBN_OK;
}

bool CiPairsReady(const fbn_ci_ctx *c) { return c->pair_mode == 2 && c->pairs_recorded; }

// Decided before the level-0 launch, so the bit-sliced store the device hand-off reads is built
// here when the dataset qualifies for it (the same test as CiLaunchDevice's bits path): a fresh ctx
// -- every one-shot CLI run -- takes the device path from its first PC run on.
bool CiL0L1DeviceEligible(fbn_ci_ctx *c, int group_size) {
    if (group_size != 1 || fbn::KnobSet("FBN_PC_HOST_L1") || fbn::KnobSet("FBN_PC_HOST_L0L1") || c->nvars < 2) return false;
    const int maxdim = *std::max_element(c->dims.begin(), c->dims.end());
    if (maxdim > 4) return false;
    if (!c->bits_ready && (!CiBitsEligible(c, maxdim) || CiBitsEnsure(c, c->stream) != FBN_OK)) return false;
    return true;
}

int CiL0L1Device(fbn_ci_ctx *c, int64_t P, int *E, int64_t *cands, PCResultHost &res) {
    const int n = c->nvars;
    if (P != (int64_t)n * (n - 1) / 2 || P > INT32_MAX / 2) return SetError(FBN_ERR_ARG, "level 0 -> 1 on the device: one complete-graph batch");
    FBN_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    CiSlot &S = c->slot[0];
    int rc;
    if ((rc = c->kcnt.ensure((size_t)n * 8)) || (rc = c->kscal.ensure(16)) || (rc = c->l1adjoff.ensure((size_t)(n + 1) * 4)) ||
        (rc = c->l1adj.ensure((size_t)std::max<int64_t>(2 * P, 1) * 4)) || (rc = c->l1pairs.ensure((size_t)std::max<int64_t>(P, 1) * 8)) ||
        (rc = c->kupoff.ensure((size_t)n * 4)))
        return rc;
    if (!c->h_kept) {
        hipError_t e = hipHostMalloc((void **)&c->h_kept, 16, hipHostMallocDefault);
        if (e != hipSuccess) return SetError(FBN_ERR_NOMEM, "hipHostMalloc: %s", hipGetErrorString(e));
    }
    if (!c->side) {
        FBN_HIP(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
        FBN_HIP(hipEventCreateWithFlags(&c->side_ev, hipEventDisableTiming));
        FBN_HIP(hipEventCreateWithFlags(&c->main_ev, hipEventDisableTiming));
    }
    // the decision flags to the host on the side stream, behind the level-0 kernels
    FBN_HIP(hipStreamWaitEvent(c->side, S.done, 0));
    FBN_HIP(hipMemcpyAsync(S.h_res, S.indep.p, (size_t)P, hipMemcpyDeviceToHost, c->side));
    int32_t *cnt = c->kcnt.as<int32_t>();
    hipError_t e = fbn_ci_kept_csr(S.indep.as<uint8_t>(), n, cnt, cnt + n, c->l1adjoff.as<int32_t>(), c->kupoff.as<int32_t>(),
                                   c->l1adj.as<int32_t>(), c->l1pairs.as<int32_t>(), c->kscal.as<long long>(), s);
    if (e != hipSuccess) return SetError(FBN_ERR_HIP, "kept-pair CSR: %s", hipGetErrorString(e));
    long long *hk = reinterpret_cast<long long *>(c->h_kept);
    FBN_HIP(hipMemcpyAsync(hk, c->kscal.p, 16, hipMemcpyDeviceToHost, s));
    FBN_HIP(hipEventRecord(c->main_ev, s));
    FBN_HIP(hipEventSynchronize(c->main_ev));
    *E = (int)hk[0];
    *cands = hk[1];
    // the edge list to the host on the side stream (the CSR kernels are done: main_ev)
    if ((rc = PinnedEnsure(c->h_pairs, c->h_pairs_bytes, (size_t)std::max(*E, 1) * 8))) return rc;
    FBN_HIP(hipStreamWaitEvent(c->side, c->main_ev, 0));
    if (*E) FBN_HIP(hipMemcpyAsync(c->h_pairs, c->l1pairs.p, (size_t)*E * 8, hipMemcpyDeviceToHost, c->side));
    FBN_HIP(hipEventRecord(c->side_ev, c->side));
    // the level-0 batch in the run's accounting (as CiBatchWait)
    float ms = 0.f;
    if (c->timing) FBN_HIP(hipEventElapsedTime(&ms, S.ev0, S.ev1));
    res.kernel_s += ms * 1e-3;
    res.device_bytes += S.last_bytes;
    S.n = 0;
    return FBN_OK;
}

int CiL0L1Host(fbn_ci_ctx *c, int64_t P, int E, std::vector<char> &removed, Skeleton &sk) {
    FBN_HIP(hipEventSynchronize(c->side_ev));
    removed.resize((size_t)P);
    memcpy(removed.data(), c->slot[0].h_res, (size_t)P);
    static_assert(sizeof(std::pair<int, int>) == 8, "pair layout");
    sk.edges.resize((size_t)E);
    if (E) memcpy(static_cast<void *>(sk.edges.data()), c->h_pairs, (size_t)E * 8);
    sk.RebuildAdj(true);
    return FBN_OK;
}
int CiPairTablesCopy(fbn_ci_ctx *c, int64_t p0, int64_t np, void *buf, bool buf_on_device, bool to_ctx) {
    if (np < 0 || p0 < 0) return SetError(FBN_ERR_ARG, "bad pair range");
    const int64_t P = (int64_t)c->nvars * (c->nvars - 1) / 2;
    if (p0 + np > P) return SetError(FBN_ERR_ARG, "pair range [%lld, %lld) beyond %lld pairs", (long long)p0,
                                     (long long)(p0 + np), (long long)P);
    FBN_HIP(hipSetDevice(c->device));
    int rc;
    if ((rc = c->pairtab.ensure(std::max<size_t>((size_t)P, 1) * 16 * 4))) return rc;
    if (!to_ctx && !c->pairs_recorded) return SetError(FBN_ERR_ARG, "no pair tables recorded on this context");
    char *ctx_ptr = c->pairtab.as<char>() + (size_t)p0 * 64;
    const size_t bytes = (size_t)np * 64;
    const hipMemcpyKind kind = to_ctx ? (buf_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice)
                                      : (buf_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost);
    FBN_HIP(hipStreamSynchronize(c->stream));
    if (bytes) FBN_HIP(hipMemcpy(to_ctx ? (void *)ctx_ptr : buf, to_ctx ? (const void *)buf : ctx_ptr, bytes, kind));
    return FBN_OK;
}
int CiMarginReset(fbn_ci_ctx *c) {
    FBN_HIP(hipSetDevice(c->device));
    return CiResetMargin(c);
}
int CiMarginRead(fbn_ci_ctx *c, double *min_margin, int64_t *near_alpha) {
    FBN_HIP(hipSetDevice(c->device));
    return CiReadMargin(c, min_margin, near_alpha);
}
bool CiPairsRecorded(const fbn_ci_ctx *c) { return c->pairs_recorded; }
void CiSetPairsRecorded(fbn_ci_ctx *c) {
    c->pair_mode = 2;
    c->pairs_recorded = true;
}
// A PC run's level 1 (group size 1) entirely on the device: ci_l1.hip's ci_l1_* kernels keep every
// edge's search state in device memory, generate each round's tests from the adjacency, count them
// from the bit-sliced store + pair tables, decide and resolve each edge's prefix in order; the host
// enqueues rounds (next chunk x4, FBN_PC_ROUND0 / FBN_PC_GROWTH as the host driver) and reads one
// open-edge count per round, one round behind, to stop.  Results equal the host driver's: the same
// tests in the same per-edge order and the same first-independent rule.  *done = false when not
// eligible (the host driver runs the level).
// Rounds are unbounded: the per-round open count lives in a two-entry ring (round r writes entry
// r & 1, the host reads round r - 1's entry while round r runs).  The per-edge chunk is clamped so
// a round's exclusive scan of the lengths (int32 offsets, hipcub) cannot overflow: E * chunk < 2^31.
constexpr int kL1Ring = 2;
int CiLevel1Device(fbn_ci_ctx *c, double alpha, const Skeleton &sk, size_t e_begin, size_t e_end, LevelOut &out,
                   PCResultHost &res, bool *done) {
    *done = false;
    if (c->pair_mode != 2 || !c->pairs_recorded || !c->bits_ready || fbn::KnobSet("FBN_PC_HOST_L1")) return FBN_OK;
    const int nv = c->nvars;
    for (int v = 0; v < nv; ++v)
        if (c->dims[v] > 4) return FBN_OK;
    const int E = (int)(e_end - e_begin);
    int64_t cands = 0;  // every candidate set of the range: the most one round could hold
    for (size_t e = e_begin; e < e_end; ++e) cands += sk.EdgeCost(e, 1);
    // a level the host driver takes in one round (full speculation, ALARM-size) stays there: one
    // launch instead of a round's seven
    if (cands <= fbn::KnobOr("FBN_PC_FULLSPEC", 16384)) return FBN_OK;
    if (E == 0) {
        out.removed.clear(), out.sep.clear(), out.d = 1, out.counted = out.launched = 0;
        *done = true;
        return FBN_OK;
    }
    const bool ptiming = fbn::PcTiming();  // diagnostic
    auto tq0 = Clock::now();
    FBN_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int rc;
    static thread_local std::vector<int32_t> adjf, adj_off;  // (capacity kept across runs)
    adjf.clear();
    adj_off.assign(nv + 1, 0);
    for (int u = 0; u < nv; ++u) {
        adj_off[u] = (int32_t)adjf.size();
        adjf.insert(adjf.end(), sk.adj[u].begin(), sk.adj[u].end());
    }
    adj_off[nv] = (int32_t)adjf.size();
    if ((rc = c->l1pairs.ensure((size_t)E * 8)) || (rc = c->l1adj.ensure(std::max<size_t>(adjf.size(), 1) * 4)) ||
        (rc = c->l1adjoff.ensure((size_t)(nv + 1) * 4)))
        return rc;
    static_assert(sizeof(std::pair<int, int>) == 8, "pair layout");
    FBN_HIP(hipMemcpyAsync(c->l1pairs.p, sk.edges.data() + e_begin, (size_t)E * 8, hipMemcpyHostToDevice, s));
    if (!adjf.empty()) FBN_HIP(hipMemcpyAsync(c->l1adj.p, adjf.data(), adjf.size() * 4, hipMemcpyHostToDevice, s));
    FBN_HIP(hipMemcpyAsync(c->l1adjoff.p, adj_off.data(), (size_t)(nv + 1) * 4, hipMemcpyHostToDevice, s));
    if (ptiming)
        fprintf(stderr, "  level 1 device setup (host): %.3f ms\n", Ms(tq0, Clock::now()));
    *done = true;
    return CiLevel1Run(c, alpha, E, cands, out, res, nullptr);
}

// The level-1 rounds over the edge list / adjacency already in c->l1pairs / l1adj / l1adjoff (E
// edges, `cands` candidate sets in all); host_work (optional) runs once, after the first round is
// enqueued, while the device works.
int CiLevel1Run(fbn_ci_ctx *c, double alpha, int E, int64_t cands, LevelOut &out, PCResultHost &res,
                const std::function<int()> &host_work) {
    const int nv = c->nvars;
    out.removed.assign(E, 0);
    out.d = 1;
    out.sep.assign(E, -1);
    out.counted = out.launched = 0;
    FBN_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int rc;
    const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(cands, fbn::KnobOr("FBN_PC_L1CAP", 1 << 19)));
    if ((rc = c->l1ed.ensure((size_t)E * fbn_ci_l1_edge_bytes())) ||
        (rc = c->l1pos.ensure((size_t)E * 4)) || (rc = c->l1st.ensure((size_t)E)) ||
        (rc = c->l1sep.ensure((size_t)E * 4)) || (rc = c->l1cnt.ensure((size_t)E * 8)) ||
        (rc = c->l1len.ensure((size_t)E * 4)) || (rc = c->l1off.ensure((size_t)E * 4)) ||
        (rc = c->l1scal.ensure(96)) || (rc = c->l1open.ensure(kL1Ring * 4)) ||
        (rc = c->l1sstat.ensure((size_t)((E + 255) / 256) * 8)) ||
        (rc = c->l1items.ensure((size_t)cap * 12)) || (rc = c->l1counts.ensure((size_t)cap * 256)) ||
        (rc = c->l1df.ensure((size_t)cap * 4)) || (rc = c->l1indep.ensure((size_t)cap)))
        return rc;
    if (!c->h_open) {
        hipError_t e = hipHostMalloc((void **)&c->h_open, kL1Ring * 4, hipHostMallocDefault);
        if (e != hipSuccess) return SetError(FBN_ERR_NOMEM, "hipHostMalloc: %s", hipGetErrorString(e));
        for (auto &ev : c->l1ev) FBN_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    const double *band = nullptr;
    int nband = 0;
    if ((rc = CiBand(c, alpha, s, &band, &nband))) return rc;
    // scalars (total, launched, rows read, scan flag, tickets; the screen's scan at + 8) and the tile
    // scan's status words (epoch 0)
    FBN_HIP(hipMemsetAsync(c->l1scal.p, 0, 96, s));
    FBN_HIP(hipMemsetAsync(c->l1sstat.p, 0, (size_t)((E + 255) / 256) * 8, s));
    // the information screen (exact; FBN_PC_NO_MISCREEN=1: every candidate runs): needs the band (a
    // decision threshold per df) and the level-0 pair tables of the complete graph
    double *mi = nullptr;
    const bool mi_from_tables = c->l1mi_covered != (int64_t)nv * (nv - 1) / 2;
    if (band && !fbn::KnobSet("FBN_PC_NO_MISCREEN")) {
        const long long P = (long long)nv * (nv - 1) / 2;
        if ((rc = c->l1mi.ensure((size_t)std::max<long long>(P, 1) * 8)) ||
            (rc = c->l1plist.ensure((size_t)std::max<int64_t>(cands, 1) * 4)) ||
            (rc = c->l1pcnt.ensure((size_t)E * 4)) || (rc = c->l1sstat2.ensure((size_t)((E + 255) / 256) * 8)))
            return rc;
        FBN_HIP(hipMemsetAsync(c->l1sstat2.p, 0, (size_t)((E + 255) / 256) * 8, s));
        mi = c->l1mi.as<double>();
    }
    CiSlot &S = c->slot[0];
    if (c->timing) FBN_HIP(hipEventRecord(S.ev0, s));
    long long *scal = c->l1scal.as<long long>();  // total, launched, rows read, scan flag, tickets
    int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(32, fbn::KnobOr("FBN_PC_ROUND0", 8192) / E));
    // chunk x2 per round: rounds here cost a few launches, speculation costs counted tests (config 5:
    // x4 launches 430k tests for 294k counted, x2 345k)
    const int64_t growth = std::max<int64_t>(2, fbn::KnobOr("FBN_PC_GROWTH", 2));
    // (FBN_PC_L1_MAXCHUNK: tuning -- a cap on the per-edge chunk trades speculative tests for rounds)
    const int64_t max_chunk = std::max<int64_t>(
        1, std::min<int64_t>(std::min<int64_t>(1 << 16, fbn::KnobOr("FBN_PC_L1_MAXCHUNK", 1 << 16)), (int64_t)INT32_MAX / E));
    chunk = std::min(chunk, max_chunk);
    // the setup writes round 0's lengths and zeroes the open-count ring; each round's resolve writes
    // the next round's lengths and zeroes the other ring slot (no length kernel or memset per round)
    CiL1Args a{};
    a.pairs = c->l1pairs.as<int32_t>();
    a.adj = c->l1adj.as<int32_t>(), a.adj_off = c->l1adjoff.as<int32_t>();
    a.E = E, a.nv = nv, a.num_cu = c->num_cu;
    a.ed = c->l1ed.p, a.pos = c->l1pos.as<int32_t>(), a.st = c->l1st.as<uint8_t>();
    a.sep = c->l1sep.as<int32_t>(), a.counted = c->l1cnt.as<long long>();
    a.len = c->l1len.as<int32_t>(), a.off = c->l1off.as<int32_t>();
    a.ring = c->l1open.as<unsigned>(), a.sstat = c->l1sstat.as<unsigned long long>();
    a.scal = scal, a.cap = cap, a.chunk0 = (int)chunk;
    a.bits = c->bits.as<uint32_t>(), a.W = c->bits_W;
    a.dims = c->ddims.as<int32_t>(), a.row0 = c->brow.as<int32_t>();
    a.pairtab = c->pairtab.as<int32_t>();
    a.items = c->l1items.as<int32_t>(), a.counts = c->l1counts.as<int32_t>(), a.df = c->l1df.as<int32_t>();
    a.indep = c->l1indep.as<uint8_t>();
    a.alpha = alpha, a.stats = c->stats.as<unsigned long long>();
    a.band = band, a.nband = nband;
    a.mi = mi, a.mi_from_tables = mi_from_tables ? 1 : 0, a.two_n = 2.0 * (double)c->N;
    a.pcnt = c->l1pcnt.as<int32_t>(), a.plist = mi ? c->l1plist.as<int32_t>() : nullptr;
    a.sstat2 = c->l1sstat2.as<unsigned long long>(), a.scal2 = scal + 8;
    hipError_t e = fbn_ci_l1_setup(&a, s);
    if (e != hipSuccess) return SetError(FBN_ERR_HIP, "ci level-1 setup: %s", hipGetErrorString(e));
    const bool l1timing = fbn::PcTiming();  // diagnostic
    const auto tl0 = Clock::now();
    int rounds = 0;
    for (int r = 0;; ++r) {
        rounds = r + 1;
        unsigned *open_r = c->l1open.as<unsigned>() + (r & 1);
        const int64_t next_chunk = std::min<int64_t>(chunk * growth, max_chunk);
        e = fbn_ci_l1_round(&a, open_r, c->l1open.as<unsigned>() + ((r + 1) & 1), (int)next_chunk, (unsigned)(r + 2), s);
        if (e != hipSuccess) return SetError(FBN_ERR_HIP, "ci level-1 round: %s", hipGetErrorString(e));
        FBN_HIP(hipMemcpyAsync(c->h_open + (r & 1), open_r, 4, hipMemcpyDeviceToHost, s));
        FBN_HIP(hipEventRecord(c->l1ev[r & 1], s));
        if (r == 0 && host_work)  // (while the first round runs)
            if ((rc = host_work())) return rc;
        if (r >= 1) {  // round r - 1's open count, while round r runs
            FBN_HIP(hipEventSynchronize(c->l1ev[(r - 1) & 1]));
            if (c->h_open[(r - 1) & 1] == 0) break;  // round r found nothing to do
        }
        chunk = next_chunk;
    }
    if (c->timing) FBN_HIP(hipEventRecord(S.ev1, s));
    const auto tl1 = Clock::now();
    // results straight into one pinned buffer by a kernel (zero-copy writes; no DMA copies):
    // [scalars 32 | sepsets 4E | removal flags E]
    if ((rc = PinnedEnsure(c->h_xfer, c->h_xfer_bytes, (size_t)E * 5 + 40))) return rc;
    if ((rc = c->l1part.ensure(256 * 8))) return rc;
    char *hx = static_cast<char *>(c->h_xfer);
    long long *sc = reinterpret_cast<long long *>(hx);
    int32_t *hsep = reinterpret_cast<int32_t *>(hx + 32);
    char *hrm = hx + 32 + (size_t)E * 4;
    e = fbn_ci_l1_results(c->l1st.as<uint8_t>(), c->l1sep.as<int32_t>(), c->l1cnt.as<long long>(), E, scal, hrm, hsep, sc,
                          c->l1part.as<long long>(), s);
    if (e != hipSuccess) return SetError(FBN_ERR_HIP, "ci level-1 results: %s", hipGetErrorString(e));
    FBN_HIP(hipStreamSynchronize(s));
    if (sc[3]) return SetError(FBN_ERR_HIP, "level-1 offset scan: look-back timed out");
    std::memcpy(out.sep.data(), hsep, (size_t)E * 4);
    std::memcpy(out.removed.data(), hrm, (size_t)E);
    out.counted = sc[0];
    out.launched = sc[1];
    if (l1timing)
        fprintf(stderr, "  level 1 device rounds: %d, loop %.3f ms, read-back + results %.3f ms\n", rounds, Ms(tl0, tl1),
                Ms(tl1, Clock::now()));
    if (c->timing) {
        float ms = 0.f;
        FBN_HIP(hipEventElapsedTime(&ms, S.ev0, S.ev1));
        res.kernel_s += ms * 1e-3;
    }
    res.device_bytes += sc[2] * c->bits_W * 4;
    return FBN_OK;
}

struct FlagIsZero {
    __host__ __device__ bool operator()(uint8_t f) const { return f == 0; }
};
// the pairs (i < j) of the complete graph kept (decision 0) by the last all-pairs batch (slot 0:
// pairs [t0, t0 + P)), appended to `kept` in pair order: compacted on the device, only the kept
// indices cross PCIe
int CiAllPairsKept(fbn_ci_ctx *c, int64_t t0, int64_t P, std::vector<std::pair<int, int>> &kept) {
    if (P <= 0) return FBN_OK;
    if (P > INT32_MAX) return SetError(FBN_ERR_LIMIT, "too many pairs for the kept-pair compaction");
    FBN_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    CiSlot &S = c->slot[0];
    hipcub::CountingInputIterator<int32_t> in(0);
    hipcub::TransformInputIterator<bool, FlagIsZero, const uint8_t *> flags(S.indep.as<uint8_t>(), FlagIsZero());
    size_t tmp = 0;
    FBN_HIP(hipcub::DeviceSelect::Flagged(nullptr, tmp, in, flags, (int32_t *)nullptr, (int *)nullptr, (int)P, s));
    int rc;
    if ((rc = c->kepttmp.ensure(std::max<size_t>(tmp, 16) + 16)) || (rc = c->keptidx.ensure((size_t)P * 4))) return rc;
    if (!c->h_kept) {
        hipError_t e = hipHostMalloc((void **)&c->h_kept, 16, hipHostMallocDefault);
        if (e != hipSuccess) return SetError(FBN_ERR_NOMEM, "hipHostMalloc: %s", hipGetErrorString(e));
    }
    int *d_num = reinterpret_cast<int *>(c->kepttmp.as<char>() + std::max<size_t>(tmp, 16));
    FBN_HIP(hipcub::DeviceSelect::Flagged(c->kepttmp.p, tmp, in, flags, c->keptidx.as<int32_t>(), d_num, (int)P, s));
    FBN_HIP(hipMemcpyAsync(c->h_kept, d_num, 4, hipMemcpyDeviceToHost, s));
    FBN_HIP(hipStreamSynchronize(s));
    const int nk = c->h_kept[0];
    if ((rc = PinnedEnsure(c->h_xfer, c->h_xfer_bytes, (size_t)std::max(nk, 1) * 4))) return rc;
    const int32_t *idx = static_cast<const int32_t *>(c->h_xfer);
    if (nk) {
        FBN_HIP(hipMemcpyAsync(c->h_xfer, c->keptidx.p, (size_t)nk * 4, hipMemcpyDeviceToHost, s));
        FBN_HIP(hipStreamSynchronize(s));
    }
    const size_t base = kept.size();
    kept.resize(base + (size_t)nk);
    const int n = c->nvars;
    int i = 0;
    int64_t row0 = 0, row1 = n - 1;  // pair indices of row i: [row0, row1)
    for (int t = 0; t < nk; ++t) {
        const int64_t q = t0 + idx[t];
        while (q >= row1) ++i, row0 = row1, row1 += n - 1 - i;
        kept[base + t] = {i, i + 1 + (int)(q - row0)};
    }
    return FBN_OK;
}
int CiBatchWait(fbn_ci_ctx *c, int k, uint8_t *indep, int32_t *df, PCResultHost &res) {
    CiSlot &S = c->slot[k];
    const int64_t n = S.n;
    if (n == 0) return FBN_OK;
    const bool timing = fbn::PcTiming();  // diagnostic
    auto t1 = std::chrono::steady_clock::now();
    FBN_HIP(hipEventSynchronize(S.done));
    auto t2 = std::chrono::steady_clock::now();
    const uint8_t *h_ind = static_cast<const uint8_t *>(S.h_res);
    memcpy(indep, h_ind, (size_t)n);
    if (df && S.want_df) memcpy(df, h_ind + (((size_t)n + 3) & ~(size_t)3), (size_t)n * 4);
    if (timing)
        fprintf(stderr, "  ci batch slot %d n=%lld: wait %.1f us\n", k, (long long)n,
                std::chrono::duration<double, std::micro>(t2 - t1).count());
    float ms = 0.f;
    if (c->timing) FBN_HIP(hipEventElapsedTime(&ms, S.ev0, S.ev1));
    res.kernel_s += ms * 1e-3;
    res.device_bytes += S.last_bytes;
    S.n = 0;
    return FBN_OK;
}
int CiRunBatch(fbn_ci_ctx *c, const int32_t *items, int64_t n, int d, double alpha, uint8_t *indep, int32_t *df,
               PCResultHost &res) {
    int rc = CiBatchLaunch(c, 0, items, n, d, alpha, df != nullptr);
    if (rc) return rc;
    return CiBatchWait(c, 0, indep, df, res);
}

// the device-resident search's domain: <= 64 variables of <= 4 states, group size 1.  N cap: one
// test's samples bound the workgroups' skew at a grid barrier (its spin limit is 2 s)
bool PCSmallShape(int nvars, int64_t N, const int32_t *dims, int group_size) {
    if (group_size != 1 || nvars < 2 || nvars > kSmallMaxVars || N < 1 || N > (1ll << 24) || fbn::KnobSet("FBN_PC_NO_SMALL"))
        return false;
    for (int v = 0; v < nvars; ++v)
        if (dims[v] < 1 || dims[v] > 4) return false;
    return true;
}
bool CiPCSmallEligible(const fbn_ci_ctx *c, int group_size) {
    return PCSmallShape(c->nvars, c->N, c->dims.data(), group_size);
}

int CiPCSmall(fbn_ci_ctx *c, double alpha, int depth, PCResultHost &res, Skeleton &sk, int *levels, bool *handoff,
              bool *fellback) {
    *levels = 0;
    *handoff = false;
    *fellback = false;
    const bool htime = fbn::PcTiming();  // diagnostic: host phases of the call
    const auto h0 = Clock::now();
    FBN_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int rc;
    if ((rc = CiBitsEnsure(c, s)) || (rc = CiPack2Ensure(c, s))) return rc;
    const double *band = nullptr;
    int nband = 0;
    if ((rc = CiBand(c, alpha, s, &band, &nband, kBandDfMax))) return rc;
    // the host-driven levels instead (same answer): the barrier words may be mid-phase, so they are
    // zeroed again before the next launch, and the margin log starts over for the host levels
    auto fall_back = [&](const char *why) {
        c->small_zeroed = nullptr;
        const bool quiet = fbn::KnobSet("FBN_PC_SMALL_FAIL");  // (the test knob expects it)
        if (!quiet) fprintf(stderr, "fastbn: device-resident PC search %s; host-driven levels instead\n", why);
        *fellback = true;
        return CiResetMargin(c);
    };
    static const int per_cu = [] {  // (a property of the kernel: queried once, thread-safe)
        int v = 0;
        return fbn_pc_small_occupancy(&v) == hipSuccess ? v : 0;
    }();
    if (per_cu < 1) return fall_back("has no workgroup that fits a CU");
    const int grid = c->num_cu;  // one workgroup per CU: every workgroup resident (grid barrier)
    // scratch: [zeroed: barrier words | first-independent words] [statistics slots] [pair tables]
    const size_t acc_off = (kSmallZeroBytes + 255) & ~(size_t)255;
    const size_t pt_off = acc_off + (size_t)grid * 64;
    const size_t pg_off = (pt_off + (size_t)kSmallMaxEdges * 16 * 4 + 255) & ~(size_t)255;
    const size_t dout_off = (pg_off + (size_t)kSmallMaxEdges * 8 + 255) & ~(size_t)255;
    const size_t bytes = dout_off + sizeof(PcSmallOut);
    if ((rc = c->small_scr.ensure(bytes))) return rc;
    if (!c->h_small) {  // coherent: the host polls its completion word while the kernel runs
        hipError_t e = hipHostMalloc((void **)&c->h_small, sizeof(PcSmallOut), hipHostMallocCoherent);
        if (e != hipSuccess) return SetError(FBN_ERR_NOMEM, "hipHostMalloc: %s", hipGetErrorString(e));
        c->h_small->done = 0;
    }
    PcSmallOut *out = c->h_small;
    out->status = -1;
    char *scr = c->small_scr.as<char>();
    if (c->small_zeroed != c->small_scr.p || c->small_zeroed_bytes != c->small_scr.bytes) {
        FBN_HIP(hipMemsetAsync(scr, 0, kSmallZeroBytes, s));  // barrier counters and first[] words: once
        c->small_zeroed = c->small_scr.p;
        c->small_zeroed_bytes = c->small_scr.bytes;
        c->small_phase = 0;
    }
    if (++c->small_epoch == 0) ++c->small_epoch;  // (wrapped: skip 0 -- the zeroed words' epoch)
    PcSmallArgs a{};
    a.bits = c->bits.as<uint32_t>();
    a.row0 = c->brow.as<int32_t>();
    a.rowcnt = c->browcnt.as<int32_t>();
    a.nrows = c->row0_host.back() + std::min(c->dims[c->nvars - 1], 8);
    a.W = c->bits_W;
    a.pk = c->pack2.as<uint32_t>();
    a.PW = c->pack2_W;
    a.dims = c->ddims.as<int32_t>();
    a.nvars = c->nvars;
    a.N = c->N;
    a.alpha = alpha;
    a.band = band;
    a.nband = nband;
    a.depth = depth;
    a.spec_a = 8;
    a.bar = reinterpret_cast<unsigned *>(scr);
    a.first = reinterpret_cast<unsigned long long *>(scr + (size_t)kSmallBarWords * 4);
    a.epoch = c->small_epoch;
    a.phase_base = c->small_phase;
    a.acc = reinterpret_cast<unsigned long long *>(scr + acc_off);
    a.pairtab = reinterpret_cast<int32_t *>(scr + pt_off);
    // the level-1 information screen (exact, see ci_l1.hip; FBN_PC_NO_MISCREEN=1: off)
    a.pg2 = band && !fbn::KnobSet("FBN_PC_NO_MISCREEN") ? reinterpret_cast<unsigned long long *>(scr + pg_off) : nullptr;
    a.ctx_stats = c->stats.as<unsigned long long>();
    a.dout = reinterpret_cast<PcSmallOut *>(scr + dout_off);
    a.out = out;
    static const bool trace = fbn::KnobSet("FBN_PC_SMALL_TRACE");  // diagnostic
    std::vector<unsigned long long> trace_host;
    unsigned long long *h_trace = nullptr;
    DevBuf trace_dev;
    if (trace) {
        const size_t tb = (64 + 10 * 1024) * 8;
        if ((rc = trace_dev.ensure(tb))) return rc;
        FBN_HIP(hipMemsetAsync(trace_dev.p, 0, tb, s));
        a.trace = trace_dev.as<unsigned long long>();
        trace_host.assign(tb / 8, 0);
    }
    CiSlot &S = c->slot[0];
    const auto h1 = Clock::now();
    if (c->timing) FBN_HIP(hipEventRecord(S.ev0, s));
    // FBN_PC_SMALL_FAIL (test knob): "launch" = treat the launch as refused, "timeout" = a barrier
    // limit of one tick, so the first level's barrier times out in the kernel itself
    const char *force = fbn::KnobValue("FBN_PC_SMALL_FAIL");  // (read per call: tests set it)
    // launch: plain by default -- the grid (one workgroup per CU, occupancy checked above) is resident
    // unless other work holds CUs, and then a barrier times out (bounded spin) and the host driver
    // takes over; hipLaunchCooperativeKernel (FBN_PC_SMALL_COOP=1, read per call) refuses such a grid
    // up front but measured 12-15 us more kernel time per call (0.140 vs 0.126 ms on ALARM-5000)
    const char *coop_env = fbn::KnobValue("FBN_PC_SMALL_COOP");
    const bool plain = !(coop_env && atoi(coop_env) != 0);
    const bool force_launch = force && !strcmp(force, "launch");
    const long long spin = (force && !strcmp(force, "timeout")) ? 1 : 0;
    {
        const hipError_t le = force_launch ? hipErrorCooperativeLaunchTooLarge
                                           : fbn_pc_small_launch(&a, grid, spin, plain ? 0 : 1, s);
        if (le != hipSuccess) {
            (void)hipGetLastError();  // (clear the sticky launch error)
            return fall_back(hipGetErrorString(le));
        }
    }
    if (c->timing) FBN_HIP(hipEventRecord(S.ev1, s));
    const auto h2 = Clock::now();
    // wait for the kernel's completion word (written after the record) instead of a stream sync;
    // a stream sync only for the events / trace, or when the word does not come (fault, hang)
    {
        const auto t0 = std::chrono::steady_clock::now();
        bool got = false;
        for (unsigned spin = 0;; ++spin) {
            if (__atomic_load_n(&out->done, __ATOMIC_ACQUIRE) == c->small_epoch) {
                got = true;
                break;
            }
            if ((spin & 1023) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(5)) break;
        }
        if (!got || c->timing || trace) FBN_HIP(hipStreamSynchronize(s));
    }
    const auto h3 = Clock::now();
    if (trace) {
        FBN_HIP(hipMemcpy(trace_host.data(), trace_dev.p, trace_host.size() * 8, hipMemcpyDeviceToHost));
        h_trace = trace_host.data();
    }
    if (h_trace) {
        const unsigned long long t0 = h_trace[63];
        for (int d = 0; d < out->levels; ++d) {
            unsigned long long mx = 0, mn = ~0ull, smx = 0, smn = ~0ull;
            double dur = 0, dmax = 0;
            for (int b = 0; b < grid; ++b) {
                const unsigned long long v = h_trace[64 + d * 1024 + b], u = h_trace[64 + 5 * 1024 + d * 1024 + b];
                if (v) mx = std::max(mx, v), mn = std::min(mn, v);
                if (u) smx = std::max(smx, u), smn = std::min(smn, u);
                if (u && v) dur += (v - u) * 0.01, dmax = std::max(dmax, (v - u) * 0.01);
            }
            fprintf(stderr, "pc small level %d: workgroups start %.2f..%.2f us, done %.2f..%.2f us (test phase mean "
                    "%.2f max %.2f us), barrier passed %.2f us, applied %.2f us\n", d, (smn - t0) * 0.01,
                    (smx - t0) * 0.01, (mn - t0) * 0.01, (mx - t0) * 0.01, dur / grid, dmax,
                    (h_trace[8 * d + 2] - t0) * 0.01, (h_trace[8 * d + 3] - t0) * 0.01);
            const double nt = (double)std::max<unsigned long long>(1, h_trace[8 * d + 7]);
            fprintf(stderr, "    one-wave tests: %.0f, cycles per test: count %.0f, complete/margins %.0f, G2/decision %.0f\n",
                    nt, h_trace[8 * d + 4] / nt, h_trace[8 * d + 5] / nt, h_trace[8 * d + 6] / nt);
        }
    }
    if (out->status != 0) {
        // a grid barrier timed out (or no record): wait for the kernel's last workgroups, so none
        // writes into the next launch's record, then run the host levels
        FBN_HIP(hipStreamSynchronize(s));
        if (out->status != 1) return SetError(FBN_ERR_HIP, "pc small kernel: no result (status %d)", out->status);
        return fall_back("timed out at a grid barrier");
    }
    c->small_phase += (unsigned)out->levels;  // one grid barrier per completed level
    if (c->timing) {
        float ms = 0.f;
        FBN_HIP(hipEventElapsedTime(&ms, S.ev0, S.ev1));
        res.kernel_s += ms * 1e-3;
    }
    // the levels the device completed -> counts, sepsets, skeleton (edges in vec_edges order =
    // lexicographic pairs of each snapshot)
    const int n = c->nvars;
    const int L = out->levels;
    std::vector<uint64_t> prev(n);
    for (int v = 0; v < n; ++v) prev[v] = (n >= 64 ? ~0ull : ((1ull << n) - 1ull)) & ~(1ull << v);
    std::vector<std::pair<int, int>> ledges;
    std::vector<char> rm;
    std::vector<int> sep;
    for (int d = 0; d < L; ++d) {
        ledges.clear();
        rm.clear();
        for (int x = 0; x < n; ++x)
            for (int y = x + 1; y < n; ++y)
                if ((prev[x] >> y) & 1ull) {
                    ledges.push_back({x, y});
                    rm.push_back(((out->adj[d][x] >> y) & 1ull) ? 0 : 1);
                }
        if (d == 0) {
            res.sepset.set_level0(n, rm.data());  // level 0 = the complete graph
        } else {
            sep.assign(ledges.size() * (size_t)d, -1);
            const int32_t *pool = out->pool + out->sep_off[d];
            size_t r = 0;
            for (size_t e = 0; e < ledges.size(); ++e)
                if (rm[e]) {
                    for (int j = 0; j < d; ++j) sep[e * d + j] = pool[r * d + j];
                    ++r;
                }
            if ((int64_t)r * d != (int64_t)(out->sep_off[d + 1] - out->sep_off[d]))
                return SetError(FBN_ERR_HIP, "pc small kernel: level %d sepset count mismatch", d);
            res.sepset.append_level(ledges.data(), rm.data(), sep.data(), ledges.size(), d);
        }
        res.tests_per_level.push_back(out->counted[d]);
        res.launched_per_level.push_back(out->launched[d]);
        // bytes of the 2-bit packed columns / bit-sliced rows the tests touched: (d + 2) columns of
        // N / 4 bytes per launched test (roofline accounting)
        res.device_bytes += out->launched[d] * (int64_t)(d + 2) * ((c->N + 3) / 4);
        for (int v = 0; v < n; ++v) prev[v] = out->adj[d][v];
    }
    sk.Reset(n);
    for (int x = 0; x < n; ++x)
        for (int y = x + 1; y < n; ++y)
            if ((prev[x] >> y) & 1ull) sk.edges.push_back({x, y});
    sk.RebuildAdj(false);  // (x then y ascending = lexicographic: the lists come out sorted)
    *levels = L;
    *handoff = out->handoff != 0;
    if (!*handoff) {
        double m;
        memcpy(&m, &out->margin_bits, 8);
        res.min_margin = m;
        res.near_alpha = (int64_t)out->near;
        res.margin_done = true;
    }
    if (htime)
        fprintf(stderr, "pc small host: set-up %.1f us, launch %.1f us, wait %.1f us, record -> result %.1f us\n",
                Us(h0, h1), Us(h1, h2), Us(h2, h3), Us(h3, Clock::now()));
    return FBN_OK;
}
}  // namespace fbn
