// capi_gci.hip -- the device entries of the Gaussian conditional-independence test (include/fastbn.h,
// fbn_gci_*): a context that holds the float64 column store and its correlation matrix R (gci_corr.hip,
// computed at upload and again when the tuning changes), batches of tests on R (gci_test.hip) in two slots
// with pinned staging, and the PC-stable run through gci_pc.cpp's driver.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "fbn_device.h"
#include "gci.h"
#include "gci_ctx.h"
#include "launchers.h"

using fbn::SetError;

namespace fbn {

namespace {

constexpr int kGciMaxVars = 32768;  // R is nvars^2 doubles; tile and pair indices stay far inside 32 bits

// R from the resident column store with the context's tuning; refuses a non-finite value and a zero variance
int GciCompute(fbn_gci_ctx *c) {
    const int n = c->nvars;
    // what fbn_gci_set_tuning left automatic: the switch table's seams (knobs.h), then the defaults
    const int64_t env_tile = KnobOr("FBN_CI_GCI_TILE", 0), env_split = KnobOr("FBN_CI_GCI_SPLITK", 0);
    const int tile = c->want_tile ? c->want_tile : (env_tile == 32 || env_tile == 64) ? (int)env_tile : (n >= 2048 ? 64 : 32);
    const int T = (n + tile - 1) / tile, nt = T * (T + 1) / 2;
    const int64_t nstages = (c->N + fbn_gci_stage() - 1) / fbn_gci_stage();
    // automatic: about sixteen blocks per CU (four resident at tile 32, their global loads hidden behind one
    // another's MFMAs: the fastest measured at 1,000 x 100,000), at most 64 slices, every slice at
    // least one stage
    int S = c->want_split                          ? c->want_split
            : env_split >= 1 && env_split <= 4096 ? (int)env_split
                                                  : (int)std::min<int64_t>(64, (16 * c->num_cu + nt - 1) / nt);
    S = (int)std::max<int64_t>(1, std::min<int64_t>(S, nstages));
    if (int rc = c->slab.ensure((size_t)S * nt * tile * tile * 8)) return rc;
    const GciCorrArgs a{c->X.as<double>(), c->mean.as<double>(), c->bad.as<int>(), c->slab.as<double>(), c->R.as<double>(),
                        c->var.as<double>(), n, (long long)c->N, tile, S};
    hipStream_t s = c->stream;
    FBN_HIP(hipEventRecord(c->cev[0], s));
    FBN_HIP(fbn_gci_means_launch(a.X, n, a.N, a.mean, a.bad, s));
    FBN_HIP(hipEventRecord(c->cev[1], s));
    FBN_HIP(fbn_gci_gram_launch(&a, s));
    FBN_HIP(hipEventRecord(c->cev[2], s));
    FBN_HIP(fbn_gci_reduce_launch(&a, s));
    FBN_HIP(hipEventRecord(c->cev[3], s));
    std::vector<int> bad((size_t)n);
    std::vector<double> var((size_t)n);
    FBN_HIP(hipMemcpyAsync(bad.data(), c->bad.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    FBN_HIP(hipMemcpyAsync(var.data(), c->var.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    FBN_HIP(hipStreamSynchronize(s));
    for (int k = 0; k < 3; ++k) FBN_HIP(hipEventElapsedTime(&c->corr_ms[k], c->cev[k], c->cev[k + 1]));
    c->last_ms = c->corr_ms[0] + c->corr_ms[1] + c->corr_ms[2];
    c->timed = true;
    c->split_k = S, c->tile = tile;
    for (int v = 0; v < n; ++v)
        if (bad[(size_t)v]) return SetError(FBN_ERR_ARG, "column store: variable %d holds a value that is not finite", v);
    for (int v = 0; v < n; ++v)
        if (!(var[(size_t)v] > 0.0)) return SetError(FBN_ERR_ARG, "column store: variable %d has zero variance", v);
    c->h_ss = std::move(var);  // the family scorer's tables are formed from it (capi_gscore.hip)
    return FBN_OK;
}

int GciCreate(const double *cols, bool on_device, int nvars, int64_t nsamples, int device, fbn_gci_ctx **out) {
    if (!cols || !out || nvars <= 0 || nsamples <= 0) return SetError(FBN_ERR_ARG, "bad argument");
    if (nvars > kGciMaxVars) return SetError(FBN_ERR_LIMIT, "%d variables (supported up to %d)", nvars, kGciMaxVars);
    if (nsamples < 2) return SetError(FBN_ERR_LIMIT, "%lld samples: a correlation needs at least 2", (long long)nsamples);
    auto c = std::unique_ptr<fbn_gci_ctx>(new (std::nothrow) fbn_gci_ctx());
    if (!c) return SetError(FBN_ERR_NOMEM, "out of memory");
    int rc = CheckDevice(device, &c->num_cu);
    if (rc) return rc;
    c->device = device, c->nvars = nvars, c->N = nsamples;
    const size_t n = (size_t)nvars;
    if ((rc = c->X.ensure(n * (size_t)nsamples * 8)) || (rc = c->mean.ensure(n * 8)) || (rc = c->bad.ensure(n * 4)) ||
        (rc = c->var.ensure(n * 8)) || (rc = c->R.ensure(n * n * 8)) || (rc = c->stats.ensure(24)))
        return rc;
    FBN_HIP(hipMemcpy(c->X.p, cols, n * (size_t)nsamples * 8, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    FBN_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    for (auto &e : c->cev) FBN_HIP(hipEventCreate(&e));
    for (auto &sl : c->slot) {
        FBN_HIP(hipEventCreate(&sl.ev0));
        FBN_HIP(hipEventCreate(&sl.ev1));
        FBN_HIP(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    }
    hipError_t e = hipHostMalloc((void **)&c->h_stats, 48, hipHostMallocDefault);
    if (e != hipSuccess) return SetError(FBN_ERR_NOMEM, "hipHostMalloc: %s", hipGetErrorString(e));
    c->h_stats[0] = 0x7FF0000000000000ull;  // +inf
    c->h_stats[1] = c->h_stats[2] = 0;
    if ((rc = GciCompute(c.get()))) return rc;
    *out = c.release();
    return FBN_OK;
}

int StatsReset(fbn_gci_ctx *c) {
    FBN_HIP(hipMemcpyAsync(c->stats.p, c->h_stats, 24, hipMemcpyHostToDevice, c->stream));
    return FBN_OK;
}
int StatsRead(fbn_gci_ctx *c, GciLog *log) {
    FBN_HIP(hipMemcpyAsync(c->h_stats + 3, c->stats.p, 24, hipMemcpyDeviceToHost, c->stream));
    FBN_HIP(hipStreamSynchronize(c->stream));
    memcpy(&log->min_margin, &c->h_stats[3], 8);
    log->near = (int64_t)c->h_stats[4];
    log->degenerate = (int64_t)c->h_stats[5];
    return FBN_OK;
}

// a batch into slot k on the ctx stream: items staged through pinned memory, decisions (and r) back to it
int GciLaunch(fbn_gci_ctx *c, int k, const int32_t *items, int64_t n, int d, double tau, bool want_r) {
    auto &S = c->slot[k];
    S.n = n, S.want_r = want_r;
    if (n == 0) return FBN_OK;
    const size_t ib = items ? (size_t)n * (2 + d) * 4 : 0, rb = (size_t)n * 8 + (((size_t)n + 7) & ~(size_t)7);
    int rc;
    if ((rc = PinnedEnsure(S.h_res, S.h_res_bytes, rb)) || (rc = S.indep.ensure((size_t)n))) return rc;
    if (want_r && (rc = S.r.ensure((size_t)n * 8))) return rc;
    hipStream_t s = c->stream;
    if (items) {
        if ((rc = PinnedEnsure(S.h_items, S.h_items_bytes, ib)) || (rc = S.items.ensure(ib))) return rc;
        memcpy(S.h_items, items, ib);
        FBN_HIP(hipMemcpyAsync(S.items.p, S.h_items, ib, hipMemcpyHostToDevice, s));
    }
    const GciTestArgs a{c->R.as<double>(), c->nvars, items ? S.items.as<int32_t>() : nullptr, (long long)n, tau,
                        want_r ? S.r.as<double>() : nullptr, S.indep.as<uint8_t>(), c->stats.as<unsigned long long>()};
    FBN_HIP(hipEventRecord(S.ev0, s));
    FBN_HIP(fbn_gci_test_launch(&a, d, s));
    FBN_HIP(hipEventRecord(S.ev1, s));
    // pinned result: r [n] first (8-byte aligned), then the decisions
    if (want_r) FBN_HIP(hipMemcpyAsync(S.h_res, S.r.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    FBN_HIP(hipMemcpyAsync(static_cast<char *>(S.h_res) + (size_t)n * 8, S.indep.p, (size_t)n, hipMemcpyDeviceToHost, s));
    FBN_HIP(hipEventRecord(S.done, s));
    return FBN_OK;
}

// (the slots share the ctx stream; each waits for its own batch's event)
int GciWait(fbn_gci_ctx *c, int k, double *r, uint8_t *indep, float *ms) {
    auto &S = c->slot[k];
    const int64_t n = S.n;
    if (n == 0) return FBN_OK;
    FBN_HIP(hipEventSynchronize(S.done));
    if (r && S.want_r) memcpy(r, S.h_res, (size_t)n * 8);
    if (indep) memcpy(indep, static_cast<char *>(S.h_res) + (size_t)n * 8, (size_t)n);
    FBN_HIP(hipEventElapsedTime(ms, S.ev0, S.ev1));
    S.n = 0;
    return FBN_OK;
}

struct DeviceTester : GciTester {
    fbn_gci_ctx *c;
    float total_ms = 0.f;
    explicit DeviceTester(fbn_gci_ctx *ctx) : c(ctx) {}
    int Launch(int k, const int32_t *items, int64_t n, int d, double tau) override {
        return GciLaunch(c, k, items, n, d, tau, false);
    }
    int Wait(int k, uint8_t *indep, PCResultHost &res) override {
        float ms = 0.f;
        if (int rc = GciWait(c, k, nullptr, indep, &ms)) return rc;
        res.kernel_s += ms * 1e-3;
        total_ms += ms;
        return FBN_OK;
    }
    int Log(GciLog *log) override { return StatsRead(c, log); }
};

}  // namespace

int GciMoments(fbn_gci_ctx *c, int *nvars, int64_t *N, std::vector<double> &mean, std::vector<double> &ss,
               std::vector<double> &R) {
    if (!c) return SetError(FBN_ERR_ARG, "null pointer");
    const size_t n = (size_t)c->nvars;
    mean.resize(n), ss.resize(n), R.resize(n * n);
    FBN_HIP(hipSetDevice(c->device));
    FBN_HIP(hipStreamSynchronize(c->stream));
    FBN_HIP(hipMemcpy(mean.data(), c->mean.p, n * 8, hipMemcpyDeviceToHost));
    FBN_HIP(hipMemcpy(ss.data(), c->var.p, n * 8, hipMemcpyDeviceToHost));
    FBN_HIP(hipMemcpy(R.data(), c->R.p, n * n * 8, hipMemcpyDeviceToHost));
    *nvars = c->nvars, *N = c->N;
    return FBN_OK;
}

}  // namespace fbn

extern "C" {

int fbn_gci_upload(const double *cols, int nvars, int64_t nsamples, int device, fbn_gci_ctx **out) {
    // a constant column (the only way S_vv comes out 0) is refused before anything is uploaded: the scan of a
    // column ends at its first value that differs from the column's first
    if (cols && nvars > 0 && nsamples > 0)
        for (int v = 0; v < nvars; ++v) {
            const double *x = cols + (size_t)v * (size_t)nsamples;
            int64_t i = 1;
            while (i < nsamples && x[i] == x[0]) ++i;
            if (i == nsamples) return SetError(FBN_ERR_ARG, "column store: variable %d has zero variance", v);
        }
    return fbn::GciCreate(cols, false, nvars, nsamples, device, out);
}
int fbn_gci_from_device(const double *d_cols, int nvars, int64_t nsamples, int device, fbn_gci_ctx **out) {
    return fbn::GciCreate(d_cols, true, nvars, nsamples, device, out);
}

int fbn_gci_corr(fbn_gci_ctx *c, double *R) {
    if (!c || !R) return SetError(FBN_ERR_ARG, "null pointer");
    FBN_HIP(hipSetDevice(c->device));
    FBN_HIP(hipStreamSynchronize(c->stream));
    FBN_HIP(hipMemcpy(R, c->R.p, (size_t)c->nvars * c->nvars * 8, hipMemcpyDeviceToHost));
    return FBN_OK;
}

int fbn_gci_set_tuning(fbn_gci_ctx *c, int32_t split_k, int32_t tile) {
    if (!c) return SetError(FBN_ERR_ARG, "null pointer");
    if (split_k < 0 || split_k > 4096) return SetError(FBN_ERR_ARG, "split_k = %d out of 0..4096", split_k);
    if (tile != 0 && tile != 32 && tile != 64) return SetError(FBN_ERR_ARG, "tile = %d: 0 (automatic), 32 or 64", tile);
    FBN_HIP(hipSetDevice(c->device));
    c->want_split = split_k, c->want_tile = tile;
    return fbn::GciCompute(c);
}

int fbn_gci_info(const fbn_gci_ctx *c, int64_t out[4]) {
    if (!c || !out) return SetError(FBN_ERR_ARG, "null pointer");
    out[0] = c->tile, out[1] = c->split_k, out[2] = (int64_t)c->slab.bytes, out[3] = c->last_degenerate;
    return FBN_OK;
}

int fbn_gci_corr_kernel_ms(const fbn_gci_ctx *c, float ms[3]) {
    if (!c || !ms) return SetError(FBN_ERR_ARG, "null pointer");
    std::copy(c->corr_ms, c->corr_ms + 3, ms);
    return FBN_OK;
}

int fbn_gci_last_kernel_ms(const fbn_gci_ctx *c, float *ms) {
    if (!c || !ms || !c->timed) return SetError(FBN_ERR_ARG, "no timed launch");
    *ms = c->last_ms;
    return FBN_OK;
}

int fbn_gci_run(fbn_gci_ctx *c, const int32_t *items, int64_t n, int d, double alpha, double *r, double *z, double *p,
                uint8_t *indep, int64_t *degenerate) {
    if (!c || n < 0 || (n > 0 && !items)) return SetError(FBN_ERR_ARG, "bad argument");
    double tau = 0.0;
    if (int rc = fbn::GciTau(alpha, c->N, d, &tau)) return rc;
    if (int rc = fbn::GciCheckItems(items, n, d, c->nvars)) return rc;
    FBN_HIP(hipSetDevice(c->device));
    std::vector<double> rv((size_t)n);
    int rc;
    if ((rc = fbn::StatsReset(c)) || (rc = fbn::GciLaunch(c, 0, items, n, d, tau, true))) return rc;
    float ms = 0.f;
    if ((rc = fbn::GciWait(c, 0, rv.data(), indep, &ms))) return rc;
    fbn::GciLog log;
    if ((rc = fbn::StatsRead(c, &log))) return rc;
    for (int64_t t = 0; t < n; ++t) {
        double zt, pt;
        fbn::GciReport(rv[(size_t)t], c->N, d, &zt, &pt);
        if (r) r[t] = rv[(size_t)t];
        if (z) z[t] = zt;
        if (p) p[t] = pt;
    }
    c->last_ms = ms, c->timed = true;
    c->last_degenerate = log.degenerate;
    if (degenerate) *degenerate = log.degenerate;
    return FBN_OK;
}

int fbn_gci_pc_stable(fbn_gci_ctx *c, double alpha, int depth, fbn_pc_result **out) {
    if (!c || !out) return SetError(FBN_ERR_ARG, "null pointer");
    auto res = std::unique_ptr<fbn_pc_result>(new (std::nothrow) fbn_pc_result());
    if (!res) return SetError(FBN_ERR_NOMEM, "out of memory");
    FBN_HIP(hipSetDevice(c->device));
    if (int rc = fbn::StatsReset(c)) return rc;
    fbn::DeviceTester T(c);
    const int rc = fbn::RunPCGauss(T, c->nvars, c->N, alpha, depth, res->r);
    (void)hipStreamSynchronize(c->stream);  // (an early return leaves no batch in flight on the pinned buffers)
    for (auto &s : c->slot) s.n = 0;
    if (rc) return rc;
    c->last_ms = T.total_ms, c->timed = true;
    c->last_degenerate = res->r.degenerate;
    *out = res.release();
    return FBN_OK;
}

int fbn_gci_ctx_destroy(fbn_gci_ctx *c) {
    if (!c) return FBN_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    delete c;
    return FBN_OK;
}

}  // extern "C"
