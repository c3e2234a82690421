// capi_ais.hip -- the fbn_ais_* section of include/fastbn.h: handles of the adaptive samplers AIS-BN
// and SIS over the host twin (ais_host.cpp) and the one launch of a device run (sample_ais_kernel,
// ais.hip).  Replaces the reference's AIS-BN and SIS stubs (src/main.cpp:175-186, :149-160).
#include <hip/hip_runtime.h>

#include <map>
#include <utility>
#include <vector>

#include "ais_model.h"
#include "capi_sampler.h"
#include "launchers.h"

using fbn::DevBuf;
using fbn::SetError;

struct fbn_ais : fbn::SamplerHandle {
    int64_t lds_bytes_max = FBN_AIS_LDS_DEFAULT;
    int max_workgroups = 0;
    DevBuf ws, di;                              // the state's global home; staging of the debug ICPT
    std::map<std::pair<int, int>, DevBuf> eta;  // (method, m) -> its table, written once
    // values [V][64], 64 weights, V flags (padded to 8); with the state in LDS also I and N
    int64_t base_bytes() const { return (int64_t)M.V * 64 + 512 + ((int64_t)M.V + 7) / 8 * 8; }
    int64_t lds_bytes() const { return base_bytes() + 16 * M.cells; }
    bool lds_state() const { return lds_bytes_max >= 0 && lds_bytes() <= lds_bytes_max; }
    int64_t grid(int64_t ncases) const {
        int per_cu = FBN_AIS_GROUPS_PER_CU;
        const int64_t b = lds_state() ? lds_bytes() : base_bytes();
        per_cu = (int)std::max<int64_t>(1, std::min<int64_t>(per_cu, fbn::kCuLdsBytes / b));
        int64_t g = std::min<int64_t>(std::max<int64_t>(ncases, 1), (int64_t)std::max(num_cu, 1) * per_cu);
        if (max_workgroups > 0) g = std::min<int64_t>(g, max_workgroups);
        return g;
    }
};

namespace {

struct RunArgs {
    int method;
    int64_t ncases, S, m, l, case_offset;
    uint64_t seed;
    double eps;
};

int AisDevice(fbn_ais *s, const RunArgs &r, const int8_t *d_ev, int32_t *d_labels, double *d_marg, double *d_stats,
              uint8_t *dv, double *dm, int32_t *de, double *di, hipStream_t st) {
    int rc;
    if ((rc = s->OpenRun(d_ev, r.ncases, &d_marg, st))) return rc;
    const bool lds = s->lds_state();
    const int64_t grid = s->grid(r.ncases);
    if (!lds)
        if ((rc = s->ws.ensure((size_t)grid * 2 * (size_t)s->M.cells * 8))) return rc;
    DevBuf &eta = s->eta[{r.method, (int)r.m}];
    if (!eta.p) {  // a new buffer no launch reads yet
        std::vector<double> h((size_t)std::max<int64_t>(r.m, 1), 1.0);
        fbn::AisEta(r.method, (int)r.m, h.data());
        if ((rc = fbn::Upload(eta, h))) return rc;
    }
    fbn::PcgStream R;
    fbn::AisDeviceArgs a;
    a.sch = fbn::AisStages(r.method, r.S, r.m, r.l);
    s->FillArgs(a, R, r.seed, d_ev, r.ncases, r.S, r.case_offset, d_labels, d_marg, d_stats, dv, dm, de);
    fbn::PcgJump(R, (uint64_t)(r.l - 64 * ((r.l - 1) / 64) - 1) * (uint64_t)s->M.V, &a.sm, &a.sc);
    a.cells = s->M.cells, a.method = r.method, a.eps = r.eps;
    a.eta = eta.as<double>(), a.ws = lds ? nullptr : s->ws.as<double>(), a.di = di;
    return s->Timed(st, [&] {
        return fbn_ais_launch(&a, lds ? 1 : 0, (size_t)(lds ? s->lds_bytes() : s->base_bytes()), (int)grid, st);
    });
}

int AisHostBuffers(fbn_ais *s, const RunArgs &r, const int8_t *evidence, int32_t *labels, double *marginals,
                   double *stats, uint8_t *values, double *mant, int32_t *expo, double *icpt) {
    if (int rc = fbn::CheckAisArgs(s->M, r.method, r.ncases, r.S, r.m, r.l, r.case_offset, r.eps)) return rc;
    if (r.ncases == 0) return FBN_OK;
    if (s->device < 0) {
        if (int rc = fbn::CheckEvidenceHost(s->M, evidence, r.ncases)) return rc;
        return fbn::HostAis(s->M, r.method, evidence, r.ncases, r.S, r.m, r.l, r.seed, r.case_offset, r.eps, labels,
                            marginals, stats, values, mant, expo, icpt);
    }
    return s->HostBuffers(evidence, r.ncases, 4, fbn::AisStages(r.method, r.S, r.m, r.l).T, labels, marginals, stats,
                          values, mant, expo, &s->di, (size_t)r.ncases * (size_t)s->M.cells * 8, icpt,
                          [&](const int8_t *d_ev, int32_t *d_labels, double *d_marg, double *d_stats, uint8_t *dv,
                              double *dm, int32_t *de) {
                              return AisDevice(s, r, d_ev, d_labels, d_marg, d_stats, dv, dm, de,
                                               dv ? s->di.as<double>() : nullptr, nullptr);
                          });
}

}  // namespace

extern "C" {

int fbn_ais_create(const fbn_network *net, int device, fbn_ais **out) {
    return fbn::CreateHandle(net, out, [&](fbn_ais *s) { return s->Create(net->net, device, true); });
}

int fbn_ais_destroy(fbn_ais *s) { return fbn::DestroyHandle(s); }

int fbn_ais_info(const fbn_ais *s, int64_t ncases, int64_t *lds_bytes, int64_t *state_bytes, int *path, int *grid) {
    if (!s) return SetError(FBN_ERR_ARG, "null pointer");
    if (lds_bytes) *lds_bytes = s->lds_bytes();
    if (state_bytes) *state_bytes = 16 * s->M.cells;
    if (path) *path = s->lds_state() ? 0 : 1;
    if (grid) *grid = (int)s->grid(ncases);
    return FBN_OK;
}

int fbn_ais_eta(int method, int m, double *eta) {
    if ((method != 0 && method != 1) || m < 0 || m > FBN_AIS_MAX_UPDATES || (m > 0 && !eta))
        return SetError(FBN_ERR_ARG, "bad argument");
    fbn::AisEta(method, m, eta);
    return FBN_OK;
}

int fbn_ais_run(fbn_ais *s, int method, const int8_t *evidence, int64_t ncases, int64_t S, int64_t m, int64_t l,
                uint64_t seed, int64_t case_offset, double eps, int32_t *labels, double *marginals, double *stats) {
    if (!s || (ncases > 0 && (!evidence || !labels))) return SetError(FBN_ERR_ARG, "bad argument");
    return AisHostBuffers(s, RunArgs{method, ncases, S, m, l, case_offset, seed, eps}, evidence, labels, marginals, stats,
                          nullptr, nullptr, nullptr, nullptr);
}

int fbn_ais_run_device(fbn_ais *s, int method, const int8_t *d_evidence, int64_t ncases, int64_t S, int64_t m, int64_t l,
                       uint64_t seed, int64_t case_offset, double eps, int32_t *d_labels, double *d_marginals,
                       double *d_stats, void *hip_stream) {
    if (!s || (ncases > 0 && (!d_evidence || !d_labels))) return SetError(FBN_ERR_ARG, "bad argument");
    if (int rc = fbn::CheckAisArgs(s->M, method, ncases, S, m, l, case_offset, eps)) return rc;
    if (s->device < 0) return SetError(FBN_ERR_NODEV, "host-only handle (created with device < 0)");
    if (ncases == 0) return FBN_OK;
    FBN_HIP(hipSetDevice(s->device));
    return AisDevice(s, RunArgs{method, ncases, S, m, l, case_offset, seed, eps}, d_evidence, d_labels, d_marginals,
                     d_stats, nullptr, nullptr, nullptr, nullptr, static_cast<hipStream_t>(hip_stream));
}

int fbn_ais_debug_samples(fbn_ais *s, int method, const int8_t *evidence, int64_t ncases, int64_t S, int64_t m,
                          int64_t l, uint64_t seed, int64_t case_offset, double eps, uint8_t *values, double *mantissas,
                          int32_t *exponents, double *icpt) {
    if (!s || (ncases > 0 && (!evidence || !values || !mantissas || !exponents || !icpt)))
        return SetError(FBN_ERR_ARG, "bad argument");
    if (int rc = fbn::CheckAisArgs(s->M, method, ncases, S, m, l, case_offset, eps)) return rc;
    const int64_t T = fbn::AisStages(method, S, m, l).T;
    if (ncases > 0 && (ncases > FBN_SAMPLE_DEBUG_MAX || T > FBN_SAMPLE_DEBUG_MAX / ncases ||
                       s->M.cells > FBN_SAMPLE_DEBUG_MAX / ncases))
        return SetError(FBN_ERR_LIMIT, "debug samples: more than %lld samples or ICPT cells", (long long)FBN_SAMPLE_DEBUG_MAX);
    std::vector<int32_t> labels((size_t)std::max<int64_t>(ncases, 1));
    return AisHostBuffers(s, RunArgs{method, ncases, S, m, l, case_offset, seed, eps}, evidence, labels.data(), nullptr,
                          nullptr, values, mantissas, exponents, icpt);
}

int fbn_ais_set_tuning(fbn_ais *s, int64_t lds_bytes_max, int max_workgroups) {
    if (!s || max_workgroups < 0) return SetError(FBN_ERR_ARG, "bad argument");
    if (lds_bytes_max > FBN_AIS_LDS_DEFAULT)
        return SetError(FBN_ERR_ARG, "lds_bytes_max %lld beyond %lld", (long long)lds_bytes_max,
                        (long long)FBN_AIS_LDS_DEFAULT);
    s->lds_bytes_max = lds_bytes_max == 0 ? FBN_AIS_LDS_DEFAULT : lds_bytes_max;
    s->max_workgroups = max_workgroups;
    return FBN_OK;
}

int fbn_ais_last_kernel_ms(const fbn_ais *s, float *ms) {
    if (!s) return SetError(FBN_ERR_ARG, "no timed launch");
    return s->LastKernelMs(ms);
}

}  // extern "C"
