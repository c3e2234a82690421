// capi_epis.hip -- the fbn_epis_* section of include/fastbn.h: EPIS-BN handles over the host twin
// (epis_host.cpp) and the two launches of a device run, the LBP kernel writing the lambda rows
// (lbp.hip through the handle's own fbn_lbp) and sample_epis_kernel reading them (epis.hip), queued on
// one stream.  Replaces the reference's EPIS-BN stub (src/main.cpp:123-134).
#include <hip/hip_runtime.h>

#include <vector>

#include "capi_sampler.h"
#include "epis_model.h"
#include "launchers.h"

using fbn::DevBuf;
using fbn::SetError;

struct fbn_epis : fbn::SamplerHandle {
    fbn_lbp *lbp = nullptr;  // the pre-propagation: its model and, on a device, its uploaded tables
    int64_t lds_bytes_max = FBN_EPIS_LDS_DEFAULT;
    DevBuf lam, lbp_stats, lbp_labels;  // between the two launches
    bool lbp_ran = false;
    ~fbn_epis() { (void)fbn_lbp_destroy(lbp); }
    int64_t lds_bytes() const { return (int64_t)M.V * 64 + (int64_t)M.sum_dom * 8; }
    bool lds_lambda() const { return lds_bytes_max >= 0 && lds_bytes() <= lds_bytes_max; }
};

namespace {

struct RunArgs {
    int64_t ncases, S, case_offset;
    uint64_t seed;
    int iters;
    double tol, damping, eps;
};

int EpisDevice(fbn_epis *s, const RunArgs &r, const int8_t *d_ev, int32_t *d_labels, double *d_marg, double *d_stats,
               uint8_t *dv, double *dm, int32_t *de, hipStream_t st) {
    const int64_t nlam = r.ncases * s->M.sum_dom;
    if (nlam / 256 >= 0x7fffffffll) return SetError(FBN_ERR_LIMIT, "%lld cases in one call", (long long)r.ncases);
    int rc;
    if ((rc = s->OpenRun(d_ev, r.ncases, &d_marg, st)) || (rc = s->lam.ensure((size_t)nlam * 8)) ||
        (rc = s->lbp_stats.ensure((size_t)r.ncases * 16)) || (rc = s->lbp_labels.ensure((size_t)r.ncases * 4)))
        return rc;
    if (r.iters > 0) {
        if ((rc = fbn::LbpLambdaDevice(s->lbp, d_ev, r.ncases, r.iters, r.tol, r.damping, s->lbp_labels.as<int32_t>(),
                                       s->lbp_stats.as<double>(), s->lam.as<double>(), st)))
            return rc;
    } else {
        FBN_HIP(fbn_epis_fill(s->lam.as<double>(), nlam, 1.0, st));
    }
    s->lbp_ran = r.iters > 0;
    fbn::PcgStream R;
    fbn::EpisDeviceArgs a;
    s->FillArgs(a, R, r.seed, d_ev, r.ncases, r.S, r.case_offset, d_labels, d_marg, d_stats, dv, dm, de);
    a.eps = r.eps;
    a.lam = s->lam.as<double>(), a.lbp_stats = r.iters > 0 ? s->lbp_stats.as<double>() : nullptr;
    return s->Timed(st, [&] { return fbn_epis_launch(&a, s->lds_lambda() ? 1 : 0, st); });
}

int EpisHostBuffers(fbn_epis *s, const RunArgs &r, const int8_t *evidence, int32_t *labels, double *marginals,
                    double *stats, uint8_t *values, double *mant, int32_t *expo, double *lambda) {
    if (int rc = fbn::CheckEpisArgs(s->M, r.ncases, r.S, r.case_offset, r.iters, r.tol, r.damping, r.eps)) return rc;
    if (r.ncases == 0) return FBN_OK;
    if (s->device < 0) {
        if (int rc = fbn::CheckEvidenceHost(s->M, evidence, r.ncases)) return rc;
        return fbn::HostEpis(s->M, fbn::LbpModelOf(s->lbp), evidence, r.ncases, r.S, r.seed, r.case_offset, r.iters, r.tol,
                             r.damping, r.eps, labels, marginals, stats, values, mant, expo, lambda);
    }
    return s->HostBuffers(evidence, r.ncases, 4, r.S, labels, marginals, stats, values, mant, expo, &s->lam,
                          (size_t)r.ncases * s->M.sum_dom * 8, lambda,
                          [&](const int8_t *d_ev, int32_t *d_labels, double *d_marg, double *d_stats, uint8_t *dv,
                              double *dm, int32_t *de) {
                              return EpisDevice(s, r, d_ev, d_labels, d_marg, d_stats, dv, dm, de, nullptr);
                          });
}

}  // namespace

extern "C" {

int fbn_epis_create(const fbn_network *net, int device, fbn_epis **out) {
    return fbn::CreateHandle(net, out, [&](fbn_epis *s) {
        int rc = fbn::BuildSamplerModel(net->net, s->M);
        if (rc == FBN_OK) rc = fbn_lbp_create(net, device, &s->lbp);
        return rc ? rc : s->AttachTables(device, false);
    });
}

int fbn_epis_destroy(fbn_epis *s) { return fbn::DestroyHandle(s); }

int fbn_epis_info(const fbn_epis *s, int64_t *lds_bytes, int *path) {
    if (!s) return SetError(FBN_ERR_ARG, "null pointer");
    if (lds_bytes) *lds_bytes = s->lds_bytes();
    if (path) *path = s->lds_lambda() ? 0 : 1;
    return FBN_OK;
}

int fbn_epis_run(fbn_epis *s, const int8_t *evidence, int64_t ncases, int64_t S, uint64_t seed, int64_t case_offset,
                 int iters, double tol, double damping, double eps, int32_t *labels, double *marginals, double *stats) {
    if (!s || (ncases > 0 && (!evidence || !labels))) return SetError(FBN_ERR_ARG, "bad argument");
    return EpisHostBuffers(s, RunArgs{ncases, S, case_offset, seed, iters, tol, damping, eps}, evidence, labels, marginals,
                           stats, nullptr, nullptr, nullptr, nullptr);
}

int fbn_epis_run_device(fbn_epis *s, const int8_t *d_evidence, int64_t ncases, int64_t S, uint64_t seed,
                        int64_t case_offset, int iters, double tol, double damping, double eps, int32_t *d_labels,
                        double *d_marginals, double *d_stats, void *hip_stream) {
    if (!s || (ncases > 0 && (!d_evidence || !d_labels))) return SetError(FBN_ERR_ARG, "bad argument");
    if (int rc = fbn::CheckEpisArgs(s->M, ncases, S, case_offset, iters, tol, damping, eps)) return rc;
    if (s->device < 0) return SetError(FBN_ERR_NODEV, "host-only handle (created with device < 0)");
    if (ncases == 0) return FBN_OK;
    FBN_HIP(hipSetDevice(s->device));
    return EpisDevice(s, RunArgs{ncases, S, case_offset, seed, iters, tol, damping, eps}, d_evidence, d_labels, d_marginals,
                      d_stats, nullptr, nullptr, nullptr, static_cast<hipStream_t>(hip_stream));
}

int fbn_epis_debug_samples(fbn_epis *s, const int8_t *evidence, int64_t ncases, int64_t S, uint64_t seed,
                           int64_t case_offset, int iters, double tol, double damping, double eps, uint8_t *values,
                           double *mantissas, int32_t *exponents, double *lambda) {
    if (!s || (ncases > 0 && (!evidence || !values || !mantissas || !exponents || !lambda)))
        return SetError(FBN_ERR_ARG, "bad argument");
    if (ncases > 0 && S > 0 && (ncases > FBN_SAMPLE_DEBUG_MAX || S > FBN_SAMPLE_DEBUG_MAX / ncases))
        return SetError(FBN_ERR_LIMIT, "debug samples: more than %lld samples", (long long)FBN_SAMPLE_DEBUG_MAX);
    std::vector<int32_t> labels((size_t)std::max<int64_t>(ncases, 1));
    return EpisHostBuffers(s, RunArgs{ncases, S, case_offset, seed, iters, tol, damping, eps}, evidence, labels.data(),
                           nullptr, nullptr, values, mantissas, exponents, lambda);
}

int fbn_epis_set_tuning(fbn_epis *s, int64_t lds_bytes_max) {
    if (!s) return SetError(FBN_ERR_ARG, "null pointer");
    if (lds_bytes_max > FBN_EPIS_LDS_DEFAULT)
        return SetError(FBN_ERR_ARG, "lds_bytes_max %lld beyond %lld", (long long)lds_bytes_max,
                        (long long)FBN_EPIS_LDS_DEFAULT);
    s->lds_bytes_max = lds_bytes_max == 0 ? FBN_EPIS_LDS_DEFAULT : lds_bytes_max;
    return FBN_OK;
}

int fbn_epis_last_kernel_ms(const fbn_epis *s, float *lbp_ms, float *sample_ms) {
    if (!s || !lbp_ms || !sample_ms || !s->timed) return SetError(FBN_ERR_ARG, "no timed launch");
    *lbp_ms = 0.f;
    if (s->lbp_ran)
        if (int rc = fbn_lbp_last_kernel_ms(s->lbp, lbp_ms)) return rc;
    return s->LastKernelMs(sample_ms);
}

}  // extern "C"
