// capi_epis.hip -- the fbn_epis_* section of include/fastbn.h: EPIS-BN handles over the host twin
// (epis_host.cpp) and the two launches of a device run, the LBP kernel writing the lambda rows
// (lbp.hip through the handle's own fbn_lbp) and sample_epis_kernel reading them (epis.hip), queued on
// one stream.  Replaces the reference's EPIS-BN stub (src/main.cpp:123-134).
#include <hip/hip_runtime.h>

#include <cstring>
#include <set>
#include <vector>

#include "epis_model.h"
#include "fbn_device.h"
#include "fbn_internal.h"
#include "launchers.h"
#include "sample_device.h"

using fbn::DevBuf;
using fbn::SetError;

struct fbn_epis {
    fbn::SamplerModel M;
    fbn_lbp *lbp = nullptr;  // the pre-propagation: its model and, on a device, its uploaded tables
    int device = -1;
    int64_t lds_bytes_max = FBN_EPIS_LDS_DEFAULT;
    DevBuf nodes, par, prob, ent, dom, evcheck;
    DevBuf lam, lbp_stats, lbp_labels, scratch;                // between the two launches; labels-only accumulators
    DevBuf evid, labels, marg, stats, dv, dm, de;              // staging of the host-buffer entries
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false, lbp_ran = false;
    std::set<hipStream_t> streams_used;
    ~fbn_epis() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        (void)fbn_lbp_destroy(lbp);
    }
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

template <class T>
int Upload(DevBuf &b, const std::vector<T> &v) {
    if (int rc = b.ensure(std::max<size_t>(v.size() * sizeof(T), 16))) return rc;
    if (!v.empty()) FBN_HIP(hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return FBN_OK;
}

int EpisDevice(fbn_epis *s, const RunArgs &r, const int8_t *d_ev, int32_t *d_labels, double *d_marg, double *d_stats,
               uint8_t *dv, double *dm, int32_t *de, hipStream_t st) {
    const int64_t nlam = r.ncases * s->M.sum_dom;
    if (r.ncases > 0x7fffffffll || nlam / 256 >= 0x7fffffffll)
        return SetError(FBN_ERR_LIMIT, "%lld cases in one call", (long long)r.ncases);
    s->streams_used.insert(st);
    // as fbn_jt_run_device's check: on the device, one stream sync
    if (int rc = fbn::EvidenceCheckDevice(d_ev, r.ncases, s->M.V, s->dom.as<int32_t>(), s->M.dom.data(),
                                          s->evcheck.as<unsigned long long>(), st))
        return rc;
    int rc;
    if ((rc = s->lam.ensure((size_t)nlam * 8)) || (rc = s->lbp_stats.ensure((size_t)r.ncases * 16)) ||
        (rc = s->lbp_labels.ensure((size_t)r.ncases * 4)))
        return rc;
    if (!d_marg) {  // labels only: the accumulator rows live in the handle
        if ((rc = s->scratch.ensure((size_t)nlam * 8))) return rc;
        d_marg = s->scratch.as<double>();
    }
    if (r.iters > 0) {
        if ((rc = fbn::LbpLambdaDevice(s->lbp, d_ev, r.ncases, r.iters, r.tol, r.damping, s->lbp_labels.as<int32_t>(),
                                       s->lbp_stats.as<double>(), s->lam.as<double>(), st)))
            return rc;
    } else {
        FBN_HIP(fbn_epis_fill(s->lam.as<double>(), nlam, 1.0, st));
    }
    s->lbp_ran = r.iters > 0;
    fbn::PcgStream R;
    fbn::PcgStreamInit(r.seed, R);
    fbn::EpisDeviceArgs a;
    memcpy(a.jump, R.jump, sizeof a.jump);
    a.M = fbn::DeviceModel{s->nodes.as<fbn::SampleNode>(), s->par.as<int32_t>(), s->prob.as<double>(), nullptr,
                           s->ent.as<int32_t>(), s->M.V, s->M.sum_dom, s->M.dom[0]};
    a.state = R.state, a.inc = R.inc;
    fbn::PcgJump(R, (uint64_t)63 * (uint64_t)s->M.V, &a.jm, &a.jc);
    a.ev = d_ev;
    a.ncases = r.ncases, a.S = r.S, a.case0 = r.case_offset, a.eps = r.eps;
    a.lam = s->lam.as<double>(), a.lbp_stats = r.iters > 0 ? s->lbp_stats.as<double>() : nullptr;
    a.labels = d_labels, a.marg = d_marg, a.stats = d_stats;
    a.dv = dv, a.dm = dm, a.de = de;
    FBN_HIP(hipEventRecord(s->ev0, st));
    FBN_HIP(fbn_epis_launch(&a, s->lds_lambda() ? 1 : 0, st));
    FBN_HIP(hipEventRecord(s->ev1, st));
    s->timed = true;
    return FBN_OK;
}

int EpisHostBuffers(fbn_epis *s, const RunArgs &r, const int8_t *evidence, int32_t *labels, double *marginals,
                    double *stats, uint8_t *values, double *mant, int32_t *expo, double *lambda) {
    if (int rc = fbn::CheckEpisArgs(s->M, r.ncases, r.S, r.case_offset, r.iters, r.tol, r.damping, r.eps)) return rc;
    if (r.ncases == 0) return FBN_OK;
    const int V = s->M.V, SD = s->M.sum_dom;
    if (s->device < 0) {
        if (int rc = fbn::CheckEvidenceHost(s->M, evidence, r.ncases)) return rc;
        return fbn::HostEpis(s->M, fbn::LbpModelOf(s->lbp), evidence, r.ncases, r.S, r.seed, r.case_offset, r.iters, r.tol,
                             r.damping, r.eps, labels, marginals, stats, values, mant, expo, lambda);
    }
    FBN_HIP(hipSetDevice(s->device));
    const size_t total = (size_t)r.ncases * (size_t)r.S;
    int rc;
    if ((rc = s->evid.ensure((size_t)r.ncases * V)) || (rc = s->labels.ensure((size_t)r.ncases * 4)) ||
        (rc = s->marg.ensure((size_t)r.ncases * SD * 8)) || (rc = s->stats.ensure((size_t)r.ncases * 32)))
        return rc;
    if (values && ((rc = s->dv.ensure(total * V)) || (rc = s->dm.ensure(total * 8)) || (rc = s->de.ensure(total * 4))))
        return rc;
    FBN_HIP(hipMemcpy(s->evid.p, evidence, (size_t)r.ncases * V, hipMemcpyHostToDevice));
    rc = EpisDevice(s, r, s->evid.as<int8_t>(), s->labels.as<int32_t>(), s->marg.as<double>(), s->stats.as<double>(),
                    values ? s->dv.as<uint8_t>() : nullptr, values ? s->dm.as<double>() : nullptr,
                    values ? s->de.as<int32_t>() : nullptr, nullptr);
    if (rc) return rc;
    FBN_HIP(hipMemcpy(labels, s->labels.p, (size_t)r.ncases * 4, hipMemcpyDeviceToHost));
    if (marginals) FBN_HIP(hipMemcpy(marginals, s->marg.p, (size_t)r.ncases * SD * 8, hipMemcpyDeviceToHost));
    if (stats) FBN_HIP(hipMemcpy(stats, s->stats.p, (size_t)r.ncases * 32, hipMemcpyDeviceToHost));
    if (values) {
        FBN_HIP(hipMemcpy(values, s->dv.p, total * V, hipMemcpyDeviceToHost));
        FBN_HIP(hipMemcpy(mant, s->dm.p, total * 8, hipMemcpyDeviceToHost));
        FBN_HIP(hipMemcpy(expo, s->de.p, total * 4, hipMemcpyDeviceToHost));
        FBN_HIP(hipMemcpy(lambda, s->lam.p, (size_t)r.ncases * SD * 8, hipMemcpyDeviceToHost));
    }
    return FBN_OK;
}

}  // namespace

extern "C" {

int fbn_epis_create(const fbn_network *net, int device, fbn_epis **out) {
    if (!net || !out) return SetError(FBN_ERR_ARG, "null pointer");
    *out = nullptr;
    fbn_epis *s = new fbn_epis;
    int rc = fbn::BuildSamplerModel(net->net, s->M);
    if (rc == FBN_OK) rc = fbn_lbp_create(net, device, &s->lbp);
    if (rc == FBN_OK && device >= 0) {
        s->device = device;
        rc = [&]() -> int {
            int r;
            if ((r = fbn::CheckDevice(device, nullptr)) || (r = Upload(s->nodes, s->M.nodes)) ||
                (r = Upload(s->par, s->M.par)) || (r = Upload(s->prob, s->M.prob)) || (r = Upload(s->ent, s->M.ent)) ||
                (r = Upload(s->dom, s->M.dom)) || (r = s->evcheck.ensure(8)))
                return r;
            FBN_HIP(hipEventCreate(&s->ev0));
            FBN_HIP(hipEventCreate(&s->ev1));
            return FBN_OK;
        }();
    }
    if (rc) {
        delete s;
        return rc;
    }
    *out = s;
    return FBN_OK;
}

int fbn_epis_destroy(fbn_epis *s) {
    if (!s) return FBN_OK;
    if (s->device >= 0) {  // runs are queued on caller streams: drain those before the buffers go
        (void)hipSetDevice(s->device);
        for (hipStream_t st : s->streams_used) (void)hipStreamSynchronize(st);
    }
    delete s;
    return FBN_OK;
}

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
    FBN_HIP(hipEventSynchronize(s->ev1));
    FBN_HIP(hipEventElapsedTime(sample_ms, s->ev0, s->ev1));
    return FBN_OK;
}

}  // extern "C"
