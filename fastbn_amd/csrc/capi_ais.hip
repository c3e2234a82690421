// capi_ais.hip -- the fbn_ais_* section of include/fastbn.h: handles of the adaptive samplers AIS-BN
// and SIS over the host twin (ais_host.cpp) and the one launch of a device run (sample_ais_kernel,
// ais.hip).  Replaces the reference's AIS-BN and SIS stubs (src/main.cpp:175-186, :149-160).
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <set>
#include <utility>
#include <vector>

#include "ais_model.h"
#include "fbn_device.h"
#include "fbn_internal.h"
#include "launchers.h"

using fbn::DevBuf;
using fbn::SetError;

struct fbn_ais {
    fbn::SamplerModel M;
    int device = -1, num_cu = 0;
    int64_t lds_bytes_max = FBN_AIS_LDS_DEFAULT;
    int max_workgroups = 0;
    DevBuf nodes, par, prob, cdf, ent, dom, evcheck;
    DevBuf ws, scratch;                                // the state's global home; labels-only accumulators
    std::map<std::pair<int, int>, DevBuf> eta;         // (method, m) -> its table, written once
    DevBuf evid, labels, marg, stats, dv, dm, de, di;  // staging of the host-buffer entries
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    std::set<hipStream_t> streams_used;
    ~fbn_ais() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
    // values [V][64], 64 weights, V flags (padded to 8); with the state in LDS also I and N
    int64_t base_bytes() const { return (int64_t)M.V * 64 + 512 + ((int64_t)M.V + 7) / 8 * 8; }
    int64_t lds_bytes() const { return base_bytes() + 16 * M.cells; }
    bool lds_state() const { return lds_bytes_max >= 0 && lds_bytes() <= lds_bytes_max; }
    int64_t grid(int64_t ncases) const {
        int per_cu = FBN_AIS_GROUPS_PER_CU;
        const int64_t b = lds_state() ? lds_bytes() : base_bytes();
        per_cu = (int)std::max<int64_t>(1, std::min<int64_t>(per_cu, 160 * 1024 / b));
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

template <class T>
int Upload(DevBuf &b, const std::vector<T> &v) {
    if (int rc = b.ensure(std::max<size_t>(v.size() * sizeof(T), 16))) return rc;
    if (!v.empty()) FBN_HIP(hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return FBN_OK;
}

int AisDevice(fbn_ais *s, const RunArgs &r, const int8_t *d_ev, int32_t *d_labels, double *d_marg, double *d_stats,
              uint8_t *dv, double *dm, int32_t *de, double *di, hipStream_t st) {
    if (r.ncases > 0x7fffffffll) return SetError(FBN_ERR_LIMIT, "%lld cases in one call", (long long)r.ncases);
    s->streams_used.insert(st);
    // as fbn_jt_run_device's check: on the device, one stream sync
    if (int rc = fbn::EvidenceCheckDevice(d_ev, r.ncases, s->M.V, s->dom.as<int32_t>(), s->M.dom.data(),
                                          s->evcheck.as<unsigned long long>(), st))
        return rc;
    int rc;
    if (!d_marg) {  // labels only: the accumulator rows live in the handle
        if ((rc = s->scratch.ensure((size_t)r.ncases * s->M.sum_dom * 8))) return rc;
        d_marg = s->scratch.as<double>();
    }
    const bool lds = s->lds_state();
    const int64_t grid = s->grid(r.ncases);
    if (!lds)
        if ((rc = s->ws.ensure((size_t)grid * 2 * (size_t)s->M.cells * 8))) return rc;
    DevBuf &eta = s->eta[{r.method, (int)r.m}];
    if (!eta.p) {  // a new buffer no launch reads yet
        std::vector<double> h((size_t)std::max<int64_t>(r.m, 1), 1.0);
        fbn::AisEta(r.method, (int)r.m, h.data());
        if ((rc = Upload(eta, h))) return rc;
    }
    fbn::PcgStream R;
    fbn::PcgStreamInit(r.seed, R);
    fbn::AisDeviceArgs a;
    memcpy(a.jump, R.jump, sizeof a.jump);
    a.M = fbn::DeviceModel{s->nodes.as<fbn::SampleNode>(), s->par.as<int32_t>(), s->prob.as<double>(), s->cdf.as<double>(),
                           s->ent.as<int32_t>(), s->M.V, s->M.sum_dom, s->M.dom[0]};
    a.state = R.state, a.inc = R.inc;
    fbn::PcgJump(R, (uint64_t)63 * (uint64_t)s->M.V, &a.jm, &a.jc);
    fbn::PcgJump(R, (uint64_t)(r.l - 64 * ((r.l - 1) / 64) - 1) * (uint64_t)s->M.V, &a.sm, &a.sc);
    a.ev = d_ev;
    a.ncases = r.ncases, a.S = r.S, a.case0 = r.case_offset, a.cells = s->M.cells;
    a.method = r.method, a.sch = fbn::AisStages(r.method, r.S, r.m, r.l), a.eps = r.eps;
    a.eta = eta.as<double>(), a.ws = lds ? nullptr : s->ws.as<double>();
    a.labels = d_labels, a.marg = d_marg, a.stats = d_stats;
    a.dv = dv, a.dm = dm, a.de = de, a.di = di;
    FBN_HIP(hipEventRecord(s->ev0, st));
    FBN_HIP(fbn_ais_launch(&a, lds ? 1 : 0, (size_t)(lds ? s->lds_bytes() : s->base_bytes()), (int)grid, st));
    FBN_HIP(hipEventRecord(s->ev1, st));
    s->timed = true;
    return FBN_OK;
}

int AisHostBuffers(fbn_ais *s, const RunArgs &r, const int8_t *evidence, int32_t *labels, double *marginals,
                   double *stats, uint8_t *values, double *mant, int32_t *expo, double *icpt) {
    if (int rc = fbn::CheckAisArgs(s->M, r.method, r.ncases, r.S, r.m, r.l, r.case_offset, r.eps)) return rc;
    if (r.ncases == 0) return FBN_OK;
    const int V = s->M.V, SD = s->M.sum_dom;
    if (s->device < 0) {
        if (int rc = fbn::CheckEvidenceHost(s->M, evidence, r.ncases)) return rc;
        return fbn::HostAis(s->M, r.method, evidence, r.ncases, r.S, r.m, r.l, r.seed, r.case_offset, r.eps, labels,
                            marginals, stats, values, mant, expo, icpt);
    }
    FBN_HIP(hipSetDevice(s->device));
    const size_t total = (size_t)r.ncases * (size_t)fbn::AisStages(r.method, r.S, r.m, r.l).T;
    const size_t nicpt = (size_t)r.ncases * (size_t)s->M.cells;
    int rc;
    if ((rc = s->evid.ensure((size_t)r.ncases * V)) || (rc = s->labels.ensure((size_t)r.ncases * 4)) ||
        (rc = s->marg.ensure((size_t)r.ncases * SD * 8)) || (rc = s->stats.ensure((size_t)r.ncases * 32)))
        return rc;
    if (values && ((rc = s->dv.ensure(total * V)) || (rc = s->dm.ensure(total * 8)) || (rc = s->de.ensure(total * 4)) ||
                   (rc = s->di.ensure(nicpt * 8))))
        return rc;
    FBN_HIP(hipMemcpy(s->evid.p, evidence, (size_t)r.ncases * V, hipMemcpyHostToDevice));
    rc = AisDevice(s, r, s->evid.as<int8_t>(), s->labels.as<int32_t>(), s->marg.as<double>(), s->stats.as<double>(),
                   values ? s->dv.as<uint8_t>() : nullptr, values ? s->dm.as<double>() : nullptr,
                   values ? s->de.as<int32_t>() : nullptr, values ? s->di.as<double>() : nullptr, nullptr);
    if (rc) return rc;
    FBN_HIP(hipMemcpy(labels, s->labels.p, (size_t)r.ncases * 4, hipMemcpyDeviceToHost));
    if (marginals) FBN_HIP(hipMemcpy(marginals, s->marg.p, (size_t)r.ncases * SD * 8, hipMemcpyDeviceToHost));
    if (stats) FBN_HIP(hipMemcpy(stats, s->stats.p, (size_t)r.ncases * 32, hipMemcpyDeviceToHost));
    if (values) {
        FBN_HIP(hipMemcpy(values, s->dv.p, total * V, hipMemcpyDeviceToHost));
        FBN_HIP(hipMemcpy(mant, s->dm.p, total * 8, hipMemcpyDeviceToHost));
        FBN_HIP(hipMemcpy(expo, s->de.p, total * 4, hipMemcpyDeviceToHost));
        FBN_HIP(hipMemcpy(icpt, s->di.p, nicpt * 8, hipMemcpyDeviceToHost));
    }
    return FBN_OK;
}

}  // namespace

extern "C" {

int fbn_ais_create(const fbn_network *net, int device, fbn_ais **out) {
    if (!net || !out) return SetError(FBN_ERR_ARG, "null pointer");
    *out = nullptr;
    fbn_ais *s = new fbn_ais;
    int rc = fbn::BuildSamplerModel(net->net, s->M);
    if (rc == FBN_OK && device >= 0) {
        s->device = device;
        rc = [&]() -> int {
            int r;
            if ((r = fbn::CheckDevice(device, &s->num_cu)) || (r = Upload(s->nodes, s->M.nodes)) ||
                (r = Upload(s->par, s->M.par)) || (r = Upload(s->prob, s->M.prob)) || (r = Upload(s->cdf, s->M.cdf)) ||
                (r = Upload(s->ent, s->M.ent)) || (r = Upload(s->dom, s->M.dom)) || (r = s->evcheck.ensure(8)))
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

int fbn_ais_destroy(fbn_ais *s) {
    if (!s) return FBN_OK;
    if (s->device >= 0) {  // runs are queued on caller streams: drain those before the buffers go
        (void)hipSetDevice(s->device);
        for (hipStream_t st : s->streams_used) (void)hipStreamSynchronize(st);
    }
    delete s;
    return FBN_OK;
}

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
    if (!s || !ms || !s->timed) return SetError(FBN_ERR_ARG, "no timed launch");
    FBN_HIP(hipEventSynchronize(s->ev1));
    FBN_HIP(hipEventElapsedTime(ms, s->ev0, s->ev1));
    return FBN_OK;
}

}  // extern "C"
