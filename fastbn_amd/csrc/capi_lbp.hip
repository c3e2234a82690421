// capi_lbp.hip -- the fbn_lbp_* section of include/fastbn.h: loopy belief propagation handles over
// the host twin (lbp_host.cpp) and the kernel (lbp.hip).  Replaces the reference's LBP stub
// (src/main.cpp:136-147) and its Parameter::propagation_length (include/Parameter.h:33).
#include <hip/hip_runtime.h>

#include <vector>

#include "fbn_device.h"
#include "fbn_internal.h"
#include "launchers.h"
#include "lbp_model.h"

using fbn::DevBuf;
using fbn::SetError;
using fbn::Upload;

// what a workgroup's dynamic LDS may hold without a function attribute
static constexpr int64_t kLbpLdsDefault = 64 * 1024;
// workgroups per CU of the persistent grid (one wave each)
static constexpr int kLbpGroupsPerCu = 16;

struct fbn_lbp : fbn::DeviceHandle {
    fbn::LbpModel M;
    int64_t lds_bytes_max = kLbpLdsDefault;
    int max_groups = 0;
    DevBuf edges, terms, bin_edge, order, var_off, var_moff, marg_var, marg_off, self_moff, prob, ws;
    DevBuf evid, labels, marg, stats, msgs;  // staging of the host-buffer entries
    int64_t lds_bytes() const { return 24 * M.M; }
    bool lds_path() const { return lds_bytes_max >= 0 && lds_bytes() <= lds_bytes_max; }
};

namespace {

// d_lambda: LbpDeviceArgs::lambda or NULL.  checked: the caller has range-checked the evidence already.
int LbpDevice(fbn_lbp *s, const int8_t *d_ev, int64_t ncases, int iters, double tol, double damping, int32_t *d_labels,
              double *d_marg, double *d_stats, double *d_msgs, hipStream_t st, double *d_lambda = nullptr,
              bool checked = false) {
    s->Note(st);
    // as fbn_jt_run_device's check: on the device, one stream sync
    if (!checked)
        if (int rc = s->evidence.Run(d_ev, ncases, st)) return rc;
    const bool lds = s->lds_path();
    int per_cu = kLbpGroupsPerCu;
    if (lds) per_cu = (int)std::max<int64_t>(1, std::min<int64_t>(per_cu, fbn::kCuLdsBytes / std::max<int64_t>(1, s->lds_bytes())));
    int64_t grid = std::min<int64_t>(ncases, (int64_t)s->num_cu * per_cu);
    if (s->max_groups > 0) grid = std::min<int64_t>(grid, s->max_groups);
    if (!lds)
        if (int rc = s->ws.ensure((size_t)grid * 3 * (size_t)s->M.M * 8)) return rc;
    fbn::LbpDeviceArgs a;
    a.edges = s->edges.as<fbn::LbpEdge>(), a.terms = s->terms.as<fbn::LbpTerm>();
    a.bin_edge = s->bin_edge.as<int32_t>(), a.order = s->order.as<int32_t>();
    a.var_off = s->var_off.as<int32_t>(), a.var_moff = s->var_moff.as<int32_t>();
    a.marg_var = s->marg_var.as<int32_t>(), a.marg_off = s->marg_off.as<int32_t>();
    a.dom = s->evidence.dom.as<int32_t>();
    a.prob = s->prob.as<double>();
    a.ev = d_ev;
    a.V = s->M.V, a.SD = s->M.sum_dom, a.M = (int)s->M.M, a.d0 = s->M.dom[0];
    a.ncases = ncases, a.iters = iters, a.tol = tol, a.damping = damping;
    a.labels = d_labels, a.marg = d_marg, a.stats = d_stats, a.messages = d_msgs;
    a.ws = s->ws.as<double>();
    a.lambda = d_lambda, a.self_moff = s->self_moff.as<int32_t>();
    return s->Timed(st, [&] { return fbn_lbp_launch(&a, lds ? 1 : 0, (size_t)s->lds_bytes(), (int)grid, st); });
}

int LbpHostBuffers(fbn_lbp *s, const int8_t *evidence, int64_t ncases, int iters, double tol, double damping,
                   int32_t *labels, double *marginals, double *stats, double *messages) {
    if (ncases == 0) return FBN_OK;
    const int V = s->M.V, SD = s->M.sum_dom;
    if (s->device < 0) {
        if (int rc = fbn::CheckLbpEvidence(s->M, evidence, ncases)) return rc;
        return fbn::HostLbp(s->M, evidence, ncases, iters, tol, damping, labels, marginals, stats, messages);
    }
    FBN_HIP(hipSetDevice(s->device));
    const size_t mbytes = (size_t)ncases * 2 * (size_t)s->M.M * 8;
    int rc;
    if ((rc = s->evid.ensure((size_t)ncases * V)) || (rc = s->labels.ensure((size_t)ncases * 4)) ||
        (rc = s->stats.ensure((size_t)ncases * 16)) || (marginals && (rc = s->marg.ensure((size_t)ncases * SD * 8))) ||
        (messages && (rc = s->msgs.ensure(mbytes))))
        return rc;
    FBN_HIP(hipMemcpy(s->evid.p, evidence, (size_t)ncases * V, hipMemcpyHostToDevice));
    rc = LbpDevice(s, s->evid.as<int8_t>(), ncases, iters, tol, damping, s->labels.as<int32_t>(),
                   marginals ? s->marg.as<double>() : nullptr, s->stats.as<double>(),
                   messages ? s->msgs.as<double>() : nullptr, nullptr);
    if (rc) return rc;
    FBN_HIP(hipMemcpy(labels, s->labels.p, (size_t)ncases * 4, hipMemcpyDeviceToHost));
    if (marginals) FBN_HIP(hipMemcpy(marginals, s->marg.p, (size_t)ncases * SD * 8, hipMemcpyDeviceToHost));
    if (stats) FBN_HIP(hipMemcpy(stats, s->stats.p, (size_t)ncases * 16, hipMemcpyDeviceToHost));
    if (messages) FBN_HIP(hipMemcpy(messages, s->msgs.p, mbytes, hipMemcpyDeviceToHost));
    return FBN_OK;
}

}  // namespace

namespace fbn {

const LbpModel &LbpModelOf(const fbn_lbp *s) { return s->M; }

int LbpLambdaDevice(fbn_lbp *s, const int8_t *d_ev, int64_t ncases, int iters, double tol, double damping,
                    int32_t *d_labels, double *d_stats, double *d_lambda, void *hip_stream) {
    return LbpDevice(s, d_ev, ncases, iters, tol, damping, d_labels, nullptr, d_stats, nullptr,
                     static_cast<hipStream_t>(hip_stream), d_lambda, true);
}

}  // namespace fbn

extern "C" {

int fbn_lbp_create(const fbn_network *net, int device, fbn_lbp **out) {
    return fbn::CreateHandle(net, out, [&](fbn_lbp *s) -> int {
        int r = fbn::BuildLbpModel(net->net, s->M);
        if (r || device < 0) return r;
        if ((r = s->Attach(device)) || (r = Upload(s->edges, s->M.edges)) || (r = Upload(s->terms, s->M.terms)) ||
            (r = Upload(s->bin_edge, s->M.bin_edge)) || (r = Upload(s->order, s->M.order)) ||
            (r = Upload(s->var_off, s->M.var_off)) || (r = Upload(s->var_moff, s->M.var_moff)) ||
            (r = Upload(s->marg_var, s->M.marg_var)) || (r = Upload(s->marg_off, s->M.marg_off)) ||
            (r = Upload(s->self_moff, s->M.self_moff)) || (r = Upload(s->prob, s->M.prob)))
            return r;
        return s->evidence.Attach(s->M.dom);
    });
}

int fbn_lbp_destroy(fbn_lbp *s) { return fbn::DestroyHandle(s); }

int fbn_lbp_info(const fbn_lbp *s, int64_t *edges, int64_t *msg_doubles, int64_t *lds_bytes, int *path) {
    if (!s) return SetError(FBN_ERR_ARG, "null pointer");
    if (edges) *edges = s->M.E;
    if (msg_doubles) *msg_doubles = s->M.M;
    if (lds_bytes) *lds_bytes = s->lds_bytes();
    if (path) *path = s->lds_path() ? 0 : 1;
    return FBN_OK;
}

int fbn_lbp_run(fbn_lbp *s, const int8_t *evidence, int64_t ncases, int iters, double tol, double damping,
                int32_t *labels, double *marginals, double *stats) {
    if (!s || (ncases > 0 && (!evidence || !labels))) return SetError(FBN_ERR_ARG, "bad argument");
    if (int rc = fbn::CheckLbpArgs(ncases, iters, tol, damping)) return rc;
    return LbpHostBuffers(s, evidence, ncases, iters, tol, damping, labels, marginals, stats, nullptr);
}

int fbn_lbp_run_device(fbn_lbp *s, const int8_t *d_evidence, int64_t ncases, int iters, double tol, double damping,
                       int32_t *d_labels, double *d_marginals, double *d_stats, void *hip_stream) {
    if (!s || (ncases > 0 && (!d_evidence || !d_labels))) return SetError(FBN_ERR_ARG, "bad argument");
    if (int rc = fbn::CheckLbpArgs(ncases, iters, tol, damping)) return rc;
    if (s->device < 0) return SetError(FBN_ERR_NODEV, "host-only handle (created with device < 0)");
    if (ncases == 0) return FBN_OK;
    FBN_HIP(hipSetDevice(s->device));
    return LbpDevice(s, d_evidence, ncases, iters, tol, damping, d_labels, d_marginals, d_stats, nullptr,
                     static_cast<hipStream_t>(hip_stream));
}

int fbn_lbp_debug_messages(fbn_lbp *s, const int8_t *evidence, int64_t ncases, int iters, double damping,
                           double *messages) {
    if (!s || (ncases > 0 && (!evidence || !messages))) return SetError(FBN_ERR_ARG, "bad argument");
    if (int rc = fbn::CheckLbpArgs(ncases, iters, 0.0, damping)) return rc;
    if (ncases > 0 && ncases > FBN_LBP_DEBUG_MAX / (2 * s->M.M))
        return SetError(FBN_ERR_LIMIT, "debug messages: more than %lld doubles", (long long)FBN_LBP_DEBUG_MAX);
    std::vector<int32_t> labels((size_t)std::max<int64_t>(ncases, 1));
    return LbpHostBuffers(s, evidence, ncases, iters, -1.0, damping, labels.data(), nullptr, nullptr, messages);
}

int fbn_lbp_set_tuning(fbn_lbp *s, int64_t lds_bytes_max, int max_groups) {
    if (!s || max_groups < 0) return SetError(FBN_ERR_ARG, "bad argument");
    if (lds_bytes_max > kLbpLdsDefault)
        return SetError(FBN_ERR_ARG, "lds_bytes_max %lld beyond %lld", (long long)lds_bytes_max, (long long)kLbpLdsDefault);
    s->lds_bytes_max = lds_bytes_max == 0 ? kLbpLdsDefault : lds_bytes_max;
    s->max_groups = max_groups;
    return FBN_OK;
}

int fbn_lbp_last_kernel_ms(const fbn_lbp *s, float *ms) {
    if (!s) return SetError(FBN_ERR_ARG, "no timed launch");
    return s->LastKernelMs(ms);
}

}  // extern "C"
