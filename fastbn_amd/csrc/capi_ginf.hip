// capi_ginf.hip -- the device entries of the linear-Gaussian networks (include/fastbn.h, fbn_ginf_* and
// fbn_gnet_learn): an inference handle on DeviceHandle's base that keeps the joint N(mu, Sigma) of one network
// resident, runs batches of evidence cases through ginf.hip (host buffers staged through pinned memory on the
// handle's own stream, or the caller's device buffers on the caller's stream), and on a host-only handle runs
// the twin (ginf_host.cpp).  Parameter learning downloads a Gaussian CI context's moments once and solves on
// the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "fbn_device.h"
#include "gci.h"
#include "ginf.h"
#include "ginf_model.h"
#include "launchers.h"

using fbn::DevBuf;
using fbn::SetError;

// workgroups per CU of the persistent grid when their LDS allows more than one
static constexpr int kGinfGroupsPerCu = 8;

struct fbn_ginf : fbn::DeviceHandle {
    int n = 0;
    std::vector<double> mu, Sigma;  // a host-only handle's joint (a device handle keeps it on the device alone)
    DevBuf d_mu, d_Sigma, d_ev, d_mean, d_var, d_logp, d_word;
    hipStream_t stream = nullptr;
    void *h_in = nullptr, *h_out = nullptr;  // pinned staging of fbn_ginf_run
    size_t h_in_bytes = 0, h_out_bytes = 0;
    unsigned long long *h_word = nullptr;  // pinned: the evidence check's two words
    int max_workgroups = 0;
    int64_t degenerate = 0;
    int last_m_max = 0, last_lds = 0, last_grid = 0;
    ~fbn_ginf() {
        if (h_in) (void)hipHostFree(h_in);
        if (h_out) (void)hipHostFree(h_out);
        if (h_word) (void)hipHostFree(h_word);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

int GinfDevice(fbn_ginf *h, const double *d_ev, int64_t ncases, int m_max, double *d_mean, double *d_var, double *d_logp,
               hipStream_t st) {
    h->Note(st);
    const int lds = fbn_ginf_lds_bytes(h->n, m_max);
    const int per_cu = (int)std::max<int64_t>(1, std::min<int64_t>(kGinfGroupsPerCu, fbn::kCuLdsBytes / lds));
    int64_t grid = std::min<int64_t>(ncases, (int64_t)h->num_cu * per_cu);
    if (h->max_workgroups > 0) grid = std::min<int64_t>(grid, h->max_workgroups);
    h->last_m_max = m_max, h->last_lds = lds, h->last_grid = (int)grid;
    const GinfArgs a{h->d_mu.as<double>(), h->d_Sigma.as<double>(), h->n, d_ev, (long long)ncases, d_mean, d_var, d_logp, lds};
    return h->Timed(st, [&] { return fbn_ginf_launch(&a, (int)grid, st); });
}

// the evidence check of a device batch: one stream sync, as the discrete engines' check
int GinfCheckDevice(fbn_ginf *h, const double *d_ev, int64_t ncases, hipStream_t st, int *m_max) {
    unsigned long long *d_word = h->d_word.as<unsigned long long>();
    FBN_HIP(hipMemsetAsync(d_word, 0xFF, 16, st));
    const int grid = (int)std::min<int64_t>(ncases, (int64_t)h->num_cu * kGinfGroupsPerCu);
    hipError_t e = fbn_ginf_check_launch(d_ev, (long long)ncases, h->n, d_word, grid, st);
    if (e != hipSuccess) return SetError(FBN_ERR_HIP, "evidence check: %s", hipGetErrorString(e));
    FBN_HIP(hipMemcpyAsync(h->h_word, d_word, 16, hipMemcpyDeviceToHost, st));
    FBN_HIP(hipStreamSynchronize(st));
    if (h->h_word[0] != ~0ull)
        return SetError(FBN_ERR_ARG, "case %lld: evidence for variable %d is infinite", (long long)(h->h_word[0] / (unsigned)h->n),
                        (int)(h->h_word[0] % (unsigned)h->n));
    const unsigned long long m = ~0ull - h->h_word[1];
    if (m > (unsigned long long)kGinfMaxObs)
        return SetError(FBN_ERR_LIMIT, "a case observes %llu variables (supported up to %d)", m, kGinfMaxObs);
    *m_max = (int)m;
    return FBN_OK;
}

}  // namespace

extern "C" {

int fbn_gnet_learn(fbn_gci_ctx *c, const int32_t *parent_off, const int32_t *parents, fbn_gnet **out) {
    if (!c || !out) return SetError(FBN_ERR_ARG, "null pointer");
    int n = 0;
    int64_t N = 0;
    std::vector<double> mean, ss, R;
    if (int rc = fbn::GciMoments(c, &n, &N, mean, ss, R)) return rc;
    auto net = std::unique_ptr<fbn_gnet>(new (std::nothrow) fbn_gnet());
    if (!net) return SetError(FBN_ERR_NOMEM, "out of memory");
    if (int rc = fbn::GnetLearn(n, N, mean.data(), ss.data(), R.data(), parent_off, parents, net.get())) return rc;
    *out = net.release();
    return FBN_OK;
}

int fbn_ginf_create(const fbn_gnet *net, int device, fbn_ginf **out) {
    if (!net || !out) return SetError(FBN_ERR_ARG, "null pointer");
    *out = nullptr;
    if (net->n > kGinfMaxVars) return SetError(FBN_ERR_LIMIT, "%d variables (supported up to %d)", net->n, kGinfMaxVars);
    auto h = std::unique_ptr<fbn_ginf>(new (std::nothrow) fbn_ginf());
    if (!h) return SetError(FBN_ERR_NOMEM, "out of memory");
    const size_t n = (size_t)net->n;
    h->n = net->n;
    h->mu.assign(n, 0.0), h->Sigma.assign(n * n, 0.0);
    fbn::GnetJoint(*net, h->mu.data(), h->Sigma.data());
    if (device >= 0) {
        int rc;
        if ((rc = h->Attach(device)) || (rc = fbn::Upload(h->d_mu, h->mu)) || (rc = fbn::Upload(h->d_Sigma, h->Sigma)) ||
            (rc = h->d_word.ensure(16)))
            return rc;
        std::vector<double>().swap(h->Sigma);
        FBN_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
        hipError_t e = hipHostMalloc((void **)&h->h_word, 16, hipHostMallocDefault);
        if (e != hipSuccess) return SetError(FBN_ERR_NOMEM, "hipHostMalloc: %s", hipGetErrorString(e));
    }
    *out = h.release();
    return FBN_OK;
}

int fbn_ginf_destroy(fbn_ginf *h) { return fbn::DestroyHandle(h); }

int fbn_ginf_run(fbn_ginf *h, const double *evidence, int64_t ncases, double *mean, double *var, double *logp,
                 int64_t *degenerate) {
    if (!h || ncases < 0 || (ncases > 0 && !evidence)) return SetError(FBN_ERR_ARG, "bad argument");
    if (degenerate) *degenerate = 0;
    h->degenerate = 0;
    if (ncases == 0) return FBN_OK;
    int m_max = 0;
    if (int rc = fbn::GinfCheckEvidence(evidence, ncases, h->n, &m_max)) return rc;
    if (h->device < 0) {
        fbn::GinfHostRun(h->mu.data(), h->Sigma.data(), h->n, evidence, ncases, mean, var, logp, &h->degenerate);
        if (degenerate) *degenerate = h->degenerate;
        return FBN_OK;
    }
    FBN_HIP(hipSetDevice(h->device));
    const size_t row = (size_t)ncases * (size_t)h->n * 8, lp = (size_t)ncases * 8;
    const size_t out_bytes = (mean ? row : 0) + (var ? row : 0) + lp;
    int rc;
    if ((rc = fbn::PinnedEnsure(h->h_in, h->h_in_bytes, row)) || (rc = fbn::PinnedEnsure(h->h_out, h->h_out_bytes, out_bytes)) ||
        (rc = h->d_ev.ensure(row)) || (mean && (rc = h->d_mean.ensure(row))) || (var && (rc = h->d_var.ensure(row))) ||
        (rc = h->d_logp.ensure(lp)))
        return rc;
    hipStream_t st = h->stream;
    memcpy(h->h_in, evidence, row);
    FBN_HIP(hipMemcpyAsync(h->d_ev.p, h->h_in, row, hipMemcpyHostToDevice, st));
    if ((rc = GinfDevice(h, h->d_ev.as<double>(), ncases, m_max, mean ? h->d_mean.as<double>() : nullptr,
                         var ? h->d_var.as<double>() : nullptr, h->d_logp.as<double>(), st)))
        return rc;
    // pinned result: mean, var (those asked for), then logp
    char *o = static_cast<char *>(h->h_out), *o_mean = o, *o_var = o + (mean ? row : 0), *o_lp = o_var + (var ? row : 0);
    if (mean) FBN_HIP(hipMemcpyAsync(o_mean, h->d_mean.p, row, hipMemcpyDeviceToHost, st));
    if (var) FBN_HIP(hipMemcpyAsync(o_var, h->d_var.p, row, hipMemcpyDeviceToHost, st));
    FBN_HIP(hipMemcpyAsync(o_lp, h->d_logp.p, lp, hipMemcpyDeviceToHost, st));
    FBN_HIP(hipStreamSynchronize(st));
    if (mean) memcpy(mean, o_mean, row);
    if (var) memcpy(var, o_var, row);
    if (logp) memcpy(logp, o_lp, lp);
    // a case is degenerate exactly when its log density is NaN
    const double *l = reinterpret_cast<const double *>(o_lp);
    for (int64_t c = 0; c < ncases; ++c) h->degenerate += l[c] != l[c];
    if (degenerate) *degenerate = h->degenerate;
    return FBN_OK;
}

int fbn_ginf_run_device(fbn_ginf *h, const double *d_evidence, int64_t ncases, double *d_mean, double *d_var, double *d_logp,
                        void *hip_stream) {
    if (!h) return SetError(FBN_ERR_ARG, "null pointer");
    if (h->device < 0) return SetError(FBN_ERR_NODEV, "host-only handle (created with device < 0)");
    if (ncases < 0 || (ncases > 0 && !d_evidence)) return SetError(FBN_ERR_ARG, "bad argument");
    if (ncases == 0) return FBN_OK;
    FBN_HIP(hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    int m_max = 0;
    if (int rc = GinfCheckDevice(h, d_evidence, ncases, st, &m_max)) return rc;
    return GinfDevice(h, d_evidence, ncases, m_max, d_mean, d_var, d_logp, st);
}

int fbn_ginf_set_tuning(fbn_ginf *h, int32_t max_workgroups) {
    if (!h || max_workgroups < 0) return SetError(FBN_ERR_ARG, "bad argument");
    h->max_workgroups = max_workgroups;
    return FBN_OK;
}

int fbn_ginf_info(const fbn_ginf *h, int64_t out[6]) {
    if (!h || !out) return SetError(FBN_ERR_ARG, "null pointer");
    out[0] = h->n, out[1] = h->last_m_max, out[2] = h->last_lds, out[3] = h->last_grid;
    out[4] = h->last_lds ? fbn_ginf_tile(h->last_lds, h->n, h->last_m_max) : 0;
    out[5] = h->degenerate;
    return FBN_OK;
}

int fbn_ginf_last_kernel_ms(const fbn_ginf *h, float *ms) {
    if (!h) return SetError(FBN_ERR_ARG, "no timed launch");
    return h->LastKernelMs(ms);
}

}  // extern "C"
