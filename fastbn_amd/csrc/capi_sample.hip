// capi_sample.hip -- the fbn_sampler_* / fbn_sample_* / fbn_lw_* section of include/fastbn.h: sampler
// handles over the host twin (sample_host.cpp) and the kernels' launches (sample.hip), and
// fbn_score_marginals.  Replaces the reference's PLS / LW stubs (src/main.cpp:97-121).
#include <hip/hip_runtime.h>

#include <vector>

#include "capi_sampler.h"
#include "launchers.h"

using fbn::SetError;

struct fbn_sampler : fbn::SamplerHandle {
    fbn::DevBuf cols;  // staging of fbn_sample_forward
};

namespace {

int ForwardDevice(fbn_sampler *s, int64_t n, uint64_t seed, uint8_t *d_cols, hipStream_t st) {
    fbn::PcgStream R;
    fbn::PcgStreamInit(seed, R);
    fbn::ForwardDeviceArgs a;
    memcpy(a.jump, R.jump, sizeof a.jump);
    a.M = s->View();
    a.state = R.state, a.inc = R.inc;
    fbn::PcgJump(R, (uint64_t)n, &a.jm, &a.jc);
    a.n = n;
    a.cols = d_cols;
    if ((n + 63) / 64 > 0x7fffffffll) return SetError(FBN_ERR_LIMIT, "forward sampling: %lld samples in one call", (long long)n);
    s->Note(st);
    return s->Timed(st, [&] { return fbn_sample_forward_launch(&a, st); });
}

int LwDevice(fbn_sampler *s, int method, const int8_t *d_ev, int64_t ncases, int64_t S, uint64_t seed,
             int64_t case_offset, int32_t *d_labels, double *d_marg, double *d_stats, uint8_t *dv, double *dm,
             int32_t *de, hipStream_t st) {
    if (int rc = s->OpenRun(d_ev, ncases, &d_marg, st)) return rc;
    fbn::PcgStream R;
    fbn::LwDeviceArgs a;
    s->FillArgs(a, R, seed, d_ev, ncases, S, case_offset, d_labels, d_marg, d_stats, dv, dm, de);
    a.method = method;
    return s->Timed(st, [&] { return fbn_lw_launch(&a, st); });
}

int LwHostBuffers(fbn_sampler *s, int method, const int8_t *evidence, int64_t ncases, int64_t S, uint64_t seed,
                  int64_t case_offset, int32_t *labels, double *marginals, double *stats, uint8_t *values, double *mant,
                  int32_t *expo) {
    if (int rc = fbn::CheckLwShape(s->M, method, ncases, S, case_offset)) return rc;
    if (ncases == 0) return FBN_OK;
    if (s->device < 0) {
        if (int rc = fbn::CheckEvidenceHost(s->M, evidence, ncases)) return rc;
        return fbn::HostLw(s->M, method, evidence, ncases, S, seed, case_offset, labels, marginals, stats, values, mant, expo);
    }
    return s->HostBuffers(evidence, ncases, 2, S, labels, marginals, stats, values, mant, expo, nullptr, 0, nullptr,
                          [&](const int8_t *d_ev, int32_t *d_labels, double *d_marg, double *d_stats, uint8_t *dv,
                              double *dm, int32_t *de) {
                              return LwDevice(s, method, d_ev, ncases, S, seed, case_offset, d_labels, d_marg, d_stats, dv,
                                              dm, de, nullptr);
                          });
}

}  // namespace

extern "C" {

int fbn_sampler_create(const fbn_network *net, int device, fbn_sampler **out) {
    return fbn::CreateHandle(net, out, [&](fbn_sampler *s) { return s->Create(net->net, device, true); });
}

int fbn_sampler_destroy(fbn_sampler *s) { return fbn::DestroyHandle(s); }

int fbn_sample_forward_device(fbn_sampler *s, int64_t n, uint64_t seed, uint8_t *d_cols, void *hip_stream) {
    if (!s || n < 0 || (n > 0 && !d_cols)) return SetError(FBN_ERR_ARG, "bad argument");
    if (s->device < 0) return SetError(FBN_ERR_NODEV, "host-only sampler (created with device < 0)");
    if (n == 0) return FBN_OK;
    if ((long double)n * s->M.V >= 9.2e18L) return SetError(FBN_ERR_ARG, "stream position beyond 2^63");
    FBN_HIP(hipSetDevice(s->device));
    return ForwardDevice(s, n, seed, d_cols, static_cast<hipStream_t>(hip_stream));
}

int fbn_sample_forward(fbn_sampler *s, int64_t n, uint64_t seed, uint8_t *cols) {
    if (!s || n < 0 || (n > 0 && !cols)) return SetError(FBN_ERR_ARG, "bad argument");
    if (n == 0) return FBN_OK;
    if ((long double)n * s->M.V >= 9.2e18L) return SetError(FBN_ERR_ARG, "stream position beyond 2^63");
    if (s->device < 0) return fbn::HostForward(s->M, n, seed, cols);
    FBN_HIP(hipSetDevice(s->device));
    const size_t bytes = (size_t)s->M.V * (size_t)n;
    if (int rc = s->cols.ensure(bytes)) return rc;
    if (int rc = ForwardDevice(s, n, seed, s->cols.as<uint8_t>(), nullptr)) return rc;
    FBN_HIP(hipMemcpy(cols, s->cols.p, bytes, hipMemcpyDeviceToHost));
    return FBN_OK;
}

int fbn_lw_run_device(fbn_sampler *s, int method, const int8_t *d_evidence, int64_t ncases, int64_t S, uint64_t seed,
                      int64_t case_offset, int32_t *d_labels, double *d_marginals, double *d_stats, void *hip_stream) {
    if (!s || (ncases > 0 && (!d_evidence || !d_labels))) return SetError(FBN_ERR_ARG, "bad argument");
    if (int rc = fbn::CheckLwShape(s->M, method, ncases, S, case_offset)) return rc;
    if (s->device < 0) return SetError(FBN_ERR_NODEV, "host-only sampler (created with device < 0)");
    if (ncases == 0) return FBN_OK;
    FBN_HIP(hipSetDevice(s->device));
    return LwDevice(s, method, d_evidence, ncases, S, seed, case_offset, d_labels, d_marginals, d_stats, nullptr, nullptr,
                    nullptr, static_cast<hipStream_t>(hip_stream));
}

int fbn_lw_run(fbn_sampler *s, int method, const int8_t *evidence, int64_t ncases, int64_t S, uint64_t seed,
               int64_t case_offset, int32_t *labels, double *marginals, double *stats) {
    if (!s || (ncases > 0 && (!evidence || !labels))) return SetError(FBN_ERR_ARG, "bad argument");
    return LwHostBuffers(s, method, evidence, ncases, S, seed, case_offset, labels, marginals, stats, nullptr, nullptr,
                         nullptr);
}

int fbn_lw_debug_samples(fbn_sampler *s, int method, const int8_t *evidence, int64_t ncases, int64_t S, uint64_t seed,
                         int64_t case_offset, uint8_t *values, double *mantissas, int32_t *exponents) {
    if (!s || (ncases > 0 && (!evidence || !values || !mantissas || !exponents))) return SetError(FBN_ERR_ARG, "bad argument");
    if (ncases > 0 && S > 0 && (ncases > FBN_SAMPLE_DEBUG_MAX || S > FBN_SAMPLE_DEBUG_MAX / ncases))
        return SetError(FBN_ERR_LIMIT, "debug samples: more than %lld samples", (long long)FBN_SAMPLE_DEBUG_MAX);
    std::vector<int32_t> labels((size_t)std::max<int64_t>(ncases, 1));
    return LwHostBuffers(s, method, evidence, ncases, S, seed, case_offset, labels.data(), nullptr, nullptr, values,
                         mantissas, exponents);
}

int fbn_sampler_last_kernel_ms(const fbn_sampler *s, float *ms) {
    if (!s) return SetError(FBN_ERR_ARG, "no timed launch");
    return s->LastKernelMs(ms);
}

int fbn_score_marginals(const fbn_network *net, const double *marginals, const double *golden, int64_t ncases,
                        double *mse_sum, double *hd_sum) {
    if (!net || !marginals || !golden || !mse_sum || !hd_sum) return SetError(FBN_ERR_ARG, "null pointer");
    return fbn::ScoreMarginals(net->net.dom, marginals, golden, ncases, mse_sum, hd_sum);
}

}  // extern "C"
