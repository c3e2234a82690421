// capi_omcmc.hip -- the device entries of order MCMC (include/fastbn.h): fbn_omcmc_run / _run_bd and the testing
// entry fbn_omcmc_order_terms over a CI context's resident column store.  The family lists are enumerated by
// exact_host.cpp's enumerator and scored through the device scorer (capi_hc.hip), as the lattice learners'
// candidates are; they go up once as one array plus offsets.  The chains are order_mcmc.hip's; the result is
// assembled by the code the host twin runs (order_mcmc_host.cpp).
//
// The state (the lists, 16 bytes an entry; per chain 512 n + 64 + 8 samples + 8 bytes) lives for one call: it is
// sized against the free device memory before anything is allocated and freed on return.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <new>
#include <vector>

#include "capi_state.h"
#include "launchers.h"
#include "learner_device.h"
#include "order_mcmc.h"

using fbn::SetError;

namespace fbn {

namespace {

struct DeviceLists {
    DevBuf ent, off;
};

// the lists through the device scorer, then up; extra_bytes: what the caller allocates beside them
int UploadLists(fbn_ci_ctx *c, const fbn_exact_options &opt, int prior, const fbn_bd_score *bd, int64_t cap, size_t extra_bytes,
                OmcmcLists *L, DeviceLists *D, fbn_exact_info *xi, double *upload_ms) {
    if (int rc = OmcmcBuildLists(c->nvars, c->dims.data(), opt, prior, HcDeviceScorer(c, bd), cap, L, xi)) return rc;
    const size_t ent_bytes = L->ent.size() * sizeof(OmcmcEntry), off_bytes = L->off.size() * sizeof(long long);
    size_t free_b = 0, total_b = 0;
    FBN_HIP(hipMemGetInfo(&free_b, &total_b));
    if (ent_bytes + off_bytes + extra_bytes > free_b)
        return SetError(FBN_ERR_LIMIT, "order MCMC: %zu family-list entries and the chains' state take %zu bytes, %zu are free on the device",
                        L->ent.size(), ent_bytes + off_bytes + extra_bytes, free_b);
    if (int rc = D->ent.ensure(ent_bytes)) return rc;
    if (int rc = D->off.ensure(off_bytes)) return rc;
    const auto t0 = Clock::now();
    static_assert(sizeof(long long) == sizeof(int64_t), "offsets are uploaded as they are");
    FBN_HIP(hipMemcpy(D->ent.p, L->ent.data(), ent_bytes, hipMemcpyHostToDevice));
    FBN_HIP(hipMemcpy(D->off.p, L->off.data(), off_bytes, hipMemcpyHostToDevice));
    *upload_ms = MsSince(t0);
    return FBN_OK;
}

int OmcmcRunDevice(fbn_ci_ctx *c, const fbn_exact_options &opt, int prior, const fbn_bd_score *bd, const fbn_omcmc_options &m,
                   fbn_omcmc_result *res) {
    const auto t_start = Clock::now();
    const int n = c->nvars;
    const size_t acc_n = (size_t)m.chains * n * 64, ord_n = (size_t)m.chains * 64, tr_n = (size_t)m.chains * m.samples;
    OmcmcLists L;
    DeviceLists D;
    fbn_exact_info xi{};
    double upload_ms = 0.0;
    if (int rc = UploadLists(c, opt, prior, bd, m.max_families, acc_n * 8 + ord_n + tr_n * 8 + (size_t)m.chains * 8, &L, &D, &xi, &upload_ms))
        return rc;
    OmcmcStartResult(n, prior, m, L, xi, res);
    fbn_omcmc_info &info = res->info;
    info.upload_wall_ms = upload_ms;
    DevBuf acc, orders, trace, accepted;
    int rc;
    if ((rc = acc.ensure(acc_n * 8)) || (rc = orders.ensure(ord_n)) || (rc = trace.ensure(tr_n * 8)) ||
        (rc = accepted.ensure((size_t)m.chains * 8)))
        return rc;

    PcgStream R;
    PcgStreamInit(m.seed, R);
    OmcmcDeviceArgs a{};
    a.ent = D.ent.as<OmcmcEntry>(), a.off = D.off.as<long long>();
    a.n = n, a.group = c->omcmc_group > 0 ? c->omcmc_group : kOmcmcGroupDefault;
    a.state = R.state, a.inc = R.inc;
    std::copy(R.jump, R.jump + 256, a.jump);
    a.chains = m.chains, a.chain0 = m.chain_offset, a.burn_in = m.burn_in, a.thin = m.thin, a.samples = m.samples;
    a.orders = orders.as<uint8_t>(), a.acc = acc.as<double>(), a.trace = trace.as<double>(), a.accepted = accepted.as<long long>();
    info.chains_per_group = a.group;
    info.steps_per_launch = c->omcmc_steps_per_launch > 0 ? c->omcmc_steps_per_launch : info.steps;

    hipStream_t s = c->stream;
    std::vector<double> h_acc;  // sized once the launches are queued: the host fills them while the chains run
    std::vector<uint8_t> h_ord;
    static_assert(sizeof(long long) == sizeof(int64_t), "accepted counts are copied as they are");
    rc = Phase(
        c, &info.chain_kernel_ms, &info.chain_wall_ms,
        [&]() -> int {
            for (int64_t t = 0; t < info.steps; t += info.steps_per_launch) {
                a.t0 = t, a.t1 = std::min<int64_t>(info.steps, t + info.steps_per_launch);
                const hipError_t e = fbn_omcmc_chain_launch(&a, s);
                if (e != hipSuccess) return SetError(FBN_ERR_HIP, "order MCMC launch at step %lld: %s", (long long)t, hipGetErrorString(e));
                ++info.launches;
            }
            return FBN_OK;
        },
        [&]() -> int {
            h_acc.resize(acc_n), h_ord.resize(ord_n);
            FBN_HIP(hipMemcpyAsync(h_acc.data(), acc.p, acc_n * 8, hipMemcpyDeviceToHost, s));
            FBN_HIP(hipMemcpyAsync(h_ord.data(), orders.p, ord_n, hipMemcpyDeviceToHost, s));
            FBN_HIP(hipMemcpyAsync(res->log_score.data(), trace.p, tr_n * 8, hipMemcpyDeviceToHost, s));
            FBN_HIP(hipMemcpyAsync(res->accepted.data(), accepted.p, (size_t)m.chains * 8, hipMemcpyDeviceToHost, s));
            return FBN_OK;
        });
    if (rc) return rc;
    OmcmcFinish(n, m, h_acc.data(), h_ord.data(), res);
    info.wall_ms = MsSince(t_start);
    return FBN_OK;
}

}  // namespace
}  // namespace fbn

// fbn_omcmc_run (bd == nullptr; *bd outlives the run) and fbn_omcmc_run_bd
static int OmcmcRun(fbn_ci_ctx *c, const fbn_exact_options *options, int32_t prior, const fbn_bd_score *bd,
                    const fbn_omcmc_options *mcmc, fbn_omcmc_result **out) {
    if (!c || !options || !mcmc || !out) return SetError(FBN_ERR_ARG, "null pointer");
    if (int rc = fbn::OmcmcCheck(c->nvars, c->dims.data(), *options, prior)) return rc;
    if (int rc = fbn::OmcmcCheckRun(*mcmc)) return rc;
    if (int rc = fbn::HcCheckSamples(c->N)) return rc;
    FBN_HIP(hipSetDevice(c->device));
    auto r = std::unique_ptr<fbn_omcmc_result>(new (std::nothrow) fbn_omcmc_result());
    if (!r) return SetError(FBN_ERR_NOMEM, "out of memory");
    if (int rc = fbn::OmcmcRunDevice(c, *options, prior, bd, *mcmc, r.get())) return rc;
    c->last_ms = (float)(r->info.score_kernel_ms + r->info.chain_kernel_ms);
    *out = r.release();
    return FBN_OK;
}

extern "C" {

int fbn_omcmc_run(fbn_ci_ctx *c, const fbn_exact_options *options, int32_t prior, const fbn_omcmc_options *mcmc,
                  fbn_omcmc_result **out) {
    return OmcmcRun(c, options, prior, nullptr, mcmc, out);
}

int fbn_omcmc_run_bd(fbn_ci_ctx *c, const fbn_exact_options *options, int32_t prior, const fbn_bd_score *bd,
                     const fbn_omcmc_options *mcmc, fbn_omcmc_result **out) {
    if (int rc = fbn::BdCheck(bd)) return rc;
    return OmcmcRun(c, options, prior, bd, mcmc, out);
}

int fbn_omcmc_order_terms(fbn_ci_ctx *c, const fbn_exact_options *options, int32_t prior, const fbn_bd_score *bd,
                          int64_t max_families, const int32_t *orders, int64_t k, double *term, double *arcs) {
    if (!c || !options || !term || !arcs) return SetError(FBN_ERR_ARG, "null pointer");
    if (bd)
        if (int rc = fbn::BdCheck(bd)) return rc;
    const int n = c->nvars;
    if (int rc = fbn::OmcmcCheck(n, c->dims.data(), *options, prior)) return rc;
    if (int rc = fbn::OmcmcCheckOrders(n, orders, k)) return rc;
    if (max_families < 0) return SetError(FBN_ERR_ARG, "max_families = %lld is negative", (long long)max_families);
    if (int rc = fbn::HcCheckSamples(c->N)) return rc;
    FBN_HIP(hipSetDevice(c->device));
    const size_t ord_b = (size_t)k * n * 4, term_b = (size_t)k * n * 8, arcs_b = term_b * n;
    fbn::OmcmcLists L;
    fbn::DeviceLists D;
    fbn_exact_info xi{};
    double upload_ms = 0.0;
    if (int rc = fbn::UploadLists(c, *options, prior, bd, max_families, ord_b + term_b + arcs_b, &L, &D, &xi, &upload_ms)) return rc;
    DevBuf d_ord, d_term, d_arcs;
    int rc;
    if ((rc = d_ord.ensure(ord_b)) || (rc = d_term.ensure(term_b)) || (rc = d_arcs.ensure(arcs_b))) return rc;
    FBN_HIP(hipMemcpy(d_ord.p, orders, ord_b, hipMemcpyHostToDevice));
    const fbn::OmcmcTermsArgs a{D.ent.as<OmcmcEntry>(), D.off.as<long long>(), n, c->omcmc_group > 0 ? c->omcmc_group : kOmcmcGroupDefault,
                                d_ord.as<int32_t>(), k, d_term.as<double>(), d_arcs.as<double>()};
    const hipError_t e = fbn_omcmc_terms_launch(&a, c->stream);
    if (e != hipSuccess) return SetError(FBN_ERR_HIP, "order terms launch: %s", hipGetErrorString(e));
    FBN_HIP(hipStreamSynchronize(c->stream));
    FBN_HIP(hipMemcpy(term, d_term.p, term_b, hipMemcpyDeviceToHost));
    FBN_HIP(hipMemcpy(arcs, d_arcs.p, arcs_b, hipMemcpyDeviceToHost));
    return FBN_OK;
}

int fbn_omcmc_set_tuning(fbn_ci_ctx *c, int32_t chains_per_group, int64_t steps_per_launch) {
    if (!c) return SetError(FBN_ERR_ARG, "null pointer");
    if (chains_per_group < 0 || chains_per_group > kOmcmcGroupMax)
        return SetError(FBN_ERR_ARG, "chains_per_group = %d out of 0..%d", chains_per_group, kOmcmcGroupMax);
    if (steps_per_launch < 0) return SetError(FBN_ERR_ARG, "steps_per_launch = %lld is negative", (long long)steps_per_launch);
    c->omcmc_group = chains_per_group;
    c->omcmc_steps_per_launch = steps_per_launch;
    return FBN_OK;
}

}  // extern "C"
