// capi_gibbs.hip -- the fbn_gibbs_* section of include/fastbn.h: handles of the Gibbs sampler over the
// host twin (gibbs_host.cpp) and the launches of a device run (gibbs_kernel and its finish, gibbs.hip).
// The reference has no counterpart.
#include <hip/hip_runtime.h>

#include <vector>

#include "capi_sampler.h"
#include "gibbs_model.h"
#include "launchers.h"

using fbn::DevBuf;
using fbn::SetError;

struct fbn_gibbs : fbn::SamplerHandle {
    fbn::GibbsModel G;
    DevBuf coff, child, ws, dstates, cond_in, cond_out;  // the CSR; the units' rows; staging of states and conditionals
    int64_t lds_bytes_max = FBN_GIBBS_LDS_DEFAULT;
    int max_workgroups = 0, pc_cache = -1;
    // values [V][64] and the conditional scratch [dmax][64]: always in LDS; the accumulators and the cached
    // parent configurations join them in that order while the budget lasts
    int64_t base_bytes() const { return (int64_t)M.V * 64 + (int64_t)G.dmax * 512; }
    int64_t acc_bytes() const { return (int64_t)M.sum_dom * 8; }
    int64_t budget() const { return lds_bytes_max < 0 ? FBN_GIBBS_LDS_DEFAULT : lds_bytes_max; }
    bool lds_acc() const { return lds_bytes_max >= 0 && base_bytes() + acc_bytes() <= budget(); }
    // auto (-1): on where it fits (profiles/gibbs/gibbs_time.json holds the measurement behind the default)
    bool pc_on() const {
        return pc_cache != 0 && base_bytes() + (lds_acc() ? acc_bytes() : 0) + (int64_t)M.V * 256 <= budget();
    }
    int64_t lds_bytes() const {
        return base_bytes() + (lds_acc() ? acc_bytes() : 0) + (pc_on() ? (int64_t)M.V * 256 : 0);
    }
    int64_t grid(int64_t units) const {
        const int per_cu = (int)std::max<int64_t>(1, std::min<int64_t>(FBN_GIBBS_GROUPS_PER_CU, fbn::kCuLdsBytes / lds_bytes()));
        int64_t g = std::min<int64_t>(std::max<int64_t>(units, 1), (int64_t)std::max(num_cu, 1) * per_cu);
        if (max_workgroups > 0) g = std::min<int64_t>(g, max_workgroups);
        return g;
    }
    int Init(const fbn::Network &net, int dev) {
        int rc;
        if ((rc = fbn::BuildSamplerModel(net, M)) || (rc = fbn::BuildGibbsModel(M, G))) return rc;
        if (base_bytes() > FBN_GIBBS_LDS_DEFAULT)
            return SetError(FBN_ERR_LIMIT, "gibbs: %d variables and %d states need %lld bytes of LDS (limit %lld)", M.V, G.dmax,
                            (long long)base_bytes(), (long long)FBN_GIBBS_LDS_DEFAULT);
        if ((rc = AttachTables(dev, true)) || dev < 0) return rc;
        if ((rc = fbn::Upload(coff, G.coff))) return rc;
        return fbn::Upload(child, G.child);
    }
};

namespace {

struct RunArgs {
    int64_t ncases, chains, burn_in, sweeps, case_offset;
    uint64_t seed;
};

int GibbsDevice(fbn_gibbs *s, const RunArgs &r, const int8_t *d_ev, int32_t *d_labels, double *d_marg, int8_t *d_states,
                hipStream_t st) {
    int rc;
    if ((rc = s->OpenRun(d_ev, r.ncases, &d_marg, st))) return rc;
    fbn::PcgStream R;
    fbn::GibbsDeviceArgs a;
    s->FillArgs(a, R, r.seed, d_ev, r.ncases, r.chains, r.case_offset, d_labels, d_marg, nullptr, nullptr, nullptr, nullptr);
    a.coff = s->coff.as<int32_t>(), a.child = s->child.as<int32_t>();
    a.burn_in = r.burn_in, a.sweeps = r.sweeps;
    a.chunks = (r.chains + 63) / 64, a.units = r.ncases * a.chunks;
    a.dmax = s->G.dmax, a.pc_cache = s->pc_on() ? 1 : 0;
    if ((rc = s->ws.ensure((size_t)a.units * (size_t)s->M.sum_dom * 8))) return rc;
    a.ws = s->ws.as<double>(), a.states = d_states;
    const int64_t grid = s->grid(a.units);
    return s->Timed(st, [&] { return fbn_gibbs_launch(&a, s->lds_acc() ? 1 : 0, (size_t)s->lds_bytes(), (int)grid, st); });
}

}  // namespace

extern "C" {

int fbn_gibbs_create(const fbn_network *net, int device, fbn_gibbs **out) {
    return fbn::CreateHandle(net, out, [&](fbn_gibbs *s) { return s->Init(net->net, device); });
}

int fbn_gibbs_destroy(fbn_gibbs *s) { return fbn::DestroyHandle(s); }

int fbn_gibbs_info(const fbn_gibbs *s, int64_t ncases, int64_t chains, int64_t *lds_bytes, int *path, int *pc_cache,
                   int *grid) {
    if (!s || ncases < 0 || chains < 1) return SetError(FBN_ERR_ARG, "bad argument");
    if (lds_bytes) *lds_bytes = s->lds_bytes();
    if (path) *path = s->lds_acc() ? 0 : 1;
    if (pc_cache) *pc_cache = s->pc_on() ? 1 : 0;
    if (grid) *grid = (int)s->grid(ncases * ((chains + 63) / 64));
    return FBN_OK;
}

int fbn_gibbs_run(fbn_gibbs *s, const int8_t *evidence, int64_t ncases, int64_t chains, int64_t burn_in, int64_t sweeps,
                  uint64_t seed, int64_t case_offset, int32_t *labels, double *marginals, int8_t *states) {
    if (!s || (ncases > 0 && (!evidence || !labels))) return SetError(FBN_ERR_ARG, "bad argument");
    if (int rc = fbn::CheckGibbsShape(s->M, ncases, chains, burn_in, sweeps, case_offset)) return rc;
    if (ncases == 0) return FBN_OK;
    if (s->device < 0) {
        if (int rc = fbn::CheckEvidenceHost(s->M, evidence, ncases)) return rc;
        return fbn::HostGibbs(s->M, s->G, evidence, ncases, chains, burn_in, sweeps, seed, case_offset, labels, marginals,
                              states);
    }
    const size_t sbytes = (size_t)ncases * (size_t)chains * (size_t)s->M.V;
    int rc = s->HostBuffers(evidence, ncases, 0, 0, labels, marginals, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr,
                            [&](const int8_t *d_ev, int32_t *d_labels, double *d_marg, double *, uint8_t *, double *, int32_t *) {
                                if (states)
                                    if (int e = s->dstates.ensure(sbytes)) return e;
                                return GibbsDevice(s, RunArgs{ncases, chains, burn_in, sweeps, case_offset, seed}, d_ev, d_labels,
                                                   d_marg, states ? s->dstates.as<int8_t>() : nullptr, nullptr);
                            });
    if (rc || !states) return rc;
    FBN_HIP(hipMemcpy(states, s->dstates.p, sbytes, hipMemcpyDeviceToHost));
    return FBN_OK;
}

int fbn_gibbs_run_device(fbn_gibbs *s, const int8_t *d_evidence, int64_t ncases, int64_t chains, int64_t burn_in,
                         int64_t sweeps, uint64_t seed, int64_t case_offset, int32_t *d_labels, double *d_marginals,
                         int8_t *d_states, void *hip_stream) {
    if (!s || (ncases > 0 && (!d_evidence || !d_labels))) return SetError(FBN_ERR_ARG, "bad argument");
    if (int rc = fbn::CheckGibbsShape(s->M, ncases, chains, burn_in, sweeps, case_offset)) return rc;
    if (s->device < 0) return SetError(FBN_ERR_NODEV, "host-only handle (created with device < 0)");
    if (ncases == 0) return FBN_OK;
    FBN_HIP(hipSetDevice(s->device));
    return GibbsDevice(s, RunArgs{ncases, chains, burn_in, sweeps, case_offset, seed}, d_evidence, d_labels, d_marginals,
                       d_states, static_cast<hipStream_t>(hip_stream));
}

int fbn_gibbs_debug_conditionals(fbn_gibbs *s, const int8_t *states, int64_t n, double *out) {
    if (!s || n < 0 || (n > 0 && (!states || !out))) return SetError(FBN_ERR_ARG, "bad argument");
    if (n > FBN_SAMPLE_DEBUG_MAX / s->M.sum_dom)
        return SetError(FBN_ERR_LIMIT, "debug conditionals: more than %lld entries", (long long)FBN_SAMPLE_DEBUG_MAX);
    if (int rc = fbn::CheckGibbsStates(s->M, states, n)) return rc;
    if (n == 0) return FBN_OK;
    if (s->device < 0) return fbn::HostGibbsConditionals(s->M, s->G, states, n, out);
    FBN_HIP(hipSetDevice(s->device));
    const size_t ibytes = (size_t)n * (size_t)s->M.V, obytes = (size_t)n * (size_t)s->M.sum_dom * 8;
    int rc;
    if ((rc = s->cond_in.ensure(ibytes)) || (rc = s->cond_out.ensure(obytes))) return rc;
    FBN_HIP(hipMemcpy(s->cond_in.p, states, ibytes, hipMemcpyHostToDevice));
    fbn::GibbsCondArgs a;
    a.M = s->View();
    a.coff = s->coff.as<int32_t>(), a.child = s->child.as<int32_t>();
    a.states = s->cond_in.as<int8_t>(), a.n = n;
    a.dmax = s->G.dmax, a.pc_cache = s->pc_on() ? 1 : 0;
    a.out = s->cond_out.as<double>();
    FBN_HIP(fbn_gibbs_cond_launch(&a, (size_t)(s->base_bytes() + (a.pc_cache ? (int64_t)s->M.V * 256 : 0)), nullptr));
    FBN_HIP(hipMemcpy(out, s->cond_out.p, obytes, hipMemcpyDeviceToHost));
    return FBN_OK;
}

int fbn_gibbs_set_tuning(fbn_gibbs *s, int64_t lds_bytes_max, int max_workgroups, int pc_cache) {
    if (!s || max_workgroups < 0 || pc_cache < -1 || pc_cache > 1) return SetError(FBN_ERR_ARG, "bad argument");
    if (lds_bytes_max > FBN_GIBBS_LDS_DEFAULT)
        return SetError(FBN_ERR_ARG, "lds_bytes_max %lld beyond %lld", (long long)lds_bytes_max,
                        (long long)FBN_GIBBS_LDS_DEFAULT);
    s->lds_bytes_max = lds_bytes_max == 0 ? FBN_GIBBS_LDS_DEFAULT : lds_bytes_max;
    s->max_workgroups = max_workgroups;
    s->pc_cache = pc_cache;
    return FBN_OK;
}

int fbn_gibbs_last_kernel_ms(const fbn_gibbs *s, float *ms) {
    if (!s) return SetError(FBN_ERR_ARG, "no timed launch");
    return s->LastKernelMs(ms);
}

}  // extern "C"
