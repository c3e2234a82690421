// capi_em.hip -- the fbn_em_* section of include/fastbn.h: expectation-maximisation handles over the
// forest plan (jt_plan.cpp), the EM program (jt_em_plan.cpp), the host twin (jt_em_host.cpp) and the
// kernels (jt_em.hip).  EM has no counterpart in the reference (its parameter learning assumes
// complete data).
#include <hip/hip_runtime.h>

#include <cmath>
#include <memory>
#include <new>
#include <vector>

#include "fbn_device.h"
#include "fbn_internal.h"
#include "jt_em_program.h"
#include "launchers.h"

using fbn::DevBuf;
using fbn::SetError;
using fbn::Upload;

// the store budget of a handle (all waves together) unless fbn_em_set_tuning says otherwise
static constexpr int64_t kEmStoreDefault = (int64_t)32 << 30;
// persistent one-wave workgroups per CU, as the max-product kernel's
static constexpr int64_t kEmWavesPerCu = 8;
// most doubles fbn_em_debug_posteriors returns
static constexpr int64_t kEmDebugMax = (int64_t)1 << 26;

struct fbn_em : fbn::DeviceHandle {
    fbn::Network structure;  // the start network: states, parent lists, names
    fbn::JTProgramEm P;      // P.theta and P.M.initv are the current parameters
    int64_t store_bytes_max = kEmStoreDefault;
    int max_workgroups = 0;
    DevBuf cl, ecl, aux, eaux, initv, dig, collect, trace, store, wacc;
    DevBuf cell_node, node_rec, entry_clique, theta, counts;
    DevBuf data, value, post;  // staging of the host-buffer entries
    // one wave's state: its store and its accumulator
    int64_t wave_bytes() const { return P.store_rows * 64 * 8 + P.cells * 8; }
    // the accumulator in LDS while it fits the workgroup's share of the CU's LDS
    bool lds_acc() const { return P.cells * 8 <= fbn::kCuLdsBytes / kEmWavesPerCu; }
};

namespace {

int CheckBudget(const fbn_em *s, int64_t budget) {
    if (s->wave_bytes() > budget)
        return SetError(FBN_ERR_LIMIT, "one wave's state takes %lld bytes (%lld rows, %lld cells), the budget is %lld",
                        (long long)s->wave_bytes(), (long long)s->P.store_rows, (long long)s->P.cells, (long long)budget);
    return FBN_OK;
}

// the E-step kernel (timed) and, with d_counts, the reduction of the waves' accumulators
int EstepDevice(fbn_em *s, const int8_t *d_data, int64_t ncases, double *d_counts, double *d_value, double *d_post,
                bool check, hipStream_t st) {
    s->Note(st);
    if (check)
        if (int rc = s->evidence.Run(d_data, ncases, st)) return rc;
    int64_t grid = std::min<int64_t>((ncases + 63) / 64, (int64_t)s->num_cu * kEmWavesPerCu);
    grid = std::min<int64_t>(grid, s->store_bytes_max / s->wave_bytes());
    grid = fbn::ClampGridToFreeMemory(grid, (size_t)s->wave_bytes(), s->store.bytes + s->wacc.bytes, fbn::kMemShareHalf);
    if (s->max_workgroups > 0) grid = std::min<int64_t>(grid, s->max_workgroups);
    grid = std::max<int64_t>(grid, 1);
    const size_t acc_bytes = (size_t)grid * (size_t)s->P.cells * 8;
    int rc;
    if ((rc = s->store.ensure((size_t)grid * (size_t)s->P.store_rows * 512)) || (rc = s->wacc.ensure(acc_bytes))) return rc;
    FBN_HIP(hipMemsetAsync(s->wacc.p, 0, acc_bytes, st));
    const fbn::JTProgramMpe &M = s->P.M;
    JtEmArgs a;
    a.cl = s->cl.as<JtMClique>(), a.ecl = s->ecl.as<JtEClique>();
    a.aux = s->aux.as<int32_t>(), a.eaux = s->eaux.as<int32_t>();
    a.initv = s->initv.as<double>(), a.dig = s->dig.as<uint64_t>();
    a.collect = s->collect.as<int32_t>(), a.trace = s->trace.as<int32_t>();
    a.data = d_data, a.value = d_value, a.dbg_post = d_post, a.store = s->store.as<double>();
    a.wacc = s->wacc.as<double>(), a.lds_acc = s->lds_acc();
    a.ncases = ncases, a.store_rows = s->P.store_rows;
    a.nc = (int)M.cl.size(), a.V = M.V, a.msg_rows = (int)M.msg_rows, a.nsep = M.nsep, a.cells = (int)s->P.cells;
    a.grid = (int)grid;
    if ((rc = s->Timed(st, [&] { return fbn_em_estep_launch(&a, st); }))) return rc;
    if (d_counts) {
        JtEmReduceArgs r;
        r.wacc = s->wacc.as<double>(), r.counts = d_counts, r.cells = (int)s->P.cells, r.grid = (int)grid;
        FBN_HIP(fbn_em_reduce_launch(&r, st));
    }
    return FBN_OK;
}

int UploadParameters(fbn_em *s) {
    if (s->device < 0) return FBN_OK;
    FBN_HIP(hipSetDevice(s->device));
    s->Drain();
    if (int rc = Upload(s->theta, s->P.theta)) return rc;
    return Upload(s->initv, s->P.M.initv);
}

// a row with m == 0 has NaN posteriors: an error, never a result (jt_mpe_program.h: CheckCaseValues)
int CheckValues(const double *value, int64_t ncases) { return fbn::CheckCaseValues("em", value, ncases); }

int EstepHostBuffers(fbn_em *s, const int8_t *data, int64_t ncases, double *counts, double *value, double *post) {
    const int64_t cells = s->P.cells;
    if (ncases == 0) {
        if (counts) std::fill(counts, counts + cells, 0.0);
        return FBN_OK;
    }
    std::vector<double> vbuf;
    if (!value) vbuf.resize((size_t)ncases * 2), value = vbuf.data();
    if (s->device < 0) {
        if (int rc = fbn::CheckMpeEvidence(s->P.M, data, ncases)) return rc;
        if (int rc = fbn::HostEmEstep(s->P, data, ncases, counts, value, post)) return rc;
        return CheckValues(value, ncases);
    }
    FBN_HIP(hipSetDevice(s->device));
    const int V = s->P.M.V;
    int rc;
    if ((rc = s->data.ensure((size_t)ncases * V)) || (rc = s->value.ensure((size_t)ncases * 16)) ||
        (rc = s->counts.ensure((size_t)cells * 8)) || (post && (rc = s->post.ensure((size_t)ncases * cells * 8))))
        return rc;
    FBN_HIP(hipMemcpy(s->data.p, data, (size_t)ncases * V, hipMemcpyHostToDevice));
    rc = EstepDevice(s, s->data.as<int8_t>(), ncases, s->counts.as<double>(), s->value.as<double>(),
                     post ? s->post.as<double>() : nullptr, true, nullptr);
    if (rc) return rc;
    if (counts) FBN_HIP(hipMemcpy(counts, s->counts.p, (size_t)cells * 8, hipMemcpyDeviceToHost));
    FBN_HIP(hipMemcpy(value, s->value.p, (size_t)ncases * 16, hipMemcpyDeviceToHost));
    if (post) FBN_HIP(hipMemcpy(post, s->post.p, (size_t)ncases * cells * 8, hipMemcpyDeviceToHost));
    FBN_HIP(hipDeviceSynchronize());
    return CheckValues(value, ncases);
}

// {L, Q} at theta from the per-case values: the logs on the host, in case order and in cell order
void Objective(const double *value, int64_t ncases, const std::vector<double> &theta, double alpha, double *out) {
    double ll = 0.0, pen = 0.0;
    for (int64_t c = 0; c < ncases; ++c) ll = ll + (std::log(value[2 * c]) + value[2 * c + 1] * std::log(2.0));
    for (double t : theta) pen = pen + std::log(t);
    out[0] = ll, out[1] = ll + alpha * pen;
}

}  // namespace

extern "C" {

int fbn_em_create(const fbn_network *start, int device, fbn_em **out) {
    if (!start || !out) return SetError(FBN_ERR_ARG, "null pointer");
    *out = nullptr;
    if ((int)fbn::TopoOrder(start->net).size() != start->net.n()) return SetError(FBN_ERR_ARG, "network has a cycle");
    return fbn::CreateHandle(start, out, [&](fbn_em *s) -> int {
        s->structure = start->net;
        fbn::JTPlanHost plan;
        int r;
        if ((r = fbn::BuildJTPlan(start->net, plan, /*forest=*/true)) ||
            (r = fbn::CompileJTProgramEm(start->net, plan, s->P)) || (r = CheckBudget(s, s->store_bytes_max)) || device < 0)
            return r;
        const fbn::JTProgramMpe &M = s->P.M;
        if ((r = s->Attach(device)) || (r = Upload(s->cl, M.cl)) || (r = Upload(s->ecl, s->P.ecl)) ||
            (r = Upload(s->aux, M.aux)) || (r = Upload(s->eaux, s->P.eaux)) || (r = Upload(s->initv, M.initv)) ||
            (r = Upload(s->dig, M.dig)) || (r = Upload(s->collect, M.collect)) || (r = Upload(s->trace, M.trace)) ||
            (r = Upload(s->cell_node, s->P.cell_node)) || (r = Upload(s->node_rec, s->P.node_rec)) ||
            (r = Upload(s->entry_clique, s->P.entry_clique)) || (r = Upload(s->theta, s->P.theta)))
            return r;
        return s->evidence.Attach(M.dom);
    });
}

int fbn_em_destroy(fbn_em *s) { return fbn::DestroyHandle(s); }

int fbn_em_info(const fbn_em *s, int64_t *cliques, int64_t *entries, int64_t *store_rows, int64_t *cells, int *components) {
    if (!s) return SetError(FBN_ERR_ARG, "null pointer");
    if (cliques) *cliques = (int64_t)s->P.M.cl.size();
    if (entries) *entries = s->P.M.entries;
    if (store_rows) *store_rows = s->P.store_rows;
    if (cells) *cells = s->P.cells;
    if (components) *components = s->P.M.components;
    return FBN_OK;
}

int fbn_em_estep(fbn_em *s, const int8_t *data, int64_t ncases, double *counts, double *value) {
    if (!s || ncases < 0 || !counts || (ncases > 0 && !data)) return SetError(FBN_ERR_ARG, "bad argument");
    return EstepHostBuffers(s, data, ncases, counts, value, nullptr);
}

int fbn_em_estep_device(fbn_em *s, const int8_t *d_data, int64_t ncases, double *d_counts, double *d_value,
                        void *hip_stream) {
    if (!s || ncases < 0 || !d_counts || (ncases > 0 && !d_data)) return SetError(FBN_ERR_ARG, "bad argument");
    if (s->device < 0) return SetError(FBN_ERR_NODEV, "host-only handle (created with device < 0)");
    FBN_HIP(hipSetDevice(s->device));
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (ncases == 0) {
        FBN_HIP(hipMemsetAsync(d_counts, 0, (size_t)s->P.cells * 8, st));
        return FBN_OK;
    }
    return EstepDevice(s, d_data, ncases, d_counts, d_value, nullptr, true, st);
}

int fbn_em_run(fbn_em *s, const int8_t *data, int64_t ncases, int max_iters, double tol, double pseudo_count,
               double *objective, int *iters_done) {
    if (!s || ncases < 0 || (ncases > 0 && !data) || !objective) return SetError(FBN_ERR_ARG, "bad argument");
    if (!(pseudo_count > 0.0) || !std::isfinite(pseudo_count))
        return SetError(FBN_ERR_ARG, "em: the pseudo-count must be > 0 (got %g)", pseudo_count);
    if (max_iters < 1 || !(tol >= 0.0)) return SetError(FBN_ERR_ARG, "em: max_iters %d, tol %g", max_iters, tol);
    if (iters_done) *iters_done = 0;
    const int64_t cells = s->P.cells;
    const int V = s->P.M.V;
    std::vector<double> value((size_t)std::max<int64_t>(2 * ncases, 1)), counts((size_t)cells);
    const bool dev = s->device >= 0;
    int rc;
    if (dev) {
        FBN_HIP(hipSetDevice(s->device));
        if ((rc = s->data.ensure((size_t)std::max<int64_t>(ncases * V, 1))) ||
            (rc = s->value.ensure((size_t)std::max<int64_t>(ncases * 16, 16))) || (rc = s->counts.ensure((size_t)cells * 8)))
            return rc;
        if (ncases > 0) FBN_HIP(hipMemcpy(s->data.p, data, (size_t)ncases * V, hipMemcpyHostToDevice));
    } else if ((rc = fbn::CheckMpeEvidence(s->P.M, data, ncases))) {
        return rc;
    }
    std::vector<double> prev;
    for (int t = 0; t < max_iters; ++t) {
        if (!dev) {
            if ((rc = fbn::HostEmEstep(s->P, data, ncases, counts.data(), value.data(), nullptr))) return rc;
        } else if (ncases > 0) {
            if ((rc = EstepDevice(s, s->data.as<int8_t>(), ncases, s->counts.as<double>(), s->value.as<double>(), nullptr,
                                  /*check=*/t == 0, nullptr)))
                return rc;
            FBN_HIP(hipMemcpy(value.data(), s->value.p, (size_t)ncases * 16, hipMemcpyDeviceToHost));
        } else {
            FBN_HIP(hipMemset(s->counts.p, 0, (size_t)cells * 8));
        }
        if ((rc = CheckValues(value.data(), ncases))) return rc;  // theta is still the last one accepted
        Objective(value.data(), ncases, s->P.theta, pseudo_count, objective + 2 * t);
        prev = s->P.theta;
        if (!dev) {
            fbn::EmMstep(s->P, counts.data(), pseudo_count, s->P.theta.data());
        } else {
            JtEmMstepArgs m;
            m.counts = s->counts.as<double>(), m.theta = s->theta.as<double>(), m.initv = s->initv.as<double>();
            m.cell_node = s->cell_node.as<int32_t>(), m.node_rec = s->node_rec.as<int32_t>();
            m.entry_clique = s->entry_clique.as<int32_t>();
            m.cl = s->cl.as<JtMClique>(), m.ecl = s->ecl.as<JtEClique>(), m.eaux = s->eaux.as<int32_t>();
            m.alpha = pseudo_count, m.cells = (int)cells, m.entries = (int)s->P.M.entries;
            FBN_HIP(fbn_em_mstep_launch(&m, nullptr));
            FBN_HIP(hipMemcpy(s->P.theta.data(), s->theta.p, (size_t)cells * 8, hipMemcpyDeviceToHost));
        }
        // the host copy of the potentials follows theta (the device's own come from the M-step kernel, the
        // same products); a theta they underflow under is refused and the handle goes back one M-step
        fbn::EmRebuildPotentials(s->P, s->P.theta.data(), s->P.M.initv.data());
        if ((rc = fbn::EmCheckPotentials(s->P, s->P.M.initv.data()))) {
            s->P.theta.swap(prev);
            fbn::EmRebuildPotentials(s->P, s->P.theta.data(), s->P.M.initv.data());
            if (int up = UploadParameters(s)) return up;
            return rc;
        }
        if (iters_done) *iters_done = t + 1;
        if (t >= 1 && objective[2 * t + 1] - objective[2 * t - 1] <= tol * std::fabs(objective[2 * t + 1])) break;
    }
    return FBN_OK;
}

int fbn_em_set_parameters(fbn_em *s, const fbn_network *net) {
    if (!s || !net) return SetError(FBN_ERR_ARG, "null pointer");
    std::vector<double> theta;
    if (int rc = fbn::EmThetaFromNetwork(s->P, s->structure, net->net, theta)) return rc;
    std::vector<double> initv(s->P.M.initv.size());
    fbn::EmRebuildPotentials(s->P, theta.data(), initv.data());
    if (int rc = fbn::EmCheckPotentials(s->P, initv.data())) return rc;  // the handle keeps its parameters
    s->P.theta.swap(theta);
    s->P.M.initv.swap(initv);
    return UploadParameters(s);
}

int fbn_em_network(const fbn_em *s, fbn_network **out) {
    if (!s || !out) return SetError(FBN_ERR_ARG, "null pointer");
    *out = nullptr;
    const fbn::Network &st = s->structure;
    std::vector<int32_t> dims(st.dom.begin(), st.dom.end()), off(1, 0), par;
    std::vector<const char *> names;
    for (int v = 0; v < st.n(); ++v) {
        par.insert(par.end(), st.given[v].begin(), st.given[v].end());
        off.push_back((int32_t)par.size());
        names.push_back(st.names[v].c_str());
    }
    par.push_back(0);
    auto h = std::unique_ptr<fbn_network>(new (std::nothrow) fbn_network());
    if (!h) return SetError(FBN_ERR_NOMEM, "out of memory");
    if (int rc = fbn::BuildNetworkCpt(st.n(), dims.data(), off.data(), par.data(), s->P.theta.data(), names.data(), h->net))
        return rc;
    *out = h.release();
    return FBN_OK;
}

int fbn_em_debug_posteriors(fbn_em *s, const int8_t *data, int64_t ncases, double *post) {
    if (!s || ncases < 0 || (ncases > 0 && (!data || !post))) return SetError(FBN_ERR_ARG, "bad argument");
    if (ncases > 0 && ncases > kEmDebugMax / std::max<int64_t>(s->P.cells, 1))
        return SetError(FBN_ERR_LIMIT, "debug posteriors: more than %lld doubles", (long long)kEmDebugMax);
    if (ncases == 0) return FBN_OK;
    return EstepHostBuffers(s, data, ncases, nullptr, nullptr, post);
}

int fbn_em_set_tuning(fbn_em *s, int max_workgroups, int64_t store_bytes_max) {
    if (!s || max_workgroups < 0 || store_bytes_max < 0) return SetError(FBN_ERR_ARG, "bad argument");
    const int64_t budget = store_bytes_max == 0 ? kEmStoreDefault : store_bytes_max;
    if (int rc = CheckBudget(s, budget)) return rc;
    s->store_bytes_max = budget;
    s->max_workgroups = max_workgroups;
    return FBN_OK;
}

int fbn_em_last_kernel_ms(const fbn_em *s, float *ms) {
    if (!s) return SetError(FBN_ERR_ARG, "no timed launch");
    return s->LastKernelMs(ms);
}

}  // extern "C"
