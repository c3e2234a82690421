// capi_mpe.hip -- the fbn_mpe_* section of include/fastbn.h: most-probable-explanation handles over
// the forest plan (jt_plan.cpp), the max-product program (jt_mpe_plan.cpp), the host twin
// (jt_mpe_host.cpp) and the kernel (jt_mpe.hip).  MPE has no counterpart in the reference.
#include <hip/hip_runtime.h>

#include <vector>

#include "fbn_device.h"
#include "fbn_internal.h"
#include "jt_mpe_program.h"
#include "launchers.h"

using fbn::DevBuf;
using fbn::SetError;
using fbn::Upload;

// the store budget of a handle (all waves together) unless fbn_mpe_set_tuning says otherwise
static constexpr int64_t kMpeStoreDefault = (int64_t)32 << 30;
// persistent one-wave workgroups per CU (two per SIMD: a wave's loads are dependent on one another)
static constexpr int kMpeWavesPerCu = 8;
// most doubles fbn_mpe_debug_messages returns
static constexpr int64_t kMpeDebugMax = (int64_t)1 << 26;

struct fbn_mpe : fbn::DeviceHandle {
    fbn::JTProgramMpe P;
    int64_t store_bytes_max = kMpeStoreDefault;
    int max_workgroups = 0;
    DevBuf cl, aux, initv, dig, collect, trace, store;
    DevBuf evid, assign, value, dmsg, dexp;  // staging of the host-buffer entries
    int64_t wave_bytes() const { return P.store_rows * 64 * 8; }
};

namespace {

int CheckBudget(const fbn_mpe *s, int64_t budget) {
    if (s->wave_bytes() > budget)
        return SetError(FBN_ERR_LIMIT, "one wave's store takes %lld bytes (%lld rows), the budget is %lld",
                        (long long)s->wave_bytes(), (long long)s->P.store_rows, (long long)budget);
    return FBN_OK;
}

int MpeDevice(fbn_mpe *s, const int8_t *d_ev, int64_t ncases, int8_t *d_assign, double *d_value, double *d_msg,
              int32_t *d_exp, hipStream_t st) {
    s->Note(st);
    // as fbn_jt_run_device's check: on the device, before anything indexes with a code; one stream sync
    if (int rc = s->evidence.Run(d_ev, ncases, st)) return rc;
    int64_t grid = std::min<int64_t>((ncases + 63) / 64, (int64_t)s->num_cu * kMpeWavesPerCu);
    grid = std::min<int64_t>(grid, s->store_bytes_max / s->wave_bytes());
    // never more than half of the free device memory (beside what the handle holds already)
    grid = fbn::ClampGridToFreeMemory(grid, (size_t)s->wave_bytes(), s->store.bytes, fbn::kMemShareHalf);
    if (s->max_workgroups > 0) grid = std::min<int64_t>(grid, s->max_workgroups);
    grid = std::max<int64_t>(grid, 1);
    if (int rc = s->store.ensure((size_t)grid * (size_t)s->wave_bytes())) return rc;
    JtMpeArgs a;
    a.cl = s->cl.as<JtMClique>(), a.aux = s->aux.as<int32_t>(), a.initv = s->initv.as<double>();
    a.dig = s->dig.as<uint64_t>(), a.collect = s->collect.as<int32_t>(), a.trace = s->trace.as<int32_t>();
    a.evid = d_ev, a.assign = d_assign, a.value = d_value, a.dbg_msg = d_msg, a.dbg_exp = d_exp;
    a.store = s->store.as<double>();
    a.ncases = ncases, a.store_rows = s->P.store_rows;
    a.nc = (int)s->P.cl.size(), a.V = s->P.V, a.msg_rows = (int)s->P.msg_rows, a.nsep = s->P.nsep;
    a.grid = (int)grid;
    return s->Timed(st, [&] { return fbn_mpe_launch(&a, st); });
}

int MpeHostBuffers(fbn_mpe *s, const int8_t *evidence, int64_t ncases, int8_t *assignment, double *value,
                   double *messages, int32_t *exponents) {
    if (ncases == 0) return FBN_OK;
    const int V = s->P.V;
    if (s->device < 0) {
        if (int rc = fbn::CheckMpeEvidence(s->P, evidence, ncases)) return rc;
        if (int rc = fbn::HostMpe(s->P, evidence, ncases, assignment, value, messages, exponents)) return rc;
        return fbn::CheckCaseValues("mpe", value, ncases);
    }
    FBN_HIP(hipSetDevice(s->device));
    const size_t mbytes = (size_t)ncases * (size_t)std::max<int64_t>(s->P.msg_rows, 1) * 8;
    const size_t ebytes = (size_t)ncases * (size_t)std::max(s->P.nsep, 1) * 4;
    int rc;
    if ((rc = s->evid.ensure((size_t)ncases * V)) || (rc = s->assign.ensure((size_t)ncases * V)) ||
        (rc = s->value.ensure((size_t)ncases * 16)) || (messages && (rc = s->dmsg.ensure(mbytes))) ||
        (exponents && (rc = s->dexp.ensure(ebytes))))
        return rc;
    FBN_HIP(hipMemcpy(s->evid.p, evidence, (size_t)ncases * V, hipMemcpyHostToDevice));
    rc = MpeDevice(s, s->evid.as<int8_t>(), ncases, s->assign.as<int8_t>(), s->value.as<double>(),
                   messages ? s->dmsg.as<double>() : nullptr, exponents ? s->dexp.as<int32_t>() : nullptr, nullptr);
    if (rc) return rc;
    FBN_HIP(hipMemcpy(assignment, s->assign.p, (size_t)ncases * V, hipMemcpyDeviceToHost));
    FBN_HIP(hipMemcpy(value, s->value.p, (size_t)ncases * 16, hipMemcpyDeviceToHost));
    if (messages && s->P.msg_rows > 0)
        FBN_HIP(hipMemcpy(messages, s->dmsg.p, (size_t)ncases * s->P.msg_rows * 8, hipMemcpyDeviceToHost));
    if (exponents && s->P.nsep > 0)
        FBN_HIP(hipMemcpy(exponents, s->dexp.p, (size_t)ncases * s->P.nsep * 4, hipMemcpyDeviceToHost));
    return fbn::CheckCaseValues("mpe", value, ncases);
}

}  // namespace

extern "C" {

int fbn_mpe_create(const fbn_network *net, int device, fbn_mpe **out) {
    if (!net || !out) return SetError(FBN_ERR_ARG, "null pointer");
    *out = nullptr;
    if ((int)fbn::TopoOrder(net->net).size() != net->net.n()) return SetError(FBN_ERR_ARG, "network has a cycle");
    return fbn::CreateHandle(net, out, [&](fbn_mpe *s) -> int {
        fbn::JTPlanHost plan;
        int r;
        if ((r = fbn::BuildJTPlan(net->net, plan, /*forest=*/true)) || (r = fbn::CompileJTProgramMpe(plan, s->P)) ||
            (r = CheckBudget(s, s->store_bytes_max)) || device < 0)
            return r;
        if ((r = s->Attach(device)) || (r = Upload(s->cl, s->P.cl)) || (r = Upload(s->aux, s->P.aux)) ||
            (r = Upload(s->initv, s->P.initv)) || (r = Upload(s->dig, s->P.dig)) ||
            (r = Upload(s->collect, s->P.collect)) || (r = Upload(s->trace, s->P.trace)))
            return r;
        return s->evidence.Attach(s->P.dom);
    });
}

int fbn_mpe_destroy(fbn_mpe *s) { return fbn::DestroyHandle(s); }

int fbn_mpe_info(const fbn_mpe *s, int64_t *cliques, int64_t *entries, int64_t *store_rows, int *components) {
    if (!s) return SetError(FBN_ERR_ARG, "null pointer");
    if (cliques) *cliques = (int64_t)s->P.cl.size();
    if (entries) *entries = s->P.entries;
    if (store_rows) *store_rows = s->P.store_rows;
    if (components) *components = s->P.components;
    return FBN_OK;
}

int fbn_mpe_run(fbn_mpe *s, const int8_t *evidence, int64_t ncases, int8_t *assignment, double *value) {
    if (!s || ncases < 0 || (ncases > 0 && (!evidence || !assignment || !value)))
        return SetError(FBN_ERR_ARG, "bad argument");
    return MpeHostBuffers(s, evidence, ncases, assignment, value, nullptr, nullptr);
}

int fbn_mpe_run_device(fbn_mpe *s, const int8_t *d_evidence, int64_t ncases, int8_t *d_assignment, double *d_value,
                       void *hip_stream) {
    if (!s || ncases < 0 || (ncases > 0 && (!d_evidence || !d_assignment || !d_value)))
        return SetError(FBN_ERR_ARG, "bad argument");
    if (s->device < 0) return SetError(FBN_ERR_NODEV, "host-only handle (created with device < 0)");
    if (ncases == 0) return FBN_OK;
    FBN_HIP(hipSetDevice(s->device));
    return MpeDevice(s, d_evidence, ncases, d_assignment, d_value, nullptr, nullptr, static_cast<hipStream_t>(hip_stream));
}

int fbn_mpe_debug_messages(fbn_mpe *s, const int8_t *evidence, int64_t ncases, double *messages, int32_t *exponents) {
    if (!s || ncases < 0 || (ncases > 0 && (!evidence || !messages || !exponents)))
        return SetError(FBN_ERR_ARG, "bad argument");
    if (ncases > 0 && ncases > kMpeDebugMax / std::max<int64_t>(s->P.msg_rows, 1))
        return SetError(FBN_ERR_LIMIT, "debug messages: more than %lld doubles", (long long)kMpeDebugMax);
    std::vector<int8_t> assign((size_t)std::max<int64_t>(ncases * s->P.V, 1));
    std::vector<double> value((size_t)std::max<int64_t>(ncases * 2, 1));
    return MpeHostBuffers(s, evidence, ncases, assign.data(), value.data(), messages, exponents);
}

int fbn_mpe_set_tuning(fbn_mpe *s, int max_workgroups, int64_t store_bytes_max) {
    if (!s || max_workgroups < 0 || store_bytes_max < 0) return SetError(FBN_ERR_ARG, "bad argument");
    const int64_t budget = store_bytes_max == 0 ? kMpeStoreDefault : store_bytes_max;
    if (int rc = CheckBudget(s, budget)) return rc;
    s->store_bytes_max = budget;
    s->max_workgroups = max_workgroups;
    return FBN_OK;
}

int fbn_mpe_last_kernel_ms(const fbn_mpe *s, float *ms) {
    if (!s) return SetError(FBN_ERR_ARG, "no timed launch");
    return s->LastKernelMs(ms);
}

}  // extern "C"
