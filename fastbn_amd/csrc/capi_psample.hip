// capi_psample.hip -- the fbn_psample_* section of include/fastbn.h: exact posterior-sampling handles
// over the forest plan (jt_plan.cpp), the max-product program's tables (jt_mpe_plan.cpp), the host twin
// (jt_psample_host.cpp) and the kernel (jt_psample.hip).  Posterior sampling has no counterpart in the
// reference.
#include <hip/hip_runtime.h>

#include <vector>

#include "fbn_device.h"
#include "fbn_internal.h"
#include "jt_psample_program.h"
#include "launchers.h"

using fbn::DevBuf;
using fbn::SetError;
using fbn::Upload;

// the store budget of a handle (all waves together) unless fbn_psample_set_tuning says otherwise
static constexpr int64_t kPsampleStoreDefault = (int64_t)32 << 30;
// persistent one-wave workgroups per CU (two per SIMD: a wave's loads are dependent on one another)
static constexpr int kPsampleWavesPerCu = 8;

struct fbn_psample : fbn::DeviceHandle {
    fbn::JTProgramMpe P;
    int64_t store_bytes_max = kPsampleStoreDefault;
    int64_t sample_chunk = 0;  // 0: chosen per run
    int max_workgroups = 0;
    DevBuf cl, aux, initv, dig, collect, trace, store;
    DevBuf evid, samples, value;  // staging of the host-buffer entry
    int64_t store_rows() const { return P.msg_rows + P.nsep + (int64_t)kPsampleU * (int64_t)P.cl.size(); }
    int64_t wave_bytes() const { return store_rows() * 64 * 8; }
};

namespace {

int CheckBudget(const fbn_psample *s, int64_t budget) {
    if (s->wave_bytes() > budget)
        return SetError(FBN_ERR_LIMIT, "one wave's store takes %lld bytes (%lld rows), the budget is %lld",
                        (long long)s->wave_bytes(), (long long)s->store_rows(), (long long)budget);
    return FBN_OK;
}

// Samples per unit.  The blocks alone fill the grid: one chunk.  Else the largest chunk that still yields
// one unit per resident wave (each further chunk repeats the block's Collect).
int64_t PickChunk(int64_t nblocks, int64_t S, int64_t resident) {
    if (nblocks >= resident) return S;
    const int64_t need = (resident + nblocks - 1) / nblocks;  // chunks per block, >= 2
    return std::max<int64_t>(1, (S - 1) / (need - 1));
}

int PsampleDevice(fbn_psample *s, const int8_t *d_ev, int64_t ncases, int64_t S, uint64_t seed, int64_t case_offset,
                  int8_t *d_samples, double *d_value, hipStream_t st) {
    s->Note(st);
    // as fbn_jt_run_device's check: on the device, before anything indexes with a code; one stream sync
    if (int rc = s->evidence.Run(d_ev, ncases, st)) return rc;
    const int64_t nblocks = (ncases + 63) / 64, resident = (int64_t)s->num_cu * kPsampleWavesPerCu;
    int64_t chunk = s->sample_chunk > 0 ? std::min(s->sample_chunk, S) : PickChunk(nblocks, S, resident);
    int64_t grid = std::min<int64_t>(nblocks * ((S + chunk - 1) / chunk), resident);
    grid = std::min<int64_t>(grid, s->store_bytes_max / s->wave_bytes());
    // never more than half of the free device memory (beside what the handle holds already)
    grid = fbn::ClampGridToFreeMemory(grid, (size_t)s->wave_bytes(), s->store.bytes, fbn::kMemShareHalf);
    if (s->max_workgroups > 0) grid = std::min<int64_t>(grid, s->max_workgroups);
    grid = std::max<int64_t>(grid, 1);
    if (int rc = s->store.ensure((size_t)grid * (size_t)s->wave_bytes())) return rc;
    JtPsampleArgs a;
    a.cl = s->cl.as<JtMClique>(), a.aux = s->aux.as<int32_t>(), a.initv = s->initv.as<double>();
    a.dig = s->dig.as<uint64_t>(), a.collect = s->collect.as<int32_t>(), a.trace = s->trace.as<int32_t>();
    a.evid = d_ev, a.samples = d_samples, a.value = d_value;
    a.store = s->store.as<double>();
    a.ncases = ncases, a.S = S, a.case0 = case_offset, a.chunk = chunk, a.store_rows = s->store_rows();
    a.nc = (int)s->P.cl.size(), a.V = s->P.V, a.msg_rows = (int)s->P.msg_rows, a.nsep = s->P.nsep;
    a.grid = (int)grid;
    fbn::PcgStream R;
    fbn::PcgStreamInit(seed, R);
    a.state = R.state, a.inc = R.inc;
    std::copy(R.jump, R.jump + 256, a.jump);
    return s->Timed(st, [&] { return fbn_psample_launch(&a, st); });
}

}  // namespace

extern "C" {

int fbn_psample_create(const fbn_network *net, int device, fbn_psample **out) {
    if (!net || !out) return SetError(FBN_ERR_ARG, "null pointer");
    *out = nullptr;
    if ((int)fbn::TopoOrder(net->net).size() != net->net.n()) return SetError(FBN_ERR_ARG, "network has a cycle");
    return fbn::CreateHandle(net, out, [&](fbn_psample *s) -> int {
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

int fbn_psample_destroy(fbn_psample *s) { return fbn::DestroyHandle(s); }

int fbn_psample_info(const fbn_psample *s, int64_t *cliques, int64_t *entries, int64_t *store_rows, int *components) {
    if (!s) return SetError(FBN_ERR_ARG, "null pointer");
    if (cliques) *cliques = (int64_t)s->P.cl.size();
    if (entries) *entries = s->P.entries;
    if (store_rows) *store_rows = s->store_rows();
    if (components) *components = s->P.components;
    return FBN_OK;
}

int fbn_psample_run(fbn_psample *s, const int8_t *evidence, int64_t ncases, int64_t nsamples, uint64_t seed,
                    int64_t case_offset, int8_t *samples, double *value) {
    if (!s || (ncases > 0 && (!evidence || !samples || !value))) return SetError(FBN_ERR_ARG, "bad argument");
    if (int rc = fbn::CheckPsampleShape(s->P, ncases, nsamples, case_offset)) return rc;
    if (ncases == 0) return FBN_OK;
    const size_t ebytes = (size_t)ncases * s->P.V, sbytes = ebytes * (size_t)nsamples;
    if (s->device < 0) {
        if (int rc = fbn::CheckMpeEvidence(s->P, evidence, ncases)) return rc;
        if (int rc = fbn::HostPsample(s->P, evidence, ncases, nsamples, seed, case_offset, samples, value)) return rc;
        return fbn::CheckCaseValues("psample", value, ncases);
    }
    FBN_HIP(hipSetDevice(s->device));
    int rc;
    if ((rc = s->evid.ensure(ebytes)) || (rc = s->samples.ensure(sbytes)) || (rc = s->value.ensure((size_t)ncases * 16)))
        return rc;
    FBN_HIP(hipMemcpy(s->evid.p, evidence, ebytes, hipMemcpyHostToDevice));
    rc = PsampleDevice(s, s->evid.as<int8_t>(), ncases, nsamples, seed, case_offset, s->samples.as<int8_t>(),
                       s->value.as<double>(), nullptr);
    if (rc) return rc;
    FBN_HIP(hipMemcpy(samples, s->samples.p, sbytes, hipMemcpyDeviceToHost));
    FBN_HIP(hipMemcpy(value, s->value.p, (size_t)ncases * 16, hipMemcpyDeviceToHost));
    return fbn::CheckCaseValues("psample", value, ncases);
}

int fbn_psample_run_device(fbn_psample *s, const int8_t *d_evidence, int64_t ncases, int64_t nsamples, uint64_t seed,
                           int64_t case_offset, int8_t *d_samples, double *d_value, void *hip_stream) {
    if (!s || (ncases > 0 && (!d_evidence || !d_samples || !d_value))) return SetError(FBN_ERR_ARG, "bad argument");
    if (s->device < 0) return SetError(FBN_ERR_NODEV, "host-only handle (created with device < 0)");
    if (int rc = fbn::CheckPsampleShape(s->P, ncases, nsamples, case_offset)) return rc;
    if (ncases == 0) return FBN_OK;
    FBN_HIP(hipSetDevice(s->device));
    return PsampleDevice(s, d_evidence, ncases, nsamples, seed, case_offset, d_samples, d_value,
                         static_cast<hipStream_t>(hip_stream));
}

int fbn_psample_set_tuning(fbn_psample *s, int max_workgroups, int64_t store_bytes_max, int64_t sample_chunk) {
    if (!s || max_workgroups < 0 || store_bytes_max < 0 || sample_chunk < 0) return SetError(FBN_ERR_ARG, "bad argument");
    const int64_t budget = store_bytes_max == 0 ? kPsampleStoreDefault : store_bytes_max;
    if (int rc = CheckBudget(s, budget)) return rc;
    s->store_bytes_max = budget;
    s->max_workgroups = max_workgroups;
    s->sample_chunk = sample_chunk;
    return FBN_OK;
}

int fbn_psample_last_kernel_ms(const fbn_psample *s, float *ms) {
    if (!s) return SetError(FBN_ERR_ARG, "no timed launch");
    return s->LastKernelMs(ms);
}

}  // extern "C"
