// capi_exact.hip -- the device entry of exact score-optimal structure learning (include/fastbn.h):
// fbn_exact_run over a CI context's resident column store.  The candidate families are enumerated and
// scored by exact_host.cpp's ExactLocalScores through the device scorer (capi_hc.hip), the lattices are
// transformed and the sink table filled by exact_dp.hip, and the DAG is traced on the host from the sink
// table (2^n bytes back) and n single reads of the arg lattices.
//
// The state (12 n 2^(n-1) + 9 2^n bytes) lives for one run: it is sized against the free device memory
// before anything is allocated and freed on return, so a context does not sit on gigabytes between runs.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <memory>
#include <new>
#include <vector>

#include "capi_state.h"
#include "exact_dp.h"
#include "hc_search.h"
#include "launchers.h"

using fbn::SetError;

namespace fbn {

namespace {

using Clock = std::chrono::steady_clock;
double MsSince(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

struct Pinned {
    void *p = nullptr;
    ~Pinned() {
        if (p) (void)hipHostFree(p);
    }
};

// everything queued on the stream since ev0, in ms (0 with timing off)
int Elapsed(fbn_ci_ctx *c, double *ms) {
    CiSlot &S = c->slot[0];
    if (c->timing) FBN_HIP(hipEventRecord(S.ev1, c->stream));
    FBN_HIP(hipStreamSynchronize(c->stream));
    if (c->timing) {
        float f = 0.f;
        FBN_HIP(hipEventElapsedTime(&f, S.ev0, S.ev1));
        *ms = f;
    }
    return FBN_OK;
}

int ExactRunDevice(fbn_ci_ctx *c, const fbn_exact_options &opt, const HcScorer &scorer, fbn_hc_result *res) {
    const auto t_start = Clock::now();
    const int n = c->nvars, M = n - 1;
    const int32_t *dims = c->dims.data();
    fbn_exact_info info{};
    info.nvars = n;
    info.lattice_bytes = (int64_t)ExactStateBytes(n);
    if (n == 1) {  // no lattice: the empty DAG, its one family scored
        if (int rc = ExactTrace(n, dims, opt, scorer, nullptr, nullptr, 0.0, &info, res)) return rc;
        res->info.score = res->node_score[0];
        info.wall_ms = res->info.wall_ms = MsSince(t_start);
        res->exact = info;
        return FBN_OK;
    }
    const size_t L = (size_t)1 << M, NW = (size_t)1 << n;
    size_t free_b = 0, total_b = 0;
    FBN_HIP(hipMemGetInfo(&free_b, &total_b));
    if ((size_t)info.lattice_bytes > free_b)
        return SetError(FBN_ERR_LIMIT, "%d variables: the subset lattices take %lld bytes, %zu are free on the device", n,
                        (long long)info.lattice_bytes, free_b);
    DevBuf val, arg, R, sink;
    int rc;
    if ((rc = val.ensure(L * n * 8)) || (rc = arg.ensure(L * n * 4)) || (rc = R.ensure(NW * 8)) || (rc = sink.ensure(NW))) return rc;
    hipStream_t s = c->stream;
    CiSlot &S = c->slot[0];

    // phase 1: the local scores of one variable at a time into pinned memory, then up
    Pinned stage;
    hipError_t e = hipHostMalloc(&stage.p, L * 8, hipHostMallocDefault);
    if (e != hipSuccess) return SetError(FBN_ERR_NOMEM, "hipHostMalloc(%zu): %s", L * 8, hipGetErrorString(e));
    for (int v = 0; v < n; ++v) {
        if ((rc = ExactLocalScores(n, dims, opt, scorer, v, static_cast<double *>(stage.p), &info))) return rc;
        const auto t0 = Clock::now();
        FBN_HIP(hipMemcpy(val.as<double>() + L * v, stage.p, L * 8, hipMemcpyHostToDevice));
        info.upload_wall_ms += MsSince(t0);
    }

    // phase 2: the subset-max transform, ceil(M / tile_bits) passes over all lattices
    const int T = c->exact_tile_bits > 0 ? c->exact_tile_bits : fbn_exact_default_tile_bits(M);
    ExactPass pass[kExactMaxVars];
    info.tile_bits = T;
    info.passes = fbn_exact_passes(M, T, pass);
    for (int p = 0; p < info.passes; ++p)
        if (((uint64_t)n << (M - pass[p].lo - pass[p].hb)) > kExactGridMax)
            return SetError(FBN_ERR_LIMIT, "tile_bits = %d: pass %d of %d variables needs more than %llu workgroups", T, p, n,
                            (unsigned long long)kExactGridMax);
    auto t0 = Clock::now();
    if (c->timing) FBN_HIP(hipEventRecord(S.ev0, s));
    for (int p = 0; p < info.passes; ++p) {
        const ExactPassArgs a{val.as<double>(), arg.as<uint32_t>(), n, M, pass[p].gpos, pass[p].hb, pass[p].lo, pass[p].s0, pass[p].G, p == 0};
        if ((e = fbn_exact_pass_launch(&a, s)) != hipSuccess)
            return SetError(FBN_ERR_HIP, "subset-max pass %d launch: %s", p, hipGetErrorString(e));
    }
    if ((rc = Elapsed(c, &info.transform_kernel_ms))) return rc;
    info.transform_wall_ms = MsSince(t0);

    // phase 3: the sink recursion, one launch per level
    t0 = Clock::now();
    info.levels = n + 1;
    if (c->timing) FBN_HIP(hipEventRecord(S.ev0, s));
    for (int k = 0; k <= n; ++k) {
        const ExactSinkArgs a{val.as<double>(), R.as<double>(), sink.as<uint8_t>(), n, k};
        if ((e = fbn_exact_sink_launch(&a, s)) != hipSuccess)
            return SetError(FBN_ERR_HIP, "sink level %d launch: %s", k, hipGetErrorString(e));
    }
    if ((rc = Elapsed(c, &info.sink_kernel_ms))) return rc;
    info.sink_wall_ms = MsSince(t0);

    // phase 4: the sink table back, the trace with n reads of the arg lattices
    t0 = Clock::now();
    std::vector<uint8_t> hsink(NW);
    double RV = 0.0;
    FBN_HIP(hipMemcpy(hsink.data(), sink.p, NW, hipMemcpyDeviceToHost));
    FBN_HIP(hipMemcpy(&RV, R.as<double>() + (NW - 1), 8, hipMemcpyDeviceToHost));
    auto arg_at = [&](int v, uint32_t i, uint32_t *a) -> int {
        FBN_HIP(hipMemcpy(a, arg.as<uint32_t>() + L * v + i, 4, hipMemcpyDeviceToHost));
        return FBN_OK;
    };
    if ((rc = ExactTrace(n, dims, opt, scorer, hsink.data(), arg_at, RV, &info, res))) return rc;
    info.trace_wall_ms = MsSince(t0);
    info.wall_ms = res->info.wall_ms = MsSince(t_start);
    res->exact = info;
    return FBN_OK;
}

}  // namespace
}  // namespace fbn

extern "C" {

int fbn_exact_set_tuning(fbn_ci_ctx *c, int32_t tile_bits) {
    if (!c) return SetError(FBN_ERR_ARG, "null pointer");
    if (tile_bits < 0 || tile_bits > kExactTileBitsMax)
        return SetError(FBN_ERR_ARG, "tile_bits = %d out of 0..%d", tile_bits, kExactTileBitsMax);
    c->exact_tile_bits = tile_bits;
    return FBN_OK;
}

}  // extern "C"

// fbn_exact_run (bd == nullptr; *bd outlives the run) and fbn_exact_run_bd
static int ExactRun(fbn_ci_ctx *c, const fbn_exact_options *options, const fbn_bd_score *bd, fbn_hc_result **out) {
    if (!c || !options || !out) return SetError(FBN_ERR_ARG, "null pointer");
    if (int rc = fbn::ExactCheck(c->nvars, c->dims.data(), *options)) return rc;
    if (int rc = fbn::HcCheckSamples(c->N)) return rc;
    FBN_HIP(hipSetDevice(c->device));
    auto r = std::unique_ptr<fbn_hc_result>(new (std::nothrow) fbn_hc_result());
    if (!r) return SetError(FBN_ERR_NOMEM, "out of memory");
    fbn::HcScorer scorer = [c, bd](const fbn::HcBatch &B, double *loglik, double *score, double *kernel_ms) {
        return fbn::HcDeviceScore(c, B, loglik, score, kernel_ms, bd);
    };
    if (int rc = fbn::ExactRunDevice(c, *options, scorer, r.get())) return rc;
    c->last_ms = (float)(r->exact.score_kernel_ms + r->exact.transform_kernel_ms + r->exact.sink_kernel_ms);
    *out = r.release();
    return FBN_OK;
}

extern "C" {

int fbn_exact_run(fbn_ci_ctx *c, const fbn_exact_options *options, fbn_hc_result **out) {
    return ExactRun(c, options, nullptr, out);
}

int fbn_exact_run_bd(fbn_ci_ctx *c, const fbn_exact_options *options, const fbn_bd_score *bd, fbn_hc_result **out) {
    if (int rc = fbn::BdCheck(bd)) return rc;
    return ExactRun(c, options, bd, out);
}

}  // extern "C"
