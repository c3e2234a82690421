// capi_exact.hip -- the device entry of exact score-optimal structure learning (include/fastbn.h):
// fbn_exact_run over a CI context's resident column store.  The candidate families are enumerated and
// scored by exact_host.cpp's ExactLocalScores through the device scorer (capi_hc.hip), the lattices are
// transformed and the sink table filled by exact_dp.hip, and the DAG is traced on the host from the sink
// table (2^n bytes back) and n single reads of the arg lattices.
//
// The lattice learners' scaffold (learner_device.h: the free-memory and grid refusals, the local scores up) is
// defined here; capi_bma.hip runs it too.
//
// The state (12 n 2^(n-1) + 9 2^n bytes) lives for one run: it is sized against the free device memory
// before anything is allocated and freed on return, so a context does not sit on gigabytes between runs.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <new>
#include <vector>

#include "capi_state.h"
#include "exact_dp.h"
#include "launchers.h"
#include "learner_device.h"

using fbn::SetError;

namespace fbn {

int LatticeFits(int n, int64_t state_bytes, const char *what) {
    size_t free_b = 0, total_b = 0;
    FBN_HIP(hipMemGetInfo(&free_b, &total_b));
    if ((size_t)state_bytes > free_b)
        return SetError(FBN_ERR_LIMIT, "%d variables: the %s lattices take %lld bytes, %zu are free on the device", n, what,
                        (long long)state_bytes, free_b);
    return FBN_OK;
}

int LatticePasses(int n, int tile_bits, int lds_bits, ExactPass *pass, int32_t *passes) {
    const int M = n - 1;
    *passes = fbn_exact_passes(M, tile_bits, pass, lds_bits);
    for (int p = 0; p < *passes; ++p)
        if (((uint64_t)n << (M - pass[p].lo - pass[p].hb)) > kExactGridMax)
            return SetError(FBN_ERR_LIMIT, "tile_bits = %d: pass %d of %d variables needs more than %llu workgroups", tile_bits, p, n,
                            (unsigned long long)kExactGridMax);
    return FBN_OK;
}

int LatticeLocalScores(fbn_ci_ctx *c, const fbn_exact_options &opt, const HcScorer &scorer, const double *size_prior, Pinned &stage,
                       double *d_ls, fbn_exact_info *xi, double *upload_wall_ms) {
    const int n = c->nvars;
    const size_t L = (size_t)1 << (n - 1);
    if (int rc = stage.alloc(L * 8)) return rc;
    for (int v = 0; v < n; ++v) {
        if (int rc = ExactLocalScores(n, c->dims.data(), opt, scorer, v, static_cast<double *>(stage.p), xi, size_prior)) return rc;
        const auto t0 = Clock::now();
        FBN_HIP(hipMemcpy(d_ls + L * v, stage.p, L * 8, hipMemcpyHostToDevice));
        *upload_wall_ms += MsSince(t0);
    }
    return FBN_OK;
}

namespace {

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
    int rc;
    if ((rc = LatticeFits(n, info.lattice_bytes, "subset"))) return rc;
    DevBuf val, arg, R, sink;
    if ((rc = val.ensure(L * n * 8)) || (rc = arg.ensure(L * n * 4)) || (rc = R.ensure(NW * 8)) || (rc = sink.ensure(NW))) return rc;
    hipStream_t s = c->stream;

    // phase 1: the local scores of one variable at a time into pinned memory, then up
    Pinned stage;
    if ((rc = LatticeLocalScores(c, opt, scorer, nullptr, stage, val.as<double>(), &info, &info.upload_wall_ms))) return rc;

    // phase 2: the subset-max transform, ceil(M / tile_bits) passes over all lattices
    ExactPass pass[kExactMaxVars];
    info.tile_bits = c->exact_tile_bits > 0 ? c->exact_tile_bits : fbn_exact_default_tile_bits(M);
    if ((rc = LatticePasses(n, info.tile_bits, kExactLdsBits, pass, &info.passes))) return rc;
    if ((rc = Phase(c, &info.transform_kernel_ms, &info.transform_wall_ms, [&]() -> int {
             for (int p = 0; p < info.passes; ++p) {
                 const ExactPassArgs a{val.as<double>(), arg.as<uint32_t>(), n, M, pass[p].gpos, pass[p].hb, pass[p].lo, pass[p].s0, pass[p].G,
                                       p == 0};
                 const hipError_t e = fbn_exact_pass_launch(&a, s);
                 if (e != hipSuccess) return SetError(FBN_ERR_HIP, "subset-max pass %d launch: %s", p, hipGetErrorString(e));
             }
             return FBN_OK;
         })))
        return rc;

    // phase 3: the sink recursion, one launch per level
    info.levels = n + 1;
    if ((rc = Phase(c, &info.sink_kernel_ms, &info.sink_wall_ms, [&]() -> int {
             for (int k = 0; k <= n; ++k) {
                 const ExactSinkArgs a{val.as<double>(), R.as<double>(), sink.as<uint8_t>(), n, k};
                 const hipError_t e = fbn_exact_sink_launch(&a, s);
                 if (e != hipSuccess) return SetError(FBN_ERR_HIP, "sink level %d launch: %s", k, hipGetErrorString(e));
             }
             return FBN_OK;
         })))
        return rc;

    // phase 4: the sink table back, the trace with n reads of the arg lattices
    const auto t0 = Clock::now();
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
    if (int rc = fbn::ExactRunDevice(c, *options, fbn::HcDeviceScorer(c, bd), r.get())) return rc;
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
