// capi_bma.hip -- the device entry of exact arc posteriors (include/fastbn.h): fbn_bma_run over a CI context's
// resident column store.  The candidate families are enumerated and scored by exact_host.cpp's
// ExactLocalScores through the device scorer (capi_hc.hip), the code the exact search runs; the lattice phases
// are exact_bma.hip's; n^2 + n + 2 doubles return to the host.
//
// The state (two value lattices, F and B: 16 n 2^(n-1) + 16 2^n bytes) lives for one run: it is sized against
// the free device memory before anything is allocated and freed on return.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <new>
#include <vector>

#include "capi_state.h"
#include "exact_bma.h"
#include "launchers.h"
#include "learner_device.h"

using fbn::SetError;

namespace fbn {

namespace {

int BmaRunDevice(fbn_ci_ctx *c, const fbn_exact_options &opt, int prior, const HcScorer &scorer, fbn_bma_result *res) {
    const auto t_start = Clock::now();
    const int n = c->nvars, M = n - 1;
    const int32_t *dims = c->dims.data();
    fbn_bma_info &info = res->info;
    fbn_exact_info xi{};
    info.nvars = n, info.prior = prior, info.levels = n + 1;
    info.lattice_bytes = (int64_t)BmaStateBytes(n);
    if (n == 1) {
        if (int rc = BmaOneVariable(dims, opt, scorer, prior, &xi, res)) return rc;
        BmaTakeScoring(xi, &info);
        info.wall_ms = MsSince(t_start);
        return FBN_OK;
    }
    const size_t L = (size_t)1 << M, NW = (size_t)1 << n, nout = (size_t)n * n + n + 2;
    int rc;
    if ((rc = LatticeFits(n, info.lattice_bytes, "posterior"))) return rc;
    ExactPass pass[kExactMaxVars];
    info.tile_bits = c->bma_tile_bits > 0 ? c->bma_tile_bits : fbn_bma_default_tile_bits(M);
    if ((rc = LatticePasses(n, info.tile_bits, kBmaLdsBits, pass, &info.passes))) return rc;
    DevBuf ls, X, Fw, Bw, out;
    if ((rc = ls.ensure(L * n * 8)) || (rc = X.ensure(L * n * 8)) || (rc = Fw.ensure(NW * 8)) || (rc = Bw.ensure(NW * 8)) ||
        (rc = out.ensure(nout * 8)))
        return rc;
    hipStream_t s = c->stream;

    // the local scores of one variable at a time into pinned memory, then up
    const std::vector<double> lp = BmaSizePrior(n, prior);
    Pinned stage;
    if ((rc = LatticeLocalScores(c, opt, scorer, lp.empty() ? nullptr : lp.data(), stage, ls.as<double>(), &xi, &info.upload_wall_ms)))
        return rc;
    BmaTakeScoring(xi, &info);

    // a transform: its first pass loads what `first_load` names, the later ones the lattice itself
    auto transform = [&](int dir, int op, int first_load, const char *what) {
        return [=, &info, &pass, &X, &ls, &Fw, &Bw]() -> int {
            for (int p = 0; p < info.passes; ++p) {
                const BmaPassArgs a{X.as<double>(), ls.as<double>(), Fw.as<double>(), Bw.as<double>(), n, M, pass[p].gpos, pass[p].hb,
                                    pass[p].lo, pass[p].s0, pass[p].G, dir, op, p == 0 ? first_load : (int)kBmaLoadX};
                const hipError_t le = fbn_bma_pass_launch(&a, s);
                if (le != hipSuccess) return SetError(FBN_ERR_HIP, "%s pass %d launch: %s", what, p, hipGetErrorString(le));
            }
            return FBN_OK;
        };
    };
    if ((rc = Phase(c, &info.alpha_kernel_ms, &info.alpha_wall_ms, transform(kBmaSubset, kBmaLse, kBmaLoadLs, "alpha")))) return rc;
    if ((rc = Phase(c, &info.level_kernel_ms, &info.level_wall_ms, [&]() -> int {
             for (int k = 0; k <= n; ++k) {
                 const BmaLevelArgs a{X.as<double>(), Fw.as<double>(), Bw.as<double>(), n, k};
                 const hipError_t le = fbn_bma_level_launch(&a, s);
                 if (le != hipSuccess) return SetError(FBN_ERR_HIP, "level %d launch: %s", k, hipGetErrorString(le));
             }
             return FBN_OK;
         })))
        return rc;
    if ((rc = Phase(c, &info.gamma_kernel_ms, &info.gamma_wall_ms, transform(kBmaSuperset, kBmaLse, kBmaLoadGamma, "Gamma")))) return rc;
    if ((rc = Phase(c, &info.q_kernel_ms, &info.q_wall_ms, transform(kBmaSuperset, kBmaAdd, kBmaLoadP, "q")))) return rc;

    const hipError_t e = fbn_bma_gather_launch(X.as<double>(), Fw.as<double>(), Bw.as<double>(), n, out.as<double>(), s);
    if (e != hipSuccess) return SetError(FBN_ERR_HIP, "gather launch: %s", hipGetErrorString(e));
    std::vector<double> h(nout);
    FBN_HIP(hipMemcpyAsync(h.data(), out.p, nout * 8, hipMemcpyDeviceToHost, s));
    FBN_HIP(hipStreamSynchronize(s));
    res->arc_prob.assign(h.begin(), h.begin() + (size_t)n * n);
    res->q_empty.assign(h.begin() + (size_t)n * n, h.begin() + (size_t)n * n + n);
    info.log_z = h[nout - 2], info.b_full = h[nout - 1];
    info.wall_ms = MsSince(t_start);
    return FBN_OK;
}

}  // namespace
}  // namespace fbn

// fbn_bma_run (bd == nullptr; *bd outlives the run) and fbn_bma_run_bd
static int BmaRun(fbn_ci_ctx *c, const fbn_exact_options *options, int32_t prior, const fbn_bd_score *bd, fbn_bma_result **out) {
    if (!c || !options || !out) return SetError(FBN_ERR_ARG, "null pointer");
    if (int rc = fbn::BmaCheck(c->nvars, c->dims.data(), *options, prior)) return rc;
    if (int rc = fbn::HcCheckSamples(c->N)) return rc;
    FBN_HIP(hipSetDevice(c->device));
    auto r = std::unique_ptr<fbn_bma_result>(new (std::nothrow) fbn_bma_result());
    if (!r) return SetError(FBN_ERR_NOMEM, "out of memory");
    if (int rc = fbn::BmaRunDevice(c, *options, prior, fbn::HcDeviceScorer(c, bd), r.get())) return rc;
    const fbn_bma_info &i = r->info;
    c->last_ms = (float)(i.score_kernel_ms + i.alpha_kernel_ms + i.level_kernel_ms + i.gamma_kernel_ms + i.q_kernel_ms);
    *out = r.release();
    return FBN_OK;
}

extern "C" {

int fbn_bma_run(fbn_ci_ctx *c, const fbn_exact_options *options, int32_t prior, fbn_bma_result **out) {
    return BmaRun(c, options, prior, nullptr, out);
}

int fbn_bma_run_bd(fbn_ci_ctx *c, const fbn_exact_options *options, int32_t prior, const fbn_bd_score *bd,
                   fbn_bma_result **out) {
    if (int rc = fbn::BdCheck(bd)) return rc;
    return BmaRun(c, options, prior, bd, out);
}

int fbn_bma_set_tuning(fbn_ci_ctx *c, int32_t tile_bits) {
    if (!c) return SetError(FBN_ERR_ARG, "null pointer");
    if (tile_bits < 0 || tile_bits > kBmaTileBitsMax)
        return SetError(FBN_ERR_ARG, "tile_bits = %d out of 0..%d", tile_bits, kBmaTileBitsMax);
    c->bma_tile_bits = tile_bits;
    return FBN_OK;
}

}  // extern "C"
