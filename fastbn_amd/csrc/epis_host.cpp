// epis_host.cpp -- host twin of EPIS-BN (device < 0 handles): lbp_host.cpp's pre-propagation, then
// sample_host.cpp's loop with the lambda rows as the importance function (epis_model.h).  Operation
// for operation what the two launches of capi_epis.hip do, so the two agree bit for bit.
#include <algorithm>
#include <vector>

#include "epis_model.h"
#include "fbn_internal.h"

namespace fbn {

int CheckEpisArgs(const SamplerModel &M, int64_t ncases, int64_t S, int64_t case_offset, int iters, double tol,
                  double damping, double eps) {
    if (int rc = CheckLwShape(M, 0, ncases, S, case_offset)) return rc;
    if (iters < 0) return SetError(FBN_ERR_ARG, "iterations must be >= 0 (got %d)", iters);
    if (!(tol >= 0.0)) return SetError(FBN_ERR_ARG, "tol must be >= 0 (got %g)", tol);
    if (!(damping >= 0.0 && damping < 1.0)) return SetError(FBN_ERR_ARG, "damping must be in [0, 1) (got %g)", damping);
    if (!(eps < 1.0)) return SetError(FBN_ERR_ARG, "eps must be below 1 (negative: the defaults; got %g)", eps);
    return FBN_OK;
}

int HostEpis(const SamplerModel &SM, const LbpModel &LM, const int8_t *ev, int64_t ncases, int64_t S, uint64_t seed,
             int64_t case_offset, int iters, double tol, double damping, double eps, int32_t *labels, double *marg,
             double *stats, uint8_t *dbg_vals, double *dbg_m, int32_t *dbg_e, double *dbg_lam) {
    if (ncases == 0) return FBN_OK;
    std::vector<double> own, lst;
    double *lam = dbg_lam;
    if (!lam) {
        own.resize((size_t)ncases * SM.sum_dom);
        lam = own.data();
    }
    if (iters > 0) {
        lst.resize((size_t)ncases * 2);
        if (int rc = HostLbp(LM, ev, ncases, iters, tol, damping, labels, nullptr, lst.data(), nullptr, lam)) return rc;
    } else {
        std::fill(lam, lam + (size_t)ncases * SM.sum_dom, 1.0);
    }
    return HostImportance(SM, 0, ev, ncases, S, seed, case_offset, lam, eps, iters > 0 ? lst.data() : nullptr, labels, marg,
                          stats, dbg_vals, dbg_m, dbg_e);
}

}  // namespace fbn
