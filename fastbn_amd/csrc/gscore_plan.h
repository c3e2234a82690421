// gscore_plan.h -- what the host twin (gscore_host.cpp) and the device entries (capi_gscore.hip) of the Gaussian
// family scorer share: the validated score record with its tables, the family checks, the host evaluation
// and the hill-climbing run over either scorer.  Internal to libfastbn.
#ifndef FBN_GSCORE_PLAN_H
#define FBN_GSCORE_PLAN_H

#include <cstdint>
#include <vector>

#include "gscore.h"
#include "hc_search.h"

namespace fbn {

// gscore.h's tables of one score on one set of moments
struct GsPlan {
    int kind = kGsLL, nvars = 0;
    int64_t N = 0;
    FbnGsConsts C{};
    std::vector<double> lss, tq;  // [nvars]; tq all 0 under kGsLL
};

// FBN_ERR_ARG: an unknown kind, a penalty or alpha_mu that is no number of its range, alpha_w <= n - 1 or a
// t that is not positive (alpha_w <= n + 1); ss [nvars] must be positive
int GsMakePlan(const fbn_gauss_score *g, int nvars, int64_t N, const double *ss, GsPlan *out);

// fbn_score_families' checks with every state count 1, then FBN_ERR_LIMIT for more than kGciMaxD parents or
// N <= p + 2; the parents come out ascending
int GsCheckFamilies(int nvars, int64_t N, int64_t nfam, const int64_t *fam_off, const int32_t *fam_cols, HcFamilies *out);
// the limits alone, of a batch the search built
int GsCheckBatch(int64_t N, const HcBatch &B);

// the twin of a device batch over R [nvars][nvars]; adds the degenerate families to *degenerate
int GsHostBatch(const GsPlan &P, const double *R, const HcBatch &B, double *loglik, double *score, int64_t *degenerate);

// HcSearch, unchanged, with every state count 1: max_parents < 0 or above kGciMaxD means kGciMaxD; a start
// graph is scored first and refused (FBN_ERR_ARG) where it holds a degenerate family
int GsRunSearch(int nvars, const fbn_hc_options &opt, const HcScorer &scorer, fbn_hc_result *res);

}  // namespace fbn

#endif
