// hc_search.h -- the hill-climbing search (hc_search.cpp) behind fbn_hc_run / fbn_hc_run_host: host code
// with no HIP in it, over a "score these families" callback, so one search runs over the device scorer
// (capi_hc.hip) and over the host scorer, its twin.  Internal to libfastbn.
#ifndef FBN_HC_SEARCH_H
#define FBN_HC_SEARCH_H

#include <cstdint>
#include <functional>
#include <vector>

#include "../../include/fastbn.h"

namespace fbn {

// families [0, nfam): columns fam_cols[fam_off[f] .. fam_off[f+1]), the child first, its parents
// ascending; pen[f] = the family's penalty term; cells[f] = its table size.  Writes loglik / score
// [nfam] and adds its device time to *kernel_ms.
struct HcBatch {
    int64_t nfam = 0;
    const int64_t *fam_off = nullptr;
    const int32_t *fam_cols = nullptr;
    const int64_t *cells = nullptr;
    const double *pen = nullptr;
};
using HcScorer = std::function<int(const HcBatch &, double *loglik, double *score, double *kernel_ms)>;

// validation and shapes of a caller's families (fbn_score_families' checks): the parents sorted into
// cols, cells and penalty terms per family
struct HcFamilies {
    std::vector<int64_t> off, cells;
    std::vector<int32_t> cols;
    std::vector<double> pen;
    HcBatch batch() const { return HcBatch{(int64_t)cells.size(), off.data(), cols.data(), cells.data(), pen.data()}; }
};
int HcCheckFamilies(int nvars, const int32_t *dims, double penalty, int64_t nfam, const int64_t *fam_off,
                    const int32_t *fam_cols, HcFamilies *out);
int HcCheckSamples(int64_t nsamples);

// the host scorer over a host column store; L = the table of fbn_hc_fill_table(nsamples)
HcScorer HcHostScorer(int nvars, const int32_t *dims, const uint8_t *cols, int64_t nsamples, const double *L);

}  // namespace fbn

struct fbn_hc_result {
    fbn_hc_info info{};
    std::vector<int32_t> parent_off, parents, ops;
    std::vector<double> node_score, node_loglik, delta;
};

namespace fbn {
int HcSearch(int nvars, const int32_t *dims, const fbn_hc_options &opt, const HcScorer &scorer, fbn_hc_result *res);
}

#endif
