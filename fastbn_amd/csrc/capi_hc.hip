// capi_hc.hip -- the device entries of score-based structure learning (include/fastbn.h): the batched
// family scorer over a CI context's resident column store (fbn_score_families) and the hill-climbing
// search over it (fbn_hc_run).  The search itself and the host twin are hc_search.cpp's.
//
// A batch is counted by param_counts.hip (fbn_param_launch, unchanged: its family descriptor is an
// arbitrary (child, parents) list) into the context's zeroed 32-bit tables and reduced by hc_score.hip to
// two doubles per family; the tables never leave the device.  A batch whose tables exceed the chunk cap
// (FBN_PARAM_MAX_CELLS, or fbn_hc_set_tuning's) is processed in chunks of consecutive families.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <memory>
#include <new>
#include <vector>

#include "capi_state.h"
#include "hc_score.h"
#include "hc_search.h"
#include "launchers.h"
#include "param_counts.h"

using fbn::SetError;

namespace fbn {

// the score table on the device, built once per context
static int HcTable(fbn_ci_ctx *c) {
    if (c->hc_table_ready) return FBN_OK;
    if (int rc = HcCheckSamples(c->N)) return rc;
    std::vector<double> L((size_t)c->N + 1);
    fbn_hc_fill_table(L.data(), c->N);
    if (int rc = c->hc_L.ensure(L.size() * 8)) return rc;
    FBN_HIP(hipMemcpy(c->hc_L.p, L.data(), L.size() * 8, hipMemcpyHostToDevice));
    c->hc_table_ready = true;  // the synchronous copy is done: L may go
    return FBN_OK;
}

// families [f0, f1) of B: descriptors up, tables zeroed, counted, reduced, 16 bytes per family back
static int HcChunk(fbn_ci_ctx *c, const HcBatch &B, int64_t f0, int64_t f1, int64_t cells, double *loglik, double *score,
                   double *kernel_ms) {
    const int64_t nf = f1 - f0;
    int64_t slice = c->par_slice;
    if (slice <= 0) slice = fbn_param_default_slice(c->N, c->num_cu, nf);
    const int64_t nslices = (c->N + slice - 1) / slice;
    if (nf * nslices > 0x7fffffffll)
        return SetError(FBN_ERR_LIMIT, "%lld families x %lld slices exceed one launch", (long long)nf, (long long)nslices);
    const int lds_max = c->par_lds == 0 ? kParamLdsCellsMax : (int)std::max<int64_t>(0, std::min<int64_t>(c->par_lds, kParamLdsCellsMax));
    const int64_t c0 = B.fam_off[f0], ncols = B.fam_off[f1] - c0;
    std::vector<FbnParamFamily> fam((size_t)nf);
    std::vector<int32_t> fstr((size_t)ncols);
    size_t lds_ints = 1;
    int64_t tab_off = 0;
    for (int64_t f = f0; f < f1; ++f) {
        const int64_t o = B.fam_off[f] - c0;
        const int k = (int)(B.fam_off[f + 1] - B.fam_off[f]) - 1;
        const int32_t *fc = B.fam_cols + B.fam_off[f];
        fam[(size_t)(f - f0)] = FbnParamFamily{(long long)tab_off, (int32_t)o, k + 1, (int32_t)B.cells[f], 0};
        int64_t str = 1;
        for (int j = k; j >= 1; --j) {
            fstr[(size_t)(o + j)] = (int32_t)str;
            str *= c->dims[fc[j]];
        }
        fstr[(size_t)o] = (int32_t)str;  // = cells / dims[child]: hc_score.hip reads it as q
        tab_off += B.cells[f];
        if (B.cells[f] <= lds_max) lds_ints = std::max(lds_ints, fbn_param_lds_ints((int)B.cells[f]));
    }
    int rc;
    if ((rc = c->par_fam.ensure(fam.size() * sizeof(FbnParamFamily))) || (rc = c->par_col.ensure((size_t)ncols * 4)) ||
        (rc = c->par_str.ensure((size_t)ncols * 4)) || (rc = c->par_tab.ensure((size_t)cells * 4)) ||
        (rc = c->hc_pen.ensure((size_t)nf * 8)) || (rc = c->hc_out.ensure((size_t)nf * 16)))
        return rc;
    hipStream_t s = c->stream;
    CiSlot &S = c->slot[0];
    std::vector<double> out((size_t)nf * 2);
    fbn::StreamDrain drain(s);  // after fam, fstr and out: an early return waits for the copies that use them
    FBN_HIP(hipMemcpyAsync(c->par_fam.p, fam.data(), fam.size() * sizeof(FbnParamFamily), hipMemcpyHostToDevice, s));
    FBN_HIP(hipMemcpyAsync(c->par_col.p, B.fam_cols + c0, (size_t)ncols * 4, hipMemcpyHostToDevice, s));
    FBN_HIP(hipMemcpyAsync(c->par_str.p, fstr.data(), (size_t)ncols * 4, hipMemcpyHostToDevice, s));
    FBN_HIP(hipMemcpyAsync(c->hc_pen.p, B.pen + f0, (size_t)nf * 8, hipMemcpyHostToDevice, s));
    if (c->timing) FBN_HIP(hipEventRecord(S.ev0, s));
    FBN_HIP(hipMemsetAsync(c->par_tab.p, 0, (size_t)cells * 4, s));
    hipError_t e = fbn_param_launch(c->cols.as<uint8_t>(), c->N, c->par_fam.as<FbnParamFamily>(), nf, c->par_col.as<int32_t>(),
                                    c->par_str.as<int32_t>(), c->par_tab.as<uint32_t>(), slice, nslices, lds_max,
                                    lds_ints * 4, s);
    if (e != hipSuccess) return SetError(FBN_ERR_HIP, "family counts launch: %s", hipGetErrorString(e));
    HcScoreArgs a{c->par_tab.as<uint32_t>(), c->par_fam.as<FbnParamFamily>(), c->par_str.as<int32_t>(),
                  c->hc_pen.as<double>(), c->hc_L.as<double>(), c->hc_out.as<double>(), (long long)nf};
    if ((e = fbn_hc_score_launch(&a, s)) != hipSuccess)
        return SetError(FBN_ERR_HIP, "family score launch: %s", hipGetErrorString(e));
    if (c->timing) FBN_HIP(hipEventRecord(S.ev1, s));
    FBN_HIP(hipMemcpyAsync(out.data(), c->hc_out.p, out.size() * 8, hipMemcpyDeviceToHost, s));
    FBN_HIP(hipStreamSynchronize(s));
    drain.done();
    if (c->timing) {
        float ms = 0.f;
        FBN_HIP(hipEventElapsedTime(&ms, S.ev0, S.ev1));
        *kernel_ms += ms;
    }
    for (int64_t f = 0; f < nf; ++f) {
        if (loglik) loglik[f0 + f] = out[(size_t)(2 * f)];
        if (score) score[f0 + f] = out[(size_t)(2 * f + 1)];
    }
    return FBN_OK;
}

// the device scorer: chunks of consecutive families whose tables fit the cap (a larger family alone)
static int HcDeviceScore(fbn_ci_ctx *c, const HcBatch &B, double *loglik, double *score, double *kernel_ms) {
    if (!B.nfam) return FBN_OK;
    FBN_HIP(hipSetDevice(c->device));
    if (int rc = HcTable(c)) return rc;
    const int64_t cap = c->hc_chunk > 0 ? std::min<int64_t>(c->hc_chunk, FBN_PARAM_MAX_CELLS) : FBN_PARAM_MAX_CELLS;
    for (int64_t f0 = 0; f0 < B.nfam;) {
        int64_t f1 = f0 + 1, cells = B.cells[f0];
        while (f1 < B.nfam && cells + B.cells[f1] <= cap) cells += B.cells[f1++];
        if (int rc = HcChunk(c, B, f0, f1, cells, loglik, score, kernel_ms)) return rc;
        f0 = f1;
    }
    return FBN_OK;
}

}  // namespace fbn

extern "C" {

int fbn_hc_set_tuning(fbn_ci_ctx *c, int64_t chunk_cells_max) {
    if (!c) return SetError(FBN_ERR_ARG, "null pointer");
    if (chunk_cells_max < 0) return SetError(FBN_ERR_ARG, "chunk_cells_max = %lld is negative", (long long)chunk_cells_max);
    c->hc_chunk = chunk_cells_max;
    return FBN_OK;
}

int fbn_score_families(fbn_ci_ctx *c, double penalty, int64_t nfam, const int64_t *fam_off, const int32_t *fam_cols,
                       double *loglik, double *score) {
    if (!c) return SetError(FBN_ERR_ARG, "null pointer");
    // everything that can be refused is refused here, on the host, before any launch
    fbn::HcFamilies F;
    if (int rc = fbn::HcCheckFamilies(c->nvars, c->dims.data(), penalty, nfam, fam_off, fam_cols, &F)) return rc;
    if (int rc = fbn::HcCheckSamples(c->N)) return rc;
    double ms = 0.0;
    const int rc = fbn::HcDeviceScore(c, F.batch(), loglik, score, &ms);
    c->last_ms = (float)ms;
    return rc;
}

int fbn_hc_run(fbn_ci_ctx *c, const fbn_hc_options *options, fbn_hc_result **out) {
    if (!c || !options || !out) return SetError(FBN_ERR_ARG, "null pointer");
    if (int rc = fbn::HcCheckSamples(c->N)) return rc;
    auto r = std::unique_ptr<fbn_hc_result>(new (std::nothrow) fbn_hc_result());
    if (!r) return SetError(FBN_ERR_NOMEM, "out of memory");
    fbn::HcScorer scorer = [c](const fbn::HcBatch &B, double *loglik, double *score, double *kernel_ms) {
        return fbn::HcDeviceScore(c, B, loglik, score, kernel_ms);
    };
    if (int rc = fbn::HcSearch(c->nvars, c->dims.data(), *options, scorer, r.get())) return rc;
    c->last_ms = (float)r->info.kernel_ms;
    *out = r.release();
    return FBN_OK;
}

}  // extern "C"
