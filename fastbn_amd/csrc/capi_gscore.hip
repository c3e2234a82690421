// capi_gscore.hip -- the device entries of the Gaussian family scorer (include/fastbn.h, fbn_gscore_*,
// fbn_hc_run_gauss): batches of families on a Gaussian context's resident R (gscore.hip) and the hill-climbing
// search over them.  The scores and their tables are gscore.h's and gscore_host.cpp's; the search is
// hc_search.cpp's, unchanged.
//
// A batch holds families of every size in the caller's order.  They are bucketed by parent count on the host
// and staged in pinned memory as one array of fixed-stride records per size, (out_index, child, parents..); one
// kernel instantiation per non-empty size runs on the context's stream and writes each family's two results at
// its out_index.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "fbn_device.h"
#include "gci.h"
#include "gci_ctx.h"
#include "gscore_plan.h"
#include "launchers.h"

using fbn::SetError;

namespace fbn {

namespace {

// the plan's per-variable tables on the device
int GsUpload(fbn_gci_ctx *c, const GsPlan &G) {
    const size_t b = (size_t)c->nvars * 8;
    int rc;
    if ((rc = c->gs_lss.ensure(b)) || (rc = c->gs_tq.ensure(b)) || (rc = c->gs_cnt.ensure(8))) return rc;
    FBN_HIP(hipMemcpy(c->gs_lss.p, G.lss.data(), b, hipMemcpyHostToDevice));
    FBN_HIP(hipMemcpy(c->gs_tq.p, G.tq.data(), b, hipMemcpyHostToDevice));
    return FBN_OK;
}

// one batch (already within the limits: GsCheckBatch) on the context's stream; synchronous
int GsDeviceBatch(fbn_gci_ctx *c, const GsPlan &G, const HcBatch &B, double *loglik, double *score, double *kernel_ms) {
    const int64_t nf = B.nfam;
    c->gs_info[0] = nf, c->gs_info[1] = c->gs_info[2] = 0;
    if (!nf) return FBN_OK;
    if (nf > 0x7fffffffll) return SetError(FBN_ERR_LIMIT, "%lld families exceed one batch (2^31 - 1)", (long long)nf);
    // the buckets: count[p] families, their records from int offset first[p]
    int64_t count[kGciMaxD + 1] = {}, first[kGciMaxD + 2] = {};
    for (int64_t f = 0; f < nf; ++f) ++count[B.fam_off[f + 1] - B.fam_off[f] - 1];
    for (int p = 0; p <= kGciMaxD; ++p) first[p + 1] = first[p] + count[p] * (2 + p);
    const size_t rec_bytes = (size_t)first[kGciMaxD + 1] * 4, out_bytes = (size_t)nf * 16;
    int rc;
    if ((rc = PinnedEnsure(c->gs_h_rec, c->gs_h_rec_bytes, rec_bytes)) || (rc = PinnedEnsure(c->gs_h_out, c->gs_h_out_bytes, out_bytes)) ||
        (rc = c->gs_rec.ensure(rec_bytes)) || (rc = c->gs_out.ensure(out_bytes)))
        return rc;
    int32_t *h = static_cast<int32_t *>(c->gs_h_rec);
    int64_t at[kGciMaxD + 1];
    std::copy(first, first + kGciMaxD + 1, at);
    for (int64_t f = 0; f < nf; ++f) {
        const int ncol = (int)(B.fam_off[f + 1] - B.fam_off[f]);
        int32_t *r = h + at[ncol - 1];
        r[0] = (int32_t)f;
        std::copy(B.fam_cols + B.fam_off[f], B.fam_cols + B.fam_off[f + 1], r + 1);
        at[ncol - 1] += 1 + ncol;
    }
    hipStream_t s = c->stream;
    auto &S = c->slot[0];
    FBN_HIP(hipMemcpyAsync(c->gs_rec.p, h, rec_bytes, hipMemcpyHostToDevice, s));
    FBN_HIP(hipMemsetAsync(c->gs_cnt.p, 0, 8, s));
    GscoreArgs a{};
    a.R = c->R.as<double>(), a.lss = c->gs_lss.as<double>(), a.tq = c->gs_tq.as<double>(), a.nvars = c->nvars;
    a.loglik = c->gs_out.as<double>(), a.score = a.loglik + nf;
    a.degenerate = c->gs_cnt.as<unsigned long long>();
    a.C = G.C;
    FBN_HIP(hipEventRecord(S.ev0, s));
    for (int p = 0; p <= kGciMaxD; ++p) {
        if (!count[p]) continue;
        a.rec = c->gs_rec.as<int32_t>() + first[p];
        a.n = count[p];
        const hipError_t e = fbn_gscore_launch(&a, p, G.kind == kGsBGE, s);
        if (e != hipSuccess) return SetError(FBN_ERR_HIP, "Gaussian family score launch: %s", hipGetErrorString(e));
        ++c->gs_info[1];
    }
    FBN_HIP(hipEventRecord(S.ev1, s));
    double *ho = static_cast<double *>(c->gs_h_out);
    FBN_HIP(hipMemcpyAsync(ho, c->gs_out.p, out_bytes, hipMemcpyDeviceToHost, s));
    unsigned long long *hc = c->h_stats + 3;
    FBN_HIP(hipMemcpyAsync(hc, c->gs_cnt.p, 8, hipMemcpyDeviceToHost, s));
    FBN_HIP(hipStreamSynchronize(s));
    float ms = 0.f;
    FBN_HIP(hipEventElapsedTime(&ms, S.ev0, S.ev1));
    if (kernel_ms) *kernel_ms += ms;
    if (loglik) memcpy(loglik, ho, (size_t)nf * 8);
    if (score) memcpy(score, ho + nf, (size_t)nf * 8);
    c->gs_info[2] = (int64_t)*hc;
    return FBN_OK;
}

int GsContextPlan(fbn_gci_ctx *c, const fbn_gauss_score *g, GsPlan *G) {
    if (!c) return SetError(FBN_ERR_ARG, "null pointer");
    if (int rc = GsMakePlan(g, c->nvars, c->N, c->h_ss.data(), G)) return rc;
    FBN_HIP(hipSetDevice(c->device));
    return GsUpload(c, *G);
}

}  // namespace

}  // namespace fbn

extern "C" {

int fbn_gci_moments(fbn_gci_ctx *c, double *mean, double *ss, double *R) {
    int n = 0;
    int64_t N = 0;
    std::vector<double> m, s, r;
    if (int rc = fbn::GciMoments(c, &n, &N, m, s, r)) return rc;
    if (mean) std::copy(m.begin(), m.end(), mean);
    if (ss) std::copy(s.begin(), s.end(), ss);
    if (R) std::copy(r.begin(), r.end(), R);
    return FBN_OK;
}

int fbn_gscore_families(fbn_gci_ctx *c, const fbn_gauss_score *g, int64_t nfam, const int64_t *fam_off,
                        const int32_t *fam_cols, double *loglik, double *score) {
    if (!c) return SetError(FBN_ERR_ARG, "null pointer");
    // everything that can be refused is refused here, on the host, before any launch
    fbn::HcFamilies F;
    if (int rc = fbn::GsCheckFamilies(c->nvars, c->N, nfam, fam_off, fam_cols, &F)) return rc;
    fbn::GsPlan G;
    if (int rc = fbn::GsContextPlan(c, g, &G)) return rc;
    double ms = 0.0;
    if (int rc = fbn::GsDeviceBatch(c, G, F.batch(), loglik, score, &ms)) return rc;
    c->last_ms = (float)ms, c->timed = true;
    return FBN_OK;
}

int fbn_hc_run_gauss(fbn_gci_ctx *c, const fbn_hc_options *options, const fbn_gauss_score *g, fbn_hc_result **out) {
    if (!c || !options || !out) return SetError(FBN_ERR_ARG, "null pointer");
    fbn::GsPlan G;
    if (int rc = fbn::GsContextPlan(c, g, &G)) return rc;
    auto r = std::unique_ptr<fbn_hc_result>(new (std::nothrow) fbn_hc_result());
    if (!r) return SetError(FBN_ERR_NOMEM, "out of memory");
    int64_t degenerate = 0;
    fbn::HcScorer scorer = [c, &G, &degenerate](const fbn::HcBatch &B, double *loglik, double *score, double *kernel_ms) {
        if (int rc = fbn::GsCheckBatch(G.N, B)) return rc;
        const int rc = fbn::GsDeviceBatch(c, G, B, loglik, score, kernel_ms);
        degenerate += c->gs_info[2];
        return rc;
    };
    if (int rc = fbn::GsRunSearch(c->nvars, *options, scorer, r.get())) return rc;
    c->gs_info[2] = degenerate;  // over the whole search
    c->last_ms = (float)r->info.kernel_ms, c->timed = true;
    *out = r.release();
    return FBN_OK;
}

int fbn_gscore_info(const fbn_gci_ctx *c, int64_t out[3]) {
    if (!c || !out) return SetError(FBN_ERR_ARG, "null pointer");
    std::copy(c->gs_info, c->gs_info + 3, out);
    return FBN_OK;
}

}  // extern "C"
