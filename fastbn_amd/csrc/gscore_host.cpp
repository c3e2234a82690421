// gscore_host.cpp -- the host side of the Gaussian family scorer (gscore_plan.h): the score record's checks and
// tables, the family limits, and the host twin -- fbn_gscore_families_host and fbn_hc_run_gauss_host evaluate
// gscore.h on the CPU over moments the caller hands in, through the very search (hc_search.cpp) the device run
// uses.  Given a context's moments they repeat its scores, deltas and graphs bit for bit.  No device.
#include <cmath>
#include <memory>
#include <new>

#include "fbn_internal.h"
#include "gscore_plan.h"

namespace fbn {

int GsMakePlan(const fbn_gauss_score *g, int nvars, int64_t N, const double *ss, GsPlan *out) {
    if (!g || !ss || nvars < 1 || N < 1) return SetError(FBN_ERR_ARG, "Gaussian score: bad arguments");
    if (g->kind != FBN_GSCORE_LL && g->kind != FBN_GSCORE_BGE)
        return SetError(FBN_ERR_ARG, "score kind %d is neither FBN_GSCORE_LL nor FBN_GSCORE_BGE", g->kind);
    for (int v = 0; v < nvars; ++v)
        if (!(ss[v] > 0.0) || std::isinf(ss[v])) return SetError(FBN_ERR_ARG, "moments: ss[%d] = %g is not a positive number", v, ss[v]);
    GsPlan &P = *out;
    P.kind = g->kind == FBN_GSCORE_BGE ? kGsBGE : kGsLL;
    P.nvars = nvars, P.N = N;
    P.lss.assign((size_t)nvars, 0.0), P.tq.assign((size_t)nvars, 0.0);
    const long double Nl = (long double)N, lnN = std::log(Nl), pi = 3.141592653589793238462643383279502884L;
    for (int v = 0; v < nvars; ++v) P.lss[(size_t)v] = (double)(std::log((long double)ss[v]) - lnN);
    P.C = FbnGsConsts{};
    P.C.halfN = (double)N / 2;
    P.C.Kll = (double)(-(Nl / 2) * (std::log(2 * pi) + 1));
    if (P.kind == kGsLL) {
        if (!(g->penalty >= 0.0) || std::isinf(g->penalty))
            return SetError(FBN_ERR_ARG, "penalty = %g is not a non-negative number", g->penalty);
        for (int p = 0; p <= kGciMaxD; ++p) P.C.pen[p] = g->penalty * (double)(p + 2);
        return FBN_OK;
    }
    const double am = g->alpha_mu, aw = g->alpha_w == 0.0 ? (double)nvars + am + 1.0 : g->alpha_w;
    if (!(am > 0.0) || std::isinf(am)) return SetError(FBN_ERR_ARG, "alpha_mu = %g is not a positive number", am);
    if (!(aw > (double)nvars - 1.0) || std::isinf(aw))
        return SetError(FBN_ERR_ARG, "alpha_w = %g must exceed nvars - 1 = %d", aw, nvars - 1);
    const long double t = (long double)am * ((long double)aw - nvars - 1) / ((long double)am + 1);
    if (!(t > 0))
        return SetError(FBN_ERR_ARG, "alpha_w = %g leaves t = alpha_mu (alpha_w - nvars - 1) / (alpha_mu + 1) not positive", aw);
    for (int v = 0; v < nvars; ++v) P.tq[(size_t)v] = (double)(t / (long double)ss[v]);
    const long double c0 = (long double)aw - nvars, c = Nl + c0, lnt = std::log(t);
    for (int p = 0; p <= kGciMaxD; ++p) {
        const long double h = (c + p + 1) / 2;
        const long double K = -(Nl / 2) * std::log(pi) + std::log((long double)am / (Nl + am)) / 2 + std::lgamma(h) -
                              std::lgamma((c0 + p + 1) / 2) + ((c0 + 2 * p + 1) / 2) * lnt - ((long double)p / 2 + h) * lnN;
        P.C.K[p] = (double)K;
        P.C.h[p] = (double)h;
    }
    return FBN_OK;
}

int GsCheckBatch(int64_t N, const HcBatch &B) {
    for (int64_t f = 0; f < B.nfam; ++f) {
        const int64_t p = B.fam_off[f + 1] - B.fam_off[f] - 1;
        if (p > kGciMaxD)
            return SetError(FBN_ERR_LIMIT, "family %lld: %lld parents (supported up to %d)", (long long)f, (long long)p, kGciMaxD);
        if (N <= p + 2)
            return SetError(FBN_ERR_LIMIT, "family %lld: %lld samples, a regression on %lld parents needs more than %lld",
                            (long long)f, (long long)N, (long long)p, (long long)p + 2);
    }
    return FBN_OK;
}

int GsCheckFamilies(int nvars, int64_t N, int64_t nfam, const int64_t *fam_off, const int32_t *fam_cols, HcFamilies *out) {
    if (nvars < 1) return SetError(FBN_ERR_ARG, "bad arguments");
    const std::vector<int32_t> ones((size_t)nvars, 1);
    if (int rc = HcCheckFamilies(nvars, ones.data(), 0.0, nfam, fam_off, fam_cols, out)) return rc;
    return GsCheckBatch(N, out->batch());
}

namespace {

template <int P>
bool HostFamily(const GsPlan &G, const double *R, const int32_t *f, double *ll, double *sc) {
    const FbnGsFull get{R, G.nvars};
    return G.kind == kGsBGE ? fbn_gs_family<P, true>(get, f, G.lss.data(), G.tq.data(), G.C, ll, sc)
                            : fbn_gs_family<P, false>(get, f, G.lss.data(), G.tq.data(), G.C, ll, sc);
}

int CheckMoments(int nvars, int64_t N, const double *ss, const double *R) {
    if (nvars < 1 || N < 1 || !ss || !R) return SetError(FBN_ERR_ARG, "moments: bad arguments");
    for (int64_t i = 0; i < (int64_t)nvars * nvars; ++i)
        if (!std::isfinite(R[i])) return SetError(FBN_ERR_ARG, "R[%lld][%lld] is not finite", (long long)(i / nvars), (long long)(i % nvars));
    return FBN_OK;
}

}  // namespace

int GsHostBatch(const GsPlan &G, const double *R, const HcBatch &B, double *loglik, double *score, int64_t *degenerate) {
    if (int rc = GsCheckBatch(G.N, B)) return rc;
    for (int64_t f = 0; f < B.nfam; ++f) {
        const int32_t *fc = B.fam_cols + B.fam_off[f];
        double ll = 0.0, sc = 0.0;
        bool ok = false;
        switch ((int)(B.fam_off[f + 1] - B.fam_off[f]) - 1) {
        case 0: ok = HostFamily<0>(G, R, fc, &ll, &sc); break;
        case 1: ok = HostFamily<1>(G, R, fc, &ll, &sc); break;
        case 2: ok = HostFamily<2>(G, R, fc, &ll, &sc); break;
        case 3: ok = HostFamily<3>(G, R, fc, &ll, &sc); break;
        case 4: ok = HostFamily<4>(G, R, fc, &ll, &sc); break;
        case 5: ok = HostFamily<5>(G, R, fc, &ll, &sc); break;
        case 6: ok = HostFamily<6>(G, R, fc, &ll, &sc); break;
        case 7: ok = HostFamily<7>(G, R, fc, &ll, &sc); break;
        default: ok = HostFamily<8>(G, R, fc, &ll, &sc); break;
        }
        if (loglik) loglik[f] = ll;
        if (score) score[f] = sc;
        if (!ok && degenerate) ++*degenerate;
    }
    return FBN_OK;
}

int GsRunSearch(int nvars, const fbn_hc_options &opt, const HcScorer &scorer, fbn_hc_result *res) {
    if (nvars < 1) return SetError(FBN_ERR_ARG, "bad arguments");
    const std::vector<int32_t> ones((size_t)nvars, 1);
    fbn_hc_options o = opt;
    o.penalty = 0.0;  // the Gaussian score carries its own; pen[] is unread
    o.max_family_cells = 0;
    if (o.max_parents < 0 || o.max_parents > kGciMaxD) o.max_parents = kGciMaxD;
    if (o.start_off) {
        HcFamilies F;
        int64_t total = 0;
        if (int rc = ParamFamilySizes(nvars, ones.data(), o.start_off, o.start_parents, nullptr, &total)) return rc;
        F.off.assign(1, 0);
        for (int y = 0; y < nvars; ++y) {
            F.cols.push_back(y);
            F.cols.insert(F.cols.end(), o.start_parents + o.start_off[y], o.start_parents + o.start_off[y + 1]);
            std::sort(F.cols.end() - (o.start_off[y + 1] - o.start_off[y]), F.cols.end());
            F.off.push_back((int64_t)F.cols.size());
            F.cells.push_back(1);
            F.pen.push_back(0.0);
        }
        std::vector<double> sc((size_t)nvars);
        double ms = 0.0;
        if (int rc = scorer(F.batch(), nullptr, sc.data(), &ms)) return rc;
        for (int y = 0; y < nvars; ++y)
            if (std::isinf(sc[(size_t)y]))
                return SetError(FBN_ERR_ARG, "the starting graph's family of node %d is degenerate (its parents or the node are collinear)", y);
    }
    return HcSearch(nvars, ones.data(), o, scorer, res);
}

}  // namespace fbn

using fbn::SetError;

extern "C" {

int fbn_gscore_families_host(int nvars, int64_t nsamples, const double *ss, const double *R, const fbn_gauss_score *g,
                             int64_t nfam, const int64_t *fam_off, const int32_t *fam_cols, double *loglik, double *score,
                             int64_t *degenerate) {
    if (int rc = fbn::CheckMoments(nvars, nsamples, ss, R)) return rc;
    fbn::GsPlan G;
    if (int rc = fbn::GsMakePlan(g, nvars, nsamples, ss, &G)) return rc;
    fbn::HcFamilies F;
    if (int rc = fbn::GsCheckFamilies(nvars, nsamples, nfam, fam_off, fam_cols, &F)) return rc;
    int64_t deg = 0;
    if (int rc = fbn::GsHostBatch(G, R, F.batch(), loglik, score, &deg)) return rc;
    if (degenerate) *degenerate = deg;
    return FBN_OK;
}

int fbn_hc_run_gauss_host(int nvars, int64_t nsamples, const double *ss, const double *R, const fbn_hc_options *options,
                          const fbn_gauss_score *g, fbn_hc_result **out) {
    if (!options || !out) return SetError(FBN_ERR_ARG, "null pointer");
    if (int rc = fbn::CheckMoments(nvars, nsamples, ss, R)) return rc;
    fbn::GsPlan G;
    if (int rc = fbn::GsMakePlan(g, nvars, nsamples, ss, &G)) return rc;
    auto r = std::unique_ptr<fbn_hc_result>(new (std::nothrow) fbn_hc_result());
    if (!r) return SetError(FBN_ERR_NOMEM, "out of memory");
    fbn::HcScorer scorer = [&G, R](const fbn::HcBatch &B, double *loglik, double *score, double *) {
        return fbn::GsHostBatch(G, R, B, loglik, score, nullptr);
    };
    if (int rc = fbn::GsRunSearch(nvars, *options, scorer, r.get())) return rc;
    *out = r.release();
    return FBN_OK;
}

}  // extern "C"
