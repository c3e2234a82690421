// exact_bma_host.cpp -- exact arc posteriors, host side: the checks, the structure prior and the host twin of
// the lattice phases in plain loops over exact_lse.h (include/fastbn.h states the definitions).  No HIP: like
// exact_host.cpp it compiles on its own for host-side sanitizer runs.  The candidates are enumerated and
// scored by exact_host.cpp's ExactLocalScores, the code the exact search runs.
//
// The reference has no score-based learner, so nothing here restates reference code; the method is Koivisto
// & Sood's exact Bayesian structure discovery (JMLR 2004) with Koivisto's backward pass for all arcs at
// once (UAI 2006).
#include <memory>
#include <new>

#include "exact_bma.h"
#include "exact_lse.h"
#include "fbn_internal.h"
#include "hc_score.h"

namespace fbn {

int BmaCheck(int nvars, const int32_t *dims, const fbn_exact_options &opt, int prior) {
    if (prior != 0 && prior != 1) return SetError(FBN_ERR_ARG, "prior = %d: 0 (uniform) or 1 (indegree-uniform)", prior);
    if (nvars > kExactMaxVars)
        return SetError(FBN_ERR_LIMIT, "%d variables: the posterior lattices would take %.0f bytes (at most %d variables)", nvars,
                        BmaStateBytes(nvars), kExactMaxVars);
    return ExactCheck(nvars, dims, opt);
}

std::vector<double> BmaSizePrior(int n, int prior) {
    std::vector<double> lp;
    if (prior != 1) return lp;
    double c = 1.0;  // C(n - 1, k), an integer below 2^24: every product and quotient here is exact
    for (int k = 0; k < n; ++k) {
        lp.push_back(-fbn_bd_ln(c));
        c = c * (double)(n - 1 - k) / (double)(k + 1);
    }
    return lp;
}

int BmaOneVariable(const int32_t *dims, const fbn_exact_options &opt, const HcScorer &scorer, int prior, fbn_exact_info *xi,
                   fbn_bma_result *res) {
    double ls = 0.0;
    const std::vector<double> lp = BmaSizePrior(1, prior);
    if (int rc = ExactLocalScores(1, dims, opt, scorer, 0, &ls, xi, lp.empty() ? nullptr : lp.data())) return rc;
    res->info.log_z = res->info.b_full = ls;
    res->arc_prob.assign(1, 0.0);
    res->q_empty.assign(1, 1.0);
    return FBN_OK;
}

// the host twin: the lattices as plain arrays, plain bit sweeps, plain level loops
static int BmaRunHost(int n, const int32_t *dims, const fbn_exact_options &opt, int prior, const HcScorer &scorer,
                      fbn_bma_result *res) {
    const auto t_start = Clock::now();
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
    const int M = n - 1;
    const size_t L = (size_t)1 << M, NW = (size_t)1 << n;
    const uint32_t full = (uint32_t)(NW - 1);
    const std::vector<double> lp = BmaSizePrior(n, prior);
    std::vector<double> ls(L * n), X(L * n), Fw(NW), Bw(NW);
    for (int v = 0; v < n; ++v)
        if (int rc = ExactLocalScores(n, dims, opt, scorer, v, ls.data() + L * v, &xi, lp.empty() ? nullptr : lp.data())) return rc;
    BmaTakeScoring(xi, &info);

    auto t0 = Clock::now();
    X = ls;
    for (int v = 0; v < n; ++v) {  // alpha: the subset direction
        double *x = X.data() + L * v;
        for (int b = 0; b < M; ++b)
            for (size_t i = 0; i < L; ++i)
                if (i >> b & 1) x[i] = fbn_lse(x[i], x[i ^ ((size_t)1 << b)]);
    }
    info.alpha_wall_ms = MsSince(t0);

    t0 = Clock::now();
    Fw[0] = Bw[0] = 0.0;
    for (int k = 1; k <= n; ++k)
        for (uint32_t W = 1; W < NW; ++W) {
            if (__builtin_popcount(W) != k) continue;
            double f = 0.0, bk = 0.0;
            bool first = true;
            for (int v = 0; v < n; ++v) {
                if (!(W >> v & 1u)) continue;
                const uint32_t Wm = W ^ (1u << v);
                const double tf = Fw[Wm] + X[L * v + fbn_exact_squeeze(Wm, v)];
                const double tb = X[L * v + fbn_exact_squeeze(full ^ W, v)] + Bw[Wm];
                f = first ? tf : fbn_lse(f, tf);
                bk = first ? tb : fbn_lse(bk, tb);
                first = false;
            }
            Fw[W] = f, Bw[W] = bk;
        }
    info.level_wall_ms = MsSince(t0);
    const double logZ = Fw[full];
    info.log_z = logZ, info.b_full = Bw[full];

    t0 = Clock::now();
    for (int v = 0; v < n; ++v) {  // gamma, then Gamma: the superset direction
        double *x = X.data() + L * v;
        for (size_t i = 0; i < L; ++i) {
            const uint32_t U = fbn_exact_expand((uint32_t)i, v);
            x[i] = Fw[U] + Bw[full ^ U ^ (1u << v)];
        }
        for (int b = 0; b < M; ++b)
            for (size_t i = 0; i < L; ++i)
                if (!(i >> b & 1)) x[i] = fbn_lse(x[i], x[i | ((size_t)1 << b)]);
    }
    info.gamma_wall_ms = MsSince(t0);

    t0 = Clock::now();
    res->arc_prob.assign((size_t)n * n, 0.0);
    res->q_empty.assign((size_t)n, 0.0);
    for (int v = 0; v < n; ++v) {  // p, then q: the linear superset sum
        double *x = X.data() + L * v;
        const double *l = ls.data() + L * v;
        for (size_t i = 0; i < L; ++i) x[i] = fbn_lse_expm((l[i] + x[i]) - logZ);
        for (int b = 0; b < M; ++b)
            for (size_t i = 0; i < L; ++i)
                if (!(i >> b & 1)) x[i] = x[i] + x[i | ((size_t)1 << b)];
        res->q_empty[(size_t)v] = x[0];
        for (int u = 0; u < n; ++u)
            if (u != v) res->arc_prob[(size_t)u * n + v] = x[fbn_exact_squeeze(1u << u, v)];
    }
    info.q_wall_ms = MsSince(t0);
    info.wall_ms = MsSince(t_start);
    return FBN_OK;
}

}  // namespace fbn

using fbn::SetError;

extern "C" {

// fbn_bma_run_host (bd == nullptr) and fbn_bma_run_bd_host
static int BmaRunHostEntry(int nvars, const int32_t *dims, const uint8_t *cols, int64_t nsamples,
                           const fbn_exact_options *options, int32_t prior, const fbn_bd_score *bd, fbn_bma_result **out) {
    if (!options || !out) return SetError(FBN_ERR_ARG, "null pointer");
    if (int rc = fbn::BmaCheck(nvars, dims, *options, prior)) return rc;
    auto r = std::unique_ptr<fbn_bma_result>(new (std::nothrow) fbn_bma_result());
    if (!r) return SetError(FBN_ERR_NOMEM, "out of memory");
    if (int rc = fbn::WithHostScorer(nvars, dims, cols, nsamples, bd, [&](const fbn::HcScorer &scorer) {
            return fbn::BmaRunHost(nvars, dims, *options, prior, scorer, r.get());
        }))
        return rc;
    *out = r.release();
    return FBN_OK;
}

int fbn_bma_run_host(int nvars, const int32_t *dims, const uint8_t *cols, int64_t nsamples,
                     const fbn_exact_options *options, int32_t prior, fbn_bma_result **out) {
    return BmaRunHostEntry(nvars, dims, cols, nsamples, options, prior, nullptr, out);
}

int fbn_bma_run_bd_host(int nvars, const int32_t *dims, const uint8_t *cols, int64_t nsamples,
                        const fbn_exact_options *options, int32_t prior, const fbn_bd_score *bd, fbn_bma_result **out) {
    if (int rc = fbn::BdCheck(bd)) return rc;
    return BmaRunHostEntry(nvars, dims, cols, nsamples, options, prior, bd, out);
}

int fbn_bma_result_info(const fbn_bma_result *r, fbn_bma_info *info) {
    if (!r || !info) return SetError(FBN_ERR_ARG, "null pointer");
    *info = r->info;
    return FBN_OK;
}

int fbn_bma_result_arcs(const fbn_bma_result *r, double *arc_prob, double *q_empty) {
    if (!r) return SetError(FBN_ERR_ARG, "null pointer");
    if (arc_prob) std::copy(r->arc_prob.begin(), r->arc_prob.end(), arc_prob);
    if (q_empty) std::copy(r->q_empty.begin(), r->q_empty.end(), q_empty);
    return FBN_OK;
}

int fbn_bma_result_destroy(fbn_bma_result *r) {
    delete r;
    return FBN_OK;
}

int fbn_bma_lse_exp(double x, double *y) {
    if (!y || !(x <= 0.0)) return SetError(FBN_ERR_ARG, "fbn_bma_lse_exp: x <= 0 and an output");
    *y = fbn_lse_exp(x);
    return FBN_OK;
}

int fbn_bma_lse(double a, double b, double *y) {
    if (!y || a != a || b != b) return SetError(FBN_ERR_ARG, "fbn_bma_lse: two numbers and an output");
    *y = fbn_lse(a, b);
    return FBN_OK;
}

}  // extern "C"
