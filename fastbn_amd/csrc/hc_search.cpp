// hc_search.cpp -- score-based structure learning, host side: greedy hill climbing over arc additions,
// deletions and reversals under a decomposable score, and the host scorer that makes it the device
// path's twin.  No HIP and no other part of the library but param_learn.cpp's family sizing: it compiles
// on its own (with a main that supplies fbn::SetError) for host-side sanitizer runs (tools/hc_host_check.cpp).
//
// The reference has no score-based learner (its StructLearnCompData is PC-stable, src/PCStable.cpp), so
// nothing here restates reference code; the algorithm is the textbook one (Heckerman, Geiger &
// Chickering 1995; the default learner of bnlearn's hc and pgmpy's HillClimbSearch).
//
// Delta cache: for every node y and every other node x, cs[y][x] = the score of y's family with x
// toggled (added if it is no parent, removed if it is), where that family is admissible (allowed mask,
// max_parents, max_family_cells; cycles are checked when an operation is considered, since they depend
// on the rest of the graph).  A step reads deltas as cs[y][x] - fs[y] (fs = the current family scores; a
// reversal of x -> y: the delete delta in row y plus the add delta in row x), applies the best legal one
// and rescores the rows of the nodes whose parent set changed, in one scorer call.  The scorer is a
// callback; scores are compared as the exact doubles it returned, so a host and a device scorer that
// agree bit for bit walk the same path.  Ties: the scan runs in (type, head y, tail x) order and keeps
// the first maximum.
#include "hc_search.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <string>

#include "fbn_internal.h"
#include "hc_score.h"

namespace fbn {

int HcCheckSamples(int64_t nsamples) {
    if (nsamples < 1) return SetError(FBN_ERR_ARG, "score table: %lld samples", (long long)nsamples);
    if (nsamples > kHcMaxSamples)
        return SetError(FBN_ERR_LIMIT, "score table: %lld samples need %lld bytes (at most 2^24 samples)", (long long)nsamples,
                        (long long)(8 * (nsamples + 1)));
    return FBN_OK;
}

static int CheckDims(int nvars, const int32_t *dims) {
    if (nvars < 1 || !dims) return SetError(FBN_ERR_ARG, "bad arguments");
    for (int v = 0; v < nvars; ++v)
        if (dims[v] < 1 || dims[v] > 256) return SetError(FBN_ERR_ARG, "dims[%d] = %d out of 1..256", v, dims[v]);
    return FBN_OK;
}

static int CheckPenalty(double penalty) {
    if (!(penalty >= 0.0) || std::isinf(penalty)) return SetError(FBN_ERR_ARG, "penalty = %g is not a non-negative number", penalty);
    return FBN_OK;
}

int HcCheckFamilies(int nvars, const int32_t *dims, double penalty, int64_t nfam, const int64_t *fam_off,
                    const int32_t *fam_cols, HcFamilies *out) {
    if (int rc = CheckDims(nvars, dims)) return rc;
    if (int rc = CheckPenalty(penalty)) return rc;
    if (nfam < 0 || (nfam > 0 && (!fam_off || !fam_cols))) return SetError(FBN_ERR_ARG, "families: bad arguments");
    if (nfam > 0 && fam_off[0] != 0) return SetError(FBN_ERR_ARG, "families: fam_off[0] = %lld, not 0", (long long)fam_off[0]);
    const int64_t cap = FBN_PARAM_MAX_CELLS;
    out->off.assign(1, 0);
    out->cols.clear();
    out->cells.clear();
    out->pen.clear();
    std::vector<int64_t> seen((size_t)nvars, -1);  // seen[q] = f: q already listed in family f
    for (int64_t f = 0; f < nfam; ++f) {
        const int64_t a = fam_off[f], b = fam_off[f + 1];
        if (b <= a) return SetError(FBN_ERR_ARG, "family %lld: no child column", (long long)f);
        if (b - a > nvars) return SetError(FBN_ERR_ARG, "family %lld: more columns than variables", (long long)f);
        const int32_t v = fam_cols[a];
        if (v < 0 || v >= nvars) return SetError(FBN_ERR_ARG, "family %lld: child %d out of range", (long long)f, v);
        seen[v] = f;
        for (int64_t k = a + 1; k < b; ++k) {
            const int32_t q = fam_cols[k];
            if (q < 0 || q >= nvars) return SetError(FBN_ERR_ARG, "family %lld: parent %d out of range", (long long)f, q);
            if (q == v) return SetError(FBN_ERR_ARG, "family %lld: node %d is its own parent", (long long)f, v);
            if (seen[q] == f) return SetError(FBN_ERR_ARG, "family %lld: repeated parent %d", (long long)f, q);
            seen[q] = f;
        }
        // the whole list validated, then the product: cells <= cap before each multiply (factor <= 256)
        int64_t cells = dims[v];
        for (int64_t k = a + 1; k < b; ++k) {
            cells *= dims[fam_cols[k]];
            if (cells > cap)
                return SetError(FBN_ERR_LIMIT, "family %lld: more than %lld cells (the cap)", (long long)f, (long long)cap);
        }
        const size_t o = out->cols.size();
        out->cols.insert(out->cols.end(), fam_cols + a, fam_cols + b);
        std::sort(out->cols.begin() + o + 1, out->cols.end());
        out->off.push_back((int64_t)out->cols.size());
        out->cells.push_back(cells);
        out->pen.push_back(fbn_hc_penalty_term(penalty, dims[v], cells / dims[v]));
    }
    return FBN_OK;
}

static int CheckColumns(int nvars, const int32_t *dims, const uint8_t *cols, int64_t nsamples) {
    if (!cols) return SetError(FBN_ERR_ARG, "null column store");
    for (int v = 0; v < nvars; ++v) {
        const uint8_t *c = cols + (size_t)v * nsamples;
        for (int64_t s = 0; s < nsamples; ++s)
            if (c[s] >= dims[v])
                return SetError(FBN_ERR_ARG, "column store: variable %d holds a code >= its state count %d", v, dims[v]);
    }
    return FBN_OK;
}

HcScorer HcHostScorer(int nvars, const int32_t *dims, const uint8_t *cols, int64_t nsamples, const double *L) {
    (void)nvars;
    return [=](const HcBatch &B, double *loglik, double *score, double *kernel_ms) -> int {
        (void)kernel_ms;
        std::vector<uint32_t> tab;
        std::vector<int32_t> key((size_t)nsamples);
        for (int64_t f = 0; f < B.nfam; ++f) {
            const int32_t *fc = B.fam_cols + B.fam_off[f];
            const int ncol = (int)(B.fam_off[f + 1] - B.fam_off[f]);
            const int r = dims[fc[0]];
            const int q = (int)(B.cells[f] / r);
            tab.assign((size_t)B.cells[f], 0u);
            // keys as param_counts.hip forms them: the child's code x q, parent j's code x the product
            // of the later parents' state counts
            std::fill(key.begin(), key.end(), 0);
            int64_t str = 1;
            for (int j = ncol - 1; j >= 0; --j) {
                const int32_t st = j == 0 ? q : (int32_t)str;
                const uint8_t *c = cols + (size_t)fc[j] * nsamples;
                for (int64_t s = 0; s < nsamples; ++s) key[(size_t)s] += (int32_t)c[s] * st;
                if (j > 0) str *= dims[fc[j]];
            }
            for (int64_t s = 0; s < nsamples; ++s) ++tab[(size_t)key[(size_t)s]];
            double ll, sc;
            fbn_hc_family_host(tab.data(), r, q, L, B.pen[f], &ll, &sc);
            if (loglik) loglik[f] = ll;
            if (score) score[f] = sc;
        }
        return FBN_OK;
    };
}

namespace {

using Clock = std::chrono::steady_clock;
double MsSince(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

struct Search {
    int n;
    const int32_t *dims;
    const fbn_hc_options &opt;
    const HcScorer &scorer;
    int64_t cap;
    std::vector<std::vector<int32_t>> par, ch;  // ascending parents; children (unordered)
    std::vector<char> arc, has;                 // arc[x * n + y]: x -> y; has[y * n + x]: cs[y][x] is set
    std::vector<double> cs, cl, fs, fl;         // toggled-family score / loglik; current family score / loglik
    fbn_hc_info info{};
    std::vector<int32_t> stack_;
    std::vector<char> mark_;

    Search(int n_, const int32_t *d, const fbn_hc_options &o, const HcScorer &s)
        : n(n_), dims(d), opt(o), scorer(s), par(n_), ch(n_), arc((size_t)n_ * n_, 0), has((size_t)n_ * n_, 0),
          cs((size_t)n_ * n_, 0.0), cl((size_t)n_ * n_, 0.0), fs(n_, 0.0), fl(n_, 0.0) {
        cap = (opt.max_family_cells <= 0 || opt.max_family_cells > FBN_PARAM_MAX_CELLS) ? FBN_PARAM_MAX_CELLS : opt.max_family_cells;
    }

    // is `to` reachable from `from` along arcs, the arc skip_a -> skip_b left out
    bool Reach(int from, int to, int skip_a, int skip_b) {
        mark_.assign((size_t)n, 0);
        stack_.assign(1, from);
        mark_[(size_t)from] = 1;
        while (!stack_.empty()) {
            const int u = stack_.back();
            stack_.pop_back();
            if (u == to) return true;
            for (int w : ch[(size_t)u]) {
                if (u == skip_a && w == skip_b) continue;
                if (!mark_[(size_t)w]) mark_[(size_t)w] = 1, stack_.push_back(w);
            }
        }
        return false;
    }

    // cells of y's family with the parents ps, or limit + 1 once past `limit` (<= FBN_PARAM_MAX_CELLS, so
    // the product cannot wrap).  The option's cap limits candidate operations only: a current family --
    // the start's may exceed the cap -- is sized by its true count, which ParamFamilySizes has bounded.
    int64_t Cells(int y, const std::vector<int32_t> &ps, int64_t limit) const {
        int64_t c = dims[y];
        for (int32_t p : ps) {
            c *= dims[p];
            if (c > limit) return limit + 1;
        }
        return c;
    }

    // one scorer call: the current families of `base` and the rows of `rows`
    int Rescore(const std::vector<int> &base, const std::vector<int> &rows) {
        HcFamilies F;
        F.off.assign(1, 0);
        std::vector<std::pair<int, int>> target;  // (y, x) of a row entry, (y, -1) of a base family
        auto push = [&](int y, const std::vector<int32_t> &ps, int64_t cells, int x) {
            F.cols.push_back(y);
            F.cols.insert(F.cols.end(), ps.begin(), ps.end());
            F.off.push_back((int64_t)F.cols.size());
            F.cells.push_back(cells);
            F.pen.push_back(fbn_hc_penalty_term(opt.penalty, dims[y], cells / dims[y]));
            target.emplace_back(y, x);
        };
        for (int y : base) {
            const int64_t cells = Cells(y, par[(size_t)y], FBN_PARAM_MAX_CELLS);
            if (cells > FBN_PARAM_MAX_CELLS)
                return SetError(FBN_ERR_LIMIT, "node %d: its family has more than %lld cells (the cap)", y,
                                (long long)FBN_PARAM_MAX_CELLS);
            push(y, par[(size_t)y], cells, -1);
        }
        std::vector<int32_t> ps;
        for (int y : rows) {
            const std::vector<int32_t> &cur = par[(size_t)y];
            for (int x = 0; x < n; ++x) {
                if (x == y) continue;
                has[(size_t)y * n + x] = 0;
                ps = cur;
                if (arc[(size_t)x * n + y]) {
                    ps.erase(std::find(ps.begin(), ps.end(), x));
                } else {
                    if (opt.allowed && !opt.allowed[(size_t)x * n + y]) continue;
                    if (opt.max_parents >= 0 && (int64_t)cur.size() + 1 > opt.max_parents) continue;
                    ps.insert(std::upper_bound(ps.begin(), ps.end(), x), x);
                }
                const int64_t cells = Cells(y, ps, cap);
                if (cells > cap) continue;
                has[(size_t)y * n + x] = 1;
                push(y, ps, cells, x);
            }
        }
        const int64_t nf = (int64_t)F.cells.size();
        if (!nf) return FBN_OK;
        std::vector<double> ll((size_t)nf), sc((size_t)nf);
        const auto t0 = Clock::now();
        double ms = 0.0;
        if (int rc = scorer(F.batch(), ll.data(), sc.data(), &ms)) return rc;
        const double wall = MsSince(t0);
        if (info.batches == 0) info.first_sweep_kernel_ms = ms, info.first_sweep_wall_ms = wall;
        info.kernel_ms += ms;
        info.score_wall_ms += wall;
        info.batches += 1;
        info.families_scored += nf;
        for (int64_t f = 0; f < nf; ++f) {
            const int y = target[(size_t)f].first, x = target[(size_t)f].second;
            if (x < 0) fs[(size_t)y] = sc[(size_t)f], fl[(size_t)y] = ll[(size_t)f];
            else cs[(size_t)y * n + x] = sc[(size_t)f], cl[(size_t)y * n + x] = ll[(size_t)f];
        }
        return FBN_OK;
    }

    void SetArc(int x, int y, bool on) {
        arc[(size_t)x * n + y] = on;
        std::vector<int32_t> &p = par[(size_t)y], &c = ch[(size_t)x];
        if (on) {
            p.insert(std::upper_bound(p.begin(), p.end(), x), x);
            c.push_back(y);
        } else {
            p.erase(std::find(p.begin(), p.end(), x));
            c.erase(std::find(c.begin(), c.end(), y));
        }
    }

    // y's family becomes the cached one with x toggled
    void Toggle(int x, int y) {
        fs[(size_t)y] = cs[(size_t)y * n + x];
        fl[(size_t)y] = cl[(size_t)y * n + x];
        SetArc(x, y, !arc[(size_t)x * n + y]);
    }
};

}  // namespace

int HcSearch(int nvars, const int32_t *dims, const fbn_hc_options &opt, const HcScorer &scorer, fbn_hc_result *res) {
    if (int rc = CheckDims(nvars, dims)) return rc;
    if (int rc = CheckPenalty(opt.penalty)) return rc;
    const int n = nvars;
    if (opt.allowed && opt.allowed_len != (int64_t)n * n)
        return SetError(FBN_ERR_ARG, "allowed mask holds %lld entries, %lld (nvars x nvars) needed", (long long)opt.allowed_len,
                        (long long)n * n);
    const auto t_start = Clock::now();
    Search S(n, dims, opt, scorer);
    if (opt.start_off) {
        int64_t total = 0;
        if (int rc = ParamFamilySizes(n, dims, opt.start_off, opt.start_parents, nullptr, &total)) return rc;
        for (int y = 0; y < n; ++y)
            for (int32_t k = opt.start_off[y]; k < opt.start_off[y + 1]; ++k) S.SetArc(opt.start_parents[k], y, true);
        // Kahn: every node must come off
        std::vector<int> indeg((size_t)n), order;
        for (int y = 0; y < n; ++y) indeg[(size_t)y] = (int)S.par[(size_t)y].size();
        for (int y = 0; y < n; ++y)
            if (!indeg[(size_t)y]) order.push_back(y);
        for (size_t i = 0; i < order.size(); ++i)
            for (int w : S.ch[(size_t)order[i]])
                if (--indeg[(size_t)w] == 0) order.push_back(w);
        if ((int)order.size() != n) return SetError(FBN_ERR_ARG, "the starting graph has a directed cycle");
    }
    std::vector<int> all((size_t)n);
    for (int y = 0; y < n; ++y) all[(size_t)y] = y;
    if (int rc = S.Rescore(all, all)) return rc;  // the first sweep: every family and every row, one batch

    std::vector<int32_t> ops;
    std::vector<double> deltas;
    int iter = 0;
    for (; opt.max_iter < 0 || iter < opt.max_iter; ++iter) {
        double best = 0.0;
        int bt = -1, bx = -1, by = -1;
        // additions x -> y
        for (int y = 0; y < n; ++y)
            for (int x = 0; x < n; ++x) {
                if (x == y || S.arc[(size_t)x * n + y] || !S.has[(size_t)y * n + x]) continue;
                const double d = S.cs[(size_t)y * n + x] - S.fs[(size_t)y];
                if (d > best && !S.arc[(size_t)y * n + x] && !S.Reach(y, x, -1, -1)) best = d, bt = 0, bx = x, by = y;
            }
        // deletions of x -> y
        for (int y = 0; y < n; ++y)
            for (int32_t x : S.par[(size_t)y]) {
                if (!S.has[(size_t)y * n + x]) continue;
                const double d = S.cs[(size_t)y * n + x] - S.fs[(size_t)y];
                if (d > best) best = d, bt = 1, bx = x, by = y;
            }
        // reversals of x -> y into y -> x
        for (int y = 0; y < n; ++y)
            for (int32_t x : S.par[(size_t)y]) {
                if (!S.has[(size_t)y * n + x] || !S.has[(size_t)x * n + y]) continue;
                const double d = (S.cs[(size_t)y * n + x] - S.fs[(size_t)y]) + (S.cs[(size_t)x * n + y] - S.fs[(size_t)x]);
                if (d > best && !S.Reach(x, y, x, y)) best = d, bt = 2, bx = x, by = y;
            }
        if (bt < 0) break;
        ops.insert(ops.end(), {bt, bx, by});
        deltas.push_back(best);
        std::vector<int> rows{by};
        if (bt == 2) {
            S.Toggle(by, bx);  // add y -> x from row x, read before row y's arc goes
            S.Toggle(bx, by);
            rows.push_back(bx);
        } else {
            S.Toggle(bx, by);
        }
        if (int rc = S.Rescore({}, rows)) return rc;
    }
    res->info = S.info;
    res->info.nvars = n;
    res->info.iterations = iter;
    res->parent_off.assign(1, 0);
    res->parents.clear();
    double score = 0.0, loglik = 0.0;
    for (int y = 0; y < n; ++y) {
        res->parents.insert(res->parents.end(), S.par[(size_t)y].begin(), S.par[(size_t)y].end());
        res->parent_off.push_back((int32_t)res->parents.size());
        score += S.fs[(size_t)y];
        loglik += S.fl[(size_t)y];
    }
    res->info.narcs = (int32_t)res->parents.size();
    res->info.score = score;
    res->info.loglik = loglik;
    res->node_score = S.fs;
    res->node_loglik = S.fl;
    res->ops = std::move(ops);
    res->delta = std::move(deltas);
    res->info.wall_ms = MsSince(t_start);
    return FBN_OK;
}

}  // namespace fbn

using fbn::SetError;

extern "C" {

int fbn_hc_table_bytes(int64_t nsamples, int64_t *bytes) {
    if (int rc = fbn::HcCheckSamples(nsamples)) return rc;
    if (bytes) *bytes = 8 * (nsamples + 1);
    return FBN_OK;
}

int fbn_hc_penalty(const char *score, int64_t nsamples, double *penalty) {
    if (!score || !penalty || nsamples < 1) return SetError(FBN_ERR_ARG, "penalty: bad arguments");
    const std::string s = score;
    if (s == "bic") *penalty = log((double)nsamples) / 2;
    else if (s == "aic") *penalty = 1.0;
    else if (s == "loglik") *penalty = 0.0;
    else return SetError(FBN_ERR_ARG, "unknown score '%s' (bic, aic, loglik)", score);
    return FBN_OK;
}

int fbn_score_families_host(int nvars, const int32_t *dims, const uint8_t *cols, int64_t nsamples, double penalty,
                            int64_t nfam, const int64_t *fam_off, const int32_t *fam_cols, double *loglik,
                            double *score) {
    fbn::HcFamilies F;
    if (int rc = fbn::HcCheckFamilies(nvars, dims, penalty, nfam, fam_off, fam_cols, &F)) return rc;
    if (int rc = fbn::HcCheckSamples(nsamples)) return rc;
    if (int rc = fbn::CheckColumns(nvars, dims, cols, nsamples)) return rc;
    if (!nfam) return FBN_OK;
    std::vector<double> L((size_t)nsamples + 1);
    fbn_hc_fill_table(L.data(), nsamples);
    double ms = 0.0;
    return fbn::HcHostScorer(nvars, dims, cols, nsamples, L.data())(F.batch(), loglik, score, &ms);
}

int fbn_hc_run_host(int nvars, const int32_t *dims, const uint8_t *cols, int64_t nsamples,
                    const fbn_hc_options *options, fbn_hc_result **out) {
    if (!options || !out) return SetError(FBN_ERR_ARG, "null pointer");
    if (int rc = fbn::CheckDims(nvars, dims)) return rc;
    if (int rc = fbn::HcCheckSamples(nsamples)) return rc;
    if (int rc = fbn::CheckColumns(nvars, dims, cols, nsamples)) return rc;
    std::vector<double> L((size_t)nsamples + 1);
    fbn_hc_fill_table(L.data(), nsamples);
    auto r = std::unique_ptr<fbn_hc_result>(new (std::nothrow) fbn_hc_result());
    if (!r) return SetError(FBN_ERR_NOMEM, "out of memory");
    if (int rc = fbn::HcSearch(nvars, dims, *options, fbn::HcHostScorer(nvars, dims, cols, nsamples, L.data()), r.get()))
        return rc;
    *out = r.release();
    return FBN_OK;
}

int fbn_hc_result_info(const fbn_hc_result *r, fbn_hc_info *info) {
    if (!r || !info) return SetError(FBN_ERR_ARG, "null pointer");
    *info = r->info;
    return FBN_OK;
}

int fbn_hc_result_parents(const fbn_hc_result *r, int32_t *parent_off, int32_t *parents) {
    if (!r || !parent_off || (!parents && !r->parents.empty())) return SetError(FBN_ERR_ARG, "null pointer");
    std::copy(r->parent_off.begin(), r->parent_off.end(), parent_off);
    std::copy(r->parents.begin(), r->parents.end(), parents);
    return FBN_OK;
}

int fbn_hc_result_node_scores(const fbn_hc_result *r, double *score, double *loglik) {
    if (!r) return SetError(FBN_ERR_ARG, "null pointer");
    if (score) std::copy(r->node_score.begin(), r->node_score.end(), score);
    if (loglik) std::copy(r->node_loglik.begin(), r->node_loglik.end(), loglik);
    return FBN_OK;
}

int fbn_hc_result_trace(const fbn_hc_result *r, int32_t *ops, double *delta) {
    if (!r) return SetError(FBN_ERR_ARG, "null pointer");
    if (ops) std::copy(r->ops.begin(), r->ops.end(), ops);
    if (delta) std::copy(r->delta.begin(), r->delta.end(), delta);
    return FBN_OK;
}

int fbn_hc_result_destroy(fbn_hc_result *r) {
    delete r;
    return FBN_OK;
}

}  // extern "C"
