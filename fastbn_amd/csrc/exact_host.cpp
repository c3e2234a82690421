// exact_host.cpp -- exact score-optimal structure learning, host side: the phases the device path shares
// (candidate enumeration and scoring, the trace) and the host twin of the lattice phases in plain loops.
// No HIP: like hc_search.cpp it compiles on its own for host-side sanitizer runs.
//
// The reference has no score-based learner (its StructLearnCompData is PC-stable, src/PCStable.cpp), so
// nothing here restates reference code; the algorithm is Silander & Myllymaki's dynamic programme over
// variable subsets (UAI 2006), with the definitions and tie rules of include/fastbn.h.
#include <algorithm>
#include <cmath>
#include <limits>
#include <memory>
#include <new>

#include "exact_dp.h"
#include "fbn_internal.h"
#include "hc_score.h"

namespace fbn {

namespace {

constexpr int64_t kExactBatch = 1 << 15;  // families per scorer call

int64_t CellCap(const fbn_exact_options &opt) {
    return (opt.max_family_cells <= 0 || opt.max_family_cells > FBN_PARAM_MAX_CELLS) ? FBN_PARAM_MAX_CELLS : opt.max_family_cells;
}

// one scorer call, timed into info
int Score(const HcScorer &scorer, const HcFamilies &F, double *ll, double *sc, fbn_exact_info *info) {
    const auto t0 = Clock::now();
    double ms = 0.0;
    if (int rc = scorer(F.batch(), ll, sc, &ms)) return rc;
    info->score_wall_ms += MsSince(t0);
    info->score_kernel_ms += ms;
    info->batches += 1;
    info->families_scored += (int64_t)F.cells.size();
    return FBN_OK;
}

void Push(HcFamilies &F, const int32_t *dims, double penalty, int v, const int32_t *ps, int k, int64_t cells) {
    F.cols.push_back(v);
    F.cols.insert(F.cols.end(), ps, ps + k);
    F.off.push_back((int64_t)F.cols.size());
    F.cells.push_back(cells);
    F.pen.push_back(fbn_hc_penalty_term(penalty, dims[v], cells / dims[v]));
}

}  // namespace

int ExactCheck(int nvars, const int32_t *dims, const fbn_exact_options &opt) {
    HcFamilies none;
    if (int rc = HcCheckFamilies(nvars, dims, opt.penalty, 0, nullptr, nullptr, &none)) return rc;  // dims, penalty
    if (opt.allowed && opt.allowed_len != (int64_t)nvars * nvars)
        return SetError(FBN_ERR_ARG, "allowed mask holds %lld entries, %lld (nvars x nvars) needed", (long long)opt.allowed_len,
                        (long long)nvars * nvars);
    if (nvars > kExactMaxVars)
        return SetError(FBN_ERR_LIMIT, "%d variables: the subset lattices would take %.0f bytes (at most %d variables)", nvars,
                        ExactStateBytes(nvars), kExactMaxVars);
    return FBN_OK;
}

int ExactEnumerate(int n, const int32_t *dims, const fbn_exact_options &opt, const HcScorer *scorer, int v, fbn_exact_info *info,
                   const double *size_prior, const std::function<void(uint64_t, double)> &sink, int64_t *count) {
    const int64_t cap = CellCap(opt);
    std::vector<int32_t> others;
    for (int x = 0; x < n; ++x)
        if (x != v && (!opt.allowed || opt.allowed[(size_t)x * n + v])) others.push_back(x);
    const int m = (int)others.size(), kmax = opt.max_parents < 0 ? m : std::min<int>(opt.max_parents, m);
    HcFamilies F;
    F.off.assign(1, 0);
    std::vector<uint64_t> where;
    std::vector<double> sc;
    auto flush = [&]() -> int {
        if (F.cells.empty()) return FBN_OK;
        sc.resize(F.cells.size());
        if (int rc = Score(*scorer, F, nullptr, sc.data(), info)) return rc;
        for (size_t f = 0; f < where.size(); ++f)
            sink(where[f], size_prior ? sc[f] + size_prior[__builtin_popcountll(where[f])] : sc[f]);
        F.off.assign(1, 0);
        F.cols.clear(), F.cells.clear(), F.pen.clear(), where.clear();
        return FBN_OK;
    };
    std::vector<int> pos;
    std::vector<int32_t> ps;
    for (int k = 0; k <= kmax; ++k) {
        pos.resize((size_t)k);
        ps.resize((size_t)k);
        for (int i = 0; i < k; ++i) pos[(size_t)i] = i;
        for (;;) {  // the k-subsets of `others` in lexicographic order
            int64_t cells = dims[v];
            uint64_t S = 0;
            for (int i = 0; i < k; ++i) {
                ps[(size_t)i] = others[(size_t)pos[(size_t)i]];
                S |= (uint64_t)1 << ps[(size_t)i];
                if (cells <= cap) cells *= dims[ps[(size_t)i]];  // <= cap * 256: no wrap
            }
            if (cells <= cap || k == 0) {  // the empty set is always a candidate
                if (count) ++*count;
                if (scorer) {
                    Push(F, dims, opt.penalty, v, ps.data(), k, cells);
                    where.push_back(S);
                    if ((int64_t)where.size() == kExactBatch)
                        if (int rc = flush()) return rc;
                }
            }
            int i = k - 1;
            while (i >= 0 && pos[(size_t)i] == m - k + i) --i;
            if (i < 0) break;
            ++pos[(size_t)i];
            for (int j = i + 1; j < k; ++j) pos[(size_t)j] = pos[(size_t)j - 1] + 1;
        }
    }
    return scorer ? flush() : FBN_OK;
}

int ExactLocalScores(int n, const int32_t *dims, const fbn_exact_options &opt, const HcScorer &scorer, int v, double *ls,
                     fbn_exact_info *info, const double *size_prior) {
    std::fill(ls, ls + ((size_t)1 << (n - 1)), -std::numeric_limits<double>::infinity());
    // squeezing keeps the size: the prior's term was chosen by the parents' number
    return ExactEnumerate(n, dims, opt, &scorer, v, info, size_prior,
                          [&](uint64_t S, double score) { ls[fbn_exact_squeeze((uint32_t)S, v)] = score; }, nullptr);
}

int ExactTrace(int n, const int32_t *dims, const fbn_exact_options &opt, const HcScorer &scorer, const uint8_t *sink,
               const std::function<int(int, uint32_t, uint32_t *)> &arg_at, double RV, fbn_exact_info *info,
               fbn_hc_result *res) {
    std::vector<std::vector<int32_t>> par((size_t)n);
    uint32_t W = n >= 32 ? ~0u : (1u << n) - 1u;
    while (W) {
        const int v = sink ? sink[W] : 0;  // no table: the single variable
        if (v >= n || !(W >> v & 1u)) return SetError(FBN_ERR_HIP, "exact search: sink table entry %u is %d", W, v);
        W ^= 1u << v;
        uint32_t a = 0;
        if (n > 1)
            if (int rc = arg_at(v, fbn_exact_squeeze(W, v), &a)) return rc;
        const uint32_t S = fbn_exact_expand(a, v);
        if (S & ~W) return SetError(FBN_ERR_HIP, "exact search: parent set %u of %d leaves its candidate set %u", S, v, W);
        for (int x = 0; x < n; ++x)
            if (S >> x & 1u) par[(size_t)v].push_back(x);
    }
    HcFamilies F;
    F.off.assign(1, 0);
    for (int v = 0; v < n; ++v) {
        int64_t cells = dims[v];
        for (int32_t p : par[(size_t)v]) cells *= dims[p];  // a candidate (or empty): within the cap
        Push(F, dims, opt.penalty, v, par[(size_t)v].data(), (int)par[(size_t)v].size(), cells);
    }
    res->node_score.assign((size_t)n, 0.0);
    res->node_loglik.assign((size_t)n, 0.0);
    if (int rc = Score(scorer, F, res->node_loglik.data(), res->node_score.data(), info)) return rc;
    res->parent_off.assign(1, 0);
    res->parents.clear();
    double loglik = 0.0;
    for (int v = 0; v < n; ++v) {
        res->parents.insert(res->parents.end(), par[(size_t)v].begin(), par[(size_t)v].end());
        res->parent_off.push_back((int32_t)res->parents.size());
        loglik += res->node_loglik[(size_t)v];
    }
    res->ops.clear();
    res->delta.clear();
    res->info = fbn_hc_info{};
    res->info.nvars = n;
    res->info.narcs = (int32_t)res->parents.size();
    res->info.iterations = 0;
    res->info.families_scored = info->families_scored;
    res->info.batches = info->batches;
    res->info.score = RV;
    res->info.loglik = loglik;
    res->info.kernel_ms = info->score_kernel_ms;
    res->info.score_wall_ms = info->score_wall_ms;
    return FBN_OK;
}

// the host twin: the lattices as plain arrays, plain bit sweeps, plain level loops
static int ExactRunHost(int n, const int32_t *dims, const fbn_exact_options &opt, const HcScorer &scorer, fbn_hc_result *res) {
    const auto t_start = Clock::now();
    fbn_exact_info info{};
    info.nvars = n;
    info.levels = n + 1;
    info.lattice_bytes = (int64_t)ExactStateBytes(n);
    const int M = n - 1;
    const size_t L = (size_t)1 << M, NW = (size_t)1 << n;
    std::vector<double> val, R;
    std::vector<uint32_t> arg;
    std::vector<uint8_t> sink;
    if (n > 1) {
        val.resize(L * n), arg.resize(L * n), R.resize(NW), sink.resize(NW);
        for (int v = 0; v < n; ++v)
            if (int rc = ExactLocalScores(n, dims, opt, scorer, v, val.data() + L * v, &info)) return rc;
        auto t0 = Clock::now();
        for (int v = 0; v < n; ++v) {
            double *x = val.data() + L * v;
            uint32_t *a = arg.data() + L * v;
            for (size_t i = 0; i < L; ++i) a[i] = (uint32_t)i;
            for (int b = 0; b < M; ++b)
                for (size_t i = 0; i < L; ++i)
                    if ((i >> b & 1) && x[i ^ ((size_t)1 << b)] > x[i]) x[i] = x[i ^ ((size_t)1 << b)], a[i] = a[i ^ ((size_t)1 << b)];
        }
        info.transform_wall_ms = MsSince(t0);
        t0 = Clock::now();
        R[0] = 0.0, sink[0] = 0xFF;
        for (int k = 1; k <= n; ++k)
            for (uint32_t W = 1; W < NW; ++W) {
                if (__builtin_popcount(W) != k) continue;
                double best = 0.0;
                int bv = -1;
                for (int v = 0; v < n; ++v) {
                    if (!(W >> v & 1u)) continue;
                    const uint32_t Wm = W ^ (1u << v);
                    const double cand = R[Wm] + val[L * v + fbn_exact_squeeze(Wm, v)];
                    if (bv < 0 || cand > best) best = cand, bv = v;
                }
                R[W] = best, sink[W] = (uint8_t)bv;
            }
        info.sink_wall_ms = MsSince(t0);
    }
    const auto t0 = Clock::now();
    auto arg_at = [&](int v, uint32_t i, uint32_t *a) {
        *a = arg[L * v + i];
        return FBN_OK;
    };
    if (int rc = ExactTrace(n, dims, opt, scorer, n > 1 ? sink.data() : nullptr, arg_at, n > 1 ? R[NW - 1] : 0.0, &info, res))
        return rc;
    if (n == 1) res->info.score = res->node_score[0];
    info.trace_wall_ms = MsSince(t0);
    info.wall_ms = res->info.wall_ms = MsSince(t_start);
    res->exact = info;
    return FBN_OK;
}

}  // namespace fbn

using fbn::SetError;

extern "C" {

// fbn_exact_run_host (bd == nullptr) and fbn_exact_run_bd_host
static int ExactRunHostEntry(int nvars, const int32_t *dims, const uint8_t *cols, int64_t nsamples,
                             const fbn_exact_options *options, const fbn_bd_score *bd, fbn_hc_result **out) {
    if (!options || !out) return SetError(FBN_ERR_ARG, "null pointer");
    if (int rc = fbn::ExactCheck(nvars, dims, *options)) return rc;
    auto r = std::unique_ptr<fbn_hc_result>(new (std::nothrow) fbn_hc_result());
    if (!r) return SetError(FBN_ERR_NOMEM, "out of memory");
    if (int rc = fbn::WithHostScorer(nvars, dims, cols, nsamples, bd, [&](const fbn::HcScorer &scorer) {
            return fbn::ExactRunHost(nvars, dims, *options, scorer, r.get());
        }))
        return rc;
    *out = r.release();
    return FBN_OK;
}

int fbn_exact_run_host(int nvars, const int32_t *dims, const uint8_t *cols, int64_t nsamples,
                       const fbn_exact_options *options, fbn_hc_result **out) {
    return ExactRunHostEntry(nvars, dims, cols, nsamples, options, nullptr, out);
}

int fbn_exact_run_bd_host(int nvars, const int32_t *dims, const uint8_t *cols, int64_t nsamples,
                          const fbn_exact_options *options, const fbn_bd_score *bd, fbn_hc_result **out) {
    if (int rc = fbn::BdCheck(bd)) return rc;
    return ExactRunHostEntry(nvars, dims, cols, nsamples, options, bd, out);
}

int fbn_exact_result_info(const fbn_hc_result *r, fbn_exact_info *info) {
    if (!r || !info) return SetError(FBN_ERR_ARG, "null pointer");
    if (!r->exact.nvars) return SetError(FBN_ERR_ARG, "not a result of the exact search");
    *info = r->exact;
    return FBN_OK;
}

}  // extern "C"
