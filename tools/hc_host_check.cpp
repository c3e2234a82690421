// hc_host_check.cpp -- stand-alone driver of fastbn_amd/csrc/hc_search.cpp (with param_learn.cpp's family
// sizing) for host sanitizer runs (no device, no libfastbn, never loaded into Python):
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -Iinclude \
//       tools/hc_host_check.cpp fastbn_amd/csrc/hc_search.cpp fastbn_amd/csrc/param_learn.cpp \
//       -o hc_host_check && ./hc_host_check
// Runs the score, validation, option, error and tie cases of tests/test_hc_host.py on data generated here,
// plus seeded random datasets under random options: whatever the search returns is acyclic, ascending,
// within its limits, the replay of its own trace, repeatable, and a local optimum under the scorer's own
// bits.  Exits non-zero on a wrong answer.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../fastbn_amd/csrc/fbn_internal.h"

namespace fbn {
static char g_msg[512];
int SetError(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof g_msg, fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace fbn

static int g_fail = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            printf("FAIL %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, fbn::g_msg); \
            ++g_fail;                                                    \
        }                                                                \
    } while (0)

using Lists = std::vector<std::vector<int32_t>>;

struct Data {
    std::vector<int32_t> dims;
    std::vector<uint8_t> cols;  // [var][sample]
    int64_t N = 0;
    int n() const { return (int)dims.size(); }
};

struct Run {
    int rc = 0;
    fbn_hc_info info{};
    Lists parents;
    std::vector<int32_t> ops;
    std::vector<double> delta, node;
};

static Run Climb(const Data &d, fbn_hc_options opt) {
    Run r;
    fbn_hc_result *res = nullptr;
    r.rc = fbn_hc_run_host(d.n(), d.dims.data(), d.cols.data(), d.N, &opt, &res);
    if (r.rc) return r;
    fbn_hc_result_info(res, &r.info);
    std::vector<int32_t> off((size_t)d.n() + 1), par((size_t)std::max(1, r.info.narcs));
    fbn_hc_result_parents(res, off.data(), par.data());
    r.parents.assign((size_t)d.n(), {});
    for (int v = 0; v < d.n(); ++v) r.parents[(size_t)v].assign(par.begin() + off[v], par.begin() + off[v + 1]);
    r.ops.resize((size_t)r.info.iterations * 3 + 1);
    r.delta.resize((size_t)r.info.iterations + 1);
    r.node.resize((size_t)d.n());
    fbn_hc_result_trace(res, r.ops.data(), r.delta.data());
    fbn_hc_result_node_scores(res, r.node.data(), nullptr);
    fbn_hc_result_destroy(res);
    return r;
}

static int Scores(const Data &d, double pen, const Lists &fams, std::vector<double> *ll, std::vector<double> *sc) {
    std::vector<int64_t> off{0};
    std::vector<int32_t> cols;
    for (auto &f : fams) {
        cols.insert(cols.end(), f.begin(), f.end());
        off.push_back((int64_t)cols.size());
    }
    ll->assign(fams.size() + 1, 0.0);
    sc->assign(fams.size() + 1, 0.0);
    return fbn_score_families_host(d.n(), d.dims.data(), d.cols.data(), d.N, pen, (int64_t)fams.size(), off.data(),
                                   cols.empty() ? nullptr : cols.data(), ll->data(), sc->data());
}

// the score of one family in long double, table by std::vector, straight from the definition
static void Plain(const Data &d, double pen, const std::vector<int32_t> &fam, double *ll, double *mag) {
    std::vector<int32_t> ps(fam.begin() + 1, fam.end());
    std::sort(ps.begin(), ps.end());
    int64_t q = 1;
    for (int p : ps) q *= d.dims[(size_t)p];
    const int r = d.dims[(size_t)fam[0]];
    std::vector<int64_t> t((size_t)(r * q), 0);
    for (int64_t s = 0; s < d.N; ++s) {
        int64_t j = 0;
        for (int p : ps) j = j * d.dims[(size_t)p] + d.cols[(size_t)p * d.N + s];
        ++t[(size_t)(d.cols[(size_t)fam[0] * d.N + s] * q + j)];
    }
    long double a = 0, b = 0;
    for (int64_t j = 0; j < q; ++j) {
        int64_t nj = 0;
        for (int k = 0; k < r; ++k) {
            const int64_t c = t[(size_t)(k * q + j)];
            nj += c;
            if (c) a += (long double)c * logl((long double)c);
        }
        if (nj) b += (long double)nj * logl((long double)nj);
    }
    (void)pen;
    *ll = (double)(a - b);
    *mag = (double)(a + b);
}

static bool Acyclic(const Lists &par) {
    const int n = (int)par.size();
    std::vector<int> indeg((size_t)n), order;
    Lists ch((size_t)n);
    for (int v = 0; v < n; ++v) {
        indeg[(size_t)v] = (int)par[(size_t)v].size();
        for (int q : par[(size_t)v]) ch[(size_t)q].push_back(v);
    }
    for (int v = 0; v < n; ++v)
        if (!indeg[(size_t)v]) order.push_back(v);
    for (size_t i = 0; i < order.size(); ++i)
        for (int c : ch[(size_t)order[i]])
            if (--indeg[(size_t)c] == 0) order.push_back(c);
    return (int)order.size() == n;
}

static Lists With(const Lists &par, int y, int x, bool on) {
    Lists p = par;
    auto &l = p[(size_t)y];
    if (on) l.insert(std::upper_bound(l.begin(), l.end(), x), x);
    else l.erase(std::find(l.begin(), l.end(), x));
    return p;
}

static std::vector<int32_t> Fam(const Lists &par, int y) {
    std::vector<int32_t> f{y};
    f.insert(f.end(), par[(size_t)y].begin(), par[(size_t)y].end());
    return f;
}

// no legal single operation improves, under the scorer's own bits and the search's own expressions
static void CheckLocalOptimum(const Data &d, const fbn_hc_options &opt, const Run &r) {
    const int n = d.n();
    std::vector<double> ll, fs, ns;
    Lists base;
    for (int y = 0; y < n; ++y) base.push_back(Fam(r.parents, y));
    CHECK(Scores(d, opt.penalty, base, &ll, &fs) == 0);
    for (int y = 0; y < n; ++y) CHECK(fs[(size_t)y] == r.node[(size_t)y]);
    const int64_t cap = opt.max_family_cells > 0 ? opt.max_family_cells : FBN_PARAM_MAX_CELLS;
    auto cells = [&](const std::vector<int32_t> &f) {
        int64_t c = 1;
        for (int v : f) c *= d.dims[(size_t)v];
        return c;
    };
    auto addable = [&](const Lists &par, int x, int y) {
        if (opt.allowed && !opt.allowed[(size_t)x * n + y]) return false;
        if (opt.max_parents >= 0 && (int)par[(size_t)y].size() + 1 > opt.max_parents) return false;
        return true;
    };
    for (int y = 0; y < n; ++y)
        for (int x = 0; x < n; ++x) {
            if (x == y) continue;
            const bool has = std::binary_search(r.parents[(size_t)y].begin(), r.parents[(size_t)y].end(), x);
            if (!has) {
                if (!addable(r.parents, x, y)) continue;
                const Lists p = With(r.parents, y, x, true);
                if (!Acyclic(p) || cells(Fam(p, y)) > cap) continue;
                CHECK(Scores(d, opt.penalty, {Fam(p, y)}, &ll, &ns) == 0);
                CHECK(!(ns[0] - fs[(size_t)y] > 0));
            } else {
                const Lists p = With(r.parents, y, x, false);
                if (cells(Fam(p, y)) > cap) continue;
                CHECK(Scores(d, opt.penalty, {Fam(p, y)}, &ll, &ns) == 0);
                const double dd = ns[0] - fs[(size_t)y];
                CHECK(!(dd > 0));
                if (!addable(r.parents, y, x)) continue;
                const Lists p2 = With(p, x, y, true);
                if (!Acyclic(p2) || cells(Fam(p2, x)) > cap) continue;
                std::vector<double> ns2;
                CHECK(Scores(d, opt.penalty, {Fam(p2, x)}, &ll, &ns2) == 0);
                CHECK(!(dd + (ns2[0] - fs[(size_t)x]) > 0));
            }
        }
}

static void CheckRun(const Data &d, const fbn_hc_options &opt, const Run &r, const Lists &start) {
    CHECK(r.rc == 0);
    if (r.rc) return;
    CHECK(Acyclic(r.parents));
    Lists replay = start.empty() ? Lists((size_t)d.n()) : start;
    for (auto &l : replay) std::sort(l.begin(), l.end());
    for (int k = 0; k < r.info.iterations; ++k) {
        const int t = r.ops[(size_t)k * 3], x = r.ops[(size_t)k * 3 + 1], y = r.ops[(size_t)k * 3 + 2];
        CHECK(r.delta[(size_t)k] > 0);
        CHECK(t >= 0 && t <= 2);
        if (t == 0) {
            CHECK(!opt.allowed || opt.allowed[(size_t)x * d.n() + y]);
            CHECK(opt.max_parents < 0 || (int)replay[(size_t)y].size() < opt.max_parents);
            replay = With(replay, y, x, true);
        } else {
            replay = With(replay, y, x, false);
            if (t == 2) {
                CHECK(!opt.allowed || opt.allowed[(size_t)y * d.n() + x]);
                replay = With(replay, x, y, true);
            }
        }
        CHECK(Acyclic(replay));
    }
    CHECK(replay == r.parents);
    CHECK(opt.max_iter < 0 || r.info.iterations <= opt.max_iter);
    int narcs = 0;
    for (auto &l : r.parents) {
        CHECK(std::is_sorted(l.begin(), l.end()));
        narcs += (int)l.size();
    }
    CHECK(narcs == r.info.narcs);
    if (opt.max_iter < 0) CheckLocalOptimum(d, opt, r);
}

static Data Random(std::mt19937 &rng, int n, int64_t N, int maxdim) {
    Data d;
    d.N = N;
    for (int v = 0; v < n; ++v) d.dims.push_back(1 + (int)(rng() % maxdim));
    d.cols.resize((size_t)n * N);
    for (int v = 0; v < n; ++v)
        for (int64_t s = 0; s < N; ++s) {
            int c = (int)(rng() % d.dims[(size_t)v]);
            if (v > 0 && rng() % 100 < 60) c = d.cols[(size_t)(rng() % v) * N + s] % d.dims[(size_t)v];  // dependence
            d.cols[(size_t)v * N + s] = (uint8_t)c;
        }
    return d;
}

int main() {
    std::mt19937 rng(2024);
    std::vector<double> ll, sc;
    fbn_hc_options none{};
    none.max_parents = -1;
    none.max_iter = -1;
    // ---- sizing, penalties
    int64_t bytes = 0;
    double pen = 0;
    CHECK(fbn_hc_table_bytes(5000, &bytes) == 0 && bytes == 8 * 5001);
    CHECK(fbn_hc_table_bytes(((int64_t)1 << 24) + 1, &bytes) == FBN_ERR_LIMIT);
    CHECK(fbn_hc_table_bytes(0, &bytes) == FBN_ERR_ARG);
    CHECK(fbn_hc_penalty("bic", 5000, &pen) == 0 && pen == log(5000.0) / 2);
    CHECK(fbn_hc_penalty("aic", 5000, &pen) == 0 && pen == 1.0);
    CHECK(fbn_hc_penalty("loglik", 5000, &pen) == 0 && pen == 0.0);
    CHECK(fbn_hc_penalty("bdeu", 5000, &pen) == FBN_ERR_ARG);
    // ---- scores against the definition; validation
    for (int64_t N : {1, 15, 1003}) {
        Data d = Random(rng, 7, N, 70);
        d.dims[1] = 1;
        std::fill(d.cols.begin() + N, d.cols.begin() + 2 * N, (uint8_t)0);
        const Lists fams{{0}, {1}, {2, 0}, {0, 1}, {1, 3}, {3, 6, 5}, {4, 2, 0, 1}, {5, 4}, {6, 5, 4}};
        CHECK(Scores(d, 0.75, fams, &ll, &sc) == 0);
        for (size_t f = 0; f < fams.size(); ++f) {
            double pl, mag;
            Plain(d, 0.75, fams[f], &pl, &mag);
            CHECK(fabs(ll[f] - pl) <= 1e-12 * mag);
            int64_t q = 1;
            for (size_t k = 1; k < fams[f].size(); ++k) q *= d.dims[(size_t)fams[f][k]];
            CHECK(sc[f] == ll[f] - 0.75 * (double)((d.dims[(size_t)fams[f][0]] - 1) * q));
        }
        std::vector<double> l1, s1;
        CHECK(Scores(d, 0.75, {{3, 5, 6}, {0}, {3, 6, 5}}, &l1, &s1) == 0 && l1[0] == ll[5] && l1[2] == ll[5] && s1[0] == sc[5]);
        CHECK(Scores(d, 0.0, {{}}, &ll, &sc) == FBN_ERR_ARG);
        CHECK(Scores(d, 0.0, {{7}}, &ll, &sc) == FBN_ERR_ARG);
        CHECK(Scores(d, 0.0, {{0, 7}}, &ll, &sc) == FBN_ERR_ARG);
        CHECK(Scores(d, 0.0, {{0, 0}}, &ll, &sc) == FBN_ERR_ARG);
        CHECK(Scores(d, 0.0, {{0, 2, 2}}, &ll, &sc) == FBN_ERR_ARG);
        CHECK(Scores(d, -1.0, {{0}}, &ll, &sc) == FBN_ERR_ARG);
        CHECK(Scores(d, NAN, {{0}}, &ll, &sc) == FBN_ERR_ARG);
        CHECK(Scores(d, 0.0, {}, &ll, &sc) == 0);
    }
    {
        Data d;  // 256^4 cells
        d.N = 4;
        d.dims.assign(4, 256);
        d.cols.assign(16, 0);
        CHECK(Scores(d, 0.0, {{0, 1, 2, 3}}, &ll, &sc) == FBN_ERR_LIMIT);
        d.cols[5] = 255;
        d.dims[1] = 255;  // a code >= its state count
        CHECK(Scores(d, 0.0, {{0}}, &ll, &sc) == FBN_ERR_ARG);
        CHECK(Climb(d, none).rc == FBN_ERR_ARG);
    }
    // ---- exact ties: columns 0 and 1 identical, 2 a noisy copy
    {
        Data d;
        d.N = 600;
        d.dims.assign(3, 3);
        d.cols.resize(3 * 600);
        for (int s = 0; s < 600; ++s) {
            const uint8_t a = (uint8_t)(rng() % 3);
            d.cols[(size_t)s] = d.cols[(size_t)600 + s] = a;
            d.cols[(size_t)1200 + s] = rng() % 100 < 70 ? a : (uint8_t)(rng() % 3);
        }
        fbn_hc_options o = none;
        CHECK(fbn_hc_penalty("bic", d.N, &o.penalty) == 0);
        CHECK(Scores(d, o.penalty, {{0, 1}, {1, 0}, {0}, {1}, {2, 0}, {2, 1}}, &ll, &sc) == 0);
        CHECK(sc[0] == sc[1] && sc[2] == sc[3] && sc[4] == sc[5]);
        const Run r = Climb(d, o);
        CheckRun(d, o, r, {});
        CHECK(r.info.iterations >= 2 && r.ops[0] == 0 && r.ops[1] == 1 && r.ops[2] == 0 && r.delta[0] == sc[0] - sc[2]);
        for (int k = 0; k < r.info.iterations; ++k) CHECK(!(r.ops[(size_t)3 * k] == 0 && r.ops[(size_t)3 * k + 1] == 1 && r.ops[(size_t)3 * k + 2] == 2));
    }
    // ---- errors of the search
    {
        Data d = Random(rng, 5, 200, 3);
        fbn_hc_options o = none;
        o.penalty = -0.5;
        CHECK(Climb(d, o).rc == FBN_ERR_ARG);
        o.penalty = 1.0;
        std::vector<uint8_t> mask(25, 1);
        o.allowed = mask.data();
        o.allowed_len = 20;
        CHECK(Climb(d, o).rc == FBN_ERR_ARG);
        o.allowed_len = 25;
        CHECK(Climb(d, o).rc == 0);
        const std::vector<int32_t> off{0, 1, 2, 3, 3, 3}, cyc{1, 2, 0}, self{0, 2, 0}, far{9, 2, 0};
        o.start_off = off.data();
        o.start_parents = cyc.data();
        CHECK(Climb(d, o).rc == FBN_ERR_ARG);
        o.start_parents = self.data();
        CHECK(Climb(d, o).rc == FBN_ERR_ARG);
        o.start_parents = far.data();
        CHECK(Climb(d, o).rc == FBN_ERR_ARG);
        fbn_hc_result *res = nullptr;
        CHECK(fbn_hc_run_host(5, d.dims.data(), d.cols.data(), ((int64_t)1 << 24) + 1, &none, &res) == FBN_ERR_LIMIT);
        CHECK(fbn_hc_run_host(5, d.dims.data(), nullptr, 200, &none, &res) == FBN_ERR_ARG);
    }
    // ---- a start family above max_family_cells: 27 cells against a cap of 12 (and of 2: nothing admissible)
    {
        const Data d = Random(rng, 3, 500, 1);
        Data e = d;
        e.dims.assign(3, 3);
        for (int s = 0; s < 500; ++s) {
            e.cols[(size_t)s] = (uint8_t)(rng() % 3);
            e.cols[(size_t)500 + s] = (uint8_t)(rng() % 3);
            e.cols[(size_t)1000 + s] = rng() % 100 < 80 ? (uint8_t)((e.cols[(size_t)s] + e.cols[(size_t)500 + s]) % 3) : (uint8_t)(rng() % 3);
        }
        const std::vector<int32_t> off{0, 0, 0, 2}, par{0, 1};
        const Lists start{{}, {}, {0, 1}};
        for (int64_t cells : {12, 2, 27, 0}) {
            fbn_hc_options o = none;
            CHECK(fbn_hc_penalty("bic", e.N, &o.penalty) == 0);
            o.max_family_cells = cells;
            o.start_off = off.data();
            o.start_parents = par.data();
            const Run r = Climb(e, o);
            CheckRun(e, o, r, start);
            fbn_hc_options z = o;
            z.max_iter = 0;
            const Run r0 = Climb(e, z);
            CHECK(r0.rc == 0 && r0.parents == start);
            CHECK(Scores(e, o.penalty, {{2, 0, 1}}, &ll, &sc) == 0 && r0.node[2] == sc[0]);  // the true 27-cell table
            if (cells == 2) CHECK(r.info.iterations == 0);
        }
    }
    // ---- seeded random data under random options
    int64_t ops = 0;
    for (int it = 0; it < 60; ++it) {
        const int n = 2 + (int)(rng() % 7);
        const Data d = Random(rng, n, 1 + (int64_t)(rng() % 400), 1 + (int)(rng() % 5));
        fbn_hc_options o = none;
        const char *names[] = {"bic", "aic", "loglik"};
        CHECK(fbn_hc_penalty(names[rng() % 3], d.N, &o.penalty) == 0);
        if (rng() % 3 == 0) o.max_parents = (int)(rng() % 3);
        if (rng() % 4 == 0) o.max_iter = (int)(rng() % 6);
        if (rng() % 3 == 0) o.max_family_cells = 4 + (int64_t)(rng() % 60);
        std::vector<uint8_t> mask((size_t)n * n, 1);
        if (rng() % 2) {
            for (auto &m : mask) m = rng() % 100 < 70;
            o.allowed = mask.data();
            o.allowed_len = (int64_t)mask.size();
        }
        Lists start;
        std::vector<int32_t> soff{0}, spar;
        if (rng() % 3 == 0) {  // a random DAG, arcs low -> high
            start.assign((size_t)n, {});
            for (int v = 0; v < n; ++v) {
                for (int q = 0; q < v; ++q)
                    if (rng() % 100 < 25) start[(size_t)v].push_back(q), spar.push_back(q);
                soff.push_back((int32_t)spar.size());
            }
            o.start_off = soff.data();
            o.start_parents = spar.data();  // its families may exceed max_family_cells: sized as they are
        }
        const Run a = Climb(d, o), b = Climb(d, o);
        CheckRun(d, o, a, start);
        CHECK(a.rc == b.rc && a.parents == b.parents && a.ops == b.ops && a.delta == b.delta && a.info.score == b.info.score);
        ops += a.info.iterations;
    }
    CHECK(ops > 100);
    printf("%s: %d failures (%lld operations over 60 random searches)\n", g_fail ? "FAILED" : "ok", g_fail, (long long)ops);
    return g_fail ? 1 : 0;
}
