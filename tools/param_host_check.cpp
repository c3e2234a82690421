// param_host_check.cpp -- stand-alone driver of fastbn_amd/csrc/param_learn.cpp for host sanitizer
// runs (no device, no libfastbn):
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/param_host_check.cpp fastbn_amd/csrc/param_learn.cpp -o param_host_check && ./param_host_check
// Runs the family_sizes and pdag_to_dag cases of tests/test_param_host.py plus seeded random PDAGs
// (CPDAG-like: a random DAG with some arcs undirected) and exits non-zero on a wrong answer.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
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

static int Sizes(const std::vector<int32_t> &dims, const Lists &par, std::vector<int64_t> *off, int64_t *total) {
    std::vector<int32_t> po{0}, p;
    for (auto &l : par) {
        p.insert(p.end(), l.begin(), l.end());
        po.push_back((int32_t)p.size());
    }
    off->assign(dims.size() + 1, -1);
    return fbn::ParamFamilySizes((int)dims.size(), dims.data(), po.data(), p.empty() ? nullptr : p.data(), off->data(), total);
}

static int Extend(int nvars, const std::vector<int32_t> &tri, Lists *dag) {
    const int n = (int)tri.size() / 3;
    std::vector<int32_t> off(nvars + 1), par(n > 0 ? n : 1);
    int rc = fbn::PdagToDag(nvars, tri.data(), n, off.data(), par.data());
    dag->assign(nvars, {});
    if (rc == 0)
        for (int v = 0; v < nvars; ++v) (*dag)[v].assign(par.begin() + off[v], par.begin() + off[v + 1]);
    return rc;
}

int main() {
    std::vector<int64_t> off;
    int64_t total = 0;
    Lists dag;
    // ---- family sizes
    CHECK(Sizes({5, 3, 7, 2}, {{}, {0}, {1, 0}, {2, 0, 1}}, &off, &total) == 0 && total == 335 &&
          off == std::vector<int64_t>({0, 5, 20, 125, 335}));
    CHECK(Sizes({5, 3, 7, 2}, {{}, {4}, {}, {}}, &off, &total) == FBN_ERR_ARG);
    CHECK(Sizes({5, 3, 7, 2}, {{}, {-1}, {}, {}}, &off, &total) == FBN_ERR_ARG);
    CHECK(Sizes({5, 3, 7, 2}, {{}, {1}, {}, {}}, &off, &total) == FBN_ERR_ARG);
    CHECK(Sizes({5, 3, 7, 2}, {{}, {}, {0, 1, 0}, {}}, &off, &total) == FBN_ERR_ARG);
    CHECK(Sizes({5, 0, 7, 2}, {{}, {}, {}, {}}, &off, &total) == FBN_ERR_ARG);
    {
        std::vector<int32_t> dims(40, 4);
        dims.push_back(2);
        Lists par(41);
        for (int q = 0; q < 40; ++q) par[40].push_back(q);
        CHECK(Sizes(dims, par, &off, &total) == FBN_ERR_LIMIT);  // 2^81 cells
        dims.assign(300, 256);  // 256^300: far past any integer width
        par.assign(300, {});
        for (int q = 0; q < 299; ++q) par[299].push_back(q);
        CHECK(Sizes(dims, par, &off, &total) == FBN_ERR_LIMIT);
        dims.assign(27, 2);  // three families of 2^25 cells: each fits, the sum does not
        par.assign(27, {});
        for (int v = 24; v < 27; ++v)
            for (int q = 0; q < 24; ++q) par[v].push_back(q);
        CHECK(Sizes(dims, par, &off, &total) == FBN_ERR_LIMIT);
        dims.assign(25, 2);
        par.assign(25, {});
        for (int q = 0; q < 24; ++q) par[24].push_back(q);
        CHECK(Sizes(dims, par, &off, &total) == 0 && total == 48 + (1ll << 25));
    }
    // ---- PDAG -> DAG
    CHECK(Extend(3, {0, 1, 0, 1, 2, 0}, &dag) == 0 && dag == Lists({{1}, {2}, {}}));
    CHECK(Extend(5, {0, 2, 1, 1, 2, 1, 2, 3, 0, 3, 4, 0}, &dag) == 0 && dag == Lists({{}, {}, {0, 1}, {2}, {3}}));
    CHECK(Extend(4, {0, 1, 0, 1, 2, 0, 2, 3, 0, 0, 3, 0}, &dag) == FBN_ERR_ARG);  // chordless 4-cycle
    CHECK(Extend(3, {0, 1, 1, 1, 2, 1, 2, 0, 1}, &dag) == FBN_ERR_ARG);           // directed 3-cycle
    CHECK(Extend(3, {0, 1, 1, 0, 1, 1}, &dag) == FBN_ERR_ARG);
    CHECK(Extend(3, {0, 1, 1, 1, 0, 1}, &dag) == FBN_ERR_ARG);
    CHECK(Extend(3, {0, 1, 1, 0, 1, 0}, &dag) == FBN_ERR_ARG);
    CHECK(Extend(3, {0, 3, 1}, &dag) == FBN_ERR_ARG);
    CHECK(Extend(3, {1, 1, 0}, &dag) == FBN_ERR_ARG);
    CHECK(Extend(3, {}, &dag) == 0 && dag == Lists({{}, {}, {}}));
    // seeded random PDAGs: a random DAG (arcs low -> high index) with a random subset of its arcs
    // undirected.  Whatever the answer, an accepted one is acyclic over the same skeleton, keeps
    // every arc, and two calls agree.
    std::mt19937 rng(12345);
    int accepted = 0;
    for (int it = 0; it < 400; ++it) {
        const int n = 2 + (int)(rng() % 30);
        std::vector<int32_t> tri;
        std::set<std::pair<int, int>> skel, arcs;
        for (int b = 1; b < n; ++b)
            for (int a = 0; a < b; ++a)
                if (rng() % 100 < 15) {
                    const bool und = rng() % 100 < 30, flip = rng() % 2;
                    tri.insert(tri.end(), {und && flip ? b : a, und && flip ? a : b, und ? 0 : 1});
                    skel.insert({a, b});
                    if (!und) arcs.insert({a, b});
                }
        Lists d2;
        const int rc = Extend(n, tri, &dag), rc2 = Extend(n, tri, &d2);
        CHECK(rc == rc2 && dag == d2);
        CHECK(rc == 0 || rc == FBN_ERR_ARG);
        if (rc) continue;
        ++accepted;
        std::set<std::pair<int, int>> got;
        std::vector<int> indeg(n, 0), order;
        Lists ch(n);
        for (int v = 0; v < n; ++v)
            for (int q : dag[v]) {
                got.insert({std::min(v, q), std::max(v, q)});
                ch[q].push_back(v);
                ++indeg[v];
            }
        CHECK(got == skel);
        for (auto &a : arcs) CHECK(std::find(dag[a.second].begin(), dag[a.second].end(), a.first) != dag[a.second].end());
        for (int v = 0; v < n; ++v)
            if (!indeg[v]) order.push_back(v);
        for (size_t i = 0; i < order.size(); ++i)
            for (int c : ch[order[i]])
                if (--indeg[c] == 0) order.push_back(c);
        CHECK((int)order.size() == n);
    }
    CHECK(accepted > 50);
    printf("%s: %d failures (%d of 400 random PDAGs had an extension)\n", g_fail ? "FAILED" : "ok", g_fail, accepted);
    return g_fail ? 1 : 0;
}
