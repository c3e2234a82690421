// pc_search_host_check.cpp -- stand-alone driver of the PC-stable level search (fastbn_amd/csrc/pc_search.cpp:
// edge state, halves, the two generators, the resolver) for host sanitizer runs (no device, no libfastbn):
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/pc_search_host_check.cpp fastbn_amd/csrc/pc_search.cpp -o pc_search_host_check && ./pc_search_host_check
// The CI tests are a deterministic function of (x, y, sorted z) -> (indep, df).  Seeded sparse graphs
// of 6-12 variables (with vertices of degree <= d and edges whose side x is too small), d = 1..3, group
// sizes 1 and 3, and three schedules (chunk 1 growing x2: the most rounds; the default round-0 budget;
// full speculation), each as one half and as two, with both generators at d = 1.  removed / sep /
// counted must equal a sequential restatement of pc_driver.cpp's header: edge by edge, side x then
// side y, candidate sets in ChoiceGenerator order in groups of group_size, the first independent set
// wins, a df == 0 inside a group of more than one is a dependence, counted = whole groups up to and
// including the deciding one.  Also: launched >= counted, and full speculation launches exactly
// the sum of EdgeCost.  Exits non-zero on a wrong answer.
#include <cstdio>
#include <random>
#include <vector>

#include "../fastbn_amd/csrc/pc_search.h"

static int g_fail = 0;
#define CHECK(cond)                                              \
    do {                                                         \
        if (!(cond)) {                                           \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_fail;                                            \
        }                                                        \
    } while (0)

// the "CI test": about one set in six independent, about one in five with df == 0
static void Decide(uint32_t seed, int x, int y, const int *z, int d, uint8_t *indep, int32_t *df) {
    uint64_t h = 0x9E3779B97F4A7C15ull ^ seed;
    auto mix = [&h](uint64_t v) {
        h ^= v + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
        h *= 0xBF58476D1CE4E5B9ull;
        h ^= h >> 29;
    };
    mix((uint64_t)x), mix((uint64_t)y);
    for (int i = 0; i < d; ++i) mix((uint64_t)z[i]);
    *indep = (h >> 8) % 6 == 0;
    *df = (h >> 24) % 5 == 0 ? 0 : (int32_t)((h >> 32) % 9) + 1;
}

// the sequential restatement (pc_driver.cpp's header)
static void Restate(const fbn::Skeleton &sk, int d, int gs, uint32_t seed, fbn::LevelOut &out) {
    const size_t E = sk.edges.size();
    out.removed.assign(E, 0);
    out.sep.assign(E * (size_t)d, -1);
    out.counted = 0;
    for (size_t e = 0; e < E; ++e) {
        const int xy[2] = {sk.edges[e].first, sk.edges[e].second};
        for (int side = 0; side < 2 && !out.removed[e]; ++side) {
            std::vector<int> cand;
            for (int v : sk.adj[xy[side]])
                if (v != xy[1 - side]) cand.push_back(v);
            const int m = (int)cand.size();
            if (m < d) continue;
            std::vector<std::vector<int>> sets;  // ChoiceGenerator order = lexicographic positions
            std::vector<int> ch(d);
            for (int i = 0; i < d; ++i) ch[i] = i;
            while (true) {
                std::vector<int> z(d);
                for (int i = 0; i < d; ++i) z[i] = cand[ch[i]];
                sets.push_back(z);
                int i = d - 1;
                while (i >= 0 && ch[i] == m - d + i) --i;
                if (i < 0) break;
                ++ch[i];
                for (int k = i + 1; k < d; ++k) ch[k] = ch[k - 1] + 1;
            }
            for (size_t g = 0; g < sets.size() && !out.removed[e]; g += gs) {
                const size_t gsz = std::min(sets.size() - g, (size_t)gs);
                out.counted += (int64_t)gsz;
                for (size_t t = g; t < g + gsz; ++t) {
                    uint8_t ind;
                    int32_t df;
                    Decide(seed, xy[0], xy[1], sets[t].data(), d, &ind, &df);
                    if (gsz > 1 && df == 0) ind = 0;
                    if (ind) {
                        out.removed[e] = 1;
                        std::copy(sets[t].begin(), sets[t].end(), out.sep.begin() + e * d);  // (ascending already)
                        break;
                    }
                }
            }
        }
    }
}

static int g_small_side = 0, g_low_degree = 0, g_two_halves = 0, g_rounds = 0;

static void RunCase(const fbn::Skeleton &sk, const std::vector<int32_t> &dims, int d, int gs, uint32_t seed,
                    const fbn::SearchSchedule &sch, bool full, const fbn::LevelOut &want) {
    fbn::LevelSearch search(sk, 0, sk.edges.size(), d, gs, dims.data(), sch);
    g_two_halves += search.halves() == 2;
    CHECK(search.halves() == 1 || sk.edges.size() >= 2);
    int64_t launched = 0;
    std::vector<uint8_t> indep;
    std::vector<int32_t> df;
    for (bool any = true; any;) {
        any = false;
        for (int h = 0; h < search.halves(); ++h) {
            if (!search.Generate(h)) continue;
            any = true;
            ++g_rounds;
            const int64_t nt = search.tests(h);
            const std::vector<int32_t> &items = search.items(h);
            CHECK((int64_t)items.size() == nt * (2 + d));
            indep.resize(nt), df.resize(nt);
            fbn::CiBatchStats st{0, 0};
            for (int64_t t = 0; t < nt; ++t) {
                const int32_t *it = items.data() + t * (2 + d);
                for (int i = 0; i < 2 + d; ++i) st.dim_rows += dims[it[i]], st.maxdim = std::max(st.maxdim, (int)dims[it[i]]);
                Decide(seed, it[0], it[1], it + 2, d, &indep[t], &df[t]);
            }
            CHECK(st.maxdim == search.stats(h).maxdim && st.dim_rows == search.stats(h).dim_rows);
            launched += nt;
            search.Resolve(h, indep.data(), df.data());
        }
    }
    fbn::LevelOut out;
    search.Finish(out);
    CHECK(out.d == d && out.removed == want.removed && out.sep == want.sep && out.counted == want.counted);
    CHECK(launched >= out.counted);
    if (full) {
        int64_t all = 0;
        for (size_t e = 0; e < sk.edges.size(); ++e) all += sk.EdgeCost(e, d);
        CHECK(launched == all);
    }
}

int main() {
    CHECK(fbn::Binom(5, 2) == 10 && fbn::Binom(3, 4) == 0 && fbn::Binom(4, 0) == 1 && fbn::Binom(200, 100) == (int64_t)1 << 40);
    int cases = 0;
    for (uint32_t seed = 1; seed <= 40; ++seed) {
        std::mt19937 rng(seed);
        const int n = 6 + (int)(rng() % 7);
        fbn::Skeleton sk;
        sk.Reset(n);
        const uint32_t density = 25 + rng() % 30;  // per cent; variable 0 keeps at most one neighbour
        for (int i = 0; i < n; ++i)
            for (int j = i + 1; j < n; ++j)
                if (i == 0 ? j == 1 + (int)(seed % (uint32_t)(n - 1)) : rng() % 100 < density) sk.edges.push_back({i, j});
        sk.RebuildAdj(seed & 1);
        std::vector<int32_t> dims(n);
        for (auto &v : dims) v = 2 + (int32_t)(rng() % 4);
        for (int d = 1; d <= 3; ++d) {
            for (auto &e : sk.edges) g_small_side += (int)sk.adj[e.first].size() - 1 < d;
            for (auto &a : sk.adj) g_low_degree += (int)a.size() <= d;
            for (int gs : {1, 3}) {
                fbn::LevelOut want;
                Restate(sk, d, gs, seed, want);
                for (int sched = 0; sched < 3; ++sched)
                    for (int two = 0; two < 2; ++two)
                        for (int general = 0; general < (d == 1 && gs == 1 ? 2 : 1); ++general) {
                            fbn::SearchSchedule sch;
                            sch.full_spec = sched == 2 ? (int64_t)1 << 40 : -1;
                            if (sched == 0) sch.round0 = 1, sch.growth = 2;
                            sch.pipeline_edges = two ? 0 : (int64_t)1 << 40;
                            sch.split_full = two ? 0 : (int64_t)1 << 40;
                            sch.general = general != 0;
                            RunCase(sk, dims, d, gs, seed, sch, sched == 2, want);
                            ++cases;
                        }
            }
        }
    }
    // the cases meant to be there were there
    CHECK(g_small_side > 0 && g_low_degree > 0 && g_two_halves > 0 && g_rounds > cases);
    if (g_fail) printf("pc_search_host_check: %d failure(s)\n", g_fail);
    else printf("pc_search_host_check: ok (%d cases, %d rounds)\n", cases, g_rounds);
    return g_fail ? 1 : 0;
}
