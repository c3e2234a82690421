// lbp_host_check.cpp -- stand-alone driver of loopy belief propagation's host side
// (fastbn_amd/csrc/lbp_host.cpp, lbp_model.h) for host sanitizer runs (no device, no libfastbn):
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -Iinclude \
//       tools/lbp_host_check.cpp fastbn_amd/csrc/lbp_host.cpp fastbn_amd/csrc/synth.cpp \
//       fastbn_amd/csrc/io.cpp -pthread -o lbp_host_check && ./lbp_host_check
// Seeded networks built in memory (every family shape of tests/test_gpu_param.py's 15-node graph and
// a 1041-variable chain-with-skips): the model's index ranges, LbpDiv against integer division,
// repeatability, batch-split invariance, beliefs that sum to one, zeros for observed variables, the
// message dump and the error returns.  The per-entry functions it runs are the ones the kernel
// compiles, so an index out of range here is one there.  Exits non-zero on a wrong answer.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../fastbn_amd/csrc/fbn_internal.h"
#include "../fastbn_amd/csrc/lbp_model.h"

static int g_fail = 0;
#define CHECK(cond)                                                                           \
    do {                                                                                      \
        if (!(cond)) {                                                                        \
            printf("FAIL %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, fbn::LastError()); \
            ++g_fail;                                                                         \
        }                                                                                     \
    } while (0)

using Lists = std::vector<std::vector<int32_t>>;

static int Build(const std::vector<int32_t> &dims, const Lists &par, uint32_t seed, int maxc, fbn::Network &net) {
    std::mt19937 rng(seed);
    std::vector<int32_t> po{0}, p;
    std::vector<int64_t> counts;
    for (size_t v = 0; v < dims.size(); ++v) {
        int64_t cells = dims[v];
        for (int q : par[v]) cells *= dims[q];
        for (int64_t c = 0; c < cells; ++c) counts.push_back((int64_t)(rng() % (uint32_t)(maxc + 1)));
        p.insert(p.end(), par[v].begin(), par[v].end());
        po.push_back((int32_t)p.size());
    }
    if (p.empty()) p.push_back(0);
    return fbn::BuildNetwork((int)dims.size(), dims.data(), po.data(), p.data(), counts.data(), nullptr, net);
}

static void CheckNetwork(const char *name, const fbn::Network &net, int iters, int nobs) {
    fbn::LbpModel M;
    CHECK(fbn::BuildLbpModel(net, M) == 0);
    const int V = M.V, SD = M.sum_dom;
    const int64_t MM = M.M;
    // index ranges of the flattened model
    CHECK((int64_t)M.bin_edge.size() == MM && (int)M.var_moff.size() == M.E && M.var_off[V] == M.E);
    std::vector<int> seen((size_t)MM, 0);
    CHECK((int64_t)M.order.size() == MM);
    for (int32_t j : M.order) CHECK(j >= 0 && j < MM && !seen[j]++);  // a permutation
    for (const fbn::LbpEdge &e : M.edges) {
        CHECK(e.x >= 0 && e.x < V && e.d == M.dom[e.x] && e.moff >= 0 && e.moff + e.d <= MM);
        CHECK(e.term >= 0 && e.term + e.nterm <= (int)M.terms.size());
        CHECK(e.toff >= 0 && (int64_t)e.toff + (int64_t)e.ncell * e.d <= M.cells);
        for (int t = 0; t < e.nterm; ++t) CHECK(M.terms[e.term + t].moff >= 0 && M.terms[e.term + t].moff < MM);
    }
    const int64_t C = 9;
    std::vector<uint8_t> full((size_t)V * C);
    CHECK(fbn::ForwardSample(net, C, 3, full.data()) == 0);
    std::vector<int8_t> ev((size_t)C * V, -1);
    std::mt19937 rng(99);
    for (int64_t c = 1; c < C; ++c)
        for (int k = 0; k < nobs; ++k) {
            const int v = (int)(rng() % (uint32_t)V);
            ev[c * V + v] = (int8_t)full[(size_t)v * C + c];
        }
    CHECK(fbn::CheckLbpEvidence(M, ev.data(), C) == 0);
    for (double damping : {0.0, 0.5}) {
        std::vector<int32_t> lab(C), lab2(C);
        std::vector<double> marg((size_t)C * SD), marg2((size_t)C * SD), st(2 * C), st2(2 * C), msg((size_t)C * 2 * MM);
        CHECK(fbn::HostLbp(M, ev.data(), C, iters, 1e-12, damping, lab.data(), marg.data(), st.data(), nullptr) == 0);
        // the split 4 + 5, no marginals buffer for the first part
        CHECK(fbn::HostLbp(M, ev.data(), 4, iters, 1e-12, damping, lab2.data(), nullptr, st2.data(), nullptr) == 0);
        CHECK(fbn::HostLbp(M, ev.data() + 4 * V, 5, iters, 1e-12, damping, lab2.data() + 4, marg2.data() + 4 * SD, st2.data() + 8, nullptr) == 0);
        CHECK(lab == lab2 && memcmp(st.data(), st2.data(), st.size() * 8) == 0);
        CHECK(memcmp(marg.data() + 4 * SD, marg2.data() + 4 * SD, (size_t)5 * SD * 8) == 0);
        CHECK(fbn::HostLbp(M, ev.data(), C, 3, -1.0, damping, lab2.data(), nullptr, nullptr, msg.data()) == 0);
        for (double x : msg) CHECK(std::isfinite(x) && x >= 0.0 && x <= 1.0);
        for (int64_t c = 0; c < C; ++c) {
            CHECK(lab[c] >= 0 && lab[c] < M.dom[0] && st[2 * c] >= 1 && st[2 * c] <= iters && std::isfinite(st[2 * c + 1]));
            int off = 0;
            for (int v = 0; v < V; ++v) {
                double sum = 0.0;
                for (int q = 0; q < M.dom[v]; ++q) {
                    const double p = marg[c * SD + off + q];
                    CHECK(std::isfinite(p) && p >= 0.0 && p <= 1.0 + 1e-12);
                    sum += p;
                }
                CHECK(ev[c * V + v] >= 0 ? sum == 0.0 : std::fabs(sum - 1.0) < 1e-9);
                off += M.dom[v];
            }
        }
    }
    std::vector<int8_t> bad(ev);
    bad[2 * V + 1] = (int8_t)M.dom[1];
    CHECK(fbn::CheckLbpEvidence(M, bad.data(), C) == FBN_ERR_ARG && strstr(fbn::LastError(), "case 2"));
    bad[2 * V + 1] = -2;
    CHECK(fbn::CheckLbpEvidence(M, bad.data(), C) == FBN_ERR_ARG);
    printf("%s: %d variables, %d edges, %lld message entries, %lld cells\n", name, V, M.E, (long long)MM, (long long)M.cells);
}

int main() {
    {  // LbpDiv = integer division over the whole range the model uses
        std::mt19937 rng(5);
        for (int i = 0; i < 2000000; ++i) {
            const int s = 1 + (int)(rng() % (i % 3 ? 300u : (1u << 26)));
            const int n = i % 5 == 0 ? (int)((rng() % 64) * (uint32_t)s % (1u << 26)) : (int)(rng() % (1u << 26));
            if (fbn::LbpDiv(n, s, 1.0 / (double)s) != n / s) {
                CHECK(!"LbpDiv");
                break;
            }
        }
        CHECK(fbn::LbpDiv((1 << 26) - 1, 1, 1.0) == (1 << 26) - 1 && fbn::LbpDiv((1 << 26) - 1, 1 << 26, 1.0 / (1 << 26)) == 0);
    }
    fbn::Network net;
    CHECK(Build({5, 3, 7, 2, 4, 2, 2, 2, 2, 2, 2, 3, 1, 127, 6},
                {{}, {0}, {}, {2, 0}, {0, 1, 2}, {}, {}, {}, {}, {}, {}, {5, 6, 7, 8, 9, 10}, {}, {12}, {1}}, 1, 50, net) == 0);
    CheckNetwork("shapes", net, 40, 4);
    {  // Munin-like size: 1041 variables, node v's parents v - 1 and (odd v) v - 3
        std::vector<int32_t> dims(1041);
        Lists par(1041);
        for (int v = 0; v < 1041; ++v) {
            dims[v] = 2 + v % 4;
            if (v >= 1) par[v].push_back(v - 1);
            if (v >= 3 && v % 2) par[v].push_back(v - 3);
        }
        CHECK(Build(dims, par, 2, 30, net) == 0);
        CheckNetwork("chain1041", net, 6, 300);
    }
    {  // arguments, a cycle
        CHECK(fbn::CheckLbpArgs(1, 0, 0.0, 0.0) == FBN_ERR_ARG && fbn::CheckLbpArgs(1, 1, -1.0, 0.0) == FBN_ERR_ARG);
        CHECK(fbn::CheckLbpArgs(1, 1, NAN, 0.0) == FBN_ERR_ARG && fbn::CheckLbpArgs(1, 1, 0.0, 1.0) == FBN_ERR_ARG);
        CHECK(fbn::CheckLbpArgs(1, 1, 0.0, NAN) == FBN_ERR_ARG && fbn::CheckLbpArgs(0, 1, 0.0, 0.99) == 0);
        fbn::Network cyc;
        cyc.dom = {2, 2, 2};
        cyc.given = cyc.parents_asc = {{2}, {0}, {1}};
        fbn::LbpModel M;
        CHECK(fbn::BuildLbpModel(cyc, M) == FBN_ERR_ARG);
    }
    printf("%s: %d failures\n", g_fail ? "FAILED" : "ok", g_fail);
    return g_fail ? 1 : 0;
}
