// sample_host_check.cpp -- stand-alone driver of the sampling engine's host path
// (fastbn_amd/csrc/sample_host.cpp) for host sanitizer runs (no device, no libfastbn):
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -Iinclude \
//       tools/sample_host_check.cpp fastbn_amd/csrc/sample_host.cpp fastbn_amd/csrc/synth.cpp \
//       fastbn_amd/csrc/io.cpp -pthread -o sample_host_check && ./sample_host_check
// Seeded networks built in memory (every family shape of tests/test_gpu_param.py's 15-node graph, a
// 1041-variable chain-with-skips, the 61-node underflow network of tests/test_sample_host.py):
// forward sampling against synth.cpp's generator bit for bit, likelihood weighting / logic sampling
// for repeatability, batch-split invariance, value ranges, finite outputs and the error returns.
// Exits non-zero on a wrong answer.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../fastbn_amd/csrc/fbn_internal.h"
#include "../fastbn_amd/csrc/sample_model.h"

namespace fbn {
const char *LastError();
}

static int g_fail = 0;
#define CHECK(cond)                                                                           \
    do {                                                                                      \
        if (!(cond)) {                                                                        \
            printf("FAIL %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, fbn::LastError()); \
            ++g_fail;                                                                         \
        }                                                                                     \
    } while (0)

using Lists = std::vector<std::vector<int32_t>>;

// a network with seeded counts (0 .. maxc per cell)
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

static void CheckNetwork(const char *name, const fbn::Network &net, int64_t S, int nobs) {
    fbn::SamplerModel M;
    CHECK(fbn::BuildSamplerModel(net, M) == 0);
    const int V = M.V, SD = M.sum_dom;
    // forward sampling = the existing generator
    for (int64_t n : {1, 63, 65, 4097}) {
        std::vector<uint8_t> a((size_t)V * n, 0xEE), b((size_t)V * n, 0xDD);
        CHECK(fbn::HostForward(M, n, 17, a.data()) == 0 && fbn::ForwardSample(net, n, 17, b.data()) == 0);
        CHECK(a == b);
    }
    // evidence: nobs observed variables per case, values from a forward sample
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
    CHECK(fbn::CheckEvidenceHost(M, ev.data(), C) == 0);
    for (int method = 0; method < 2; ++method) {
        std::vector<int32_t> lab(C), lab2(C), e((size_t)C * S);
        std::vector<double> marg((size_t)C * SD), marg2((size_t)C * SD), st((size_t)C * 2), st2((size_t)C * 2), m((size_t)C * S);
        std::vector<uint8_t> val((size_t)V * C * S);
        CHECK(fbn::CheckLwShape(M, method, C, S, 0) == 0);
        CHECK(fbn::HostLw(M, method, ev.data(), C, S, 5, 0, lab.data(), marg.data(), st.data(), val.data(), m.data(), e.data()) == 0);
        // the split 4 + 5 with case_offset, no marginals buffer for the first part
        CHECK(fbn::HostLw(M, method, ev.data(), 4, S, 5, 0, lab2.data(), nullptr, st2.data(), nullptr, nullptr, nullptr) == 0);
        CHECK(fbn::HostLw(M, method, ev.data() + 4 * V, 5, S, 5, 4, lab2.data() + 4, marg2.data() + 4 * SD, st2.data() + 8,
                          nullptr, nullptr, nullptr) == 0);
        CHECK(lab == lab2 && memcmp(st.data(), st2.data(), st.size() * 8) == 0);
        CHECK(memcmp(marg.data() + 4 * SD, marg2.data() + 4 * SD, (size_t)5 * SD * 8) == 0);
        for (int64_t c = 0; c < C; ++c) {
            const bool dead = lab[c] < 0;
            CHECK(dead ? (std::isinf(st[2 * c]) && st[2 * c] < 0 && st[2 * c + 1] == 0.0)
                       : (std::isfinite(st[2 * c]) && st[2 * c + 1] >= 1.0 - 1e-9 && st[2 * c + 1] <= (double)S + 1e-9));
            CHECK(method == 1 || !dead);
            int off = 0;
            for (int v = 0; v < V; ++v) {
                double sum = 0.0;
                for (int q = 0; q < M.dom[v]; ++q) {
                    const double p = marg[c * SD + off + q];
                    CHECK(std::isfinite(p) && p >= 0.0 && p <= 1.0 + 1e-12);
                    sum += p;
                }
                CHECK(ev[c * V + v] >= 0 || dead ? sum == 0.0 : std::fabs(sum - 1.0) < 1e-9);
                off += M.dom[v];
            }
        }
        for (int v = 0; v < V; ++v)
            for (int64_t i = 0; i < C * S; ++i) {
                CHECK(val[(size_t)v * C * S + i] < M.dom[v]);
                if (method == 0 && ev[(i / S) * V + v] >= 0) CHECK(val[(size_t)v * C * S + i] == (uint8_t)ev[(i / S) * V + v]);
            }
        for (int64_t i = 0; i < C * S; ++i)
            CHECK(method == 0 ? (m[i] == 1.0 && e[i] == 0) || (m[i] >= 0.5 && m[i] < 1.0) : (m[i] == 0.0 || m[i] == 1.0) && e[i] == 0);
        if (method == 0)  // case 0 has no evidence: every weight 1
            CHECK(st[0] == 0.0 && st[1] == (double)S);
    }
    // errors
    std::vector<int8_t> bad(ev);
    bad[2 * V + 1] = (int8_t)M.dom[1];
    CHECK(fbn::CheckEvidenceHost(M, bad.data(), C) == FBN_ERR_ARG && strstr(fbn::LastError(), "case 2"));
    bad[2 * V + 1] = -2;
    CHECK(fbn::CheckEvidenceHost(M, bad.data(), C) == FBN_ERR_ARG);
    CHECK(fbn::CheckLwShape(M, 0, C, 0, 0) == FBN_ERR_ARG);
    CHECK(fbn::CheckLwShape(M, 2, C, 8, 0) == FBN_ERR_ARG);
    CHECK(fbn::CheckLwShape(M, 0, C, (int64_t)1 << 62, 0) == FBN_ERR_ARG);
    printf("%s: %d variables, %d marginal entries, %lld cells\n", name, V, SD, (long long)M.cells);
}

int main() {
    fbn::Network net;
    // every family shape: a 1-state node, 127 states, six parents, a descending parent order
    CHECK(Build({5, 3, 7, 2, 4, 2, 2, 2, 2, 2, 2, 3, 1, 127, 6},
                {{}, {0}, {}, {2, 0}, {0, 1, 2}, {}, {}, {}, {}, {}, {}, {5, 6, 7, 8, 9, 10}, {}, {12}, {1}}, 1, 50, net) == 0);
    CheckNetwork("shapes", net, 200, 4);
    {  // Munin-like size: 1041 variables, node v's parents v - 1 and (odd v) v - 3
        std::vector<int32_t> dims(1041);
        Lists par(1041);
        for (int v = 0; v < 1041; ++v) {
            dims[v] = 2 + v % 4;
            if (v >= 1) par[v].push_back(v - 1);
            if (v >= 3 && v % 2) par[v].push_back(v - 3);
        }
        CHECK(Build(dims, par, 2, 30, net) == 0);
        CheckNetwork("chain1041", net, 70, 300);
    }
    {  // weights below fp64: 60 observed children at 1 / (10^6 + 2) under root = 0
        std::vector<int32_t> dims(61, 2), po{0}, p;
        std::vector<int64_t> counts{2, 0};
        for (int v = 1; v <= 60; ++v) {
            p.push_back(0);
            po.push_back((int32_t)p.size());
            counts.insert(counts.end(), {1000000, 1, 0, 1});
        }
        po.insert(po.begin(), 0);
        CHECK(fbn::BuildNetwork(61, dims.data(), po.data(), p.data(), counts.data(), nullptr, net) == 0);
        fbn::SamplerModel M;
        CHECK(fbn::BuildSamplerModel(net, M) == 0);
        std::vector<int8_t> ev(61, 1);
        ev[0] = -1;
        int32_t lab = 7;
        std::vector<double> marg(122), st(2);
        CHECK(fbn::HostLw(M, 0, ev.data(), 1, 256, 1, 0, &lab, marg.data(), st.data(), nullptr, nullptr, nullptr) == 0);
        CHECK(lab == 1 && std::isfinite(st[0]) && st[0] > -100.0 && std::fabs(marg[0] + marg[1] - 1.0) < 1e-12 && marg[0] < 1e-300);
        CHECK(fbn::HostLw(M, 1, ev.data(), 1, 256, 1, 0, &lab, marg.data(), st.data(), nullptr, nullptr, nullptr) == 0);
        CHECK(lab == -1 && std::isinf(st[0]) && st[1] == 0.0 && marg[0] == 0.0 && marg[1] == 0.0);
    }
    {  // limits: a cycle, too many variables
        fbn::Network cyc;
        cyc.dom = {2, 2, 2};
        cyc.given = cyc.parents_asc = {{2}, {0}, {1}};
        fbn::SamplerModel M;
        CHECK(fbn::BuildSamplerModel(cyc, M) == FBN_ERR_ARG);
        std::vector<int32_t> dims(FBN_SAMPLE_MAX_VARS + 1, 2);
        CHECK(Build(dims, Lists(dims.size()), 3, 9, net) == 0);
        CHECK(fbn::BuildSamplerModel(net, M) == FBN_ERR_LIMIT);
        dims.pop_back();
        CHECK(Build(dims, Lists(dims.size()), 3, 9, net) == 0);
        CHECK(fbn::BuildSamplerModel(net, M) == 0 && M.V == FBN_SAMPLE_MAX_VARS);
    }
    {  // scoring: one case by hand (Round(., 7), evidence node skipped)
        const double a[5] = {0.25, 0.75, 0.5, 0.3, 0.2}, g[5] = {0.5, 0.5, -1.0, 0.0, 0.0};
        double mse = 0, hd = 0;
        CHECK(fbn::ScoreMarginals({2, 3}, a, g, 1, &mse, &hd) == 0);
        CHECK(std::fabs(mse - 0.25) < 1e-15 && hd > 0.0);
    }
    printf("%s: %d failures\n", g_fail ? "FAILED" : "ok", g_fail);
    return g_fail ? 1 : 0;
}
