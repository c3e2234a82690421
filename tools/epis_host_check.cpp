// epis_host_check.cpp -- stand-alone driver of EPIS-BN's host side (fastbn_amd/csrc/epis_host.cpp,
// epis_model.h over lbp_host.cpp and sample_host.cpp) for host sanitizer runs (no device, no libfastbn):
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -Iinclude \
//       tools/epis_host_check.cpp fastbn_amd/csrc/epis_host.cpp fastbn_amd/csrc/lbp_host.cpp \
//       fastbn_amd/csrc/sample_host.cpp fastbn_amd/csrc/synth.cpp fastbn_amd/csrc/io.cpp -pthread \
//       -o epis_host_check && ./epis_host_check
// Seeded networks built in memory (every family shape of tests/test_gpu_param.py's 15-node graph, and
// a root with 1,100 children, on which LBP fails and the draws fall back to lambda = 1): lambda rows
// in range, finite outputs, repeatability, batch-split invariance, both cutoff settings, a partial
// last chunk, and the error returns.  EpisDraw is the function the kernel compiles, so an index out
// of range here is one there.  Exits non-zero on a wrong answer.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../fastbn_amd/csrc/epis_model.h"
#include "../fastbn_amd/csrc/fbn_internal.h"

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

static void CheckNetwork(const fbn::Network &net, int iters, int nobs, bool expect_fallback) {
    fbn::SamplerModel SM;
    fbn::LbpModel LM;
    CHECK(fbn::BuildSamplerModel(net, SM) == 0 && fbn::BuildLbpModel(net, LM) == 0);
    const int V = SM.V, SD = SM.sum_dom;
    CHECK(LM.sum_dom == SD && (int)LM.self_moff.size() == V);
    for (int v = 0; v < V; ++v) CHECK(LM.self_moff[v] >= 0 && LM.self_moff[v] + LM.dom[v] <= LM.M);
    const int64_t C = 7, S = 70;  // one full chunk and a 6-lane tail
    std::vector<uint8_t> full((size_t)V * C);
    CHECK(fbn::ForwardSample(net, C, 3, full.data()) == 0);
    std::vector<int8_t> ev((size_t)C * V, -1);
    std::mt19937 rng(99);
    for (int64_t c = 1; c < C; ++c)
        for (int k = 0; k < nobs; ++k) {
            const int v = (int)(rng() % (uint32_t)V);
            ev[c * V + v] = (int8_t)full[(size_t)v * C + c];
        }
    CHECK(fbn::CheckEvidenceHost(SM, ev.data(), C) == 0);
    for (double eps : {-1.0, 0.0, 0.25}) {
        std::vector<int32_t> lab(C), lab2(C), ex((size_t)C * S);
        std::vector<double> marg((size_t)C * SD), marg2((size_t)C * SD), st(4 * C), st2(4 * C), m((size_t)C * S),
            lam((size_t)C * SD);
        std::vector<uint8_t> val((size_t)V * C * S);
        CHECK(fbn::CheckEpisArgs(SM, C, S, 2, iters, 0.0, 0.0, eps) == 0);
        CHECK(fbn::HostEpis(SM, LM, ev.data(), C, S, 5, 2, iters, 0.0, 0.0, eps, lab.data(), marg.data(), st.data(),
                            val.data(), m.data(), ex.data(), lam.data()) == 0);
        // the split 3 + 4 without the debug outputs, no marginals buffer for the first part
        CHECK(fbn::HostEpis(SM, LM, ev.data(), 3, S, 5, 2, iters, 0.0, 0.0, eps, lab2.data(), nullptr, st2.data(), nullptr,
                            nullptr, nullptr, nullptr) == 0);
        CHECK(fbn::HostEpis(SM, LM, ev.data() + 3 * V, 4, S, 5, 5, iters, 0.0, 0.0, eps, lab2.data() + 3,
                            marg2.data() + 3 * SD, st2.data() + 12, nullptr, nullptr, nullptr, nullptr) == 0);
        CHECK(lab == lab2 && memcmp(st.data(), st2.data(), sizeof(double) * 4 * C) == 0);
        CHECK(memcmp(marg.data() + 3 * SD, marg2.data() + 3 * SD, sizeof(double) * 4 * SD) == 0);
        for (double x : marg) CHECK(std::isfinite(x) && x >= 0.0 && x <= 1.0 + 1e-12);
        for (double x : lam) CHECK(x >= 0.0 && x <= 1.0);
        for (double x : m) CHECK(x == 0.0 || (x >= 0.5 && x < 1.0));
        for (int64_t c = 0; c < C; ++c) {
            CHECK(std::isfinite(st[4 * c]) && st[4 * c + 1] > 0.0 && st[4 * c + 1] <= (double)S * (1 + 1e-12));
            CHECK(iters == 0 ? st[4 * c + 2] == 0.0 : st[4 * c + 2] >= 1.0);
            CHECK(std::isinf(st[4 * c + 3]) == expect_fallback);
            for (int v = 0; v < V; ++v)
                for (int64_t s = 0; s < S; ++s) {
                    const int x = val[(size_t)v * C * S + c * S + s];
                    CHECK(x < SM.dom[v] && (ev[c * V + v] < 0 || x == ev[c * V + v]));
                }
        }
        if (expect_fallback || iters == 0)
            for (double x : lam) CHECK(x == 1.0);
    }
}

int main() {
    fbn::Network shapes, star;
    const std::vector<int32_t> dims = {5, 3, 7, 2, 4, 2, 2, 2, 2, 2, 2, 3, 1, 127, 6};
    const Lists graph = {{}, {0}, {}, {2, 0}, {0, 1, 2}, {}, {}, {}, {}, {}, {}, {5, 6, 7, 8, 9, 10}, {}, {12}, {1}};
    CHECK(Build(dims, graph, 15, 40, shapes) == 0);
    CheckNetwork(shapes, 6, 3, false);
    CheckNetwork(shapes, 0, 3, false);
    Lists sp(1101);
    for (size_t v = 1; v < sp.size(); ++v) sp[v] = {0};
    CHECK(Build(std::vector<int32_t>(1101, 2), sp, 7, 3, star) == 0);
    CheckNetwork(star, 3, 2, true);
    fbn::SamplerModel SM;
    CHECK(fbn::BuildSamplerModel(shapes, SM) == 0);
    CHECK(fbn::CheckEpisArgs(SM, 1, 0, 0, 1, 0.0, 0.0, 0.0) == FBN_ERR_ARG);
    CHECK(fbn::CheckEpisArgs(SM, 1, 8, 0, -1, 0.0, 0.0, 0.0) == FBN_ERR_ARG);
    CHECK(fbn::CheckEpisArgs(SM, 1, 8, 0, 1, -1.0, 0.0, 0.0) == FBN_ERR_ARG);
    CHECK(fbn::CheckEpisArgs(SM, 1, 8, 0, 1, 0.0, 1.0, 0.0) == FBN_ERR_ARG);
    CHECK(fbn::CheckEpisArgs(SM, 1, 8, 0, 1, 0.0, 0.0, 1.0) == FBN_ERR_ARG);
    CHECK(fbn::CheckEpisArgs(SM, 1, 8, 0, 1, 0.0, 0.0, std::nan("")) == FBN_ERR_ARG);
    printf(g_fail ? "epis_host_check: %d failure(s)\n" : "epis_host_check: ok\n", g_fail);
    return g_fail ? 1 : 0;
}
