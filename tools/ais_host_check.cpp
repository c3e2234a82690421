// ais_host_check.cpp -- stand-alone driver of the adaptive samplers' host side
// (fastbn_amd/csrc/ais_host.cpp, ais_model.h over sample_host.cpp) for host sanitizer runs (no device,
// no libfastbn):
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -Iinclude \
//       tools/ais_host_check.cpp fastbn_amd/csrc/ais_host.cpp fastbn_amd/csrc/sample_host.cpp \
//       fastbn_amd/csrc/synth.cpp fastbn_amd/csrc/io.cpp -pthread -o ais_host_check && ./ais_host_check
// Seeded networks built in memory (every family shape of tests/test_gpu_param.py's 15-node graph, a
// 1-state and a 127-state node included): both methods, a partial last chunk in every stage, an
// interval that is no multiple of 64, intervals of 1 and beyond S, values in range, finite outputs,
// ICPT rows untouched outside the learnable set, repeatability, batch-split invariance and the error
// returns.  A hand-built model with zero CPT entries (no Network has one) drives the stage whose
// weights are all 0: the update is skipped, nothing becomes NaN, and a case without one positive weight
// is the empty estimate.  AisDraw and AisUpdateRow are the functions the kernel compiles, so an index
// out of range here is one there.  Exits non-zero on a wrong answer.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../fastbn_amd/csrc/ais_model.h"
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

static void CheckNetwork(const fbn::Network &net, int method, int64_t S, int64_t m, int64_t l, int nobs) {
    fbn::SamplerModel SM;
    CHECK(fbn::BuildSamplerModel(net, SM) == 0);
    const int V = SM.V, SD = SM.sum_dom;
    const int64_t C = 7, cells = SM.cells, T = fbn::AisStages(method, S, m, l).T;
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
    for (double eps : {-1.0, 0.25}) {
        std::vector<int32_t> lab(C), lab2(C), ex((size_t)C * T);
        std::vector<double> marg((size_t)C * SD), marg2((size_t)C * SD), st(4 * C), st2(4 * C), mant((size_t)C * T),
            icpt((size_t)C * cells);
        std::vector<uint8_t> val((size_t)V * C * T);
        CHECK(fbn::CheckAisArgs(SM, method, C, S, m, l, 2, eps) == 0);
        CHECK(fbn::HostAis(SM, method, ev.data(), C, S, m, l, 5, 2, eps, lab.data(), marg.data(), st.data(), val.data(),
                           mant.data(), ex.data(), icpt.data()) == 0);
        // the split 3 + 4 without the debug outputs, no marginals buffer for the first part
        CHECK(fbn::HostAis(SM, method, ev.data(), 3, S, m, l, 5, 2, eps, lab2.data(), nullptr, st2.data(), nullptr, nullptr,
                           nullptr, nullptr) == 0);
        CHECK(fbn::HostAis(SM, method, ev.data() + 3 * V, 4, S, m, l, 5, 5, eps, lab2.data() + 3, marg2.data() + 3 * SD,
                           st2.data() + 12, nullptr, nullptr, nullptr, nullptr) == 0);
        CHECK(lab == lab2 && memcmp(st.data(), st2.data(), sizeof(double) * 4 * C) == 0);
        CHECK(memcmp(marg.data() + 3 * SD, marg2.data() + 3 * SD, sizeof(double) * 4 * SD) == 0);
        for (double x : marg) CHECK(std::isfinite(x) && x >= 0.0 && x <= 1.0 + 1e-12);
        for (double x : icpt) CHECK(std::isfinite(x) && x >= 0.0 && x <= 1.0 + 1e-12);
        for (double x : mant) CHECK(x >= 0.5 && x <= 1.0);  // positive tables: no weight is 0 (1.0: no factor at all)
        const int64_t nupd = fbn::AisStages(method, S, m, l).nupd;
        for (int64_t c = 0; c < C; ++c) {
            CHECK(std::isfinite(st[4 * c]) && st[4 * c + 1] > 0.0 && st[4 * c + 1] <= (double)S * (1 + 1e-12));
            CHECK(st[4 * c + 2] == (double)nupd && st[4 * c + 3] > 0.0 && st[4 * c + 3] <= 1.0 + 1e-12);
            for (int v = 0; v < V; ++v)
                for (int64_t t = 0; t < T; ++t) {
                    const int x = val[(size_t)v * C * T + c * T + t];
                    CHECK(x < SM.dom[v] && (ev[c * V + v] < 0 || x == ev[c * V + v]));
                }
            // observed variables and variables without an observed descendant keep their CPT rows
            std::vector<char> desc((size_t)V, 0);
            for (int k = V - 1; k >= 0; --k) {
                const fbn::SampleNode &nd = SM.nodes[(size_t)k];
                if (ev[c * V + nd.v] >= 0 || desc[(size_t)nd.v])
                    for (int j = 0; j < nd.npar; ++j) desc[(size_t)SM.par[2 * (size_t)(nd.poff + j)]] = 1;
            }
            for (int k = 0; k < V; ++k) {
                const fbn::SampleNode &nd = SM.nodes[(size_t)k];
                const int64_t end = k + 1 < V ? SM.nodes[(size_t)k + 1].toff : cells;
                if (ev[c * V + nd.v] >= 0 || !desc[(size_t)nd.v])
                    CHECK(memcmp(icpt.data() + c * cells + nd.toff, SM.prob.data() + nd.toff,
                                 sizeof(double) * (size_t)(end - nd.toff)) == 0);
            }
        }
    }
}

// A -> B with P(B = 1 | A = 0) = 0 exactly and P(A = 1) = 0.1: with B = 1 observed, a stage of 4 samples
// without an A = 1 has no positive weight.
static void CheckZeroWeightStage() {
    fbn::SamplerModel M;
    M.V = 2, M.sum_dom = 4, M.cells = 6;
    M.dom = {2, 2};
    M.nodes = {fbn::SampleNode{0, 2, 0, 0, 0, 0}, fbn::SampleNode{1, 2, 1, 0, 2, 2}};
    M.par = {0, 2};
    M.prob = {0.9, 0.1, 1.0, 0.0, 0.25, 0.75};
    M.cdf = {0.9, 1.0, 1.0, 1.0, 0.25, 1.0};
    M.ent = {0, 1, 1 << 8, 1 << 8 | 1};
    const int64_t C = 32;
    std::vector<int8_t> ev((size_t)C * 2, -1);
    for (int64_t c = 0; c < C; ++c) ev[2 * c + 1] = 1;
    for (int method : {0, 1}) {
        const int64_t S = 40, m = 5, l = 4, T = fbn::AisStages(method, S, m, l).T;
        std::vector<int32_t> lab(C), ex((size_t)C * T);
        std::vector<double> marg((size_t)C * 4), st(4 * C), mant((size_t)C * T), icpt((size_t)C * 6);
        std::vector<uint8_t> val((size_t)2 * C * T);
        CHECK(fbn::HostAis(M, method, ev.data(), C, S, m, l, 1, 0, 0.01, lab.data(), marg.data(), st.data(), val.data(),
                           mant.data(), ex.data(), icpt.data()) == 0);
        int dead_first = 0, skipped = 0, untouched = 0, empty = 0;
        for (int64_t c = 0; c < C; ++c) {
            for (int j = 0; j < 4; ++j) CHECK(std::isfinite(marg[4 * c + j]));
            for (int j = 0; j < 6; ++j) CHECK(std::isfinite(icpt[6 * c + j]) && icpt[6 * c + j] >= 0.0);
            CHECK(!std::isnan(st[4 * c]) && std::isfinite(st[4 * c + 1]) && st[4 * c + 2] >= 0.0 && st[4 * c + 2] <= 5.0);
            bool first_dead = true;
            for (int64_t t = 0; t < l; ++t) first_dead = first_dead && mant[c * T + t] == 0.0;
            CHECK(first_dead == (st[4 * c + 3] == 0.0));
            dead_first += first_dead;
            skipped += st[4 * c + 2] < 5.0;
            if (st[4 * c + 2] == 0.0) {  // no update saw a positive weight: the ICPT is still the CPTs
                ++untouched;
                CHECK(memcmp(icpt.data() + 6 * c, M.prob.data(), sizeof(double) * 6) == 0);
            }
            if (st[4 * c + 1] == 0.0) {
                ++empty;
                CHECK(lab[c] == -1 && std::isinf(st[4 * c]) && st[4 * c] < 0.0);
                for (int j = 0; j < 4; ++j) CHECK(marg[4 * c + j] == 0.0);
            } else {
                CHECK(lab[c] == 1 && marg[4 * c] == 0.0 && std::fabs(marg[4 * c + 1] - 1.0) <= 1e-12);
            }
            CHECK(icpt[6 * c + 2] == 1.0 && icpt[6 * c + 3] == 0.0);  // the observed variable's rows
        }
        CHECK(dead_first > 0 && skipped > 0);
        printf("zero-weight stages, method %d: %d of %lld cases with a dead first stage, %d with a skipped update, %d never "
               "updated, %d empty estimates\n",
               method, dead_first, (long long)C, skipped, untouched, empty);
        // S = 1, no update: an A = 0 draw is the whole estimate
        CHECK(fbn::HostAis(M, method, ev.data(), C, 1, 0, 1, 1, 0, 0.01, lab.data(), marg.data(), st.data(), nullptr, nullptr,
                           nullptr, nullptr) == 0);
        empty = 0;
        for (int64_t c = 0; c < C; ++c)
            if (st[4 * c + 1] == 0.0) {
                ++empty;
                CHECK(lab[c] == -1 && std::isinf(st[4 * c]) && marg[4 * c + 1] == 0.0 && st[4 * c + 3] == 0.0);
            }
        CHECK(empty > 0);
    }
}

int main() {
    fbn::Network shapes;
    const std::vector<int32_t> dims = {5, 3, 7, 2, 4, 2, 2, 2, 2, 2, 2, 3, 1, 127, 6};
    const Lists graph = {{}, {0}, {}, {2, 0}, {0, 1, 2}, {}, {}, {}, {}, {}, {}, {5, 6, 7, 8, 9, 10}, {}, {12}, {1}};
    CHECK(Build(dims, graph, 15, 40, shapes) == 0);
    for (int method : {0, 1}) {
        CheckNetwork(shapes, method, 130, 3, 70, 3);  // 64 + 6 and 128 + 2: a partial chunk ends every stage
        CheckNetwork(shapes, method, 70, 2, 1, 3);    // an update after every sample
        CheckNetwork(shapes, method, 64, 2, 100, 3);  // SIS: S <= l, no update
        CheckNetwork(shapes, method, 1, 0, 1, 3);
    }
    CheckZeroWeightStage();
    fbn::SamplerModel SM;
    CHECK(fbn::BuildSamplerModel(shapes, SM) == 0);
    CHECK(fbn::CheckAisArgs(SM, 2, 1, 8, 1, 8, 0, -1.0) == FBN_ERR_ARG);
    CHECK(fbn::CheckAisArgs(SM, 0, 1, 0, 1, 8, 0, -1.0) == FBN_ERR_ARG);
    CHECK(fbn::CheckAisArgs(SM, 0, 1, 8, 1025, 8, 0, -1.0) == FBN_ERR_ARG);
    CHECK(fbn::CheckAisArgs(SM, 0, 1, 8, -1, 8, 0, -1.0) == FBN_ERR_ARG);
    CHECK(fbn::CheckAisArgs(SM, 0, 1, 8, 1, 0, 0, -1.0) == FBN_ERR_ARG);
    CHECK(fbn::CheckAisArgs(SM, 0, 1, 8, 1, 8, 0, 1.0) == FBN_ERR_ARG);
    CHECK(fbn::CheckAisArgs(SM, 0, 1, 8, 1, 8, 0, std::nan("")) == FBN_ERR_ARG);
    CHECK(fbn::CheckAisArgs(SM, 1, 1, 8, 1, 8, 0, 0.0) == FBN_ERR_ARG);
    CHECK(fbn::CheckAisArgs(SM, 0, 1, 8, 1, 8, 0, 0.0) == 0);
    CHECK(fbn::CheckAisArgs(SM, 0, 1, 8, 1024, (int64_t)1 << 52, 0, -1.0) == FBN_ERR_ARG);  // the stream overflows
    printf(g_fail ? "ais_host_check: %d failure(s)\n" : "ais_host_check: ok\n", g_fail);
    return g_fail ? 1 : 0;
}
