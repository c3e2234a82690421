// gibbs_host_check.cpp -- stand-alone driver of the Gibbs sampler's host side
// (fastbn_amd/csrc/gibbs_host.cpp, gibbs_model.h over sample_host.cpp) for host sanitizer runs (no device,
// no libfastbn):
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -Iinclude \
//       tools/gibbs_host_check.cpp fastbn_amd/csrc/gibbs_host.cpp fastbn_amd/csrc/sample_host.cpp \
//       fastbn_amd/csrc/synth.cpp fastbn_amd/csrc/io.cpp -pthread -o gibbs_host_check && ./gibbs_host_check
// A seeded network with every family shape of tests/test_gpu_param.py's 15-node graph (a 1-state and a
// 127-state node, six parents): one lane, a tail lane, two chunks; values in range and clamped, rows that
// sum to 1, repeatability, batch-split invariance, conditionals that sum to 1, the error returns.  A
// hand-built A -> B with P(B = 1 | A = 0) = 0 exactly (no Network holds a zero) and B = 1 observed drives the
// dead ends: a chain started at A = 0 has g = (0.9 * 0, 0.1 * p1), so it enters the support in its first sweep
// and never leaves it; with both columns of B = 1 zero, tot == 0 everywhere and A keeps its start.  GibbsConditional is the
// function the kernel compiles, so an index out of range here is one there.  Exits non-zero on a wrong answer.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../fastbn_amd/csrc/fbn_internal.h"
#include "../fastbn_amd/csrc/gibbs_model.h"

static int g_fail = 0;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            printf("FAIL %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, fbn::LastError()); \
            ++g_fail;                                                                     \
        }                                                                                 \
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

static void CheckNetwork(const fbn::Network &net, int64_t chains, int64_t burn_in, int64_t sweeps, int nobs) {
    fbn::SamplerModel SM;
    fbn::GibbsModel GM;
    CHECK(fbn::BuildSamplerModel(net, SM) == 0 && fbn::BuildGibbsModel(SM, GM) == 0);
    const int V = SM.V, SD = SM.sum_dom;
    const int64_t C = 7;
    std::vector<uint8_t> full((size_t)V * C);
    CHECK(fbn::ForwardSample(net, C, 3, full.data()) == 0);
    std::vector<int8_t> ev((size_t)C * V, -1);
    std::mt19937 rng(99);
    for (int64_t c = 1; c < C; ++c)
        for (int k = 0; k < nobs; ++k) {
            const int v = (int)(rng() % (uint32_t)V);
            ev[c * V + v] = (int8_t)full[(size_t)v * C + c];
        }
    CHECK(fbn::CheckGibbsShape(SM, C, chains, burn_in, sweeps, 2) == 0);
    std::vector<int32_t> lab(C), lab2(C);
    std::vector<double> marg((size_t)C * SD), marg2((size_t)C * SD);
    std::vector<int8_t> st((size_t)C * chains * V), st2(st.size());
    CHECK(fbn::HostGibbs(SM, GM, ev.data(), C, chains, burn_in, sweeps, 5, 2, lab.data(), marg.data(), st.data()) == 0);
    // the split 3 + 4, no marginals buffer for the first part
    CHECK(fbn::HostGibbs(SM, GM, ev.data(), 3, chains, burn_in, sweeps, 5, 2, lab2.data(), nullptr, st2.data()) == 0);
    CHECK(fbn::HostGibbs(SM, GM, ev.data() + 3 * V, 4, chains, burn_in, sweeps, 5, 5, lab2.data() + 3, marg2.data() + 3 * SD,
                         st2.data() + 3 * chains * V) == 0);
    CHECK(lab == lab2 && st == st2 && memcmp(marg.data() + 3 * SD, marg2.data() + 3 * SD, sizeof(double) * 4 * SD) == 0);
    for (int64_t c = 0; c < C; ++c) {
        for (int v = 0, j = 0; v < V; j += SM.dom[(size_t)v], ++v) {
            double sum = 0.0;
            for (int q = 0; q < SM.dom[(size_t)v]; ++q) sum += marg[c * SD + j + q];
            CHECK(ev[c * V + v] >= 0 ? sum == 0.0 : std::fabs(sum - 1.0) <= 1e-12);
            for (int64_t i = 0; i < chains; ++i) {
                const int x = st[(c * chains + i) * V + v];
                CHECK(x >= 0 && x < SM.dom[(size_t)v] && (ev[c * V + v] < 0 || x == ev[c * V + v]));
            }
        }
    }
    // the conditionals of the last states of case 0
    std::vector<double> cond((size_t)chains * SD);
    CHECK(fbn::CheckGibbsStates(SM, st.data(), chains) == 0);
    CHECK(fbn::HostGibbsConditionals(SM, GM, st.data(), chains, cond.data()) == 0);
    for (int64_t i = 0; i < chains; ++i)
        for (int v = 0, j = 0; v < V; j += SM.dom[(size_t)v], ++v) {
            double sum = 0.0;
            for (int q = 0; q < SM.dom[(size_t)v]; ++q) sum += cond[i * SD + j + q];
            CHECK(std::fabs(sum - 1.0) <= 1e-12);
        }
}

// A -> B, B = 1 observed.  p1: P(B = 1 | A = 1); P(B = 1 | A = 0) = 0 exactly.
static void CheckDeadEnds(double p1) {
    fbn::SamplerModel M;
    M.V = 2, M.sum_dom = 4, M.cells = 6;
    M.dom = {2, 2};
    M.nodes = {fbn::SampleNode{0, 2, 0, 0, 0, 0}, fbn::SampleNode{1, 2, 1, 0, 2, 2}};
    M.par = {0, 2};
    M.prob = {0.9, 0.1, 1.0, 0.0, 1.0 - p1, p1};
    M.cdf = {0.9, 1.0, 1.0, 1.0, 1.0 - p1, 1.0};
    M.ent = {0, 1, 1 << 8, 1 << 8 | 1};
    fbn::GibbsModel GM;
    CHECK(fbn::BuildGibbsModel(M, GM) == 0);
    CHECK(GM.coff == (std::vector<int32_t>{0, 1, 1}) && GM.child[0] == 1 && GM.child[1] == 1);
    const int64_t C = 4, chains = 70;
    std::vector<int8_t> ev{-1, 1, -1, 1, -1, 1, -1, 1}, st0((size_t)C * chains * 2), st((size_t)C * chains * 2);
    std::vector<int32_t> lab(C);
    std::vector<double> marg((size_t)C * 4);
    // burn_in 0, one sweep: the start is the prior draw of A (some chains start at A = 0, a dead end for B)
    CHECK(fbn::HostGibbs(M, GM, ev.data(), C, chains, 0, 1, 1, 0, lab.data(), marg.data(), st.data()) == 0);
    int zeros = 0;
    for (size_t i = 0; i < st.size(); i += 2) zeros += st[i] == 0;
    for (int64_t c = 0; c < C; ++c) {
        for (int j = 0; j < 4; ++j) CHECK(std::isfinite(marg[4 * c + j]));
        CHECK(std::fabs(marg[4 * c] + marg[4 * c + 1] - 1.0) <= 1e-12 && marg[4 * c + 2] == 0.0 && marg[4 * c + 3] == 0.0);
    }
    if (p1 > 0.0) {  // g = (0.9 * 0, 0.1 * p1): every chain is at A = 1 after its first sweep, with certainty
        CHECK(zeros == 0);
        for (int64_t c = 0; c < C; ++c) CHECK(marg[4 * c] == 0.0 && marg[4 * c + 1] == 1.0 && lab[c] == 1);
    } else {  // tot == 0 for every chain: the start is kept, the estimator counts the kept value
        CHECK(fbn::HostGibbs(M, GM, ev.data(), C, chains, 3, 2, 1, 0, lab.data(), nullptr, st0.data()) == 0);
        CHECK(zeros > 0 && zeros < (int)(C * chains));
        for (int64_t c = 0; c < C; ++c) {
            int kept = 0;
            for (int64_t i = 0; i < chains; ++i) kept += st[(size_t)(c * chains + i) * 2] == 0;
            CHECK(marg[4 * c] == (double)kept / (double)chains);
        }
        int zeros3 = 0;
        for (size_t i = 0; i < st0.size(); i += 2) zeros3 += st0[i] == 0;
        printf("dead ends: %d of %lld chains keep A = 0 after one sweep, %d after five\n", zeros, (long long)(C * chains), zeros3);
    }
}

int main() {
    fbn::Network shapes;
    const std::vector<int32_t> dims = {5, 3, 7, 2, 4, 2, 2, 2, 2, 2, 2, 3, 1, 127, 6};
    const Lists graph = {{}, {0}, {}, {2, 0}, {0, 1, 2}, {}, {}, {}, {}, {}, {}, {5, 6, 7, 8, 9, 10}, {}, {12}, {1}};
    CHECK(Build(dims, graph, 15, 40, shapes) == 0);
    CheckNetwork(shapes, 1, 0, 1, 3);
    CheckNetwork(shapes, 63, 2, 3, 3);
    CheckNetwork(shapes, 130, 1, 2, 6);
    CheckDeadEnds(0.75);
    CheckDeadEnds(0.0);
    fbn::SamplerModel SM;
    CHECK(fbn::BuildSamplerModel(shapes, SM) == 0);
    CHECK(fbn::CheckGibbsShape(SM, 1, 0, 0, 1, 0) == FBN_ERR_ARG);
    CHECK(fbn::CheckGibbsShape(SM, 1, 1, -1, 1, 0) == FBN_ERR_ARG);
    CHECK(fbn::CheckGibbsShape(SM, 1, 1, 0, 0, 0) == FBN_ERR_ARG);
    CHECK(fbn::CheckGibbsShape(SM, 1, 1, 0, 1, -1) == FBN_ERR_ARG);
    CHECK(fbn::CheckGibbsShape(SM, 1, (int64_t)1 << 40, 0, (int64_t)1 << 20, 0) == FBN_ERR_ARG);  // the stream overflows
    CHECK(fbn::CheckGibbsShape(SM, (int64_t)1 << 31, 1, 0, 1, 0) == FBN_ERR_LIMIT);
    CHECK(fbn::CheckGibbsShape(SM, 0, 1, 0, 1, 0) == 0);
    std::vector<int8_t> bad((size_t)SM.V, 0);
    bad[3] = 2;
    CHECK(fbn::CheckGibbsStates(SM, bad.data(), 1) == FBN_ERR_ARG);
    printf(g_fail ? "gibbs_host_check: %d failure(s)\n" : "gibbs_host_check: ok\n", g_fail);
    return g_fail ? 1 : 0;
}
