// em_host_check.cpp -- stand-alone driver of the EM plan compiler, host twin, M-step and potential rebuild
// (fastbn_amd/csrc/jt_em_plan.cpp, jt_em_host.cpp) for host sanitizer runs (no device, no libfastbn):
//   c++ -std=c++17 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/em_host_check.cpp fastbn_amd/csrc/jt_em_plan.cpp fastbn_amd/csrc/jt_em_host.cpp \
//       fastbn_amd/csrc/jt_mpe_plan.cpp fastbn_amd/csrc/jt_mpe_host.cpp fastbn_amd/csrc/jt_plan.cpp \
//       fastbn_amd/csrc/io.cpp fastbn_amd/csrc/synth.cpp -pthread -o em_host_check && ./em_host_check
// Builds the forest plan and the EM program for ALARM and for a 1,200-node binary chain, checks that the
// rebuild of the potentials from theta gives the plan's own potentials to the byte, runs the host E-step
// on three rows each (nothing observed, some observed, all observed) and checks that every family's
// posterior cells sum to 1, that the complete row puts exactly 1.0 on one cell per family, that the counts
// are the posteriors added in row order, and that two M-step / rebuild / E-step rounds run clean and give
// the same bytes twice.  Exits non-zero on a wrong answer.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../fastbn_amd/csrc/fbn_internal.h"
#include "../fastbn_amd/csrc/jt_em_program.h"

static int g_fail = 0;
#define CHECK(cond)                                              \
    do {                                                         \
        if (!(cond)) {                                           \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_fail;                                            \
        }                                                        \
    } while (0)

static void CheckNetwork(const char *name, const fbn::Network &net, const std::vector<int8_t> &ev, int64_t ncases) {
    const int V = net.n();
    fbn::JTPlanHost plan;
    fbn::JTProgramEm P;
    CHECK(fbn::BuildJTPlan(net, plan, /*forest=*/true) == FBN_OK);
    CHECK(fbn::CompileJTProgramEm(net, plan, P) == FBN_OK);
    CHECK(P.store_rows == std::max<int64_t>(2 * P.M.msg_rows + P.M.nsep, 1) && (int64_t)P.theta.size() == P.cells);
    std::vector<double> iv(P.M.initv.size());
    fbn::EmRebuildPotentials(P, P.theta.data(), iv.data());
    CHECK(std::memcmp(iv.data(), P.M.initv.data(), iv.size() * 8) == 0);
    CHECK(fbn::CheckMpeEvidence(P.M, ev.data(), ncases) == FBN_OK);
    std::vector<double> first;
    for (int round = 0; round < 2; ++round) {
        std::vector<double> counts((size_t)P.cells), c2 = counts, val((size_t)ncases * 2), post((size_t)(ncases * P.cells));
        CHECK(fbn::HostEmEstep(P, ev.data(), ncases, counts.data(), val.data(), nullptr) == FBN_OK);
        CHECK(fbn::HostEmEstep(P, ev.data(), ncases, c2.data(), nullptr, post.data()) == FBN_OK);
        CHECK(std::memcmp(counts.data(), c2.data(), counts.size() * 8) == 0);
        std::vector<double> sum((size_t)P.cells, 0.0);
        for (int64_t c = 0; c < ncases; ++c) {
            for (int64_t i = 0; i < P.cells; ++i) sum[i] = sum[i] + post[c * P.cells + i];
            for (int v = 0; v < V; ++v) {
                const int32_t *r = &P.node_rec[3 * v];
                double s = 0.0;
                int ones = 0;
                for (int64_t i = r[0]; i < r[0] + (int64_t)r[1] * r[2]; ++i) s += post[c * P.cells + i], ones += post[c * P.cells + i] == 1.0;
                CHECK(std::fabs(s - 1.0) <= 4.0 * (P.M.entries + 3.0 * V) * 0x1p-53);
                if (c == 2) CHECK(ones == 1 && s == 1.0);
            }
            CHECK(val[2 * c] >= 0.5 && val[2 * c] < 1.0 && val[2 * c + 1] == std::floor(val[2 * c + 1]));
        }
        CHECK(std::memcmp(sum.data(), counts.data(), sum.size() * 8) == 0);
        printf("%s round %d: P(e) of the rows = %.6g * 2^%g, %.6g * 2^%g, %.6g * 2^%g\n", name, round, val[0], val[1], val[2],
               val[3], val[4], val[5]);
        if (round == 0) first = counts;
        fbn::EmMstep(P, counts.data(), 1.0, P.theta.data());
        fbn::EmRebuildPotentials(P, P.theta.data(), P.M.initv.data());
        for (double t : P.theta) CHECK(t > 0.0 && t < 1.0 + 1e-15);
    }
    std::vector<int8_t> bad(ev.begin(), ev.begin() + V);
    bad[V - 1] = (int8_t)net.dom[V - 1];
    CHECK(fbn::CheckMpeEvidence(P.M, bad.data(), 1) == FBN_ERR_ARG);
    std::vector<double> theta;
    CHECK(fbn::EmThetaFromNetwork(P, net, net, theta) == FBN_OK && (int64_t)theta.size() == P.cells);
}

// none observed, every step-th variable observed, all observed: the observed codes from a forward sample
static std::vector<int8_t> Cases(const fbn::Network &net, int step) {
    const int V = net.n();
    std::vector<uint8_t> full((size_t)V);
    CHECK(fbn::ForwardSample(net, 1, 5, full.data()) == FBN_OK);
    std::vector<int8_t> ev((size_t)3 * V, -1);
    for (int v = 0; v < V; ++v) {
        if (v % step == 0) ev[(size_t)V + v] = (int8_t)full[v];
        ev[(size_t)2 * V + v] = (int8_t)full[v];
    }
    return ev;
}

int main(int argc, char **argv) {
    const char *xml = argc > 1 ? argv[1] : "tests/golden/alarm/alarm.xml";
    fbn::Network alarm;
    if (fbn::LoadXmlbif(xml, alarm) != FBN_OK) {
        printf("FAIL: %s: %s\n", xml, fbn::LastError());
        return 1;
    }
    CheckNetwork("alarm", alarm, Cases(alarm, 5), 3);

    const int N = 1200;
    std::mt19937 rng(1200);
    std::vector<int32_t> dims(N, 2), off(N + 1, 0), par;
    std::vector<int64_t> counts;
    for (int v = 0; v < N; ++v) {
        if (v > 0) par.push_back(v - 1);
        off[v + 1] = (int32_t)par.size();
        for (int k = 0; k < (v > 0 ? 4 : 2); ++k) counts.push_back(1 + (int64_t)(rng() % 9));
    }
    fbn::Network chain;
    CHECK(fbn::BuildNetwork(N, dims.data(), off.data(), par.data(), counts.data(), nullptr, chain) == FBN_OK);
    CheckNetwork("chain", chain, Cases(chain, 10), 3);

    // a probability network: validation, and Prob returns the entries
    std::vector<int32_t> d2{2, 2}, o2{0, 0, 1}, p2{0};
    std::vector<double> cpt{0.25, 0.75, 0.5, 0.125, 0.5, 0.875};
    fbn::Network pn;
    CHECK(fbn::BuildNetworkCpt(2, d2.data(), o2.data(), p2.data(), cpt.data(), nullptr, pn) == FBN_OK);
    const int one = 1;
    CHECK(pn.Prob(1, 1, &one) == 0.875 && pn.Prob(0, 1, nullptr) == 0.75);
    cpt[5] = 0.9;
    CHECK(fbn::BuildNetworkCpt(2, d2.data(), o2.data(), p2.data(), cpt.data(), nullptr, pn) == FBN_ERR_ARG);

    if (g_fail) {
        printf("%d check(s) failed\n", g_fail);
        return 1;
    }
    printf("em_host_check ok\n");
    return 0;
}
