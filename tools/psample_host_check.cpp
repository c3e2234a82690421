// psample_host_check.cpp -- stand-alone driver of the posterior sampler's program and host twin
// (fastbn_amd/csrc/jt_mpe_plan.cpp, jt_psample_host.cpp) for host sanitizer runs (no device, no libfastbn):
//   c++ -std=c++17 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/psample_host_check.cpp fastbn_amd/csrc/jt_psample_host.cpp fastbn_amd/csrc/jt_mpe_plan.cpp \
//       fastbn_amd/csrc/jt_mpe_host.cpp fastbn_amd/csrc/jt_plan.cpp fastbn_amd/csrc/sample_host.cpp \
//       fastbn_amd/csrc/io.cpp fastbn_amd/csrc/synth.cpp -pthread \
//       -o psample_host_check && ./psample_host_check [tests/golden/alarm/alarm.xml]
// Builds the forest plan and the program for ALARM and for a 1,200-node binary chain (seeded counts in
// 1..9), draws 7 samples for a few cases each (nothing observed, a few variables observed, a complete
// forward sample) and checks that every sample is complete, in range and carries its evidence, that a
// complete row returns itself, that the value is a mantissa in [0.5, 1) with an integral exponent, that two
// runs give the same bytes, that a batch split with case_offset gives the same bytes, and the shape limits.
// Exits non-zero on a wrong answer.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../fastbn_amd/csrc/fbn_internal.h"
#include "../fastbn_amd/csrc/jt_psample_program.h"

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
    const int64_t S = 7, off = 11;
    fbn::JTPlanHost plan;
    fbn::JTProgramMpe P;
    CHECK(fbn::BuildJTPlan(net, plan, /*forest=*/true) == FBN_OK);
    CHECK(fbn::CompileJTProgramMpe(plan, P) == FBN_OK);
    CHECK(fbn::CheckMpeEvidence(P, ev.data(), ncases) == FBN_OK);
    CHECK(fbn::CheckPsampleShape(P, ncases, S, off) == FBN_OK);
    CHECK(fbn::CheckPsampleShape(P, ncases, 0, off) == FBN_ERR_ARG);
    CHECK(fbn::CheckPsampleShape(P, 2, (int64_t)1 << 30, 0) == FBN_ERR_LIMIT);
    std::vector<int8_t> x((size_t)(ncases * S) * V, -9), x2 = x;
    std::vector<double> val((size_t)ncases * 2), val2 = val;
    CHECK(fbn::HostPsample(P, ev.data(), ncases, S, 3, off, x.data(), val.data()) == FBN_OK);
    CHECK(fbn::HostPsample(P, ev.data(), ncases, S, 3, off, x2.data(), val2.data()) == FBN_OK);
    CHECK(x == x2 && std::memcmp(val.data(), val2.data(), val.size() * 8) == 0);
    // the batch split after its first case
    std::fill(x2.begin(), x2.end(), (int8_t)-9);
    CHECK(fbn::HostPsample(P, ev.data(), 1, S, 3, off, x2.data(), val2.data()) == FBN_OK);
    CHECK(fbn::HostPsample(P, ev.data() + V, ncases - 1, S, 3, off + 1, x2.data() + S * V, val2.data() + 2) == FBN_OK);
    CHECK(x == x2 && std::memcmp(val.data(), val2.data(), val.size() * 8) == 0);
    CHECK(fbn::CheckCaseValues("psample", val.data(), ncases) == FBN_OK);
    for (int64_t c = 0; c < ncases; ++c) {
        const int8_t *e = &ev[(size_t)c * V];
        bool complete = true;
        for (int v = 0; v < V; ++v) complete = complete && e[v] >= 0;
        for (int64_t s = 0; s < S; ++s) {
            const int8_t *r = &x[(size_t)(c * S + s) * V];
            bool ok = true;
            for (int v = 0; v < V; ++v) ok = ok && r[v] >= 0 && r[v] < net.dom[v] && (e[v] < 0 || e[v] == r[v]);
            CHECK(ok);
            if (complete) CHECK(std::memcmp(r, e, (size_t)V) == 0);
        }
        const double vm = val[2 * c], vex = val[2 * c + 1];
        CHECK(vm >= 0.5 && vm < 1.0 && vex == std::floor(vex));
        printf("%s case %lld: P(e) = %.17g * 2^%lld\n", name, (long long)c, vm, (long long)vex);
    }
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

    if (g_fail) {
        printf("%d check(s) failed\n", g_fail);
        return 1;
    }
    printf("psample_host_check ok\n");
    return 0;
}
