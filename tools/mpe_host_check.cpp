// mpe_host_check.cpp -- stand-alone driver of the max-product plan compiler and host twin
// (fastbn_amd/csrc/jt_mpe_plan.cpp, jt_mpe_host.cpp) for host sanitizer runs (no device, no libfastbn):
//   c++ -std=c++17 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/mpe_host_check.cpp fastbn_amd/csrc/jt_mpe_plan.cpp fastbn_amd/csrc/jt_mpe_host.cpp \
//       fastbn_amd/csrc/jt_plan.cpp fastbn_amd/csrc/io.cpp fastbn_amd/csrc/synth.cpp -pthread \
//       -o mpe_host_check && ./mpe_host_check [tests/golden/alarm/alarm.xml]
// Builds the forest plan and the program for ALARM and for a 1,200-node binary chain (seeded counts in
// 1..9), runs the host twin on a few cases each (nothing observed, a few variables observed, a complete
// forward sample) and checks that every assignment is complete, in range and agrees with its evidence,
// that the product of its CPT entries equals the reported value m * 2^ex (within 4 V 2^-53: the bound
// 3 V 2^-53 of the value plus the V multiplies of this check), that the stored messages lie in [0, 1),
// and that two runs give the same bytes.  Exits non-zero on a wrong answer.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../fastbn_amd/csrc/fbn_internal.h"
#include "../fastbn_amd/csrc/jt_mpe_program.h"

static int g_fail = 0;
#define CHECK(cond)                                              \
    do {                                                         \
        if (!(cond)) {                                           \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_fail;                                            \
        }                                                        \
    } while (0)

// (m, ex) of the product of the assignment's CPT entries, rescaled by powers of two only
static void CptProduct(const fbn::Network &net, const int8_t *x, double *m, long long *ex) {
    *m = 1.0, *ex = 0;
    std::vector<int> pv;
    for (int v = 0; v < net.n(); ++v) {
        pv.clear();
        for (int p : net.parents_asc[v]) pv.push_back(x[p]);
        int k = 0;
        *m = std::frexp(*m * net.Prob(v, x[v], pv.data()), &k);
        *ex += k;
    }
}

static void CheckNetwork(const char *name, const fbn::Network &net, const std::vector<int8_t> &ev, int64_t ncases) {
    const int V = net.n();
    fbn::JTPlanHost plan;
    fbn::JTProgramMpe P;
    CHECK(fbn::BuildJTPlan(net, plan, /*forest=*/true) == FBN_OK);
    CHECK(fbn::CompileJTProgramMpe(plan, P) == FBN_OK);
    CHECK(P.V == V && (int)P.cl.size() == (int)plan.cliques.size() && P.collect.size() == P.cl.size() &&
          P.trace.size() == P.cl.size());
    CHECK(P.store_rows == P.msg_rows + P.nsep + (int64_t)P.cl.size());
    CHECK(fbn::CheckMpeEvidence(P, ev.data(), ncases) == FBN_OK);
    std::vector<int8_t> a((size_t)ncases * V, -9), a2 = a;
    std::vector<double> val((size_t)ncases * 2), val2 = val, msg((size_t)ncases * P.msg_rows);
    std::vector<int32_t> exps((size_t)ncases * P.nsep);
    CHECK(fbn::HostMpe(P, ev.data(), ncases, a.data(), val.data(), msg.data(), exps.data()) == FBN_OK);
    CHECK(fbn::HostMpe(P, ev.data(), ncases, a2.data(), val2.data(), nullptr, nullptr) == FBN_OK);
    CHECK(a == a2 && std::memcmp(val.data(), val2.data(), val.size() * 8) == 0);
    for (double x : msg) CHECK(x >= 0.0 && x < 1.0);
    for (int64_t c = 0; c < ncases; ++c) {
        const int8_t *x = &a[(size_t)c * V], *e = &ev[(size_t)c * V];
        bool ok = true;
        for (int v = 0; v < V; ++v) ok = ok && x[v] >= 0 && x[v] < net.dom[v] && (e[v] < 0 || e[v] == x[v]);
        CHECK(ok);
        if (!ok) continue;
        double m;
        long long ex;
        CptProduct(net, x, &m, &ex);
        const double vm = val[2 * c], vex = val[2 * c + 1];
        CHECK(vm >= 0.5 && vm < 1.0 && vex == std::floor(vex));
        const double ratio = std::ldexp(m / vm, (int)(ex - (long long)vex));
        CHECK(std::fabs(ratio - 1.0) <= 4.0 * V * 0x1p-53);
        printf("%s case %lld: P(x*, e) = %.17g * 2^%lld, CPT product / value - 1 = %.3g\n", name, (long long)c, vm,
               (long long)vex, ratio - 1.0);
    }
    // a bad code is named, not indexed with
    std::vector<int8_t> bad(ev.begin(), ev.begin() + V);
    bad[V - 1] = (int8_t)net.dom[V - 1];
    CHECK(fbn::CheckMpeEvidence(P, bad.data(), 1) == FBN_ERR_ARG);
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
    printf("mpe_host_check ok\n");
    return 0;
}
