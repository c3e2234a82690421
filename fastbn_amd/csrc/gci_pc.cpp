// gci_pc.cpp -- the PC-stable skeleton search on continuous data: the level loop of RunPCGauss (gci.h).
// The tests come from a GciTester (the device's batches, capi_gci.hip; or the host twin's, gci_host.cpp),
// so both runs share every line below and differ only in who evaluates gci_elim.h.
#include <algorithm>
#include <cstdio>

#include "fbn_internal.h"
#include "gci.h"
#include "pc_search.h"

namespace fbn {

namespace {

// levels d >= 1: LevelSearch's rounds in two alternating halves (RunLevel's shape, pc_driver.cpp)
int GaussLevel(GciTester &T, const Skeleton &sk, int d, double tau, const int32_t *ones, LevelOut &out, PCResultHost &res) {
    SearchSchedule sch;  // (the knobs: test overrides, read per level)
    sch.round0 = KnobOr("FBN_PC_ROUND0", sch.round0);
    sch.growth = KnobOr("FBN_PC_GROWTH", sch.growth);
    sch.full_spec = KnobOr("FBN_PC_FULLSPEC", sch.full_spec);
    sch.pipeline_edges = KnobOr("FBN_PC_PIPELINE_EDGES", sch.pipeline_edges);
    sch.general = KnobSet("FBN_PC_GEN_GENERAL");
    LevelSearch search(sk, 0, sk.edges.size(), d, 1, ones, sch);
    std::vector<uint8_t> indep[2];
    out.d = d;
    out.counted = out.launched = 0;
    auto launch = [&](int h) -> int {  // generate + launch half h's next round; 0 tests = done
        if (!search.Generate(h)) return FBN_OK;
        const int64_t nt = search.tests(h);
        indep[h].resize((size_t)nt);
        if (int rc = T.Launch(h, search.items(h).data(), nt, d, tau)) return rc;
        out.launched += nt;
        return FBN_OK;
    };
    const int nh = search.halves();
    for (int h = 0; h < nh; ++h)
        if (int rc = launch(h)) return rc;
    while (true) {
        bool any = false;
        for (int h = 0; h < nh; ++h) {
            if (search.tests(h) == 0) continue;
            any = true;
            if (int rc = T.Wait(h, indep[h].data(), res)) return rc;
            search.Resolve(h, indep[h].data(), nullptr);  // (group size 1: df is not read)
            if (int rc = launch(h)) return rc;
        }
        if (!any) break;
    }
    search.Finish(out);
    return FBN_OK;
}

}  // namespace

int RunPCGauss(GciTester &T, int nvars, int64_t N, double alpha, int depth, PCResultHost &res) {
    if (nvars < 1 || depth < 1) return SetError(FBN_ERR_ARG, "bad argument");
    const auto t0 = Clock::now();
    res = PCResultHost();
    res.num_nodes = nvars;
    Skeleton sk;
    sk.Reset(nvars);
    const int64_t P = (int64_t)nvars * (nvars - 1) / 2;
    double tau = 0.0;
    if (int rc = GciTau(alpha, N, 0, &tau)) return rc;
    // level 0: every pair of the implicit complete graph, decoded from the test index; the kept pairs
    // become the skeleton
    std::vector<char> removed((size_t)P);
    static_assert(sizeof(char) == sizeof(uint8_t), "flag layout");
    if (P > 0) {
        if (int rc = T.Launch(0, nullptr, P, 0, tau)) return rc;
        if (int rc = T.Wait(0, reinterpret_cast<uint8_t *>(removed.data()), res)) return rc;
    }
    res.tests_per_level.push_back(P);
    res.launched_per_level.push_back(P);
    int64_t k = 0;
    for (int i = 0; i < nvars; ++i)
        for (int j = i + 1; j < nvars; ++j, ++k)
            if (!removed[(size_t)k]) sk.edges.push_back({i, j});
    res.sepset.set_level0(nvars, std::move(removed));
    sk.RebuildAdj(true);
    const std::vector<int32_t> ones((size_t)nvars, 1);  // LevelSearch's batch statistics are not used here
    for (int d = 1; d < std::max(depth, 1); ++d) {  // (RunLevels' loop, pc_driver.cpp: level 1 always runs)
        if (d > kMaxD) return SetError(FBN_ERR_LIMIT, "conditioning set size %d (supported 0..%d)", d, kMaxD);
        if (int rc = GciTau(alpha, N, d, &tau)) return rc;
        LevelOut out;
        if (int rc = GaussLevel(T, sk, d, tau, ones.data(), out, res)) return rc;
        res.sepset.append_level(sk.edges.data(), out.removed.data(), out.sep.data(), sk.edges.size(), d);
        res.tests_per_level.push_back(out.counted);
        res.launched_per_level.push_back(out.launched);
        sk.ApplyRemovals(out.removed);
        if (!sk.ContinueAfter(d)) break;
    }
    res.edges = sk.edges;
    GciLog log;
    if (int rc = T.Log(&log)) return rc;
    res.min_margin = log.min_margin, res.near_alpha = log.near, res.degenerate = log.degenerate;
    res.margin_done = true;
    res.total_s = std::chrono::duration<double>(Clock::now() - t0).count();
    return OrientPC(nvars, res);
}

}  // namespace fbn
