// pc_driver.cpp -- PC-stable skeleton search driven from the host, CI tests on the device.
//
// Semantics are the reference's sequential (t = 1) ones (src/PCStable.cpp:49-563):
//   * level 0 tests every edge of the complete graph marginally;
//   * level d >= 1 works on a snapshot of the adjacencies; for edge (x, y) (x < y) the candidate
//     conditioning sets are the size-d subsets of adj(x)\{y} in ChoiceGenerator order, then those
//     of adj(y)\{x}; the first independent one removes the edge and becomes its sepset;
//   * with -g gs > 1, sets are evaluated in groups of gs per side (NextN), the whole group counts,
//     and a df == 0 result inside a group of size > 1 is a dependence (src/IndependenceTest.cpp:262-271);
//   * removals are applied after the level in vec_edges order; the search continues while
//     FreeDegree > d.
// RunPCStable picks one way of doing level 0 (the Start* steps), then runs the level loop; RunLevel
// runs one level's tests, which a LevelSearch (pc_search.h) generates round by round and resolves.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fbn_internal.h"
#include "pc_search.h"

namespace fbn {

namespace {

// levels whose candidate sets number at most this many run in a single round (FBN_PC_FULLSPEC: test
// and diagnostic override, read per level)
int64_t FullSpeculation() { return KnobOr("FBN_PC_FULLSPEC", 16384); }
int64_t L0Chunk() { return std::max<int64_t>(1, KnobOr("FBN_PC_L0CHUNK", (int64_t)1 << 22)); }

// Level 0 of an edge range: one marginal test per edge (src/PCStable.cpp:73-157)
int RunLevel0(fbn_ci_ctx *ctx, double alpha, const Skeleton &sk, size_t e_begin, size_t e_end, LevelOut &out,
              PCResultHost &res) {
    const auto &edges = sk.edges;
    const size_t E = e_end - e_begin;
    out.removed.assign(E, 0);
    out.sep.clear();
    // the (x, y) pairs of the edge range are the items, in place (pair<int, int> = two ints)
    static_assert(sizeof(std::pair<int, int>) == 2 * sizeof(int32_t), "pair layout");
    const int32_t *pairs = reinterpret_cast<const int32_t *>(edges.data() + e_begin);
    // statistics of the pairs without the validation pass (they come from the skeleton); for
    // the whole complete graph in closed form: every variable is in nv - 1 pairs
    const int32_t *dims = CiCtxDims(ctx);
    int nv = 0;
    int64_t ns = 0;
    CiCtxShape(ctx, &nv, &ns);
    CiBatchStats st0{0, 0};
    if (e_begin == 0 && (int64_t)E == (int64_t)nv * (nv - 1) / 2 && edges.size() == E) {
        st0 = CiAllPairsStats(dims, nv);
    } else {
        for (size_t e = e_begin; e < e_end; ++e) {
            const int a = dims[edges[e].first], b = dims[edges[e].second];
            st0.dim_rows += a + b, st0.maxdim = std::max(st0.maxdim, std::max(a, b));
        }
    }
    // the complete graph (a PC run's level 0): edge index = pair index, the kernels decode the
    // pairs of the range themselves
    const bool all_pairs = (int64_t)edges.size() == (int64_t)nv * (nv - 1) / 2 && CiAllPairsEligible(ctx, st0);
    int rc = all_pairs ? CiBatchLaunchAllPairs(ctx, alpha, &st0, (int64_t)e_begin, (int64_t)E)
                       : CiBatchLaunch(ctx, 0, pairs, (int64_t)E, 0, alpha, false, &st0);
    if (rc) return rc;
    // the device's 0/1 decisions land in the removal flags directly
    static_assert(sizeof(char) == sizeof(uint8_t), "flag layout");
    rc = CiBatchWait(ctx, 0, reinterpret_cast<uint8_t *>(out.removed.data()), nullptr, res);
    if (rc) return rc;
    out.counted = out.launched = (int64_t)E;
    return FBN_OK;
}

}  // namespace

int RunImplicitLevel0(fbn_ci_ctx *ctx, double alpha, const CiBatchStats &st, int64_t t0, int64_t t1, uint8_t *flags,
                      std::vector<std::pair<int, int>> *kept, PCResultHost &res, double *ms) {
    const int64_t chunk = L0Chunk();
    for (int64_t t = t0; t < t1; t += chunk) {
        const int64_t m = std::min(chunk, t1 - t);
        const auto q0 = Clock::now();
        if (int rc = CiBatchLaunchAllPairs(ctx, alpha, &st, t, m)) return rc;
        if (int rc = CiBatchWait(ctx, 0, flags + (t - t0), nullptr, res)) return rc;
        const auto q1 = Clock::now();
        if (kept)
            if (int rc = CiAllPairsKept(ctx, t, m, *kept)) return rc;
        if (ms) ms[0] += Ms(q0, q1), ms[1] += Ms(q1, Clock::now());
    }
    return FBN_OK;
}

// One level of the skeleton search for the edges [e_begin, e_end) of sk (vec_edges order), against
// sk's adjacency snapshot.  Level 0: one marginal test per edge; level d >= 1: SearchAtDepth /
// CheckEdge semantics (see file header).  Outputs per edge of the range: removed flag and, if
// removed, its sepset (sorted).
int RunLevel(fbn_ci_ctx *ctx, double alpha, int d, int group_size, const Skeleton &sk, size_t e_begin, size_t e_end,
             LevelOut &out, PCResultHost &res, const std::function<void()> &deferred) {
    out.d = d;
    out.counted = out.launched = 0;
    if (d == 0) return RunLevel0(ctx, alpha, sk, e_begin, e_end, out, res);
    if (d > kMaxD) return SetError(FBN_ERR_LIMIT, "conditioning set size %d (supported 0..%d)", d, kMaxD);
    if (d == 1 && group_size == 1) {  // the whole level on the device when eligible
        bool done = false;
        if (int rc = CiLevel1Device(ctx, alpha, sk, e_begin, e_end, out, res, &done)) return rc;
        if (done) return FBN_OK;
    }
    SearchSchedule sch;  // (the knobs: test and diagnostic overrides, read per level)
    sch.round0 = KnobOr("FBN_PC_ROUND0", sch.round0);
    sch.growth = KnobOr("FBN_PC_GROWTH", sch.growth);
    sch.full_spec = FullSpeculation();
    sch.pipeline_edges = KnobOr("FBN_PC_PIPELINE_EDGES", sch.pipeline_edges);
    sch.general = KnobSet("FBN_PC_GEN_GENERAL");
    LevelSearch search(sk, e_begin, e_end, d, group_size, CiCtxDims(ctx), sch);
    const bool timing = PcTiming();
    std::vector<uint8_t> indep[2];
    std::vector<int32_t> dfv[2];
    auto launch = [&](int h) -> int {  // generate + launch half h's next round; 0 tests = done
        const auto t0 = Clock::now();
        if (!search.Generate(h)) return FBN_OK;
        const int64_t nt = search.tests(h);
        indep[h].resize(nt);
        dfv[h].resize(nt);
        if (int rc = CiBatchLaunch(ctx, h, search.items(h).data(), nt, d, alpha, true, &search.stats(h))) return rc;
        out.launched += nt;
        if (timing)
            fprintf(stderr, "   half %d d=%d: %lld tests, generate + launch %.2f ms\n", h, d, (long long)nt,
                    Ms(t0, Clock::now()));
        return FBN_OK;
    };
    const int nh = search.halves();
    for (int h = 0; h < nh; ++h)
        if (int rc = launch(h)) return rc;
    if (deferred) deferred();  // (while the first batches run)
    while (true) {
        bool any = false;
        for (int h = 0; h < nh; ++h) {
            if (search.tests(h) == 0) continue;
            any = true;
            if (int rc = CiBatchWait(ctx, h, indep[h].data(), dfv[h].data(), res)) return rc;
            search.Resolve(h, indep[h].data(), dfv[h].data());
            if (int rc = launch(h)) return rc;
        }
        if (!any) break;
    }
    search.Finish(out);
    return FBN_OK;
}

namespace {

// what the steps of one RunPCStable call share
struct PCRun {
    fbn_ci_ctx *ctx;
    double alpha;
    int depth, group_size, n;
    int64_t P;              // pairs of the complete graph
    bool pairs, timing;     // level 0 records pair tables; FBN_PC_TIMING (host phase times per level)
    CiBatchStats st_all;    // of the complete graph's pairs
    Skeleton &sk;
    PendingSepsets &pend;
    PCResultHost &res;
};
// a Start* step fills the skeleton / the result and sets the depth the level loop starts at, or:
constexpr int kFinished = -1;  // the search ended in the step
constexpr int kNotTaken = -2;  // the step left everything untouched: another one runs

// Small graph: the whole search (or its first levels) in one device launch; refused at launch or
// timed out at a grid barrier: the host-driven levels (same answer)
int StartSmall(PCRun &R, int *d0) {
    const auto ta = Clock::now();
    int levels = 0;
    bool handoff = false, fellback = false;
    if (int rc = CiPCSmall(R.ctx, R.alpha, R.depth, R.res, R.sk, &levels, &handoff, &fellback)) return rc;
    R.res.path = fellback ? 2 : 1;
    *d0 = fellback ? kNotTaken : handoff ? levels : kFinished;
    if (fellback) return FBN_OK;
    if (R.timing)
        fprintf(stderr, "pc device-resident levels 0-%d: %.3f ms%s\n", levels - 1, Ms(ta, Clock::now()),
                handoff ? " (host continues)" : "");
    if (handoff) CiSetPairMode(R.ctx, 0);  // the ctx recorded no pair tables: the host levels count in full
    return FBN_OK;
}

// Level 0 -> level 1 without a host round trip: one complete-graph batch, whose kept pairs become the
// level-1 edge list / adjacency on the device; the host reads back only (E, the level's candidate
// sets) and builds its own copies (flags, edges, adjacency) while the first level-1 round runs
// (FBN_PC_HOST_L0L1: the host path)
int StartL0L1Device(PCRun &R, int *d0) {
    const auto ta = Clock::now();
    PCResultHost &res = R.res;
    int rc;
    if ((rc = CiBatchLaunchAllPairs(R.ctx, R.alpha, &R.st_all, 0, R.P, false))) return rc;
    int E = 0;
    int64_t cands = 0;
    if ((rc = CiL0L1Device(R.ctx, R.P, &E, &cands, res))) return rc;
    res.tests_per_level.push_back(R.P);
    res.launched_per_level.push_back(R.P);
    if (res.path == 0) res.path = 3;  // (2 -- a refused device-resident search -- stays)
    CiSetPairMode(R.ctx, 2);
    bool host_done = false;
    auto host_side = [&]() -> int {
        std::vector<char> removed;
        if (int r = CiL0L1Host(R.ctx, R.P, E, removed, R.sk)) return r;
        res.sepset.set_level0(R.n, std::move(removed));
        host_done = true;
        return FBN_OK;
    };
    const auto tb = Clock::now();
    *d0 = 1;
    if (!(E > 0 && CiPairsReady(R.ctx) && cands > FullSpeculation())) return host_side();  // level 1 (if any): host path
    LevelOut out;
    const double k1 = res.kernel_s;
    if ((rc = CiLevel1Run(R.ctx, R.alpha, E, cands, out, res, host_side))) return rc;
    if (!host_done && (rc = host_side())) return rc;
    const auto tr = Clock::now();
    res.tests_per_level.push_back(out.counted);
    res.launched_per_level.push_back(out.launched);
    // the level-1 sepsets are recorded while level 2 runs (only the orientation reads them): the
    // level-1 edge list moves aside, the kept edges (few) become the skeleton
    PendingSepsets &pend = R.pend;
    pend.keys.swap(R.sk.edges);
    R.sk.edges.clear();
    for (size_t i = 0; i < pend.keys.size(); ++i)
        if (!out.removed[i]) R.sk.edges.push_back(pend.keys[i]);
    R.sk.RebuildAdj(false);
    pend.rm.swap(out.removed);
    pend.sep.swap(out.sep);
    pend.d = 1;
    pend.armed = true;
    if (R.timing) {
        fprintf(stderr, "  level 1 removals %.3f ms\n", Ms(tr, Clock::now()));
        fprintf(stderr, "pc levels 0-1 on the device: level 0 %.2f ms, level 1 %.2f ms (kernels %.2f)\n", Ms(ta, tb),
                Ms(tb, Clock::now()), (res.kernel_s - k1) * 1e3);
    }
    *d0 = R.sk.ContinueAfter(1) ? 2 : std::max(R.depth, 1);
    return FBN_OK;
}

// Level 0 over the implicit complete graph (the kernels decode pair indices): no edge list or
// adjacency of the complete graph is built; the kept pairs become the skeleton directly
int StartL0Chunked(PCRun &R, int *d0) {
    const auto ta = Clock::now();
    PCResultHost &res = R.res;
    const double k0 = res.kernel_s;
    const int n = R.n;
    std::vector<char> removed((size_t)R.P);
    static_assert(sizeof(char) == sizeof(uint8_t), "flag layout");
    // small graphs: a host pass over the flags costs less than the device compaction's round trip
    const bool on_device = R.P > (1 << 16);
    double ms[2] = {0, 0};
    if (int rc = RunImplicitLevel0(R.ctx, R.alpha, R.st_all, 0, R.P, reinterpret_cast<uint8_t *>(removed.data()),
                                   on_device ? &R.sk.edges : nullptr, res, ms))
        return rc;
    const auto tb = Clock::now();
    if (R.timing) fprintf(stderr, "pc level 0: launch + wait %.3f ms, kept pairs %.3f ms\n", ms[0], ms[1]);
    res.tests_per_level.push_back(R.P);
    res.launched_per_level.push_back(R.P);
    if (!on_device) {
        int64_t k = 0;
        for (int i = 0; i < n; ++i)
            for (int j = i + 1; j < n; ++j, ++k)
                if (!removed[k]) R.sk.edges.push_back({i, j});
    }
    res.sepset.set_level0(n, std::move(removed));
    R.sk.RebuildAdj(true);
    if (R.pairs) CiSetPairMode(R.ctx, 2);
    if (R.timing)
        fprintf(stderr, "pc level 0 (implicit): run %.2f ms (kernels %.2f), skeleton %.2f ms\n", Ms(ta, tb),
                (res.kernel_s - k0) * 1e3, Ms(tb, Clock::now()));
    *d0 = 1;
    return FBN_OK;
}

// Not eligible for the implicit level 0: the complete graph explicitly, level 0 in the level loop
int StartComplete(PCRun &R, int *d0) {
    R.sk.SetComplete(R.n);
    *d0 = 0;
    return FBN_OK;
}

int RunLevels(PCRun &R, int d0) {
    PCResultHost &res = R.res;
    Skeleton &sk = R.sk;
    const std::function<void()> deferred = [&R]() { R.pend.Flush(R.res.sepset); };
    for (int d = d0; d < std::max(R.depth, 1); ++d) {
        LevelOut out;
        const auto ta = Clock::now();
        const double k0 = res.kernel_s;
        if (int rc = RunLevel(R.ctx, R.alpha, d, R.group_size, sk, 0, sk.edges.size(), out, res, deferred)) return rc;
        R.pend.Flush(res.sepset);
        const auto tb = Clock::now();
        // (recording a level's sepsets on a worker thread while the next level runs measured slower:
        // config 5 4.3 -> 4.5 ms of driver time, the orientation then reads a map built on another core)
        if (d == 0) res.sepset.set_level0(R.n, out.removed.data());  // edges = the complete graph
        else res.sepset.append_level(sk.edges.data(), out.removed.data(), out.sep.data(), sk.edges.size(), d);
        res.tests_per_level.push_back(out.counted);
        res.launched_per_level.push_back(out.launched);
        sk.ApplyRemovals(out.removed);
        const auto tc = Clock::now();
        if (d == 0 && R.pairs) CiSetPairMode(R.ctx, 2);
        if (R.timing)
            fprintf(stderr, "pc level %d: run %.2f ms (kernels %.2f), sepsets + removals %.2f ms, %.2f ms\n", d,
                    Ms(ta, tb), (res.kernel_s - k0) * 1e3, Ms(tb, tc), Ms(tc, Clock::now()));
        if (d >= 1 && !sk.ContinueAfter(d)) break;
    }
    return FBN_OK;
}

}  // namespace

int RunPCStable(fbn_ci_ctx *ctx, double alpha, int depth, int group_size, PCResultHost &res) {
    if (group_size < 1 || group_size > 8) return SetError(FBN_ERR_ARG, "group_size must be 1..8 (reference cap, src/IndependenceTest.cpp:170)");
    const auto t0 = Clock::now();
    res = PCResultHost();
    int n = 0;
    int64_t nsamples = 0;
    CiCtxShape(ctx, &n, &nsamples);
    // the skeleton and the pending record keep their capacity from the previous run on this thread
    static thread_local Skeleton sk_tls;
    static thread_local PendingSepsets pend_tls;
    sk_tls.Reset(n);
    pend_tls.armed = false;
    // level 0 tests every pair: its tables are recorded for the level-1 kernel (derived counting)
    // and dropped when this run ends, however it ends
    struct PairModeGuard {
        fbn_ci_ctx *c;
        ~PairModeGuard() { CiSetPairMode(c, 0); }
    } pair_guard{ctx};
    const bool pairs = !KnobSet("FBN_CI_NO_PAIRS");
    CiSetPairMode(ctx, pairs ? 1 : 0);
    PCRun R{ctx, alpha, depth, group_size, n, (int64_t)n * (n - 1) / 2, pairs, PcTiming(),
            CiAllPairsStats(CiCtxDims(ctx), n), sk_tls, pend_tls, res};
    int d0 = kNotTaken, rc = FBN_OK;
    if (CiPCSmallEligible(ctx, group_size)) rc = StartSmall(R, &d0);
    if (!rc && d0 == kNotTaken) {
        if (n < 2 || !CiAllPairsEligible(ctx, R.st_all)) rc = StartComplete(R, &d0);
        else if (pairs && R.P <= L0Chunk() && depth > 1 && CiL0L1DeviceEligible(ctx, group_size)) rc = StartL0L1Device(R, &d0);
        else rc = StartL0Chunked(R, &d0);
    }
    if (!rc && d0 != kFinished) rc = RunLevels(R, d0);
    if (rc) return rc;
    R.pend.Flush(res.sepset);
    res.edges = R.sk.edges;
    res.total_s = std::chrono::duration<double>(Clock::now() - t0).count();
    return FBN_OK;
}

}  // namespace fbn
