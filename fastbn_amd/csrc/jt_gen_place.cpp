// jt_gen_place.cpp -- message placement of the plan-specialized JT kernel.
//
// Every stored message has a live interval on the schedule's clock (Collect clique k of the
// post-order at time k, Distribute clique k of the pre-order at time nc + k): the Collect message
// of separator s from its child's Collect to its parent's Distribute, the Distribute message from
// the parent's Distribute to the child's.  The per-wave workspace of all of them (ALARM: 265 rows =
// 136 KB per wave, 139 MB for 1,024 waves) does not stay in L2, and each row written twice per
// block left L2 twice (PMC, round 5: 0.49 GB written per 100k cases, the kernel 20 % slower than
// with the workspace L2-resident).  So the LDS left over by the clique tail (the budget of four
// waves per CU) holds a pool of rows, and messages get pool rows by interval: shortest intervals
// first while the pool has room at every time of the interval, rows then assigned in start order
// (an interval graph: the room suffices).  The rest keep global rows (Collect and Distribute
// message of a separator in the same rows).  FBN_JT_LDS_POOL=n caps the pool at n rows (0: off).
// Before the LDS pool, the fast order parks message entries in registers the small cliques leave
// unused (opt.reg_cap rows at most, 0: off); a message may be split: its leading entries in
// registers, the others in one of the two memories.
// JtGenPlace is a function of its arguments: the search over child orders keeps the value it likes.
#include <algorithm>
#include <cstdio>

#include "jt_gen.h"

namespace fbn {

namespace {

std::vector<JtGenMessage> StoredMessages(const JTPlanHost &plan, const JtGenSchedule &sch) {
    const int nc = (int)plan.cliques.size(), ns = (int)plan.seps.size();
    std::vector<JtGenMessage> items;
    auto add = [&](int s, bool dist, int a, int b) {
        JtGenMessage m;
        m.sep = s, m.dist = dist, m.a = a, m.b = b, m.n = plan.seps[s].size();
        items.push_back(m);
    };
    for (int s = 0; s < ns; ++s) {
        const int c = plan.sep_down[s], p = plan.sep_up[s];
        if (!sch.leaf_rc[s]) add(s, false, sch.qi[c], nc + sch.pi[p]);
        else if (sch.col_store[s]) add(s, false, sch.qi[c], sch.qi[p]);
        if (!sch.md_reg[s]) add(s, true, nc + sch.pi[p], nc + sch.pi[c]);
    }
    return items;
}

// Register pool (fast order, FBN_JT_REG_POOL): the leading nreg entries of a message stay in
// named registers for its whole interval.  An op needs its table (the register-resident part)
// and the messages it loads, prefetches or keeps (JtGenOp::need); what is left of the 256 fp64
// values per lane, less a slack for temporaries, may hold parked rows at that time.  A message is
// checked at its producer (which would otherwise store each entry as it is formed) and at every
// op before its consumer; an op that loads it on the way anyway (JtGenOp::touch: the parent's
// Collect of a message parked until the parent's Distribute, a prefetch) pays nothing extra for it.
void ParkInRegisters(const JtGenSchedule &sch, const JtGenOptions &opt, const std::vector<int> &order, JtGenPlacement &pl) {
    for (int i : order) {
        JtGenMessage &it = pl.msgs[i];
        const int id = 2 * it.sep + (it.dist ? 1 : 0);
        int64_t room = it.n;
        for (int t = it.a; t <= it.b; ++t) room = std::min(room, opt.reg_cap - pl.live[t]);
        std::vector<int> pay;  // the times this message costs registers of its own
        for (int t = it.a; t < it.b; ++t) {
            const std::vector<int> &touch = sch.ops[t].touch;
            if (t == it.a || std::find(touch.begin(), touch.end(), id) == touch.end()) pay.push_back(t);
        }
        for (int t : pay) room = std::min(room, kJtRegFile - opt.slack() - sch.ops[t].need - pl.reg_extra[t]);
        if (room <= 0) continue;
        it.nreg = room;
        for (int t = it.a; t <= it.b; ++t) pl.live[t] += room;
        for (int t : pay) pl.reg_extra[t] += room;
    }
}

// LDS pool: which messages (their rows not in registers), then concrete rows in start order
void AssignPoolRows(const std::vector<int> &order, JtGenPlacement &pl) {
    std::vector<JtGenMessage> &items = pl.msgs;
    for (int i : order) {
        JtGenMessage &it = items[i];
        const int64_t n = it.n - it.nreg;
        if (n == 0 || n > pl.pool_cap) continue;
        int64_t mx = 0;
        for (int t = it.a; t <= it.b; ++t) mx = std::max(mx, pl.use[t]);
        if (mx + n > pl.pool_cap) continue;
        for (int t = it.a; t <= it.b; ++t) pl.use[t] += n;
        it.in_lds = true;
    }
    std::vector<int> byst;
    for (size_t i = 0; i < items.size(); ++i)
        if (items[i].in_lds) byst.push_back((int)i);
    std::stable_sort(byst.begin(), byst.end(), [&](int x, int y) { return items[x].a < items[y].a; });
    std::vector<int64_t> free_rows;
    for (int64_t r = pl.pool_cap - 1; r >= 0; --r) free_rows.push_back(r);  // (pop_back takes the lowest)
    std::vector<int> active;
    for (int i : byst) {
        JtGenMessage &it = items[i];
        for (size_t k = 0; k < active.size();) {  // release intervals that ended before this one
            if (items[active[k]].b < it.a) {
                for (int64_t r : items[active[k]].rows) free_rows.push_back(r);
                std::sort(free_rows.rbegin(), free_rows.rend());
                active.erase(active.begin() + k);
            } else {
                ++k;
            }
        }
        for (int64_t j = it.nreg; j < it.n; ++j) {
            it.rows.push_back(free_rows.back());
            pl.pool_rows = std::max<int64_t>(pl.pool_rows, free_rows.back() + 1);
            free_rows.pop_back();
        }
        active.push_back(i);
    }
}

// global rows, the location strings and the counts
void NamePlaces(const JTPlanHost &plan, JtGenPlacement &pl) {
    const int ns = (int)plan.seps.size();
    pl.col_of.assign(ns, -1), pl.dis_of.assign(ns, -1);
    pl.sep_row.assign(ns, -1);
    // global rows of a separator: shared by both its messages, entry j in row sep_row + j - sep_skip
    // (sep_skip: leading entries neither message keeps there)
    std::vector<int64_t> sep_skip(ns, 0);
    for (int s = 0; s < ns; ++s) sep_skip[s] = plan.seps[s].size();
    for (const JtGenMessage &it : pl.msgs)
        if (!it.in_lds) sep_skip[it.sep] = std::min(sep_skip[it.sep], it.nreg);
    int64_t grow = 0;
    for (size_t i = 0; i < pl.msgs.size(); ++i) {
        JtGenMessage &it = pl.msgs[i];
        (it.dist ? pl.dis_of : pl.col_of)[it.sep] = (int)i;
        it.loc.assign(it.n, std::string());
        for (int64_t j = 0; j < it.nreg; ++j) {
            it.loc[j] = (it.dist ? "rd" : "rc") + std::to_string(it.sep) + "_" + std::to_string(j);
            pl.reg_names.push_back(it.loc[j]);
        }
        pl.counts.reg[it.dist] += it.nreg;
        if (it.in_lds) {
            for (int64_t j = it.nreg; j < it.n; ++j) it.loc[j] = "LP(" + std::to_string(it.rows[j - it.nreg]) + ")";
            pl.counts.lds[it.dist] += it.n - it.nreg;
            continue;
        }
        if (it.nreg == it.n) continue;
        if (pl.sep_row[it.sep] < 0) pl.sep_row[it.sep] = grow, grow += it.n - sep_skip[it.sep];  // (shared by both messages)
        for (int64_t j = it.nreg; j < it.n; ++j) {
            it.rows.push_back(pl.sep_row[it.sep] + j - sep_skip[it.sep]);
            it.loc[j] = "W(" + std::to_string(it.rows.back()) + "LL)";
        }
        pl.counts.global[it.dist] += it.n - it.nreg;
    }
    pl.counts.workspace_rows = grow;
    pl.counts.lds_pool_rows = pl.pool_rows;
    for (int s = 0; s < ns; ++s)
        if (pl.sep_row[s] < 0) pl.sep_row[s] = 0;
}

}  // namespace

JtGenPlacement JtGenPlace(const JTPlanHost &plan, const JtGenSchedule &sch, const JtGenOptions &opt, int64_t lds_rows) {
    const int nc = (int)plan.cliques.size();
    JtGenPlacement pl;
    pl.msgs = StoredMessages(plan, sch);
    std::vector<int> order(pl.msgs.size());  // shortest interval first
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
        return pl.msgs[x].b - pl.msgs[x].a < pl.msgs[y].b - pl.msgs[y].a;
    });
    pl.reg_extra.assign(2 * nc + 1, 0);
    pl.live.assign(2 * nc + 1, 0);
    pl.use.assign(2 * nc + 1, 0);
    if (opt.reg_cap > 0) ParkInRegisters(sch, opt, order, pl);
    // room: the LDS of four waves per CU (160 KB) less the clique tail
    const int64_t per_wave = 160 * 1024 / 4 / 8;  // fp64 values
    pl.pool_cap = std::max<int64_t>(0, (per_wave - lds_rows * 64) / 64);
    if (opt.lds_pool >= 0) pl.pool_cap = std::min(pl.pool_cap, opt.lds_pool);
    AssignPoolRows(order, pl);
    NamePlaces(plan, pl);
    return pl;
}

int64_t JtGenWaveEntries(const JTPlanHost &plan, const JtGenPlacement &pl) {
    int64_t rows = 1;
    for (size_t s = 0; s < plan.seps.size(); ++s) rows = std::max<int64_t>(rows, pl.sep_row[s] + plan.seps[s].size());
    return rows;
}

// With the register pool on, the child order of each phase is chosen by the placement itself:
// the plan's, heaviest subtree (sum of clique entries) first, or heaviest last -- whichever
// leaves the fewest message rows in global memory (a tie keeps the earlier candidate, the
// plan's order first).
int JtGenPlan(const JTPlanHost &plan, const JtGenOptions &opt, JtGenTables &tab, JtGenSchedule &sch, JtGenPlacement &pl) {
    const size_t nc = plan.cliques.size();
    const std::vector<int> post = JtGenOrder(plan, true, 0);
    if (post.size() != nc) return SetError(FBN_ERR_LIMIT, "codegen: tree traversal covers %zu of %d cliques", post.size(), (int)nc);
    tab = JtGenBuildTables(plan, opt.fast);
    sch = JtGenBuildSchedule(plan, opt, post, JtGenOrder(plan, false, 0));
    pl = JtGenPlace(plan, sch, opt, tab.lds_rows);
    const int64_t plan_peak = sch.peak_need;
    int best = 0;
    for (int v = 1; v < 9 && opt.reg_cap > 0; ++v) {
        JtGenSchedule s = JtGenBuildSchedule(plan, opt, JtGenOrder(plan, true, v / 3), JtGenOrder(plan, false, v % 3));
        // (an order whose ops themselves need more registers than the plan order's at their
        // peak is left out: the plan order's peak already fills the register file)
        if (s.peak_need > plan_peak) continue;
        JtGenPlacement p = JtGenPlace(plan, s, opt, tab.lds_rows);
        if (p.counts.global[0] + p.counts.global[1] < pl.counts.global[0] + pl.counts.global[1])
            sch = std::move(s), pl = std::move(p), best = v;
    }
    if (opt.place_debug) {
        if (opt.reg_cap > 0)
            fprintf(stderr, "child order (0 plan, 1 heaviest subtree first, 2 last): Collect %d, Distribute %d\n", best / 3, best % 3);
        JtGenDescribe(plan, sch, pl, opt, tab);
    }
    return FBN_OK;
}

// FBN_JT_PLACE_DEBUG: the chosen placement's summary on stderr
void JtGenDescribe(const JTPlanHost &plan, const JtGenSchedule &sch, const JtGenPlacement &pl, const JtGenOptions &opt,
                   const JtGenTables &tab) {
    const int nc = (int)plan.cliques.size(), ns = (int)plan.seps.size();
    const JTPlacement &n = pl.counts;
    if (opt.reg_cap > 0) {
        std::string u;
        for (int t = 0; t < 2 * nc; ++t)
            u += std::to_string(sch.ops[t].need) + "+" + std::to_string(pl.reg_extra[t]) + (t == nc - 1 ? " | " : " ");
        fprintf(stderr, "register rows by time, the op's own + parked (Collect | Distribute): %s\n", u.c_str());
    }
    int64_t leaf = 0;
    for (int s = 0; s < ns; ++s)
        if (plan.clique_down[plan.sep_down[s]].empty()) leaf += plan.seps[s].size();
    fprintf(stderr, "placement: pool %lld of %lld rows; Collect rows LDS %lld global %lld; Distribute rows LDS %lld "
                    "global %lld (registers: the rest); global rows %lld; leaf-separator rows %lld\n",
            (long long)pl.pool_rows, (long long)pl.pool_cap, (long long)n.lds[0], (long long)n.global[0],
            (long long)n.lds[1], (long long)n.global[1], (long long)n.workspace_rows, (long long)leaf);
    if (opt.reg_cap > 0)
        fprintf(stderr, "register pool (cap %lld rows): Collect rows %lld, Distribute rows %lld\n", (long long)opt.reg_cap,
                (long long)n.reg[0], (long long)n.reg[1]);
    std::string u;
    for (int t = 0; t <= 2 * nc; ++t) u += std::to_string(pl.use[t]) + (t == nc - 1 ? " | " : " ");
    fprintf(stderr, "pool rows in use by time (Collect | Distribute): %s\n", u.c_str());
    if (opt.fast) {
        std::string m;
        for (int v = 0; v < (int)plan.dom.size(); ++v) {
            const int t = tab.msep[v] >= 0 ? nc + sch.pi[plan.sep_up[tab.msep[v]]] : nc + sch.pi[tab.mclq[v]];
            m += std::to_string(v) + ":" + std::to_string(t) + " ";
        }
        fprintf(stderr, "marginal time per variable: %s\n", m.c_str());
    }
}

}  // namespace fbn
