// jt_gen_schedule.cpp -- traversal orders and the op schedule of the plan-specialized JT kernel.
//
// Schedule (values identical to the reference's level order -- a clique's Collect result depends
// only on its subtree and the fixed order of its child messages, its Distribute result only on its
// parent's -- so any children-first / parent-first traversal gives the same bits):
//  * Collect in DFS post-order: the last child's message stays in registers for its parent; other
//    messages are stored (they are needed again anyway as the "old" separator of Distribute).
//  * Distribute in DFS pre-order: a clique's Collect table is not parked and reloaded but
//    recomputed from its initial potential and its children's stored messages (which Distribute
//    loads anyway) -- ALU is cheap here, HBM round trips are not.  The message to the first child
//    stays in registers; the others are stored.
//  * Loads for the next clique are issued at the start of the current one (register budget
//    permitting) so their latency hides behind its arithmetic.
// Register policy of Distribute (opt.budget fp64 values per lane):
//  * the message to a first child stays in registers if that child's table, the message and
//    its largest child message fit; otherwise it is stored and loaded ("ld") right before DMul
//  * a clique's children's Collect messages ("lb") are loaded at its start (or prefetched by
//    the previous clique) if they fit next to its table; otherwise each is loaded right before
//    its Mul and loaded again ("lc") right before its SepDis
// JtGenBuildSchedule states these rules once; the placement charges registers by the ops' need and
// touch, the emitter walks the ops.  Three places where the two read an op differently are kept as
// they were measured; each is marked "kept asymmetry" where it is decided.
#include <algorithm>
#include <functional>

#include "jt_gen.h"

namespace fbn {

// Collect in post-order, Distribute in pre-order of a DFS.  Any child order gives the same values
// (schedule freedom, section 4 of DESIGN.md); products and sums keep the plan's child order
// whatever is visited first.
std::vector<int> JtGenOrder(const JTPlanHost &plan, bool collect, int visit) {
    const int nc = (int)plan.cliques.size();
    std::vector<int64_t> weight(nc, 0);  // entries of a clique's subtree
    std::function<int64_t(int)> w = [&](int c) {
        weight[c] = plan.cliques[c].size();
        for (int s : plan.clique_down[c]) weight[c] += w(plan.sep_down[s]);
        return weight[c];
    };
    for (int r : plan.roots) w(r);
    std::vector<std::vector<int>> kids(nc);
    for (int c = 0; c < nc; ++c) {
        kids[c] = plan.clique_down[c];
        if (visit)
            std::stable_sort(kids[c].begin(), kids[c].end(), [&](int x, int y) {
                const int64_t wx = weight[plan.sep_down[x]], wy = weight[plan.sep_down[y]];
                return visit == 1 ? wx > wy : wx < wy;
            });
    }
    // a forest: tree after tree -- Collect in component order, Distribute in the reverse, so the
    // root collected last is the one distributed first (it continues from its Collect registers)
    std::vector<int> roots = plan.roots, order;
    if (!collect) std::reverse(roots.begin(), roots.end());
    std::vector<std::pair<int, size_t>> st;
    size_t next_root = 0;
    while (!st.empty() || next_root < roots.size()) {  // iterative DFS
        if (st.empty()) st.push_back({roots[next_root++], 0});
        auto &top = st.back();
        const int c = top.first;
        if (top.second == 0 && !collect) order.push_back(c);
        if (top.second < kids[c].size()) {
            st.push_back({plan.sep_down[kids[c][top.second++]], 0});
        } else {
            if (collect) order.push_back(c);
            st.pop_back();
        }
    }
    return order;
}

namespace {

struct Rules {  // the register rules, each stated once
    const JTPlanHost &plan;
    const JtGenSchedule &sch;
    const int64_t budget;
    int64_t tsize(int c) const { return plan.cliques[c].size(); }
    int64_t ssize(int s) const { return plan.seps[s].size(); }
    int64_t rows_of(const std::vector<int> &ls) const {
        int64_t r = 0;
        for (int s : ls) r += ssize(s);
        return r;
    }
    int64_t kids_rows(int c) const { return rows_of(plan.clique_down[c]); }
    // loads of clique post[k]: its children's messages except a last child that is post[k - 1]
    // (the child just collected: registers)
    std::vector<int> collect_loads(int k) const {
        std::vector<int> ls;
        for (int s : plan.clique_down[sch.post[k]])
            if (!(k > 0 && plan.sep_down[s] == sch.post[k - 1])) ls.push_back(s);
        return ls;
    }
    bool early_lb(int c) const {
        const int up = plan.clique_up[c];
        const int64_t held = (up >= 0) ? ssize(up) : 0;  // in registers at DMul either way
        return tsize(c) + kids_rows(c) + held <= budget;
    }
    // the Distribute message to the child visited first (the next clique of the pre-order)
    bool md_reg_rule(int q) const {
        int64_t mk = 0;
        for (int s2 : plan.clique_down[q]) mk = std::max<int64_t>(mk, ssize(s2));
        return tsize(q) + ssize(plan.clique_up[q]) + mk <= budget;
    }
    // the next Distribute op's parent message, unless still in registers or produced by clique c
    // (or it has none: the next tree's root)
    int ld_next(int c, int nx) const {
        const int nup = plan.clique_up[nx];
        return nup >= 0 && !sch.md_reg[nup] && plan.sep_up[nup] != c ? nup : -1;
    }
};

// An op's prefetch fits when prefetch_cost <= budget.  Kept asymmetry 1: this test, which sets the
// need and touch the placement reads, leaves out the parked rows; the emitter adds reg_extra[t].
void ClosePrefetch(JtGenOp &op, int64_t budget) {
    if (op.prefetch_cost > budget) return;
    op.need += op.prefetch_rows;
    for (int s : op.prefetch) op.touch.push_back(2 * s);
    if (op.prefetch_ld >= 0) op.touch.push_back(2 * op.prefetch_ld + 1);
}

JtGenOp CollectOp(const Rules &R, int k) {
    const JTPlanHost &plan = R.plan;
    const int nc = (int)plan.cliques.size(), c = R.sch.post[k];
    JtGenOp op;
    op.clique = c;
    // The root collected last stays in registers for its Distribute.  Every other root of a forest
    // sends no message, so its Collect is left out; its Distribute recomputes the table like any
    // clique's, from the initial potential and the children's stored messages.
    // Kept asymmetry 2: need, touch and the candidates below are charged for such a root as well.
    op.runs = plan.clique_up[c] >= 0 || c == R.sch.cont_root;
    op.loads = R.collect_loads(k);
    op.need = std::min<int64_t>(R.tsize(c), kJtRegEntries) + R.kids_rows(c);
    for (int s : plan.clique_down[c]) op.touch.push_back(2 * s);
    if (k + 1 < nc) {
        op.prefetch = R.collect_loads(k + 1);
        op.prefetch_rows = R.rows_of(op.prefetch);
        op.prefetch_cost = R.tsize(c) + R.rows_of(op.loads) + op.prefetch_rows;
        ClosePrefetch(op, R.budget);
    }
    return op;
}

JtGenOp DistributeOp(const Rules &R, int k) {
    const JTPlanHost &plan = R.plan;
    const int nc = (int)plan.cliques.size(), c = R.sch.pre[k], up = plan.clique_up[c];
    JtGenOp op;
    op.clique = c;
    op.early = R.early_lb(c);
    if (op.early) op.loads = plan.clique_down[c];
    int64_t kmax = 0, pend = op.early ? R.kids_rows(c) : 0;
    for (int s : plan.clique_down[c]) {
        kmax = std::max<int64_t>(kmax, R.ssize(s));
        op.touch.push_back(2 * s);
        if (R.sch.md_reg[s]) op.need += R.ssize(s);
    }
    op.need += std::min<int64_t>(R.tsize(c), kJtRegEntries) + (op.early ? R.kids_rows(c) : kmax);
    if (up >= 0) {
        op.need += R.ssize(up);
        op.touch.push_back(2 * up + 1);
        if (R.sch.md_reg[up]) pend += R.ssize(up);
    }
    if (k + 1 < nc) {  // (before this clique's stores)
        const int nx = R.sch.pre[k + 1];
        // Kept asymmetry 3: a leaf-recomputed message among the candidates is charged here; the
        // emitter does not load it (it has no place to load from).
        if (R.early_lb(nx)) op.prefetch = plan.clique_down[nx];
        op.prefetch_ld = R.ld_next(c, nx);
        op.prefetch_rows = R.rows_of(op.prefetch) + (op.prefetch_ld >= 0 ? R.ssize(op.prefetch_ld) : 0);
        op.prefetch_cost = R.tsize(c) + pend + op.prefetch_rows;
        ClosePrefetch(op, R.budget);
    }
    return op;
}

}  // namespace

JtGenSchedule JtGenBuildSchedule(const JTPlanHost &plan, const JtGenOptions &opt, std::vector<int> post, std::vector<int> pre) {
    const int nc = (int)plan.cliques.size(), ns = (int)plan.seps.size();
    JtGenSchedule sch;
    sch.post = std::move(post), sch.pre = std::move(pre);
    sch.cont_root = sch.post.back() == sch.pre.front() ? sch.pre.front() : -1;
    sch.qi.assign(nc, 0), sch.pi.assign(nc, 0);
    for (int k = 0; k < nc; ++k) sch.qi[sch.post[k]] = k, sch.pi[sch.pre[k]] = k;
    const Rules R{plan, sch, opt.budget};
    sch.md_reg.assign(ns, false);
    for (int c : sch.pre)
        if (!plan.clique_down[c].empty()) {
            const int q = sch.pre[sch.pi[c] + 1];
            sch.md_reg[plan.clique_up[q]] = R.md_reg_rule(q);
        }
    sch.leaf_rc.assign(ns, false);
    sch.col_store.assign(ns, true);
    for (int s = 0; s < ns; ++s) {
        const int c = plan.sep_down[s], p = plan.sep_up[s];
        if (!opt.fast || !opt.leaf_rc || !plan.clique_down[c].empty() || R.tsize(c) > 64) continue;
        sch.leaf_rc[s] = true;
        // the parent's Collect takes the last child's message from registers when that child ran
        // just before it (collect_loads)
        sch.col_store[s] = !(sch.qi[p] > 0 && sch.post[sch.qi[p] - 1] == c);
    }
    for (int k = 0; k < nc; ++k) sch.ops.push_back(CollectOp(R, k));
    for (int k = 0; k < nc; ++k) sch.ops.push_back(DistributeOp(R, k));
    for (const JtGenOp &op : sch.ops) sch.peak_need = std::max(sch.peak_need, op.need);
    return sch;
}

}  // namespace fbn
