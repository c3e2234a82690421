// jt_mpe_plan.cpp -- compiles the junction-forest plan (BuildJTPlan, forest = true) into the
// max-product program of jt_mpe_program.h: per clique its initial potentials, packed evidence digits
// (CompileJTProgram's packing) and one int32 map per adjacent separator; the row offsets of the
// message store; the Collect and back-trace orders.  Case-independent; host only.
#include <algorithm>
#include <climits>

#include "fbn_internal.h"
#include "jt_mpe_program.h"

namespace fbn {

int CompileJTProgramMpe(const JTPlanHost &plan, JTProgramMpe &prog) {
    prog = JTProgramMpe();
    if (int rc = CheckPlanPotentials(plan)) return rc;
    const int nc = (int)plan.cliques.size(), ns = (int)plan.seps.size();
    prog.V = plan.num_nodes;
    prog.nsep = ns;
    prog.components = plan.num_components;
    prog.dom.assign(plan.dom.begin(), plan.dom.end());
    std::vector<int64_t> soff(ns);
    int64_t off = 0;
    for (int s = 0; s < ns; ++s) soff[s] = off, off += plan.seps[s].size();
    prog.msg_rows = off;
    prog.store_rows = off + ns + nc;
    for (int c = 0; c < nc; ++c) prog.entries += plan.cliques[c].size();
    if (prog.store_rows > INT32_MAX / 2 || prog.entries > INT32_MAX / 2)
        return SetError(FBN_ERR_LIMIT, "junction forest too large (%lld clique entries, %lld store rows)",
                        (long long)prog.entries, (long long)prog.store_rows);

    auto loc_of = [](const Table &t, int v) {
        for (size_t i = 0; i < t.vars.size(); ++i)
            if (t.vars[i] == v) return (int)i;
        return -1;
    };
    // a clique entry -> the index of a separator over a subset of its variables
    auto sub_index = [&](const Table &t, const Table &sub, int64_t e) {
        int64_t r = e, idx = 0;
        for (size_t j = 0; j < t.vars.size(); ++j) {
            const int64_t digit = r / t.cum[j];
            r %= t.cum[j];
            const int l = loc_of(sub, t.vars[j]);
            if (l >= 0) idx += digit * sub.cum[l];
        }
        return idx;
    };

    std::vector<int32_t> sepmap_off(ns, -1);  // the parent's map onto separator s
    prog.cl.assign(nc, JtMClique());
    for (int c = 0; c < nc; ++c) {
        const Table &t = plan.cliques[c];
        JtMClique &q = prog.cl[c];
        const int nv = (int)t.vars.size();
        if (nv > 8 * JT_MAX_DIG_WORDS)
            return SetError(FBN_ERR_LIMIT, "clique with %d variables (max %d)", nv, 8 * JT_MAX_DIG_WORDS);
        q.T = (int32_t)t.size(), q.nv = nv, q.k = (int32_t)plan.clique_down[c].size();
        q.nw = std::max(1, (nv + 7) / 8);
        q.vars_off = (int32_t)prog.aux.size();
        for (int v : t.vars) prog.aux.push_back(v);
        q.dig_off = (int32_t)prog.dig.size();
        for (int64_t e = 0; e < t.size(); ++e) {
            uint64_t w[JT_MAX_DIG_WORDS] = {0, 0, 0, 0};
            int64_t r = e;
            for (int j = 0; j < nv; ++j) {
                const uint64_t digit = (uint64_t)(r / t.cum[j]);
                r %= t.cum[j];
                w[j / 8] |= digit << (8 * (j % 8));
            }
            for (int k = 0; k < q.nw; ++k) prog.dig.push_back(w[k]);
        }
        q.iv_off = (int32_t)prog.initv.size();
        prog.initv.insert(prog.initv.end(), t.pot.begin(), t.pot.end());
        q.estar_row = (int32_t)(prog.msg_rows + ns + c);

        std::vector<int32_t> rec;
        for (int s : plan.clique_down[c]) {
            sepmap_off[s] = (int32_t)prog.aux.size();
            for (int64_t e = 0; e < t.size(); ++e) prog.aux.push_back((int32_t)sub_index(t, plan.seps[s], e));
            rec.insert(rec.end(), {sepmap_off[s], (int32_t)soff[s], (int32_t)(prog.msg_rows + s), plan.sep_down[s]});
        }
        q.child_off = (int32_t)prog.aux.size();
        prog.aux.insert(prog.aux.end(), rec.begin(), rec.end());

        const int s = plan.clique_up[c];
        q.parent = -1, q.nown = nv;
        if (s >= 0) {
            const int64_t Ts = plan.seps[s].size();
            q.up_Ts = (int32_t)Ts, q.up_row = (int32_t)soff[s], q.up_exp_row = (int32_t)(prog.msg_rows + s);
            q.parent = plan.sep_up[s];
            q.nown = nv - (int)plan.seps[s].vars.size();
            q.up_map_off = (int32_t)prog.aux.size();
            for (int64_t e = 0; e < t.size(); ++e) {
                const int64_t u = sub_index(t, plan.seps[s], e);
                // ReorganizeTableStorage put the separator's variables last, in the separator's order
                if (u != e % Ts) return SetError(FBN_ERR_ARG, "internal: clique %d is not reorganised for its separator", c);
                prog.aux.push_back((int32_t)u);
            }
        }
        if (prog.aux.size() > (size_t)INT32_MAX / 2) return SetError(FBN_ERR_LIMIT, "max-product program too large");
    }
    for (int c = 0; c < nc; ++c) {
        const int s = plan.clique_up[c];
        if (s < 0) continue;
        if (sepmap_off[s] < 0 || prog.cl[c].parent < 0) return SetError(FBN_ERR_ARG, "internal: separator %d has no parent", s);
        prog.cl[c].parent_map_off = sepmap_off[s];
    }
    const int L = (int)plan.levels.size();
    for (int i = L - 1; i >= 0; --i)
        if (i % 2 == 0)
            for (int c : plan.levels[i]) prog.collect.push_back(c);
    for (int i = 0; i < L; i += 2)
        for (int c : plan.levels[i]) prog.trace.push_back(c);
    if ((int)prog.collect.size() != nc) return SetError(FBN_ERR_ARG, "internal: %d of %d cliques levelled", (int)prog.collect.size(), nc);
    std::vector<char> covered(plan.num_nodes, 0);
    for (const Table &t : plan.cliques)
        for (int v : t.vars) covered[v] = 1;
    for (int v = 0; v < plan.num_nodes; ++v)
        if (!covered[v]) return SetError(FBN_ERR_ARG, "variable %d appears in no clique", v);
    return FBN_OK;
}

}  // namespace fbn
