// jt_em_plan.cpp -- compiles the junction-forest plan into the expectation-maximisation program of
// jt_em_program.h: the max-product program's tables (CompileJTProgramMpe), the family each clique
// hosts (the first clique in plan order that contains it, recomputed here from the plan's variable
// sets), the entry -> family cell maps and the grouped entry lists of the register sums; and the host
// forms of the M-step and of the rebuild of the initial potentials.  Case-independent; host only.
#include <algorithm>
#include <climits>
#include <numeric>

#include "fbn_internal.h"
#include "jt_em_program.h"

namespace fbn {

namespace {
// the entries 0 .. T-1 sorted by (key[e], e)
std::vector<int32_t> GroupBy(const int32_t *key, int64_t T) {
    std::vector<int32_t> g((size_t)T);
    std::iota(g.begin(), g.end(), 0);
    std::stable_sort(g.begin(), g.end(), [&](int32_t a, int32_t b) { return key[a] < key[b]; });
    return g;
}
}  // namespace

int CompileJTProgramEm(const Network &net, const JTPlanHost &plan, JTProgramEm &prog) {
    prog = JTProgramEm();
    if (int rc = CompileJTProgramMpe(plan, prog.M)) return rc;
    const JTProgramMpe &M = prog.M;
    const int nc = (int)plan.cliques.size(), V = plan.num_nodes;

    // the cells, fbn_param_family_sizes' offsets
    std::vector<int64_t> foff(V + 1, 0);
    for (int v = 0; v < V; ++v) {
        int64_t cells = net.dom[v];
        for (int q : net.parents_asc[v]) {
            cells *= net.dom[q];
            if (cells > FBN_PARAM_MAX_CELLS) break;
        }
        foff[v + 1] = foff[v] + cells;
        if (cells > FBN_PARAM_MAX_CELLS || foff[v + 1] > FBN_PARAM_MAX_CELLS)
            return SetError(FBN_ERR_LIMIT, "em: tables beyond %lld cells (node %d)", (long long)FBN_PARAM_MAX_CELLS, v);
        prog.node_rec.insert(prog.node_rec.end(), {(int32_t)foff[v], (int32_t)(cells / net.dom[v]), (int32_t)net.dom[v]});
        for (int64_t i = 0; i < cells; ++i) prog.cell_node.push_back(v);
    }
    prog.cells = foff[V];
    prog.store_rows = std::max<int64_t>(2 * M.msg_rows + M.nsep, 1);
    if (prog.store_rows > INT32_MAX / 2)
        return SetError(FBN_ERR_LIMIT, "em: %lld store rows", (long long)prog.store_rows);

    // theta = the network's own CPTs
    prog.theta.assign((size_t)prog.cells, 0.0);
    for (int v = 0; v < V; ++v) {
        const std::vector<int> &pa = net.parents_asc[v];
        const int64_t npc = (foff[v + 1] - foff[v]) / net.dom[v];
        std::vector<int> pv(pa.size());
        for (int64_t pc = 0; pc < npc; ++pc) {
            int64_t r = pc;
            for (int j = (int)pa.size() - 1; j >= 0; --j) pv[j] = (int)(r % net.dom[pa[j]]), r /= net.dom[pa[j]];
            for (int q = 0; q < net.dom[v]; ++q) prog.theta[(size_t)(foff[v] + q * npc + pc)] = net.Prob(v, q, pv.data());
        }
    }

    // hosting: the first clique in plan order whose variables include the family (jt_plan.cpp's rule)
    std::vector<std::vector<int>> hosted(nc);
    for (int v = 0; v < V; ++v) {
        int host = -1;
        for (int c = 0; c < nc && host < 0; ++c) {
            const std::vector<int> &cv = plan.cliques[c].vars;
            bool all = std::find(cv.begin(), cv.end(), v) != cv.end();
            for (int q : net.parents_asc[v]) all = all && std::find(cv.begin(), cv.end(), q) != cv.end();
            if (all) host = c;
        }
        if (host < 0) return SetError(FBN_ERR_ARG, "internal: the family of node %d is in no clique", v);
        hosted[host].push_back(v);  // ascending node order
    }

    prog.ecl.assign(nc, JtEClique());
    prog.entry_clique.reserve((size_t)M.entries);
    for (int c = 0; c < nc; ++c) {
        const Table &t = plan.cliques[c];
        JtEClique &q = prog.ecl[c];
        const int64_t T = t.size();
        if ((int64_t)prog.entry_clique.size() != M.cl[c].iv_off)
            return SetError(FBN_ERR_ARG, "internal: clique %d's potentials are not at its entry offset", c);
        for (int64_t e = 0; e < T; ++e) prog.entry_clique.push_back(c);
        q.nfam = (int32_t)hosted[c].size();
        std::vector<int32_t> rec;
        for (int v : hosted[c]) {
            const std::vector<int> &pa = net.parents_asc[v];
            const int64_t npc = (foff[v + 1] - foff[v]) / net.dom[v];
            // the stride of each clique variable in the family's cell index
            std::vector<int64_t> stride(t.vars.size(), 0);
            int64_t st = 1;
            for (int j = (int)pa.size() - 1; j >= 0; --j) {
                const size_t l = std::find(t.vars.begin(), t.vars.end(), pa[j]) - t.vars.begin();
                stride[l] = st, st *= net.dom[pa[j]];
            }
            stride[std::find(t.vars.begin(), t.vars.end(), v) - t.vars.begin()] = npc;
            const int32_t map_off = (int32_t)prog.eaux.size();
            for (int64_t e = 0; e < T; ++e) {
                int64_t r = e, cell = foff[v];
                for (size_t j = 0; j < t.vars.size(); ++j) cell += (r / t.cum[j]) * stride[j], r %= t.cum[j];
                prog.eaux.push_back((int32_t)cell);
            }
            const int32_t grp_off = (int32_t)prog.eaux.size();
            const std::vector<int32_t> g = GroupBy(&prog.eaux[map_off], T);
            prog.eaux.insert(prog.eaux.end(), g.begin(), g.end());
            rec.insert(rec.end(), {v, (int32_t)foff[v], (int32_t)(foff[v + 1] - foff[v]), map_off, grp_off});
        }
        q.fam_off = (int32_t)prog.eaux.size();
        prog.eaux.insert(prog.eaux.end(), rec.begin(), rec.end());
        if (prog.eaux.size() > (size_t)INT32_MAX / 2) return SetError(FBN_ERR_LIMIT, "em program too large");
    }
    // the parent's entries grouped by the child's separator entry
    for (int c = 0; c < nc; ++c) {
        JtEClique &q = prog.ecl[c];
        q.slot = -1, q.pgroup_off = 0;
        const int p = M.cl[c].parent;
        if (p < 0) continue;
        const JtMClique &qp = M.cl[p];
        for (int j = 0; j < qp.k; ++j)
            if (M.aux[qp.child_off + 4 * j + 3] == c) q.slot = j;
        if (q.slot < 0) return SetError(FBN_ERR_ARG, "internal: clique %d is not a child of its parent", c);
        q.pgroup_off = (int32_t)prog.eaux.size();
        const std::vector<int32_t> g = GroupBy(&M.aux[M.cl[c].parent_map_off], qp.T);
        prog.eaux.insert(prog.eaux.end(), g.begin(), g.end());
        if (prog.eaux.size() > (size_t)INT32_MAX / 2) return SetError(FBN_ERR_LIMIT, "em program too large");
    }
    return FBN_OK;
}

int EmThetaFromNetwork(const JTProgramEm &P, const Network &st, const Network &net, std::vector<double> &theta) {
    if (net.n() != st.n()) return SetError(FBN_ERR_ARG, "em: the network has %d nodes, the handle's %d", net.n(), st.n());
    for (int v = 0; v < st.n(); ++v)
        if (net.dom[v] != st.dom[v] || net.parents_asc[v] != st.parents_asc[v])
            return SetError(FBN_ERR_ARG, "em: node %d differs from the handle's structure (states or parents)", v);
    theta.assign((size_t)P.cells, 0.0);
    for (int v = 0; v < st.n(); ++v) {
        const std::vector<int> &pa = st.parents_asc[v];
        const int64_t off = P.node_rec[3 * v], npc = P.node_rec[3 * v + 1];
        std::vector<int> pv(pa.size());
        for (int64_t pc = 0; pc < npc; ++pc) {
            int64_t r = pc;
            for (int j = (int)pa.size() - 1; j >= 0; --j) pv[j] = (int)(r % st.dom[pa[j]]), r /= st.dom[pa[j]];
            for (int q = 0; q < st.dom[v]; ++q) theta[(size_t)(off + q * npc + pc)] = net.Prob(v, q, pv.data());
        }
    }
    return FBN_OK;
}

void EmRebuildPotentials(const JTProgramEm &P, const double *theta, double *initv) {
    for (size_t c = 0; c < P.ecl.size(); ++c) {
        const JtEClique &q = P.ecl[c];
        const JtMClique &m = P.M.cl[c];
        for (int64_t e = 0; e < m.T; ++e) {
            double x = 1.0;
            for (int f = 0; f < q.nfam; ++f) x = x * theta[P.eaux[P.eaux[q.fam_off + kEmFamRec * f + 3] + e]];
            initv[m.iv_off + e] = x;
        }
    }
}

int EmCheckPotentials(const JTProgramEm &P, const double *initv) {
    for (size_t c = 0; c < P.M.cl.size(); ++c) {
        const JtMClique &m = P.M.cl[c];
        if (int rc = CheckCliquePotential((int)c, &P.M.aux[m.vars_off], m.nv, initv + m.iv_off, m.T)) return rc;
    }
    return FBN_OK;
}

void EmMstep(const JTProgramEm &P, const double *counts, double alpha, double *theta) {
    for (int64_t cell = 0; cell < P.cells; ++cell) {
        const int32_t *r = &P.node_rec[3 * P.cell_node[(size_t)cell]];
        const int64_t pc = (cell - r[0]) % r[1];
        double tot = 0.0;
        for (int q = 0; q < r[2]; ++q) tot = tot + counts[r[0] + q * (int64_t)r[1] + pc];
        theta[cell] = (counts[cell] + alpha) / (tot + alpha * (double)r[2]);
    }
}

}  // namespace fbn
