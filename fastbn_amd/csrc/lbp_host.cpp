// lbp_host.cpp -- host side of loopy belief propagation: the flattened factor graph and the host
// twin of the kernel in lbp.hip (device < 0 handles).
//
// LBP is the reference's `-a 7`, which only prints "LBP is under development" there
// (src/main.cpp:136-147; its propagation length is Parameter::propagation_length,
// include/Parameter.h:33).  Flooding schedule, sum-product: per iteration every factor -> variable
// message is recomputed from the previous variable -> factor messages, then every variable ->
// factor message from the new factor -> variable messages; observed variables send the indicator
// of their value throughout.  Every sum and product has one stated order (lbp_model.h), so the
// twin, the kernel and a restatement in any language agree bit for bit.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <thread>

#include "fbn_internal.h"
#include "lbp_model.h"

namespace fbn {

int BuildLbpModel(const Network &net, LbpModel &M) {
    const int V = net.n();
    if (V < 1) return SetError(FBN_ERR_ARG, "lbp: empty network");
    if ((int)TopoOrder(net).size() != V) return SetError(FBN_ERR_ARG, "network has a cycle");
    M = LbpModel();
    M.V = V;
    M.dom.assign(net.dom.begin(), net.dom.end());
    // table sizes first: nothing is allocated for a network past the cap
    int64_t cells = 0, msg = 0, nterms = 0;
    for (int v = 0; v < V; ++v) {
        if (net.dom[v] < 1) return SetError(FBN_ERR_ARG, "node %d has %d states", v, net.dom[v]);
        int64_t c = net.dom[v];
        msg += net.dom[v];
        for (int p : net.given[v]) {
            c *= net.dom[p];
            msg += net.dom[p];
            if (c > FBN_PARAM_MAX_CELLS) break;
        }
        cells += c;
        nterms += (int64_t)net.given[v].size() * (int64_t)(net.given[v].size() + 1);
        if (c > FBN_PARAM_MAX_CELLS || cells > FBN_PARAM_MAX_CELLS)
            return SetError(FBN_ERR_LIMIT, "lbp: tables beyond %lld cells (node %d)", (long long)FBN_PARAM_MAX_CELLS, v);
    }
    if (msg > 0x3fffffff || nterms > 0x3fffffff) return SetError(FBN_ERR_LIMIT, "lbp: %lld message entries", (long long)msg);
    M.cells = cells;
    M.prob.resize((size_t)cells);
    M.marg_off.resize(V);
    M.self_moff.resize(V);
    for (int v = 0; v < V; ++v) {
        M.marg_off[v] = M.sum_dom;
        M.marg_var.insert(M.marg_var.end(), net.dom[v], v);
        M.sum_dom += net.dom[v];
    }
    std::vector<std::vector<int32_t>> on(V);  // moff of the edges on each variable
    int64_t toff = 0;
    int32_t moff = 0;
    for (int f = 0; f < V; ++f) {
        const std::vector<int> &g = net.given[f];
        const int ns = (int)g.size() + 1, d = net.dom[f];
        std::vector<int> var(ns), stride(ns);
        var[0] = f, stride[0] = 1;
        int64_t s = d;
        for (int j = ns - 1; j >= 1; --j) var[j] = g[j - 1], stride[j] = (int)s, s *= net.dom[g[j - 1]];
        const int64_t ncell = s, ncfg = s / d;
        // rows of every parent configuration (GIVEN order, last fastest), as BuildSamplerModel's
        std::vector<int> gv(g.size(), 0), asc(net.parents_asc[f].size(), 0);
        for (int64_t pc = 0; pc < ncfg; ++pc) {
            for (size_t a = 0; a < asc.size(); ++a)
                for (size_t j = 0; j < g.size(); ++j)
                    if (g[j] == net.parents_asc[f][a]) asc[a] = gv[j];
            for (int q = 0; q < d; ++q) M.prob[(size_t)(toff + pc * d + q)] = net.Prob(f, q, asc.data());
            for (int j = (int)g.size() - 1; j >= 0; --j) {
                if (++gv[j] < net.dom[g[j]]) break;
                gv[j] = 0;
            }
        }
        std::vector<int32_t> smoff(ns);
        for (int j = 0; j < ns; ++j) smoff[j] = moff, moff += net.dom[var[j]];
        M.self_moff[f] = smoff[0];
        for (int j = 0; j < ns; ++j) {
            LbpEdge e;
            e.x = var[j], e.d = net.dom[var[j]], e.moff = smoff[j], e.toff = (int32_t)toff;
            e.stride = stride[j], e.ncell = (int32_t)(ncell / e.d);
            e.term = (int32_t)M.terms.size(), e.nterm = ns - 1;
            e.rinv = 1.0 / (double)e.stride;
            for (int u = 0; u < ns; ++u) {
                if (u == j) continue;
                LbpTerm t;
                t.moff = smoff[u], t.pad = 0;
                t.lsd = u == 0;
                t.rstride = u == 0 ? d : (stride[u] > stride[j] ? stride[u] / e.d : stride[u]);
                t.rinv = 1.0 / (double)t.rstride;
                M.terms.push_back(t);
            }
            M.edges.push_back(e);
            M.bin_edge.insert(M.bin_edge.end(), e.d, (int32_t)M.edges.size() - 1);
            on[e.x].push_back(e.moff);
        }
        toff += ncell;
    }
    M.E = (int)M.edges.size();
    M.M = moff;
    // the kernel hands entries to lanes 64 at a time and a pass lasts as long as its heaviest entry:
    // entries of similar cost go together (the order of work, not of any sum)
    M.order.resize((size_t)moff);
    for (int32_t j = 0; j < moff; ++j) M.order[j] = j;
    std::stable_sort(M.order.begin(), M.order.end(), [&](int32_t a, int32_t b) {
        const LbpEdge &ea = M.edges[M.bin_edge[a]], &eb = M.edges[M.bin_edge[b]];
        return (int64_t)ea.ncell * (ea.nterm + 1) > (int64_t)eb.ncell * (eb.nterm + 1);
    });
    M.var_off.assign(V + 1, 0);
    for (int v = 0; v < V; ++v) {
        M.var_off[v + 1] = M.var_off[v] + (int32_t)on[v].size();
        M.var_moff.insert(M.var_moff.end(), on[v].begin(), on[v].end());
    }
    if (M.terms.empty()) M.terms.push_back(LbpTerm{0, 1, 0, 0, 1.0});
    return FBN_OK;
}

int CheckLbpArgs(int64_t ncases, int iters, double tol, double damping) {
    if (ncases < 0) return SetError(FBN_ERR_ARG, "bad argument");
    if (iters < 1) return SetError(FBN_ERR_ARG, "iterations must be >= 1 (got %d)", iters);
    if (!(tol >= 0.0)) return SetError(FBN_ERR_ARG, "tol must be >= 0 (got %g)", tol);
    if (!(damping >= 0.0 && damping < 1.0)) return SetError(FBN_ERR_ARG, "damping must be in [0, 1) (got %g)", damping);
    return FBN_OK;
}

int CheckLbpEvidence(const LbpModel &M, const int8_t *ev, int64_t ncases) {
    for (int64_t c = 0; c < ncases; ++c)
        for (int v = 0; v < M.V; ++v) {
            const int x = ev[c * M.V + v];
            if (x < -1 || x >= M.dom[v])
                return SetError(FBN_ERR_ARG, "case %lld: evidence %d for node %d (domain %d)", (long long)c, x, v, M.dom[v]);
        }
    return FBN_OK;
}

int HostLbp(const LbpModel &M, const int8_t *ev, int64_t ncases, int iters, double tol, double damping,
            int32_t *labels, double *marg, double *stats, double *messages, double *lambda) {
    if (ncases == 0) return FBN_OK;
    const int V = M.V, SD = M.sum_dom;
    const size_t MM = (size_t)M.M;
    auto run = [&](int64_t c0, int64_t c1) {
        std::vector<double> buf(3 * MM);
        double *m = buf.data(), *mu = m + MM, *raw = mu + MM;
        for (int64_t c = c0; c < c1; ++c) {
            const int8_t *e_row = ev + c * V;
            for (size_t j = 0; j < MM; ++j) {
                const LbpEdge &ed = M.edges[M.bin_edge[j]];
                const int q = (int)j - ed.moff, o = e_row[ed.x];
                m[j] = 1.0 / (double)ed.d;
                mu[j] = o >= 0 ? (q == o ? 1.0 : 0.0) : 1.0 / (double)ed.d;
            }
            bool bad = false;
            int used = 0;
            double res = 0.0;
            for (int it = 1; it <= iters; ++it) {
                res = 0.0;
                for (int half = 0; half < 2; ++half) {
                    double *dst = half ? mu : m;
                    for (size_t j = 0; j < MM; ++j) {
                        const LbpEdge &ed = M.edges[M.bin_edge[j]];
                        if (e_row[ed.x] >= 0) continue;
                        const int q = (int)j - ed.moff;
                        raw[j] = half ? LbpVarRaw(M.var_moff.data() + M.var_off[ed.x], M.var_off[ed.x + 1] - M.var_off[ed.x], ed.moff, m, q)
                                      : LbpFactorRaw(ed, M.terms.data(), M.prob.data(), mu, q);
                    }
                    for (size_t j = 0; j < MM; ++j) {
                        const LbpEdge &ed = M.edges[M.bin_edge[j]];
                        if (e_row[ed.x] >= 0) continue;
                        const double z = LbpRowSum(raw + ed.moff, ed.d);
                        if (LbpBadZ(z)) {
                            bad = true;
                            continue;
                        }
                        double nw = raw[j] / z;
                        if (!half && damping != 0.0) nw = (1.0 - damping) * nw + damping * dst[j];
                        res = std::max(res, std::fabs(nw - dst[j]));
                        dst[j] = nw;
                    }
                }
                used = it;
                if (bad || res <= tol) break;
            }
            // beliefs
            for (int j = 0; j < SD; ++j) {
                const int x = M.marg_var[j];
                raw[j] = e_row[x] >= 0 ? 0.0 : LbpVarRaw(M.var_moff.data() + M.var_off[x], M.var_off[x + 1] - M.var_off[x], -1, m, j - M.marg_off[x]);
            }
            for (int x = 0; x < V && !bad; ++x)
                if (e_row[x] < 0 && LbpBadZ(LbpRowSum(raw + M.marg_off[x], M.dom[x]))) bad = true;
            int lab = -1;
            if (!bad) {
                lab = 0;
                double mp = 0.0;  // ArgMax, strict '>' from 0 (src/Inference.cpp:92-102), as fbn_jt_run
                if (e_row[0] < 0) {
                    const double z = LbpRowSum(raw, M.dom[0]);
                    for (int q = 0; q < M.dom[0]; ++q)
                        if (raw[q] / z > mp) mp = raw[q] / z, lab = q;
                }
            }
            labels[c] = lab;
            if (marg) {
                double *row = marg + c * SD;
                for (int j = 0; j < SD; ++j) {
                    const int x = M.marg_var[j];
                    row[j] = bad || e_row[x] >= 0 ? 0.0 : raw[j] / LbpRowSum(raw + M.marg_off[x], M.dom[x]);
                }
            }
            if (stats) {
                stats[2 * c] = (double)used;
                stats[2 * c + 1] = bad ? std::numeric_limits<double>::infinity() : res;
            }
            if (messages) std::copy(m, m + 2 * MM, messages + (size_t)c * 2 * MM);
            if (lambda)
                for (int j = 0; j < SD; ++j) {
                    const int x = M.marg_var[j];
                    lambda[(size_t)c * SD + j] = bad ? 1.0 : mu[M.self_moff[x] + j - M.marg_off[x]];
                }
        }
    };
    const int T = (int)std::min<int64_t>(HostThreads(), ncases);
    std::vector<std::thread> th;
    for (int t = 1; t < T; ++t) th.emplace_back(run, ncases * t / T, ncases * (t + 1) / T);
    run(0, ncases / T);
    for (auto &x : th) x.join();
    return FBN_OK;
}

}  // namespace fbn
