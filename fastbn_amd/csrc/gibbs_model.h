// gibbs_model.h -- what the Gibbs sampler's host twin (gibbs_host.cpp) and its kernels (gibbs.hip)
// share: the children CSR beside the flattened network, the conditional of one variable given its
// Markov blanket, the draw from it and the Rao-Blackwell term, each defined once and compiled by both
// sides (include/fastbn.h, "Gibbs sampling", is the specification).
//
// Both sides keep a chunk of 64 chains in the same layout: values x[v * 64 + lane] (bytes), conditional
// scratch g[k * 64 + lane] (doubles), cached parent configurations pc[t * 64 + lane] (int32, by
// topological position).  The functions below take the lane's column of each (pointer + lane), so a lane
// touches nothing another lane owns.
#ifndef FBN_GIBBS_MODEL_H
#define FBN_GIBBS_MODEL_H

#include <cstdint>
#include <vector>

#include "sample_model.h"

// fbn_gibbs_set_tuning: the most dynamic LDS a workgroup may take (also the maximum: one workgroup's
// share of a gfx950 CU)
#define FBN_GIBBS_LDS_DEFAULT ((int64_t)160 * 1024)
// workgroups per CU of the persistent grid (one wave each)
#define FBN_GIBBS_GROUPS_PER_CU 16
// smallest product of the smallest positive CPT entries of a node and its children a network may have:
// DBL_MIN * 2^53, so no conditional entry is subnormal or rounds to zero (0x1p-969)
#define FBN_GIBBS_MIN_PRODUCT 0x1p-969

namespace fbn {

// The children of every node beside SamplerModel: node t (topological position) has the entries
// e in [coff[t], coff[t + 1]), ascending by the child's position; child[2 e] = the child's position,
// child[2 e + 1] = the stride of t's variable in the child's parent configuration.
struct GibbsModel {
    std::vector<int32_t> coff, child;
    int dmax = 1;
};
// FBN_ERR_LIMIT naming the node whose family products can underflow (FBN_GIBBS_MIN_PRODUCT)
int BuildGibbsModel(const SamplerModel &M, GibbsModel &G);

// the tables both sides read (host: the vectors' data; device: their uploads)
struct GibbsView {
    const SampleNode *nodes;
    const int32_t *par;
    const double *prob, *cdf;
    const int32_t *coff, *child;
    int V, sum_dom;
};
inline GibbsView HostGibbsView(const SamplerModel &M, const GibbsModel &G) {
    return GibbsView{M.nodes.data(), M.par.data(), M.prob.data(), M.cdf.data(), G.coff.data(), G.child.data(), M.V, M.sum_dom};
}

// passes and stream positions of one chain: the start, burn_in discarded sweeps, `sweeps` counted ones
FBN_HD long long GibbsPasses(long long burn_in, long long sweeps) { return 1 + burn_in + sweeps; }

FBN_HD int GibbsParentConfig(const GibbsView &G, const SampleNode &nd, const uint8_t *x) {
    int pc = 0;
    for (int j = 0; j < nd.npar; ++j) pc = pc * G.par[2 * (nd.poff + j) + 1] + x[G.par[2 * (nd.poff + j)] * 64];
    return pc;
}

// The unnormalised conditional of node t given every other value of the lane:
//   g[k] = P(v = k | pa(v)) * prod_c P(x_c | pa(c) with v = k),  k ascending, children in CSR order,
// the product formed left to right; returns tot, the running sum of g in ascending k from 0.0.
// pc: the lane's cached parent configurations, or NULL (recomputed from x: the same integers).
FBN_HD double GibbsConditional(const GibbsView &G, int t, const uint8_t *x, const int32_t *pc, double *g) {
    const SampleNode nd = G.nodes[t];
    const int d = nd.d, xo = x[nd.v * 64];
    const double *row = G.prob + nd.toff + (long long)(pc ? pc[t * 64] : GibbsParentConfig(G, nd, x)) * d;
    for (int k = 0; k < d; ++k) g[k * 64] = row[k];
    for (int e = G.coff[t]; e < G.coff[t + 1]; ++e) {
        const int ct = G.child[2 * e], st = G.child[2 * e + 1];
        const SampleNode cn = G.nodes[ct];
        const int pcc = pc ? pc[ct * 64] : GibbsParentConfig(G, cn, x);
        // the child's entry with v's digit at 0; v = k is k * st configurations on
        const double *col = G.prob + cn.toff + (long long)(pcc - xo * st) * cn.d + x[cn.v * 64];
        const long long step = (long long)st * cn.d;
        for (int k = 0; k < d; ++k) g[k * 64] = g[k * 64] * col[k * step];
    }
    double tot = 0.0;
    for (int k = 0; k < d; ++k) tot = tot + g[k * 64];
    return tot;
}

// SelectValue over the running sums of g (the sums tot was formed from)
FBN_HD int GibbsSelect(const double *g, int d, double u, double tot) {
    const double x = u * tot;
    double c = 0.0;
    int q = 0;
    for (;; ++q) {
        c = c + g[q * 64];
        if (!(q < d - 1 && x >= c)) break;
    }
    return q;
}

// the Rao-Blackwell term of entry k: the normalised conditional; in a dead end (tot == 0) the kept value
FBN_HD double GibbsTerm(const double *g, int k, double tot, int kept) {
    return tot == 0.0 ? (k == kept ? 1.0 : 0.0) : g[k * 64] / tot;
}

// chains >= 1, burn_in >= 0, sweeps >= 1, ncases, case_offset >= 0 and stream positions
// ((case_offset + ncases) * chains + 64) * V * passes below 2^63, else FBN_ERR_ARG; more than 2^31 - 1
// (case, chunk) units in one call: FBN_ERR_LIMIT
int CheckGibbsShape(const SamplerModel &M, int64_t ncases, int64_t chains, int64_t burn_in, int64_t sweeps,
                    int64_t case_offset);
// The algorithm on CPU threads, operation for operation what the kernels do.  labels [ncases], marg
// [ncases][sum_dom] or NULL, states int8 [ncases][chains][V] or NULL.
int HostGibbs(const SamplerModel &M, const GibbsModel &G, const int8_t *ev, int64_t ncases, int64_t chains,
              int64_t burn_in, int64_t sweeps, uint64_t seed, int64_t case_offset, int32_t *labels, double *marg,
              int8_t *states);
// complete assignments in range, else FBN_ERR_ARG naming the first bad one
int CheckGibbsStates(const SamplerModel &M, const int8_t *states, int64_t n);
// out [n][sum_dom]: for every assignment and variable the normalised conditional given all the others
int HostGibbsConditionals(const SamplerModel &M, const GibbsModel &G, const int8_t *states, int64_t n, double *out);

}  // namespace fbn

#if defined(__HIPCC__)
#include "sample_device.h"

namespace fbn {

// gibbs_kernel's arguments (gibbs.hip; filled by capi_gibbs.hip).  Of SampleCaseArgs: S = chains; marg is
// the finish kernel's output; stats and the debug arrays are unused.
struct GibbsDeviceArgs : SampleCaseArgs {
    const int32_t *coff, *child;
    long long burn_in, sweeps, chunks, units;  // chunks of 64 chains per case; units = ncases * chunks
    int dmax;
    int pc_cache;    // the parent configurations cached in LDS behind the scratch
    double *ws;      // [units][sum_dom]: the units' accumulator rows
    int8_t *states;  // [ncases][chains][V] or NULL
};
struct GibbsCondArgs {
    DeviceModel M;
    const int32_t *coff, *child;
    const int8_t *states;  // [n][V], checked
    long long n;
    int dmax, pc_cache;
    double *out;  // [n][sum_dom]
};

}  // namespace fbn
#endif

#endif
