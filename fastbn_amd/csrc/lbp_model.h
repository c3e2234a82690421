// lbp_model.h -- what loopy belief propagation's host twin (lbp_host.cpp) and its kernel (lbp.hip)
// share: the factor graph of a network, flattened, and the exact digit extraction both use.
//
// One factor per node f over (f, GIVEN parents of f in the node's own order); its table is
// prob[toff + pc * d + q], pc over the GIVEN parents, last parent fastest (the sampler's layout).
// Edge (f, slot), slot 0 = f itself, slot j = the j-th GIVEN parent; edges are numbered with f
// ascending, slot ascending.  Edge e carries two messages of dom(x_e) doubles, factor -> variable m
// and variable -> factor mu, at entries [moff, moff + d) of two arrays of M = sum_e dom(x_e) doubles.
#ifndef FBN_LBP_MODEL_H
#define FBN_LBP_MODEL_H

#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FBN_LBP_HD __host__ __device__ __forceinline__
#else
#define FBN_LBP_HD inline
#endif

// fbn_lbp_debug_messages: doubles per call (ncases * 2 * M)
#define FBN_LBP_DEBUG_MAX ((int64_t)1 << 24)

namespace fbn {

// The table cells with x_slot = q are c = k + (hi * (d - 1) + q) * stride, hi = k / stride, for
// k = 0 .. ncell - 1 in ascending c: k numbers the cells of the table without this slot.
struct LbpEdge {
    int32_t x, d;        // the variable in this slot, its state count
    int32_t moff;        // first message entry
    int32_t toff;        // first cell of the factor's table
    int32_t stride;      // cells between consecutive values of x
    int32_t ncell;       // table cells / d
    int32_t term, nterm; // the factor's other slots, ascending: terms[term .. term + nterm)
    double rinv;         // 1.0 / stride
};
// One other slot u of the factor, seen from an edge.  Ascending slot order is slot 0 (the least
// significant digit of k), then the parents from the most to the least significant.  Slot 0's
// term (lsd = 1, rstride = its state count) takes digit = k % rstride and leaves r = k; a parent's
// term takes digit = r / rstride and r -= digit * rstride (rstride: its stride in the table without
// the edge's own slot).
struct LbpTerm {
    int32_t moff;     // first entry of that slot's variable -> factor message
    int32_t rstride;
    int32_t lsd;
    int32_t pad;
    double rinv;      // 1.0 / rstride
};
// n / s for 0 <= n < 2^26 and 1 <= s <= 2^26 with rinv = 1.0 / s: n * rinv is within 2^-26 of n / s,
// so its truncation is the quotient or one beside it; the remainder tests settle which.  Integer
// results, hence the same on host and device.
FBN_LBP_HD int LbpDiv(int n, int s, double rinv) {
    int q = (int)((double)n * rinv);
    if (n - q * s >= s) ++q;
    if (n - q * s < 0) --q;
    return q;
}
// the digit of term t in reduced cell index k; r carries the not yet consumed part of k
FBN_LBP_HD int LbpDigit(const LbpTerm &t, int k, int &r) {
    if (t.lsd) return k - LbpDiv(k, t.rstride, t.rinv) * t.rstride;
    const int g = LbpDiv(r, t.rstride, t.rinv);
    r -= g * t.rstride;
    return g;
}
// The unnormalised factor -> variable value of entry (edge ed, q): the sum over the cells with
// x_slot = q in ascending cell index, from 0.0, of ((P[c] * mu_u1[..]) * mu_u2[..]) ... over the other
// slots in ascending order.  The one definition both sides compile.
FBN_LBP_HD double LbpFactorRaw(const LbpEdge &ed, const LbpTerm *terms, const double *prob, const double *mu, int q) {
    const double *P = prob + ed.toff;
    const LbpTerm *T = terms + ed.term;
    const int add = q * ed.stride, dm1 = ed.d - 1;
    double acc = 0.0;
    for (int k = 0; k < ed.ncell; ++k) {
        const int hi = LbpDiv(k, ed.stride, ed.rinv);
        double p = P[k + hi * dm1 * ed.stride + add];
        int r = k;
        for (int t = 0; t < ed.nterm; ++t) {
            const LbpTerm tm = T[t];
            p = p * mu[tm.moff + LbpDigit(tm, k, r)];
        }
        acc = acc + p;
    }
    return acc;
}
// The product from 1.0 of m_g[q] over the edges on a variable (their moff in vm[0 .. n), ascending)
// but the one at `skip` (-1: none, the belief).
FBN_LBP_HD double LbpVarRaw(const int32_t *vm, int n, int skip, const double *m, int q) {
    double p = 1.0;
    for (int i = 0; i < n; ++i)
        if (vm[i] != skip) p = p * m[vm[i] + q];
    return p;
}
// sum of a row in ascending order from its first entry
FBN_LBP_HD double LbpRowSum(const double *row, int d) {
    double z = row[0];
    for (int q = 1; q < d; ++q) z = z + row[q];
    return z;
}
FBN_LBP_HD bool LbpBadZ(double z) { return !(z > 0.0 && z <= 1.7976931348623157e308); }

struct LbpModel {
    int V = 0, E = 0, sum_dom = 0;
    int64_t M = 0, cells = 0;
    std::vector<int32_t> dom;
    std::vector<LbpEdge> edges;
    std::vector<LbpTerm> terms;
    std::vector<int32_t> bin_edge;   // message entry -> edge
    std::vector<int32_t> order;      // message entries by descending cost of their factor pass (cells x slots), ties ascending
    std::vector<int32_t> var_off;    // [V + 1] into var_moff
    std::vector<int32_t> var_moff;   // the edges on a variable, ascending: their moff
    std::vector<int32_t> marg_var;   // marginal entry -> variable
    std::vector<int32_t> marg_off;   // [V] first marginal entry
    std::vector<int32_t> self_moff;  // [V] moff of edge (f = x, slot 0): x's message into its own family
    std::vector<double> prob;
};
// the kernel's arguments (device pointers): the model, one batch, where the messages live
struct LbpDeviceArgs {
    const LbpEdge *edges;
    const LbpTerm *terms;
    const int32_t *bin_edge, *order, *var_off, *var_moff, *marg_var, *marg_off, *dom;
    const double *prob;
    const int8_t *ev;  // [ncases][V], checked
    int V, SD, M, d0;  // d0: states of variable 0, the query
    long long ncases;
    int iters;
    double tol, damping;  // tol < 0: never stops early
    int32_t *labels;
    double *marg;      // [ncases][SD] or NULL
    double *stats;     // [ncases][2] or NULL
    double *messages;  // [ncases][2][M] or NULL
    double *ws;        // global path: [grid][3][M]
    // EPIS-BN's importance function (epis_model.h), or NULL: lambda [ncases][SD], entry (x, q) = mu of
    // edge (f = x, slot 0) at q as the run leaves it, a row of 1.0 for a case that failed
    double *lambda;
    const int32_t *self_moff;
};
struct Network;
// FBN_ERR_ARG for a cyclic network, FBN_ERR_LIMIT past FBN_PARAM_MAX_CELLS table cells
int BuildLbpModel(const Network &net, LbpModel &M);

// iters >= 1, tol >= 0 (not NaN), 0 <= damping < 1, else FBN_ERR_ARG
int CheckLbpArgs(int64_t ncases, int iters, double tol, double damping);
// -1 .. dom - 1 everywhere, else FBN_ERR_ARG naming the first bad case / node
int CheckLbpEvidence(const LbpModel &M, const int8_t *ev, int64_t ncases);
// The algorithm over cases on CPU threads, operation for operation what the kernel does.  labels
// [ncases], marg [ncases][sum_dom] or NULL, stats [ncases][2] or NULL, messages [ncases][2][M] or
// NULL, lambda [ncases][sum_dom] (LbpDeviceArgs::lambda) or NULL.  tol < 0: never stops early
// (fbn_lbp_debug_messages).
int HostLbp(const LbpModel &M, const int8_t *ev, int64_t ncases, int iters, double tol, double damping,
            int32_t *labels, double *marg, double *stats, double *messages, double *lambda = nullptr);

}  // namespace fbn

// What EPIS-BN's handle (capi_epis.hip) needs of an fbn_lbp beyond include/fastbn.h (capi_lbp.hip):
// its model, and a run on the device that writes the lambda rows [ncases][sum_dom] (no marginals;
// d_stats [ncases][2]) for evidence the caller has range-checked, asynchronous on the stream.
struct fbn_lbp;
namespace fbn {
const LbpModel &LbpModelOf(const fbn_lbp *s);
int LbpLambdaDevice(fbn_lbp *s, const int8_t *d_ev, int64_t ncases, int iters, double tol, double damping,
                    int32_t *d_labels, double *d_stats, double *d_lambda, void *hip_stream);
}  // namespace fbn

#endif
