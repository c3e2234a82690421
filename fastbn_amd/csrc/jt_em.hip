// jt_em.hip -- expectation-maximisation on gfx950: the E-step of include/fastbn.h (above fbn_em_create)
// over the program of jt_em_program.h, the reduction of the waves' counts, and the M-step with the
// rebuild of the initial potentials.
//
// The E-step has jt_mpe_kernel's shape.  One lane = one data row: the 64-lane wave walks the cliques in
// lock-step, so every loop bound, index map, entry list, initial potential and digit word is
// wave-uniform and comes through the const __restrict__ pointers as a scalar load.  The per-case state is
// the store [row][64] of one wave in global memory (upward message rows, exponent rows, downward message
// rows): a row access is one coalesced 512-byte transaction.  Waves are persistent and recycle their
// store for the next 64 rows.  No atomics; a case leaves its lane only when its posteriors are counted.
//
// Clique tables are never stored: v(e) is recomputed in Collect, in the parent's pass that forms a
// downward message, in the pass that forms Z and in one pass per hosted family.  Addition is not
// order-free, so every sum follows the stated ascending-entry order: the host compiled, for each
// separator entry and each family cell, the ascending list of the entries that map to it, and the
// running sum of one such list lives in a register -- nothing is read-modify-written per entry.  kU
// lists are walked at once (kU independent chains keep kU message rows in flight).
//
// Counts: the posterior of a cell is summed over the wave's 64 cases by wave_sum (ci_wave.h: a butterfly,
// the same bits in every lane) and lane 0 adds the sum to the wave's own accumulator, one update per
// cell and block -- in LDS while the cells fit the workgroup's share of the CU's LDS (written out when
// the wave retires), else directly in the wave's private global row.  The reduction kernel then adds
// the waves' accumulators in wave order.  A tail lane runs on a copy of the last case and adds exactly 0.
// (Per-lane count rows [cell][64] in the store with a lane reduction at the end were measured too and
// lost: DESIGN.md 5.10.)
//
// Numerics: the host twin's operations in the host twin's order (-ffp-contract=off: no FMA) -- the
// same per-case bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ci_wave.h"
#include "jt_em_program.h"
#include "launchers.h"

namespace {

#define ROW(r) S[(size_t)(r) * 64]

struct JtEParams {
    long long ncases, store_rows;
    int nc, V, msg_rows, nsep, cells;
};

extern __shared__ double em_lds_acc[];

// evidence pattern of a clique for this lane's case
struct EvMask {
    uint64_t M0, M1, M2, M3, W0, W1, W2, W3;
    __device__ __forceinline__ bool consistent(const uint64_t *__restrict__ d, int nw) const {
        bool cons = (d[0] & M0) == W0;
        if (nw > 1) cons = cons && ((d[1] & M1) == W1);
        if (nw > 2) cons = cons && ((d[2] & M2) == W2);
        if (nw > 3) cons = cons && ((d[3] & M3) == W3);
        return cons;
    }
};
__device__ __forceinline__ EvMask make_mask(const int32_t *__restrict__ vars, int nv, const int8_t *__restrict__ ev) {
    EvMask k{0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < nv; ++j) {
        const int x = ev[vars[j]];
        const uint64_t m = x >= 0 ? (0xFFull << (8 * (j & 7))) : 0ull;
        const uint64_t w = x >= 0 ? ((uint64_t)x << (8 * (j & 7))) : 0ull;
        if (j < 8) k.M0 |= m, k.W0 |= w;
        else if (j < 16) k.M1 |= m, k.W1 |= w;
        else if (j < 24) k.M2 |= m, k.W2 |= w;
        else k.M3 |= m, k.W3 |= w;
    }
    return k;
}

// For the kU wave-uniform entries e[u] of clique q (all valid indices; u >= n are repeats, reported
// masked): ((init[e] * M_1[map_1(e)]) * M_2[map_2(e)]) ... over the children in clique_down order
// without child `skip` (-1: all), then * D_q[up(e)] where down0 >= 0 and q is not a root.
constexpr int kU = 4;
__device__ __forceinline__ void entry_values(const double *S, const JtMClique &q, const int32_t *__restrict__ aux,
                                             const double *__restrict__ initv, const uint64_t *__restrict__ dig,
                                             const EvMask &mk, const int (&e)[kU], int n, int skip, int down0,
                                             double (&v)[kU], bool (&cons)[kU]) {
    const double *__restrict__ iv = initv + q.iv_off;
    const uint64_t *__restrict__ dg = dig + q.dig_off;
    const int32_t *__restrict__ rec = aux + q.child_off;
#pragma unroll
    for (int u = 0; u < kU; ++u) {
        v[u] = iv[e[u]];
        cons[u] = u < n && mk.consistent(dg + (size_t)e[u] * q.nw, q.nw);
    }
    for (int j = 0; j < q.k; ++j) {
        if (j == skip) continue;
        const int mo = rec[4 * j], row = rec[4 * j + 1];
#pragma unroll
        for (int u = 0; u < kU; ++u) v[u] = v[u] * ROW(row + aux[mo + e[u]]);
    }
    if (down0 >= 0 && q.parent >= 0) {
#pragma unroll
        for (int u = 0; u < kU; ++u) v[u] = v[u] * ROW(down0 + q.up_row + aux[q.up_map_off + e[u]]);
    }
}

// rows r0 .. r0 + n - 1 scaled by the power of two that brings their maximum mx into [0.5, 1) -> its exponent
__device__ __forceinline__ int rescale_rows(double *S, int r0, int n, double mx) {
    int k = 0;
    (void)frexp(mx, &k);
    for (int s = 0; s < n; ++s) ROW(r0 + s) = ldexp(ROW(r0 + s), -k);
    return k;
}

template <bool kLdsAcc>
__global__ __launch_bounds__(64) void jt_em_estep_kernel(const JtMClique *__restrict__ cl, const JtEClique *__restrict__ ecl,
                                                         const int32_t *__restrict__ aux, const int32_t *__restrict__ eaux,
                                                         const double *__restrict__ initv, const uint64_t *__restrict__ dig,
                                                         const int32_t *__restrict__ collect,
                                                         const int32_t *__restrict__ trace, const int8_t *__restrict__ data,
                                                         double *__restrict__ value, double *__restrict__ dbg_post,
                                                         double *__restrict__ store, double *__restrict__ wacc,
                                                         JtEParams P) {
    const int lane = threadIdx.x;
    double *__restrict__ S = store + (size_t)blockIdx.x * (size_t)P.store_rows * 64 + lane;
    const int down0 = P.msg_rows + P.nsep;
    // the wave's accumulator [cells]: LDS (zeroed here), or its row of wacc (zeroed by the launcher's caller)
    double *__restrict__ gacc = wacc + (size_t)blockIdx.x * (size_t)P.cells;
    if (kLdsAcc)
        for (int c = lane; c < P.cells; c += 64) em_lds_acc[c] = 0.0;

    for (long long blk = blockIdx.x; blk * 64 < P.ncases; blk += gridDim.x) {
        const long long cs = blk * 64 + lane;
        const bool act = cs < P.ncases;
        const long long csr = act ? cs : P.ncases - 1;  // a tail lane runs on a copy of the last case
        const int8_t *__restrict__ ev = data + csr * P.V;

        // ---- Collect: deepest level first
        double m = 1.0;
        int ex = 0;
        for (int i = 0; i < P.nc; ++i) {
            const JtMClique q = cl[collect[i]];
            const EvMask mk = make_mask(aux + q.vars_off, q.nv, ev);
            const int32_t *__restrict__ rec = aux + q.child_off;
            int esum = 0;
            for (int j = 0; j < q.k; ++j) esum += (int)__double_as_longlong(ROW(rec[4 * j + 2]));
            if (q.parent >= 0) {
                // up(e) = e % Ts: the entries of separator entry s are s, s + Ts, ... ascending
                const int Ts = q.up_Ts, per = q.T / Ts;
                double mx = 0.0;
                for (int s0 = 0; s0 < Ts; s0 += kU) {
                    const int n = Ts - s0 < kU ? Ts - s0 : kU;
                    double acc[kU];
#pragma unroll
                    for (int u = 0; u < kU; ++u) acc[u] = 0.0;
                    for (int qi = 0; qi < per; ++qi) {
                        int e[kU];
                        double v[kU];
                        bool cons[kU];
#pragma unroll
                        for (int u = 0; u < kU; ++u) e[u] = qi * Ts + s0 + (u < n ? u : 0);
                        entry_values(S, q, aux, initv, dig, mk, e, n, -1, -1, v, cons);
#pragma unroll
                        for (int u = 0; u < kU; ++u) acc[u] = cons[u] ? acc[u] + v[u] : acc[u];
                    }
#pragma unroll
                    for (int u = 0; u < kU; ++u)
                        if (u < n) {
                            ROW(q.up_row + s0 + u) = acc[u];
                            mx = acc[u] > mx ? acc[u] : mx;
                        }
                }
                const int k = rescale_rows(S, q.up_row, Ts, mx);
                ROW(q.up_exp_row) = __longlong_as_double((long long)k + esum);
            } else {
                double sum = 0.0;
                for (int e0 = 0; e0 < q.T; e0 += kU) {
                    const int n = q.T - e0 < kU ? q.T - e0 : kU;
                    int e[kU];
                    double v[kU];
                    bool cons[kU];
#pragma unroll
                    for (int u = 0; u < kU; ++u) e[u] = e0 + (u < n ? u : 0);
                    entry_values(S, q, aux, initv, dig, mk, e, n, -1, -1, v, cons);
#pragma unroll
                    for (int u = 0; u < kU; ++u) sum = cons[u] ? sum + v[u] : sum;  // ascending e
                }
                int k = 0;
                const double f = frexp(sum, &k);
                ex += k + esum;
                m = frexp(m * f, &k);
                ex += k;
            }
        }
        if (act && value) value[2 * cs] = m, value[2 * cs + 1] = (double)ex;

        // ---- Distribute and the family posteriors: levels ascending
        for (int i = 0; i < P.nc; ++i) {
            const int c = trace[i];
            const JtMClique q = cl[c];
            const JtEClique qe = ecl[c];
            if (q.parent >= 0) {
                // D_c[s] over the parent's entries that map to s, ascending
                const JtMClique qp = cl[q.parent];
                const EvMask mp = make_mask(aux + qp.vars_off, qp.nv, ev);
                const int32_t *__restrict__ grp = eaux + qe.pgroup_off;
                const int Ts = q.up_Ts, per = qp.T / Ts;
                double mx = 0.0;
                for (int s0 = 0; s0 < Ts; s0 += kU) {
                    const int n = Ts - s0 < kU ? Ts - s0 : kU;
                    double acc[kU];
#pragma unroll
                    for (int u = 0; u < kU; ++u) acc[u] = 0.0;
                    for (int qi = 0; qi < per; ++qi) {
                        int e[kU];
                        double v[kU];
                        bool cons[kU];
#pragma unroll
                        for (int u = 0; u < kU; ++u) e[u] = grp[(s0 + (u < n ? u : 0)) * per + qi];
                        entry_values(S, qp, aux, initv, dig, mp, e, n, qe.slot, down0, v, cons);
#pragma unroll
                        for (int u = 0; u < kU; ++u) acc[u] = cons[u] ? acc[u] + v[u] : acc[u];
                    }
#pragma unroll
                    for (int u = 0; u < kU; ++u)
                        if (u < n) {
                            ROW(down0 + q.up_row + s0 + u) = acc[u];
                            mx = acc[u] > mx ? acc[u] : mx;
                        }
                }
                (void)rescale_rows(S, down0 + q.up_row, Ts, mx);
            }
            if (qe.nfam == 0) continue;
            const EvMask mk = make_mask(aux + q.vars_off, q.nv, ev);
            double Z = 0.0;
            for (int e0 = 0; e0 < q.T; e0 += kU) {
                const int n = q.T - e0 < kU ? q.T - e0 : kU;
                int e[kU];
                double v[kU];
                bool cons[kU];
#pragma unroll
                for (int u = 0; u < kU; ++u) e[u] = e0 + (u < n ? u : 0);
                entry_values(S, q, aux, initv, dig, mk, e, n, -1, down0, v, cons);
#pragma unroll
                for (int u = 0; u < kU; ++u) Z = cons[u] ? Z + v[u] : Z;  // ascending e
            }
            for (int f = 0; f < qe.nfam; ++f) {
                const int32_t *__restrict__ fr = eaux + qe.fam_off + kEmFamRec * f;
                const int cell0 = fr[1], ncell = fr[2], per = q.T / ncell;
                const int32_t *__restrict__ grp = eaux + fr[4];
                for (int c0 = 0; c0 < ncell; c0 += kU) {
                    const int n = ncell - c0 < kU ? ncell - c0 : kU;
                    double acc[kU];
#pragma unroll
                    for (int u = 0; u < kU; ++u) acc[u] = 0.0;
                    for (int qi = 0; qi < per; ++qi) {
                        int e[kU];
                        double v[kU];
                        bool cons[kU];
#pragma unroll
                        for (int u = 0; u < kU; ++u) e[u] = grp[(c0 + (u < n ? u : 0)) * per + qi];
                        entry_values(S, q, aux, initv, dig, mk, e, n, -1, down0, v, cons);
#pragma unroll
                        for (int u = 0; u < kU; ++u) acc[u] = cons[u] ? acc[u] + v[u] / Z : acc[u];
                    }
#pragma unroll
                    for (int u = 0; u < kU; ++u)
                        if (u < n) {
                            const int cell = cell0 + c0 + u;
                            const double ws = wave_sum(act ? acc[u] : 0.0);
                            if (lane == 0) {
                                if (kLdsAcc) em_lds_acc[cell] = em_lds_acc[cell] + ws;
                                else gacc[cell] = gacc[cell] + ws;
                            }
                            if (dbg_post && act) dbg_post[cs * P.cells + cell] = acc[u];
                        }
                }
            }
        }
    }
    if (kLdsAcc)
        for (int c = lane; c < P.cells; c += 64) gacc[c] = em_lds_acc[c];
}

// counts[cell] = the waves' accumulators added in wave order; one thread per cell
__global__ __launch_bounds__(256) void jt_em_reduce_kernel(const double *__restrict__ wacc, double *__restrict__ counts,
                                                           int cells, int grid) {
    const int cell = blockIdx.x * 256 + threadIdx.x;
    if (cell >= cells) return;
    double x = 0.0;
    for (int w = 0; w < grid; ++w) x = x + wacc[(size_t)w * cells + cell];
    counts[cell] = x;
}

// theta from the counts (one thread per cell), then the initial potentials from theta (one thread per
// clique entry); one workgroup, so the barrier between the two orders them
constexpr int kMstepThreads = 1024;
__global__ __launch_bounds__(kMstepThreads) void jt_em_mstep_kernel(JtEmMstepArgs a) {
    for (int cell = threadIdx.x; cell < a.cells; cell += kMstepThreads) {
        const int32_t *__restrict__ r = a.node_rec + 3 * a.cell_node[cell];
        const int pc = (cell - r[0]) % r[1];
        double tot = 0.0;
        for (int q = 0; q < r[2]; ++q) tot = tot + a.counts[r[0] + (size_t)q * r[1] + pc];
        a.theta[cell] = (a.counts[cell] + a.alpha) / (tot + a.alpha * (double)r[2]);
    }
    __threadfence();
    __syncthreads();
    for (int g = threadIdx.x; g < a.entries; g += kMstepThreads) {
        const int c = a.entry_clique[g];
        const int e = g - a.cl[c].iv_off;
        const JtEClique q = a.ecl[c];
        double x = 1.0;
        for (int f = 0; f < q.nfam; ++f) x = x * a.theta[a.eaux[a.eaux[q.fam_off + kEmFamRec * f + 3] + e]];
        a.initv[g] = x;
    }
}

}  // namespace

extern "C" hipError_t fbn_em_estep_launch(const JtEmArgs *a, hipStream_t stream) {
    JtEParams P;
    P.ncases = a->ncases, P.store_rows = a->store_rows;
    P.nc = a->nc, P.V = a->V, P.msg_rows = a->msg_rows, P.nsep = a->nsep, P.cells = a->cells;
    if (a->lds_acc)
        hipLaunchKernelGGL(jt_em_estep_kernel<true>, dim3(a->grid), dim3(64), (size_t)a->cells * 8, stream, a->cl, a->ecl,
                           a->aux, a->eaux, a->initv, a->dig, a->collect, a->trace, a->data, a->value, a->dbg_post,
                           a->store, a->wacc, P);
    else
        hipLaunchKernelGGL(jt_em_estep_kernel<false>, dim3(a->grid), dim3(64), 0, stream, a->cl, a->ecl, a->aux, a->eaux,
                           a->initv, a->dig, a->collect, a->trace, a->data, a->value, a->dbg_post, a->store, a->wacc, P);
    return hipGetLastError();
}

extern "C" hipError_t fbn_em_reduce_launch(const JtEmReduceArgs *a, hipStream_t stream) {
    hipLaunchKernelGGL(jt_em_reduce_kernel, dim3((a->cells + 255) / 256), dim3(256), 0, stream, a->wacc, a->counts,
                       a->cells, a->grid);
    return hipGetLastError();
}

extern "C" hipError_t fbn_em_mstep_launch(const JtEmMstepArgs *a, hipStream_t stream) {
    hipLaunchKernelGGL(jt_em_mstep_kernel, dim3(1), dim3(kMstepThreads), 0, stream, *a);
    return hipGetLastError();
}
