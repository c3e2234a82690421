// jt_mpe.hip -- batched most probable explanation on gfx950: the max-product Collect and top-down
// back-trace of include/fastbn.h (above fbn_mpe_create) over the program of jt_mpe_program.h.
//
// One lane = one evidence case, as jt_interp_kernel: the 64-lane wave walks the cliques in lock-step,
// so in Collect every loop bound, index map, initial potential and digit word is wave-uniform and
// comes through the const __restrict__ pointers as a scalar load.  The per-case state is the store
// [row][64] of one wave in global memory (message rows, exponent rows, e* rows): a row access is one
// coalesced 512-byte transaction.  Waves are persistent (grid = CUs x waves) and recycle their store
// for the next 64 cases.  No atomics, no LDS, no cross-lane traffic: a case never leaves its lane.
//
// Clique tables are never stored.  Collect forms v(e) in a register and keeps the running maximum of
// one separator entry in a register too: after the plan's reorganisation up(e) = e % Ts, and a
// maximum does not depend on the order it is taken in, so "for s, for the entries e = s (mod Ts)"
// gives the bits of the stated ascending-e scan without a read-modify-write of the message rows.
// The root's arg-max and the back-trace scan ascending e with a strict '>' exactly as stated.  In the
// back-trace the entries a lane visits depend on its parent's choice, so there the maps, digits and
// potentials are per-lane loads -- T / Ts entries per clique instead of T.
//
// Numerics: *, comparisons, frexp and ldexp only (no adds: nothing to contract), the host twin's
// operations in the host twin's order -- the same bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jt_mpe_program.h"
#include "launchers.h"

namespace {

#define ROW(r) S[(size_t)(r) * 64]

struct JtMParams {
    long long ncases, store_rows;
    int nc, V, msg_rows, nsep;
};

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

// v(e) = ((init[e] * M^_1[map_1(e)]) * M^_2[map_2(e)]) ..., children in clique_down order, for the kU
// entries e0 + u * stride at once: kU independent chains, so kU message rows are in flight per child
// (a lane's multiplies are dependent; one wave per SIMD hides nothing by itself).  With a wave-uniform
// e0 the map and digit reads are scalar loads; a message read is one row.  Entries u >= n are not
// there: they are computed on entry e0 (always a valid index) and reported masked.
constexpr int kU = 4;
__device__ __forceinline__ void entry_values(const double *S, const double *__restrict__ iv,
                                             const int32_t *__restrict__ aux, const int32_t *__restrict__ rec, int k,
                                             const uint64_t *__restrict__ dg, int nw, const EvMask &mk, int e0,
                                             int stride, int n, double (&v)[kU], bool (&cons)[kU]) {
    int e[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
        e[u] = e0 + (u < n ? u : 0) * stride;
        v[u] = iv[e[u]];
        cons[u] = u < n && mk.consistent(dg + (size_t)e[u] * nw, nw);
    }
    for (int j = 0; j < k; ++j) {
        const int mo = rec[4 * j], row = rec[4 * j + 1];
#pragma unroll
        for (int u = 0; u < kU; ++u) v[u] = v[u] * ROW(row + aux[mo + e[u]]);
    }
}

__global__ __launch_bounds__(64) void jt_mpe_kernel(const JtMClique *__restrict__ cl, const int32_t *__restrict__ aux,
                                                    const double *__restrict__ initv, const uint64_t *__restrict__ dig,
                                                    const int32_t *__restrict__ collect, const int32_t *__restrict__ trace,
                                                    const int8_t *__restrict__ evid, int8_t *__restrict__ assign,
                                                    double *__restrict__ value, double *__restrict__ dbg_msg,
                                                    int32_t *__restrict__ dbg_exp, double *__restrict__ store,
                                                    JtMParams P) {
    const int lane = threadIdx.x;
    double *__restrict__ S = store + (size_t)blockIdx.x * (size_t)P.store_rows * 64 + lane;
    const int estar0 = P.msg_rows + P.nsep;

    for (long long blk = blockIdx.x; blk * 64 < P.ncases; blk += gridDim.x) {
        const long long cs = blk * 64 + lane;
        const bool act = cs < P.ncases;
        const long long csr = act ? cs : P.ncases - 1;  // a tail lane runs on a copy of the last case
        const int8_t *__restrict__ ev = evid + csr * P.V;

        // ---- Collect: deepest level first
        double m = 1.0;
        int ex = 0;  // sums of a few thousand binary exponents: far inside int32
        for (int i = 0; i < P.nc; ++i) {
            const JtMClique q = cl[collect[i]];
            const EvMask mk = make_mask(aux + q.vars_off, q.nv, ev);
            const uint64_t *__restrict__ dg = dig + q.dig_off;
            const double *__restrict__ iv = initv + q.iv_off;
            const int32_t *__restrict__ rec = aux + q.child_off;
            int esum = 0;
            for (int j = 0; j < q.k; ++j) esum += (int)__double_as_longlong(ROW(rec[4 * j + 2]));
            if (q.parent >= 0) {
                // up(e) = e % Ts: kU neighbouring separator entries at a time, each with its running
                // maximum in a register, over the entries e = s (mod Ts) in ascending order
                const int Ts = q.up_Ts, per = q.T / Ts;
                double mx = 0.0;
                for (int s0 = 0; s0 < Ts; s0 += kU) {
                    const int n = Ts - s0 < kU ? Ts - s0 : kU;
                    double acc[kU];
#pragma unroll
                    for (int u = 0; u < kU; ++u) acc[u] = 0.0;
                    for (int qi = 0; qi < per; ++qi) {
                        double v[kU];
                        bool cons[kU];
                        entry_values(S, iv, aux, rec, q.k, dg, q.nw, mk, qi * Ts + s0, 1, n, v, cons);
#pragma unroll
                        for (int u = 0; u < kU; ++u) acc[u] = (cons[u] && v[u] > acc[u]) ? v[u] : acc[u];
                    }
#pragma unroll
                    for (int u = 0; u < kU; ++u)
                        if (u < n) {
                            ROW(q.up_row + s0 + u) = acc[u];
                            mx = acc[u] > mx ? acc[u] : mx;
                        }
                }
                int k = 0;
                (void)frexp(mx, &k);
                for (int s = 0; s < Ts; ++s) ROW(q.up_row + s) = ldexp(ROW(q.up_row + s), -k);
                ROW(q.up_exp_row) = __longlong_as_double((long long)k + esum);
            } else {
                double best = -1.0;
                int es = -1;
                for (int e0 = 0; e0 < q.T; e0 += kU) {
                    double v[kU];
                    bool cons[kU];
                    entry_values(S, iv, aux, rec, q.k, dg, q.nw, mk, e0, 1, q.T - e0 < kU ? q.T - e0 : kU, v, cons);
#pragma unroll
                    for (int u = 0; u < kU; ++u)  // ascending e, strict '>'
                        if (cons[u] && v[u] > best) best = v[u], es = e0 + u;
                }
                if (es < 0) best = 0.0, es = 0;  // guard: validated evidence leaves an entry unmasked
                ROW(q.estar_row) = __longlong_as_double((long long)es);
                int k = 0;
                const double f = frexp(best, &k);
                ex += k + esum;
                m = frexp(m * f, &k);
                ex += k;
            }
        }
        if (act) {
            value[2 * cs] = m, value[2 * cs + 1] = (double)ex;
            if (dbg_msg)
                for (int r = 0; r < P.msg_rows; ++r) dbg_msg[cs * P.msg_rows + r] = ROW(r);
            if (dbg_exp)
                for (int s = 0; s < P.nsep; ++s) dbg_exp[cs * P.nsep + s] = (int32_t)__double_as_longlong(ROW(P.msg_rows + s));
        }

        // ---- back-trace: levels ascending; the entries scanned are this lane's own
        for (int i = 0; i < P.nc; ++i) {
            const JtMClique q = cl[trace[i]];
            const uint64_t *__restrict__ dg = dig + q.dig_off;
            int es;
            if (q.parent >= 0) {
                const EvMask mk = make_mask(aux + q.vars_off, q.nv, ev);
                const double *__restrict__ iv = initv + q.iv_off;
                const int32_t *__restrict__ rec = aux + q.child_off;
                const int ep = (int)__double_as_longlong(ROW(estar0 + q.parent));
                const int ss = aux[q.parent_map_off + ep];
                const int Ts = q.up_Ts, per = q.T / Ts;
                double best = -1.0;
                es = -1;
                for (int q0 = 0; q0 < per; q0 += kU) {
                    double v[kU];
                    bool cons[kU];
                    entry_values(S, iv, aux, rec, q.k, dg, q.nw, mk, q0 * Ts + ss, Ts, per - q0 < kU ? per - q0 : kU, v, cons);
#pragma unroll
                    for (int u = 0; u < kU; ++u)  // ascending e, strict '>'
                        if (cons[u] && v[u] > best) best = v[u], es = (q0 + u) * Ts + ss;
                }
                if (es < 0) es = ss;
                ROW(q.estar_row) = __longlong_as_double((long long)es);
            } else {
                es = (int)__double_as_longlong(ROW(q.estar_row));
            }
            if (act) {
                const int32_t *__restrict__ vars = aux + q.vars_off;
                for (int j = 0; j < q.nown; ++j)
                    assign[cs * P.V + vars[j]] = (int8_t)((dg[(size_t)es * q.nw + (j >> 3)] >> (8 * (j & 7))) & 0xFF);
            }
        }
    }
}

}  // namespace

extern "C" hipError_t fbn_mpe_launch(const JtMpeArgs *a, hipStream_t stream) {
    JtMParams P;
    P.ncases = a->ncases, P.store_rows = a->store_rows;
    P.nc = a->nc, P.V = a->V, P.msg_rows = a->msg_rows, P.nsep = a->nsep;
    hipLaunchKernelGGL(jt_mpe_kernel, dim3(a->grid), dim3(64), 0, stream, a->cl, a->aux, a->initv, a->dig, a->collect,
                       a->trace, a->evid, a->assign, a->value, a->dbg_msg, a->dbg_exp, a->store, P);
    return hipGetLastError();
}
