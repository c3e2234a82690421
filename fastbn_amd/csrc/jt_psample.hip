// jt_psample.hip -- exact posterior sampling on gfx950: the sum-product Collect and the sampled back-trace
// of include/fastbn.h (above fbn_psample_create) over the program of jt_mpe_program.h.
//
// A persistent-wave kernel of jt_mpe_kernel's family: 64-lane one-wave workgroups, a per-wave store
// [row][64] in global memory recycled across units, no atomics, no LDS.  What differs is the unit of work and
// the draw phase.
//
// Unit = (64-case block b, chunk k of A.chunk samples).  Collect runs once per unit with lane = case, so
// every loop bound, index map, initial potential and digit word is wave-uniform and comes as a scalar
// load; a tail lane runs a copy of the last case.  It leaves the block's messages in the store, case j of
// the block in column j.  A Collect is thereby amortised over the chunk's draws; with few cases the host
// cuts S into more chunks so that the units still fill the chip, at the price of one more Collect each.
//
// Draw phase: the unit's items are B * Cn (B real cases of the block, Cn samples of the chunk); lane l
// takes items l, l + 64, ...; item i is case i % B, sample k * chunk + i / B.  With B = 64 that is lane =
// case looping over the chunk; with one case all 64 lanes draw for it, each reading store column `case`
// instead of column `lane`.  The entries a draw visits depend on its parent's choice, so maps, digits,
// potentials and message rows are per-lane gathers here (as in MPE's back-trace) and the remap costs nothing
// extra.  Because a lane now reads rows another lane wrote, a workgroup-scope release / acquire fence stands
// between Collect and the draws, and again before the next unit's Collect overwrites the rows.
//
// A draw's dependent chain is a gather, a multiply, an add and a compare per candidate: latency-bound.  A
// lane keeps U independent draws in flight (its items i, i + 64, ..., i + 64 (U - 1)), their chains
// interleaved; their chosen entries live in U e* rows per clique, column = lane.  Z is formed by a first
// pass over the slice, the choice by a second one (the stated arithmetic, no own-exponent row).
//
// Numerics: the host twin's operations in the host twin's order (-ffp-contract=off: no FMA) -- the same
// bytes, whatever the grid, the chunk and the batch.
//
// Resources (gfx950, U = 4): 167 VGPRs, 106 SGPRs, no scratch.  fp64 and integer code only: the Makefile's
// -packed-fp32-ops guard for this file changes nothing in it today.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jt_psample_program.h"
#include "launchers.h"

namespace {

#define ROW(r) S[(size_t)(r) * 64]

// evidence pattern of a clique for one case
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

// Collect: v(e) of the kC wave-uniform entries e0 + u (u < n; the rest repeat e0 and are reported masked),
// kC independent chains as in jt_em.hip.  S: the wave's store at this lane's column.
constexpr int kC = 4;
__device__ __forceinline__ void collect_values(const double *S, const JtMClique &q, const int32_t *__restrict__ aux,
                                               const double *__restrict__ initv, const uint64_t *__restrict__ dig,
                                               const EvMask &mk, int e0, int n, double (&v)[kC], bool (&cons)[kC]) {
    const double *__restrict__ iv = initv + q.iv_off;
    const uint64_t *__restrict__ dg = dig + q.dig_off;
    const int32_t *__restrict__ rec = aux + q.child_off;
    int e[kC];
#pragma unroll
    for (int u = 0; u < kC; ++u) {
        e[u] = e0 + (u < n ? u : 0);
        v[u] = iv[e[u]];
        cons[u] = u < n && mk.consistent(dg + (size_t)e[u] * q.nw, q.nw);
    }
    for (int j = 0; j < q.k; ++j) {
        const int mo = rec[4 * j], row = rec[4 * j + 1];
#pragma unroll
        for (int u = 0; u < kC; ++u) v[u] = v[u] * ROW(row + aux[mo + e[u]]);
    }
}

// Draw: v(e[u]) of U per-lane entries, draw u reading store column col[u] of the wave's store W
template <int U>
__device__ __forceinline__ void draw_values(const double *W, const int (&col)[U], const JtMClique &q,
                                            const int32_t *__restrict__ aux, const double *__restrict__ initv,
                                            const uint64_t *__restrict__ dig, const EvMask (&mk)[U], const int (&e)[U],
                                            double (&v)[U], bool (&cons)[U]) {
    const double *__restrict__ iv = initv + q.iv_off;
    const uint64_t *__restrict__ dg = dig + q.dig_off;
    const int32_t *__restrict__ rec = aux + q.child_off;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        v[u] = iv[e[u]];
        cons[u] = mk[u].consistent(dg + (size_t)e[u] * q.nw, q.nw);
    }
    for (int j = 0; j < q.k; ++j) {
        const int mo = rec[4 * j], row = rec[4 * j + 1];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = v[u] * W[(size_t)(row + aux[mo + e[u]]) * 64 + col[u]];
    }
}

__device__ __forceinline__ void unit_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <int U>
__global__ __launch_bounds__(64) void jt_psample_kernel(const JtPsampleArgs A) {
    const int lane = threadIdx.x;
    double *W = A.store + (size_t)blockIdx.x * (size_t)A.store_rows * 64;  // the wave's store
    double *S = W + lane;
    const int estar0 = A.msg_rows + A.nsep;
    const long long nchunk = (A.S + A.chunk - 1) / A.chunk;
    const long long units = ((A.ncases + 63) / 64) * nchunk;

    for (long long unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const long long blk = unit / nchunk, ck = unit - blk * nchunk;
        {
            // ---- Collect, lane = case: deepest level first (jt_em.hip's, to the operation)
            const long long cs = blk * 64 + lane;
            const bool act = cs < A.ncases;
            const long long csr = act ? cs : A.ncases - 1;  // a tail lane runs on a copy of the last case
            const int8_t *__restrict__ ev = A.evid + csr * A.V;
            double m = 1.0;
            int ex = 0;
            for (int i = 0; i < A.nc; ++i) {
                const JtMClique q = A.cl[A.collect[i]];
                const EvMask mk = make_mask(A.aux + q.vars_off, q.nv, ev);
                const int32_t *__restrict__ rec = A.aux + q.child_off;
                int esum = 0;
                for (int j = 0; j < q.k; ++j) esum += (int)__double_as_longlong(ROW(rec[4 * j + 2]));
                if (q.parent >= 0) {
                    // up(e) = e % Ts: the entries of separator entry s are s, s + Ts, ... ascending
                    const int Ts = q.up_Ts, per = q.T / Ts;
                    double mx = 0.0;
                    for (int s0 = 0; s0 < Ts; s0 += kC) {
                        const int n = Ts - s0 < kC ? Ts - s0 : kC;
                        double acc[kC];
#pragma unroll
                        for (int u = 0; u < kC; ++u) acc[u] = 0.0;
                        for (int qi = 0; qi < per; ++qi) {
                            double v[kC];
                            bool cons[kC];
                            collect_values(S, q, A.aux, A.initv, A.dig, mk, qi * Ts + s0, n, v, cons);
#pragma unroll
                            for (int u = 0; u < kC; ++u) acc[u] = cons[u] ? acc[u] + v[u] : acc[u];
                        }
#pragma unroll
                        for (int u = 0; u < kC; ++u)
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
                    double sum = 0.0;
                    for (int e0 = 0; e0 < q.T; e0 += kC) {
                        double v[kC];
                        bool cons[kC];
                        collect_values(S, q, A.aux, A.initv, A.dig, mk, e0, q.T - e0 < kC ? q.T - e0 : kC, v, cons);
#pragma unroll
                        for (int u = 0; u < kC; ++u) sum = cons[u] ? sum + v[u] : sum;  // ascending e
                    }
                    int k = 0;
                    const double f = frexp(sum, &k);
                    ex += k + esum;
                    m = frexp(m * f, &k);
                    ex += k;
                }
            }
            if (act && ck == 0) A.value[2 * cs] = m, A.value[2 * cs + 1] = (double)ex;  // every chunk has the same
        }
        unit_fence();  // the draws read message rows that other lanes of the wave wrote

        // ---- draws, lane = item: item i is case i % B of the block, sample s0 + i / B
        const int B = (int)(A.ncases - blk * 64 < 64 ? A.ncases - blk * 64 : 64);
        const long long s0 = ck * A.chunk;
        const long long items = (long long)B * (A.S - s0 < A.chunk ? A.S - s0 : A.chunk);
        for (long long i0 = lane; i0 < items; i0 += 64 * U) {
            int col[U];
            bool ok[U];
            long long out[U];  // the draw's row of A.samples
            const int8_t *ev[U];
            fbn::U128 st[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                long long it = i0 + 64 * u;
                ok[u] = it < items;  // a draw past the end repeats item i0 and stores no sample
                it = ok[u] ? it : i0;
                col[u] = (int)(it % B);
                const long long cs = blk * 64 + col[u], smp = s0 + it / B;
                ev[u] = A.evid + cs * A.V;
                out[u] = (cs * A.S + smp) * A.V;
                st[u] = fbn::PcgJumpTo(A.state, ((uint64_t)(A.case0 + cs) * (uint64_t)A.S + (uint64_t)smp) * (uint64_t)A.nc,
                                       A.jump);
            }
            for (int i = 0; i < A.nc; ++i) {  // levels ascending
                const int c = A.trace[i];
                const JtMClique q = A.cl[c];
                const uint64_t *__restrict__ dg = A.dig + q.dig_off;
                const int stride = q.parent >= 0 ? q.up_Ts : 1;
                const int n = q.T / stride;
                EvMask mk[U];
                int first[U], es[U], last[U];
                double Z[U], t[U], run[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    mk[u] = make_mask(A.aux + q.vars_off, q.nv, ev[u]);
                    st[u] = fbn::PcgStep(st[u], A.inc);  // every clique takes one draw
                    first[u] = 0;
                    if (q.parent >= 0)
                        first[u] = A.aux[q.parent_map_off + (int)__double_as_longlong(ROW(estar0 + u * A.nc + q.parent))];
                    Z[u] = 0.0, run[u] = 0.0, es[u] = -1, last[u] = -1;
                }
                for (int qi = 0; qi < n; ++qi) {  // Z: the candidates' sum, ascending
                    int e[U];
                    double v[U];
                    bool cons[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) e[u] = first[u] + qi * stride;
                    draw_values<U>(W, col, q, A.aux, A.initv, A.dig, mk, e, v, cons);
#pragma unroll
                    for (int u = 0; u < U; ++u) Z[u] = cons[u] ? Z[u] + v[u] : Z[u];
                }
#pragma unroll
                for (int u = 0; u < U; ++u) t[u] = fbn::PcgDouble(fbn::PcgOutput(st[u])) * Z[u];
                for (int qi = 0; qi < n; ++qi) {  // the first candidate whose running sum is > t
                    int e[U];
                    double v[U];
                    bool cons[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) e[u] = first[u] + qi * stride;
                    draw_values<U>(W, col, q, A.aux, A.initv, A.dig, mk, e, v, cons);
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        run[u] = cons[u] ? run[u] + v[u] : run[u];
                        es[u] = (cons[u] && es[u] < 0 && run[u] > t[u]) ? e[u] : es[u];
                        last[u] = (cons[u] && v[u] > 0.0) ? e[u] : last[u];
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    es[u] = es[u] < 0 ? last[u] : es[u];   // u * Z rounded up to Z
                    es[u] = es[u] < 0 ? first[u] : es[u];  // guard: a case of value 0
                    ROW(estar0 + u * A.nc + c) = __longlong_as_double((long long)es[u]);
                    if (ok[u]) {
                        const int32_t *__restrict__ vars = A.aux + q.vars_off;
                        for (int j = 0; j < q.nown; ++j)
                            A.samples[out[u] + vars[j]] =
                                (int8_t)((dg[(size_t)es[u] * q.nw + (j >> 3)] >> (8 * (j & 7))) & 0xFF);
                    }
                }
            }
        }
        unit_fence();  // the next unit's Collect overwrites rows other lanes may still be reading
    }
}

}  // namespace

extern "C" hipError_t fbn_psample_launch(const JtPsampleArgs *a, hipStream_t stream) {
    hipLaunchKernelGGL(jt_psample_kernel<kPsampleU>, dim3(a->grid), dim3(64), 0, stream, *a);
    return hipGetLastError();
}
