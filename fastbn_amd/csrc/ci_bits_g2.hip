// ci_bits_g2.hip -- G^2, df, p and the decision of tests with at most one conditioning variable from
// their 64-slot count records (ci_bits_count.hip, ci_bits_gram.hip), gfx950.
//
// Marginals, the adjusted df and G^2 in the reference's operation order (one running G^2 sum over
// z -> x -> y: ComputeGSquareXY / XYZ, src/IndependenceTest.cpp:65-155, 295-364), the arithmetic and
// the decision being ci_g2.h's, as in ci_kernels.hip and pc_small.hip, so the kernels agree bit for bit.
// Two passes with the same item decode and decision tail and different middles: one lane per test
// (ci_bits_g2, large launches: no idle lanes in the log / incomplete-gamma code) and four lanes per
// test (ci_bits_g2q, launches too small to fill the chip with a lane each).  With no p output and a
// decision band, p is only evaluated for G^2 inside the band.  The margin log is reduced per wave
// (one atomic pair per wave, not per test).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ci_bits.h"
#include "ci_g2.h"
#include "launchers.h"

namespace {

// test t of the batch: its state counts and its count record (not live: a padding lane's 1 x 1 x 1
// test on record 0)
struct G2Item {
    int dx, dy, dimz, dxy;
    const int32_t *hz;
};
template <int D>
__device__ __forceinline__ G2Item g2_item(const CiG2Args &A, long long t, bool live) {
    int px = 0, py = 0, pz = 0;
    if (live) {
        if (D == 0 && !A.items) pair_of(A.t0 + t, A.nvars, px, py);
        else px = A.items[(2 + D) * t], py = A.items[(2 + D) * t + 1];
        if (D == 1) pz = A.items[3 * t + 2];
    }
    G2Item it;
    it.dx = live ? A.dims[px] : 1, it.dy = live ? A.dims[py] : 1;
    it.dimz = D == 1 && live ? A.dims[pz] : 1;
    it.dxy = it.dx * it.dy;
    it.hz = A.counts + (live ? t : 0) * kBitsCells;
    return it;
}

__device__ __forceinline__ G2Decision g2_decide(const CiG2Args &A, double g2, int df) {
    return fbn_g2_decide(g2, df, A.alpha, A.band, A.nband, A.p != nullptr);
}

// the outputs of test t, by the one lane that owns it
__device__ __forceinline__ void g2_write(const CiG2Args &A, long long t, const G2Item &it, double g2, int df,
                                         const G2Decision &r) {
    if (A.g2) A.g2[t] = g2;
    A.df[t] = df;
    if (A.p) A.p[t] = r.p;
    A.indep[t] = r.ind;
    if (A.counts0 && t == 0)
        for (int c = 0; c < it.dimz * it.dxy; ++c) A.counts0[c] = it.hz[c];
}

// one lane per test.  (Measured and not kept: 16 lanes per test with the terms in LDS, 10x slower
// at level 0; per-class instantiations with the table in registers, 1.7x slower.)
template <int D>
__global__ __launch_bounds__(256) void ci_bits_g2(CiG2Args A) {
    const long long n = A.n_dev ? *A.n_dev : A.n;
    const long long stride = (long long)gridDim.x * 256;
    // wave-uniform trip count (the margin reduction below is a whole-wave operation)
    for (long long wb = (long long)blockIdx.x * 256 + (threadIdx.x & ~63); wb < n; wb += stride) {
        const long long t = wb + (threadIdx.x & 63);
        unsigned long long mbits = kNoMargin;
        bool near = false;
        if (t < n) {
            const G2Item it = g2_item<D>(A, t, true);
            const int dx = it.dx, dy = it.dy, dimz = it.dimz, dxy = it.dxy;
            const int32_t *hz = it.hz;
            // the record unpacked into a fixed KZ x 4 x 4 register table (absent cells 0): every load
            // is independent (one memory latency per test, not one per loop step) and every index
            // below is static.  Absent rows / columns / z values have zero counts, so they add
            // nothing to df (max(0, 1) - 1 = 0) or G^2 (their terms are skipped) -- the sums are the
            // reference's over the real table, in its order.
            constexpr int KZ = D == 1 ? 4 : 1;
            int h[KZ][4][4];
#pragma unroll
            for (int k = 0; k < KZ; ++k)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool in = k < dimz && i < dx && j < dy;
                        const int v = hz[in ? k * dxy + i * dy + j : 0];
                        h[k][i][j] = in ? v : 0;
                    }
            // one running sum over z -> x -> y, exactly the reference's loop (no per-z partials)
            double g2 = 0.0;
            int df = 0;
#pragma unroll
            for (int k = 0; k < KZ; ++k) {
                int ni[4], nj[4], alx = 0, aly = 0;
                long total = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    ni[i] = (h[k][i][0] + h[k][i][1]) + (h[k][i][2] + h[k][i][3]);
                    alx += ni[i] > 0;
                    total += ni[i];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    nj[j] = (h[k][0][j] + h[k][1][j]) + (h[k][2][j] + h[k][3][j]);
                    aly += nj[j] > 0;
                }
                df += fbn_g2_slice_df(alx, aly);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const long sum_row = ni[i];
                    if (total == 0 || sum_row == 0) continue;
                    // the row's four terms side by side (independent latency chains; absent cells on
                    // placeholder operands), then the present ones added in order
                    double tm[4];
                    bool on[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        on[j] = nj[j] != 0 && h[k][i][j] != 0;
                        tm[j] = fbn_g2_term_nz(on[j] ? h[k][i][j] : 1, sum_row, on[j] ? nj[j] : 1, total);
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (on[j]) g2 += tm[j];
                }
            }
            const G2Decision r = g2_decide(A, g2, df);
            g2_write(A, t, it, g2, df, r);
            mbits = fbn_margin_bits(r.margin);
            near = fbn_margin_near(r.margin);
        }
        if (A.stats) fbn_margin_log_wave(A.stats, mbits, near, threadIdx.x & 63);
    }
}

// four lanes per test.  Lane q of a test's group owns z value q (D = 1: a 4 x 4 slice) or x value q
// (D = 0: a row of 4): it unpacks its part of the 256-B count record into a zero-padded register
// table (independent loads, static indices; absent rows, columns and z values add nothing to df or
// G^2), evaluates its terms -- the costly part, a division chain and a log each -- in parallel with
// the other three lanes, and then the four lanes add their terms into the one running sum in turn.
constexpr int kG2Lanes = 4;
constexpr int kG2TestsPerBlock = 256 / kG2Lanes;
template <int D>
__global__ __launch_bounds__(256) void ci_bits_g2q(CiG2Args A) {
    const long long n = A.n_dev ? *A.n_dev : A.n;
    const int lane = threadIdx.x & 63, q = lane & (kG2Lanes - 1), g0 = lane & ~(kG2Lanes - 1);
    const long long stride = (long long)gridDim.x * kG2TestsPerBlock;
    // wave-uniform trip count (the shuffles and the margin reduction are whole-wave operations)
    for (long long wb = (long long)blockIdx.x * kG2TestsPerBlock + (threadIdx.x >> 6) * (64 / kG2Lanes); wb < n;
         wb += stride) {
        const long long t = wb + lane / kG2Lanes;
        const bool live = t < n;
        const G2Item it = g2_item<D>(A, t, live);
        const int dx = it.dx, dy = it.dy, dimz = it.dimz, dxy = it.dxy;
        const int32_t *hz = it.hz;
        constexpr int NR = D == 1 ? 4 : 1;  // rows this lane owns
        int h[NR][4];
#pragma unroll
        for (int r = 0; r < NR; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = D == 1 ? q : 0, i = D == 1 ? r : q;
                const bool in = live && k < dimz && i < dx && j < dy;
                const int v = hz[in ? k * dxy + i * dy + j : 0];
                h[r][j] = in ? v : 0;
            }
        // this lane's slice (D = 1) or the test's only slice (D = 0): marginals, total, df
        int ni[NR], nj[4], df;
        long total = 0;
        {
            int alx = 0, aly = 0;
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                ni[r] = (h[r][0] + h[r][1]) + (h[r][2] + h[r][3]);
                alx += ni[r] > 0;
                total += ni[r];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int c = 0;
#pragma unroll
                for (int r = 0; r < NR; ++r) c += h[r][j];
                nj[j] = c;
            }
            if (D == 0) {  // the slice's rows are spread over the group
#pragma unroll
                for (int o = 1; o < kG2Lanes; o <<= 1) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) nj[j] += __shfl_xor(nj[j], o);
                    alx += __shfl_xor(alx, o);
                    total += __shfl_xor(total, o);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) aly += nj[j] > 0;
            df = fbn_g2_slice_df(alx, aly);
            if (D == 1)
#pragma unroll
                for (int o = 1; o < kG2Lanes; o <<= 1) df += __shfl_xor(df, o);
        }
        // this lane's terms, side by side (independent latency chains; absent cells on placeholder operands)
        double tm[NR][4];
        bool on[NR][4];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const long sum_row = ni[r];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                on[r][j] = total != 0 && sum_row != 0 && nj[j] != 0 && h[r][j] != 0;
                tm[r][j] = 0.0;
            }
            if (total != 0 && sum_row != 0) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    tm[r][j] = fbn_g2_term_nz(on[r][j] ? h[r][j] : 1, sum_row, on[r][j] ? nj[j] : 1, total);
            }
        }
        // the running sum, lane 0's cells first: z (D = 1) or x (D = 0) is the group's outer digit
        double g2 = 0.0;
#pragma unroll
        for (int s = 0; s < kG2Lanes; ++s) {
            if (q == s)
#pragma unroll
                for (int r = 0; r < NR; ++r)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (on[r][j]) g2 += tm[r][j];
            g2 = __shfl(g2, g0 + s);
        }
        unsigned long long mbits = kNoMargin;
        bool near = false;
        if (live) {
            const G2Decision r = g2_decide(A, g2, df);
            if (q == 0) {
                g2_write(A, t, it, g2, df, r);
                mbits = fbn_margin_bits(r.margin);
                near = fbn_margin_near(r.margin);
            }
        }
        if (A.stats) fbn_margin_log_wave(A.stats, mbits, near, lane);
    }
}

// G^2 = 2N I(X;Y) of every pair of the complete graph from its level-0 table (pairtab, 16 counts:
// N[a][b] at a * dy + b for x < y), one thread per pair -- the level-1 information screen's input
// (ci_l1.hip) when level 0's own G^2 values are not all on this device (a rank of the distributed
// session ran part of level 0 and imported the others' tables).  The screen reads pairs that need
// not be edges: (y, z) for z a neighbour of x.
__global__ __launch_bounds__(256) void ci_pair_g2(const int32_t *__restrict__ pairtab, const int32_t *__restrict__ dims,
                                                  int nv, long long P, double *__restrict__ g2) {
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < P; t += (long long)gridDim.x * 256) {
        int x, y;
        pair_of(t, nv, x, y);
        const int dx = dims[x], dy = dims[y];
        const int32_t *T = pairtab + 16 * t;
        double r[4] = {0, 0, 0, 0}, c[4] = {0, 0, 0, 0}, n = 0.0;
        for (int a = 0; a < dx; ++a)  // (dims <= 4 on this path)
            for (int b = 0; b < dy; ++b) {
                const double w = T[a * dy + b];
                r[a] += w, c[b] += w, n += w;
            }
        double acc = 0.0;
        for (int a = 0; a < dx; ++a)
            for (int b = 0; b < dy; ++b) {
                const double w = T[a * dy + b];
                if (w > 0.0) acc += w * log(w * n / (r[a] * c[b]));
            }
        g2[t] = 2.0 * acc;
    }
}

}  // namespace

hipError_t fbn::CiG2Launch(const CiG2Args &a, int d, bool quad, int num_cu, hipStream_t s) {
    const long long per = quad ? kG2TestsPerBlock : 256;
    const long long g = (a.n + per - 1) / per, cap = (long long)num_cu * 8;
    const dim3 grid((unsigned)(g < cap ? g : cap));
    if (d == 0) hipLaunchKernelGGL((quad ? ci_bits_g2q<0> : ci_bits_g2<0>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((quad ? ci_bits_g2q<1> : ci_bits_g2<1>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t fbn::CiPairG2Launch(const int32_t *pairtab, const int32_t *dims, int nv, double *g2, hipStream_t s) {
    const long long P = (long long)nv * (nv - 1) / 2, b = (P + 255) / 256;
    hipLaunchKernelGGL(ci_pair_g2, dim3((unsigned)(b < 4096 ? b : 4096)), dim3(256), 0, s, pairtab, dims, nv, P, g2);
    return hipGetLastError();
}
