// ginf.hip -- batched exact inference in a linear-Gaussian network on the device: every case conditions the
// resident joint N(mu, Sigma) on its own observed set (include/fastbn.h states the model; the per-element
// arithmetic is ginf_model.h's, which the host twin evaluates too, so the results are its bits).
//
// One workgroup of 256 threads per case, a persistent grid striding over the cases.  Per case, all in LDS:
//  * the index lists E (observed, ascending) and U (unobserved, ascending) as 16-bit entries: 256 variables
//    at a time, a ballot over the NaN mask per wave, the four waves' counts exchanged through LDS and
//    prefix-summed by every thread; no atomics.
//  * Sigma_EE gathered into the packed lower triangle L, delta = x_E - mu_E into a.
//  * the factorisation in place, column by column: thread t owns row t (t < m) and thread m owns delta as one
//    more row below L, so L a = delta is solved by the same steps.  In step j a thread forms its row's entry j
//    (its k loop ascending over its own row and the finished row j, both in LDS) and adds the entry's square
//    to a running sum in a register; the thread of row j + 1 then has that row's whole sum and writes d_{j+1}
//    and L_{j+1,j+1} = sqrt(d_{j+1}) before the step's barrier.  One barrier per column.
//  * the unobserved variables in tiles of T lanes, one variable per lane: Sigma[e_i][u] is read along row
//    e_i, so neighbouring lanes read neighbouring doubles; the lane's y lies in LDS as y[i][lane] (its bank
//    depends on the lane alone) and L_ik is the same address for every lane, a broadcast.  The solve runs in
//    place over y with y . a and y . y accumulated beside it.  No barrier: a lane touches its own column.
//    T is the largest multiple of 64 up to 256 for which y fits beside L in the launch's LDS
//    (fbn_ginf_tile): 64 at m = 128, 256 for small m.
// The fp64 matrix instructions are not used: their accumulation order cannot be restated on the host.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ginf_model.h"
#include "launchers.h"

namespace {

__device__ __forceinline__ void fill_nan(const GinfArgs &A, long long c, int t) {
    const double nan = __builtin_nan("");
    for (int v = t; v < A.n; v += 256) {
        if (A.mean) A.mean[c * A.n + v] = nan;
        if (A.var) A.var[c * A.n + v] = nan;
    }
    if (t == 0 && A.logp) A.logp[c] = nan;
}

__global__ __launch_bounds__(256) void ginf_cases(GinfArgs A) {
    extern __shared__ double smem[];
    const int n = A.n, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    // fbn_ginf_lds_fixed's plan
    double *s_a = smem, *s_d = smem + kGinfMaxObs;
    uint16_t *s_E = reinterpret_cast<uint16_t *>(smem + 2 * kGinfMaxObs);
    int *s_cnt = reinterpret_cast<int *>(s_E + kGinfMaxObs);  // [2][2][4]: chunk parity, observed / not, wave
    int *s_flag = s_cnt + 16;
    uint16_t *s_U = reinterpret_cast<uint16_t *>(s_flag + 4);
    double *s_L = reinterpret_cast<double *>(reinterpret_cast<char *>(smem) + fbn_ginf_lds_fixed(n));

    for (long long c = blockIdx.x; c < A.ncases; c += gridDim.x) {
        __syncthreads();  // the previous case is done with the LDS
        const double *x = A.ev + c * n;
        if (t == 0) s_flag[0] = 0;
        int m = 0, nu = 0;
        for (int c0 = 0, it = 0; c0 < n; c0 += 256, ++it) {
            const int v = c0 + t;
            const double xv = v < n ? x[v] : 0.0;
            const bool obs = v < n && xv == xv, un = v < n && xv != xv;
            const unsigned long long bo = __ballot(obs), bu = __ballot(un);
            int *cnt = s_cnt + (it & 1) * 8;
            if (lane == 0) cnt[wave] = __popcll(bo), cnt[4 + wave] = __popcll(bu);
            __syncthreads();
            int po = m, pu = nu;
            for (int w = 0; w < 4; ++w) {
                if (w < wave) po += cnt[w], pu += cnt[4 + w];
                m += cnt[w], nu += cnt[4 + w];
            }
            const unsigned long long below = (1ull << lane) - 1ull;
            po += __popcll(bo & below), pu += __popcll(bu & below);
            if (obs && po < kGinfMaxObs) s_E[po] = (uint16_t)v;
            if (un) s_U[pu] = (uint16_t)v;
        }
        __syncthreads();
        const int T = m <= kGinfMaxObs ? fbn_ginf_tile(A.lds_bytes, n, m) : 0;
        if (T < 64) {  // refused on the host before the launch; never indexed with here
            fill_nan(A, c, t);
            continue;
        }

        for (int i = t >> 7, j = t & 127; i < m; i += 2)
            if (j <= i) s_L[fbn_ginf_tri(i, j)] = A.Sigma[(long long)s_E[i] * n + s_E[j]];
        if (t < m) s_a[t] = x[s_E[t]] - A.mu[s_E[t]];
        __syncthreads();

        const bool rowL = t < m, rowA = t == m;
        double *row = rowL ? s_L + fbn_ginf_tri(t, 0) : s_a;
        const double sigma_tt = rowL ? row[t] : 0.0;
        double sq = 0.0;
        bool deg = false;
        if (t == 0 && m > 0) {
            const double d = fbn_ginf_diag(sigma_tt, sq, &deg);
            s_d[0] = d;
            row[0] = sqrt(d);
        }
        __syncthreads();
        for (int j = 0; j < m; ++j) {
            if ((rowL && t > j) || rowA) {
                const double *Lj = s_L + fbn_ginf_tri(j, 0);
                const double l = fbn_ginf_elim(row[j], row, 1, Lj, 1, j, Lj[j]);
                row[j] = l;
                sq = fbn_ginf_more(sq, l, l);
                if (t == j + 1 && rowL) {
                    const double d = fbn_ginf_diag(sigma_tt, sq, &deg);
                    s_d[t] = d;
                    row[t] = sqrt(d);
                }
            }
            if (deg) s_flag[0] = 1;
            __syncthreads();
        }
        if (s_flag[0]) {
            fill_nan(A, c, t);
            continue;
        }
        if (rowA && A.logp) A.logp[c] = fbn_ginf_logp(m, s_d, sq);
        if (!A.mean && !A.var) continue;
        if (rowL) {
            const int v = s_E[t];
            if (A.mean) A.mean[c * n + v] = x[v];
            if (A.var) A.var[c * n + v] = 0.0;
        }
        double *s_y = s_L + fbn_ginf_tri(m, 0);
        for (int ub = 0; ub < nu; ub += T) {
            if (t >= T || ub + t >= nu) continue;
            const int u = s_U[ub + t];
            double *y = s_y + t;
            for (int i = 0; i < m; ++i) y[i * T] = A.Sigma[(long long)s_E[i] * n + u];
            double ya = 0.0, yy = 0.0;
            for (int i = 0; i < m; ++i) {
                const double *Li = s_L + fbn_ginf_tri(i, 0);
                const double yi = fbn_ginf_elim(y[i * T], Li, 1, y, T, i, Li[i]);
                y[i * T] = yi;
                ya = fbn_ginf_more(ya, yi, s_a[i]);
                yy = fbn_ginf_more(yy, yi, yi);
            }
            double pm, pv;
            fbn_ginf_posterior(A.mu[u], A.Sigma[(long long)u * n + u], ya, yy, &pm, &pv);
            if (A.mean) A.mean[c * n + u] = pm;
            if (A.var) A.var[c * n + u] = pv;
        }
    }
}

// word[0] = the smallest flat index of an infinite value, word[1] = ~0 - the largest observed count; both
// start as ~0
__global__ __launch_bounds__(256) void ginf_check(const double *ev, long long ncases, int n, unsigned long long *word) {
    __shared__ int s_m[4];
    const int t = threadIdx.x;
    for (long long c = blockIdx.x; c < ncases; c += gridDim.x) {
        int m = 0;
        for (int v = t; v < n; v += 256) {
            const double xv = ev[c * n + v];
            if (xv != xv) continue;
            ++m;
            if (xv - xv != 0.0) atomicMin(word, (unsigned long long)(c * n + v));
        }
        for (int off = 32; off > 0; off >>= 1) m += __shfl_down(m, off);
        __syncthreads();
        if ((t & 63) == 0) s_m[t >> 6] = m;
        __syncthreads();
        if (t == 0) atomicMin(word + 1, ~0ull - (unsigned long long)(s_m[0] + s_m[1] + s_m[2] + s_m[3]));
    }
}

}  // namespace

extern "C" hipError_t fbn_ginf_check_launch(const double *ev, long long ncases, int n, unsigned long long *word, int grid,
                                            hipStream_t s) {
    if (ncases <= 0) return hipSuccess;
    if (n < 1 || grid < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ginf_check, dim3((unsigned)grid), dim3(256), 0, s, ev, ncases, n, word);
    return hipGetLastError();
}

// a->lds_bytes = fbn_ginf_lds_bytes(n, the batch's largest observed count <= kGinfMaxObs)
extern "C" hipError_t fbn_ginf_launch(const GinfArgs *a, int grid, hipStream_t s) {
    if (a->ncases <= 0) return hipSuccess;
    if (a->n < 1 || a->n > kGinfMaxVars || grid < 1 || a->lds_bytes < fbn_ginf_lds_fixed(a->n) || a->lds_bytes > 160 * 1024)
        return hipErrorInvalidValue;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(ginf_cases),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, a->lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ginf_cases, dim3((unsigned)grid), dim3(256), (size_t)a->lds_bytes, s, *a);
    return hipGetLastError();
}
