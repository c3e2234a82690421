// gci_corr.hip -- the correlation matrix of a continuous column store on the gfx950 matrix cores,
// hand-written: the sufficient statistic of the Gaussian conditional-independence test (gci.h).
//
// X is float64 [nvars][N], a variable's samples contiguous.  R = D^-1/2 S D^-1/2 with the centred Gram
// S_ij = sum_s (x_is - mu_i)(x_js - mu_j), in two passes:
//
//  * gci_means: one block per column, every thread a strided partial, then a fixed halving tree in LDS; no
//    atomics.  The block also flags a column that holds a non-finite value.
//  * gci_gram: S on v_mfma_f64_16x16x4_f64.  Output tiles of TM x TM variables (TM = 64 or 32) on or above
//    the diagonal only; split-K over the samples in whole stages of 32, so a small nvars still fills the
//    chip: block = (tile, K-slice).  256 threads = 4 waves (2 x 2), TM/2 x TM/2 per wave = (TM/32)^2
//    accumulator tiles of 16 x 16 (4 doubles per lane each).
//      - A stage is TM variables x 32 samples per panel.  Thread t loads sample t % 32 of rows t / 32 + 8 p
//        (a half-wave reads 256 contiguous bytes of one column), subtracts the row's mean and writes the
//        centred value -- or 0.0 for a row >= nvars or a sample beyond N, so ragged edges are zero-filled
//        after centring and no branch goes around the MFMAs -- to LDS.  Centred data is never stored.
//      - LDS rows are 34 doubles (32 + 2 of padding).  The MFMA's A / B fragment is 16 variables x 4 samples:
//        lane l holds variable l % 16, sample l / 16.  A ds_read_b64 is served per half-wave: rows i = 0..15,
//        k in {0, 1} (or {2, 3}) at double offset 34 i + k = 2 i + k (mod 32): 32 distinct 8-byte bank pairs,
//        no conflict; the staging writes of a half-wave are 32 consecutive doubles of one row, none either.
//      - Two LDS buffers: the next stage's global loads are issued before the current stage's MFMAs and
//        written to the other buffer after them; one barrier per stage.  The fp64 MFMA occupies the matrix
//        pipe for 16 passes, so 2 x (TM/32) fragment reads per (TM/32)^2 MFMAs keep it fed.
//      - A diagonal tile stages one panel and reads both fragments from it.
//      - Each block writes its TM x TM partial to slab[slice][tile]; no atomics.
//  * gci_reduce: one thread per entry on or above the diagonal: the slices' partials summed in slice order,
//    divided by sqrt(S_ii S_jj) (both read from the diagonal tiles' slabs in the same order), written to
//    R[i][j] and R[j][i]; the diagonal is 1.0 exactly, and S_ii goes to var[i] for the zero-variance check.
// For a given tile size and slice count the result is therefore the same bits from run to run.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "launchers.h"

namespace {

constexpr int kStage = 32;       // samples per stage
constexpr int kLd = kStage + 2;  // LDS row stride in doubles (see above)

typedef double v4d __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void gci_means(const double *__restrict__ X, long long N, double *__restrict__ mean,
                                                 int *__restrict__ bad) {
    __shared__ double part[256];
    __shared__ int flag[256];
    const int v = blockIdx.x, t = threadIdx.x;
    const double *x = X + (long long)v * N;
    double s = 0.0;
    int nf = 0;
    for (long long i = t; i < N; i += 256) {
        const double a = x[i];
        nf |= !(a - a == 0.0);  // inf or NaN
        s += a;
    }
    part[t] = s;
    flag[t] = nf;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (t < h) part[t] += part[t + h], flag[t] |= flag[t + h];
        __syncthreads();
    }
    if (t == 0) mean[v] = part[0] / (double)N, bad[v] = flag[0];
}

// tile index -> (I, J), I <= J < T, rows of the upper triangle in order
__device__ __forceinline__ void tile_of(int t, int T, int *I, int *J) {
    int i = 0;
    while (t >= T - i) t -= T - i, ++i;
    *I = i, *J = i + t;
}

template <int TM>
__global__ __launch_bounds__(256) void gci_gram(const double *__restrict__ X, const double *__restrict__ mean, int nvars,
                                                long long N, int T, int nt, int S, long long nstages,
                                                double *__restrict__ slab) {
    constexpr int WT = TM / 2, MT = WT / 16, RP = TM / 8;  // wave tile, MFMA tiles per side, rows per thread
    __shared__ double lds[2][2][TM * kLd];
    const int w = blockIdx.x, split = w / nt, tile = w - split * nt;
    int I, J;
    tile_of(tile, T, &I, &J);
    const bool diag = I == J;
    const long long st0 = split * nstages / S, st1 = (split + 1) * nstages / S;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, wm = wave >> 1, wn = wave & 1;
    const int col = tid & 31, rbase = tid >> 5;

    double ma[RP], mb[RP], ra[RP], rb[RP];
    bool oka[RP], okb[RP];
#pragma unroll
    for (int p = 0; p < RP; ++p) {
        const int va = I * TM + rbase + 8 * p, vb = J * TM + rbase + 8 * p;
        oka[p] = va < nvars, okb[p] = vb < nvars;
        ma[p] = oka[p] ? mean[va] : 0.0;
        mb[p] = okb[p] ? mean[vb] : 0.0;
    }
    auto load = [&](long long st) {
        const long long s = st * kStage + col;
        const bool in = s < N;
#pragma unroll
        for (int p = 0; p < RP; ++p) {
            const long long va = (long long)I * TM + rbase + 8 * p;
            ra[p] = in && oka[p] ? X[va * N + s] - ma[p] : 0.0;
        }
        if (!diag) {
#pragma unroll
            for (int p = 0; p < RP; ++p) {
                const long long vb = (long long)J * TM + rbase + 8 * p;
                rb[p] = in && okb[p] ? X[vb * N + s] - mb[p] : 0.0;
            }
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int p = 0; p < RP; ++p) lds[buf][0][(rbase + 8 * p) * kLd + col] = ra[p];
        if (!diag) {
#pragma unroll
            for (int p = 0; p < RP; ++p) lds[buf][1][(rbase + 8 * p) * kLd + col] = rb[p];
        }
    };

    v4d acc[MT][MT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < MT; ++n) acc[m][n] = v4d{0.0, 0.0, 0.0, 0.0};

    const int fi = lane & 15, fk = lane >> 4;
    if (st0 < st1) {
        load(st0);
        store(0);
        __syncthreads();
    }
    for (long long st = st0; st < st1; ++st) {
        const int cur = (int)((st - st0) & 1);
        const bool more = st + 1 < st1;
        if (more) load(st + 1);
        const double *pa = lds[cur][0] + (wm * WT + fi) * kLd + fk;
        const double *pb = lds[cur][diag ? 0 : 1] + (wn * WT + fi) * kLd + fk;
#pragma unroll
        for (int ks = 0; ks < kStage / 4; ++ks) {
            double a[MT], b[MT];
#pragma unroll
            for (int m = 0; m < MT; ++m) a[m] = pa[16 * m * kLd + 4 * ks];
#pragma unroll
            for (int n = 0; n < MT; ++n) b[n] = pb[16 * n * kLd + 4 * ks];
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int n = 0; n < MT; ++n) acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], b[n], acc[m][n], 0, 0, 0);
        }
        if (more) store(cur ^ 1);
        __syncthreads();
    }
    // C/D layout of the 16 x 16 x 4 fp64 MFMA: register v of lane l is row 4 v + l / 16, column l % 16
    double *out = slab + ((long long)split * nt + tile) * TM * TM;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < MT; ++n)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int row = wm * WT + 16 * m + 4 * v + fk, c = wn * WT + 16 * n + fi;
                out[row * TM + c] = acc[m][n][v];
            }
}

template <int TM>
__global__ __launch_bounds__(256) void gci_reduce(const double *__restrict__ slab, int nvars, int T, int nt, int S,
                                                  double *__restrict__ R, double *__restrict__ var) {
    const int tile = blockIdx.x, e = blockIdx.y * 256 + threadIdx.x, ii = e / TM, jj = e % TM;
    int I, J;
    tile_of(tile, T, &I, &J);
    const int i = I * TM + ii, j = J * TM + jj;
    if (i >= nvars || j >= nvars || j < i) return;
    // the diagonal tiles of rows I and J: tile_of's inverse at (I, I)
    const long long tdi = (long long)I * T - (long long)I * (I - 1) / 2, tdj = (long long)J * T - (long long)J * (J - 1) / 2;
    const long long TT = (long long)TM * TM;
    double sij = 0.0, sii = 0.0, sjj = 0.0;
    for (int s = 0; s < S; ++s) {
        const double *base = slab + (long long)s * nt * TT;
        sij += base[tile * TT + ii * TM + jj];
        sii += base[tdi * TT + ii * TM + ii];
        sjj += base[tdj * TT + jj * TM + jj];
    }
    if (i == j) {
        R[(long long)i * nvars + i] = 1.0;
        var[i] = sii;
        return;
    }
    const double den = sqrt(sii * sjj);
    const double r = den > 0.0 ? sij / den : 0.0;  // (a zero variance is refused by the caller through var)
    R[(long long)i * nvars + j] = r;
    R[(long long)j * nvars + i] = r;
}

}  // namespace

extern "C" int fbn_gci_stage(void) { return kStage; }

extern "C" hipError_t fbn_gci_means_launch(const double *X, int nvars, long long N, double *mean, int *bad, hipStream_t s) {
    hipLaunchKernelGGL(gci_means, dim3((unsigned)nvars), dim3(256), 0, s, X, N, mean, bad);
    return hipGetLastError();
}

// tile = 64 or 32; split_k >= 1 and at most the number of stages; slab: split_k * nt * tile^2 doubles with
// nt = T (T + 1) / 2, T = ceil(nvars / tile)
extern "C" hipError_t fbn_gci_gram_launch(const GciCorrArgs *a, hipStream_t s) {
    const int T = (a->nvars + a->tile - 1) / a->tile, nt = T * (T + 1) / 2, S = a->split_k;
    const long long nstages = (a->N + kStage - 1) / kStage;
    if ((a->tile != 32 && a->tile != 64) || S < 1 || S > nstages) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(nt * S));
    if (a->tile == 64)
        hipLaunchKernelGGL(gci_gram<64>, grid, dim3(256), 0, s, a->X, a->mean, a->nvars, a->N, T, nt, S, nstages, a->slab);
    else
        hipLaunchKernelGGL(gci_gram<32>, grid, dim3(256), 0, s, a->X, a->mean, a->nvars, a->N, T, nt, S, nstages, a->slab);
    return hipGetLastError();
}

extern "C" hipError_t fbn_gci_reduce_launch(const GciCorrArgs *a, hipStream_t s) {
    const int T = (a->nvars + a->tile - 1) / a->tile, nt = T * (T + 1) / 2;
    if (a->tile != 32 && a->tile != 64) return hipErrorInvalidValue;
    const dim3 grid((unsigned)nt, (unsigned)(a->tile * a->tile / 256));
    if (a->tile == 64)
        hipLaunchKernelGGL(gci_reduce<64>, grid, dim3(256), 0, s, a->slab, a->nvars, T, nt, a->split_k, a->R, a->var);
    else
        hipLaunchKernelGGL(gci_reduce<32>, grid, dim3(256), 0, s, a->slab, a->nvars, T, nt, a->split_k, a->R, a->var);
    return hipGetLastError();
}
