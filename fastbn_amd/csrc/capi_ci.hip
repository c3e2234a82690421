// capi_ci.hip -- the CI-test and parameter-learning entries of include/fastbn.h: the CI context (column
// store, bit-sliced / packed / one-hot stores, Grams), the batch launch, the family counts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "capi_state.h"
#include "ci_chisq.h"
#include "launchers.h"
#include "param_counts.h"
#include "pc_internal.h"

using fbn::SetError;

namespace fbn {

// the band for `alpha` (delta = alpha / 1024: few tests fall inside, so few evaluate p) over df 1..max(want_df, kBandDf) (at most kBandDfMax),
// computed on the host per ctx and alpha and extended on demand; *out = nullptr (p evaluated for
// every test) when alpha is outside (0, 1) or FBN_CI_NO_BAND is set
int CiBand(fbn_ci_ctx *c, double alpha, hipStream_t s, const double **out, int *nband, int want_df) {
    *out = nullptr;
    *nband = 0;
    if (!(alpha > 0.0 && alpha < 1.0) || fbn::KnobSet("FBN_CI_NO_BAND")) return FBN_OK;
    const int want = std::min(kBandDfMax, std::max(kBandDf, want_df));
    if (c->band_alpha != alpha || c->band_n < want) {
        const double delta = alpha / 1024;
        const int have = c->band_alpha == alpha ? c->band_n : 0;
        FBN_HIP(hipStreamSynchronize(s));  // the previous upload of the host table has completed
        c->band_host.resize(2 * (size_t)want + 1);
        for (int df = have + 1; df <= want; ++df)
            fbn_chisq_band(alpha, delta, df, &c->band_host[2 * df - 2], &c->band_host[2 * df - 1]);
        c->band_host[2 * (size_t)want] = delta;
        if (int rc = c->band.ensure(c->band_host.size() * 8)) return rc;
        FBN_HIP(hipMemcpyAsync(c->band.p, c->band_host.data(), c->band_host.size() * 8, hipMemcpyHostToDevice, s));
        c->band_alpha = alpha;
        c->band_n = want;
    }
    *out = c->band.as<double>();
    *nband = c->band_n;
    return FBN_OK;
}

// The margin log lives on the device (atomics of every batch kernel); reset and read are
// stream-ordered copies through a pinned 32-byte buffer ([0..1] the reset value, constant; [2..3]
// the read-back).  Work the caller queued on its own streams (fbn_ci_run_device) is drained first.
static int CiMarginPinned(fbn_ci_ctx *c) {
    if (c->h_margin) return FBN_OK;
    hipError_t e = hipHostMalloc((void **)&c->h_margin, 32, hipHostMallocDefault);
    if (e != hipSuccess) return SetError(FBN_ERR_NOMEM, "hipHostMalloc: %s", hipGetErrorString(e));
    c->h_margin[0] = 0x7FF0000000000000ull;  // +inf
    c->h_margin[1] = 0;
    return FBN_OK;
}

int CiResetMargin(fbn_ci_ctx *c) {
    if (int rc = CiMarginPinned(c)) return rc;
    FBN_HIP(hipDeviceSynchronize());
    FBN_HIP(hipMemcpyAsync(c->stats.p, c->h_margin, 16, hipMemcpyHostToDevice, c->stream));
    return FBN_OK;
}

int CiReadMargin(fbn_ci_ctx *c, double *min_margin, int64_t *near_alpha, bool own_stream_only) {
    if (int rc = CiMarginPinned(c)) return rc;
    if (!own_stream_only) FBN_HIP(hipDeviceSynchronize());
    FBN_HIP(hipMemcpyAsync(c->h_margin + 2, c->stats.p, 16, hipMemcpyDeviceToHost, c->stream));
    FBN_HIP(hipStreamSynchronize(c->stream));
    double m;
    memcpy(&m, &c->h_margin[2], 8);
    if (min_margin) *min_margin = m;
    if (near_alpha) *near_alpha = (int64_t)c->h_margin[3];
    return FBN_OK;
}

}  // namespace fbn

extern "C" {

// ------------------------------------------------------------------ CI tests
// the column store from host memory (cols_on_device = false) or from a device buffer of the same
// device, e.g. one filled by an RCCL broadcast (true); every code is checked < dims[v] on the
// device before any kernel bins with it
static int CiCreate(const uint8_t *cols, bool cols_on_device, int nvars, int64_t nsamples, const int32_t *dims,
                    int device, fbn_ci_ctx **out) {
    if (!cols || !dims || !out || nvars <= 0 || nsamples <= 0) return SetError(FBN_ERR_ARG, "bad argument");
    for (int v = 0; v < nvars; ++v)
        if (dims[v] < 1 || dims[v] > 256) return SetError(FBN_ERR_ARG, "dims[%d] = %d out of 1..256", v, dims[v]);
    auto c = std::unique_ptr<fbn_ci_ctx>(new (std::nothrow) fbn_ci_ctx());
    if (!c) return SetError(FBN_ERR_NOMEM, "out of memory");
    int rc = fbn::CheckDevice(device, &c->num_cu);
    if (rc) return rc;
    FBN_HIP(hipSetDevice(device));
    c->device = device;
    c->nvars = nvars;
    c->N = nsamples;
    c->dims.assign(dims, dims + nvars);
    // 32 readable bytes past the last column: param_counts.hip reads a misaligned column as aligned
    // dwords, up to 19 bytes past the column's last sample
    if ((rc = c->cols.ensure((size_t)nvars * nsamples + 32))) return rc;
    if ((rc = c->ddims.ensure((size_t)nvars * 4))) return rc;
    if ((rc = c->stats.ensure(16))) return rc;
    FBN_HIP(hipMemcpy(c->cols.p, cols, (size_t)nvars * nsamples,
                      cols_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    FBN_HIP(hipMemcpy(c->ddims.p, dims, (size_t)nvars * 4, hipMemcpyHostToDevice));
    {
        FBN_HIP(hipMemset(c->stats.p, 0, 16));
        hipError_t e = fbn_ci_cols_check(c->cols.as<uint8_t>(), c->ddims.as<int32_t>(), nvars, nsamples,
                                         c->stats.as<int>(), nullptr);
        if (e != hipSuccess) return SetError(FBN_ERR_HIP, "column check: %s", hipGetErrorString(e));
        int bad[2] = {0, 0};
        FBN_HIP(hipMemcpy(bad, c->stats.p, 8, hipMemcpyDeviceToHost));
        if (bad[0])
            return SetError(FBN_ERR_ARG, "column store: variable %d holds a code >= its state count %d", bad[1] - 1,
                            dims[bad[1] - 1]);
    }
    for (auto &sl : c->slot) {
        FBN_HIP(hipEventCreate(&sl.ev0));
        FBN_HIP(hipEventCreate(&sl.ev1));
        FBN_HIP(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    }
    FBN_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    if ((rc = fbn::CiResetMargin(c.get()))) return rc;
    *out = c.release();
    return FBN_OK;
}
int fbn_ci_set_kernel_timing(fbn_ci_ctx *c, int enable) {
    if (!c) return SetError(FBN_ERR_ARG, "null pointer");
    c->timing = enable != 0;
    return FBN_OK;
}
int fbn_ci_dataset_upload(const uint8_t *cols, int nvars, int64_t nsamples, const int32_t *dims, int device,
                          fbn_ci_ctx **out) {
    return CiCreate(cols, false, nvars, nsamples, dims, device, out);
}
int fbn_ci_dataset_from_device(const uint8_t *d_cols, int nvars, int64_t nsamples, const int32_t *dims, int device,
                               fbn_ci_ctx **out) {
    return CiCreate(d_cols, true, nvars, nsamples, dims, device, out);
}

}  // extern "C"

namespace fbn {

// Tasks of the register-blocked level-0 kernel for the pairs [t0, t1) of the complete graph (pair
// index = lexicographic (u < v) order): x-side variables = the range's rows u, y-side = all variables,
// both cut into sorted blocks per state-count class (fbn_ci_pair_block); a task is kept if it holds
// a pair (x < y) of the range, so every pair of the range is in exactly one task (x-side = its u).
// Cached per range (a PC run's level 0 repeats it).
static int CiPairTasks(fbn_ci_ctx *c, int64_t t0, int64_t t1, hipStream_t s) {
    if (c->ptask_t0 == t0 && c->ptask_t1 == t1) return FBN_OK;
    const int nv = c->nvars;
    const int64_t P = (int64_t)nv * (nv - 1) / 2;
    const int u0 = t1 > t0 ? PairRow(t0, nv) : 0, u1 = t1 > t0 ? PairRow(t1 - 1, nv) : -1;
    const bool full = t0 == 0 && t1 == P;
    std::vector<int> cls[5], ucls[5];
    for (int v = 0; v < nv; ++v) {
        const int d = c->dims[v];
        if (d < 1 || d > 4) return SetError(FBN_ERR_ARG, "blocked pairs: variable %d has %d states", v, d);
        cls[d].push_back(v);
        if (v >= u0 && v <= u1) ucls[d].push_back(v);
    }
    std::vector<int32_t> tasks;
    for (int dx = 1; dx <= 4; ++dx)
        for (int dy = 1; dy <= 4; ++dy) {
            const int bx = fbn_ci_pair_block(dx), by = fbn_ci_pair_block(dy);
            const std::vector<int> &X = ucls[dx], &Y = cls[dy];
            for (size_t i = 0; i < X.size(); i += bx) {
                const int nxs = (int)std::min<size_t>(bx, X.size() - i);
                for (size_t j = 0; j < Y.size(); j += by) {
                    const int nys = (int)std::min<size_t>(by, Y.size() - j);
                    if (Y[j + nys - 1] <= X[i]) continue;  // no y above any x
                    bool any = full;
                    for (int a = 0; a < nxs && !any; ++a)
                        for (int b = 0; b < nys && !any; ++b) {
                            const int x = X[i + a], y = Y[j + b];
                            if (x < y) {
                                const int64_t t = PairIndex(x, y, nv);
                                any = t >= t0 && t < t1;
                            }
                        }
                    if (!any) continue;
                    const size_t o = tasks.size();
                    tasks.resize(o + 12, -1);
                    tasks[o] = dx, tasks[o + 1] = dy, tasks[o + 2] = nxs, tasks[o + 3] = nys;
                    for (int a = 0; a < nxs; ++a) tasks[o + 4 + a] = X[i + a];
                    for (int b = 0; b < nys; ++b) tasks[o + 8 + b] = Y[j + b];
                }
            }
        }
    int rc;
    if ((rc = c->ptasks.ensure(std::max<size_t>(tasks.size(), 1) * 4))) return rc;
    if (!tasks.empty()) FBN_HIP(hipMemcpyAsync(c->ptasks.p, tasks.data(), tasks.size() * 4, hipMemcpyHostToDevice, s));
    FBN_HIP(hipStreamSynchronize(s));  // the host vector goes out of scope
    c->ptask_t0 = t0, c->ptask_t1 = t1, c->ptask_n = (int64_t)tasks.size() / 12;
    return FBN_OK;
}

// the leading rows of the bit-sliced store (once per ctx, after the bits build)
int CiLeadEnsure(fbn_ci_ctx *c, hipStream_t s) {
    if (c->lead_ready) return FBN_OK;
    const int nv = c->nvars;
    c->lead0_host.assign(nv, 0);
    c->leadrows_host.clear();
    for (int v = 0; v < nv; ++v) {
        c->lead0_host[v] = (int32_t)c->leadrows_host.size();
        for (int a = 0; a + 1 < c->dims[v]; ++a) c->leadrows_host.push_back(c->row0_host[v] + a);
    }
    int rc;
    if ((rc = c->lead0.ensure((size_t)nv * 4))) return rc;
    if ((rc = c->leadrows.ensure(std::max<size_t>(c->leadrows_host.size(), 1) * 4))) return rc;
    FBN_HIP(hipMemcpyAsync(c->lead0.p, c->lead0_host.data(), (size_t)nv * 4, hipMemcpyHostToDevice, s));
    if (!c->leadrows_host.empty())
        FBN_HIP(hipMemcpyAsync(c->leadrows.p, c->leadrows_host.data(), c->leadrows_host.size() * 4,
                               hipMemcpyHostToDevice, s));
    c->lead_ready = true;
    return FBN_OK;
}

// level 0 through the Gram when its ld x ld int32 matrix fits this budget (else the tiled kernel)
constexpr int64_t kGram0MaxBytes = (int64_t)1 << 30;
static bool CiGram0Eligible(const fbn_ci_ctx *c) {
    int64_t R = 0;
    for (int v = 0; v < c->nvars; ++v) R += c->dims[v] - 1;
    return R > 0 && R * R * 4 <= kGram0MaxBytes && !fbn::KnobSet("FBN_CI_NO_GRAM");
}

// 8 x 8 tiles (i-block <= j-block) of the leading-row Gram holding a pair (x < y) of [t0, t1): row
// i of x's leading rows, column j of y's (x < y puts every needed entry in an upper tile).  Cached
// per range.
static int CiGram0Tasks(fbn_ci_ctx *c, int64_t t0, int64_t t1, hipStream_t s) {
    if (c->g0_t0 == t0 && c->g0_t1 == t1) return FBN_OK;
    const int nv = c->nvars;
    const int64_t R = (int64_t)c->leadrows_host.size(), nb = (R + 7) / 8;
    std::vector<int32_t> var_of(R);
    for (int v = 0; v < nv; ++v)
        for (int a = 0; a + 1 < c->dims[v]; ++a) var_of[c->lead0_host[v] + a] = v;
    const int TI = fbn_ci_gram_task_ints();
    std::vector<int32_t> tasks;
    // tiles in 16 x 16-tile super-blocks (128 + 128 rows = 3.2 MB at 100k samples: one XCD's L2),
    // consecutive in the task list, which the kernel splits XCD-contiguously
    constexpr int64_t SB = 16;
    for (int64_t si = 0; si < nb; si += SB)
    for (int64_t sj = si; sj < nb; sj += SB)
    for (int64_t bi = si; bi < std::min(nb, si + SB); ++bi) {
        const int64_t r0 = 8 * bi, r1 = std::min(R, r0 + 8);
        const int vi0 = var_of[r0], vi1 = var_of[r1 - 1];
        for (int64_t bj = std::max(bi, sj); bj < std::min(nb, sj + SB); ++bj) {
            const int64_t c0 = 8 * bj, c1 = std::min(R, c0 + 8);
            const int vj0 = var_of[c0], vj1 = var_of[c1 - 1];
            if (vi0 >= vj1) continue;  // no x < y in the tile
            const int64_t tmin = PairIndex(vi0, std::max(vj0, vi0 + 1), nv),
                          tmax = PairIndex(std::min(vi1, vj1 - 1), vj1, nv);
            if (tmax < t0 || tmin >= t1) continue;
            const int64_t off = r0 * R + c0;
            const int32_t t[8] = {-1, (int32_t)r0, (int32_t)(r1 - r0), (int32_t)c0, (int32_t)(c1 - c0),
                                  (int32_t)(uint32_t)(off & 0xffffffff), (int32_t)(off >> 32), (int32_t)R};
            tasks.insert(tasks.end(), t, t + TI);
        }
    }
    int rc;
    if ((rc = c->g0tasks.ensure(std::max<size_t>(tasks.size(), 1) * 4))) return rc;
    if (!tasks.empty()) FBN_HIP(hipMemcpyAsync(c->g0tasks.p, tasks.data(), tasks.size() * 4, hipMemcpyHostToDevice, s));
    FBN_HIP(hipStreamSynchronize(s));  // the host vector goes out of scope
    c->g0_t0 = t0, c->g0_t1 = t1, c->g0_ntasks = (int64_t)tasks.size() / TI;
    return FBN_OK;
}

// x-variable row range [r0, r1) of the leading rows that the pairs [t0, t0 + n) read as rows of G
static void CiPairRowRange(const fbn_ci_ctx *c, int64_t t0, int64_t n, int64_t *r0, int64_t *r1) {
    const int nv = c->nvars;
    const int u0 = PairRow(t0, nv), u1 = PairRow(t0 + n - 1, nv);
    *r0 = c->lead0_host[u0];
    *r1 = u1 + 1 < nv ? c->lead0_host[u1 + 1] : (int64_t)c->leadrows_host.size();
}

// The level-0 Gram on the matrix cores, hand-written (ci_gram_mfma.hip): FP4 one-hot store built
// once per ctx, the 256 x 256 tiles (I, J >= I) covering rows [r0, r1) x all columns, split-K so the
// launch fills the CUs, uint16 partial slabs summed into gram0 (entries i < j).  *done = false: not
// used (small Gram -- ALARM's 60 rows x 5k samples stay on the popcount kernel --, over the byte
// budget, or FBN_CI_GRAM_NO_MFMA).
constexpr int64_t kOnehot4MaxBytes = (int64_t)4 << 30;
static int CiGram0Mfma(fbn_ci_ctx *c, int64_t t0, int64_t n, hipStream_t s, bool *done) {
    *done = false;
    const int64_t R = (int64_t)c->leadrows_host.size(), T = fbn_ci_gram4_tile(), KT = fbn_ci_gram4_stage();
    const int64_t Rp = (R + T - 1) / T * T, KS = (c->N + KT - 1) / KT, Kb = KS * KT / 2;
    if (fbn::KnobSet("FBN_CI_GRAM_NO_MFMA") || (double)R * R * c->N < 1e10 || Rp * Kb > kOnehot4MaxBytes || KS > INT32_MAX)
        return FBN_OK;
    int rc;
    if (!c->onehot4_ready) {
        if ((rc = c->onehot4.ensure((size_t)(Rp * Kb)))) return rc;
        FBN_HIP(hipMemsetAsync(c->onehot4.p, 0, (size_t)(Rp * Kb), s));  // pad rows R..Rp-1
        hipError_t e = fbn_ci_onehot4_build(c->cols.as<uint8_t>(), c->ddims.as<int32_t>(), c->lead0.as<int32_t>(), c->N,
                                            KS, Rp, c->nvars, c->onehot4.as<uint8_t>(), s);
        if (e != hipSuccess) return SetError(FBN_ERR_HIP, "fp4 one-hot build: %s", hipGetErrorString(e));
        c->onehot4_ready = true;
    }
    int64_t r0, r1;
    CiPairRowRange(c, t0, n, &r0, &r1);
    const int64_t info0[8] = {2, R, Rp, KS, 0, 0, 0, 0};
    std::copy(info0, info0 + 8, c->l0_info);
    if (r1 <= r0) {  // the range's x variables have no leading rows: nothing of G is read
        *done = true;
        return FBN_OK;
    }
    if (c->g4_r0 != r0 || c->g4_r1 != r1) {
        std::vector<int32_t> tasks;
        const int64_t nb = Rp / T;
        for (int64_t I = r0 / T; I <= (r1 - 1) / T; ++I)
            for (int64_t J = I; J < nb; ++J) tasks.push_back((int32_t)I), tasks.push_back((int32_t)J);
        if ((rc = c->g4tasks.ensure(tasks.size() * 4))) return rc;
        FBN_HIP(hipMemcpyAsync(c->g4tasks.p, tasks.data(), tasks.size() * 4, hipMemcpyHostToDevice, s));
        FBN_HIP(hipStreamSynchronize(s));  // the host vector goes out of scope
        c->g4_nt = (int)(tasks.size() / 2), c->g4_r0 = r0, c->g4_r1 = r1;
    }
    // split-K: about one block per CU; uint16 partials need every slice <= 65535 samples
    const int nt = c->g4_nt;
    int64_t S = std::max<int64_t>(1, fbn::KnobOr("FBN_CI_GRAM4_SPLITS", c->num_cu / nt));
    S = std::max<int64_t>(S, (KS + 510) / 511);  // slices of <= 511 stages x 128 samples
    S = std::min<int64_t>(S, KS);
    // slice `split` covers stages [split * KS / S, (split + 1) * KS / S): floor or ceil of KS / S
    c->l0_info[4] = nt, c->l0_info[5] = S, c->l0_info[6] = KS / S, c->l0_info[7] = (KS + S - 1) / S;
    if ((rc = c->g4slab.ensure((size_t)(nt * S * T * T * 2)))) return rc;
    hipError_t e = fbn_ci_gram4(c->onehot4.as<uint8_t>(), Rp, c->g4tasks.as<int2>(), nt, (int)S, (int)KS,
                                c->g4slab.as<uint16_t>(), (int)R, R, c->gram0.as<int32_t>(), s);
    if (e != hipSuccess) return SetError(FBN_ERR_HIP, "mfma gram: %s", hipGetErrorString(e));
    *done = true;
    return FBN_OK;
}

// the bit-sliced store (one mask row per value, W words per row padded to a multiple of 4 for
// 16-byte loads) and the per-row sample counts, built once per ctx on stream s
int CiBitsEnsure(fbn_ci_ctx *c, hipStream_t s) {
    if (c->bits_ready) return FBN_OK;
    int rc;
    const int64_t W = ((c->N + 31) / 32 + 3) & ~(int64_t)3;
    std::vector<int32_t> row0(c->nvars);
    int64_t rows = 0;
    for (int v = 0; v < c->nvars; ++v) row0[v] = (int32_t)rows, rows += std::min(c->dims[v], 8);
    c->row0_host = row0;
    if ((rc = c->bits.ensure((size_t)std::max<int64_t>(rows * W, 1) * 4))) return rc;
    if ((rc = c->brow.ensure((size_t)c->nvars * 4))) return rc;
    FBN_HIP(hipMemcpyAsync(c->brow.p, c->row0_host.data(), (size_t)c->nvars * 4, hipMemcpyHostToDevice, s));
    hipError_t e = fbn_ci_bits_build(c->cols.as<uint8_t>(), c->ddims.as<int32_t>(), c->brow.as<int32_t>(), c->N, W,
                                     c->nvars, c->bits.as<uint32_t>(), s);
    if (e != hipSuccess) return SetError(FBN_ERR_HIP, "ci bits build: %s", hipGetErrorString(e));
    if ((rc = c->browcnt.ensure((size_t)std::max<int64_t>(rows, 1) * 4))) return rc;
    e = fbn_ci_bits_rowcount(c->bits.as<uint32_t>(), rows, W, c->browcnt.as<int32_t>(), s);
    if (e != hipSuccess) return SetError(FBN_ERR_HIP, "ci bits row counts: %s", hipGetErrorString(e));
    c->bits_W = W;
    c->bits_ready = true;
    return FBN_OK;
}

// the 2-bit packed columns (every state count <= 4): PW words per variable, built once per ctx
int CiPack2Ensure(fbn_ci_ctx *c, hipStream_t s) {
    if (c->pack2_ready) return FBN_OK;
    int rc;
    const int64_t PW = (c->N + 15) / 16;
    if ((rc = c->pack2.ensure((size_t)std::max<int64_t>(PW * c->nvars, 1) * 4))) return rc;
    hipError_t e = fbn_ci_pack2_build(c->cols.as<uint8_t>(), c->nvars, c->N, PW, c->pack2.as<uint32_t>(), s);
    if (e != hipSuccess) return SetError(FBN_ERR_HIP, "ci pack2 build: %s", hipGetErrorString(e));
    c->pack2_W = PW;
    c->pack2_ready = true;
    return FBN_OK;
}

// The histogram kernel (ci_kernels.hip) holds a test's cell count, every cell index and every
// offset of its table layout (cells, sub-histograms, marginals, term buffer: fbn_ci_lds_bytes) in
// 32-bit ints: a test whose layout does not fit is refused here, before anything is allocated or
// launched.  it: the test's variables (x, y, z_1 .. z_d, validated); -> its conditioning
// configurations and layout bytes.
static int CiTableCheck(const fbn_ci_ctx *c, const int32_t *it, int d, long long test, int64_t *dimz_out,
                        size_t *bytes_out) {
    int64_t dimz = 1;
    for (int j = 0; j < d; ++j) {
        dimz *= c->dims[it[2 + j]];
        if (dimz > (1 << 24)) return SetError(FBN_ERR_LIMIT, "test %lld: conditioning table too large", test);
    }
    const int dx = c->dims[it[0]], dy = c->dims[it[1]];
    const size_t bytes = fbn_ci_lds_bytes((int)dimz, dx, dy);
    if (bytes / 4 > (size_t)INT32_MAX)
        return SetError(FBN_ERR_LIMIT,
                        "test %lld: table of %lld cells (%lld conditioning configurations x %d x %d states) is beyond "
                        "the kernel's 32-bit int cell indexing (cells, marginals and term buffer: at most 2^31 - 1 ints)",
                        test, (long long)(dimz * dx * dy), (long long)dimz, dx, dy);
    if (dimz_out) *dimz_out = dimz;
    if (bytes_out) *bytes_out = bytes;
    return FBN_OK;
}

// tests with <= 1 conditioning variable over variables with <= 4 states: popcounts of bit-sliced
// columns (ci_bits_count.hip).  From kCiBitsMinSamples samples up (ALARM-5000 included: 0.46 -> 0.40 ms per
// PC run with the pair-table level 1); below, the byte-column kernel (untuned regime).
bool CiBitsEligible(const fbn_ci_ctx *c, int maxdim) {
    return maxdim <= 4 && !fbn::KnobSet("FBN_CI_NO_BITS") &&
           (c->N >= kCiBitsMinSamples || fbn::KnobSet("FBN_CI_FORCE_BITS"));
}

// the slot's item and decision buffers and, for want_g2p, the ctx's G^2 / p buffers, for n tests
static int CiOutputsEnsure(fbn_ci_ctx *c, CiSlot &S, const CiBatchReq &q) {
    int rc;
    if (!q.all_pairs && (rc = S.items.ensure((size_t)q.n * (2 + q.d) * 4))) return rc;
    if ((rc = S.indep.ensure((size_t)q.n))) return rc;
    if ((rc = S.df.ensure((size_t)q.n * 4))) return rc;
    if (q.want_g2p) {
        if ((rc = c->g2.ensure((size_t)q.n * 8))) return rc;
        if ((rc = c->p.ensure((size_t)q.n * 8))) return rc;
    }
    return FBN_OK;
}

// the bit-sliced path (d <= 1, every state count <= 4); dim_rows: sum of the items' state counts
static int CiLaunchBits(fbn_ci_ctx *c, const CiBatchReq &q, int64_t dim_rows, hipStream_t s) {
    CiSlot &S = c->slot[q.k];
    const int64_t n = q.n, pair0 = q.pair0;
    const int d = q.d;
    const bool all_pairs = q.all_pairs, want_g2p = q.want_g2p;
    int rc;
    if ((rc = CiBitsEnsure(c, s))) return rc;
    if ((rc = CiOutputsEnsure(c, S, q))) return rc;
    if ((rc = S.bcounts.ensure((size_t)n * 64 * 4))) return rc;
    if (!q.zc_items && !all_pairs)
        FBN_HIP(hipMemcpyAsync(S.items.p, q.items, (size_t)n * (2 + d) * 4, hipMemcpyHostToDevice, s));
    int pmode = 0;
    double *g2rec = nullptr;  // level 0's G^2 per pair, kept for the level-1 screen
    if (c->pair_mode == 1 && d == 0) {
        const size_t np = (size_t)c->nvars * (c->nvars - 1) / 2;
        if ((rc = c->pairtab.ensure(std::max<size_t>(np, 1) * 16 * 4))) return rc;
        pmode = 1;
        c->pairs_recorded = true;
        if (all_pairs && !want_g2p && pair0 == c->l1mi_covered) {
            if ((rc = c->l1mi.ensure(std::max<size_t>(np, 1) * 8))) return rc;
            g2rec = c->l1mi.as<double>() + pair0;
            c->l1mi_covered = pair0 + n;
        }
    } else if (c->pair_mode == 2 && d == 1 && c->pairs_recorded) {
        pmode = 2;
    }
    // mask rows the count kernel reads: the last value of x and y (and z with pair tables)
    // is derived, not read (ci_bits_count.hip)
    const int64_t skipped = d == 0 ? 2 : (pmode == 2 ? 3 : 0);
    S.last_bytes = (dim_rows - skipped * n) * c->bits_W * 4;
    const double *band = nullptr;  // decisions only: p evaluated inside the band
    int nband = 0;
    if (!want_g2p && (rc = CiBand(c, q.alpha, s, &band, &nband))) return rc;
    if (c->timing) FBN_HIP(hipEventRecord(S.ev0, s));
    // all pairs of a range: register-blocked count kernel (ci_bits_pairs_tiled), then phase 2
    const bool gram0 = all_pairs && d == 0 && CiGram0Eligible(c);
    const bool tiled = all_pairs && d == 0 && !gram0;
    if (tiled && (rc = CiPairTasks(c, pair0, pair0 + n, s))) return rc;
    if (all_pairs && d == 0) {  // fbn_ci_level0_info (the Gram branches below fill in theirs)
        std::fill(c->l0_info, c->l0_info + 8, 0);
        c->l0_info[0] = tiled ? 3 : 0;
    }
    hipError_t e = hipSuccess;
    if (gram0) {  // Gram of the leading rows, then every pair's table from it
        if ((rc = CiLeadEnsure(c, s))) return rc;
        const int64_t R = (int64_t)c->leadrows_host.size();
        if ((rc = c->gram0.ensure((size_t)(R * R * 4)))) return rc;
        bool done = false;
        if ((rc = CiGram0Mfma(c, pair0, n, s, &done))) return rc;
        if (!done) {
            if ((rc = CiGram0Tasks(c, pair0, pair0 + n, s))) return rc;
            c->l0_info[0] = 1, c->l0_info[1] = R, c->l0_info[4] = c->g0_ntasks;
            e = fbn_ci_gram(c->bits.as<uint32_t>(), c->bits_W, c->leadrows.as<int32_t>(),
                            c->g0tasks.as<int32_t>(), c->g0_ntasks, c->gram0.as<int32_t>(), c->num_cu, s);
        }
        if (e == hipSuccess)
            e = fbn_ci_gram_pairs(c->gram0.as<int32_t>(), R, c->lead0.as<int32_t>(), c->ddims.as<int32_t>(),
                                  c->brow.as<int32_t>(), c->browcnt.as<int32_t>(), pair0, n, c->nvars,
                                  S.bcounts.as<int32_t>(), pmode == 1 ? c->pairtab.as<int32_t>() : nullptr,
                                  c->num_cu, s);
        if (e != hipSuccess) return SetError(FBN_ERR_HIP, "ci gram level 0: %s", hipGetErrorString(e));
    }
    if (tiled) {
        e = fbn_ci_bits_pairs_tiled(c->bits.as<uint32_t>(), c->brow.as<int32_t>(), c->browcnt.as<int32_t>(),
                                    c->bits_W, c->ptasks.as<int32_t>(), c->ptask_n, c->nvars, pair0, pair0 + n,
                                    S.bcounts.as<int32_t>(), pmode == 1 ? c->pairtab.as<int32_t>() : nullptr,
                                    c->num_cu, s);
        if (e != hipSuccess) return SetError(FBN_ERR_HIP, "ci tiled pairs launch: %s", hipGetErrorString(e));
    }
    CiBitsArgs a{};
    a.bits = c->bits.as<uint32_t>(), a.dims = c->ddims.as<int32_t>();
    a.row0 = c->brow.as<int32_t>(), a.rowcnt = c->browcnt.as<int32_t>();
    // all pairs of the complete graph: the kernels decode test t into its pair (no item array)
    a.items = all_pairs ? nullptr : q.zc_items ? q.zc_items : S.items.as<int32_t>();
    a.W = c->bits_W, a.n = n, a.t0 = pair0;
    a.d = d, a.alpha = q.alpha;
    a.g2 = want_g2p ? c->g2.as<double>() : g2rec;
    a.df = q.zc_df ? q.zc_df : S.df.as<int32_t>();
    a.p = want_g2p ? c->p.as<double>() : nullptr;
    a.indep = q.zc_indep ? q.zc_indep : S.indep.as<uint8_t>();
    a.counts = S.bcounts.as<int32_t>(), a.counts0 = q.counts_dev;
    a.stats = c->stats.as<unsigned long long>();
    a.pairtab = c->pairtab.as<int32_t>(), a.pmode = pmode;
    a.nvars = c->nvars, a.num_cu = c->num_cu;
    a.counted = (tiled || gram0) ? 1 : 0;
    a.band = band, a.nband = nband;
    e = fbn_ci_bits_launch(&a, s);
    if (e != hipSuccess) return SetError(FBN_ERR_HIP, "ci bits kernel launch: %s", hipGetErrorString(e));
    if (c->timing) FBN_HIP(hipEventRecord(S.ev1, s));
    return FBN_OK;
}

// the histogram path (ci_kernels.hip); maxdim: the items' largest state count
static int CiLaunchHist(fbn_ci_ctx *c, const CiBatchReq &q, int maxdim, hipStream_t s) {
    CiSlot &S = c->slot[q.k];
    const int32_t *items = q.items;
    const int64_t n = q.n;
    const int d = q.d, w = 2 + d;
    const bool want_g2p = q.want_g2p;
    int rc;
    size_t lds = 0;
    int64_t mask_rows = 0;  // bit-sliced counting: dimz * (dx + dy + d) mask rows per test
    for (int64_t i = 0; i < n; ++i) {
        const int32_t *it = items + i * w;
        int64_t dimz = 0;
        size_t bytes = 0;
        if ((rc = CiTableCheck(c, it, d, i, &dimz, &bytes))) return rc;
        lds = std::max(lds, bytes);
        mask_rows += dimz * (c->dims[it[0]] + c->dims[it[1]] + d);
    }
    // tables beyond the LDS budget: the same layout in a per-workgroup global scratch region
    // (the kernel's own static LDS comes on top of the dynamic region)
    const bool global_tables = lds + fbn_ci_static_lds_bytes() > (size_t)fbn::kCuLdsBytes;
    if ((rc = CiOutputsEnsure(c, S, q))) return rc;
    if (!q.zc_items) FBN_HIP(hipMemcpyAsync(S.items.p, items, (size_t)n * w * 4, hipMemcpyHostToDevice, s));
    int grid = (int)std::min<int64_t>(n, (int64_t)c->num_cu * 8);
    int32_t *gscratch = nullptr;
    if (global_tables) {
        // one table region per workgroup, at most 4 GiB of scratch in total (fewer, longer-lived
        // workgroups for very large tables; each loops over its tests)
        const size_t stride = ((lds / 4 + 1) & ~(size_t)1) * 4;
        grid = (int)std::max<size_t>(1, std::min<size_t>((size_t)grid, ((size_t)4 << 30) / stride));
        if ((rc = S.scratch.ensure((size_t)grid * stride))) return rc;
        gscratch = S.scratch.as<int32_t>();
    }
    // FBN_CI_BITSN = 1: d >= 2 tests with every state count <= 4 count from the bit-sliced store
    // (ci_kernels.hip) when it is built.  Opt-in: every z-configuration re-reads the x / y value rows,
    // so config 5 level 2 moves more bytes than the byte columns (0.79 vs 0.76 ms) and levels 3-5
    // are several times slower (up to 4^5 configurations per test)
    const bool bitsn0 = d >= 2 && c->bits_ready && maxdim <= 4 && fbn::KnobSet("FBN_CI_BITSN");
    // d = 2 within a PC run (level-0 pair tables recorded), every state count <= 4, the bit-sliced
    // store built: derived counting of the leading cells (ci_kernels.hip MODE 3; FBN_CI_NO_DER2 = 1
    // takes the 2-bit packed histogram kernel instead)
    const bool der2 = d == 2 && c->bits_ready && maxdim <= 4 && c->pair_mode == 2 && c->pairs_recorded &&
                      !global_tables && !fbn::KnobSet("FBN_CI_NO_DER2");
    const bool bitsn = bitsn0 || der2;
    // decisions only: the decision band up to this batch's largest df ((maxdim-1)^2 maxdim^d)
    const double *hband = nullptr;
    int hnband = 0;
    if (!want_g2p) {
        double dfmax = (double)(maxdim - 1) * (maxdim - 1);
        for (int j = 0; j < d; ++j) dfmax *= maxdim;
        if ((rc = CiBand(c, q.alpha, s, &hband, &hnband, (int)std::min<double>(dfmax, kBandDfMax)))) return rc;
    }
    // every variable of the batch with <= 4 states and >= 64k samples: the histogram kernel reads
    // the columns packed 2 bits per sample (a quarter of the byte columns' bytes; built once per
    // context, 25 MB for config 5).  Config-5 level 2: 0.614 -> 0.589 ms (the kernel's binning, not
    // its column reads, bounds it); below 64k samples (ALARM-5000) the byte columns measured faster.
    // FBN_CI_PACK2 = 1 forces it at any size, FBN_CI_NO_PACK2 = 1 disables it.
    const bool pk = !bitsn && maxdim <= 4 && !fbn::KnobSet("FBN_CI_NO_PACK2") &&
                    (c->N >= 65536 || fbn::KnobSet("FBN_CI_PACK2"));
    if (pk && (rc = CiPack2Ensure(c, s))) return rc;
    S.last_bytes = bitsn ? mask_rows * c->bits_W * 4  // the mask rows each z-configuration reads
                   : pk  ? n * c->pack2_W * 4 * (2 + d)  // the 2-bit columns x, y, z_1..z_d
                         : n * c->N * (2 + d);  // uint8 columns x, y, z_1..z_d streamed once
    // small batches on the packed columns (config 5 levels 3-5: 1056 / 260 / 30 tests of 100k
    // samples): each test's words split over several workgroups so the batch fills the chip, the
    // partial histograms added into a global table per test, then one workgroup per test decides
    int split = 1, split_grid = 0;
    int64_t tstride = 0;
    int32_t *tab = nullptr;
    if (pk && !bitsn && !global_tables) {
        const int64_t want = 4 * (int64_t)c->num_cu;  // counting workgroups to aim for
        split = (int)std::min<int64_t>(16, want / std::max<int64_t>(n, 1));
        if (split > 1) {
            int64_t cmax = 1;
            for (int64_t i = 0; i < n; ++i) {
                const int32_t *it = items + i * w;
                int64_t cells = (int64_t)c->dims[it[0]] * c->dims[it[1]];
                for (int j = 0; j < d; ++j) cells *= c->dims[it[2 + j]];
                cmax = std::max(cmax, cells);
            }
            tstride = (cmax + 63) & ~(int64_t)63;
            if ((rc = S.scratch.ensure((size_t)n * tstride * 4))) return rc;
            tab = S.scratch.as<int32_t>();
            split_grid = (int)std::min<int64_t>(n * split, (int64_t)c->num_cu * 8);
        }
    }
    if (c->timing) FBN_HIP(hipEventRecord(S.ev0, s));
    CiArgs a{};
    a.cols = c->cols.as<uint8_t>(), a.dims = c->ddims.as<int32_t>();
    a.items = q.zc_items ? q.zc_items : S.items.as<int32_t>();
    a.N = c->N, a.n = n, a.alpha = q.alpha;
    a.g2 = want_g2p ? c->g2.as<double>() : nullptr;
    a.df = q.zc_df ? q.zc_df : S.df.as<int32_t>();
    a.p = want_g2p ? c->p.as<double>() : nullptr;
    a.indep = q.zc_indep ? q.zc_indep : S.indep.as<uint8_t>();
    a.counts = q.counts_dev, a.cstride = c->counts_stride;
    a.gscratch = gscratch;
    a.stats = c->stats.as<unsigned long long>();
    a.bits = bitsn ? c->bits.as<uint32_t>() : nullptr;
    a.row0 = c->brow.as<int32_t>(), a.W = c->bits_W;
    a.band = hband, a.nband = hnband;
    a.pk = pk ? c->pack2.as<uint32_t>() : nullptr, a.PW = c->pack2_W;
    a.tab = tab, a.tstride = tstride, a.split = split;
    a.pairtab = der2 ? c->pairtab.as<int32_t>() : nullptr;
    a.nvars = c->nvars;
    hipError_t e = fbn_ci_launch(&a, d, lds, grid, split_grid, s);
    if (e != hipSuccess) return SetError(FBN_ERR_HIP, "ci kernel launch: %s", hipGetErrorString(e));
    if (c->timing) FBN_HIP(hipEventRecord(S.ev1, s));
    return FBN_OK;
}

int CiLaunchDevice(fbn_ci_ctx *c, const CiBatchReq &q, hipStream_t s) {
    if (q.d < 0 || q.d > 8) return SetError(FBN_ERR_LIMIT, "conditioning set size %d (supported 0..8)", q.d);
    const int w = 2 + q.d;
    // one validation pass: variable ranges and the largest state count (bit-sliced eligibility)
    // (skipped for batches generated by the driver from the skeleton, which pass the same figures)
    int maxdim = 0;
    int64_t dim_rows = 0;  // sum of the items' state counts (bit-sliced input bytes)
    const int *dims = c->dims.data();
    if (q.pre) {
        maxdim = q.pre->maxdim, dim_rows = q.pre->dim_rows;
    } else {
        for (int64_t i = 0; i < q.n * w; ++i) {
            const int v = q.items[i];
            if ((unsigned)v >= (unsigned)c->nvars)
                return SetError(FBN_ERR_ARG, "test %lld: variable %d out of range", (long long)(i / w), v);
            maxdim = std::max(maxdim, dims[v]);
            dim_rows += dims[v];
        }
    }
    if (q.d <= 1 && CiBitsEligible(c, maxdim)) return CiLaunchBits(c, q, dim_rows, s);
    if (q.all_pairs) return SetError(FBN_ERR_ARG, "implicit pair batches need the bit-sliced path");
    return CiLaunchHist(c, q, maxdim, s);
}

}  // namespace fbn

extern "C" {

int fbn_ci_run(fbn_ci_ctx *c, const int32_t *items, int64_t n, int d, double alpha, double *g2, int32_t *df, double *p,
               uint8_t *indep, void *hip_stream) {
    if (!c || (!items && n > 0) || n < 0) return SetError(FBN_ERR_ARG, "bad argument");
    if (n == 0) return FBN_OK;
    FBN_HIP(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (std::find(c->streams_used.begin(), c->streams_used.end(), s) == c->streams_used.end())
        c->streams_used.push_back(s);
    fbn::CiBatchReq q;
    q.items = items, q.n = n, q.d = d, q.alpha = alpha;
    q.want_g2p = g2 || p;
    int rc = fbn::CiLaunchDevice(c, q, s);
    if (rc) return rc;
    if (g2) FBN_HIP(hipMemcpyAsync(g2, c->g2.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    if (p) FBN_HIP(hipMemcpyAsync(p, c->p.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    if (df) FBN_HIP(hipMemcpyAsync(df, c->slot[0].df.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (indep) FBN_HIP(hipMemcpyAsync(indep, c->slot[0].indep.p, (size_t)n, hipMemcpyDeviceToHost, s));
    FBN_HIP(hipStreamSynchronize(s));
    c->last_ms = 0.f;
    if (c->timing) FBN_HIP(hipEventElapsedTime(&c->last_ms, c->slot[0].ev0, c->slot[0].ev1));
    return FBN_OK;
}

int fbn_ci_counts(fbn_ci_ctx *c, int x, int y, const int32_t *z, int d, int32_t *counts, int64_t cap, int64_t *cells) {
    if (!c || (!z && d > 0) || d < 0 || d > 8) return SetError(FBN_ERR_ARG, "bad argument");
    std::vector<int32_t> item{x, y};
    for (int j = 0; j < d; ++j) item.push_back(z[j]);
    for (int32_t v : item)
        if (v < 0 || v >= c->nvars) return SetError(FBN_ERR_ARG, "variable out of range");
    int rc;
    int64_t dimz = 0;
    if ((rc = fbn::CiTableCheck(c, item.data(), d, 0, &dimz, nullptr))) return rc;
    const int64_t nc = dimz * c->dims[x] * c->dims[y];
    if (cells) *cells = nc;
    FBN_HIP(hipSetDevice(c->device));
    if ((rc = c->counts.ensure((size_t)nc * 4))) return rc;
    fbn::CiBatchReq q;
    q.items = item.data(), q.n = 1, q.d = d;
    q.counts_dev = c->counts.as<int32_t>();
    const hipStream_t null_stream = nullptr;
    rc = fbn::CiLaunchDevice(c, q, null_stream);
    if (rc) return rc;
    if (counts) FBN_HIP(hipMemcpy(counts, c->counts.p, (size_t)std::min(nc, cap) * 4, hipMemcpyDeviceToHost));
    FBN_HIP(hipDeviceSynchronize());
    return FBN_OK;
}

// a debug call must not change which path later batches on this ctx take: the pair mode (and
// with it the derived level-1 / level-2 counting) is restored on every exit
namespace {
struct PairModeGuard {
    fbn_ci_ctx *c;
    int mode;
    bool recorded;
    ~PairModeGuard() { c->pair_mode = mode, c->pairs_recorded = recorded; }
};
}  // namespace

// Counts of n tests through the kernels a PC run uses at level d (parity pinning of the production
// paths): d = 0 the complete-graph level-0 batch (the Gram of the leading mask rows, then every
// pair's table, recorded for level 1), d = 1 the derived counting from those recorded pair tables
// (the level-0 batch runs first if none are recorded), d >= 2 the histogram kernel over one batch.
// counts [n][cap]: test t's table in Counts3D order, cells beyond it untouched.
int fbn_ci_debug_counts(fbn_ci_ctx *c, const int32_t *items, int64_t n, int d, int32_t *counts, int64_t cap) {
    if (!c || (!items && n > 0) || n < 0 || d < 0 || d > 8 || (!counts && n > 0) || cap < 1)
        return SetError(FBN_ERR_ARG, "bad argument");
    if (n == 0) return FBN_OK;
    const int w = 2 + d;
    for (int64_t i = 0; i < n * w; ++i)
        if ((unsigned)items[i] >= (unsigned)c->nvars) return SetError(FBN_ERR_ARG, "variable out of range");
    FBN_HIP(hipSetDevice(c->device));
    int rc;
    const int nv = c->nvars;
    fbn::PCResultHost scratch;
    PairModeGuard guard{c, c->pair_mode, c->pairs_recorded};
    auto level0 = [&]() -> int {  // the PC run's level 0, pair tables recorded
        const fbn::CiBatchStats st = fbn::CiAllPairsStats(c->dims.data(), nv);
        if (!fbn::CiAllPairsEligible(c, st))
            return SetError(FBN_ERR_ARG, "dataset not eligible for the bit-sliced level-0 path");
        const int64_t P = (int64_t)nv * (nv - 1) / 2;
        fbn::CiSetPairMode(c, 1);
        int r = fbn::CiBatchLaunchAllPairs(c, 0.05, &st, 0, P);
        std::vector<uint8_t> flags((size_t)P);
        if (!r) r = fbn::CiBatchWait(c, 0, flags.data(), nullptr, scratch);
        if (!r) fbn::CiSetPairMode(c, 2);
        return r;
    };
    std::vector<int32_t> rec((size_t)n * 64);
    if (d == 0) {
        if ((rc = level0())) return rc;
        FBN_HIP(hipStreamSynchronize(c->stream));
        for (int64_t t = 0; t < n; ++t) {
            const int x = items[2 * t], y = items[2 * t + 1];
            if (x >= y) return SetError(FBN_ERR_ARG, "level-0 tests are pairs x < y");
            const int64_t pi = fbn::PairIndex(x, y, nv);
            FBN_HIP(hipMemcpy(rec.data() + t * 64, c->slot[0].bcounts.as<int32_t>() + pi * 64, 64 * 4,
                              hipMemcpyDeviceToHost));
        }
    } else if (d == 1) {
        if (!c->pairs_recorded && (rc = level0())) return rc;
        fbn::CiSetPairMode(c, 2);
        std::vector<uint8_t> ind((size_t)n);
        if ((rc = fbn::CiBatchLaunch(c, 0, items, n, 1, 0.05, false)) || (rc = fbn::CiBatchWait(c, 0, ind.data(), nullptr, scratch)))
            return rc;
        FBN_HIP(hipMemcpy(rec.data(), c->slot[0].bcounts.p, (size_t)n * 64 * 4, hipMemcpyDeviceToHost));
    }
    if (d <= 1) {
        for (int64_t t = 0; t < n; ++t) {
            int64_t cells = (int64_t)c->dims[items[w * t]] * c->dims[items[w * t + 1]];
            if (d == 1) cells *= c->dims[items[w * t + 2]];
            std::copy(rec.begin() + t * 64, rec.begin() + t * 64 + std::min<int64_t>(cells, cap), counts + t * cap);
        }
        return FBN_OK;
    }
    if (d == 2) {  // a PC run's level 2 has its level-0 pair tables (derived counting, ci_kernels.hip MODE 3)
        // (the rule of CiBitsEligible without its knobs: with FBN_CI_NO_BITS this call refuses, as it
        // always has, where the knob-reading form would fall through to the plain histogram)
        const int maxdim = *std::max_element(c->dims.begin(), c->dims.end());
        if (!c->pairs_recorded && maxdim <= 4 && c->N >= fbn::kCiBitsMinSamples && (rc = level0())) return rc;
        if (c->pairs_recorded) fbn::CiSetPairMode(c, 2);
    }
    for (int64_t t = 0; t < n; ++t) {  // the kernel writes every cell of a table: each must fit its row
        int64_t dimz = 0;
        if ((rc = fbn::CiTableCheck(c, items + w * t, d, t, &dimz, nullptr))) return rc;
        const int64_t cells = dimz * c->dims[items[w * t]] * c->dims[items[w * t + 1]];
        if (cells > cap)
            return SetError(FBN_ERR_ARG, "test %lld: %lld cells exceed cap %lld", (long long)t, (long long)cells,
                            (long long)cap);
    }
    if ((rc = c->counts.ensure((size_t)n * cap * 4))) return rc;
    FBN_HIP(hipMemsetAsync(c->counts.p, 0, (size_t)n * cap * 4, c->stream));  // cells beyond a table: 0
    c->counts_stride = cap;
    fbn::CiBatchReq q;
    q.items = items, q.n = n, q.d = d;
    q.counts_dev = c->counts.as<int32_t>();
    rc = fbn::CiLaunchDevice(c, q, c->stream);
    c->counts_stride = 0;
    if (rc) return rc;
    FBN_HIP(hipStreamSynchronize(c->stream));
    FBN_HIP(hipMemcpy(counts, c->counts.p, (size_t)n * cap * 4, hipMemcpyDeviceToHost));
    return FBN_OK;
}

int fbn_ci_level0_info(const fbn_ci_ctx *c, int64_t out[8]) {
    if (!c || !out) return SetError(FBN_ERR_ARG, "null pointer");
    std::copy(c->l0_info, c->l0_info + 8, out);
    return FBN_OK;
}

// The complete-graph pairs [pair0, pair0 + n) as one batch of the PC driver's level-0 chunk loop
// (pair tables recorded); counts [n][16]: pair pair0 + t's table, cells beyond it 0.  The level-0
// Gram is filled with 0xFF bytes first, so an entry the Gram kernels leave unwritten reads as -1
// (a wrong count) instead of a stale value of an earlier launch or context.
int fbn_ci_debug_level0_range(fbn_ci_ctx *c, int64_t pair0, int64_t n, int32_t *counts) {
    if (!c || n < 0 || (!counts && n > 0)) return SetError(FBN_ERR_ARG, "bad argument");
    const int nv = c->nvars;
    const int64_t P = (int64_t)nv * (nv - 1) / 2;
    if (pair0 < 0 || pair0 > P || n > P - pair0)
        return SetError(FBN_ERR_ARG, "pairs [%lld, %lld) outside the complete graph's %lld", (long long)pair0,
                        (long long)(pair0 + n), (long long)P);
    if (n == 0) return FBN_OK;
    FBN_HIP(hipSetDevice(c->device));
    PairModeGuard guard{c, c->pair_mode, c->pairs_recorded};
    const fbn::CiBatchStats st = fbn::CiAllPairsStats(c->dims.data(), nv);
    int64_t R = 0;
    for (int v = 0; v < nv; ++v) R += c->dims[v] - 1;
    if (!fbn::CiAllPairsEligible(c, st))
        return SetError(FBN_ERR_ARG, "dataset not eligible for the bit-sliced level-0 path");
    int rc;
    if (fbn::CiGram0Eligible(c)) {
        if ((rc = c->gram0.ensure((size_t)(R * R * 4)))) return rc;
        FBN_HIP(hipMemsetAsync(c->gram0.p, 0xFF, (size_t)(R * R * 4), c->stream));
    }
    fbn::PCResultHost scratch;
    std::vector<uint8_t> flags((size_t)n);
    fbn::CiSetPairMode(c, 1);
    if ((rc = fbn::CiBatchLaunchAllPairs(c, 0.05, &st, pair0, n)) ||
        (rc = fbn::CiBatchWait(c, 0, flags.data(), nullptr, scratch)))
        return rc;
    FBN_HIP(hipStreamSynchronize(c->stream));
    std::vector<int32_t> rec((size_t)n * 64);
    FBN_HIP(hipMemcpy(rec.data(), c->slot[0].bcounts.p, rec.size() * 4, hipMemcpyDeviceToHost));
    int x = fbn::PairRow(pair0, nv);
    int y = x + 1 + (int)(pair0 - fbn::PairIndex(x, x + 1, nv));
    for (int64_t t = 0; t < n; ++t) {
        const int cells = c->dims[x] * c->dims[y];
        std::fill(std::copy(rec.begin() + t * 64, rec.begin() + t * 64 + cells, counts + t * 16), counts + t * 16 + 16, 0);
        if (++y == nv) ++x, y = x + 1;
    }
    return FBN_OK;
}

int fbn_ci_decision_margin(fbn_ci_ctx *c, double *min_margin, int64_t *near_alpha, int reset) {
    if (!c) return SetError(FBN_ERR_ARG, "null pointer");
    FBN_HIP(hipSetDevice(c->device));
    int rc = fbn::CiReadMargin(c, min_margin, near_alpha);
    if (rc == FBN_OK && reset) rc = fbn::CiResetMargin(c);
    return rc;
}

int fbn_pc_decision_margin(const fbn_pc_result *r, double *min_margin, int64_t *near_alpha) {
    if (!r) return SetError(FBN_ERR_ARG, "null pointer");
    if (min_margin) *min_margin = r->r.min_margin;
    if (near_alpha) *near_alpha = r->r.near_alpha;
    return FBN_OK;
}

int fbn_ci_last_kernel_ms(const fbn_ci_ctx *c, float *ms) {
    if (!c || !ms) return SetError(FBN_ERR_ARG, "null pointer");
    *ms = c->last_ms;
    return FBN_OK;
}

int fbn_ci_ctx_destroy(fbn_ci_ctx *c) {
    if (!c) return FBN_OK;
    // nothing of this ctx may still run when its buffers, pinned records and stream go: the device-
    // resident search returns on its completion word, and batches may be queued on caller streams
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (hipStream_t s : c->streams_used) (void)hipStreamSynchronize(s);
    delete c;
    return FBN_OK;
}

// ------------------------------------------------------------------ parameter learning
int fbn_param_family_sizes(int nvars, const int32_t *dims, const int32_t *parent_off, const int32_t *parents,
                           int64_t *family_off, int64_t *ncounts) {
    return fbn::ParamFamilySizes(nvars, dims, parent_off, parents, family_off, ncounts);
}

int fbn_pdag_to_dag(int nvars, const int32_t *triples, int n, int32_t *parent_off, int32_t *parents) {
    return fbn::PdagToDag(nvars, triples, n, parent_off, parents);
}

int fbn_param_set_tuning(fbn_ci_ctx *c, int64_t samples_per_slice, int64_t lds_cells_max) {
    if (!c) return SetError(FBN_ERR_ARG, "null pointer");
    if (samples_per_slice < 0) return SetError(FBN_ERR_ARG, "samples_per_slice = %lld is negative", (long long)samples_per_slice);
    c->par_slice = samples_per_slice;
    c->par_lds = lds_cells_max;
    return FBN_OK;
}

int fbn_param_counts(fbn_ci_ctx *c, const int32_t *parent_off, const int32_t *parents, int64_t *counts, int64_t cap,
                     int64_t *ncounts) {
    if (!c || !parent_off) return SetError(FBN_ERR_ARG, "null pointer");
    const int V = c->nvars;
    // everything that can be refused is refused here, on the host, before any launch
    std::vector<int64_t> foff((size_t)V + 1);
    int64_t total = 0;
    int rc = fbn::ParamFamilySizes(V, c->dims.data(), parent_off, parents, foff.data(), &total);
    if (rc) return rc;
    if (ncounts) *ncounts = total;
    if (!counts) return FBN_OK;
    if (cap < total) return SetError(FBN_ERR_ARG, "counts holds %lld cells, %lld needed", (long long)cap, (long long)total);
    if (c->N >= (1ll << 31)) return SetError(FBN_ERR_LIMIT, "%lld samples: the device accumulators are 32-bit", (long long)c->N);
    int64_t slice = c->par_slice;
    if (slice <= 0) slice = fbn_param_default_slice(c->N, c->num_cu, V);
    const int64_t nslices = (c->N + slice - 1) / slice;
    if ((int64_t)V * nslices > 0x7fffffffll)
        return SetError(FBN_ERR_LIMIT, "%d families x %lld slices exceed one launch", V, (long long)nslices);
    const int lds_max = c->par_lds == 0 ? kParamLdsCellsMax : (int)std::max<int64_t>(0, std::min<int64_t>(c->par_lds, kParamLdsCellsMax));
    // family descriptors: the node's column first (stride = parent configurations), then its parents
    // ascending, the last one fastest
    std::vector<FbnParamFamily> fam((size_t)V);
    std::vector<int32_t> fcol((size_t)parent_off[V] + V), fstr(fcol.size());
    size_t lds_ints = 1;
    for (int v = 0, o = 0; v < V; ++v) {
        std::vector<int32_t> ps(parents + parent_off[v], parents + parent_off[v + 1]);
        std::sort(ps.begin(), ps.end());
        const int k = (int)ps.size();
        const int64_t cells = foff[v + 1] - foff[v];
        fam[v] = FbnParamFamily{(long long)foff[v], o, k + 1, (int32_t)cells, 0};
        int64_t str = 1;
        for (int j = k - 1; j >= 0; --j) {
            fcol[o + 1 + j] = ps[j];
            fstr[o + 1 + j] = (int32_t)str;
            str *= c->dims[ps[j]];
        }
        fcol[o] = v;
        fstr[o] = (int32_t)str;  // = cells / dims[v]
        o += k + 1;
        if (cells <= lds_max) lds_ints = std::max(lds_ints, fbn_param_lds_ints((int)cells));
    }
    FBN_HIP(hipSetDevice(c->device));
    if ((rc = c->par_fam.ensure(fam.size() * sizeof(FbnParamFamily))) || (rc = c->par_col.ensure(fcol.size() * 4)) ||
        (rc = c->par_str.ensure(fstr.size() * 4)) || (rc = c->par_tab.ensure((size_t)total * 4)))
        return rc;
    hipStream_t s = c->stream;
    CiSlot &S = c->slot[0];
    std::vector<uint32_t> h((size_t)total);
    fbn::StreamDrain drain(s);  // after fam, fcol, fstr and h: an early return waits for the copies that use them
    FBN_HIP(hipMemcpyAsync(c->par_fam.p, fam.data(), fam.size() * sizeof(FbnParamFamily), hipMemcpyHostToDevice, s));
    FBN_HIP(hipMemcpyAsync(c->par_col.p, fcol.data(), fcol.size() * 4, hipMemcpyHostToDevice, s));
    FBN_HIP(hipMemcpyAsync(c->par_str.p, fstr.data(), fstr.size() * 4, hipMemcpyHostToDevice, s));
    if (c->timing) FBN_HIP(hipEventRecord(S.ev0, s));
    FBN_HIP(hipMemsetAsync(c->par_tab.p, 0, (size_t)total * 4, s));  // every call: no earlier call's counts
    hipError_t e = fbn_param_launch(c->cols.as<uint8_t>(), c->N, c->par_fam.as<FbnParamFamily>(), V, c->par_col.as<int32_t>(),
                                    c->par_str.as<int32_t>(), c->par_tab.as<uint32_t>(), slice, nslices, lds_max,
                                    lds_ints * 4, s);
    if (e != hipSuccess) return SetError(FBN_ERR_HIP, "param counts launch: %s", hipGetErrorString(e));
    if (c->timing) FBN_HIP(hipEventRecord(S.ev1, s));
    FBN_HIP(hipMemcpyAsync(h.data(), c->par_tab.p, (size_t)total * 4, hipMemcpyDeviceToHost, s));
    FBN_HIP(hipStreamSynchronize(s));
    drain.done();
    c->last_ms = 0.f;
    if (c->timing) FBN_HIP(hipEventElapsedTime(&c->last_ms, S.ev0, S.ev1));
    for (int64_t i = 0; i < total; ++i) counts[i] = (int64_t)h[i];
    return FBN_OK;
}

int fbn_param_learn(fbn_ci_ctx *c, const int32_t *parent_off, const int32_t *parents, const char *const *names,
                    fbn_network **out) {
    if (!c || !parent_off || !out) return SetError(FBN_ERR_ARG, "null pointer");
    int64_t total = 0;
    int rc = fbn_param_counts(c, parent_off, parents, nullptr, 0, &total);
    if (rc) return rc;
    // BuildNetwork's own limits first (1..127 states), so a graph it would refuse costs no launch
    for (int v = 0; v < c->nvars; ++v)
        if (c->dims[v] > 127) return SetError(FBN_ERR_LIMIT, "node %d has %d states (supported 1..127)", v, c->dims[v]);
    std::vector<int64_t> counts((size_t)total);
    if ((rc = fbn_param_counts(c, parent_off, parents, counts.data(), total, &total))) return rc;
    auto h = std::unique_ptr<fbn_network>(new (std::nothrow) fbn_network());
    if (!h) return SetError(FBN_ERR_NOMEM, "out of memory");
    if ((rc = fbn::BuildNetwork(c->nvars, c->dims.data(), parent_off, parents, counts.data(), names, h->net))) return rc;
    *out = h.release();
    return FBN_OK;
}

}  // extern "C"
