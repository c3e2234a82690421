// ci_bits_count.hip -- the bit-sliced column store and the contingency counts of G^2 tests with at
// most one conditioning variable, gfx950.
//
// The level-0 sweep tests every pair of variables (499,500 tests at 1000 variables), each a
// 2-D contingency table N[x][y] over all samples (Counts2D::FillTable, src/CellTable.cpp:430-455).
// Instead of re-reading two byte columns and binning sample by sample, every column is stored
// once as one bit mask per value (bit s of mask (v, a) = [sample s of v has value a], 32 samples
// per word): N[a][b] = sum over words of popcount(mask(x, a) & mask(y, b)).  One wave per test,
// lanes stride over the words, one v_bcnt (popcount + accumulate) per cell per 32 samples; the
// masks are 1/8 of the byte columns per value (HBM / Infinity-cache traffic per test: (dx + dy
// [+ dz]) rows of N/8 bytes), counts are exact integers.  Level 1 (one conditioning variable z)
// adds z's masks: N[c][a][b] = sum popcount(x_a & y_b & z_c) (Counts3D, src/CellTable.cpp:226-291).
//
// Every test's table goes to a 64-slot record; ci_bits_g2.hip evaluates G^2 and the decision from it.
// (The row Gram, level 0's other way to the same records: ci_bits_gram.hip.)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ci_bits.h"
#include "ci_wave.h"
#include "fbn_device.h"
#include "launchers.h"

namespace {

// bits[(row0[v] + a) * W + w]: samples 32w .. 32w+31 of variable v equal to a
__global__ __launch_bounds__(256) void ci_bits_build(const uint8_t *__restrict__ cols, const int32_t *__restrict__ dims,
                                                     const int32_t *__restrict__ row0, long long N, long long W,
                                                     int nvars, uint32_t *__restrict__ bits) {
    const long long total = (long long)nvars * W;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const int v = (int)(t / W);
        const long long w = t % W;
        const uint8_t *c = cols + (size_t)v * N + 32 * w;
        const int n = (int)((N - 32 * w) < 32 ? (N - 32 * w) : 32);
        uint32_t m[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const int d = dims[v];
        for (int s = 0; s < n; ++s) {
            const int a = c[s];
#pragma unroll
            for (int k = 0; k < 8; ++k) m[k] |= (a == k ? 1u : 0u) << s;
        }
        for (int a = 0; a < d; ++a) bits[(size_t)(row0[v] + a) * W + w] = m[a];
    }
}

// counts of one test: N[z][a][b] += popcount(x_a & y_b & z_c) over this lane's words, then a
// wave reduction; cells (c * DX + a) * DY + b (Counts3D layout, src/CellTable.cpp:277-281).
// DZ = 1 for marginal tests; conditional tests (one conditioning variable) use DZ = 4 with the
// masks of absent values zero (their cells stay 0 and are never read).
template <int DX, int DY, int DZ>
__device__ __forceinline__ void count_test(const uint32_t *__restrict__ bx, const uint32_t *__restrict__ by,
                                           const uint32_t *__restrict__ bz, int dz, long long W, int lane,
                                           int32_t *__restrict__ out) {
    constexpr int NC = DX * DY * DZ;
    uint32_t cnt[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) cnt[c] = 0u;
    // four consecutive words per lane per step, one 16-byte load per mask row (W is a multiple
    // of 4, padding words are zero)
    typedef __attribute__((ext_vector_type(4))) unsigned u4;
    auto quad = [&](long long w4) {
        u4 x[DX], y[DY], z[DZ];
#pragma unroll
        for (int a = 0; a < DX; ++a) x[a] = *reinterpret_cast<const u4 *>(bx + a * W + 4 * w4);
#pragma unroll
        for (int b = 0; b < DY; ++b) y[b] = *reinterpret_cast<const u4 *>(by + b * W + 4 * w4);
#pragma unroll
        for (int c = 0; c < DZ; ++c) {
            if (DZ == 1) z[c] = u4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
            else z[c] = c < dz ? *reinterpret_cast<const u4 *>(bz + c * W + 4 * w4) : u4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int a = 0; a < DX; ++a)
#pragma unroll
                for (int b = 0; b < DY; ++b) {
                    const uint32_t xy = x[a][k] & y[b][k];
#pragma unroll
                    for (int c = 0; c < DZ; ++c) cnt[(c * DX + a) * DY + b] += __builtin_popcount(xy & z[c][k]);
                }
    };
    for (long long w4 = lane; 4 * w4 < W; w4 += 64) quad(w4);
#pragma unroll
    for (int c = 0; c < NC; ++c) cnt[c] = wave_sum(cnt[c]);
    const int ncells = DX * DY * (DZ == 1 ? 1 : dz);
    if (lane < ncells) out[lane] = (int32_t)lane_select(lane, cnt);
}

// marginal test N[a][b] from (DX-1)(DY-1) popcounts per word, the last value's row and column
// derived from the per-value sample counts nx / ny (complete_pair); only DX-1 and DY-1 mask rows are read
template <int DX, int DY>
__device__ __forceinline__ void count_pair(const uint32_t *__restrict__ bx, const uint32_t *__restrict__ by,
                                           const int32_t *__restrict__ nx, const int32_t *__restrict__ ny,
                                           long long W, int lane, int32_t *__restrict__ out,
                                           int32_t *__restrict__ rec) {
    constexpr int MX = DX - 1, MY = DY - 1, NC = MX * MY > 0 ? MX * MY : 1;
    uint32_t cnt[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) cnt[c] = 0u;
    if (MX > 0 && MY > 0) {
        typedef __attribute__((ext_vector_type(4))) unsigned u4;
        for (long long w4 = lane; 4 * w4 < W; w4 += 64) {
            u4 x[MX > 0 ? MX : 1], y[MY > 0 ? MY : 1];
#pragma unroll
            for (int a = 0; a < MX; ++a) x[a] = *reinterpret_cast<const u4 *>(bx + a * W + 4 * w4);
#pragma unroll
            for (int b = 0; b < MY; ++b) y[b] = *reinterpret_cast<const u4 *>(by + b * W + 4 * w4);
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int a = 0; a < MX; ++a)
#pragma unroll
                    for (int b = 0; b < MY; ++b) cnt[a * MY + b] += __builtin_popcount(x[a][k] & y[b][k]);
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) cnt[c] = wave_sum(cnt[c]);
    }
    // every lane now holds the wave totals: complete the table with the marginals
    int32_t full[DX * DY];
    complete_pair<DX, DY>([&](int a, int b) { return (int32_t)cnt[a * MY + b]; }, nx, ny, full);
    lane_store(lane, full, out, rec);
}

// conditional test N[c][a][b] (one conditioning variable z) from (DZ-1)(DX-1)(DY-1) popcounts per
// word: the pair tables N_xy, N_xz, N_yz this run's level 0 recorded (every pair of the complete
// graph, table of (u < v) stored [value of u][value of v]) give the last value of each variable
// exactly -- N[c][a][DY-1] = N_xz[a][c] - sum_b, N[c][DX-1][b] = N_yz[b][c] - sum_a,
// N[DZ-1][a][b] = N_xy[a][b] - sum_c; only DX-1, DY-1, DZ-1 mask rows are read.
// derived_finish: the wave totals of the leading cells (butterfly) and the derived rest of the table
// (written out, not through complete_pair: its marginals are transposable table lookups, not two count rows)
template <int DX, int DY, int DZ>
__device__ __forceinline__ void derived_finish(uint32_t (&cnt)[(DX - 1) * (DY - 1) * (DZ - 1) > 0 ? (DX - 1) * (DY - 1) * (DZ - 1) : 1],
                                               const int32_t *__restrict__ Txy, bool txy,
                                               const int32_t *__restrict__ Txz, bool txz,
                                               const int32_t *__restrict__ Tyz, bool tyz,
                                               int32_t (&full)[DZ * DX * DY]) {
    constexpr int MX = DX - 1, MY = DY - 1, MZ = DZ - 1, M = MX * MY * MZ, NC = M > 0 ? M : 1;
    if (M > 0) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {  // (wave_sum written out: ci_bits_count_derived's code stays as it was)
            uint32_t v = cnt[c];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
            cnt[c] = v;
        }
    }
    auto nxy = [&](int a, int b) { return txy ? Txy[b * DX + a] : Txy[a * DY + b]; };
    auto nxz = [&](int a, int c) { return txz ? Txz[c * DX + a] : Txz[a * DZ + c]; };
    auto nyz = [&](int b, int c) { return tyz ? Tyz[c * DY + b] : Tyz[b * DZ + c]; };
#pragma unroll
    for (int c = 0; c < MZ; ++c) {
#pragma unroll
        for (int a = 0; a < MX; ++a) {
            int32_t r = nxz(a, c);
#pragma unroll
            for (int b = 0; b < MY; ++b) {
                const int32_t v = (int32_t)cnt[(c * MX + a) * MY + b];
                full[(c * DX + a) * DY + b] = v;
                r -= v;
            }
            full[(c * DX + a) * DY + MY] = r;
        }
#pragma unroll
        for (int b = 0; b < DY; ++b) {
            int32_t r = nyz(b, c);
#pragma unroll
            for (int a = 0; a < MX; ++a) r -= full[(c * DX + a) * DY + b];
            full[(c * DX + MX) * DY + b] = r;
        }
    }
#pragma unroll
    for (int a = 0; a < DX; ++a)
#pragma unroll
        for (int b = 0; b < DY; ++b) {
            int32_t r = nxy(a, b);
#pragma unroll
            for (int c = 0; c < MZ; ++c) r -= full[(c * DX + a) * DY + b];
            full[(MZ * DX + a) * DY + b] = r;
        }
}

template <int DX, int DY, int DZ>
__device__ __forceinline__ void count_test_derived_full(const uint32_t *__restrict__ bx,
                                                        const uint32_t *__restrict__ by,
                                                        const uint32_t *__restrict__ bz, long long W, int lane,
                                                        const int32_t *__restrict__ Txy, bool txy,
                                                        const int32_t *__restrict__ Txz, bool txz,
                                                        const int32_t *__restrict__ Tyz, bool tyz,
                                                        int32_t (&full)[DZ * DX * DY]) {
    constexpr int MX = DX - 1, MY = DY - 1, MZ = DZ - 1, M = MX * MY * MZ, NC = M > 0 ? M : 1;
    uint32_t cnt[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) cnt[c] = 0u;
    if (M > 0) {
        typedef __attribute__((ext_vector_type(4))) unsigned u4;
        for (long long w4 = lane; 4 * w4 < W; w4 += 64) {
            u4 x[MX > 0 ? MX : 1], y[MY > 0 ? MY : 1], z[MZ > 0 ? MZ : 1];
#pragma unroll
            for (int a = 0; a < MX; ++a) x[a] = *reinterpret_cast<const u4 *>(bx + a * W + 4 * w4);
#pragma unroll
            for (int b = 0; b < MY; ++b) y[b] = *reinterpret_cast<const u4 *>(by + b * W + 4 * w4);
#pragma unroll
            for (int c = 0; c < MZ; ++c) z[c] = *reinterpret_cast<const u4 *>(bz + c * W + 4 * w4);
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int a = 0; a < MX; ++a)
#pragma unroll
                    for (int b = 0; b < MY; ++b) {
                        const uint32_t xy = x[a][k] & y[b][k];
#pragma unroll
                        for (int c = 0; c < MZ; ++c) cnt[(c * MX + a) * MY + b] += __builtin_popcount(xy & z[c][k]);
                    }
        }
    }
    derived_finish<DX, DY, DZ>(cnt, Txy, txy, Txz, txz, Tyz, tyz, full);
}

template <int DX, int DY, int DZ>
__device__ __forceinline__ void count_test_derived(const uint32_t *__restrict__ bx, const uint32_t *__restrict__ by,
                                                   const uint32_t *__restrict__ bz, long long W, int lane,
                                                   int32_t *__restrict__ out, const int32_t *__restrict__ Txy, bool txy,
                                                   const int32_t *__restrict__ Txz, bool txz,
                                                   const int32_t *__restrict__ Tyz, bool tyz) {
    int32_t full[DZ * DX * DY];
    count_test_derived_full<DX, DY, DZ>(bx, by, bz, W, lane, Txy, txy, Txz, txz, Tyz, tyz, full);
    if (lane < DZ * DX * DY) {  // (lane_store written out: ci_bits_count_derived's code stays as it was)
        int32_t v = 0;
#pragma unroll
        for (int c = 0; c < DZ * DX * DY; ++c) v = lane == c ? full[c] : v;
        out[lane] = v;
    }
}

// ---- register-blocked marginal tests (a PC run's level 0, all pairs of a pair-index range)
// One wave per task = a block of BX x-variables x BY y-variables of one state-count class each
// (tasks built on the host, CiPairTasks in capi_ci.hip): per 4-word step every mask row of the block's
// variables is loaded once and feeds every pair of the block, so L2 / fabric traffic per pair drops
// from (dx-1 + dy-1) rows to (BX (dx-1) + BY (dy-1)) / (BX BY) rows.  A pair is the block's
// (x, y) with x < y and its index in [t0, t1) (each pair of the range exactly once); the counts
// and the derived last row / column are exactly count_pair's (Counts2D, src/CellTable.cpp:430-455).
template <int DX, int DY>
struct PairBlock {
    static constexpr int MX = DX - 1, MY = DY - 1;
    static constexpr int BX = MX <= 1 ? 4 : (MX == 2 ? 3 : 2), BY = MY <= 1 ? 4 : (MY == 2 ? 3 : 2);
    static constexpr int NCC = MX * MY > 0 ? MX * MY : 1;
};
constexpr int kPairTaskInts = 12;  // dx, dy, nx, ny, xs[4], ys[4]

template <int DX, int DY>
__device__ __forceinline__ void pair_block(const uint32_t *__restrict__ bits, const int32_t *__restrict__ row0,
                                           const int32_t *__restrict__ rowcnt, long long W,
                                           const int32_t *__restrict__ task, int nvars, long long t0, long long t1,
                                           int32_t *__restrict__ counts, int32_t *__restrict__ pairtab, int lane) {
    using PB = PairBlock<DX, DY>;
    constexpr int MX = PB::MX, MY = PB::MY, BX = PB::BX, BY = PB::BY, NCC = PB::NCC;
    const int nx = task[2], ny = task[3];
    int xs[BX], ys[BY];
#pragma unroll
    for (int a = 0; a < BX; ++a) xs[a] = task[4 + (a < nx ? a : 0)];  // padding repeats the first
#pragma unroll
    for (int b = 0; b < BY; ++b) ys[b] = task[8 + (b < ny ? b : 0)];
    uint32_t cnt[BX][BY][NCC];
#pragma unroll
    for (int a = 0; a < BX; ++a)
#pragma unroll
        for (int b = 0; b < BY; ++b)
#pragma unroll
            for (int c = 0; c < NCC; ++c) cnt[a][b][c] = 0u;
    if (MX > 0 && MY > 0) {
        typedef __attribute__((ext_vector_type(4))) unsigned u4;
        const uint32_t *px[BX], *py[BY];
#pragma unroll
        for (int a = 0; a < BX; ++a) px[a] = bits + (size_t)row0[xs[a]] * W;
#pragma unroll
        for (int b = 0; b < BY; ++b) py[b] = bits + (size_t)row0[ys[b]] * W;
        for (long long w4 = lane; 4 * w4 < W; w4 += 64) {
            u4 xv[BX][MX > 0 ? MX : 1], yv[BY][MY > 0 ? MY : 1];
#pragma unroll
            for (int a = 0; a < BX; ++a)
#pragma unroll
                for (int r = 0; r < MX; ++r) xv[a][r] = *reinterpret_cast<const u4 *>(px[a] + r * W + 4 * w4);
#pragma unroll
            for (int b = 0; b < BY; ++b)
#pragma unroll
                for (int r = 0; r < MY; ++r) yv[b][r] = *reinterpret_cast<const u4 *>(py[b] + r * W + 4 * w4);
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int a = 0; a < BX; ++a)
#pragma unroll
                    for (int r = 0; r < MX; ++r)
#pragma unroll
                        for (int b = 0; b < BY; ++b)
#pragma unroll
                            for (int q = 0; q < MY; ++q) cnt[a][b][r * MY + q] += __builtin_popcount(xv[a][r][k] & yv[b][q][k]);
        }
#pragma unroll
        for (int a = 0; a < BX; ++a)
#pragma unroll
            for (int b = 0; b < BY; ++b)
#pragma unroll
                for (int c = 0; c < NCC; ++c) cnt[a][b][c] = wave_sum(cnt[a][b][c]);
    }
#pragma unroll
    for (int a = 0; a < BX; ++a)
#pragma unroll
        for (int b = 0; b < BY; ++b) {
            const int x = xs[a], y = ys[b];
            const int u = x < y ? x : y, v = x < y ? y : x;
            // (fbn_pair_index written out: through the helper this kernel's register allocation changes)
            const long long t = (long long)u * nvars - (long long)u * (u + 1) / 2 + (v - u - 1);
            if (!(a < nx && b < ny && x < y && t >= t0 && t < t1)) continue;  // wave-uniform
            int32_t full[DX * DY];
            complete_pair<DX, DY>([&](int i, int j) { return (int32_t)cnt[a][b][i * MY + j]; }, rowcnt + row0[x],
                                  rowcnt + row0[y], full);
            // x < y here: the table is N[value of x][value of y] (Counts2D of the pair (u, v))
            lane_store(lane, full, counts + (t - t0) * kBitsCells, pairtab ? pairtab + 16 * t : nullptr);
        }
}

__global__ __launch_bounds__(256) void ci_bits_pairs_tiled(const uint32_t *__restrict__ bits,
                                                           const int32_t *__restrict__ row0,
                                                           const int32_t *__restrict__ rowcnt, long long W,
                                                           const int32_t *__restrict__ tasks, long long ntasks,
                                                           int nvars, long long t0, long long t1,
                                                           int32_t *__restrict__ counts, int32_t *__restrict__ pairtab) {
    const int lane = threadIdx.x & 63;
    for (long long k = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); k < ntasks; k += (long long)gridDim.x * 4) {
        const int32_t *task = tasks + k * kPairTaskInts;
        switch (task[0] * 8 + task[1]) {
#define FBN_PB(A, B)                                                                                       \
    case A * 8 + B:                                                                                        \
        pair_block<A, B>(bits, row0, rowcnt, W, task, nvars, t0, t1, counts, pairtab, lane);               \
        break;
            FBN_DIMS_4x4(FBN_PB)
#undef FBN_PB
        default: break;
        }
    }
}

// phase 1: counts[t][64] of every test, one wave per test; D = 0 (x, y) or 1 (x, y, z);
// items == nullptr for a marginal batch: test t is pair t0 + t of the complete graph (pair_of)
template <int D>
__global__ __launch_bounds__(256) void ci_bits_count(const uint32_t *__restrict__ bits, const int32_t *__restrict__ dims,
                                                     const int32_t *__restrict__ row0, const int32_t *__restrict__ items,
                                                     long long W, long long n, int32_t *__restrict__ counts,
                                                     const int32_t *__restrict__ rowcnt, int32_t *__restrict__ pairtab,
                                                     int nvars, long long t0) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    for (long long t = wave; t < n; t += (long long)gridDim.x * 4) {
        int x, y;
        if (D == 0 && !items) pair_of(t0 + t, nvars, x, y);
        else x = items[(2 + D) * t], y = items[(2 + D) * t + 1];
        const int dx = dims[x], dy = dims[y];
        const uint32_t *bx = bits + (size_t)row0[x] * W, *by = bits + (size_t)row0[y] * W;
        const uint32_t *bz = bx;
        int dz = 1;
        if (D == 1) {
            const int z = items[3 * t + 2];
            dz = dims[z];
            bz = bits + (size_t)row0[z] * W;
        }
        int32_t *out = counts + t * kBitsCells;
        constexpr int DZ = D == 1 ? 4 : 1;
        const int32_t *nx = rowcnt + row0[x], *ny = rowcnt + row0[y];
        // level 0 of a PC run records every pair's table (pair index of x < y, 16 slots)
        int32_t *rec = (D == 0 && pairtab && x < y)
                           ? pairtab + 16 * fbn_pair_index(x, y, nvars)
                           : nullptr;
        switch (dx * 8 + dy) {
#define FBN_PAIR(A, B)                                                             \
    case A * 8 + B:                                                                \
        if (D == 0) count_pair<A, B>(bx, by, nx, ny, W, lane, out, rec);           \
        else count_test<A, B, DZ>(bx, by, bz, dz, W, lane, out);                   \
        break;
            FBN_DIMS_4x4(FBN_PAIR)
#undef FBN_PAIR
        default: break;  // the host only routes tests with dims <= 4 here
        }
    }
}

// level >= 1 of a PC run, one conditioning variable, pair tables recorded: derived counting
__device__ __forceinline__ const int32_t *pair_table(const int32_t *pairtab, int nvars, int u, int v) {
    const int i = u < v ? u : v, j = u < v ? v : u;
    return pairtab + 16 * fbn_pair_index(i, j, nvars);
}

// n_dev != nullptr: the test count is read on the device (batches generated on the device)
__global__ __launch_bounds__(256) void ci_bits_count_derived(const uint32_t *__restrict__ bits,
                                                             const int32_t *__restrict__ dims,
                                                             const int32_t *__restrict__ row0,
                                                             const int32_t *__restrict__ items, long long W, long long n,
                                                             int32_t *__restrict__ counts,
                                                             const int32_t *__restrict__ pairtab, int nvars, int xcd,
                                                             const long long *__restrict__ n_dev) {
    const int lane = threadIdx.x & 63;
    const XcdSplit sp = xcd_split(n_dev ? *n_dev : n, threadIdx.x >> 6, 4, xcd);
    for (long long t = sp.first; t < sp.end; t += sp.stride) {
        const int x = items[3 * t], y = items[3 * t + 1], z = items[3 * t + 2];
        const int dx = dims[x], dy = dims[y], dz = dims[z];
        const uint32_t *bx = bits + (size_t)row0[x] * W, *by = bits + (size_t)row0[y] * W,
                       *bz = bits + (size_t)row0[z] * W;
        const int32_t *Txy = pair_table(pairtab, nvars, x, y), *Txz = pair_table(pairtab, nvars, x, z),
                      *Tyz = pair_table(pairtab, nvars, y, z);
        int32_t *out = counts + t * kBitsCells;
        switch (dz * 64 + dx * 8 + dy) {
#define FBN_TRIPLE(C, A, B)                                                                                  \
    case C * 64 + A * 8 + B:                                                                                 \
        count_test_derived<A, B, C>(bx, by, bz, W, lane, out, Txy, x > y, Txz, x > z, Tyz, y > z);          \
        break;
#define FBN_T1(A, B) FBN_TRIPLE(1, A, B)
#define FBN_T2(A, B) FBN_TRIPLE(2, A, B)
#define FBN_T3(A, B) FBN_TRIPLE(3, A, B)
#define FBN_T4(A, B) FBN_TRIPLE(4, A, B)
            FBN_DIMS_4x4(FBN_T1) FBN_DIMS_4x4(FBN_T2) FBN_DIMS_4x4(FBN_T3) FBN_DIMS_4x4(FBN_T4)
#undef FBN_T4
#undef FBN_T3
#undef FBN_T2
#undef FBN_T1
#undef FBN_TRIPLE
        default: break;
        }
    }
}

// bad[0] = 1 and bad[1] = v + 1 (some such v) if any code of variable v is >= dims[v]
__global__ __launch_bounds__(256) void ci_cols_check(const uint8_t *__restrict__ cols, const int32_t *__restrict__ dims,
                                                     int nvars, long long N, int *__restrict__ bad) {
    for (int v = blockIdx.y; v < nvars; v += gridDim.y) {
        const uint8_t *c = cols + (size_t)v * N;
        const int d = dims[v];
        bool b = false;
        for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < N; k += (long long)gridDim.x * 256)
            b |= c[k] >= d;
        if (b) {
            bad[0] = 1;
            bad[1] = v + 1;
        }
    }
}

// sample count of every mask row (variable v, value a): one wave per row
__global__ __launch_bounds__(256) void ci_bits_rowcount(const uint32_t *__restrict__ bits, long long rows,
                                                        long long W, int32_t *__restrict__ rowcnt) {
    const int lane = threadIdx.x & 63;
    for (long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (long long)gridDim.x * 4) {
        uint32_t v = 0;
        for (long long w = lane; w < W; w += 64) v += __builtin_popcount(bits[r * W + w]);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);  // (wave_sum written out: this kernel's code stays as it was)
        if (lane == 0) rowcnt[r] = (int32_t)v;
    }
}

// grid of one wave per unit, four per block, at most 8 blocks per CU
dim3 wave_grid(long long n, int num_cu) {
    const long long g = (n + 3) / 4, cap = (long long)num_cu * 8;
    return dim3((unsigned)(g < cap ? g : cap));
}

}  // namespace

extern "C" hipError_t fbn_ci_cols_check(const uint8_t *cols, const int32_t *dims, int nvars, long long N, int *bad,
                                        hipStream_t s) {
    const long long bx = (N + 255) / 256;
    const dim3 grid((unsigned)(bx < 16 ? bx : 16), (unsigned)(nvars < 4096 ? nvars : 4096));
    hipLaunchKernelGGL(ci_cols_check, grid, dim3(256), 0, s, cols, dims, nvars, N, bad);
    return hipGetLastError();
}

extern "C" hipError_t fbn_ci_bits_rowcount(const uint32_t *bits, long long rows, long long W, int32_t *rowcnt,
                                           hipStream_t s) {
    const long long g = (rows + 3) / 4;
    hipLaunchKernelGGL(ci_bits_rowcount, dim3((unsigned)(g < 4096 ? (g > 0 ? g : 1) : 4096)), dim3(256), 0, s, bits,
                       rows, W, rowcnt);
    return hipGetLastError();
}

extern "C" hipError_t fbn_ci_bits_build(const uint8_t *cols, const int32_t *dims, const int32_t *row0, long long N,
                                        long long W, int nvars, uint32_t *bits, hipStream_t s) {
    const long long total = (long long)nvars * W;
    const int grid = (int)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);
    hipLaunchKernelGGL(ci_bits_build, dim3(grid > 0 ? grid : 1), dim3(256), 0, s, cols, dims, row0, N, W, nvars, bits);
    return hipGetLastError();
}

// block size per state-count class (the host builds tasks with these)
extern "C" int fbn_ci_pair_block(int d) { return d - 1 <= 1 ? 4 : (d - 1 == 2 ? 3 : 2); }

extern "C" hipError_t fbn_ci_bits_pairs_tiled(const uint32_t *bits, const int32_t *row0, const int32_t *rowcnt,
                                              long long W, const int32_t *tasks, long long ntasks, int nvars,
                                              long long t0, long long t1, int32_t *counts, int32_t *pairtab,
                                              int num_cu, hipStream_t s) {
    if (ntasks > 0)
        hipLaunchKernelGGL(ci_bits_pairs_tiled, wave_grid(ntasks, num_cu), dim3(256), 0, s, bits, row0, rowcnt, W, tasks,
                           ntasks, nvars, t0, t1, counts, pairtab);
    return hipGetLastError();
}

// (xcd = 1: the XCD-contiguous split of the items)
hipError_t fbn::CiCountDerivedLaunch(const CiBitsArgs &a, const long long *n_dev, hipStream_t s) {
    hipLaunchKernelGGL(ci_bits_count_derived, wave_grid(a.n, a.num_cu), dim3(256), 0, s, a.bits, a.dims, a.row0, a.items,
                       a.W, a.n, a.counts, (const int32_t *)a.pairtab, a.nvars, 1, n_dev);
    return hipGetLastError();
}

extern "C" hipError_t fbn_ci_bits_launch(const CiBitsArgs *a, hipStream_t s) {
    if (a->d != 0 && a->d != 1) return hipErrorInvalidValue;
    const dim3 b1 = wave_grid(a->n, a->num_cu);
    if (a->d == 0) {
        if (!a->counted)  // counted = 1: the counts are already in place (ci_bits_pairs_tiled)
            hipLaunchKernelGGL(ci_bits_count<0>, b1, dim3(256), 0, s, a->bits, a->dims, a->row0, a->items, a->W, a->n,
                               a->counts, a->rowcnt, a->pmode == 1 ? a->pairtab : nullptr, a->nvars, a->t0);
    } else if (a->pmode == 2) {
        const hipError_t err = fbn::CiCountDerivedLaunch(*a, nullptr, s);
        if (err != hipSuccess) return err;
    } else {
        hipLaunchKernelGGL(ci_bits_count<1>, b1, dim3(256), 0, s, a->bits, a->dims, a->row0, a->items, a->W, a->n,
                           a->counts, a->rowcnt, nullptr, a->nvars, 0ll);
    }
    CiG2Args g{};
    g.counts = a->counts, g.dims = a->dims, g.items = a->items;
    g.n = a->n, g.t0 = a->d == 0 ? a->t0 : 0, g.nvars = a->nvars;
    g.alpha = a->alpha;
    g.g2 = a->g2, g.df = a->df, g.p = a->p, g.indep = a->indep, g.counts0 = a->counts0;
    g.stats = a->stats, g.band = a->band, g.nband = a->nband;
    // launches too small to fill the chip with a lane per test (ALARM's 8.7k level-1 tests: 137
    // waves on 1024 SIMDs) take four lanes per test, which cuts each test's latency chain ~4x
    return fbn::CiG2Launch(g, a->d, a->n <= kG2QuadMax, a->num_cu, s);
}
