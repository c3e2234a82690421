// ci_l1.hip -- the device-resident level-1 search of a PC run (group size 1) and the kept-edge CSR
// that feeds it, gfx950.
//
// Edge e = (x < y) of the level's range; its candidate k walks the combined list adj(x)\{y} then
// adj(y)\{x} in sorted order (CheckEdge's two sides, src/PCStable.cpp:402-470 with d = 1); pos =
// next candidate, st = 0 open / 1 removed (sep = z of its first independent test) / 2 kept
// (exhausted).  Every round takes the next `chunk` candidates of each open edge, counts and tests
// them (ci_bits_count_derived + ci_bits_g2q<1> with the test count read on the device) and resolves
// each edge's prefix in order: counted = tests up to and including the first independent one.  The
// host only enqueues rounds; nothing per test crosses PCIe.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "ci_bits.h"
#include "ci_wave.h"
#include "fbn_device.h"
#include "launchers.h"

namespace {

struct L1Edge {
    int32_t x, y, m0, L, skx, sky, ax, ay;  // ax / ay: adjacency offsets, skx / sky: position of y / x
    // the candidates the information screen keeps (below): P of them, positions plist[pl .. pl + P)
    // (pl = -1: no screen, every candidate k = its own position)
    int32_t P, pl;
};

// position of v in the sorted list a[0..n) (present by construction)
__device__ __forceinline__ int find_sorted(const int32_t *__restrict__ a, int n, int v) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] <= v) lo = mid;
        else hi = mid;
    }
    return lo < n && a[lo] == v ? lo : -1;
}

// ---- the information screen of level 1 (exact: it only skips tests whose answer is known)
// With empirical (plug-in) mutual information I over the same N samples, the chain rule holds
// exactly: I(X;Y) + I(X;Z|Y) = I(X;Z) + I(X;Y|Z), so I(X;Y) <= I(X;Z) + I(X;Y|Z) (and likewise for
// Y).  G^2 of a test is 2N I(X;Y|Z) (src/IndependenceTest.cpp:94-138: the sum of 2 O log(O / E)),
// and "independent" needs G^2 <= hi(df), the upper end of the decision band for its df (df <=
// (dx-1)(dy-1)dz; hi grows with df).  Hence a candidate z with
//     I(X;Z) < I(X;Y) - tau   or   I(Y;Z) < I(X;Y) - tau,   tau = hi((dx-1)(dy-1)dz) / 2N (+ margins)
// can never be the independent one: its test is dependent whatever its counts.  Level 1 runs only
// the other candidates; counted tests stay the reference's (every candidate up to the first
// independent one, src/PCStable.cpp:465-551), launched tests are the ones run.  The pairwise I come
// from the level-0 pair tables.  (The margins, 1e-9 relative on hi and 1e-9 absolute in nats, are
// orders above the rounding of either side: a few 1e-16 relative on values <= log 4.)
__device__ __forceinline__ long long l1_pidx(int u, int v, int nv) {
    const int i = u < v ? u : v, j = u < v ? v : u;
    return fbn_pair_index(i, j, nv);
}
// (in G^2 units: g2[pair] = 2N I of the pair's level-0 table; the margin 1e-9 nats = two_n * 1e-9)
__device__ __forceinline__ bool l1_plausible(const double *__restrict__ g2, int nv, const int32_t *__restrict__ dims,
                                             const double *__restrict__ band, int nband, double two_n, int x, int y,
                                             int z, double gxy) {
    const int df = (dims[x] - 1) * (dims[y] - 1) * dims[z];
    if (df <= 0 || df > nband) return true;
    const double lim = gxy - (band[2 * df - 1] * (1.0 + 1e-9) + two_n * 1e-9);
    if (lim <= 0.0) return true;
    return g2[l1_pidx(x, z, nv)] >= lim && g2[l1_pidx(y, z, nv)] >= lim;
}

// The rounds' test offsets: a single-pass exclusive scan of the edges' lengths inside the kernel
// that computes them (ci_l1_setup for round 0, ci_l1_resolve for the next round), 256-edge tiles
// taken in ticket order (so every earlier tile belongs to a running workgroup) with a decoupled
// look-back over the earlier tiles' published aggregates / prefixes, then the round's clip at cap
// (edges past it continue next round).  Status word per tile: epoch << 34 | flag << 32 | value
// (flag 1 = tile aggregate, 2 = inclusive prefix); the epoch (1 = setup, r + 2 = round r's resolve)
// makes stale words of earlier kernels invisible without a memset.  scal: [0] total, [1] launched,
// [2] rows read, [3] scan-timeout flag, then two ticket counters (kernel of epoch k uses k & 1 and
// zeroes the other for the next kernel).
constexpr long long kScanSpin = 1ll << 24;  // look-back spins before giving up (never reached)

__device__ __forceinline__ int l1_ticket(unsigned *tickets, unsigned epoch) {
    __shared__ int t_sh;
    if (threadIdx.x == 0) t_sh = (int)atomicAdd(tickets + (epoch & 1u), 1u);
    __syncthreads();
    const int t = t_sh;
    __syncthreads();
    return t;
}

// exclusive offset of this thread's edge (len: this round's length, clipped in place)
__device__ __forceinline__ int32_t l1_tile_scan(int tile, int ntiles, int32_t &len, unsigned long long *sstat,
                                                unsigned epoch, long long cap, long long *scal) {
    __shared__ int wsum[4];
    __shared__ long long ex_sh;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int v = len;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int wbase = 0, agg = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) wbase += k < w ? wsum[k] : 0, agg += wsum[k];
    if (w == 0) {  // wave 0: publish the aggregate, then look back 64 tiles at a time
        const unsigned long long tag = (unsigned long long)epoch << 34;
        long long ex = 0;
        if (tile > 0) {
            if (lane == 0)
                __hip_atomic_store(sstat + tile, tag | (1ull << 32) | (unsigned)agg, __ATOMIC_RELEASE,
                                   __HIP_MEMORY_SCOPE_AGENT);
            long long spins = 0;
            for (int j0 = tile - 1; j0 >= 0; j0 -= 64) {
                const int j = j0 - lane;  // lane l looks at tile j0 - l
                unsigned long long st = 0;
                for (;;) {  // until every looked-at tile has published
                    st = j >= 0 ? __hip_atomic_load(sstat + j, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)
                                : tag | (2ull << 32);
                    if (__ballot((st >> 34) != epoch) == 0ull) break;
                    if (++spins > kScanSpin) {  // cannot happen (tiles are taken in order by running
                        scal[3] = 1;            // workgroups); reported instead of hanging
                        break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                }
                // the nearest inclusive prefix among them ends the look-back: add the values of the
                // lanes up to and including it
                const unsigned long long pre = __ballot(((st >> 32) & 3ull) == 2ull && j >= 0);
                const int stop = pre ? __builtin_ctzll(pre) : 64;
                ex += wave_sum((lane <= stop && j >= 0) ? (long long)(st & 0xFFFFFFFFull) : 0);
                if (pre || spins > kScanSpin) break;
            }
        }
        if (lane == 0) {
            __hip_atomic_store(sstat + tile, tag | (2ull << 32) | (unsigned long long)(ex + agg), __ATOMIC_RELEASE,
                               __HIP_MEMORY_SCOPE_AGENT);
            ex_sh = ex;
            if (tile == ntiles - 1) {
                const long long t = ex + agg < cap ? ex + agg : cap;
                scal[0] = t;
                scal[1] += t;
            }
        }
    }
    __syncthreads();
    long long run = ex_sh + wbase + inc - v;
    if (run + v > cap) {  // the clip: this round holds at most cap tests
        len = (int32_t)(run >= cap ? 0 : cap - run);
        run = run < cap ? run : cap;
    }
    return (int32_t)run;
}

// candidate k of an edge: adj(x)\{y} then adj(y)\{x}, each ascending
__device__ __forceinline__ int l1_cand(const L1Edge &g, const int32_t *__restrict__ adj, int k) {
    return k < g.m0 ? adj[g.ax + k + (k >= g.skx)] : adj[g.ay + (k - g.m0) + ((k - g.m0) >= g.sky)];
}

// the screen, one wave per edge (64 candidates per step, ballots): count the candidates it keeps ...
__device__ __forceinline__ L1Edge l1_edge_of(const int32_t *__restrict__ pairs, const int32_t *__restrict__ adj,
                                             const int32_t *__restrict__ adj_off, int e) {
    const int x = pairs[2 * e], y = pairs[2 * e + 1];
    const int ax = adj_off[x], nx = adj_off[x + 1] - ax, ay = adj_off[y], ny = adj_off[y + 1] - ay;
    int skx = find_sorted(adj + ax, nx, y), sky = find_sorted(adj + ay, ny, x);
    const int m0 = skx >= 0 ? nx - 1 : nx, m1 = sky >= 0 ? ny - 1 : ny;
    skx = skx >= 0 ? skx : nx + 1, sky = sky >= 0 ? sky : ny + 1;
    return L1Edge{x, y, m0, m0 + m1, skx, sky, ax, ay, m0 + m1, -1};
}
__global__ __launch_bounds__(256) void ci_l1_screen_count(const int32_t *__restrict__ pairs, int E,
                                                          const int32_t *__restrict__ adj,
                                                          const int32_t *__restrict__ adj_off,
                                                          const double *__restrict__ mi, const int32_t *__restrict__ dims,
                                                          const double *__restrict__ band, int nband, int nv,
                                                          double two_n, int32_t *__restrict__ pcnt) {
    const int lane = threadIdx.x & 63;
    for (int e = blockIdx.x * 4 + (threadIdx.x >> 6); e < E; e += gridDim.x * 4) {  // (whole waves)
        const L1Edge g = l1_edge_of(pairs, adj, adj_off, e);
        const double gxy = mi[l1_pidx(g.x, g.y, nv)];
        int n = 0;
        for (int k0 = 0; k0 < g.L; k0 += 64) {
            const int k = k0 + lane;
            n += __popcll(__ballot(k < g.L && l1_plausible(mi, nv, dims, band, nband, two_n, g.x, g.y, l1_cand(g, adj, k), gxy)));
        }
        if (lane == 0) pcnt[e] = n;
    }
}
// ... and, once ci_l1_setup has placed every edge's list, write the kept positions in order
__global__ __launch_bounds__(256) void ci_l1_screen_fill(const L1Edge *__restrict__ ed, int E,
                                                         const int32_t *__restrict__ adj, const double *__restrict__ mi,
                                                         const int32_t *__restrict__ dims,
                                                         const double *__restrict__ band, int nband, int nv,
                                                         double two_n, int32_t *__restrict__ plist) {
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int e = blockIdx.x * 4 + (threadIdx.x >> 6); e < E; e += gridDim.x * 4) {
        const L1Edge g = ed[e];
        const double gxy = mi[l1_pidx(g.x, g.y, nv)];
        int q = g.pl;
        for (int k0 = 0; k0 < g.L; k0 += 64) {
            const int k = k0 + lane;
            const bool keep = k < g.L && l1_plausible(mi, nv, dims, band, nband, two_n, g.x, g.y, l1_cand(g, adj, k), gxy);
            const unsigned long long m = __ballot(keep);
            if (keep) plist[q + __popcll(m & below)] = k;
            q += __popcll(m);
        }
    }
}

// every edge's search state, the first round's lengths (chunk0 candidates per edge) and their
// offsets; both open-count ring slots zeroed; with the screen (A.mi) each edge's kept count from
// A.pcnt and its list offset pl first
__global__ __launch_bounds__(256) void ci_l1_setup(CiL1Args A) {
    constexpr unsigned epoch = 1;
    L1Edge *ed = static_cast<L1Edge *>(A.ed);
    const int E = A.E;
    unsigned *tickets = reinterpret_cast<unsigned *>(A.scal + 4);
    if (blockIdx.x == 0 && threadIdx.x < 2) A.ring[threadIdx.x] = 0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) tickets[(epoch + 1) & 1u] = 0u;
    const int ntiles = (E + 255) / 256;
    for (;;) {
        const int tile = l1_ticket(tickets, epoch);
        if (tile >= ntiles) break;
        const int e = tile * 256 + threadIdx.x;
        int32_t l = 0;
        L1Edge g{};
        if (e < E) {
            g = l1_edge_of(A.pairs, A.adj, A.adj_off, e);
            if (A.mi) g.P = A.pcnt[e];  // the candidates the screen keeps (ci_l1_screen_count)
        }
        if (A.mi) {  // their positions go to plist[pl .. pl + P) (ci_l1_screen_fill, after this kernel)
            int32_t pcount = e < E ? g.P : 0;
            const int32_t pl = l1_tile_scan(tile, ntiles, pcount, A.sstat2, epoch, 1ll << 62, A.scal2);
            if (e < E) g.pl = pl;
        }
        if (e < E) {
            ed[e] = g;
            A.pos[e] = 0;
            // no candidate left to run: kept, every candidate counted (a dependent test each)
            A.st[e] = g.P == 0 ? 2 : 0;
            A.sep[e] = -1;
            A.counted[e] = g.P == 0 ? g.L : 0;
            l = g.P < A.chunk0 ? g.P : A.chunk0;
        }
        const int32_t o = l1_tile_scan(tile, ntiles, l, A.sstat, epoch, A.cap, A.scal);
        if (e < E) A.len[e] = l, A.off[e] = o;
    }
}

// one thread per generated test: its edge by binary search over off (edges with len 0 share an
// offset with the next one; the last edge whose off <= t owns t)
__global__ __launch_bounds__(256) void ci_l1_gen(const L1Edge *__restrict__ ed, const int32_t *__restrict__ pos,
                                                 const int32_t *__restrict__ off, int E,
                                                 const long long *__restrict__ total,
                                                 const int32_t *__restrict__ adj, int32_t *__restrict__ items,
                                                 const int32_t *__restrict__ dims,
                                                 unsigned long long *__restrict__ rows_read,
                                                 const int32_t *__restrict__ plist) {
    const long long n = *total;
    // wave-uniform trip count (the row tally below is reduced per wave)
    for (long long wb = (long long)blockIdx.x * 256 + (threadIdx.x & ~63); wb < n; wb += (long long)gridDim.x * 256) {
        const long long t = wb + (threadIdx.x & 63);
        unsigned rows = 0;
        if (t < n) {
            int lo = 0, hi = E;  // last e with off[e] <= t
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (off[mid] <= t) lo = mid;
                else hi = mid;
            }
            const L1Edge g = ed[lo];
            const int j = pos[lo] + (int)(t - off[lo]);
            const int z = l1_cand(g, adj, g.pl < 0 ? j : plist[g.pl + j]);
            items[3 * t] = g.x, items[3 * t + 1] = g.y, items[3 * t + 2] = z;
            rows = dims[g.x] + dims[g.y] + dims[z] - 3;  // mask rows the derived count reads
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) rows += __shfl_xor(rows, o);  // (wave_sum written out: this kernel's code stays as it was)
        if ((threadIdx.x & 63) == 0 && rows) atomicAdd(rows_read, (unsigned long long)rows);
    }
}

// a round's end (epoch = round + 2): every open edge's prefix resolved in order, then the next
// round's lengths (next_chunk candidates per edge) and offsets; open_cnt += edges still open
__global__ __launch_bounds__(256) void ci_l1_resolve(CiL1Args A, unsigned *__restrict__ open_cnt,
                                                     unsigned *__restrict__ open_next, int next_chunk, unsigned epoch) {
    const L1Edge *ed = static_cast<const L1Edge *>(A.ed);
    const int E = A.E;
    unsigned *tickets = reinterpret_cast<unsigned *>(A.scal + 4);
    // the next round's open-count slot (its previous value went to the host before this round) and
    // the next kernel's ticket counter
    if (blockIdx.x == 0 && threadIdx.x == 0) *open_next = 0u, tickets[(epoch + 1) & 1u] = 0u;
    const int ntiles = (E + 255) / 256;
    for (;;) {
        const int tile = l1_ticket(tickets, epoch);
        if (tile >= ntiles) break;
        const int e = tile * 256 + threadIdx.x;
        bool open = false;
        if (e < E && A.st[e] == 0) {
            const int n = A.len[e], o = A.off[e];
            int found = -1;
            for (int i = 0; i < n; ++i)
                if (A.indep[o + i]) {
                    found = i;
                    break;
                }
            const L1Edge g = ed[e];
            if (found >= 0) {  // counted: every candidate up to its position (the screened-out ones dependent)
                A.st[e] = 1;
                A.sep[e] = A.items[3 * (o + found) + 2];
                const int j = A.pos[e] + found;
                A.counted[e] = (g.pl < 0 ? j : A.plist[g.pl + j]) + 1;
            } else {
                A.pos[e] += n;
                if (A.pos[e] >= g.P) A.st[e] = 2, A.counted[e] = g.L;
                else open = true;
            }
        }
        // the next round's length of this edge and, through the tile scan, its offset
        int32_t l = 0;
        if (e < E && open) {
            const int left = ed[e].P - A.pos[e];
            l = left < next_chunk ? left : next_chunk;
        }
        const int32_t o = l1_tile_scan(tile, ntiles, l, A.sstat, epoch, A.cap, A.scal);
        if (e < E) A.len[e] = l, A.off[e] = o;
        const unsigned nopen = (unsigned)__popcll(__ballot(open));  // one atomic per wave
        if ((threadIdx.x & 63) == 0 && nopen) atomicAdd(open_cnt, nopen);
    }
}

// ---- level 0 -> level 1 without the host: the pairs level 0 kept (decision flag 0 over the
// implicit complete graph, pair (i < j) at i*n - i(i+1)/2 + j-i-1) become the level-1 edge list
// (lexicographic, as the host's vec_edges) and the CSR adjacency (each list ascending: the lower
// neighbours, then the upper ones -- the order the host builds from the edge list).  One wave per
// variable, 64 flags per step with a ballot.
__global__ __launch_bounds__(256) void ci_kept_count(const uint8_t *__restrict__ indep, int n, int32_t *__restrict__ low,
                                                     int32_t *__restrict__ up) {
    const int lane = threadIdx.x & 63, v = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= n) return;  // (whole wave)
    int lo = 0, hi = 0;
    for (int u0 = 0; u0 < v; u0 += 64) {
        const int u = u0 + lane;
        lo += __popcll(__ballot(u < v && indep[fbn_pair_index(u, v, n)] == 0));
    }
    for (int w0 = v + 1; w0 < n; w0 += 64) {
        const int w = w0 + lane;
        hi += __popcll(__ballot(w < n && indep[fbn_pair_index(v, w, n)] == 0));
    }
    if (lane == 0) low[v] = lo, up[v] = hi;
}
// one workgroup: off = exclusive scan of the degrees (off[n] = 2E), upoff = exclusive scan of the
// upper counts; scal[0] = E, scal[1] = the level's candidate sets sum_e (deg x + deg y - 2) =
// sum_v deg(v)^2 - 2E
__global__ __launch_bounds__(1024) void ci_kept_scan(const int32_t *__restrict__ low, const int32_t *__restrict__ up,
                                                     int n, int32_t *__restrict__ off, int32_t *__restrict__ upoff,
                                                     long long *__restrict__ scal) {
    __shared__ long long sd[1024], su[1024];
    __shared__ long long carry_d, carry_u, sq;
    const int t = threadIdx.x;
    if (t == 0) carry_d = carry_u = sq = 0;
    __syncthreads();
    for (int b = 0; b < n; b += 1024) {
        const int v = b + t;
        const long long d = v < n ? (long long)low[v] + up[v] : 0, u = v < n ? up[v] : 0;
        sd[t] = d, su[t] = u;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {  // inclusive Hillis-Steele scan
            const long long xd = t >= o ? sd[t - o] : 0, xu = t >= o ? su[t - o] : 0;
            __syncthreads();
            sd[t] += xd, su[t] += xu;
            __syncthreads();
        }
        if (v < n) off[v] = (int32_t)(carry_d + sd[t] - d), upoff[v] = (int32_t)(carry_u + su[t] - u);
        if (d) atomicAdd((unsigned long long *)&sq, (unsigned long long)(d * d));
        __syncthreads();
        if (t == 1023) carry_d += sd[1023], carry_u += su[1023];
        __syncthreads();
    }
    if (t == 0) {
        off[n] = (int32_t)carry_d;
        scal[0] = carry_u;
        scal[1] = sq - 2 * carry_u;
    }
}
__global__ __launch_bounds__(256) void ci_kept_fill(const uint8_t *__restrict__ indep, int n,
                                                    const int32_t *__restrict__ off, const int32_t *__restrict__ upoff,
                                                    int32_t *__restrict__ adj, int32_t *__restrict__ pairs) {
    const int lane = threadIdx.x & 63, v = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= n) return;
    const unsigned long long below = (1ull << lane) - 1ull;
    int r = off[v], q = upoff[v];
    for (int u0 = 0; u0 < v; u0 += 64) {
        const int u = u0 + lane;
        const bool k = u < v && indep[fbn_pair_index(u, v, n)] == 0;
        const unsigned long long m = __ballot(k);
        if (k) adj[r + __popcll(m & below)] = u;
        r += __popcll(m);
    }
    for (int w0 = v + 1; w0 < n; w0 += 64) {
        const int w = w0 + lane;
        const bool k = w < n && indep[fbn_pair_index(v, w, n)] == 0;
        const unsigned long long m = __ballot(k);
        if (k) {
            const int i = __popcll(m & below);
            adj[r + i] = w;
            pairs[2 * (q + i)] = v, pairs[2 * (q + i) + 1] = w;
        }
        r += __popcll(m), q += __popcll(m);
    }
}
// level-1 results straight into pinned host memory (one kernel instead of four DMA copies): the
// removal flag (status 1) and the sepset (or -1) of every edge, per-workgroup sums of the counted
// tests in `part`; ci_l1_results_tail adds them up and copies the launched count and the scan flag
__global__ __launch_bounds__(256) void ci_l1_results(const uint8_t *__restrict__ st, const int32_t *__restrict__ sep,
                                                     const long long *__restrict__ cnt, int E, char *__restrict__ h_rm,
                                                     int32_t *__restrict__ h_sep, long long *__restrict__ part) {
    __shared__ long long ws[4];
    long long acc = 0;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < E; e += gridDim.x * 256) {
        const bool rm = st[e] == 1;
        h_rm[e] = rm ? 1 : 0;
        h_sep[e] = rm ? sep[e] : -1;
        acc += cnt[e];
    }
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);  // (wave_sum written out: code as it was)
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}
__global__ __launch_bounds__(64) void ci_l1_results_tail(const long long *__restrict__ part, int nparts,
                                                         const long long *__restrict__ scal, long long *__restrict__ h_sc) {
    long long acc = 0;
    for (int i = threadIdx.x; i < nparts; i += 64) acc += part[i];
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);  // (wave_sum written out: code as it was)
    // (scal[11]: the information screen's scan flag, ci_l1_setup's second scan at scal + 8)
    if (threadIdx.x == 0) h_sc[0] = acc, h_sc[1] = scal[1], h_sc[2] = scal[2], h_sc[3] = scal[3] | scal[11];
}

}  // namespace

extern "C" size_t fbn_ci_l1_edge_bytes(void) { return sizeof(L1Edge); }

// h_sc: 4 long longs (counted, launched, rows read, scan flag); part: >= 256 long longs of scratch
extern "C" hipError_t fbn_ci_l1_results(const uint8_t *st, const int32_t *sep, const long long *cnt, int E,
                                        const long long *scal, char *h_rm, int32_t *h_sep, long long *h_sc,
                                        long long *part, hipStream_t s) {
    const int g = std::max(1, std::min(256, (E + 255) / 256));
    hipLaunchKernelGGL(ci_l1_results, dim3(g), dim3(256), 0, s, st, sep, cnt, E, h_rm, h_sep, part);
    hipLaunchKernelGGL(ci_l1_results_tail, dim3(1), dim3(64), 0, s, part, g, scal, h_sc);
    return hipGetLastError();
}

// low / up: n ints of scratch each; scal: 2 long longs (E, candidate sets)
extern "C" hipError_t fbn_ci_kept_csr(const uint8_t *indep, int n, int32_t *low, int32_t *up, int32_t *off,
                                      int32_t *upoff, int32_t *adj, int32_t *pairs, long long *scal, hipStream_t s) {
    const dim3 g((unsigned)((n + 3) / 4));
    hipLaunchKernelGGL(ci_kept_count, g, dim3(256), 0, s, indep, n, low, up);
    hipLaunchKernelGGL(ci_kept_scan, dim3(1), dim3(1024), 0, s, low, up, n, off, upoff, scal);
    hipLaunchKernelGGL(ci_kept_fill, g, dim3(256), 0, s, indep, n, off, upoff, adj, pairs);
    return hipGetLastError();
}

// a->mi != nullptr: the information screen first (ci_args.h)
extern "C" hipError_t fbn_ci_l1_setup(const CiL1Args *a, hipStream_t s) {
    const int E = a->E, nv = a->nv;
    const int ntiles = (E + 255) / 256;
    if (E <= 0) return hipSuccess;
    const unsigned gw = (unsigned)std::min((E + 3) / 4, a->num_cu * 8);  // one wave per edge
    if (a->mi) {
        if (a->mi_from_tables) {
            const hipError_t err = fbn::CiPairG2Launch(a->pairtab, a->dims, nv, a->mi, s);
            if (err != hipSuccess) return err;
        }
        hipLaunchKernelGGL(ci_l1_screen_count, dim3(gw), dim3(256), 0, s, a->pairs, E, a->adj, a->adj_off,
                           (const double *)a->mi, a->dims, a->band, a->nband, nv, a->two_n, a->pcnt);
    }
    hipLaunchKernelGGL(ci_l1_setup, dim3((unsigned)std::min(ntiles, a->num_cu * 4)), dim3(256), 0, s, *a);
    if (a->mi)
        hipLaunchKernelGGL(ci_l1_screen_fill, dim3(gw), dim3(256), 0, s, (const L1Edge *)a->ed, E, a->adj,
                           (const double *)a->mi, a->dims, a->band, a->nband, nv, a->two_n, a->plist);
    return hipGetLastError();
}

// one round (its lengths and offsets come from ci_l1_setup or the previous round's resolve):
// generation, counting, G^2 / decisions, resolution + the next round's lengths and offsets for
// next_chunk; scal[0] = the round's test count (device), open_cnt += edges still open after it,
// *open_next = 0; epoch = round + 2
extern "C" hipError_t fbn_ci_l1_round(const CiL1Args *a, unsigned *open_cnt, unsigned *open_next, int next_chunk,
                                      unsigned epoch, hipStream_t s) {
    const int E = a->E, ntiles = (E + 255) / 256;
    const long long cap = a->cap, gcap = (long long)a->num_cu * 8, gt = (cap + 255) / 256;
    const dim3 gT((unsigned)(gt < gcap ? gt : gcap));
    const long long *total = a->scal;  // the round's test count, read on the device
    unsigned long long *rows_read = reinterpret_cast<unsigned long long *>(a->scal + 2);
    hipLaunchKernelGGL(ci_l1_gen, gT, dim3(256), 0, s, (const L1Edge *)a->ed, a->pos, a->off, E, total, a->adj, a->items,
                       a->dims, rows_read, (const int32_t *)a->plist);
    CiBitsArgs c{};  // the derived counting of up to cap tests (the pair tables are only read)
    c.bits = a->bits, c.dims = a->dims, c.row0 = a->row0, c.items = a->items, c.W = a->W, c.n = cap;
    c.counts = a->counts, c.pairtab = const_cast<int32_t *>(a->pairtab), c.nvars = a->nv, c.num_cu = a->num_cu;
    hipError_t err = fbn::CiCountDerivedLaunch(c, total, s);
    if (err != hipSuccess) return err;
    // four lanes per test: the screened rounds are small (a few thousand to ~27k tests on config 5),
    // where the lane-per-test kernel's single latency chain per test dominated (config 5: 0.22 ->
    // 0.13 ms of G^2 per run)
    CiG2Args g{};
    g.counts = a->counts, g.dims = a->dims, g.items = a->items, g.n = cap, g.nvars = a->nv, g.alpha = a->alpha;
    g.df = a->df, g.indep = a->indep, g.stats = a->stats, g.band = a->band, g.nband = a->nband, g.n_dev = total;
    err = fbn::CiG2Launch(g, 1, /*quad*/ true, a->num_cu, s);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(ci_l1_resolve, dim3((unsigned)std::min(ntiles, a->num_cu * 4)), dim3(256), 0, s, *a, open_cnt,
                       open_next, next_chunk, epoch);
    return hipGetLastError();
}
