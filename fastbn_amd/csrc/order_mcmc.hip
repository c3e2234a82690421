// order_mcmc.hip -- order MCMC on gfx950 (include/fastbn.h, "order MCMC", states the definitions; DESIGN.md 5.18
// the design).  One chain per wave, resident for the whole launch; `group` chains share a workgroup so that the
// family lists, which every chain reads, stay hot in L2.  Nothing is shared between the waves of a workgroup and
// no workgroup barrier is used: a wave orders its own LDS traffic with wavefront fences.
//
// A wave's state is 3,136 bytes of LDS: the order (bytes by position), pred and term by node, the proposed pred
// and term of the nodes a move touches, and the 128-slot ring of the term scan.  Everything that steers control
// flow (positions, nodes, list bounds, ballots) is wave-uniform.
//
// The term scan reads a node's list 64 entries at a time (one coalesced 16-byte load per lane) and tests
// consistency with one AND.  Pass 1 takes the maximum.  Pass 2 COMPACTS: the consistent scores of a chunk go,
// by ballot and prefix count, to consecutive slots of the ring, and every time 64 are waiting each lane takes
// one and runs one exp chain -- so the exp chains run over the consistent entries alone, about (p / n)^k of the
// list at position p, and slot l of the definition (rank = l mod 64) is lane l by construction.
//
// At a sample, lane u owns arc u -> v: the wave walks v's consistent entries in list order, broadcasts (mask,
// weight) from the owning lane and lane u adds the weight when bit u is set.  No atomics, no n x n LDS.
//
// fp64 and integer code only; no library exp / log (exact_lse.h, hc_bd.h).  Built with contraction off and the
// packed-fp32 guard (Makefile).
#include <hip/hip_runtime.h>

#include "launchers.h"
#include "order_mcmc.h"
#include "sample_device.h"

namespace fbn {
namespace {

struct WaveState {
    double ring[128];
    double term[64], nterm[64];
    uint64_t pred[64], npred[64];
    uint8_t order[64];
};

// orders this wave's LDS stores before its later LDS loads of other lanes' slots
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ uint64_t uni64(uint64_t x) {
    return ((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(x >> 32)) << 32) |
           (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)x);
}
__device__ __forceinline__ uint64_t read_lane64(uint64_t x, int l) {
    return ((uint64_t)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(x >> 32), l) << 32) |
           (unsigned)__builtin_amdgcn_readlane((int)(unsigned)x, l);
}
__device__ __forceinline__ double wave_max(double x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double y = __shfl_xor(x, off, 64);
        x = y > x ? y : x;
    }
    return x;
}
// entry f of a list of len >= 1 entries, clamped: a lane past the end reads the last entry and ignores it
__device__ __forceinline__ OmcmcEntry load_entry(const OmcmcEntry *e, int f, int len) { return e[f < len ? f : len - 1]; }

// term_v: e = the node's list (len >= 1, entry 0 the empty set), pred wave-uniform
__device__ double scan_term(const OmcmcEntry *e, int len, uint64_t pred, double *ring, int lane) {
    double m = e[0].score;
    for (int base = 0; base < len; base += 256) {  // four loads in flight per lane
        OmcmcEntry x[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = load_entry(e, base + 64 * q + lane, len);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (base + 64 * q + lane < len && !(x[q].mask & ~pred) && x[q].score > m) m = x[q].score;
    }
    m = wave_max(m);

    double acc = 0.0;
    int cnt = 0, head = 0;  // scores waiting in the ring: slots head .. head + cnt - 1 (mod 128), cnt < 64 between chunks
    OmcmcEntry nx = load_entry(e, lane, len);
    for (int base = 0; base < len; base += 64) {
        const OmcmcEntry x = nx;
        nx = load_entry(e, base + 64 + lane, len);  // the next chunk's load overlaps this chunk's work
        const bool ok = base + lane < len && !(x.mask & ~pred);
        const uint64_t bal = __ballot(ok);
        if (ok) ring[(head + cnt + __popcll(bal & (((uint64_t)1 << lane) - 1))) & 127] = x.score;
        cnt += __popcll(bal);
        if (cnt >= 64) {
            wave_lds_sync();
            acc = acc + fbn_lse_exp(ring[(head + lane) & 127] - m);
            head = (head + 64) & 127;
            cnt -= 64;
        }
    }
    wave_lds_sync();
    if (lane < cnt) acc = acc + fbn_lse_exp(ring[(head + lane) & 127] - m);
    wave_lds_sync();  // the ring is free for the next scan
    return m + fbn_bd_ln(wave_sum(acc));
}

// lane u's P(u -> v | order): the consistent entries of v's list in list order
__device__ double arc_row(const OmcmcEntry *e, int len, uint64_t pred, double term, int lane) {
    double row = 0.0;
    for (int base = 0; base < len; base += 64) {
        const OmcmcEntry x = load_entry(e, base + lane, len);
        const bool ok = base + lane < len && !(x.mask & ~pred);
        const double w = ok ? fbn_lse_exp(x.score - term) : 0.0;
        for (uint64_t bal = __ballot(ok); bal; bal &= bal - 1) {
            const int l = uni(__ffsll((unsigned long long)bal) - 1);
            const uint64_t mk = read_lane64(x.mask, l);
            const double wl = read_lane(w, l);
            if (mk >> lane & 1) row = row + wl;
        }
    }
    return row;
}

struct Lists {
    const OmcmcEntry *ent;
    const long long *off;
    __device__ const OmcmcEntry *at(int v) const { return ent + off[v]; }
    __device__ int len(int v) const { return (int)(off[v + 1] - off[v]); }
};

// pred and term of every node from W.order
__device__ void order_terms(const Lists &F, int n, WaveState &W, int lane) {
    uint64_t before = 0;
    for (int p = 0; p < n; ++p) {
        const int v = uni(W.order[p]);
        const double t = scan_term(F.at(v), F.len(v), before, W.ring, lane);
        if (lane == 0) W.pred[v] = before, W.term[v] = t;
        before |= (uint64_t)1 << v;
    }
    wave_lds_sync();
}

__device__ __forceinline__ WaveState &wave_state(int w) {
    extern __shared__ __align__(16) unsigned char omcmc_lds[];
    return reinterpret_cast<WaveState *>(omcmc_lds)[w];
}

__global__ __launch_bounds__(64 * kOmcmcGroupMax) void omcmc_chain_kernel(const OmcmcDeviceArgs A) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, n = A.n;
    const long long c = (long long)blockIdx.x * A.group + w;
    if (c >= A.chains) return;  // whole waves leave; there is no workgroup barrier below
    WaveState &W = wave_state(w);
    const Lists F{A.ent, A.off};
    const uint64_t g = (uint64_t)(A.chain0 + c);
    double *acc = A.acc + (size_t)c * n * 64;
    long long accepted = 0;

    if (A.t0 == 0) {
        W.order[lane] = 0;
        wave_lds_sync();
        if (lane == 0) OmcmcStartOrder(PcgJumpTo(A.state, OmcmcStartPos(g), A.jump), A.inc, n, W.order);
        for (int v = 0; v < n; ++v) acc[v * 64 + lane] = 0.0;
    } else {
        W.order[lane] = A.orders[c * 64 + lane];
        accepted = A.accepted[c];
    }
    wave_lds_sync();
    order_terms(F, n, W, lane);
    double L = 0.0;
    for (int v = 0; v < n; ++v) L = L + W.term[v];

    U128 s = PcgJumpTo(A.state, OmcmcStepPos(g, (uint64_t)A.t0), A.jump);
    for (long long t = A.t0; t < A.t1; ++t) {
        s = PcgStep(s, A.inc);
        const uint64_t r1 = PcgOutput(s);
        s = PcgStep(s, A.inc);
        const uint64_t r2 = PcgOutput(s);
        s = PcgStep(s, A.inc);
        const double u = PcgDouble(PcgOutput(s));
        if (n >= 2) {
            int pi, pj;
            OmcmcProposal(r1, r2, n, &pi, &pj);
            const int i = uni(pi), j = uni(pj);
            const int a = uni(W.order[i]), b = uni(W.order[j]);
            const uint64_t flip = ((uint64_t)1 << a) | ((uint64_t)1 << b);
            uint64_t changed = 0;
            for (int p = i; p <= j; ++p) {
                const int old = uni(W.order[p]);
                const int v = p == i ? b : p == j ? a : old;
                const uint64_t np = uni64(W.pred[old]) ^ (p > i ? flip : 0);
                const double nt = scan_term(F.at(v), F.len(v), np, W.ring, lane);
                if (lane == 0) W.npred[v] = np, W.nterm[v] = nt;
                changed |= (uint64_t)1 << v;
            }
            wave_lds_sync();
            double Ln = 0.0;
            for (int v = 0; v < n; ++v) Ln = Ln + (changed >> v & 1 ? W.nterm[v] : W.term[v]);
            if (OmcmcAccept(Ln - L, u)) {
                if (changed >> lane & 1) W.term[lane] = W.nterm[lane], W.pred[lane] = W.npred[lane];
                if (lane == 0) W.order[i] = (uint8_t)b, W.order[j] = (uint8_t)a;
                L = Ln;
                ++accepted;
                wave_lds_sync();
            }
        }
        if (t + 1 > A.burn_in && (t + 1 - A.burn_in) % A.thin == 0) {
            for (int v = 0; v < n; ++v) {
                const double row = arc_row(F.at(v), F.len(v), uni64(W.pred[v]), W.term[v], lane);
                acc[v * 64 + lane] = acc[v * 64 + lane] + row;
            }
            if (lane == 0) A.trace[c * A.samples + ((t + 1 - A.burn_in) / A.thin - 1)] = L;
        }
    }
    A.orders[c * 64 + lane] = W.order[lane];
    if (lane == 0) A.accepted[c] = accepted;
}

__global__ __launch_bounds__(64 * kOmcmcGroupMax) void omcmc_terms_kernel(const OmcmcTermsArgs A) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, n = A.n;
    const long long i = (long long)blockIdx.x * A.group + w;
    if (i >= A.k) return;
    WaveState &W = wave_state(w);
    const Lists F{A.ent, A.off};
    W.order[lane] = lane < n ? (uint8_t)A.orders[i * n + lane] : 0;
    wave_lds_sync();
    order_terms(F, n, W, lane);
    for (int v = 0; v < n; ++v) {
        const double row = arc_row(F.at(v), F.len(v), uni64(W.pred[v]), W.term[v], lane);
        if (lane < n) A.arcs[((size_t)i * n + lane) * n + v] = row;
        if (lane == 0) A.term[i * n + v] = W.term[v];
    }
}

}  // namespace
}  // namespace fbn

extern "C" size_t fbn_omcmc_wave_lds_bytes(void) { return sizeof(fbn::WaveState); }

extern "C" hipError_t fbn_omcmc_chain_launch(const fbn::OmcmcDeviceArgs *a, hipStream_t stream) {
    if (a->group < 1 || a->group > kOmcmcGroupMax || a->n < 1 || a->n > kOmcmcMaxVars || a->chains < 1 || a->t0 < 0 || a->t1 < a->t0)
        return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((a->chains + a->group - 1) / a->group);
    hipLaunchKernelGGL(fbn::omcmc_chain_kernel, dim3(grid), dim3(64 * a->group), a->group * sizeof(fbn::WaveState), stream, *a);
    return hipGetLastError();
}

extern "C" hipError_t fbn_omcmc_terms_launch(const fbn::OmcmcTermsArgs *a, hipStream_t stream) {
    if (a->group < 1 || a->group > kOmcmcGroupMax || a->n < 1 || a->n > kOmcmcMaxVars || a->k < 1) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((a->k + a->group - 1) / a->group);
    hipLaunchKernelGGL(fbn::omcmc_terms_kernel, dim3(grid), dim3(64 * a->group), a->group * sizeof(fbn::WaveState), stream, *a);
    return hipGetLastError();
}
