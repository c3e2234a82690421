// sample_model.h -- what the sampling engine's host twin (sample_host.cpp) and its kernels
// (sample.hip) share, and with them EPIS-BN's and the adaptive samplers': the flattened network, numpy's
// PCG64 in 64-bit halves, the value-selection rule, the scaled-weight arithmetic of a case.
#ifndef FBN_SAMPLE_MODEL_H
#define FBN_SAMPLE_MODEL_H

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FBN_HD __host__ __device__ __forceinline__
#else
#define FBN_HD inline
#endif

// Variables per sampler: one wave keeps its 64 samples' values as bytes [V][64] in LDS, 64 V bytes
// of the CU's 160 KiB; 2048 variables take 128 KiB (one wave per CU).
#define FBN_SAMPLE_MAX_VARS 2048
// fbn_lw_debug_samples: samples per call (ncases * S)
#define FBN_SAMPLE_DEBUG_MAX ((int64_t)1 << 22)

namespace fbn {

// ---- numpy.random.PCG64 (128-bit LCG, XSL-RR 128/64) in 64-bit halves
struct U128 {
    uint64_t hi, lo;
};
constexpr uint64_t kPcgMultHi = 0x2360ED051FC65DA4ull, kPcgMultLo = 0x4385DF649FCCF645ull;

FBN_HD uint64_t MulHi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}
// m * s + c mod 2^128
FBN_HD U128 Affine(U128 s, U128 m, U128 c) {
    U128 r;
    const uint64_t lo = m.lo * s.lo;
    const uint64_t hi = MulHi64(m.lo, s.lo) + m.hi * s.lo + m.lo * s.hi;
    r.lo = lo + c.lo;
    r.hi = hi + c.hi + (r.lo < lo ? 1u : 0u);
    return r;
}
FBN_HD U128 PcgStep(U128 s, U128 inc) { return Affine(s, U128{kPcgMultHi, kPcgMultLo}, inc); }
FBN_HD uint64_t PcgOutput(U128 s) {
    const unsigned rot = (unsigned)(s.hi >> 58);
    const uint64_t x = s.hi ^ s.lo;
    return (x >> rot) | (x << ((64 - rot) & 63));
}
FBN_HD double PcgDouble(uint64_t r) { return (double)(r >> 11) * (1.0 / 9007199254740992.0); }

// ForwardSample's rule (synth.cpp): x = u * cdf[d - 1], value = min(#{q : x >= cdf[q]}, d - 1).  A
// cdf row is a running sum of positive probabilities, hence non-decreasing, so the count is the
// index of the first entry above x.
FBN_HD int SelectValue(const double *cdf, int d, double u) {
    const double x = u * cdf[d - 1];
    int q = 0;
    while (q < d - 1 && x >= cdf[q]) ++q;
    return q;
}

// ---- the network, flattened for the sampler
struct SampleNode {  // one per variable, in topological order
    int32_t v, d;        // variable, its state count
    int32_t npar, poff;  // parents (GIVEN order): par[2 * (poff + j)] = parent, [.. + 1] = its state count
    int32_t toff;        // first cell of its tables: prob / cdf [toff + pc * d + q], pc over GIVEN order, last fastest
    int32_t moff;        // first entry of its marginal row
};
struct SamplerModel {
    int V = 0, sum_dom = 0;
    int64_t cells = 0;
    std::vector<int32_t> dom;
    std::vector<SampleNode> nodes;
    std::vector<int32_t> par;
    std::vector<double> prob, cdf;
    std::vector<int32_t> ent;  // marginal entry -> variable << 8 | value
};
struct Network;
// FBN_ERR_ARG for a cyclic network, FBN_ERR_LIMIT past FBN_SAMPLE_MAX_VARS or FBN_PARAM_MAX_CELLS
int BuildSamplerModel(const Network &net, SamplerModel &M);

// PCG64(seed) after seeding and the (multiplier, increment) pairs of its 2^j-step jumps, j < 64:
// jump[4 * j ..] = mult.hi, mult.lo, plus.hi, plus.lo
struct PcgStream {
    U128 state, inc;
    uint64_t jump[256];
};
void PcgStreamInit(uint64_t seed, PcgStream &R);
// the affine map of `delta` steps
void PcgJump(const PcgStream &R, uint64_t delta, U128 *mult, U128 *plus);
// the state `delta` steps on: one table pair per set bit
FBN_HD U128 PcgJumpTo(U128 s, uint64_t delta, const uint64_t *jump) {
    for (int j = 0; j < 64 && (delta >> j) != 0; ++j)
        if ((delta >> j) & 1)
            s = Affine(s, U128{jump[4 * j], jump[4 * j + 1]}, U128{jump[4 * j + 2], jump[4 * j + 3]});
    return s;
}

// ---- the scaled weights of one case, the arithmetic every sampling kernel and host twin compiles.  A
// sample weighs ldexp(m, e); a chunk's weights are taken relative to the largest exponent seen since the
// scope opened, w = ldexp(m, e - emax), and sumw, sumw2 are the sums of w and w^2 on that scale.
struct WeightState {
    int emax = 0;
    double sumw = 0.0, sumw2 = 0.0;
};
// Open or rescale: cm is the chunk's maximum exponent, first says that this chunk opens the scope.  Sets
// emax and returns the exact power of two f by which everything summed so far is multiplied.
FBN_HD double WeightRescale(WeightState &ws, int cm, bool first) {
    double f = 1.0;
    if (first) ws.emax = cm;
    else if (cm > ws.emax) f = ldexp(1.0, ws.emax - cm), ws.emax = cm;
    return f;
}
// the chunk's sums of w and w^2 (butterfly order) join the rescaled running sums
FBN_HD void WeightAdd(WeightState &ws, double f, double sw, double sw2) {
    ws.sumw = ws.sumw * f + sw;
    ws.sumw2 = ws.sumw2 * f * f + sw2;
}
FBN_HD double WeightLogEvidence(const WeightState &ws, long long S) {
    return ws.sumw > 0.0 ? log(ws.sumw / (double)S) + (double)ws.emax * 0.6931471805599453 : -INFINITY;
}
FBN_HD double WeightEss(const WeightState &ws) { return ws.sumw > 0.0 ? ws.sumw * ws.sumw / ws.sumw2 : 0.0; }
// the query label from the case's normalised row: ArgMax, strict '>' from 0 (src/Inference.cpp:92-102), as
// fbn_jt_run; -1 when no sample weighs anything
FBN_HD int QueryLabel(const double *row, int d0, double sumw) {
    if (!(sumw > 0.0)) return -1;
    int lab = 0;
    double mp = 0.0;
    for (int q = 0; q < d0; ++q)
        if (row[q] > mp) mp = row[q], lab = q;
    return lab;
}

// what the host twins share (sample_host.cpp, ais_host.cpp): fn(begin, end) over [0, n) in contiguous
// ranges of at least `grain`, in parallel on HostThreads() threads (knobs.h); the sum over 64 lanes in the kernels' butterfly order (lane i adds lane i ^ off, off = 32 .. 1; a is
// overwritten); the parent configuration of node nd from one sample's values (stride between variables: vs)
void ParallelRanges(int64_t n, int64_t grain, const std::function<void(int64_t, int64_t)> &fn);
double Butterfly(double *a);
inline int ParentConfig(const SamplerModel &M, const SampleNode &nd, const uint8_t *x, size_t vs) {
    int pc = 0;
    for (int j = 0; j < nd.npar; ++j) pc = pc * M.par[2 * (nd.poff + j) + 1] + x[(size_t)M.par[2 * (nd.poff + j)] * vs];
    return pc;
}
// One 64-sample chunk of a case on the host, as the kernels' chunk tail: from the mantissas and exponents
// of its act samples, rescale ws (first: the chunk opens the scope), write the weights w[0 .. 64) (0.0 from
// act on), add their sums to ws, return f.  w stays intact: the butterflies run on copies.
double HostChunkWeights(WeightState &ws, const double *m, const int *e, int act, bool first, double *w);
// the chunk's marginal sums by entry into the case's row: samples l < act in ascending order (x: values [V][64])
void HostAccumulateChunk(const SamplerModel &M, const uint8_t *x, const double *w, int act, double f, bool first,
                         double *row);
// the kernels' case tail: normalise the row (observed variables and a weightless case: zeros), the query
// label, stats[0 .. 2) = log_evidence, ess unless stats is NULL
void HostFinishCase(const SamplerModel &M, const int8_t *e_row, double *row, const WeightState &ws, int64_t S,
                    int32_t *label, double *stats);

// the host path (device < 0 samplers, tools/sample_host_check.cpp): the kernels' algorithm, chunk
// for chunk, on CPU threads.  Arguments are checked by the callers except the evidence codes.
int HostForward(const SamplerModel &M, int64_t n, uint64_t seed, uint8_t *cols);
// labels [ncases], marg [ncases][sum_dom] or NULL, stats [ncases][2] or NULL; dbg_* (all or none):
// values [V][ncases * S], mantissas / exponents [ncases * S]
int HostLw(const SamplerModel &M, int method, const int8_t *ev, int64_t ncases, int64_t S, uint64_t seed,
           int64_t case_offset, int32_t *labels, double *marg, double *stats, uint8_t *dbg_vals, double *dbg_m,
           int32_t *dbg_e);
// HostLw's loop with an importance function (EPIS-BN, epis_model.h).  lam == NULL: HostLw itself.  Else
// lam [ncases][sum_dom], method 0: an unobserved variable is drawn by EpisDraw from its table row and
// its lambda row with cutoff EpisCutoff(eps, d) and the weight takes the draw's factor through the same
// frexp pair; stats is then [ncases][4], the last two copied from lbp_stats [ncases][2] (NULL: zeros).
int HostImportance(const SamplerModel &M, int method, const int8_t *ev, int64_t ncases, int64_t S, uint64_t seed,
                   int64_t case_offset, const double *lam, double eps, const double *lbp_stats, int32_t *labels,
                   double *marg, double *stats, uint8_t *dbg_vals, double *dbg_m, int32_t *dbg_e);
// -1 .. dom - 1 everywhere, else FBN_ERR_ARG naming the first bad case / node
int CheckEvidenceHost(const SamplerModel &M, const int8_t *ev, int64_t ncases);
// S >= 1, method 0 / 1, and stream positions ((case_offset + ncases) * S + 64) * V below 2^63
int CheckLwShape(const SamplerModel &M, int method, int64_t ncases, int64_t S, int64_t case_offset);
// fbn_jt_score's sums from the state counts alone
int ScoreMarginals(const std::vector<int> &dom, const double *marginals, const double *golden, int64_t ncases,
                   double *mse_sum, double *hd_sum);

}  // namespace fbn

#endif
