// sample.hip -- the sampling engine on gfx950: forward (ancestral) sampling, likelihood weighting
// and probabilistic logic sampling, one sample per lane (algorithm, stream maps and the host twin:
// sample_host.cpp).  Replaces the reference's PLS / LW stubs (src/main.cpp:97-121) and, for workload
// generation, its wall-clock seeded SampleSetGenerator.
//
// Both kernels run one wave per workgroup.  The wave keeps the values its 64 samples have drawn so
// far as bytes [V][64] in LDS (64 V bytes: 2.4 KB for ALARM, 66.6 KB for the 1041-variable
// Munin-like network), walks the variables in topological order, forms each lane's parent
// configuration from its own LDS column and gathers its cdf row (or, for an observed variable under
// likelihood weighting, one probability) from the fp64 tables in global memory.  The per-variable
// records and parent lists are wave-uniform reads.  Random numbers: every lane jumps numpy's
// PCG64(seed) to its first stream position with the host's 2^j jump pairs (2 KB, passed in the kernel
// arguments; one 128-bit affine step per set bit, 64-bit halves, __umul64hi), then takes one affine
// step per variable.
//
// sample_lw_kernel: one evidence case per wave, its S samples in chunks of 64.  A sample's weight is
// a scaled pair (m, e), (m, de) = frexp(m * P(v = ev | parents)), e += de, so 520 observed variables
// do not underflow.  Per chunk: emax by a wave max; when it grows the running sums are rescaled by
// the exact power of two; w = ldexp(m, e - emax); sum w and sum w^2 by a shuffle butterfly; the
// marginal sums by entry -- lane j owns entries j, j + 64, ... of the case's output row, reads that
// variable's 64 value bytes from LDS (four 16-byte reads) and adds w of lane l (v_readlane) where
// the byte equals its value, l = 0 .. 63 in order.  The case's output row is the accumulator between
// chunks (always the same lane on the same address).  No floating-point atomics; every sum has one
// fixed order, so runs and batch splits are bit-identical.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>
#include <set>

#include "fbn_device.h"
#include "fbn_internal.h"
#include "launchers.h"
#include "sample_device.h"
#include "sample_model.h"

using fbn::DevBuf;
using fbn::DeviceModel;
using fbn::parent_config;
using fbn::wave_max;
using fbn::wave_sum;
using fbn::SampleNode;
using fbn::SetError;
using fbn::U128;

namespace {

struct ForwardArgs {
    DeviceModel M;
    U128 state, inc, jm, jc;  // seeded state; the jump of n positions (one variable on)
    uint64_t jump[256];       // this seed's 2^j jump pairs (PcgStream::jump), read from the kernel arguments
    long long n;
    uint8_t *cols;  // [V][n]
};

struct LwArgs {
    DeviceModel M;
    U128 state, inc, jm, jc;  // the jump of 63 V positions (the same lane's sample in the next chunk)
    uint64_t jump[256];
    const int8_t *ev;         // [ncases][V], checked
    long long ncases, S, case0;
    int method;
    int32_t *labels;
    double *marg;   // [ncases][sum_dom]: accumulators, then the result
    double *stats;  // [ncases][2] or NULL
    uint8_t *dv;    // debug (all or none): values [V][ncases * S], mantissas, exponents [ncases * S]
    double *dm;
    int32_t *de;
};

__global__ __launch_bounds__(64) void sample_forward_kernel(ForwardArgs A) {
    extern __shared__ __align__(16) uint8_t vals[];  // [V][64]
    const int lane = threadIdx.x;
    const long long i = (long long)blockIdx.x * 64 + lane;
    const bool active = i < A.n;
    // a tail lane draws sample n - 1 again and stores nothing
    U128 s = fbn::PcgJumpTo(A.state, (uint64_t)(active ? i : A.n - 1), A.jump);
    for (int k = 0; k < A.M.V; ++k) {
        const SampleNode nd = A.M.nodes[k];
        const int pc = parent_config(A.M, nd, vals, lane);
        const double u = fbn::PcgDouble(fbn::PcgOutput(fbn::PcgStep(s, A.inc)));
        s = fbn::Affine(s, A.jm, A.jc);
        const int q = fbn::SelectValue(A.M.cdf + nd.toff + (long long)pc * nd.d, nd.d, u);
        vals[nd.v * 64 + lane] = (uint8_t)q;
        if (active) A.cols[(long long)nd.v * A.n + i] = (uint8_t)q;
    }
}

__global__ __launch_bounds__(64) void sample_lw_kernel(LwArgs A) {
    extern __shared__ __align__(16) uint8_t vals[];  // [V][64]
    const int lane = threadIdx.x, V = A.M.V, SD = A.M.sum_dom;
    const long long c = blockIdx.x;
    const int8_t *ev = A.ev + c * V;
    double *row = A.marg + c * SD;
    const long long total = A.ncases * A.S;
    U128 s;
    int emax = 0;
    double sumw = 0.0, sumw2 = 0.0;
    for (long long s0 = 0; s0 < A.S; s0 += 64) {
        const bool active = s0 + lane < A.S;  // a tail lane samples (in bounds) with weight 0
        if (s0 == 0)
            s = fbn::PcgJumpTo(A.state, ((uint64_t)(A.case0 + c) * (uint64_t)A.S + (uint64_t)lane) * (uint64_t)V, A.jump);
        else
            s = fbn::Affine(s, A.jm, A.jc);
        double m = 1.0;
        int e = 0;
        for (int k = 0; k < V; ++k) {
            const SampleNode nd = A.M.nodes[k];
            const int evv = ev[nd.v];
            const int pc = parent_config(A.M, nd, vals, lane);
            s = fbn::PcgStep(s, A.inc);
            int q;
            if (evv >= 0 && A.method == 0) {  // likelihood weighting: clamp, weigh
                q = evv;
                int de;
                m = frexp(m * A.M.prob[nd.toff + (long long)pc * nd.d + q], &de);
                e += de;
            } else {
                q = fbn::SelectValue(A.M.cdf + nd.toff + (long long)pc * nd.d, nd.d, fbn::PcgDouble(fbn::PcgOutput(s)));
                if (evv >= 0 && q != evv) m = 0.0;  // logic sampling: reject
            }
            vals[nd.v * 64 + lane] = (uint8_t)q;
            if (A.dv && active) A.dv[(long long)nd.v * total + c * A.S + s0 + lane] = (uint8_t)q;
        }
        if (A.dm && active) {
            A.dm[c * A.S + s0 + lane] = m;
            A.de[c * A.S + s0 + lane] = e;
        }
        const int cm = wave_max(active ? e : INT_MIN);
        double f = 1.0;
        if (s0 == 0) emax = cm;
        else if (cm > emax) f = ldexp(1.0, emax - cm), emax = cm;
        const double w = active ? ldexp(m, e - emax) : 0.0;
        sumw = sumw * f + wave_sum(w);
        sumw2 = sumw2 * f * f + wave_sum(w * w);
        __syncthreads();
        fbn::accumulate_marginals(A.M, vals, row, w, f, s0 == 0, lane);
        __syncthreads();
    }
    int lab = -1;
    if (sumw > 0.0) {
        for (int j = lane; j < SD; j += 64) row[j] = ev[A.M.ent[j] >> 8] >= 0 ? 0.0 : row[j] / sumw;
    } else {
        for (int j = lane; j < SD; j += 64) row[j] = 0.0;
    }
    __syncthreads();  // the row's entries are other lanes' stores
    if (lane == 0) {
        if (sumw > 0.0) {
            lab = 0;
            double mp = 0.0;  // ArgMax, strict '>' from 0 (src/Inference.cpp:92-102), as fbn_jt_run
            for (int q = 0; q < A.M.d0; ++q)
                if (row[q] > mp) mp = row[q], lab = q;
        }
        A.labels[c] = lab;
        if (A.stats) {
            A.stats[2 * c] = sumw > 0.0 ? log(sumw / (double)A.S) + (double)emax * 0.6931471805599453 : -INFINITY;
            A.stats[2 * c + 1] = sumw > 0.0 ? sumw * sumw / sumw2 : 0.0;
        }
    }
}

}  // namespace

struct fbn_sampler {
    fbn::SamplerModel M;
    int device = -1;
    DevBuf nodes, par, prob, cdf, ent, dom, evcheck;
    DevBuf evid, labels, marg, stats, cols, dv, dm, de, scratch;  // staging of the host-buffer entries
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    std::set<hipStream_t> streams_used;
    ~fbn_sampler() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};

namespace {

template <class T>
int Upload(DevBuf &b, const std::vector<T> &v) {
    if (int rc = b.ensure(std::max<size_t>(v.size() * sizeof(T), 16))) return rc;
    if (!v.empty()) FBN_HIP(hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return FBN_OK;
}

DeviceModel DevModel(const fbn_sampler *s) {
    return DeviceModel{s->nodes.as<SampleNode>(), s->par.as<int32_t>(), s->prob.as<double>(), s->cdf.as<double>(),
                       s->ent.as<int32_t>(), s->M.V, s->M.sum_dom, s->M.dom[0]};
}

int ForwardDevice(fbn_sampler *s, int64_t n, uint64_t seed, uint8_t *d_cols, hipStream_t st) {
    fbn::PcgStream R;
    fbn::PcgStreamInit(seed, R);
    ForwardArgs a;
    memcpy(a.jump, R.jump, sizeof a.jump);
    a.M = DevModel(s);
    a.state = R.state, a.inc = R.inc;
    fbn::PcgJump(R, (uint64_t)n, &a.jm, &a.jc);
    a.n = n;
    a.cols = d_cols;
    const int64_t grid = (n + 63) / 64;
    if (grid > 0x7fffffffll) return SetError(FBN_ERR_LIMIT, "forward sampling: %lld samples in one call", (long long)n);
    s->streams_used.insert(st);
    FBN_HIP(hipEventRecord(s->ev0, st));
    hipLaunchKernelGGL(sample_forward_kernel, dim3((unsigned)grid), dim3(64), (size_t)s->M.V * 64, st, a);
    FBN_HIP(hipGetLastError());
    FBN_HIP(hipEventRecord(s->ev1, st));
    s->timed = true;
    return FBN_OK;
}

int LwDevice(fbn_sampler *s, int method, const int8_t *d_ev, int64_t ncases, int64_t S, uint64_t seed,
             int64_t case_offset, int32_t *d_labels, double *d_marg, double *d_stats, uint8_t *dv, double *dm,
             int32_t *de, hipStream_t st) {
    if (ncases > 0x7fffffffll) return SetError(FBN_ERR_LIMIT, "%lld cases in one call", (long long)ncases);
    s->streams_used.insert(st);
    // as fbn_jt_run_device's check: on the device, one stream sync
    if (int rc = fbn::EvidenceCheckDevice(d_ev, ncases, s->M.V, s->dom.as<int32_t>(), s->M.dom.data(),
                                          s->evcheck.as<unsigned long long>(), st))
        return rc;
    if (!d_marg) {  // labels only: the accumulator rows live in the handle
        if (int rc = s->scratch.ensure((size_t)ncases * s->M.sum_dom * 8)) return rc;
        d_marg = s->scratch.as<double>();
    }
    fbn::PcgStream R;
    fbn::PcgStreamInit(seed, R);
    LwArgs a;
    memcpy(a.jump, R.jump, sizeof a.jump);
    a.M = DevModel(s);
    a.state = R.state, a.inc = R.inc;
    fbn::PcgJump(R, (uint64_t)63 * (uint64_t)s->M.V, &a.jm, &a.jc);
    a.ev = d_ev;
    a.ncases = ncases, a.S = S, a.case0 = case_offset, a.method = method;
    a.labels = d_labels, a.marg = d_marg, a.stats = d_stats;
    a.dv = dv, a.dm = dm, a.de = de;
    FBN_HIP(hipEventRecord(s->ev0, st));
    hipLaunchKernelGGL(sample_lw_kernel, dim3((unsigned)ncases), dim3(64), (size_t)s->M.V * 64, st, a);
    FBN_HIP(hipGetLastError());
    FBN_HIP(hipEventRecord(s->ev1, st));
    s->timed = true;
    return FBN_OK;
}

}  // namespace

extern "C" {

int fbn_sampler_create(const fbn_network *net, int device, fbn_sampler **out) {
    if (!net || !out) return SetError(FBN_ERR_ARG, "null pointer");
    *out = nullptr;
    fbn_sampler *s = new fbn_sampler;
    int rc = fbn::BuildSamplerModel(net->net, s->M);
    if (rc == FBN_OK && device >= 0) {
        s->device = device;
        rc = [&]() -> int {
            int r;
            if ((r = fbn::CheckDevice(device, nullptr)) || (r = Upload(s->nodes, s->M.nodes)) || (r = Upload(s->par, s->M.par)) || (r = Upload(s->prob, s->M.prob)) ||
                (r = Upload(s->cdf, s->M.cdf)) || (r = Upload(s->ent, s->M.ent)) || (r = Upload(s->dom, s->M.dom)) ||
                (r = s->evcheck.ensure(8)))
                return r;
            FBN_HIP(hipEventCreate(&s->ev0));
            FBN_HIP(hipEventCreate(&s->ev1));
            return FBN_OK;
        }();
    }
    if (rc) {
        delete s;
        return rc;
    }
    *out = s;
    return FBN_OK;
}

int fbn_sampler_destroy(fbn_sampler *s) {
    if (!s) return FBN_OK;
    if (s->device >= 0) {  // runs are queued on caller streams: drain those before the buffers go
        (void)hipSetDevice(s->device);
        for (hipStream_t st : s->streams_used) (void)hipStreamSynchronize(st);
    }
    delete s;
    return FBN_OK;
}

int fbn_sample_forward_device(fbn_sampler *s, int64_t n, uint64_t seed, uint8_t *d_cols, void *hip_stream) {
    if (!s || n < 0 || (n > 0 && !d_cols)) return SetError(FBN_ERR_ARG, "bad argument");
    if (s->device < 0) return SetError(FBN_ERR_NODEV, "host-only sampler (created with device < 0)");
    if (n == 0) return FBN_OK;
    if ((long double)n * s->M.V >= 9.2e18L) return SetError(FBN_ERR_ARG, "stream position beyond 2^63");
    FBN_HIP(hipSetDevice(s->device));
    return ForwardDevice(s, n, seed, d_cols, static_cast<hipStream_t>(hip_stream));
}

int fbn_sample_forward(fbn_sampler *s, int64_t n, uint64_t seed, uint8_t *cols) {
    if (!s || n < 0 || (n > 0 && !cols)) return SetError(FBN_ERR_ARG, "bad argument");
    if (n == 0) return FBN_OK;
    if ((long double)n * s->M.V >= 9.2e18L) return SetError(FBN_ERR_ARG, "stream position beyond 2^63");
    if (s->device < 0) return fbn::HostForward(s->M, n, seed, cols);
    FBN_HIP(hipSetDevice(s->device));
    const size_t bytes = (size_t)s->M.V * (size_t)n;
    if (int rc = s->cols.ensure(bytes)) return rc;
    if (int rc = ForwardDevice(s, n, seed, s->cols.as<uint8_t>(), nullptr)) return rc;
    FBN_HIP(hipMemcpy(cols, s->cols.p, bytes, hipMemcpyDeviceToHost));
    return FBN_OK;
}

int fbn_lw_run_device(fbn_sampler *s, int method, const int8_t *d_evidence, int64_t ncases, int64_t S, uint64_t seed,
                      int64_t case_offset, int32_t *d_labels, double *d_marginals, double *d_stats, void *hip_stream) {
    if (!s || (ncases > 0 && (!d_evidence || !d_labels))) return SetError(FBN_ERR_ARG, "bad argument");
    if (int rc = fbn::CheckLwShape(s->M, method, ncases, S, case_offset)) return rc;
    if (s->device < 0) return SetError(FBN_ERR_NODEV, "host-only sampler (created with device < 0)");
    if (ncases == 0) return FBN_OK;
    FBN_HIP(hipSetDevice(s->device));
    return LwDevice(s, method, d_evidence, ncases, S, seed, case_offset, d_labels, d_marginals, d_stats, nullptr, nullptr,
                    nullptr, static_cast<hipStream_t>(hip_stream));
}

static int LwHostBuffers(fbn_sampler *s, int method, const int8_t *evidence, int64_t ncases, int64_t S, uint64_t seed,
                         int64_t case_offset, int32_t *labels, double *marginals, double *stats, uint8_t *values,
                         double *mant, int32_t *expo) {
    if (int rc = fbn::CheckLwShape(s->M, method, ncases, S, case_offset)) return rc;
    if (ncases == 0) return FBN_OK;
    const int V = s->M.V, SD = s->M.sum_dom;
    if (s->device < 0) {
        if (int rc = fbn::CheckEvidenceHost(s->M, evidence, ncases)) return rc;
        return fbn::HostLw(s->M, method, evidence, ncases, S, seed, case_offset, labels, marginals, stats, values, mant, expo);
    }
    FBN_HIP(hipSetDevice(s->device));
    const size_t total = (size_t)ncases * (size_t)S;
    int rc;
    if ((rc = s->evid.ensure((size_t)ncases * V)) || (rc = s->labels.ensure((size_t)ncases * 4)) ||
        (rc = s->marg.ensure((size_t)ncases * SD * 8)) || (rc = s->stats.ensure((size_t)ncases * 16)))
        return rc;
    if (values && ((rc = s->dv.ensure(total * V)) || (rc = s->dm.ensure(total * 8)) || (rc = s->de.ensure(total * 4))))
        return rc;
    FBN_HIP(hipMemcpy(s->evid.p, evidence, (size_t)ncases * V, hipMemcpyHostToDevice));
    rc = LwDevice(s, method, s->evid.as<int8_t>(), ncases, S, seed, case_offset, s->labels.as<int32_t>(),
                  s->marg.as<double>(), s->stats.as<double>(), values ? s->dv.as<uint8_t>() : nullptr,
                  values ? s->dm.as<double>() : nullptr, values ? s->de.as<int32_t>() : nullptr, nullptr);
    if (rc) return rc;
    FBN_HIP(hipMemcpy(labels, s->labels.p, (size_t)ncases * 4, hipMemcpyDeviceToHost));
    if (marginals) FBN_HIP(hipMemcpy(marginals, s->marg.p, (size_t)ncases * SD * 8, hipMemcpyDeviceToHost));
    if (stats) FBN_HIP(hipMemcpy(stats, s->stats.p, (size_t)ncases * 16, hipMemcpyDeviceToHost));
    if (values) {
        FBN_HIP(hipMemcpy(values, s->dv.p, total * V, hipMemcpyDeviceToHost));
        FBN_HIP(hipMemcpy(mant, s->dm.p, total * 8, hipMemcpyDeviceToHost));
        FBN_HIP(hipMemcpy(expo, s->de.p, total * 4, hipMemcpyDeviceToHost));
    }
    return FBN_OK;
}

int fbn_lw_run(fbn_sampler *s, int method, const int8_t *evidence, int64_t ncases, int64_t S, uint64_t seed,
               int64_t case_offset, int32_t *labels, double *marginals, double *stats) {
    if (!s || (ncases > 0 && (!evidence || !labels))) return SetError(FBN_ERR_ARG, "bad argument");
    return LwHostBuffers(s, method, evidence, ncases, S, seed, case_offset, labels, marginals, stats, nullptr, nullptr,
                         nullptr);
}

int fbn_lw_debug_samples(fbn_sampler *s, int method, const int8_t *evidence, int64_t ncases, int64_t S, uint64_t seed,
                         int64_t case_offset, uint8_t *values, double *mantissas, int32_t *exponents) {
    if (!s || (ncases > 0 && (!evidence || !values || !mantissas || !exponents))) return SetError(FBN_ERR_ARG, "bad argument");
    if (ncases > 0 && S > 0 && (ncases > FBN_SAMPLE_DEBUG_MAX || S > FBN_SAMPLE_DEBUG_MAX / ncases))
        return SetError(FBN_ERR_LIMIT, "debug samples: more than %lld samples", (long long)FBN_SAMPLE_DEBUG_MAX);
    std::vector<int32_t> labels((size_t)std::max<int64_t>(ncases, 1));
    return LwHostBuffers(s, method, evidence, ncases, S, seed, case_offset, labels.data(), nullptr, nullptr, values,
                         mantissas, exponents);
}

int fbn_sampler_last_kernel_ms(const fbn_sampler *s, float *ms) {
    if (!s || !ms || !s->timed) return SetError(FBN_ERR_ARG, "no timed launch");
    FBN_HIP(hipEventSynchronize(s->ev1));
    FBN_HIP(hipEventElapsedTime(ms, s->ev0, s->ev1));
    return FBN_OK;
}

int fbn_score_marginals(const fbn_network *net, const double *marginals, const double *golden, int64_t ncases,
                        double *mse_sum, double *hd_sum) {
    if (!net || !marginals || !golden || !mse_sum || !hd_sum) return SetError(FBN_ERR_ARG, "null pointer");
    return fbn::ScoreMarginals(net->net.dom, marginals, golden, ncases, mse_sum, hd_sum);
}

}  // extern "C"
