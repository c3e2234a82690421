// jt_psample_host.cpp -- the host twin of jt_psample.hip: the sum-product Collect and the sampled
// back-trace of include/fastbn.h (above fbn_psample_create) over the program of jt_mpe_program.h, one
// evidence case at a time (one Collect, then its S draws), cases spread over CPU threads.  *, +,
// comparisons, frexp and ldexp in the stated order, built with -ffp-contract=off: the device kernel gives
// the same bytes.
#include <algorithm>
#include <cmath>
#include <thread>

#include "fbn_internal.h"
#include "jt_psample_program.h"

namespace fbn {

int CheckPsampleShape(const JTProgramMpe &P, int64_t ncases, int64_t S, int64_t case_offset) {
    if (S < 1) return SetError(FBN_ERR_ARG, "samples per case must be >= 1 (got %lld)", (long long)S);
    if (ncases < 0 || case_offset < 0) return SetError(FBN_ERR_ARG, "bad argument");
    if ((long double)ncases * (long double)S > 2147483647.0L)
        return SetError(FBN_ERR_LIMIT, "%lld cases x %lld samples: more than 2^31 - 1 samples per call", (long long)ncases,
                        (long long)S);
    if ((long double)ncases * (long double)S * (long double)P.V >= 9.2e18L)
        return SetError(FBN_ERR_LIMIT, "the samples are beyond int64 indexing");
    const long double pos = ((long double)case_offset + (long double)ncases) * (long double)S * (long double)P.cl.size();
    if (pos >= 9.2e18L) return SetError(FBN_ERR_ARG, "stream position beyond 2^63");
    return FBN_OK;
}

namespace {

struct Mask {
    uint64_t M[JT_MAX_DIG_WORDS], W[JT_MAX_DIG_WORDS];
    Mask(const JTProgramMpe &P, const JtMClique &q, const int8_t *ev) {
        for (int k = 0; k < JT_MAX_DIG_WORDS; ++k) M[k] = W[k] = 0;
        for (int j = 0; j < q.nv; ++j) {
            const int x = ev[P.aux[q.vars_off + j]];
            if (x < 0) continue;
            M[j / 8] |= 0xFFull << (8 * (j % 8));
            W[j / 8] |= (uint64_t)x << (8 * (j % 8));
        }
    }
    bool consistent(const uint64_t *d, int nw) const {
        for (int k = 0; k < nw; ++k)
            if ((d[k] & M[k]) != W[k]) return false;
        return true;
    }
};

// v(e): the initial potential times the children's messages, clique_down order
inline double EntryValue(const JTProgramMpe &P, const JtMClique &q, int64_t e, const double *msg) {
    double v = P.initv[q.iv_off + e];
    for (int j = 0; j < q.k; ++j) {
        const int32_t *rec = &P.aux[q.child_off + 4 * j];
        v = v * msg[rec[1] + P.aux[rec[0] + e]];
    }
    return v;
}

// the E-step's Collect (jt_em_host.cpp), to the operation
void Collect(const JTProgramMpe &P, const int8_t *ev, double *value, double *msg, int64_t *exps) {
    const int64_t R = P.msg_rows;
    double m = 1.0;
    int64_t ex = 0;
    for (int c : P.collect) {
        const JtMClique &q = P.cl[c];
        const Mask mk(P, q, ev);
        const uint64_t *dg = &P.dig[q.dig_off];
        int64_t esum = 0;
        for (int j = 0; j < q.k; ++j) esum += exps[P.aux[q.child_off + 4 * j + 2] - R];
        if (q.parent >= 0) {
            double *up = msg + q.up_row;
            for (int s = 0; s < q.up_Ts; ++s) up[s] = 0.0;
            for (int64_t e = 0; e < q.T; ++e) {
                if (!mk.consistent(dg + e * q.nw, q.nw)) continue;
                const int32_t u = P.aux[q.up_map_off + e];
                up[u] = up[u] + EntryValue(P, q, e, msg);
            }
            double mx = 0.0;
            for (int s = 0; s < q.up_Ts; ++s)
                if (up[s] > mx) mx = up[s];
            int k = 0;
            (void)std::frexp(mx, &k);
            for (int s = 0; s < q.up_Ts; ++s) up[s] = std::ldexp(up[s], -k);
            exps[q.up_exp_row - R] = k + esum;
        } else {
            double sum = 0.0;
            for (int64_t e = 0; e < q.T; ++e) {
                if (!mk.consistent(dg + e * q.nw, q.nw)) continue;
                sum = sum + EntryValue(P, q, e, msg);
            }
            int k = 0;
            const double f = std::frexp(sum, &k);
            ex += k + esum;
            m = std::frexp(m * f, &k);
            ex += k;
        }
    }
    value[0] = m, value[1] = (double)ex;
}

// one draw: s is the stream state at the draw's first position; row [V]
void Draw(const JTProgramMpe &P, const int8_t *ev, const double *msg, U128 s, U128 inc, int64_t *estar, int8_t *row) {
    for (int c : P.trace) {
        const JtMClique &q = P.cl[c];
        const uint64_t *dg = &P.dig[q.dig_off];
        const Mask mk(P, q, ev);
        s = PcgStep(s, inc);  // every clique takes one draw
        const double u = PcgDouble(PcgOutput(s));
        const int64_t first = q.parent >= 0 ? P.aux[q.parent_map_off + estar[q.parent]] : 0;
        const int64_t stride = q.parent >= 0 ? q.up_Ts : 1;
        double Z = 0.0;
        for (int64_t e = first; e < q.T; e += stride)
            if (mk.consistent(dg + e * q.nw, q.nw)) Z = Z + EntryValue(P, q, e, msg);
        const double t = u * Z;
        double run = 0.0;
        int64_t es = -1, last = -1;
        for (int64_t e = first; e < q.T && es < 0; e += stride) {
            if (!mk.consistent(dg + e * q.nw, q.nw)) continue;
            const double v = EntryValue(P, q, e, msg);
            run = run + v;
            if (run > t) es = e;
            if (v > 0.0) last = e;
        }
        if (es < 0) es = last;   // u * Z rounded up to Z
        if (es < 0) es = first;  // guard: a case of value 0 (reported by the caller)
        estar[c] = es;
        for (int j = 0; j < q.nown; ++j)
            row[P.aux[q.vars_off + j]] = (int8_t)((dg[es * q.nw + j / 8] >> (8 * (j % 8))) & 0xFF);
    }
}

}  // namespace

int HostPsample(const JTProgramMpe &P, const int8_t *ev, int64_t ncases, int64_t S, uint64_t seed, int64_t case_offset,
                int8_t *samples, double *value) {
    if (ncases == 0) return FBN_OK;
    const uint64_t nc = P.cl.size();
    PcgStream R;
    PcgStreamInit(seed, R);
    auto run = [&](int64_t c0, int64_t c1) {
        std::vector<double> msg((size_t)std::max<int64_t>(P.msg_rows, 1));
        std::vector<int64_t> exps((size_t)std::max(P.nsep, 1)), estar((size_t)nc);
        for (int64_t c = c0; c < c1; ++c) {
            Collect(P, ev + c * P.V, value + 2 * c, msg.data(), exps.data());
            for (int64_t s = 0; s < S; ++s) {
                const uint64_t pos = ((uint64_t)(case_offset + c) * (uint64_t)S + (uint64_t)s) * nc;
                Draw(P, ev + c * P.V, msg.data(), PcgJumpTo(R.state, pos, R.jump), R.inc, estar.data(),
                     samples + (c * S + s) * P.V);
            }
        }
    };
    const int T = (int)std::min<int64_t>(HostThreads(), ncases);
    std::vector<std::thread> th;
    for (int t = 1; t < T; ++t) th.emplace_back(run, ncases * t / T, ncases * (t + 1) / T);
    run(0, ncases / T);
    for (auto &x : th) x.join();
    return FBN_OK;
}

}  // namespace fbn
