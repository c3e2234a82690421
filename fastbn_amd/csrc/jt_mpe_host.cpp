// jt_mpe_host.cpp -- the host twin of jt_mpe.hip: the max-product Collect and back-trace of
// include/fastbn.h (above fbn_mpe_create) over the program of jt_mpe_program.h, one evidence case at a
// time, cases spread over CPU threads.  Only *, comparisons, frexp and ldexp: the device kernel gives
// the same bytes.  Built with -ffp-contract=off (there is nothing to contract: no adds).
#include <algorithm>
#include <cmath>
#include <thread>

#include "fbn_internal.h"
#include "jt_mpe_program.h"

namespace fbn {

int CheckMpeEvidence(const JTProgramMpe &P, const int8_t *ev, int64_t ncases) {
    for (int64_t c = 0; c < ncases; ++c)
        for (int v = 0; v < P.V; ++v) {
            const int x = ev[c * P.V + v];
            if (x < -1 || x >= P.dom[v])
                return SetError(FBN_ERR_ARG, "case %lld: evidence %d for node %d (domain %d)", (long long)c, x, v, P.dom[v]);
        }
    return FBN_OK;
}

int CheckCaseValues(const char *what, const double *value, int64_t ncases) {
    for (int64_t c = 0; c < ncases; ++c)
        if (!(value[2 * c] > 0.0))
            return SetError(FBN_ERR_LIMIT,
                            "%s: case %lld: the value underflows inside a clique (potential times messages; reported {%g, %g})",
                            what, (long long)c, value[2 * c], value[2 * c + 1]);
    return FBN_OK;
}

namespace {

// the evidence pattern of one clique for one case: mask / value words over the digit slots
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

void OneCase(const JTProgramMpe &P, const int8_t *ev, int8_t *assign, double *value, double *msg, int64_t *exps,
             int64_t *estar) {
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
                const double v = EntryValue(P, q, e, msg);
                const int32_t u = P.aux[q.up_map_off + e];
                if (v > up[u]) up[u] = v;
            }
            double mx = 0.0;
            for (int s = 0; s < q.up_Ts; ++s)
                if (up[s] > mx) mx = up[s];
            int k = 0;
            (void)std::frexp(mx, &k);
            for (int s = 0; s < q.up_Ts; ++s) up[s] = std::ldexp(up[s], -k);
            exps[q.up_exp_row - R] = k + esum;
        } else {
            double best = -1.0;
            int64_t es = -1;
            for (int64_t e = 0; e < q.T; ++e) {
                if (!mk.consistent(dg + e * q.nw, q.nw)) continue;
                const double v = EntryValue(P, q, e, msg);
                if (v > best) best = v, es = e;
            }
            if (es < 0) best = 0.0, es = 0;  // guard: validated evidence leaves an entry unmasked
            estar[c] = es;
            int k = 0;
            const double f = std::frexp(best, &k);
            ex += k + esum;
            m = std::frexp(m * f, &k);
            ex += k;
        }
    }
    value[0] = m, value[1] = (double)ex;
    for (int c : P.trace) {
        const JtMClique &q = P.cl[c];
        const uint64_t *dg = &P.dig[q.dig_off];
        int64_t es = estar[c];
        if (q.parent >= 0) {
            const Mask mk(P, q, ev);
            const int64_t ss = P.aux[q.parent_map_off + estar[q.parent]];
            double best = -1.0;
            es = -1;
            for (int64_t e = ss; e < q.T; e += q.up_Ts) {
                if (!mk.consistent(dg + e * q.nw, q.nw)) continue;
                const double v = EntryValue(P, q, e, msg);
                if (v > best) best = v, es = e;
            }
            if (es < 0) es = ss;
            estar[c] = es;
        }
        for (int j = 0; j < q.nown; ++j)
            assign[P.aux[q.vars_off + j]] = (int8_t)((dg[es * q.nw + j / 8] >> (8 * (j % 8))) & 0xFF);
    }
}

}  // namespace

int HostMpe(const JTProgramMpe &P, const int8_t *ev, int64_t ncases, int8_t *assign, double *value,
            double *messages, int32_t *exponents) {
    if (ncases == 0) return FBN_OK;
    const int nc = (int)P.cl.size();
    auto run = [&](int64_t c0, int64_t c1) {
        std::vector<double> msg((size_t)std::max<int64_t>(P.msg_rows, 1));
        std::vector<int64_t> exps((size_t)std::max(P.nsep, 1)), estar((size_t)nc);
        for (int64_t c = c0; c < c1; ++c) {
            OneCase(P, ev + c * P.V, assign + c * P.V, value + 2 * c, msg.data(), exps.data(), estar.data());
            if (messages) std::copy(msg.begin(), msg.begin() + P.msg_rows, messages + c * P.msg_rows);
            if (exponents)
                for (int s = 0; s < P.nsep; ++s) exponents[c * P.nsep + s] = (int32_t)exps[s];
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
