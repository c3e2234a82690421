// jt_em_host.cpp -- the host twin of jt_em.hip: the E-step of include/fastbn.h (above fbn_em_create)
// over the program of jt_em_program.h, one data row at a time in the stated ascending-entry order,
// rows spread over CPU threads.  *, +, /, comparisons, frexp and ldexp in the stated order, built with
// -ffp-contract=off: the device kernel gives the same per-case bytes.
#include <algorithm>
#include <cmath>
#include <thread>

#include "fbn_internal.h"
#include "jt_em_program.h"

namespace fbn {

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

// init[e] times the children's messages in clique_down order, child `skip` left out (-1: none)
inline double EntryValue(const JTProgramMpe &P, const JtMClique &q, int64_t e, const double *msg, int skip) {
    double v = P.initv[q.iv_off + e];
    for (int j = 0; j < q.k; ++j) {
        if (j == skip) continue;
        const int32_t *rec = &P.aux[q.child_off + 4 * j];
        v = v * msg[rec[1] + P.aux[rec[0] + e]];
    }
    return v;
}

// msg: the Collect messages, down: the Distribute messages (both [msg_rows]); post [cells], zeroed here
void OneCase(const JTProgramEm &E, const int8_t *ev, double *value, double *post, double *msg, double *down,
             int64_t *exps) {
    const JTProgramMpe &P = E.M;
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
                up[u] = up[u] + EntryValue(P, q, e, msg, -1);
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
                sum = sum + EntryValue(P, q, e, msg, -1);
            }
            int k = 0;
            const double f = std::frexp(sum, &k);
            ex += k + esum;
            m = std::frexp(m * f, &k);
            ex += k;
        }
    }
    if (value) value[0] = m, value[1] = (double)ex;
    if (!post) return;
    std::fill(post, post + E.cells, 0.0);
    for (int c : P.trace) {
        const JtMClique &q = P.cl[c];
        const JtEClique &qe = E.ecl[c];
        if (q.parent >= 0) {
            const JtMClique &qp = P.cl[q.parent];
            const Mask mp(P, qp, ev);
            const uint64_t *dgp = &P.dig[qp.dig_off];
            double *D = down + q.up_row;
            for (int s = 0; s < q.up_Ts; ++s) D[s] = 0.0;
            for (int64_t e = 0; e < qp.T; ++e) {
                if (!mp.consistent(dgp + e * qp.nw, qp.nw)) continue;
                double t = EntryValue(P, qp, e, msg, qe.slot);
                if (qp.parent >= 0) t = t * down[qp.up_row + P.aux[qp.up_map_off + e]];
                const int32_t s = P.aux[q.parent_map_off + e];
                D[s] = D[s] + t;
            }
            double mx = 0.0;
            for (int s = 0; s < q.up_Ts; ++s)
                if (D[s] > mx) mx = D[s];
            int k = 0;
            (void)std::frexp(mx, &k);
            for (int s = 0; s < q.up_Ts; ++s) D[s] = std::ldexp(D[s], -k);
        }
        if (qe.nfam == 0) continue;
        const Mask mk(P, q, ev);
        const uint64_t *dg = &P.dig[q.dig_off];
        auto belief = [&](int64_t e) {
            double b = EntryValue(P, q, e, msg, -1);
            if (q.parent >= 0) b = b * down[q.up_row + P.aux[q.up_map_off + e]];
            return b;
        };
        double Z = 0.0;
        for (int64_t e = 0; e < q.T; ++e)
            if (mk.consistent(dg + e * q.nw, q.nw)) Z = Z + belief(e);
        for (int64_t e = 0; e < q.T; ++e) {
            if (!mk.consistent(dg + e * q.nw, q.nw)) continue;
            const double r = belief(e) / Z;
            for (int f = 0; f < qe.nfam; ++f) {
                const int32_t cell = E.eaux[E.eaux[qe.fam_off + kEmFamRec * f + 3] + e];
                post[cell] = post[cell] + r;
            }
        }
    }
}

}  // namespace

int HostEmEstep(const JTProgramEm &E, const int8_t *data, int64_t ncases, double *counts, double *value, double *post) {
    const JTProgramMpe &P = E.M;
    if (counts) std::fill(counts, counts + E.cells, 0.0);
    if (ncases == 0) return FBN_OK;
    const bool need_post = counts || post;
    // blocks of cases: the threads fill the block's posteriors, then the counts take them in case order
    const int64_t block = post ? ncases : std::min<int64_t>(ncases, 1024);
    std::vector<double> buf;
    if (!post && counts) buf.resize((size_t)(block * E.cells));
    for (int64_t b0 = 0; b0 < ncases; b0 += block) {
        const int64_t nb = std::min(block, ncases - b0);
        double *pb = post ? post : (counts ? buf.data() : nullptr);
        auto run = [&](int64_t c0, int64_t c1) {
            std::vector<double> msg((size_t)std::max<int64_t>(P.msg_rows, 1)), down(msg.size());
            std::vector<int64_t> exps((size_t)std::max(P.nsep, 1));
            for (int64_t c = c0; c < c1; ++c)
                OneCase(E, data + (b0 + c) * P.V, value ? value + 2 * (b0 + c) : nullptr,
                        need_post ? pb + c * E.cells : nullptr, msg.data(), down.data(), exps.data());
        };
        const int T = (int)std::min<int64_t>(HostThreads(), nb);
        std::vector<std::thread> th;
        for (int t = 1; t < T; ++t) th.emplace_back(run, nb * t / T, nb * (t + 1) / T);
        run(0, nb / T);
        for (auto &x : th) x.join();
        if (counts)
            for (int64_t c = 0; c < nb; ++c)
                for (int64_t i = 0; i < E.cells; ++i) counts[i] = counts[i] + pb[c * E.cells + i];
    }
    return FBN_OK;
}

}  // namespace fbn
