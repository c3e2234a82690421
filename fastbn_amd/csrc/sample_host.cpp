// sample_host.cpp -- host side of the sampling engine: the flattened network, the seeded stream's
// jump tables, and the host twin of the kernels in sample.hip (device < 0 samplers).
//
// Forward sampling, likelihood weighting (the reference's `-a 5`) and probabilistic logic sampling
// (`-a 4`) -- both only print "under development" there (src/main.cpp:97-121) -- walk the network in
// synth.cpp's topological order and pick each value by ForwardSample's rule from the cdf row of the
// sample's own parent values.  The random stream is numpy's PCG64(seed); the draw of (k-th variable
// in topological order, sample i) sits at a fixed stream position, reached by jump-ahead:
//   forward sampling  p = k * n + i                       (synth.cpp's map: outputs equal it bit for bit)
//   inference         p = i * V + k,  i = (case_offset + c) * S + s
// so a case's result depends on (seed, global case index, S) only.  Every variable consumes its
// position whether or not its draw is used.
//
// HostImportance is the inference loop itself: HostLw calls it without an importance function, EPIS-BN's
// twin (epis_host.cpp) with the lambda rows of its pre-propagation (epis_model.h).
//
// The twin repeats the kernels' arithmetic operation for operation -- 64-sample chunks, the same
// butterfly and per-entry summation orders, the same power-of-two rescaling -- so the two agree bit
// for bit on (value, mantissa, exponent) and on every sum.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <thread>

#include "epis_model.h"
#include "fbn_internal.h"
#include "sample_model.h"

namespace fbn {

int BuildSamplerModel(const Network &net, SamplerModel &M) {
    const int V = net.n();
    if (V < 1) return SetError(FBN_ERR_ARG, "sampler: empty network");
    if (V > FBN_SAMPLE_MAX_VARS)
        return SetError(FBN_ERR_LIMIT, "sampler: %d variables (limit %d)", V, FBN_SAMPLE_MAX_VARS);
    const std::vector<int> order = TopoOrder(net);
    if ((int)order.size() != V) return SetError(FBN_ERR_ARG, "network has a cycle");
    M = SamplerModel();
    M.V = V;
    M.dom.assign(net.dom.begin(), net.dom.end());
    std::vector<int32_t> moff(V);
    for (int v = 0; v < V; ++v) {
        if (net.dom[v] < 1 || net.dom[v] > 255) return SetError(FBN_ERR_ARG, "node %d has %d states", v, net.dom[v]);
        moff[v] = M.sum_dom;
        for (int q = 0; q < net.dom[v]; ++q) M.ent.push_back(v << 8 | q);
        M.sum_dom += net.dom[v];
    }
    // table sizes first: nothing is allocated for a network past the cap
    int64_t cells = 0;
    for (int v = 0; v < V; ++v) {
        int64_t c = net.dom[v];
        for (int p : net.given[v]) {
            c *= net.dom[p];
            if (c > FBN_PARAM_MAX_CELLS) break;
        }
        cells += c;
        if (c > FBN_PARAM_MAX_CELLS || cells > FBN_PARAM_MAX_CELLS)
            return SetError(FBN_ERR_LIMIT, "sampler: tables beyond %lld cells (node %d)", (long long)FBN_PARAM_MAX_CELLS, v);
    }
    M.cells = cells;
    M.prob.resize((size_t)cells);
    M.cdf.resize((size_t)cells);
    int64_t toff = 0;
    for (int v : order) {
        const std::vector<int> &g = net.given[v];
        SampleNode nd;
        nd.v = v, nd.d = net.dom[v], nd.npar = (int)g.size(), nd.poff = (int)(M.par.size() / 2);
        nd.toff = (int32_t)toff, nd.moff = moff[v];
        int64_t ncfg = 1;
        for (int p : g) {
            M.par.push_back(p);
            M.par.push_back(net.dom[p]);
            ncfg *= net.dom[p];
        }
        // rows of every parent configuration (GIVEN order, last fastest), as ForwardSample builds them
        const int d = nd.d;
        std::vector<int> gv(g.size(), 0), asc(net.parents_asc[v].size(), 0);
        for (int64_t pc = 0; pc < ncfg; ++pc) {
            for (size_t a = 0; a < asc.size(); ++a)
                for (size_t j = 0; j < g.size(); ++j)
                    if (g[j] == net.parents_asc[v][a]) asc[a] = gv[j];
            double acc = 0.0;
            for (int q = 0; q < d; ++q) {
                const double p = net.Prob(v, q, asc.data());
                acc += p;
                M.prob[(size_t)(toff + pc * d + q)] = p;
                M.cdf[(size_t)(toff + pc * d + q)] = acc;
            }
            for (int j = (int)g.size() - 1; j >= 0; --j) {
                if (++gv[j] < net.dom[g[j]]) break;
                gv[j] = 0;
            }
        }
        toff += ncfg * d;
        M.nodes.push_back(nd);
    }
    if (M.par.empty()) M.par.assign(2, 0);
    return FBN_OK;
}

void PcgStreamInit(uint64_t seed, PcgStream &R) {
    uint64_t st[2], inc[2];
    Pcg64Seed(seed, st, inc);
    R.state = U128{st[0], st[1]};
    R.inc = U128{inc[0], inc[1]};
    // 2^j steps: x -> m x + c twice is x -> m^2 x + (m + 1) c
    U128 m{kPcgMultHi, kPcgMultLo}, c = R.inc;
    for (int j = 0; j < 64; ++j) {
        R.jump[4 * j] = m.hi, R.jump[4 * j + 1] = m.lo, R.jump[4 * j + 2] = c.hi, R.jump[4 * j + 3] = c.lo;
        c = Affine(c, m, c);
        m = Affine(m, m, U128{0, 0});
    }
}

void PcgJump(const PcgStream &R, uint64_t delta, U128 *mult, U128 *plus) {
    U128 am{0, 1}, ap{0, 0};
    for (int j = 0; j < 64 && (delta >> j) != 0; ++j)
        if ((delta >> j) & 1) {
            const U128 m{R.jump[4 * j], R.jump[4 * j + 1]}, c{R.jump[4 * j + 2], R.jump[4 * j + 3]};
            am = Affine(am, m, U128{0, 0});
            ap = Affine(ap, m, c);
        }
    *mult = am, *plus = ap;
}

void ParallelRanges(int64_t n, int64_t grain, const std::function<void(int64_t, int64_t)> &fn) {
    const int T = (int)std::min<int64_t>(HostThreads(), std::max<int64_t>(1, n / grain));
    std::vector<std::thread> th;
    for (int t = 1; t < T; ++t) th.emplace_back(fn, n * t / T, n * (t + 1) / T);
    fn(0, n / T);
    for (auto &x : th) x.join();
}

double Butterfly(double *a) {
    double t[64];
    for (int off = 32; off >= 1; off >>= 1) {
        for (int i = 0; i < 64; ++i) t[i] = a[i] + a[i ^ off];
        std::copy(t, t + 64, a);
    }
    return a[0];
}

double HostChunkWeights(WeightState &ws, const double *m, const int *e, int act, bool first, double *w) {
    int cm = INT_MIN;
    for (int l = 0; l < act; ++l) cm = std::max(cm, e[l]);
    const double f = WeightRescale(ws, cm, first);
    double a[64], a2[64];
    for (int l = 0; l < 64; ++l) {
        w[l] = a[l] = l < act ? ldexp(m[l], e[l] - ws.emax) : 0.0;
        a2[l] = w[l] * w[l];
    }
    const double sw = Butterfly(a);
    WeightAdd(ws, f, sw, Butterfly(a2));
    return f;
}

void HostAccumulateChunk(const SamplerModel &M, const uint8_t *x, const double *w, int act, double f, bool first,
                         double *row) {
    for (int j = 0; j < M.sum_dom; ++j) {
        const int v = M.ent[j] >> 8, q = M.ent[j] & 255;
        double acc = first ? 0.0 : row[j] * f;
        const uint8_t *xv = x + (size_t)v * 64;
        for (int l = 0; l < act; ++l) acc += xv[l] == q ? w[l] : 0.0;
        row[j] = acc;
    }
}

void HostFinishCase(const SamplerModel &M, const int8_t *e_row, double *row, const WeightState &ws, int64_t S,
                    int32_t *label, double *stats) {
    if (ws.sumw > 0.0) {
        for (int j = 0; j < M.sum_dom; ++j) row[j] = e_row[M.ent[j] >> 8] >= 0 ? 0.0 : row[j] / ws.sumw;
    } else {
        std::fill(row, row + M.sum_dom, 0.0);
    }
    *label = QueryLabel(row, M.dom[0], ws.sumw);
    if (stats) stats[0] = WeightLogEvidence(ws, S), stats[1] = WeightEss(ws);
}

int HostForward(const SamplerModel &M, int64_t n, uint64_t seed, uint8_t *cols) {
    if (n == 0) return FBN_OK;
    PcgStream R;
    PcgStreamInit(seed, R);
    U128 jm, jc;  // one variable on: n positions
    PcgJump(R, (uint64_t)n, &jm, &jc);
    ParallelRanges(n, 4096, [&](int64_t a, int64_t b) {
        for (int64_t i = a; i < b; ++i) {
            U128 s = PcgJumpTo(R.state, (uint64_t)i, R.jump);
            for (const SampleNode &nd : M.nodes) {
                const int pc = ParentConfig(M, nd, cols + i, (size_t)n);
                const double u = PcgDouble(PcgOutput(PcgStep(s, R.inc)));
                s = Affine(s, jm, jc);
                cols[(size_t)nd.v * n + i] = (uint8_t)SelectValue(M.cdf.data() + nd.toff + (int64_t)pc * nd.d, nd.d, u);
            }
        }
    });
    return FBN_OK;
}

int CheckEvidenceHost(const SamplerModel &M, const int8_t *ev, int64_t ncases) {
    for (int64_t c = 0; c < ncases; ++c)
        for (int v = 0; v < M.V; ++v) {
            const int x = ev[c * M.V + v];
            if (x < -1 || x >= M.dom[v])
                return SetError(FBN_ERR_ARG, "case %lld: evidence %d for node %d (domain %d)", (long long)c, x, v, M.dom[v]);
        }
    return FBN_OK;
}

int CheckLwShape(const SamplerModel &M, int method, int64_t ncases, int64_t S, int64_t case_offset) {
    if (method != 0 && method != 1) return SetError(FBN_ERR_ARG, "method %d (0 likelihood weighting, 1 logic sampling)", method);
    if (S < 1) return SetError(FBN_ERR_ARG, "samples per case must be >= 1 (got %lld)", (long long)S);
    if (ncases < 0 || case_offset < 0) return SetError(FBN_ERR_ARG, "bad argument");
    const long double pos = ((long double)case_offset + (long double)ncases) * (long double)S + 64.0L;
    if (pos * (long double)M.V >= 9.2e18L) return SetError(FBN_ERR_ARG, "stream position beyond 2^63");
    return FBN_OK;
}

int HostLw(const SamplerModel &M, int method, const int8_t *ev, int64_t ncases, int64_t S, uint64_t seed,
           int64_t case_offset, int32_t *labels, double *marg, double *stats, uint8_t *dbg_vals, double *dbg_m,
           int32_t *dbg_e) {
    return HostImportance(M, method, ev, ncases, S, seed, case_offset, nullptr, 0.0, nullptr, labels, marg, stats, dbg_vals,
                          dbg_m, dbg_e);
}

int HostImportance(const SamplerModel &M, int method, const int8_t *ev, int64_t ncases, int64_t S, uint64_t seed,
                   int64_t case_offset, const double *lam, double eps, const double *lbp_stats, int32_t *labels,
                   double *marg, double *stats, uint8_t *dbg_vals, double *dbg_m, int32_t *dbg_e) {
    if (ncases == 0) return FBN_OK;
    const int V = M.V, SD = M.sum_dom;
    const size_t total = (size_t)ncases * (size_t)S;
    PcgStream R;
    PcgStreamInit(seed, R);
    ParallelRanges(ncases, 1, [&](int64_t c0, int64_t c1) {
        std::vector<uint8_t> x((size_t)V * 64);
        std::vector<double> own((size_t)SD);
        for (int64_t c = c0; c < c1; ++c) {
            const int8_t *e_row = ev + c * V;
            double *row = marg ? marg + c * SD : own.data();
            WeightState ws;
            for (int64_t s0 = 0; s0 < S; s0 += 64) {
                const int act = (int)std::min<int64_t>(64, S - s0);
                double m[64], w[64];
                int e[64];
                for (int l = 0; l < act; ++l) {
                    const uint64_t i = (uint64_t)(case_offset + c) * (uint64_t)S + (uint64_t)(s0 + l);
                    U128 s = PcgJumpTo(R.state, i * (uint64_t)V, R.jump);
                    double mm = 1.0;
                    int ee = 0;
                    for (const SampleNode &nd : M.nodes) {
                        const int pc = ParentConfig(M, nd, x.data() + l, 64);
                        const int evv = e_row[nd.v];
                        s = PcgStep(s, R.inc);
                        int q;
                        if (evv >= 0 && method == 0) {
                            q = evv;
                            int de;
                            mm = frexp(mm * M.prob[(size_t)nd.toff + (size_t)pc * nd.d + q], &de);
                            ee += de;
                        } else if (lam) {  // EPIS-BN: draw from P * lambda, weigh by the ratio
                            double fac;
                            q = EpisDraw(M.prob.data() + nd.toff + (int64_t)pc * nd.d, lam + c * SD + nd.moff, nd.d,
                                         EpisCutoff(eps, nd.d), PcgDouble(PcgOutput(s)), &fac);
                            int de;
                            mm = frexp(mm * fac, &de);
                            ee += de;
                        } else {
                            q = SelectValue(M.cdf.data() + nd.toff + (int64_t)pc * nd.d, nd.d, PcgDouble(PcgOutput(s)));
                            if (evv >= 0 && q != evv) mm = 0.0;
                        }
                        x[(size_t)nd.v * 64 + l] = (uint8_t)q;
                        if (dbg_vals) dbg_vals[(size_t)nd.v * total + (size_t)c * S + s0 + l] = (uint8_t)q;
                    }
                    m[l] = mm, e[l] = ee;
                    if (dbg_m) dbg_m[(size_t)c * S + s0 + l] = mm, dbg_e[(size_t)c * S + s0 + l] = ee;
                }
                const double f = HostChunkWeights(ws, m, e, act, s0 == 0, w);
                HostAccumulateChunk(M, x.data(), w, act, f, s0 == 0, row);
            }
            double *st = stats ? stats + (lam ? 4 : 2) * c : nullptr;
            HostFinishCase(M, e_row, row, ws, S, labels + c, st);
            if (st && lam) st[2] = lbp_stats ? lbp_stats[2 * c] : 0.0, st[3] = lbp_stats ? lbp_stats[2 * c + 1] : 0.0;
        }
    });
    return FBN_OK;
}

int ScoreMarginals(const std::vector<int> &dom, const double *marginals, const double *golden, int64_t ncases,
                   double *mse_sum, double *hd_sum) {
    int SD = 0;
    for (int d : dom) SD += d;
    auto round7 = [](double number) {  // Round(x, 7), src/Inference.cpp:195-206
        long long integerpart = (long long)number;
        number -= integerpart;
        for (int i = 0; i < 7; ++i) number *= 10;
        number = (double)(long long)(number + 0.5);
        for (int i = 0; i < 7; ++i) number /= 10;
        return integerpart + number;
    };
    double mse = 0.0, hd = 0.0;
    for (int64_t c = 0; c < ncases; ++c) {  // CalculateMSE / CalculateHellingerDistance (:153-193)
        const double *a = marginals + c * SD, *x = golden + c * SD;
        int num = 0, off = 0;
        double e1 = 0.0, e2 = 0.0;
        for (size_t v = 0; v < dom.size(); ++v) {
            if (x[off] > 0) {
                num += dom[v];
                for (int j = 0; j < dom[v]; ++j) {
                    double r = round7(a[off + j]);
                    e1 += pow(r - x[off + j], 2);
                    e2 += pow(sqrt(r) - sqrt(x[off + j]), 2);
                }
            }
            off += dom[v];
        }
        mse += sqrt(e1 / num);
        hd += sqrt(e2 / num);
    }
    *mse_sum = mse;
    *hd_sum = hd;
    return FBN_OK;
}

}  // namespace fbn
