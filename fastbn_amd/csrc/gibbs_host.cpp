// gibbs_host.cpp -- host side of the Gibbs sampler: the children CSR with its underflow guard, the
// argument checks, and the host twin of gibbs.hip (device < 0 handles): the same units of 64 chains, the
// same stream positions, the same conditional (gibbs_model.h compiles it on both sides), the same
// butterfly, sweep and chunk summation orders -- so the two agree bit for bit.
#include <algorithm>
#include <cmath>
#include <vector>

#include "fbn_internal.h"
#include "gibbs_model.h"

namespace fbn {

int BuildGibbsModel(const SamplerModel &M, GibbsModel &G) {
    const int V = M.V;
    G = GibbsModel();
    std::vector<int> pos((size_t)V);
    for (int t = 0; t < V; ++t) pos[(size_t)M.nodes[(size_t)t].v] = t;
    // the smallest positive entry of every node's tables
    std::vector<double> least((size_t)V, 1.0);
    for (int t = 0; t < V; ++t) {
        const int64_t end = t + 1 < V ? M.nodes[(size_t)t + 1].toff : M.cells;
        for (int64_t j = M.nodes[(size_t)t].toff; j < end; ++j)
            if (M.prob[(size_t)j] > 0.0) least[(size_t)t] = std::min(least[(size_t)t], M.prob[(size_t)j]);
        G.dmax = std::max(G.dmax, (int)M.nodes[(size_t)t].d);
    }
    // children by ascending position: a child's position is above its parents', so one pass in order
    std::vector<std::vector<int32_t>> ch((size_t)V);
    for (int t = 0; t < V; ++t) {
        const SampleNode &nd = M.nodes[(size_t)t];
        int32_t stride = 1;
        for (int j = nd.npar - 1; j >= 0; --j) {
            const int p = M.par[2 * (size_t)(nd.poff + j)];
            ch[(size_t)pos[(size_t)p]].push_back(t);
            ch[(size_t)pos[(size_t)p]].push_back(stride);
            stride *= M.par[2 * (size_t)(nd.poff + j) + 1];
        }
    }
    G.coff.push_back(0);
    for (int t = 0; t < V; ++t) {
        double prod = least[(size_t)t];
        for (size_t e = 0; e < ch[(size_t)t].size(); e += 2) prod *= least[(size_t)ch[(size_t)t][e]];
        if (prod < FBN_GIBBS_MIN_PRODUCT)
            return SetError(FBN_ERR_LIMIT,
                            "gibbs: node %d: the smallest table entries of the node and its %zu children multiply to %g, "
                            "below 2^-969: a conditional could underflow",
                            M.nodes[(size_t)t].v, ch[(size_t)t].size() / 2, prod);
        G.child.insert(G.child.end(), ch[(size_t)t].begin(), ch[(size_t)t].end());
        G.coff.push_back((int32_t)(G.child.size() / 2));
    }
    if (G.child.empty()) G.child.assign(2, 0);
    return FBN_OK;
}

int CheckGibbsShape(const SamplerModel &M, int64_t ncases, int64_t chains, int64_t burn_in, int64_t sweeps,
                    int64_t case_offset) {
    if (chains < 1) return SetError(FBN_ERR_ARG, "chains per case must be >= 1 (got %lld)", (long long)chains);
    if (sweeps < 1) return SetError(FBN_ERR_ARG, "counted sweeps must be >= 1 (got %lld)", (long long)sweeps);
    if (burn_in < 0) return SetError(FBN_ERR_ARG, "burn-in sweeps must be >= 0 (got %lld)", (long long)burn_in);
    if (ncases < 0 || case_offset < 0) return SetError(FBN_ERR_ARG, "bad argument");
    const long double P = (long double)M.V * (1.0L + (long double)burn_in + (long double)sweeps);
    const long double g = ((long double)case_offset + (long double)ncases) * (long double)chains + 64.0L;
    if (g * P >= 9.2e18L) return SetError(FBN_ERR_ARG, "stream position beyond 2^63");
    if ((long double)ncases * (long double)((chains + 63) / 64) > 2147483647.0L)
        return SetError(FBN_ERR_LIMIT, "more than 2^31 - 1 units (case, 64 chains) in one call");
    return FBN_OK;
}

int HostGibbs(const SamplerModel &M, const GibbsModel &GM, const int8_t *ev, int64_t ncases, int64_t chains,
              int64_t burn_in, int64_t sweeps, uint64_t seed, int64_t case_offset, int32_t *labels, double *marg,
              int8_t *states) {
    if (ncases == 0) return FBN_OK;
    const int V = M.V, SD = M.sum_dom;
    const GibbsView G = HostGibbsView(M, GM);
    const int64_t chunks = (chains + 63) / 64, units = ncases * chunks, passes = GibbsPasses(burn_in, sweeps);
    const uint64_t P = (uint64_t)V * (uint64_t)passes;
    std::vector<double> ws((size_t)units * (size_t)SD);
    PcgStream R;
    PcgStreamInit(seed, R);
    ParallelRanges(units, 1, [&](int64_t u0, int64_t u1) {
        std::vector<uint8_t> x((size_t)V * 64);
        std::vector<double> g((size_t)GM.dmax * 64), term((size_t)GM.dmax * 64);
        for (int64_t u = u0; u < u1; ++u) {
            const int64_t c = u / chunks, j0 = (u % chunks) * 64;
            const int act = (int)std::min<int64_t>(64, chains - j0);
            const int8_t *e_row = ev + c * V;
            double *acc = ws.data() + (size_t)u * SD;
            std::fill(acc, acc + SD, 0.0);
            U128 s[64];
            for (int ln = 0; ln < act; ++ln)
                s[ln] = PcgJumpTo(R.state, ((uint64_t)(case_offset + c) * (uint64_t)chains + (uint64_t)(j0 + ln)) * P, R.jump);
            for (int t = 0; t < V; ++t) {  // the start: likelihood weighting's draw without the weight
                const SampleNode &nd = M.nodes[(size_t)t];
                for (int ln = 0; ln < act; ++ln) {
                    s[ln] = PcgStep(s[ln], R.inc);
                    const int pc = GibbsParentConfig(G, nd, x.data() + ln);
                    x[(size_t)nd.v * 64 + ln] =
                        (uint8_t)(e_row[nd.v] >= 0 ? e_row[nd.v]
                                                   : SelectValue(G.cdf + nd.toff + (int64_t)pc * nd.d, nd.d, PcgDouble(PcgOutput(s[ln]))));
                }
            }
            for (int64_t p = 1; p < passes; ++p) {
                const bool counted = p > burn_in;
                for (int t = 0; t < V; ++t) {
                    const SampleNode &nd = M.nodes[(size_t)t];
                    for (int ln = 0; ln < act; ++ln) s[ln] = PcgStep(s[ln], R.inc);
                    if (e_row[nd.v] >= 0) continue;
                    if (counted) std::fill(term.begin(), term.begin() + (size_t)nd.d * 64, 0.0);
                    for (int ln = 0; ln < act; ++ln) {
                        const int xo = x[(size_t)nd.v * 64 + ln];
                        const double tot = GibbsConditional(G, t, x.data() + ln, nullptr, g.data() + ln);
                        const int xn = tot == 0.0 ? xo : GibbsSelect(g.data() + ln, nd.d, PcgDouble(PcgOutput(s[ln])), tot);
                        if (counted)
                            for (int k = 0; k < nd.d; ++k) term[(size_t)k * 64 + ln] = GibbsTerm(g.data() + ln, k, tot, xo);
                        x[(size_t)nd.v * 64 + ln] = (uint8_t)xn;
                    }
                    if (counted)
                        for (int k = 0; k < nd.d; ++k) acc[nd.moff + k] = acc[nd.moff + k] + Butterfly(term.data() + (size_t)k * 64);
                }
            }
            if (states)
                for (int ln = 0; ln < act; ++ln)
                    for (int v = 0; v < V; ++v)
                        states[((size_t)c * (size_t)chains + (size_t)(j0 + ln)) * V + v] = (int8_t)x[(size_t)v * 64 + ln];
        }
    });
    // the finish: a case's chunk rows in ascending order, the division, zeros for the observed variables
    const double denom = (double)(chains * sweeps);
    std::vector<double> own((size_t)SD);
    for (int64_t c = 0; c < ncases; ++c) {
        double *row = marg ? marg + c * SD : own.data();
        for (int j = 0; j < SD; ++j) {
            double sum = 0.0;
            for (int64_t k = 0; k < chunks; ++k) sum = sum + ws[(size_t)(c * chunks + k) * SD + j];
            row[j] = ev[c * V + (M.ent[(size_t)j] >> 8)] >= 0 ? 0.0 : sum / denom;
        }
        labels[c] = QueryLabel(row, M.dom[0], 1.0);
    }
    return FBN_OK;
}

int CheckGibbsStates(const SamplerModel &M, const int8_t *states, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        for (int v = 0; v < M.V; ++v) {
            const int x = states[i * M.V + v];
            if (x < 0 || x >= M.dom[(size_t)v])
                return SetError(FBN_ERR_ARG, "assignment %lld: value %d for node %d (domain %d)", (long long)i, x, v, M.dom[(size_t)v]);
        }
    return FBN_OK;
}

int HostGibbsConditionals(const SamplerModel &M, const GibbsModel &GM, const int8_t *states, int64_t n, double *out) {
    const int V = M.V, SD = M.sum_dom;
    const GibbsView G = HostGibbsView(M, GM);
    ParallelRanges(n, 64, [&](int64_t a, int64_t b) {
        std::vector<uint8_t> x((size_t)V * 64);
        std::vector<double> g((size_t)GM.dmax * 64);
        for (int64_t i = a; i < b; ++i) {
            for (int v = 0; v < V; ++v) x[(size_t)v * 64] = (uint8_t)states[i * V + v];
            for (int t = 0; t < V; ++t) {
                const SampleNode &nd = M.nodes[(size_t)t];
                const double tot = GibbsConditional(G, t, x.data(), nullptr, g.data());
                for (int k = 0; k < nd.d; ++k) out[i * SD + nd.moff + k] = GibbsTerm(g.data(), k, tot, x[(size_t)nd.v * 64]);
            }
        }
    });
    return FBN_OK;
}

}  // namespace fbn
