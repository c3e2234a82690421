// ais_host.cpp -- host twin of the adaptive samplers AIS-BN and SIS (device < 0 handles): ais.hip's
// kernel operation for operation on CPU threads -- the same stages and 64-sample chunks, the same
// stream positions, butterfly and per-entry summation orders, the same ascending-sample count order
// and power-of-two rescaling -- so the two agree bit for bit (ais_model.h holds what both compile).
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "ais_model.h"
#include "fbn_internal.h"

namespace fbn {

void AisEta(int method, int m, double *eta) {
    const double a = 0.4, b = 0.14;
    for (int k = 0; k < m; ++k) eta[k] = method == 0 ? a * pow(b / a, (double)k / (double)m) : 1.0;
}

int CheckAisArgs(const SamplerModel &M, int method, int64_t ncases, int64_t S, int64_t m, int64_t l,
                 int64_t case_offset, double eps) {
    if (method != 0 && method != 1) return SetError(FBN_ERR_ARG, "method %d (0 AIS-BN, 1 SIS)", method);
    if (S < 1) return SetError(FBN_ERR_ARG, "samples per case must be >= 1 (got %lld)", (long long)S);
    if (m < 0 || m > FBN_AIS_MAX_UPDATES)
        return SetError(FBN_ERR_ARG, "maximum updates must be in [0, %d] (got %lld)", FBN_AIS_MAX_UPDATES, (long long)m);
    if (l < 1) return SetError(FBN_ERR_ARG, "updating interval must be >= 1 (got %lld)", (long long)l);
    if (!(eps < 1.0)) return SetError(FBN_ERR_ARG, "eps must be below 1 (negative: the defaults; got %g)", eps);
    if (method == 1 && eps == 0.0)
        return SetError(FBN_ERR_ARG, "SIS needs a cutoff: eps 0 leaves states the counts missed without support");
    if (ncases < 0 || case_offset < 0) return SetError(FBN_ERR_ARG, "bad argument");
    const long double T = method == 0 ? (long double)m * (long double)l + (long double)S : (long double)S;
    const long double pos = ((long double)case_offset + (long double)ncases) * T + 64.0L;
    if (pos * (long double)M.V >= 9.2e18L) return SetError(FBN_ERR_ARG, "stream position beyond 2^63");
    return FBN_OK;
}

int HostAis(const SamplerModel &M, int method, const int8_t *ev, int64_t ncases, int64_t S, int64_t m, int64_t l,
            uint64_t seed, int64_t case_offset, double eps, int32_t *labels, double *marg, double *stats,
            uint8_t *dbg_vals, double *dbg_m, int32_t *dbg_e, double *dbg_icpt) {
    if (ncases == 0) return FBN_OK;
    const int V = M.V, SD = M.sum_dom;
    const int64_t cells = M.cells;
    const AisSchedule sch = AisStages(method, S, m, l);
    const size_t total = (size_t)ncases * (size_t)sch.T;
    std::vector<double> eta((size_t)std::max<int64_t>(m, 1));
    AisEta(method, (int)m, eta.data());  // nupd <= m: SIS reads a prefix of ones
    PcgStream R;
    PcgStreamInit(seed, R);
    ParallelRanges(ncases, 1, [&](int64_t c0, int64_t c1) {
        std::vector<uint8_t> x((size_t)V * 64), lrn((size_t)V);
        std::vector<double> own((size_t)SD), I((size_t)cells), N((size_t)cells);
        for (int64_t c = c0; c < c1; ++c) {
            const int8_t *e_row = ev + c * V;
            double *row = marg ? marg + c * SD : own.data();
            // the learnable set: unobserved with an observed descendant (one reverse-topological pass)
            std::fill(lrn.begin(), lrn.end(), 0);
            for (int k = V - 1; k >= 0; --k) {
                const SampleNode &nd = M.nodes[k];
                if (e_row[nd.v] >= 0 || lrn[nd.v])
                    for (int j = 0; j < nd.npar; ++j) lrn[M.par[2 * (nd.poff + j)]] = 1;
            }
            for (int v = 0; v < V; ++v) lrn[v] = lrn[v] && e_row[v] < 0;
            std::copy(M.prob.begin(), M.prob.end(), I.begin());
            WeightState ws;
            int upd = 0;
            double ess0 = 0.0;
            bool first = true;  // the next chunk opens the scope of emax, the sums and the counts
            int64_t tbase = 0;
            for (int64_t st = 0; st <= sch.nupd; ++st) {
                const int64_t n = st < sch.nupd ? sch.l : sch.last;
                const bool counted = method == 1 || st == sch.nupd, learn = st < sch.nupd;
                if (method == 0 || st == 0) {
                    first = true, ws.sumw = 0.0, ws.sumw2 = 0.0;
                    if (learn) std::fill(N.begin(), N.end(), 0.0);
                }
                for (int64_t s0 = 0; s0 < n; s0 += 64) {
                    const int act = (int)std::min<int64_t>(64, n - s0);
                    double mm[64], w[64];
                    int e[64];
                    for (int ln = 0; ln < act; ++ln) {
                        const uint64_t i = (uint64_t)(case_offset + c) * (uint64_t)sch.T + (uint64_t)(tbase + s0 + ln);
                        const size_t di = (size_t)c * sch.T + (size_t)(tbase + s0 + ln);
                        U128 s = PcgJumpTo(R.state, i * (uint64_t)V, R.jump);
                        double mant = 1.0;
                        int ee = 0;
                        for (const SampleNode &nd : M.nodes) {
                            const int pc = ParentConfig(M, nd, x.data() + ln, 64);
                            const int evv = e_row[nd.v];
                            const size_t r = (size_t)nd.toff + (size_t)pc * nd.d;
                            s = PcgStep(s, R.inc);
                            int q, de;
                            if (evv >= 0) {  // clamp, weigh: as likelihood weighting
                                q = evv;
                                mant = frexp(mant * M.prob[r + q], &de);
                                ee += de;
                            } else if (lrn[nd.v]) {
                                double fac;
                                q = AisDraw(M.prob.data() + r, I.data() + r, nd.d, EpisCutoff(eps, nd.d),
                                            PcgDouble(PcgOutput(s)), &fac);
                                mant = frexp(mant * fac, &de);
                                ee += de;
                            } else {
                                q = SelectValue(M.cdf.data() + r, nd.d, PcgDouble(PcgOutput(s)));
                            }
                            x[(size_t)nd.v * 64 + ln] = (uint8_t)q;
                            if (dbg_vals) dbg_vals[(size_t)nd.v * total + di] = (uint8_t)q;
                        }
                        mm[ln] = mant, e[ln] = ee;
                        if (dbg_m) dbg_m[di] = mant, dbg_e[di] = ee;
                    }
                    const double f = HostChunkWeights(ws, mm, e, act, first, w);
                    if (counted) HostAccumulateChunk(M, x.data(), w, act, f, first, row);
                    if (learn) {
                        if (f != 1.0)
                            for (int64_t j = 0; j < cells; ++j) N[(size_t)j] = N[(size_t)j] * f;
                        for (const SampleNode &nd : M.nodes) {
                            if (!lrn[nd.v]) continue;
                            for (int ln = 0; ln < act; ++ln) {
                                const int pc = ParentConfig(M, nd, x.data() + ln, 64);
                                N[(size_t)nd.toff + (size_t)pc * nd.d + x[(size_t)nd.v * 64 + ln]] += w[ln];
                            }
                        }
                    }
                    first = false;
                }
                if (st == 0) ess0 = WeightEss(ws) / (double)n;
                if (learn) {
                    if (ws.sumw > 0.0) ++upd;
                    for (int k = 0; k < V; ++k) {
                        const SampleNode &nd = M.nodes[k];
                        if (!lrn[nd.v]) continue;
                        const int64_t end = k + 1 < V ? M.nodes[k + 1].toff : cells;
                        for (int64_t r = nd.toff; r < end; r += nd.d)
                            AisUpdateRow(I.data() + r, N.data() + r, nd.d, eta[(size_t)st]);
                    }
                }
                tbase += n;
            }
            double *st = stats ? stats + 4 * c : nullptr;
            HostFinishCase(M, e_row, row, ws, S, labels + c, st);
            if (st) st[2] = (double)upd, st[3] = ess0;
            if (dbg_icpt) std::copy(I.begin(), I.end(), dbg_icpt + c * cells);
        }
    });
    return FBN_OK;
}

}  // namespace fbn
