// order_mcmc_host.cpp -- order MCMC, host side: the checks, the sparse family lists (exact_host.cpp's enumerator,
// scored through an HcScorer), the result's assembly and the host twin of the kernels in plain loops over
// order_mcmc.h (include/fastbn.h states the definitions).  No HIP: like exact_bma_host.cpp it compiles on its own
// for host-side sanitizer runs.
//
// The reference has no score-based learner, so nothing here restates reference code; the method is Friedman &
// Koller's MCMC over node orders (Machine Learning 2003).
#include <algorithm>
#include <memory>
#include <new>

#include "exact_bma.h"
#include "fbn_internal.h"
#include "hc_score.h"
#include "order_mcmc.h"

namespace fbn {

namespace {

// term_v of node v's list under pred: the maximum, the ranked slots, the butterfly, the logarithm
double HostTerm(const OmcmcEntry *e, int64_t len, uint64_t pred) {
    double m = e[0].score;  // the empty set is consistent with every order
    for (int64_t f = 1; f < len; ++f)
        if (!(e[f].mask & ~pred) && e[f].score > m) m = e[f].score;
    double slot[64] = {};
    int64_t rank = 0;
    for (int64_t f = 0; f < len; ++f)
        if (!(e[f].mask & ~pred)) {
            slot[rank & 63] = slot[rank & 63] + fbn_lse_exp(e[f].score - m);
            ++rank;
        }
    return m + fbn_bd_ln(Butterfly(slot));
}

// row[u] = P(u -> v | order): the consistent entries in list order
void HostArcRow(const OmcmcEntry *e, int64_t len, uint64_t pred, double term, double *row) {
    std::fill(row, row + 64, 0.0);
    for (int64_t f = 0; f < len; ++f) {
        if (e[f].mask & ~pred) continue;
        const double w = fbn_lse_exp(e[f].score - term);
        for (uint64_t b = e[f].mask; b; b &= b - 1) row[__builtin_ctzll(b)] += w;
    }
}

double SumTerms(const double *term, int n) {
    double L = 0.0;
    for (int v = 0; v < n; ++v) L = L + term[v];
    return L;
}

struct Chain {
    uint8_t order[64];
    uint64_t pred[64];
    double term[64];
};

void ChainTerms(int n, const OmcmcLists &L, Chain &c) {
    uint64_t before = 0;
    for (int p = 0; p < n; ++p) {
        const int v = c.order[p];
        c.pred[v] = before;
        c.term[v] = HostTerm(L.ent.data() + L.off[(size_t)v], L.off[(size_t)v + 1] - L.off[(size_t)v], before);
        before |= (uint64_t)1 << v;
    }
}

}  // namespace

int OmcmcCheck(int nvars, const int32_t *dims, const fbn_exact_options &opt, int prior) {
    if (prior != 0 && prior != 1) return SetError(FBN_ERR_ARG, "prior = %d: 0 (uniform) or 1 (indegree-uniform)", prior);
    if (nvars > kOmcmcMaxVars)
        return SetError(FBN_ERR_LIMIT, "%d variables: a parent set is one 64-bit mask (at most %d variables)", nvars, kOmcmcMaxVars);
    HcFamilies none;
    if (int rc = HcCheckFamilies(nvars, dims, opt.penalty, 0, nullptr, nullptr, &none)) return rc;  // dims, penalty
    if (opt.allowed && opt.allowed_len != (int64_t)nvars * nvars)
        return SetError(FBN_ERR_ARG, "allowed mask holds %lld entries, %lld (nvars x nvars) needed", (long long)opt.allowed_len,
                        (long long)nvars * nvars);
    return FBN_OK;
}

int OmcmcCheckRun(const fbn_omcmc_options &m) {
    if (m.chains < 1 || m.samples < 1 || m.thin < 1 || m.burn_in < 0 || m.chain_offset < 0 || m.max_families < 0)
        return SetError(FBN_ERR_ARG, "order MCMC: chains = %d, samples = %d, thin = %lld (each >= 1), burn_in = %lld, chain_offset = %lld, "
                        "max_families = %lld (each >= 0)", m.chains, m.samples, (long long)m.thin, (long long)m.burn_in,
                        (long long)m.chain_offset, (long long)m.max_families);
    if (m.chain_offset > kOmcmcMaxChains - m.chains)
        return SetError(FBN_ERR_LIMIT, "order MCMC: chain_offset + chains = %lld exceeds %lld", (long long)(m.chain_offset + m.chains),
                        (long long)kOmcmcMaxChains);
    if (m.burn_in >= kOmcmcMaxSteps || m.thin > (kOmcmcMaxSteps - 1 - m.burn_in) / m.samples)
        return SetError(FBN_ERR_LIMIT, "order MCMC: burn_in + thin * samples must stay below %lld steps", (long long)kOmcmcMaxSteps);
    return FBN_OK;
}

int OmcmcCheckOrders(int n, const int32_t *orders, int64_t k) {
    if (!orders || k < 1) return SetError(FBN_ERR_ARG, "order terms: at least one order");
    for (int64_t i = 0; i < k; ++i) {
        uint64_t seen = 0;
        for (int p = 0; p < n; ++p) {
            const int32_t v = orders[i * n + p];
            if (v < 0 || v >= n || (seen >> v & 1)) return SetError(FBN_ERR_ARG, "order %lld is not a permutation of 0 .. %d", (long long)i, n - 1);
            seen |= (uint64_t)1 << v;
        }
    }
    return FBN_OK;
}

int OmcmcBuildLists(int n, const int32_t *dims, const fbn_exact_options &opt, int prior, const HcScorer &scorer, int64_t cap,
                    OmcmcLists *out, fbn_exact_info *xi) {
    if (cap <= 0 || cap > kOmcmcMaxFamilies) cap = kOmcmcMaxFamilies;
    // the subsets of up to max_parents of the n - 1 others, before the cell cap and the allowed mask thin them: where
    // even that many can be walked in seconds they are counted exactly, else this number is the one reported
    double subsets = 0.0, ck = 1.0;
    for (int k = 0; k <= (opt.max_parents < 0 ? n - 1 : std::min<int>(opt.max_parents, n - 1)); ++k) {
        subsets += ck;
        ck = ck * (double)(n - 1 - k) / (double)(k + 1);
    }
    subsets *= (double)n;
    if (subsets > 0x1p33)
        return SetError(FBN_ERR_LIMIT, "order MCMC: up to %.0f candidate families, at most %lld allowed (lower max_parents)", subsets,
                        (long long)cap);
    int64_t total = 0;
    for (int v = 0; v < n; ++v)
        if (int rc = ExactEnumerate(n, dims, opt, nullptr, v, xi, nullptr, nullptr, &total)) return rc;
    if (total > cap)
        return SetError(FBN_ERR_LIMIT, "order MCMC: the family lists hold %lld entries, at most %lld allowed "
                        "(lower max_parents or max_family_cells)", (long long)total, (long long)cap);
    // C(n - 1, k) is exact for every size the cap lets through at n > 54; the term is computed once, here
    const std::vector<double> lp = BmaSizePrior(n, prior);
    out->off.assign(1, 0);
    out->ent.clear();
    out->ent.reserve((size_t)total);
    for (int v = 0; v < n; ++v) {
        if (int rc = ExactEnumerate(n, dims, opt, &scorer, v, xi, lp.empty() ? nullptr : lp.data(),
                                    [&](uint64_t S, double score) { out->ent.push_back(OmcmcEntry{S, score}); }, nullptr))
            return rc;
        out->off.push_back((int64_t)out->ent.size());
    }
    return FBN_OK;
}

void OmcmcStartResult(int n, int prior, const fbn_omcmc_options &m, const OmcmcLists &L, const fbn_exact_info &xi,
                      fbn_omcmc_result *res) {
    fbn_omcmc_info &i = res->info;
    i.nvars = n, i.prior = prior, i.chains = m.chains, i.samples = m.samples;
    i.burn_in = m.burn_in, i.thin = m.thin, i.steps = m.burn_in + m.thin * m.samples;
    i.families = (int64_t)L.ent.size(), i.family_bytes = i.families * (int64_t)sizeof(OmcmcEntry);
    i.families_scored = xi.families_scored, i.batches = xi.batches;
    i.score_kernel_ms = xi.score_kernel_ms, i.score_wall_ms = xi.score_wall_ms;
    res->log_score.assign((size_t)m.chains * m.samples, 0.0);
    res->accepted.assign((size_t)m.chains, 0);
}

void OmcmcFinish(int n, const fbn_omcmc_options &m, const double *acc, const uint8_t *orders, fbn_omcmc_result *res) {
    const size_t nn = (size_t)n * n;
    res->chain_arc_prob.assign((size_t)m.chains * nn, 0.0);
    res->arc_prob.assign(nn, 0.0);
    res->orders.assign((size_t)m.chains * n, 0);
    for (int c = 0; c < m.chains; ++c) {
        double *P = res->chain_arc_prob.data() + (size_t)c * nn;
        for (int u = 0; u < n; ++u)
            for (int v = 0; v < n; ++v) {
                P[(size_t)u * n + v] = acc[((size_t)c * n + v) * 64 + u] / (double)m.samples;
                res->arc_prob[(size_t)u * n + v] += P[(size_t)u * n + v];
            }
        for (int p = 0; p < n; ++p) res->orders[(size_t)c * n + p] = orders[(size_t)c * 64 + p];
    }
    for (double &x : res->arc_prob) x = x / (double)m.chains;
}

void OmcmcHostChains(int n, const OmcmcLists &L, const fbn_omcmc_options &m, double *acc, uint8_t *orders, double *trace,
                     int64_t *accepted) {
    PcgStream R;
    PcgStreamInit(m.seed, R);
    const int64_t steps = m.burn_in + m.thin * m.samples;
    ParallelRanges(m.chains, 1, [&](int64_t c0, int64_t c1) {
        for (int64_t c = c0; c < c1; ++c) {
            const uint64_t g = (uint64_t)(m.chain_offset + c);
            Chain ch;
            std::fill(ch.order, ch.order + 64, (uint8_t)0);
            OmcmcStartOrder(PcgJumpTo(R.state, OmcmcStartPos(g), R.jump), R.inc, n, ch.order);
            ChainTerms(n, L, ch);
            double Lc = SumTerms(ch.term, n);
            double *A = acc + (size_t)c * n * 64, row[64];
            std::fill(A, A + (size_t)n * 64, 0.0);
            int64_t acc_n = 0, taken = 0;
            U128 s = PcgJumpTo(R.state, OmcmcStepPos(g, 0), R.jump);
            for (int64_t t = 0; t < steps; ++t) {
                s = PcgStep(s, R.inc);
                const uint64_t r1 = PcgOutput(s);
                s = PcgStep(s, R.inc);
                const uint64_t r2 = PcgOutput(s);
                s = PcgStep(s, R.inc);
                const double u = PcgDouble(PcgOutput(s));
                if (n >= 2) {
                    int i, j;
                    OmcmcProposal(r1, r2, n, &i, &j);
                    const int a = ch.order[i], b = ch.order[j];
                    const uint64_t flip = ((uint64_t)1 << a) | ((uint64_t)1 << b);
                    uint64_t npred[64], changed = 0;
                    double nterm[64];
                    for (int p = i; p <= j; ++p) {
                        const int v = p == i ? b : p == j ? a : ch.order[p];
                        npred[v] = ch.pred[ch.order[p]] ^ (p > i ? flip : 0);
                        nterm[v] = HostTerm(L.ent.data() + L.off[(size_t)v], L.off[(size_t)v + 1] - L.off[(size_t)v], npred[v]);
                        changed |= (uint64_t)1 << v;
                    }
                    double Ln = 0.0;
                    for (int v = 0; v < n; ++v) Ln = Ln + (changed >> v & 1 ? nterm[v] : ch.term[v]);
                    if (OmcmcAccept(Ln - Lc, u)) {
                        for (int v = 0; v < n; ++v)
                            if (changed >> v & 1) ch.term[v] = nterm[v], ch.pred[v] = npred[v];
                        ch.order[i] = (uint8_t)b, ch.order[j] = (uint8_t)a;
                        Lc = Ln;
                        ++acc_n;
                    }
                }
                if (t + 1 > m.burn_in && (t + 1 - m.burn_in) % m.thin == 0) {
                    for (int v = 0; v < n; ++v) {
                        HostArcRow(L.ent.data() + L.off[(size_t)v], L.off[(size_t)v + 1] - L.off[(size_t)v], ch.pred[v], ch.term[v], row);
                        for (int x = 0; x < 64; ++x) A[(size_t)v * 64 + x] += row[x];
                    }
                    trace[(size_t)c * m.samples + taken++] = Lc;
                }
            }
            std::copy(ch.order, ch.order + 64, orders + (size_t)c * 64);
            accepted[c] = acc_n;
        }
    });
}

void OmcmcHostTerms(int n, const OmcmcLists &L, const int32_t *orders, int64_t k, double *term, double *arcs) {
    for (int64_t i = 0; i < k; ++i) {
        Chain ch;
        for (int p = 0; p < n; ++p) ch.order[p] = (uint8_t)orders[i * n + p];
        ChainTerms(n, L, ch);
        double row[64];
        for (int v = 0; v < n; ++v) {
            term[i * n + v] = ch.term[v];
            HostArcRow(L.ent.data() + L.off[(size_t)v], L.off[(size_t)v + 1] - L.off[(size_t)v], ch.pred[v], ch.term[v], row);
            for (int u = 0; u < n; ++u) arcs[((size_t)i * n + u) * n + v] = row[u];
        }
    }
}

// the twin's run over a host column store
static int OmcmcRunHost(int n, const int32_t *dims, const fbn_exact_options &opt, int prior, const fbn_omcmc_options &m,
                        const HcScorer &scorer, fbn_omcmc_result *res) {
    const auto t_start = Clock::now();
    OmcmcLists L;
    fbn_exact_info xi{};
    if (int rc = OmcmcBuildLists(n, dims, opt, prior, scorer, m.max_families, &L, &xi)) return rc;
    OmcmcStartResult(n, prior, m, L, xi, res);
    std::vector<double> acc((size_t)m.chains * n * 64);
    std::vector<uint8_t> orders((size_t)m.chains * 64);
    const auto t0 = Clock::now();
    OmcmcHostChains(n, L, m, acc.data(), orders.data(), res->log_score.data(), res->accepted.data());
    res->info.chain_wall_ms = MsSince(t0);
    OmcmcFinish(n, m, acc.data(), orders.data(), res);
    res->info.wall_ms = MsSince(t_start);
    return FBN_OK;
}

}  // namespace fbn

using fbn::SetError;

extern "C" {

// fbn_omcmc_run_host (bd == nullptr) and fbn_omcmc_run_bd_host
static int OmcmcRunHostEntry(int nvars, const int32_t *dims, const uint8_t *cols, int64_t nsamples, const fbn_exact_options *options,
                             int32_t prior, const fbn_bd_score *bd, const fbn_omcmc_options *mcmc, fbn_omcmc_result **out) {
    if (!options || !mcmc || !out) return SetError(FBN_ERR_ARG, "null pointer");
    if (int rc = fbn::OmcmcCheck(nvars, dims, *options, prior)) return rc;
    if (int rc = fbn::OmcmcCheckRun(*mcmc)) return rc;
    auto r = std::unique_ptr<fbn_omcmc_result>(new (std::nothrow) fbn_omcmc_result());
    if (!r) return SetError(FBN_ERR_NOMEM, "out of memory");
    if (int rc = fbn::WithHostScorer(nvars, dims, cols, nsamples, bd, [&](const fbn::HcScorer &scorer) {
            return fbn::OmcmcRunHost(nvars, dims, *options, prior, *mcmc, scorer, r.get());
        }))
        return rc;
    *out = r.release();
    return FBN_OK;
}

int fbn_omcmc_run_host(int nvars, const int32_t *dims, const uint8_t *cols, int64_t nsamples, const fbn_exact_options *options,
                       int32_t prior, const fbn_omcmc_options *mcmc, fbn_omcmc_result **out) {
    return OmcmcRunHostEntry(nvars, dims, cols, nsamples, options, prior, nullptr, mcmc, out);
}

int fbn_omcmc_run_bd_host(int nvars, const int32_t *dims, const uint8_t *cols, int64_t nsamples, const fbn_exact_options *options,
                          int32_t prior, const fbn_bd_score *bd, const fbn_omcmc_options *mcmc, fbn_omcmc_result **out) {
    if (int rc = fbn::BdCheck(bd)) return rc;
    return OmcmcRunHostEntry(nvars, dims, cols, nsamples, options, prior, bd, mcmc, out);
}

int fbn_omcmc_order_terms_host(int nvars, const int32_t *dims, const uint8_t *cols, int64_t nsamples, const fbn_exact_options *options,
                               int32_t prior, const fbn_bd_score *bd, int64_t max_families, const int32_t *orders, int64_t k,
                               double *term, double *arcs) {
    if (!options || !term || !arcs) return SetError(FBN_ERR_ARG, "null pointer");
    if (bd)
        if (int rc = fbn::BdCheck(bd)) return rc;
    if (int rc = fbn::OmcmcCheck(nvars, dims, *options, prior)) return rc;
    if (int rc = fbn::OmcmcCheckOrders(nvars, orders, k)) return rc;
    if (max_families < 0) return SetError(FBN_ERR_ARG, "max_families = %lld is negative", (long long)max_families);
    return fbn::WithHostScorer(nvars, dims, cols, nsamples, bd, [&](const fbn::HcScorer &scorer) {
        fbn::OmcmcLists L;
        fbn_exact_info xi{};
        if (int rc = fbn::OmcmcBuildLists(nvars, dims, *options, prior, scorer, max_families, &L, &xi)) return rc;
        fbn::OmcmcHostTerms(nvars, L, orders, k, term, arcs);
        return (int)FBN_OK;
    });
}

int fbn_omcmc_result_info(const fbn_omcmc_result *r, fbn_omcmc_info *info) {
    if (!r || !info) return SetError(FBN_ERR_ARG, "null pointer");
    *info = r->info;
    return FBN_OK;
}

int fbn_omcmc_result_arcs(const fbn_omcmc_result *r, double *arc_prob, double *chain_arc_prob, int32_t *orders, double *log_score,
                          int64_t *accepted) {
    if (!r) return SetError(FBN_ERR_ARG, "null pointer");
    if (arc_prob) std::copy(r->arc_prob.begin(), r->arc_prob.end(), arc_prob);
    if (chain_arc_prob) std::copy(r->chain_arc_prob.begin(), r->chain_arc_prob.end(), chain_arc_prob);
    if (orders) std::copy(r->orders.begin(), r->orders.end(), orders);
    if (log_score) std::copy(r->log_score.begin(), r->log_score.end(), log_score);
    if (accepted) std::copy(r->accepted.begin(), r->accepted.end(), accepted);
    return FBN_OK;
}

int fbn_omcmc_result_destroy(fbn_omcmc_result *r) {
    delete r;
    return FBN_OK;
}

}  // extern "C"
