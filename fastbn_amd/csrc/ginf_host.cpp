// ginf_host.cpp -- the host side of the linear-Gaussian networks (ginf.h; include/fastbn.h states the model):
// validation of a network, its joint N(mu, Sigma) in Kahn's order, maximum-likelihood parameters of a known
// structure from the moments a Gaussian CI context holds, the evidence check, and the host twin of ginf.hip --
// plain loops over ginf_model.h, the header the kernel evaluates too, so both give the same bits.  Also the
// fbn_gnet_* entries, which need no device.
#include <algorithm>
#include <cmath>
#include <functional>
#include <memory>
#include <new>
#include <queue>

#include "gci_elim.h"
#include "ginf.h"
#include "ginf_model.h"

namespace fbn {

int GnetBuild(int nvars, const int32_t *parent_off, const int32_t *parents, const double *intercept, const double *coef,
              const double *variance, fbn_gnet *net) {
    if (nvars <= 0 || !parent_off || !intercept || !variance || !net) return SetError(FBN_ERR_ARG, "bad argument");
    const int n = nvars;
    if (parent_off[0] != 0) return SetError(FBN_ERR_ARG, "parent_off[0] = %d, not 0", parent_off[0]);
    for (int v = 0; v < n; ++v)
        if (parent_off[v + 1] < parent_off[v]) return SetError(FBN_ERR_ARG, "node %d: parent_off decreases", v);
    const int32_t np = parent_off[n];
    if (np > 0 && (!parents || !coef)) return SetError(FBN_ERR_ARG, "null parent or coefficient list");
    std::vector<int> indeg((size_t)n, 0);
    std::vector<std::vector<int>> children((size_t)n);
    for (int v = 0; v < n; ++v) {
        if (!std::isfinite(intercept[v])) return SetError(FBN_ERR_ARG, "node %d: intercept is not finite", v);
        if (!(variance[v] > 0.0) || !std::isfinite(variance[v]))
            return SetError(FBN_ERR_ARG, "node %d: variance %g is not positive and finite", v, variance[v]);
        for (int32_t k = parent_off[v]; k < parent_off[v + 1]; ++k) {
            const int p = parents[k];
            if (p < 0 || p >= n || p == v) return SetError(FBN_ERR_ARG, "node %d: parent %d out of 0..%d or the node itself", v, p, n - 1);
            for (int32_t q = parent_off[v]; q < k; ++q)
                if (parents[q] == p) return SetError(FBN_ERR_ARG, "node %d: parent %d listed twice", v, p);
            if (!std::isfinite(coef[k])) return SetError(FBN_ERR_ARG, "node %d: coefficient of parent %d is not finite", v, p);
            children[(size_t)p].push_back(v);
            ++indeg[(size_t)v];
        }
    }
    std::priority_queue<int, std::vector<int>, std::greater<int>> ready;
    for (int v = 0; v < n; ++v)
        if (indeg[(size_t)v] == 0) ready.push(v);
    net->order.clear();
    while (!ready.empty()) {
        const int v = ready.top();
        ready.pop();
        net->order.push_back(v);
        for (int c : children[(size_t)v])
            if (--indeg[(size_t)c] == 0) ready.push(c);
    }
    if ((int)net->order.size() != n) {
        int v = 0;
        while (indeg[(size_t)v] == 0) ++v;
        return SetError(FBN_ERR_ARG, "the parent lists hold a cycle (through node %d)", v);
    }
    net->n = n;
    net->off.assign(parent_off, parent_off + n + 1);
    net->par.assign(parents, parents + np);
    net->coef.assign(coef, coef + np);
    net->intercept.assign(intercept, intercept + n);
    net->variance.assign(variance, variance + n);
    return FBN_OK;
}

void GnetJoint(const fbn_gnet &net, double *mu, double *Sigma) {
    FBN_GCI_NO_CONTRACT
    const int n = net.n;
    std::vector<std::pair<int, double>> pa;  // the node's parents in ascending index order
    for (int pos = 0; pos < n; ++pos) {
        const int v = net.order[(size_t)pos];
        pa.clear();
        for (int32_t k = net.off[(size_t)v]; k < net.off[(size_t)v + 1]; ++k) pa.emplace_back(net.par[(size_t)k], net.coef[(size_t)k]);
        std::sort(pa.begin(), pa.end());
        double m = net.intercept[(size_t)v];
        for (const auto &pw : pa) m = m + pw.second * mu[pw.first];
        mu[v] = m;
        double *row = Sigma + (size_t)v * n;
        for (int q = 0; q < pos; ++q) {
            const int u = net.order[(size_t)q];
            double s = 0.0;
            for (const auto &pw : pa) s = s + pw.second * Sigma[(size_t)pw.first * n + u];
            row[u] = s;
            Sigma[(size_t)u * n + v] = s;
        }
        double s = net.variance[(size_t)v];
        for (const auto &pw : pa) s = s + pw.second * row[pw.first];
        row[v] = s;
    }
}

int GnetLearn(int nvars, int64_t N, const double *mean, const double *ss, const double *R, const int32_t *parent_off,
              const int32_t *parents, fbn_gnet *net) {
    FBN_GCI_NO_CONTRACT
    if (nvars <= 0 || N <= 0 || !mean || !ss || !R || !parent_off || !net) return SetError(FBN_ERR_ARG, "bad argument");
    const int n = nvars;
    for (int v = 0; v < n; ++v)
        if (!(ss[v] > 0.0) || !std::isfinite(ss[v]) || !std::isfinite(mean[v]))
            return SetError(FBN_ERR_ARG, "variable %d: its moments are not those of a column with a variance", v);
    if (parent_off[0] != 0) return SetError(FBN_ERR_ARG, "parent_off[0] = %d, not 0", parent_off[0]);
    for (int v = 0; v < n; ++v) {
        if (parent_off[v + 1] < parent_off[v]) return SetError(FBN_ERR_ARG, "node %d: parent_off decreases", v);
        for (int32_t k = parent_off[v]; k < parent_off[v + 1]; ++k)
            if (!parents || parents[k] < 0 || parents[k] >= n || parents[k] == v)
                return SetError(FBN_ERR_ARG, "node %d: bad parent", v);
    }
    std::vector<double> b((size_t)n), s((size_t)n), coef((size_t)parent_off[n]), W, beta;
    std::vector<int> idx;  // ascending parents, then the node
    for (int v = 0; v < n; ++v) {
        const int32_t k0 = parent_off[v], np = parent_off[v + 1] - k0;
        idx.assign(parents + k0, parents + k0 + np);
        std::sort(idx.begin(), idx.end());
        idx.push_back(v);
        const int M = np + 1;
        // gci_elim.h's elimination on the upper triangle of R over (parents.., v), a full M x M store
        W.assign((size_t)M * M, 0.0);
        for (int i = 0; i < M; ++i)
            for (int j = i; j < M; ++j) W[(size_t)i * M + j] = R[(size_t)idx[(size_t)i] * n + idx[(size_t)j]];
        for (int k = 0; k < np; ++k) {
            const double piv = W[(size_t)k * M + k];
            if (!(piv > kGciPivotMin))
                return SetError(FBN_ERR_ARG, "node %d: its parents are collinear (pivot %g at parent %d)", v, piv, idx[(size_t)k]);
            for (int i = k + 1; i < M; ++i) {
                const double l = W[(size_t)k * M + i] / piv;
                for (int j = i; j < M; ++j) W[(size_t)i * M + j] = W[(size_t)i * M + j] - l * W[(size_t)k * M + j];
            }
        }
        const double schur = W[(size_t)np * M + np];
        if (!(schur > kGciPivotMin))
            return SetError(FBN_ERR_ARG, "node %d is a linear function of its parents (Schur complement %g)", v, schur);
        // back substitution on the eliminated rows: U beta = c, c the last column
        beta.assign((size_t)np, 0.0);
        for (int i = np - 1; i >= 0; --i) {
            double acc = W[(size_t)i * M + np];
            for (int j = i + 1; j < np; ++j) acc = acc - W[(size_t)i * M + j] * beta[(size_t)j];
            beta[(size_t)i] = acc / W[(size_t)i * M + i];
        }
        const double var_v = ss[v] / (double)N, sd_v = std::sqrt(var_v);
        double icpt = mean[v];
        for (int32_t k = 0; k < np; ++k) {
            const int p = parents[k0 + k];
            const int at = (int)(std::lower_bound(idx.begin(), idx.begin() + np, p) - idx.begin());
            const double w = beta[(size_t)at] * sd_v / std::sqrt(ss[p] / (double)N);
            coef[(size_t)(k0 + k)] = w;
        }
        for (int i = 0; i < np; ++i) {  // ascending parents
            const int p = idx[(size_t)i];
            icpt = icpt - (beta[(size_t)i] * sd_v / std::sqrt(ss[p] / (double)N)) * mean[p];
        }
        b[(size_t)v] = icpt;
        s[(size_t)v] = var_v * schur;
    }
    return GnetBuild(n, parent_off, parents, b.data(), coef.data(), s.data(), net);
}

int GinfCheckEvidence(const double *ev, int64_t ncases, int n, int *m_max) {
    int mm = 0;
    for (int64_t c = 0; c < ncases; ++c) {
        const double *x = ev + c * n;
        int m = 0;
        for (int v = 0; v < n; ++v) {
            if (x[v] != x[v]) continue;
            if (std::isinf(x[v])) return SetError(FBN_ERR_ARG, "case %lld: evidence for variable %d is infinite", (long long)c, v);
            ++m;
        }
        if (m > kGinfMaxObs)
            return SetError(FBN_ERR_LIMIT, "case %lld observes %d variables (supported up to %d)", (long long)c, m, kGinfMaxObs);
        mm = std::max(mm, m);
    }
    *m_max = mm;
    return FBN_OK;
}

void GinfHostRun(const double *mu, const double *Sigma, int n, const double *ev, int64_t ncases, double *mean, double *var,
                 double *logp, int64_t *degenerate) {
    std::vector<int> E, U;
    std::vector<double> L, a, d, y;
    const double nan = __builtin_nan("");
    int64_t ndeg = 0;
    for (int64_t c = 0; c < ncases; ++c) {
        const double *x = ev + c * n;
        E.clear(), U.clear();
        for (int v = 0; v < n; ++v) (x[v] != x[v] ? U : E).push_back(v);
        const int m = (int)E.size();
        L.assign((size_t)fbn_ginf_tri(m, 0), 0.0), a.assign((size_t)m, 0.0), d.assign((size_t)m, 0.0), y.assign((size_t)m, 0.0);
        bool deg = false;
        for (int i = 0; i < m; ++i) {
            const double *row = Sigma + (size_t)E[(size_t)i] * n;
            double *Li = L.data() + fbn_ginf_tri(i, 0);
            double sq = 0.0;
            for (int j = 0; j < i; ++j) {
                const double *Lj = L.data() + fbn_ginf_tri(j, 0);
                Li[j] = fbn_ginf_elim(row[E[(size_t)j]], Li, 1, Lj, 1, j, Lj[j]);
                sq = fbn_ginf_more(sq, Li[j], Li[j]);
            }
            bool dg;
            d[(size_t)i] = fbn_ginf_diag(row[E[(size_t)i]], sq, &dg);
            Li[i] = sqrt(d[(size_t)i]);
            deg = deg || dg;
        }
        double aa = 0.0;
        for (int j = 0; j < m; ++j) {
            const double *Lj = L.data() + fbn_ginf_tri(j, 0);
            a[(size_t)j] = fbn_ginf_elim(x[E[(size_t)j]] - mu[E[(size_t)j]], a.data(), 1, Lj, 1, j, Lj[j]);
            aa = fbn_ginf_more(aa, a[(size_t)j], a[(size_t)j]);
        }
        double *mc = mean ? mean + c * n : nullptr, *vc = var ? var + c * n : nullptr;
        if (deg) {
            ++ndeg;
            for (int v = 0; v < n; ++v) {
                if (mc) mc[v] = nan;
                if (vc) vc[v] = nan;
            }
            if (logp) logp[c] = nan;
            continue;
        }
        if (logp) logp[c] = fbn_ginf_logp(m, d.data(), aa);
        if (!mc && !vc) continue;
        for (int v : E) {
            if (mc) mc[v] = x[v];
            if (vc) vc[v] = 0.0;
        }
        for (int u : U) {
            double ya = 0.0, yy = 0.0;
            for (int i = 0; i < m; ++i) {
                const double *Li = L.data() + fbn_ginf_tri(i, 0);
                y[(size_t)i] = fbn_ginf_elim(Sigma[(size_t)E[(size_t)i] * n + u], Li, 1, y.data(), 1, i, Li[i]);
                ya = fbn_ginf_more(ya, y[(size_t)i], a[(size_t)i]);
                yy = fbn_ginf_more(yy, y[(size_t)i], y[(size_t)i]);
            }
            double pm, pv;
            fbn_ginf_posterior(mu[u], Sigma[(size_t)u * n + u], ya, yy, &pm, &pv);
            if (mc) mc[u] = pm;
            if (vc) vc[u] = pv;
        }
    }
    if (degenerate) *degenerate = ndeg;
}

}  // namespace fbn

using fbn::SetError;

extern "C" {

int fbn_gnet_create(int nvars, const int32_t *parent_off, const int32_t *parents, const double *intercept, const double *coef,
                    const double *variance, fbn_gnet **out) {
    if (!out) return SetError(FBN_ERR_ARG, "null pointer");
    auto net = std::unique_ptr<fbn_gnet>(new (std::nothrow) fbn_gnet());
    if (!net) return SetError(FBN_ERR_NOMEM, "out of memory");
    if (int rc = fbn::GnetBuild(nvars, parent_off, parents, intercept, coef, variance, net.get())) return rc;
    *out = net.release();
    return FBN_OK;
}

int fbn_gnet_learn_host(int nvars, int64_t nsamples, const double *mean, const double *ss, const double *R,
                        const int32_t *parent_off, const int32_t *parents, fbn_gnet **out) {
    if (!out) return SetError(FBN_ERR_ARG, "null pointer");
    auto net = std::unique_ptr<fbn_gnet>(new (std::nothrow) fbn_gnet());
    if (!net) return SetError(FBN_ERR_NOMEM, "out of memory");
    if (int rc = fbn::GnetLearn(nvars, nsamples, mean, ss, R, parent_off, parents, net.get())) return rc;
    *out = net.release();
    return FBN_OK;
}

int fbn_gnet_params(const fbn_gnet *net, double *intercept, double *coef, double *variance) {
    if (!net) return SetError(FBN_ERR_ARG, "null pointer");
    if (intercept) std::copy(net->intercept.begin(), net->intercept.end(), intercept);
    if (coef) std::copy(net->coef.begin(), net->coef.end(), coef);
    if (variance) std::copy(net->variance.begin(), net->variance.end(), variance);
    return FBN_OK;
}

int fbn_gnet_joint(const fbn_gnet *net, double *mean, double *cov) {
    if (!net || !mean || !cov) return SetError(FBN_ERR_ARG, "null pointer");
    fbn::GnetJoint(*net, mean, cov);
    return FBN_OK;
}

int fbn_gnet_destroy(fbn_gnet *net) {
    delete net;
    return FBN_OK;
}

}  // extern "C"
