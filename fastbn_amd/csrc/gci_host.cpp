// gci_host.cpp -- the host side of the Gaussian conditional-independence test (gci.h): the threshold tau_d,
// the reported z and p, and the host twin -- fbn_gci_host_run and fbn_gci_host_pc_stable evaluate gci_elim.h
// on the CPU over a correlation matrix the caller hands in, through the very driver the device run uses
// (RunPCGauss).  Given the device's R they repeat its decisions, counts and sepsets bit for bit.  Also the
// continuous dataset handle (fbn_cdataset_*).  No device.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>

#include "fbn_internal.h"
#include "gci.h"
#include "gci_elim.h"

namespace fbn {

// Phi^-1(1 - alpha / 2): the root z >= 0 of f(z) = erfc(z / sqrt 2) / 2 - alpha / 2 by Newton from z = 0.
// f is convex and decreasing on z >= 0, so the iterates rise monotonically to the root.
static double UpperQuantile(double alpha) {
    const double target = alpha / 2, rs2 = 0.70710678118654752440, rs2pi = 0.39894228040143267794;
    double z = 0.0;
    for (int it = 0; it < 200; ++it) {
        const double f = 0.5 * std::erfc(z * rs2) - target;
        const double step = f / (rs2pi * std::exp(-0.5 * z * z));
        if (!(step > 0.0) || z + step == z) break;
        z += step;
    }
    return z;
}

int GciTau(double alpha, int64_t N, int d, double *tau) {
    if (!(alpha > 0.0 && alpha < 1.0)) return SetError(FBN_ERR_ARG, "alpha = %g outside (0, 1)", alpha);
    if (d < 0 || d > kGciMaxD) return SetError(FBN_ERR_LIMIT, "conditioning set size %d (supported 0..%d)", d, kGciMaxD);
    if (N - d - 3 <= 0)
        return SetError(FBN_ERR_LIMIT, "%lld samples: the Fisher-z test of %d conditioning variables needs more than %d",
                        (long long)N, d, d + 3);
    *tau = std::tanh(UpperQuantile(alpha) / std::sqrt((double)(N - d - 3)));
    return FBN_OK;
}

void GciReport(double r, int64_t N, int d, double *z, double *p) {
    *z = std::sqrt((double)(N - d - 3)) * std::atanh(r);
    *p = std::erfc(std::fabs(*z) * 0.70710678118654752440);
}

int GciCheckItems(const int32_t *items, int64_t n, int d, int nvars) {
    for (int64_t t = 0; t < n; ++t) {
        const int32_t *v = items + t * (2 + d);
        for (int k = 0; k < 2 + d; ++k)
            if (v[k] < 0 || v[k] >= nvars) return SetError(FBN_ERR_ARG, "test %lld: variable %d out of 0..%d", (long long)t, v[k], nvars - 1);
        if (v[0] == v[1]) return SetError(FBN_ERR_ARG, "test %lld: x == y == %d", (long long)t, v[0]);
        for (int k = 2; k < 2 + d; ++k)
            if (v[k] == v[0] || v[k] == v[1])
                return SetError(FBN_ERR_ARG, "test %lld: conditioning variable %d is x or y", (long long)t, v[k]);
    }
    return FBN_OK;
}

namespace {

template <int D>
void HostBatchD(const double *R, int nvars, const int32_t *items, int64_t n, double tau, double *r, uint8_t *indep,
                GciLog &log) {
    for (int64_t t = 0; t < n; ++t) {
        int32_t pair[2];
        const int32_t *v = items ? items + t * (2 + D) : pair;
        if (!items) {
            pair[0] = PairRow(t, nvars);
            pair[1] = (int32_t)(t - PairIndex(pair[0], pair[0] + 1, nvars)) + pair[0] + 1;
        }
        const double rt = fbn_gci_partial_r<D>(R, nvars, v);
        double m;
        const bool ind = fbn_gci_decide(rt, tau, &m);
        if (r) r[t] = rt;
        if (indep) indep[t] = ind;
        if (m < 0.0) ++log.degenerate;
        else log.min_margin = std::min(log.min_margin, m), log.near += m < 1e-9;
    }
}

struct HostTester : GciTester {
    const double *R;
    int nvars;
    std::vector<uint8_t> out[2];
    GciLog log;
    HostTester(const double *R_, int n) : R(R_), nvars(n) {}
    int Launch(int k, const int32_t *items, int64_t n, int d, double tau) override {
        out[k].resize((size_t)n);
        return GciHostBatch(R, nvars, items, n, d, tau, nullptr, out[k].data(), log);
    }
    int Wait(int k, uint8_t *indep, PCResultHost &) override {
        std::copy(out[k].begin(), out[k].end(), indep);
        return FBN_OK;
    }
    int Log(GciLog *l) override {
        *l = log;
        return FBN_OK;
    }
};

int CheckR(const double *R, int nvars) {
    if (!R || nvars < 1) return SetError(FBN_ERR_ARG, "bad argument");
    for (int64_t i = 0; i < (int64_t)nvars * nvars; ++i)
        if (!std::isfinite(R[i])) return SetError(FBN_ERR_ARG, "R[%lld][%lld] is not finite", (long long)(i / nvars), (long long)(i % nvars));
    return FBN_OK;
}

}  // namespace

int GciHostBatch(const double *R, int nvars, const int32_t *items, int64_t n, int d, double tau, double *r,
                 uint8_t *indep, GciLog &log) {
    switch (d) {
    case 0: HostBatchD<0>(R, nvars, items, n, tau, r, indep, log); break;
    case 1: HostBatchD<1>(R, nvars, items, n, tau, r, indep, log); break;
    case 2: HostBatchD<2>(R, nvars, items, n, tau, r, indep, log); break;
    case 3: HostBatchD<3>(R, nvars, items, n, tau, r, indep, log); break;
    case 4: HostBatchD<4>(R, nvars, items, n, tau, r, indep, log); break;
    case 5: HostBatchD<5>(R, nvars, items, n, tau, r, indep, log); break;
    case 6: HostBatchD<6>(R, nvars, items, n, tau, r, indep, log); break;
    case 7: HostBatchD<7>(R, nvars, items, n, tau, r, indep, log); break;
    case 8: HostBatchD<8>(R, nvars, items, n, tau, r, indep, log); break;
    default: return SetError(FBN_ERR_LIMIT, "conditioning set size %d (supported 0..%d)", d, kGciMaxD);
    }
    return FBN_OK;
}

}  // namespace fbn

using fbn::SetError;

extern "C" {

int fbn_gci_host_run(const double *R, int nvars, int64_t nsamples, const int32_t *items, int64_t n, int d, double alpha,
                     double *r, double *z, double *p, uint8_t *indep, int64_t *degenerate) {
    if (n < 0 || (n > 0 && !items)) return SetError(FBN_ERR_ARG, "bad argument");
    if (int rc = fbn::CheckR(R, nvars)) return rc;
    double tau = 0.0;
    if (int rc = fbn::GciTau(alpha, nsamples, d, &tau)) return rc;
    if (int rc = fbn::GciCheckItems(items, n, d, nvars)) return rc;
    std::vector<double> rv((size_t)n);
    fbn::GciLog log;
    if (int rc = fbn::GciHostBatch(R, nvars, items, n, d, tau, rv.data(), indep, log)) return rc;
    for (int64_t t = 0; t < n; ++t) {
        double zt, pt;
        fbn::GciReport(rv[(size_t)t], nsamples, d, &zt, &pt);
        if (r) r[t] = rv[(size_t)t];
        if (z) z[t] = zt;
        if (p) p[t] = pt;
    }
    if (degenerate) *degenerate = log.degenerate;
    return FBN_OK;
}

int fbn_gci_host_pc_stable(const double *R, int nvars, int64_t nsamples, double alpha, int depth, fbn_pc_result **out) {
    if (!out) return SetError(FBN_ERR_ARG, "null pointer");
    if (int rc = fbn::CheckR(R, nvars)) return rc;
    auto res = std::unique_ptr<fbn_pc_result>(new (std::nothrow) fbn_pc_result());
    if (!res) return SetError(FBN_ERR_NOMEM, "out of memory");
    fbn::HostTester T(R, nvars);
    if (int rc = fbn::RunPCGauss(T, nvars, nsamples, alpha, depth, res->r)) return rc;
    *out = res.release();
    return FBN_OK;
}

int fbn_gci_tau(double alpha, int64_t nsamples, int d, double *tau) {
    if (!tau) return SetError(FBN_ERR_ARG, "null pointer");
    return fbn::GciTau(alpha, nsamples, d, tau);
}

int fbn_pc_degenerate(const fbn_pc_result *r, int64_t *n) {
    if (!r || !n) return SetError(FBN_ERR_ARG, "null pointer");
    *n = r->r.degenerate;
    return FBN_OK;
}

int fbn_cdataset_load_csv(const char *path, fbn_cdataset **out) {
    if (!path || !out) return SetError(FBN_ERR_ARG, "null pointer");
    auto h = std::unique_ptr<fbn_cdataset>(new (std::nothrow) fbn_cdataset());
    if (!h) return SetError(FBN_ERR_NOMEM, "out of memory");
    if (int rc = fbn::LoadRealCsv(path, &h->nvars, &h->nsamples, h->names, h->cols)) return rc;
    *out = h.release();
    return FBN_OK;
}
int fbn_cdataset_shape(const fbn_cdataset *ds, int *nvars, int64_t *nsamples) {
    if (!ds) return SetError(FBN_ERR_ARG, "null pointer");
    if (nvars) *nvars = ds->nvars;
    if (nsamples) *nsamples = ds->nsamples;
    return FBN_OK;
}
int fbn_cdataset_columns(const fbn_cdataset *ds, double *cols) {
    if (!ds || !cols) return SetError(FBN_ERR_ARG, "null pointer");
    std::copy(ds->cols.begin(), ds->cols.end(), cols);
    return FBN_OK;
}
int fbn_cdataset_var_name(const fbn_cdataset *ds, int v, char *buf, int cap) {
    if (!ds || !buf || cap <= 0 || v < 0 || v >= ds->nvars) return SetError(FBN_ERR_ARG, "bad argument");
    snprintf(buf, cap, "%s", ds->names[v].c_str());
    return FBN_OK;
}
int fbn_cdataset_destroy(fbn_cdataset *ds) {
    delete ds;
    return FBN_OK;
}

}  // extern "C"
