// ginf.h -- linear-Gaussian networks: what the host side (ginf_host.cpp) and the device entries
// (capi_ginf.hip) share.  The model, the joint and the per-case conventions are stated in include/fastbn.h;
// the per-element arithmetic is ginf_model.h's.  Internal to libfastbn.
#ifndef FBN_GINF_H
#define FBN_GINF_H

#include <cstdint>
#include <vector>

#include "fbn_internal.h"

struct fbn_gnet {
    int n = 0;
    std::vector<int32_t> off, par;  // the caller's CSR parent lists
    std::vector<double> intercept, coef, variance;
    std::vector<int32_t> order;  // Kahn's order, the lowest index first among the ready nodes
};

namespace fbn {

// validates and fills *net (a bad parent, a cycle, a variance that is not positive and finite: FBN_ERR_ARG)
int GnetBuild(int nvars, const int32_t *parent_off, const int32_t *parents, const double *intercept, const double *coef,
              const double *variance, fbn_gnet *net);
// mu [n], Sigma [n][n]
void GnetJoint(const fbn_gnet &net, double *mu, double *Sigma);
// maximum-likelihood parameters of the structure from the columns' means, centred sums of squares S_vv and
// correlation matrix R over N samples
int GnetLearn(int nvars, int64_t N, const double *mean, const double *ss, const double *R, const int32_t *parent_off,
              const int32_t *parents, fbn_gnet *net);

// every case's observed count against kGinfMaxObs and every value against infinity; *m_max: the largest count
int GinfCheckEvidence(const double *ev, int64_t ncases, int n, int *m_max);
// the host twin of ginf.hip; mean, var [ncases][n], logp [ncases] and the count of degenerate cases may each be null
void GinfHostRun(const double *mu, const double *Sigma, int n, const double *ev, int64_t ncases, double *mean, double *var,
                 double *logp, int64_t *degenerate);

}  // namespace fbn

#endif
