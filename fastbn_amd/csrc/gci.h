// gci.h -- PC-stable on continuous data (Fisher-z partial correlation): what the driver (gci_pc.cpp), the
// host twin (gci_host.cpp) and the device entry (capi_gci.hip) share.  Internal to libfastbn.
//
// The test of (x, y | Z), |Z| = d, on N samples: r = the partial correlation from the correlation matrix R
// (gci_elim.h); independent iff |r| <= tau_d, tau_d = tanh(Phi^-1(1 - alpha / 2) / sqrt(N - d - 3)) -- exactly
// "p > alpha" of the two-sided Fisher-z test, with no transcendental per test.  z = sqrt(N - d - 3) atanh(r)
// and p = erfc(|z| / sqrt 2) are formed on the host from r for reporting only.
#ifndef FBN_GCI_H
#define FBN_GCI_H

#include <cstdint>
#include <string>
#include <vector>

#include "pc_internal.h"

namespace fbn {

// tau_d of (alpha, N, d); FBN_ERR_ARG unless 0 < alpha < 1, FBN_ERR_LIMIT when N - d - 3 <= 0
int GciTau(double alpha, int64_t N, int d, double *tau);
// z and p of r (NaN for a degenerate test's NaN)
void GciReport(double r, int64_t N, int d, double *z, double *p);
// items [n][2 + d] checked against nvars (every index in range, x != y, no z equal to x or y)
int GciCheckItems(const int32_t *items, int64_t n, int d, int nvars);

// what a batch leaves beside its decisions
struct GciLog {
    double min_margin = __builtin_inf();  // smallest | |r| - tau | over the non-degenerate tests
    int64_t near = 0;                     // of them, those within 1e-9 of tau
    int64_t degenerate = 0;
};

// n tests on the host: items == nullptr: test t is pair t of the complete graph over nvars variables
// (PairIndex order).  r and indep are optional.
int GciHostBatch(const double *R, int nvars, const int32_t *items, int64_t n, int d, double tau, double *r,
                 uint8_t *indep, GciLog &log);

// Who runs the tests of RunPCGauss: two slots, as CiBatchLaunch / CiBatchWait (pc_internal.h).
class GciTester {
  public:
    virtual ~GciTester() {}
    // n tests of size d into slot k; items == nullptr: the complete graph's pairs [0, n)
    virtual int Launch(int k, const int32_t *items, int64_t n, int d, double tau) = 0;
    // slot k's decisions; adds the batch's kernel time to res
    virtual int Wait(int k, uint8_t *indep, PCResultHost &res) = 0;
    virtual int Log(GciLog *log) = 0;  // over every batch since the tester was made
};

// The reference's sequential PC-stable (pc_driver.cpp's header; group size 1) with Gaussian tests: level 0
// over the implicit complete graph, levels d >= 1 by LevelSearch in two alternating halves, removals and
// ContinueAfter after each level, OrientPC at the end.
int RunPCGauss(GciTester &T, int nvars, int64_t N, double alpha, int depth, PCResultHost &res);

// the moments a device context holds, downloaded: mean [n], the centred sums of squares S_vv [n], R [n][n]
// (defined beside the context, capi_gci.hip)
int GciMoments(fbn_gci_ctx *c, int *nvars, int64_t *N, std::vector<double> &mean, std::vector<double> &ss,
               std::vector<double> &R);

int LoadRealCsv(const std::string &path, int *nvars, int64_t *nsamples, std::vector<std::string> &names,
                std::vector<double> &cols);

}  // namespace fbn

struct fbn_cdataset {
    int nvars = 0;
    int64_t nsamples = 0;
    std::vector<std::string> names;
    std::vector<double> cols;  // [var][sample]
};

#endif
