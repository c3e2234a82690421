// epis_model.h -- what EPIS-BN's host twin (epis_host.cpp) and its kernel (epis.hip) share: the
// cutoff rule and the one definition of a draw from the importance function that both compile.
//
// EPIS-BN (Evidence Pre-propagation Importance Sampling, Yuan & Druzdzel 2003; the reference's
// `-a 6`, ALGEPISBN, which only prints "EPIS-BN is under development", src/main.cpp:123-134): loopy
// belief propagation first, then every unobserved variable x is drawn in topological order from
// P(x | pa) * lambda(x) instead of P(x | pa), lambda(x) being the variable -> factor message of x into
// its own family (the normalised product of what its children's families send it), and the sample's
// weight takes the ratio.
#ifndef FBN_EPIS_MODEL_H
#define FBN_EPIS_MODEL_H

#include <cstdint>

#include "lbp_model.h"
#include "sample_model.h"

// fbn_epis_set_tuning: what the values [V][64] and the lambda row may take in LDS together
#define FBN_EPIS_LDS_DEFAULT ((int64_t)64 * 1024)

namespace fbn {

// eps < 0: the defaults by state count after Yuan & Druzdzel (0.006 below 5 states, 0.001 for 5 to
// 8, 0.0005 above); else eps itself for every variable
FBN_HD double EpisCutoff(double eps, int d) { return eps >= 0.0 ? eps : (d < 5 ? 0.006 : (d <= 8 ? 0.001 : 0.0005)); }

// One draw of a variable with d states from table row P[0 .. d) and lambda row L[0 .. d), uniform u:
//   g(q) = P[q] * L[q];  Z = sum_q g(q), ascending from 0.0;
//   Z zero or not finite: g' = P (a likelihood-weighting draw, no cutoff);
//   else with cutoff eps > 0: g'(q) = max(g(q), eps * Z) (raise, then renormalise by c(d - 1)); else g' = g;
//   c(q) = the running sum of g', ascending from 0.0;  x = u * c(d - 1);  value = SelectValue's rule on c;
//   *factor = (P[value] * c(d - 1)) / g'(value), or 0.0 when g'(value) is 0 (x == c(d - 1) by rounding
//   on a last state of probability 0: the sample is impossible and weighs nothing).
// Passes that recompute g' -- no per-draw array, nothing indexed dynamically.  The pass that sums g'
// is skipped when it would repeat the sum of g term for term (no cutoff, or no g below it).  Only +, *,
// / and comparisons: the same bits on host and device.
FBN_HD int EpisDraw(const double *P, const double *L, int d, double eps, double u, double *factor) {
    double z = 0.0, gmin = P[0] * L[0];
    for (int q = 0; q < d; ++q) {
        const double g = P[q] * L[q];
        z = z + g;
        gmin = g < gmin ? g : gmin;
    }
    const bool lw = LbpBadZ(z);
    const double flo = (lw || !(eps > 0.0)) ? 0.0 : eps * z;
    double tot = z;  // nothing raised: c(d - 1) is the sum just taken
    if (lw || gmin < flo) {
        tot = 0.0;
        for (int q = 0; q < d; ++q) {
            const double g = lw ? P[q] : P[q] * L[q];
            tot = tot + (g < flo ? flo : g);
        }
    }
    const double x = u * tot;
    double c = 0.0, gv = 0.0;
    int q = 0;
    for (;; ++q) {
        const double g = lw ? P[q] : P[q] * L[q];
        gv = g < flo ? flo : g;
        c = c + gv;
        if (!(q < d - 1 && x >= c)) break;
    }
    *factor = gv > 0.0 ? (P[q] * tot) / gv : 0.0;
    return q;
}

// The algorithm over cases on CPU threads, operation for operation what the two launches do:
// HostLbp's lambda rows (iters == 0: rows of 1.0), then HostImportance.  labels [ncases], marg
// [ncases][sum_dom] or NULL, stats [ncases][4] or NULL; dbg_* (all or none): values [V][ncases * S],
// mantissas / exponents [ncases * S], lambda rows [ncases][sum_dom].
int HostEpis(const SamplerModel &SM, const LbpModel &LM, const int8_t *ev, int64_t ncases, int64_t S, uint64_t seed,
             int64_t case_offset, int iters, double tol, double damping, double eps, int32_t *labels, double *marg,
             double *stats, uint8_t *dbg_vals, double *dbg_m, int32_t *dbg_e, double *dbg_lam);
// S >= 1, iters >= 0, tol >= 0 (not NaN), 0 <= damping < 1, eps < 1 (not NaN), stream positions
// below 2^63, else FBN_ERR_ARG
int CheckEpisArgs(const SamplerModel &M, int64_t ncases, int64_t S, int64_t case_offset, int iters, double tol,
                  double damping, double eps);

}  // namespace fbn

#if defined(__HIPCC__)
#include "sample_device.h"

namespace fbn {

// sample_epis_kernel's arguments (epis.hip; filled by capi_epis.hip); stats [ncases][4], draws = S
struct EpisDeviceArgs : SampleCaseArgs {
    double eps;               // < 0: EpisCutoff's defaults
    const double *lam;        // [ncases][sum_dom]
    const double *lbp_stats;  // [ncases][2] or NULL (no pre-propagation: zeros)
};

}  // namespace fbn
#endif

#endif
