// ais_model.h -- what the adaptive samplers' host twin (ais_host.cpp) and their kernel (ais.hip)
// share: the stage schedule, the draw from an importance CPT row and the row update, each defined
// once and compiled by both sides.
//
// AIS-BN (Adaptive Importance Sampling, Cheng & Druzdzel 2000; the reference's `-a 10`, ALGAISBN) and
// self-importance sampling (SIS, after Shachter & Peot 1989; `-a 8`, ALGSIS) only print "under
// development" there (src/main.cpp:175-186, :149-160).  Both learn, per evidence case, an importance
// CPT (ICPT) for the unobserved ancestors of the evidence from weighted family counts of their own
// samples; they differ in the schedule (fastbn.h, "adaptive importance sampling", is the specification).
#ifndef FBN_AIS_MODEL_H
#define FBN_AIS_MODEL_H

#include <cstdint>

#include "epis_model.h"
#include "sample_model.h"

// fbn_ais_set_tuning: what the values, the weights, the flags and the state (ICPT, counts) may take in LDS
#define FBN_AIS_LDS_DEFAULT ((int64_t)64 * 1024)
// maximum updates (-m)
#define FBN_AIS_MAX_UPDATES 1024
// workgroups per CU of the persistent grid (one wave each)
#define FBN_AIS_GROUPS_PER_CU 16

namespace fbn {

// The stages of one case: nupd learning stages of l samples, each followed by an update, then one stage
// of `last` samples.  AIS-BN (method 0): nupd = m, last = S, only the last stage is counted.  SIS
// (method 1): nupd = min(m, (S - 1) / l) (full blocks of l after which samples remain), last = S - nupd * l,
// every stage is counted.  T = nupd * l + last draws per case.
struct AisSchedule {
    int64_t nupd, l, last, T;
};
FBN_HD AisSchedule AisStages(int method, int64_t S, int64_t m, int64_t l) {
    AisSchedule s;
    s.l = l;
    if (method == 0) {
        s.nupd = m, s.last = S;
    } else {
        const int64_t full = (S - 1) / l;
        s.nupd = m < full ? m : full;
        s.last = S - s.nupd * l;
    }
    s.T = s.nupd * l + s.last;
    return s;
}

// One draw of a learnable variable with d states from table row P[0 .. d) and ICPT row I[0 .. d),
// uniform u: EpisDraw's rule (epis_model.h) with g(q) = I[q] in place of P[q] * lambda[q].
FBN_HD int AisDraw(const double *P, const double *I, int d, double eps, double u, double *factor) {
    double z = 0.0, gmin = I[0];
    for (int q = 0; q < d; ++q) {
        const double g = I[q];
        z = z + g;
        gmin = g < gmin ? g : gmin;
    }
    const bool lw = LbpBadZ(z);
    const double flo = (lw || !(eps > 0.0)) ? 0.0 : eps * z;
    double tot = z;  // nothing raised: c(d - 1) is the sum just taken
    if (lw || gmin < flo) {
        tot = 0.0;
        for (int q = 0; q < d; ++q) {
            const double g = lw ? P[q] : I[q];
            tot = tot + (g < flo ? flo : g);
        }
    }
    const double x = u * tot;
    double c = 0.0, gv = 0.0;
    int q = 0;
    for (;; ++q) {
        const double g = lw ? P[q] : I[q];
        gv = g < flo ? flo : g;
        c = c + gv;
        if (!(q < d - 1 && x >= c)) break;
    }
    *factor = gv > 0.0 ? (P[q] * tot) / gv : 0.0;
    return q;
}

// Update of one ICPT row I[0 .. d) from its counts N[0 .. d) with learning rate eta: t = sum_q N[q]
// ascending from 0.0; t > 0 and finite: I[q] <- I[q] + eta * (N[q] / t - I[q]); else the row stays.  Not
// renormalised (the draw normalises by its own running sum).
FBN_HD void AisUpdateRow(double *I, const double *N, int d, double eta) {
    double t = 0.0;
    for (int q = 0; q < d; ++q) t = t + N[q];
    if (!(t > 0.0) || LbpBadZ(t)) return;
    for (int q = 0; q < d; ++q) I[q] = I[q] + eta * (N[q] / t - I[q]);
}

// eta[0 .. m): AIS-BN a * (b / a)^(k / m) with a = 0.4, b = 0.14 (the paper's schedule); SIS 1.0.  Host
// only (pow): the kernel reads the table.
void AisEta(int method, int m, double *eta);

// The algorithm over cases on CPU threads, operation for operation what the kernel does.  labels
// [ncases], marg [ncases][sum_dom] or NULL, stats [ncases][4] or NULL; dbg_* (all or none): values
// [V][ncases * T], mantissas / exponents [ncases * T], ICPT [ncases][cells].
int HostAis(const SamplerModel &M, int method, const int8_t *ev, int64_t ncases, int64_t S, int64_t m, int64_t l,
            uint64_t seed, int64_t case_offset, double eps, int32_t *labels, double *marg, double *stats,
            uint8_t *dbg_vals, double *dbg_m, int32_t *dbg_e, double *dbg_icpt);
// method 0 / 1, S >= 1, 0 <= m <= 1024, l >= 1, eps < 1 (not NaN) and not 0 with method 1, stream
// positions below 2^63, else FBN_ERR_ARG
int CheckAisArgs(const SamplerModel &M, int method, int64_t ncases, int64_t S, int64_t m, int64_t l,
                 int64_t case_offset, double eps);

}  // namespace fbn

#if defined(__HIPCC__)
#include "sample_device.h"

namespace fbn {

// sample_ais_kernel's arguments (ais.hip; filled by capi_ais.hip); stats [ncases][4], draws = sch.T
struct AisDeviceArgs : SampleCaseArgs {
    U128 sm, sc;  // a learning stage's last chunk to the next stage's first: (l - 64 ((l - 1) / 64) - 1) V
    long long cells;
    int method;
    AisSchedule sch;
    double eps;         // < 0: EpisCutoff's defaults
    const double *eta;  // [sch.nupd]
    double *ws;         // state in global memory: [grid][2 * cells], or NULL (state in LDS)
    double *di;         // debug, with dv: the ICPT after the last update [ncases][cells]
};

}  // namespace fbn
#endif

#endif
