// launchers.h -- the extern "C" kernel launchers of libfastbn, declared once: included by the file that
// defines each one (jt_kernels.hip, jt_virt.hip, jt_tile.hip, ci_kernels.hip, ci_bits_*.hip, ci_l1.hip,
// ci_gram_mfma.hip, lbp.hip, sample.hip, epis.hip, ais.hip, jt_mpe.hip, jt_em.hip, jt_psample.hip, hc_score.hip, hc_bd.hip, gibbs.hip, exact_dp.hip, exact_bma.hip, order_mcmc.hip, gci_corr.hip, gci_test.hip, gscore.hip, ginf.hip) and by every caller (capi_*.hip), so a
// definition that disagrees with its declaration does not compile.  A launcher with many arguments
// takes one record that its caller fills by name: ci_args.h (CiArgs, CiBitsArgs, CiG2Args, CiL1Args),
// jt_program.h (JtArgs, JtLdsArgs), and the newer subsystems' own *_model.h / sample_device.h.
// Internal to libfastbn.  (pc_small.h and param_counts.h carry their own kernels' launchers.)
#ifndef FBN_LAUNCHERS_H
#define FBN_LAUNCHERS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ci_args.h"
#include "gscore.h"
#include "jt_program.h"
#include "lbp_model.h"

extern "C" hipError_t fbn_jt_launch(const JtArgs *a, int grid, hipStream_t stream);
extern "C" hipError_t fbn_jt_marg_transpose(const double *in, double *out, long long n, int SD, hipStream_t s);
extern "C" hipError_t fbn_jt_score_terms(const double *marg, const double *golden, long long n, int SD, int vmajor,
                                         const int32_t *dom, int V, double *terms, hipStream_t s);
// a->gstride is derived from lds_bytes here (the caller leaves it 0); split_grid: the counting launch
// of the split mode (a->split > 1)
extern "C" hipError_t fbn_ci_launch(const CiArgs *a, int d, size_t lds_bytes, int grid, int split_grid,
                                    hipStream_t stream);
extern "C" hipError_t fbn_ci_pack2_build(const uint8_t *cols, int nvars, long long N, long long PW, uint32_t *pk,
                                         hipStream_t stream);
extern "C" size_t fbn_ci_lds_bytes(int dimz, int dx, int dy);
extern "C" size_t fbn_ci_static_lds_bytes();
extern "C" hipError_t fbn_jt_evidence_check(const int8_t *ev, long long n, int V, const int32_t *dom,
                                            unsigned long long *first, hipStream_t s);
extern "C" hipError_t fbn_ci_cols_check(const uint8_t *cols, const int32_t *dims, int nvars, long long N, int *bad,
                                        hipStream_t s);
extern "C" hipError_t fbn_ci_bits_build(const uint8_t *cols, const int32_t *dims, const int32_t *row0, long long N,
                                        long long W, int nvars, uint32_t *bits, hipStream_t s);
extern "C" hipError_t fbn_ci_bits_launch(const CiBitsArgs *a, hipStream_t s);
extern "C" hipError_t fbn_ci_bits_rowcount(const uint32_t *bits, long long rows, long long W, int32_t *rowcnt,
                                           hipStream_t s);
extern "C" int fbn_ci_pair_block(int d);
extern "C" int fbn_ci_gram_task_ints(void);
extern "C" hipError_t fbn_ci_onehot4_build(const uint8_t *cols, const int32_t *dims, const int32_t *lead0, long long N,
                                           long long KS, long long Rp, int nvars, uint8_t *O4, hipStream_t s);
extern "C" hipError_t fbn_ci_gram4(const uint8_t *O4, long long Rp, const int2 *tasks, int nt, int S, int KS,
                                   uint16_t *slab, int R, long long ld, int32_t *gram, hipStream_t s);
extern "C" int fbn_ci_gram4_tile(void);
extern "C" int fbn_ci_gram4_stage(void);
extern "C" size_t fbn_ci_l1_edge_bytes(void);
extern "C" hipError_t fbn_ci_l1_results(const uint8_t *st, const int32_t *sep, const long long *cnt, int E,
                                        const long long *scal, char *h_rm, int32_t *h_sep, long long *h_sc,
                                        long long *part, hipStream_t s);
extern "C" hipError_t fbn_ci_kept_csr(const uint8_t *indep, int n, int32_t *low, int32_t *up, int32_t *off,
                                      int32_t *upoff, int32_t *adj, int32_t *pairs, long long *scal, hipStream_t s);
extern "C" hipError_t fbn_ci_l1_setup(const CiL1Args *a, hipStream_t s);
extern "C" hipError_t fbn_ci_l1_round(const CiL1Args *a, unsigned *open_cnt, unsigned *open_next, int next_chunk,
                                      unsigned epoch, hipStream_t s);
extern "C" hipError_t fbn_ci_gram(const uint32_t *bits, long long W, const int32_t *rl, const int32_t *tasks,
                                  long long ntasks, int32_t *out, int num_cu, hipStream_t s);
extern "C" hipError_t fbn_ci_gram_pairs(const int32_t *G, long long ld, const int32_t *lead0, const int32_t *dims,
                                        const int32_t *row0, const int32_t *rowcnt, long long t0, long long n,
                                        int nvars, int32_t *counts, int32_t *pairtab, int num_cu, hipStream_t s);
extern "C" hipError_t fbn_ci_bits_pairs_tiled(const uint32_t *bits, const int32_t *row0, const int32_t *rowcnt,
                                              long long W, const int32_t *tasks, long long ntasks, int nvars,
                                              long long t0, long long t1, int32_t *counts, int32_t *pairtab,
                                              int num_cu, hipStream_t s);
extern "C" hipError_t fbn_jt_tile_launch(const JtTPass *passes, int npass, const int32_t *tab, const double *iv,
                                         const int8_t *evid, double *marg, int32_t *labels, double *ws, int *flags,
                                         long long ncases, long long store_rows, long long scr_row, long long red_row,
                                         int V, int SD, int lds_bytes, int grid, int waves,
                                         unsigned long long *prof, hipStream_t stream);
extern "C" hipError_t fbn_jt_virt_launch(const JtVClique *cls, const int32_t *aux, const double *initv,
                                         const uint64_t *dig, const int32_t *order, const int32_t *sched,
                                         const int32_t *vsel, const int8_t *evid, double *marg, int32_t *labels,
                                         double *ws, int32_t *wsi, int *flags, long long ncases, long long store_rows,
                                         long long scratch_row, long long scratch_rows, int nc, int V, int SD,
                                         int grid, int dbg, hipStream_t stream);
extern "C" hipError_t fbn_jt_lds_launch(const JtLdsArgs *a, hipStream_t stream);
// lds != 0: the messages in lds_bytes of LDS per workgroup; else in a->ws, 3 * a->M doubles per workgroup
extern "C" hipError_t fbn_lbp_launch(const fbn::LbpDeviceArgs *a, int lds, size_t lds_bytes, int grid,
                                     hipStream_t stream);
// The sampling engine's kernels (sample_device.h's arguments): forward sampling, 64 samples per one-wave
// workgroup, and likelihood weighting / logic sampling, one workgroup per case.
namespace fbn {
struct ForwardDeviceArgs;
struct LwDeviceArgs;
struct EpisDeviceArgs;
}
extern "C" hipError_t fbn_sample_forward_launch(const fbn::ForwardDeviceArgs *a, hipStream_t stream);
extern "C" hipError_t fbn_lw_launch(const fbn::LwDeviceArgs *a, hipStream_t stream);
// EPIS-BN's sampling kernel (epis_model.h's arguments), one workgroup per case; lds_lambda != 0: the
// case's lambda row in LDS behind the values.  fbn_epis_fill: p[0 .. n) = x.
extern "C" hipError_t fbn_epis_launch(const fbn::EpisDeviceArgs *a, int lds_lambda, hipStream_t stream);
extern "C" hipError_t fbn_epis_fill(double *p, long long n, double x, hipStream_t stream);
// The adaptive samplers' kernel (ais_model.h's arguments): a persistent grid of `grid` one-wave
// workgroups striding over the cases, lds_bytes of dynamic LDS each; lds_state != 0: the ICPT and the
// counts in LDS behind the values and the weights, else in a->ws, 2 * a->cells doubles per workgroup.
namespace fbn {
struct AisDeviceArgs;
}
extern "C" hipError_t fbn_ais_launch(const fbn::AisDeviceArgs *a, int lds_state, size_t lds_bytes, int grid,
                                     hipStream_t stream);
// The max-product kernel (jt_mpe_program.h's arguments): a persistent grid of a->grid one-wave
// workgroups, 64 cases each per round, a->store_rows rows of a->store per workgroup.
struct JtMpeArgs;
extern "C" hipError_t fbn_mpe_launch(const JtMpeArgs *a, hipStream_t stream);
// The expectation-maximisation kernels (jt_em_program.h's arguments): the E-step, a persistent grid of
// a->grid one-wave workgroups as the max-product kernel's; the reduction of the waves' accumulators in
// wave order; the M-step with the rebuild of the initial potentials (one workgroup).
struct JtEmArgs;
struct JtEmReduceArgs;
struct JtEmMstepArgs;
extern "C" hipError_t fbn_em_estep_launch(const JtEmArgs *a, hipStream_t stream);
extern "C" hipError_t fbn_em_reduce_launch(const JtEmReduceArgs *a, hipStream_t stream);
extern "C" hipError_t fbn_em_mstep_launch(const JtEmMstepArgs *a, hipStream_t stream);
// The posterior-sampling kernel (jt_psample_program.h's arguments): a persistent grid of a->grid one-wave
// workgroups over the units (64-case block, chunk of a->chunk samples), a->store_rows rows of a->store each.
struct JtPsampleArgs;
extern "C" hipError_t fbn_psample_launch(const JtPsampleArgs *a, hipStream_t stream);
// The Gibbs sampler's kernels (gibbs_model.h's arguments).  fbn_gibbs_launch: a persistent grid of `grid`
// one-wave workgroups over the a->units (case, 64-chain chunk) units, lds_bytes of dynamic LDS each
// (lds_acc != 0: the accumulators among them; a->pc_cache: the parent configurations too), then the
// finish kernel over the cases.  fbn_gibbs_cond_launch: one assignment per lane.
namespace fbn {
struct GibbsDeviceArgs;
struct GibbsCondArgs;
}
extern "C" hipError_t fbn_gibbs_launch(const fbn::GibbsDeviceArgs *a, int lds_acc, size_t lds_bytes, int grid,
                                       hipStream_t stream);
extern "C" hipError_t fbn_gibbs_cond_launch(const fbn::GibbsCondArgs *a, size_t lds_bytes, hipStream_t stream);
// The family-score reduction of the hill-climbing learner (hc_score.hip): the counted tables of
// families [0, nfam) (param_counts.h's descriptors and key strides; tab as fbn_param_launch left it)
// -> out[2 f] = log-likelihood, out[2 f + 1] = log-likelihood - pen[f]; L[n] = n ln n for n <= N.
struct FbnParamFamily;
struct HcScoreArgs {
    const uint32_t *tab;
    const FbnParamFamily *fam;
    const int32_t *fstr;
    const double *pen, *L;
    double *out;
    long long nfam;
};
extern "C" hipError_t fbn_hc_score_launch(const HcScoreArgs *a, hipStream_t stream);
// The Bayesian Dirichlet reduction (hc_bd.hip) over the same tables: prior[2 f], prior[2 f + 1] = hc_bd.h's
// records of family f's cell and configuration parameter -> out[2 f] = log-likelihood (hc_score.hip's
// bits), out[2 f + 1] = the BD score.  Families are packed 64 / w to a wave by their width class (q <= w
// = 1, 2, .., 32; class 6: one wave each): fbn_hc_bd_bin (host) fills order (to be uploaded by the caller)
// and the class tables from the families' q; pack == 0 puts every family in class 6.
struct FbnBdPrior;
constexpr int kBdClasses = 7;
struct HcBdArgs {
    const uint32_t *tab;
    const FbnParamFamily *fam;
    const int32_t *fstr;
    const FbnBdPrior *prior;
    const double *L;
    double *out;
    const int32_t *order;                // [nfam] family indices, class by class
    long long cls_count[kBdClasses + 1]; // families of class c
    long long cls_first[kBdClasses + 1]; // its first entry of order
    long long cls_block[kBdClasses + 1]; // its first workgroup; [kBdClasses] = the grid
    long long nfam;
};
extern "C" void fbn_hc_bd_bin(const int32_t *q, long long nfam, int pack, int32_t *order, HcBdArgs *a);
extern "C" hipError_t fbn_hc_bd_launch(const HcBdArgs *a, hipStream_t stream);
// The lattice kernels of the exact learner (exact_dp.hip; the pass geometry is exact_dp.h's ExactPass).
// fbn_exact_pass_launch: one pass of the subset-max transform over all nvars lattices of 2^M entries
// (val fp64, arg uint32, variable-major), in place; init_arg != 0: the args are not read but start as the
// entries' own indices (the first pass).  fbn_exact_sink_launch: level `level` of the sink recursion over
// the subsets of that popcount (level 0 writes R[0] = 0).
struct ExactPassArgs {
    double *val;
    uint32_t *arg;
    int nvars, M;
    int gpos, hb, lo, s0, G;  // ExactPass
    int init_arg;
};
extern "C" hipError_t fbn_exact_pass_launch(const ExactPassArgs *a, hipStream_t stream);
struct ExactSinkArgs {
    const double *bps;
    double *R;
    uint8_t *sink;
    int nvars, level;
};
extern "C" hipError_t fbn_exact_sink_launch(const ExactSinkArgs *a, hipStream_t stream);
// The lattice kernels of the arc-posterior learner (exact_bma.hip; include/fastbn.h states the quantities).
// fbn_bma_pass_launch: one pass (ExactPass geometry over kBmaLdsBits) of a transform of all nvars value
// lattices x [nvars][2^M], in place after the load.  dir: kBmaSubset (an index with the bit set combines with
// its partner) or kBmaSuperset (with the bit clear); op: kBmaLse or kBmaAdd; load, what an entry starts as:
// kBmaLoadX x itself; kBmaLoadLs ls (the first alpha pass); kBmaLoadGamma F[U] + B[V \ U \ v] (the first
// Gamma pass); kBmaLoadP exp((ls + x) - F[V]) (the first q pass).  The valid triples are the six the
// learner uses; any other is hipErrorInvalidValue.
enum { kBmaSubset = 0, kBmaSuperset = 1 };
enum { kBmaLse = 0, kBmaAdd = 1 };
enum { kBmaLoadX = 0, kBmaLoadLs = 1, kBmaLoadGamma = 2, kBmaLoadP = 3 };
struct BmaPassArgs {
    double *x;
    const double *ls, *F, *B;  // read by the loads that name them
    int nvars, M;
    int gpos, hb, lo, s0, G;  // ExactPass
    int dir, op, load;
};
extern "C" hipError_t fbn_bma_pass_launch(const BmaPassArgs *a, hipStream_t stream);
// level `level` of the forward and backward recursions: F[W] and B[W] of every W of that popcount from level
// - 1 and the alpha lattices (level 0 writes F[0] = B[0] = 0)
struct BmaLevelArgs {
    const double *alpha;
    double *F, *B;
    int nvars, level;
};
extern "C" hipError_t fbn_bma_level_launch(const BmaLevelArgs *a, hipStream_t stream);
// out[u * nvars + v] = q_v[{u}] (0 on the diagonal), out[nvars * nvars + v] = q_v[{}], then F[V] and B[V]:
// nvars * nvars + nvars + 2 doubles
extern "C" hipError_t fbn_bma_gather_launch(const double *q, const double *F, const double *B, int nvars, double *out,
                                            hipStream_t stream);
// The order-MCMC kernels (order_mcmc.hip; order_mcmc.h's arguments): a->group chains (one wave each) per
// workgroup, fbn_omcmc_wave_lds_bytes() of dynamic LDS per wave.  fbn_omcmc_chain_launch: the steps [a->t0, a->t1)
// of every chain; fbn_omcmc_terms_launch: the terms and arc features of a->k given orders, one wave each.
namespace fbn {
struct OmcmcDeviceArgs;
struct OmcmcTermsArgs;
}
extern "C" size_t fbn_omcmc_wave_lds_bytes(void);
extern "C" hipError_t fbn_omcmc_chain_launch(const fbn::OmcmcDeviceArgs *a, hipStream_t stream);
extern "C" hipError_t fbn_omcmc_terms_launch(const fbn::OmcmcTermsArgs *a, hipStream_t stream);
// The correlation kernels of the Gaussian CI test (gci_corr.hip) over X float64 [nvars][N].
// fbn_gci_means_launch: mean[v] and bad[v] (the column holds a non-finite value).  fbn_gci_gram_launch: the
// centred Gram's upper tiles of tile x tile variables (64 or 32) in split_k sample slices of whole stages
// (fbn_gci_stage() samples; 1 <= split_k <= stages) into slab, split_k * nt * tile^2 doubles with nt = T (T + 1) / 2,
// T = ceil(nvars / tile).  fbn_gci_reduce_launch: the slices summed in order -> R [nvars][nvars] (symmetric, unit
// diagonal) and var[v] = S_vv.
struct GciCorrArgs {
    const double *X;
    double *mean;
    int *bad;
    double *slab, *R, *var;
    int nvars;
    long long N;
    int tile, split_k;
};
extern "C" int fbn_gci_stage(void);
extern "C" hipError_t fbn_gci_means_launch(const double *X, int nvars, long long N, double *mean, int *bad, hipStream_t stream);
extern "C" hipError_t fbn_gci_gram_launch(const GciCorrArgs *a, hipStream_t stream);
extern "C" hipError_t fbn_gci_reduce_launch(const GciCorrArgs *a, hipStream_t stream);
// The test kernel (gci_test.hip): n tests of d conditioning variables (0..8), one per lane; items [n][2 + d], or
// null with d == 0: test t is pair t of the complete graph.  r is optional.  stats: {smallest | |r| - tau | as
// IEEE bits, tests within 1e-9 of tau, degenerate tests}, updated with one atomic group per wave.
struct GciTestArgs {
    const double *R;
    int nvars;
    const int32_t *items;
    long long n;
    double tau;
    double *r;
    uint8_t *indep;
    unsigned long long *stats;
};
extern "C" hipError_t fbn_gci_test_launch(const GciTestArgs *a, int d, hipStream_t stream);
// The Gaussian family scorer (gscore.hip; gscore.h's scores): n families of p parents (0..8), one per lane, as
// records rec [n][2 + p] = (out_index, child, parents ascending); each lane writes loglik[out_index] and
// score[out_index] and the waves add their degenerate families to *degenerate.  lss, tq [nvars] and C are
// gscore.h's tables.
struct GscoreArgs {
    const double *R, *lss, *tq;
    int nvars;
    const int32_t *rec;
    long long n;
    double *loglik, *score;
    unsigned long long *degenerate;
    FbnGsConsts C;
};
extern "C" hipError_t fbn_gscore_launch(const GscoreArgs *a, int p, int bge, hipStream_t stream);
// Exact inference in a linear-Gaussian network (ginf.hip): ncases evidence rows ev [ncases][n] (NaN = unobserved)
// conditioned on the joint mu [n], Sigma [n][n]; one workgroup of 256 threads per case, a persistent grid of
// `grid` workgroups with lds_bytes = fbn_ginf_lds_bytes(n, m_max) (ginf_model.h) of dynamic LDS each, m_max the
// batch's largest observed count (<= kGinfMaxObs: a case past it, which the caller refuses beforehand, gets
// NaN).  mean, var [ncases][n] and logp [ncases] may each be null.  fbn_ginf_check_launch: word[0] = the
// smallest flat index of an infinite value, word[1] = ~0 - the largest observed count (both start as ~0).
struct GinfArgs {
    const double *mu, *Sigma;
    int n;
    const double *ev;
    long long ncases;
    double *mean, *var, *logp;
    int lds_bytes;
};
extern "C" hipError_t fbn_ginf_launch(const GinfArgs *a, int grid, hipStream_t stream);
extern "C" hipError_t fbn_ginf_check_launch(const double *ev, long long ncases, int n, unsigned long long *word, int grid,
                                            hipStream_t stream);

#endif
