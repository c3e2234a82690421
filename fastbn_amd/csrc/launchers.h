// launchers.h -- the extern "C" kernel launchers of libfastbn, declared once: included by the file that
// defines each one (jt_kernels.hip, jt_virt.hip, jt_tile.hip, ci_kernels.hip, ci_bits_*.hip, ci_l1.hip,
// ci_gram_mfma.hip, lbp.hip, sample.hip, epis.hip, ais.hip, jt_mpe.hip, jt_em.hip, hc_score.hip) and by every caller (capi_*.hip), so a
// definition that disagrees with its declaration does not compile.  A launcher with many arguments
// takes one record that its caller fills by name: ci_args.h (CiArgs, CiBitsArgs, CiG2Args, CiL1Args),
// jt_program.h (JtArgs, JtLdsArgs), and the newer subsystems' own *_model.h / sample_device.h.
// Internal to libfastbn.  (pc_small.h and param_counts.h carry their own kernels' launchers.)
#ifndef FBN_LAUNCHERS_H
#define FBN_LAUNCHERS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ci_args.h"
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

#endif
