/* fastbn.h -- C-ABI of the MI355X-native FastBN hot paths (libfastbn.so).
 *
 * Drop-in boundary for the two data-parallel paths of the reference:
 *   * JT: batched junction-tree sum-product.  Replaces the per-case loop of
 *         JunctionTree::PredictUseJTInfer (src/JunctionTree.cpp:1473-1534) behind
 *         Inference::EvaluateAccuracy (include/Inference.h:44).
 *   * PC: the PC-stable skeleton CI sweep.  Replaces IndependenceTest::IndependenceResult
 *         (include/IndependenceTest.h:56, src/IndependenceTest.cpp:35-364) and the level loop of
 *         PCStable::StructLearnByPCStable / SearchAtDepth (src/PCStable.cpp:49-563) behind
 *         StructureLearning::StructLearnCompData (include/StructureLearning.h:22).
 *
 * Conventions: every function returns 0 (FBN_OK) or a negative fbn_err_t; fbn_last_error()
 * gives the message of the last failure on the calling thread.  No exceptions cross the ABI.
 * Plain pointers and sizes only.  Host arrays are caller-owned and only touched during the call;
 * device buffers are owned by the handle.  A handle is bound to one device and is not
 * thread-safe; multi-GPU = one handle per device (one process per GPU).
 */
#ifndef FASTBN_H
#define FASTBN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    FBN_OK = 0,
    FBN_ERR_ARG = -1,     /* bad argument / shape */
    FBN_ERR_IO = -2,      /* file missing or malformed (the reference exit(1)s here) */
    FBN_ERR_HIP = -3,     /* HIP runtime / kernel failure */
    FBN_ERR_NOMEM = -4,   /* host or device allocation failed */
    FBN_ERR_NODEV = -5,   /* no usable gfx950 device */
    FBN_ERR_LIMIT = -6    /* plan exceeds a kernel limit (e.g. variables per clique) */
} fbn_err_t;

const char *fbn_last_error(void);
int fbn_version(int *major, int *minor);
int fbn_device_count(int *n);

/* ------------------------------------------------------------------ networks & data (host) */
typedef struct fbn_network fbn_network;

/* XMLBIF -> discrete network with the reference's CPT convention ((int(p*1e4)+1)/(sum+|dom|),
 * node-major TABLE).  Replaces CustomNetwork::GetNetFromXMLBIFFile (src/CustomNetwork.cpp:20-41)
 * + XMLBIFParser (src/XMLBIFParser.cpp:3-218). */
int fbn_network_load_xmlbif(const char *path, fbn_network **out);
/* A network built in memory -- learned, or constructed by the caller -- with no file in between.
 * Mirrors what the reference's Network of DiscreteNodes holds after InitializeCPT + AddCount
 * (src/DiscreteNode.cpp:114-147): node v has dims[v] states, parents parents[parent_off[v] ..
 * parent_off[v+1]) (any order: the node's own parent order) and the count map
 * map_cond_prob_table_statistics as int64 counts[value][parent config] (parent configurations over
 * the parents in ASCENDING index order, last fastest -- a DiscreteConfig is an ordered set), node
 * after node in one array; totals are the sums over the values (as AddCount keeps
 * map_total_count_under_parents_config), probabilities (count + 1) / (total + dims[v]) as
 * GetProbability (:154-164).  names may be NULL ("X<v>").  The parent lists must form a DAG.
 * The JunctionTree(Network*, ...) constructor of the reference (src/JunctionTree.cpp:3-9) binds to
 * this + fbn_jt_plan_create. */
int fbn_network_create(int nvars, const int32_t *dims, const int32_t *parent_off /* [nvars+1] */,
                       const int32_t *parents, const int64_t *counts, const char *const *names,
                       fbn_network **out);
/* Node v's parents (ascending) and count map in fbn_network_create's layout; NULL buffers: sizes only.
 * A probability network (fbn_network_create_cpt) has no counts: FBN_ERR_ARG. */
int fbn_network_node_counts(const fbn_network *net, int node, int32_t *parents, int64_t *counts, int *nparents,
                            int64_t *ncounts);
/* A network that holds probabilities instead of counts (what expectation-maximisation produces: its
 * expected counts are fractional).  Arguments and validation as fbn_network_create, with cpt in its
 * layout: fp64 cpt[value][config of the ascending parents, last fastest], node after node.  Every entry
 * must be finite and > 0 and every column (the values under one parent configuration) must sum to 1
 * within 1e-9, else FBN_ERR_ARG naming the node.  Every consumer of a network reads such a network's
 * entries as they are (no smoothing); a count network behaves as before. */
int fbn_network_create_cpt(int nvars, const int32_t *dims, const int32_t *parent_off /* [nvars+1] */,
                           const int32_t *parents, const double *cpt, const char *const *names, fbn_network **out);
/* Node v's parents (ascending) and probability table in fbn_network_create's layout, for either kind of
 * network: the stored entries, or (count + 1) / (total + dims[v]).  NULL buffers: sizes only. */
int fbn_network_node_probs(const fbn_network *net, int node, int32_t *parents, double *probs, int *nparents,
                           int64_t *nprobs);
int fbn_network_num_nodes(const fbn_network *net, int *n);
int fbn_network_dims(const fbn_network *net, int32_t *dims /* [n] */);
int fbn_network_name(const fbn_network *net, int node, char *buf, int cap);
int fbn_network_destroy(fbn_network *net);

/* LIBSVM test set -> evidence rows.  Replaces Dataset::LoadLIBSVMDataKnownNetwork
 * (src/Dataset.cpp:162-262) + the evidence extraction of Inference::Inference
 * (src/Inference.cpp:13-42).  evidence: [ncases][num_nodes] int8, -1 = unobserved.
 * Call with evidence == NULL to get the case count. */
int fbn_evidence_load_libsvm(const char *path, int num_nodes, int8_t *evidence, int32_t *labels,
                             int64_t cap, int64_t *ncases);

/* Seeded workload generators (the reference's SampleSetGenerator is wall-clock seeded
 * and unreachable): forward sampling of n complete cases (cols [V][n] uint8, the reference's CPT
 * convention) and n evidence cases observing k variables each, never `query`, -1 elsewhere
 * (evidence [n][V] int8).  Bit-identical to fastbn_amd/synth.py's numpy PCG64(seed) generators. */
int fbn_synth_forward_sample(const fbn_network *net, int64_t n, uint64_t seed, uint8_t *cols);
int fbn_synth_evidence(const fbn_network *net, int64_t n, int k, uint64_t seed, int query, int8_t *evidence);
/* Writers of the reference's input formats (multi-threaded): CSV with header (network names or
 * X<v>) and values "s<code>"; LIBSVM rows "label v:x ..." of the observed variables. */
int fbn_write_csv(const char *path, const uint8_t *cols, int nvars, int64_t n, const fbn_network *net);
int fbn_write_libsvm(const char *path, const int8_t *evidence, int64_t n, int num_nodes, const int32_t *labels);

typedef struct fbn_dataset fbn_dataset;
/* CSV with header and string values coded by first appearance; column store uint8 [var][sample].
 * Replaces Dataset::LoadCSVData + RowMajor2ColumnMajor (src/Dataset.cpp:267-414,568-580). */
int fbn_dataset_load_csv(const char *path, fbn_dataset **out);
int fbn_dataset_shape(const fbn_dataset *ds, int *nvars, int64_t *nsamples);
int fbn_dataset_dims(const fbn_dataset *ds, int32_t *dims);
int fbn_dataset_columns(const fbn_dataset *ds, uint8_t *cols /* [nvars][nsamples] */);
int fbn_dataset_var_name(const fbn_dataset *ds, int v, char *buf, int cap);
int fbn_dataset_destroy(fbn_dataset *ds);

/* ------------------------------------------------------------------ junction tree */
typedef struct fbn_jt_plan fbn_jt_plan;

typedef struct {
    int32_t num_nodes, num_cliques, num_separators, num_levels;
    int32_t root, sum_dom;
    int64_t clique_entries;     /* sum of clique table sizes */
    int64_t separator_entries;  /* sum of separator table sizes */
    int64_t algorithmic_bytes_per_case; /* 16*(clique+sep entries) + 8*sum_dom + num_nodes */
    int32_t num_ops;            /* device program length */
    int32_t max_vars_per_table;
    int32_t specialized_eligible; /* cliques small enough for the plan-specialized kernel */
    int32_t variant;              /* kernel variant runs use (-1 auto before the first run) */
    int32_t streamed_eligible;    /* the streamed kernel (variant 4) can take the plan */
    int32_t streamed_waves;       /* waves sharing one 64-case block in variant 4 */
    double streamed_split_efficiency; /* modelled parallel efficiency of their subtree split */
    int32_t tiled_eligible;       /* the tiled kernel (variant 5, fast order) can take the plan */
    int32_t tiled_passes;         /* its clique passes per case group */
    int64_t tiled_entry_visits;   /* clique entries summed over those passes (one case) */
    int64_t tiled_lds_bytes;      /* LDS per wave for staged factors */
    int64_t tiled_table_bytes;    /* its index tables (G / R records, ...) */
} fbn_jt_plan_info;

/* Build the case-independent schedule (JunctionTree ctor, src/JunctionTree.cpp:3-46:
 * JunctionTreeStructure src/JunctionTreeStructure.cpp:12-348, root/levels/reorganization
 * :137-281), compile it to a device program and upload it to `device`.  device < 0 builds a
 * host-only plan (info / dump; runs return FBN_ERR_NODEV).
 * A clique's initial potential is the plain fp64 product of the CPT entries it hosts.  A probability
 * network's entries can take one below DBL_MIN (zero or subnormal); such a plan is refused with
 * FBN_ERR_LIMIT naming the clique and one of its nodes, here and in fbn_jt_forest_plan_create. */
int fbn_jt_plan_create(const fbn_network *net, int device, fbn_jt_plan **out);
/* The same plan for any DAG: where the moral graph is disconnected (fbn_jt_plan_create: FBN_ERR_ARG)
 * this builds a junction FOREST -- per component exactly the tree fbn_jt_plan_create builds for that
 * component alone (an isolated node: one clique of one variable), one root per component, nothing
 * passed between the trees (a message across components would be the constant 1).  Its cost is the
 * sum of its trees'; the product of the components' evidence likelihoods is never formed.  The
 * result is an ordinary plan: every fbn_jt_* call takes it, in every kernel variant whose limits the
 * trees meet.  On a connected network the plan is fbn_jt_plan_create's, byte for byte in
 * fbn_jt_plan_dump (a forest's dump adds one line, "roots <n> <clique> ...", after "root"). */
int fbn_jt_forest_plan_create(const fbn_network *net, int device, fbn_jt_plan **out);
/* Components of the plan's moral graph, numbered by their lowest node: component_of_node
 * [num_nodes] (NULL: the count alone).  A plan from fbn_jt_plan_create has one. */
int fbn_jt_plan_components(const fbn_jt_plan *p, int32_t *component_of_node /* [num_nodes] or NULL */,
                           int32_t *num_components);
int fbn_jt_plan_info_get(const fbn_jt_plan *p, fbn_jt_plan_info *info);
/* Text dump in the same format as the reference harness (tests/golden/alarm_1k.plan/.init). */
int fbn_jt_plan_dump(const fbn_jt_plan *p, const char *plan_path, const char *init_path);
/* Diagnostics: the streamed kernel's clique schedule.  order[n_order] = clique ids of the segments
 * sched[0..n_sched-1] delimits (waves W = streamed_waves): Collect per wave (W), Collect top,
 * Distribute top, Distribute per wave (W), end.  Pass NULL buffers to query the sizes. */
int fbn_jt_stream_schedule(const fbn_jt_plan *p, int32_t *order, int64_t order_cap, int32_t *sched,
                           int64_t sched_cap, int64_t *n_order, int64_t *n_sched);
/* Evidence cases on the host: evidence [ncases][num_nodes] int8; labels_out [ncases] (arg-max
 * of the query variable 0, InferenceUsingJT src/JunctionTree.cpp:1459-1467; 0 for a case that
 * observes the query itself: the arg-max of its row of zeros, as the sampling engines); marginals_out
 * [ncases][sum_dom] fp64 or NULL (GetProbabilitiesAllNodes :1385-1454, evidence nodes = 0).
 * Copies in/out over PCIe; synchronous. */
int fbn_jt_run(fbn_jt_plan *p, const int8_t *evidence, int64_t ncases, int32_t *labels_out,
               double *marginals_out, void *hip_stream);
/* Same with device-resident buffers (inputs already in HBM); asynchronous on hip_stream.  Every
 * evidence code must be -1 or < the node's state count: by default the call checks that on the
 * device first (one stream sync) and returns FBN_ERR_ARG naming the first bad case/node; see
 * fbn_jt_set_evidence_check. */
int fbn_jt_run_device(fbn_jt_plan *p, const int8_t *d_evidence, int64_t ncases, int32_t *d_labels,
                      double *d_marginals, void *hip_stream);
/* The device-side evidence check alone (synchronous on hip_stream): FBN_ERR_ARG on the first
 * out-of-domain code.  For callers that validate a buffer once and run it many times. */
int fbn_jt_evidence_validate(fbn_jt_plan *p, const int8_t *d_evidence, int64_t ncases, void *hip_stream);
/* enable = 0: fbn_jt_run_device skips its check (fully asynchronous); the caller guarantees valid
 * evidence (e.g. fbn_jt_evidence_validate once per buffer).  An unchecked out-of-domain code gives
 * unspecified marginals and labels for its case (never an out-of-bounds access).  Default 1.
 * fbn_jt_run always checks. */
int fbn_jt_set_evidence_check(fbn_jt_plan *p, int enable);
/* Per-case MSE and Hellinger distance vs a golden table (CalculateMSE / CalculateHellingerDistance
 * with Round(.,7), src/Inference.cpp:153-206); golden [ncases][sum_dom], evidence nodes marked by
 * golden[.][first state] <= 0.  Host arrays; sums accumulated in case order. */
int fbn_jt_score(const fbn_jt_plan *p, const double *marginals, const double *golden, int64_t ncases,
                 double *mse_sum, double *hd_sum);
/* Layout of the d_marginals buffer of fbn_jt_run_device: 0 = case-major [ncases][sum_dom] (default,
 * the reference's per-case vectors, GetProbabilitiesAllNodes src/JunctionTree.cpp:1385-1454),
 * 1 = variable-major [sum_dom][ncases] (value k of every case contiguous: a kernel store covers 64
 * consecutive cases, written once per cache line).  Same values either way; fbn_jt_run (host
 * buffers) always returns case-major. */
int fbn_jt_set_output_layout(fbn_jt_plan *p, int layout);
/* The per-case terms of fbn_jt_score on the device: d_terms[2 * c] = sqrt(e1 / num) (MSE) and
 * d_terms[2 * c + 1] = sqrt(e2 / num) (HD) of case c, computed exactly as fbn_jt_score computes
 * them (same operations, no contraction), from d_marginals in the plan's output layout and
 * d_golden [ncases][sum_dom] (case-major, as read from the golden file).  Summing the terms in case
 * order reproduces fbn_jt_score's sums bit for bit; asynchronous on hip_stream.  Replaces
 * Inference::CalculateMSE / CalculateHellingerDistance (src/Inference.cpp:153-206) for marginals
 * that stay on the device (the multi-GPU CLI: 16 bytes per case leave a rank instead of sum_dom * 8). */
int fbn_jt_score_terms_device(fbn_jt_plan *p, const double *d_marginals, const double *d_golden, int64_t ncases,
                              double *d_terms, void *hip_stream);
/* Device kernel time (ms, hipEvent) of the last fbn_jt_run*; launches of the main kernel. */
int fbn_jt_last_kernel_ms(const fbn_jt_plan *p, float *ms);
/* enable = 0: fbn_jt_run* records no timing events (two fewer stream markers per call; callers that
 * time with their own events); fbn_jt_last_kernel_ms then fails.  Default 1. */
int fbn_jt_set_kernel_timing(fbn_jt_plan *p, int enable);
/* Tuning: persistent waves per CU (0 = default: as many as keep the largest clique in LDS). */
int fbn_jt_set_waves_per_cu(fbn_jt_plan *p, int waves);
/* Kernel variant: -1 = auto (default: 3 when eligible and its code object loads, else 5 in the fast
 * order, else 4, else 0/1), 0 = clique-in-LDS interpreter, 1 = whole case state in a global
 * workspace interpreter, 2 = variant 0 with the IEEE division sequence forced (ablation / testing),
 * 3 = plan-specialized kernel (jt_gen_*.cpp; hiprtc or the on-disk code-object cache) followed
 *     by an exact-path fixup of the blocks it flags.  Selecting 3 fails if the plan is not eligible.
 * 4 = streamed ("virtual table") kernel for large trees (jt_virt.hip): tables recomputed per pass
 *     from initial potentials + received messages, only messages stored; exact-path fixup as 3.
 *     Selecting 4 fails for plans it cannot take (a clique with more than 6 children, ...).
 * 5 = tiled kernel (jt_tile.hip, the Munin-class default): 16 evidence cases x 4 entry slots per
 *     wave, every clique entry recomputed per pass from its initial potential and the messages,
 *     fast arithmetic order only (the exact setting does not apply); exact-path fixup as 3.  Fails
 *     for plans with > 6 children per clique, > 32 digit bits per clique or a domain > 8 states. */
int fbn_jt_set_variant(fbn_jt_plan *p, int variant);
/* Arithmetic order of the specialized (3) and streamed (4) kernels: 1 = exact (the reference's
 * sequential Normalize after every multiply: bit-identical marginals), 0 = fast (a clique's table is
 * its initial potential times its messages, normalized once where a result is formed -- the
 * reference's intermediate normalizations cancel: labels equal, marginals within 1e-12 relative,
 * inside north_star's 1e-6), -1 = auto (default: fast).  This is a parity-relevant default: a
 * caller that needs the reference's bits selects 1.  Replaces no reference interface (the reference
 * has one arithmetic order, src/JunctionTree.cpp:829-941). */
int fbn_jt_set_exact(fbn_jt_plan *p, int exact);
/* Diagnostics (LDS variant): enable per-op-type s_memtime accounting for subsequent runs and/or
 * read the totals of the last run (cycles[10], op types JT_L_INIT..JT_L_EVZERO, summed over waves). */
int fbn_jt_debug_op_cycles(fbn_jt_plan *p, int enable, unsigned long long *cycles);
/* Source of the plan-specialized kernel (variant 3); *len = bytes incl. NUL.  FBN_ERR_ARG if the
 * plan is not eligible (cliques too large for the register-resident form). */
int fbn_jt_kernel_source(const fbn_jt_plan *p, char *buf, int64_t cap, int64_t *len);
/* Testing: variant 3 marks every block for the exact fixup pass (exercises the fixup path). */
int fbn_jt_debug_force_fixup(fbn_jt_plan *p, int enable);
/* Testing: number of 64-case blocks the last run of variant 3 / 4 / 5 flagged for the exact fixup
 * (0 for other variants); synchronizes the device. */
int fbn_jt_debug_flagged_blocks(fbn_jt_plan *p, int64_t *count);
/* Path of the specialized kernel's code object in the on-disk cache (whether or not it exists);
 * a build step may compile fbn_jt_kernel_source() there with the options of fbn_jt_kernel_options. */
int fbn_jt_kernel_cache_path(const fbn_jt_plan *p, char *buf, int64_t cap);
/* Where the specialized kernel of the current order and layout keeps its stored messages, in rows
 * (one fp64 per lane): rows[0..5] = global Collect, global Distribute, LDS Collect, LDS Distribute,
 * register Collect, register Distribute; rows[6] = rows of the per-wave global workspace in use (a
 * separator's two messages share theirs), rows[7] = rows of the per-wave LDS pool (the most in use
 * at one time).  No device needed. */
int fbn_jt_kernel_placement(const fbn_jt_plan *p, int64_t *rows);
/* Compile the specialized kernel into the on-disk cache now (no device needed); FBN_OK if cached. */
int fbn_jt_kernel_build(const fbn_jt_plan *p);
/* Compile options of the specialized kernel, '\n'-separated. */
int fbn_jt_kernel_options(char *buf, int64_t cap);
/* The tiled kernel's program (variant 5, jt_program.h JtTPass): passes [n_passes] (33 int32 each),
 * index tables [n_tab], initial potentials [n_init]; geometry = {n_passes, n_tab, n_init,
 * partial-bin row, reduced-bin row, store rows, cases per wave, slots per case}.  Buffers may be
 * NULL (sizes only).  For tests that execute the tables on the host (tests/tile_emulator.py). */
int fbn_jt_tile_program(const fbn_jt_plan *p, int32_t *passes, int32_t *tab, double *initv, int64_t *geometry);
int fbn_jt_plan_destroy(fbn_jt_plan *p);

/* ------------------------------------------------------------------ CI tests (G^2) */
typedef struct fbn_ci_ctx fbn_ci_ctx;

/* Upload the column store (uint8 [nvars][nsamples], codes < dims[v] <= 255) to `device`. */
int fbn_ci_dataset_upload(const uint8_t *cols, int nvars, int64_t nsamples, const int32_t *dims,
                          int device, fbn_ci_ctx **out);
/* The same from a column store already in `device`'s memory (uint8 [nvars][nsamples]), e.g. filled
 * by one RCCL broadcast from the rank that loaded the file; copied into the handle.
 * Replaces every rank's own Dataset::LoadCSVData (src/Dataset.cpp:267-414) in a multi-GPU run.
 * Both entry points reject a code >= dims[v] (FBN_ERR_ARG). */
int fbn_ci_dataset_from_device(const uint8_t *d_cols, int nvars, int64_t nsamples, const int32_t *dims,
                               int device, fbn_ci_ctx **out);
/* Kernel-time accounting of a context (default on): HIP events around every CI kernel, summed into
 * fbn_ci_last_kernel_ms / fbn_pc_timing's kernel time.  Off: no events (≈30 µs less per ALARM-5000
 * PC-stable run; the reference's Timer measures wall time only), kernel times read 0. */
int fbn_ci_set_kernel_timing(fbn_ci_ctx *c, int enable);
/* n tests of one conditioning size d: items [n][2+d] = (x, y, z_0..z_{d-1}).  Outputs per test
 * (any may be NULL): G^2, adjusted df, p = 1 - pchisq(G^2, df), indep = (df == 0 || p > alpha).
 * ComputeGSquareXY / ComputeGSquareXYZ semantics (src/IndependenceTest.cpp:65-155,295-364).
 * Host arrays, synchronous. */
int fbn_ci_run(fbn_ci_ctx *c, const int32_t *items, int64_t n, int d, double alpha, double *g2,
               int32_t *df, double *p, uint8_t *indep, void *hip_stream);
/* Debug/parity: the contingency table N[z][x][y] of one test (int32, cells = dimz*dx*dy). */
int fbn_ci_counts(fbn_ci_ctx *c, int x, int y, const int32_t *z, int d, int32_t *counts, int64_t cap,
                  int64_t *cells);
int fbn_ci_last_kernel_ms(const fbn_ci_ctx *c, float *ms);
/* Parity pinning of the production paths: counts of n tests (items [n][2+d], level-0 pairs x < y)
 * through the kernels a PC run uses at level d -- d = 0 the complete-graph level-0 batch (Gram of
 * the leading bit-sliced rows, every pair's table recorded), d = 1 the derived counting from those
 * recorded pair tables, d >= 2 the histogram kernel (2-bit packed columns at >= 64k samples) over
 * one batch.  counts [n][cap], Counts3D cell order (src/CellTable.cpp:277-281). */
int fbn_ci_debug_counts(fbn_ci_ctx *c, const int32_t *items, int64_t n, int d, int32_t *counts, int64_t cap);
/* Which kernels the context's last level-0 all-pairs launch took (tests assert the path they mean
 * to check): out = {path, R, Rp, KS, nt, S, shortest slice, longest slice}.  path: 1 the popcount
 * Gram, 2 the FP4 MFMA Gram, 3 the tiled pairs kernel, 0 none yet (or none of the three).  R leading
 * rows (paths 1, 2); path 2: Rp = R padded to the 256-row tile, KS stages of 128 samples, nt tiles,
 * S split-K slices and the shortest / longest slice in stages (nt = S = 0: the range's x variables
 * have one state each, nothing was launched); path 1: nt = its 8 x 8 tile tasks.  Others 0. */
int fbn_ci_level0_info(const fbn_ci_ctx *c, int64_t out[8]);
/* The complete-graph pairs [pair0, pair0 + n) (lexicographic (x < y) order) launched as one batch of
 * a PC run's level-0 chunk loop; counts [n][16]: each pair's table, cells beyond it 0.  The level-0
 * Gram is poisoned (0xFF bytes) before the launch: an entry the Gram kernels did not write shows as
 * a wrong count, never as a stale right one.  The pair mode is restored on exit. */
int fbn_ci_debug_level0_range(fbn_ci_ctx *c, int64_t pair0, int64_t n, int32_t *counts);
/* Decision-margin log: the p-value CDF (stats::pchisq, src/IndependenceTest.cpp:146,
 * 268,355) is not pinned by any reference fixture, so every test records min |p - alpha| and counts
 * tests with |p - alpha| < 1e-9 (a decision a different-but-accurate CDF could flip).  Covers every
 * test run on `c` since the last reset (creation resets; `reset` != 0 resets after reading). */
int fbn_ci_decision_margin(fbn_ci_ctx *c, double *min_margin, int64_t *near_alpha, int reset);
int fbn_ci_ctx_destroy(fbn_ci_ctx *c);

/* ------------------------------------------------------------------ PC-stable skeleton */
typedef struct fbn_pc_result fbn_pc_result;

/* Skeleton phase of PC-stable (levels 0 .. depth-1, stop when FreeDegree <= level) with the
 * reference's sequential semantics: per edge the conditioning sets of adj(x)\{y} then adj(y)\{x}
 * in ChoiceGenerator order, first independent set wins, removals applied after each level.
 * group_size as the reference's -g.  CI tests run on the device in speculative batches; the
 * reported counts are the reference's (t = 1) counts. */
int fbn_pc_stable(fbn_ci_ctx *c, double alpha, int depth, int group_size, fbn_pc_result **out);
int fbn_pc_num_levels(const fbn_pc_result *r, int *n);
/* The run's decision-margin log (see fbn_ci_decision_margin): over every test of the skeleton phase. */
int fbn_pc_decision_margin(const fbn_pc_result *r, double *min_margin, int64_t *near_alpha);
int fbn_pc_level_tests(const fbn_pc_result *r, int64_t *tests /* [n_levels] */);
int fbn_pc_level_launched(const fbn_pc_result *r, int64_t *tests /* device tests incl. speculation */);
int fbn_pc_num_edges(const fbn_pc_result *r, int *n);
int fbn_pc_edges(const fbn_pc_result *r, int32_t *pairs /* [n][2], vec_edges order */);
/* sepsets flattened as (x, y, k, z_0..z_{k-1})*, key x < y; returns total int count in *len */
int fbn_pc_sepsets(const fbn_pc_result *r, int32_t *buf, int64_t cap, int64_t *len);
/* One skeleton level for the edge range [e_begin, e_end) of the current skeleton `edges`
 * ([nedges][2], x < y, lexicographic = the reference's vec_edges order): level 0 = one marginal test
 * per edge (src/PCStable.cpp:73-157), level d >= 1 = SearchAtDepth/CheckEdge over the adjacency
 * snapshot implied by `edges` (:209-551).  removed[e - e_begin] = 1 if the edge goes; sepsets
 * [(e_end - e_begin)][d] (or NULL) holds the removing set (sorted, -1 if kept); counted = tests the
 * reference would run, launched = device tests incl. speculation.  The unit a multi-GPU driver
 * partitions (fastbn_amd/pc_dist.py): ranges are independent within a level. */
int fbn_pc_level(fbn_ci_ctx *c, double alpha, int d, int group_size, const int32_t *edges, int64_t nedges,
                 int64_t e_begin, int64_t e_end, uint8_t *removed, int32_t *sepsets, int64_t *counted,
                 int64_t *launched);
/* Host-only: orient a given skeleton (pairs [nedges][2] in vec_edges order) with its sepsets
 * (records (x, y, m, z_0..z_{m-1}) as fbn_pc_sepsets writes them) into a new result. */
int fbn_pc_orient_skeleton(int nvars, const int32_t *pairs, int nedges, const int32_t *sepsets, int64_t len,
                           fbn_pc_result **out);
/* After the skeleton, fbn_pc_stable orients like StructLearnByPCStable steps 2-3
 * (OrientVStructure / OrientImplied, src/PCStable.cpp:576-843): triples [n][3] =
 * (from, to, 1) for arcs, (min, max, 0) for undirected edges, in the reference's vec_edges order. */
int fbn_pc_num_oriented_edges(const fbn_pc_result *r, int *n);
int fbn_pc_oriented_edges(const fbn_pc_result *r, int32_t *triples);
/* SHD against the CPDAG of the DAG in a BIF file (BNSLComparison::GetSHD, src/BNSLComparison.cpp:12-121,
 * true graph via CustomNetwork::LoadBIFFile, src/CustomNetwork.cpp:49-160). */
int fbn_pc_shd_bif(const fbn_pc_result *r, const char *bif_path, int *shd);
/* Same for any learned graph given as triples [n][3] (from, to, 1) / (a, b, 0). */
int fbn_shd_bif(const char *bif_path, int nvars, const int32_t *triples, int n, int *shd);
int fbn_pc_timing(const fbn_pc_result *r, double *total_s, double *kernel_s);
/* Which skeleton path ran: 0 host-driven levels, 1 the device-resident search (small graphs, one
 * launch: plain by default after an occupancy check, cooperative with FBN_PC_SMALL_COOP=1), 2 the
 * device-resident search was refused at launch or timed out at a grid
 * barrier and the host-driven levels ran instead (same answer), 3 host-driven levels whose level 0
 * -> level 1 hand-off ran on the device (the kept pairs became the level-1 edge list / adjacency
 * there; FBN_PC_HOST_L0L1=1 forces 0). */
int fbn_pc_path(const fbn_pc_result *r, int *path);
/* The result as one flat int32 record (for moving it between ranks): magic 0x52504246, n_levels,
 * n_levels (lo, hi) halves of the per-level test counts, n_edges, pairs [n_edges][2], then the
 * fbn_pc_sepsets ints preceded by their count.  *len = ints needed; FBN_ERR_LIMIT if cap is short. */
int fbn_pc_result_record(const fbn_pc_result *r, int32_t *buf, int64_t cap, int64_t *len);
/* 1 if fbn_pc_stable on this context runs the device-resident search (small graphs: <= 64 variables
 * of <= 4 states, group size 1): multi-GPU drivers run such graphs as replicas, not partitioned. */
int fbn_pc_small_eligible(const fbn_ci_ctx *c, int group_size, int *eligible);
/* The same rule from the dataset's shape (no context needed). */
int fbn_pc_small_eligible_shape(int nvars, int64_t nsamples, const int32_t *dims, int group_size, int *eligible);

/* ------------------------------------------------------------------ multi-GPU PC-stable session
 * One session per rank (one process per GPU); the per-level exchange is the caller's collective
 * (RCCL all-gather), everything per edge stays native (fastbn_amd/csrc/pc_dist.cpp).  Replaces the
 * level loop of PCStable::StructLearnByPCStable (src/PCStable.cpp:49-200) for a partitioned run:
 *   create -> { level(world, rank) -> run (or pack) -> [level 0: pairs_export / all-gather /
 *   pairs_import] -> all-gather the records -> apply } until apply reports no further level ->
 *   result (orientation included).  Every rank must apply the same records in rank order. */
typedef struct fbn_pc_dist fbn_pc_dist;
int fbn_pc_dist_create(int nvars, double alpha, int depth, int group_size, fbn_pc_dist **out);
/* Partition of the current level: d (-1 when finished), this rank's edge range [e_begin, e_end) of
 * the current skeleton (vec_edges order) and the int32 length of every rank's record. */
int fbn_pc_dist_level(fbn_pc_dist *s, int world, int rank, int *d, int64_t *e_begin, int64_t *e_end,
                      int64_t *record_len);
int fbn_pc_dist_num_edges(const fbn_pc_dist *s, int64_t *n);
int fbn_pc_dist_edges(const fbn_pc_dist *s, int32_t *pairs /* [n][2] */, int64_t cap);
/* This rank's range on the device of `c` (column store resident there) -> record [record_len]. */
int fbn_pc_dist_run(fbn_pc_dist *s, fbn_ci_ctx *c, int32_t *record);
/* A record from results computed elsewhere: removed [n], sepsets [n][d] (sorted; ignored where
 * not removed), counted / launched tests.  For engines other than the device (testing). */
int fbn_pc_dist_pack(fbn_pc_dist *s, const uint8_t *removed, const int32_t *sepsets, int64_t counted,
                     int64_t launched, int32_t *record);
/* Level 0 pair tables (16 int32 per pair) for the derived level-1 counting: after this rank's
 * level-0 run, export writes its chunk (pairs_chunk pairs, the tail zero-padded by the caller) to
 * buf; the caller all-gathers the chunks in rank order (pair index = offset / 16) and imports the
 * gathered buffer into its context.  buf in device (buf_on_device = 1) or host memory.
 * pairs_chunk = 0: this rank's level 0 recorded no pair tables (the bit-sliced path was not eligible
 * for the dataset, or FBN_CI_NO_PAIRS); the exchange is then skipped on every rank (eligibility
 * depends on the dataset only) and level 1 counts without them. */
int fbn_pc_dist_pairs_chunk(const fbn_pc_dist *s, int64_t *pairs_per_rank);
int fbn_pc_dist_pairs_export(fbn_pc_dist *s, void *buf, int buf_on_device);
int fbn_pc_dist_pairs_import(fbn_pc_dist *s, fbn_ci_ctx *c, const void *buf, int buf_on_device);
/* All ranks' records [world][record_len], rank order: sepsets, counts, removals; *more = 1 if
 * another level follows (depth and FreeDegree, src/PCStable.cpp:159-178). */
int fbn_pc_dist_apply(fbn_pc_dist *s, const int32_t *records, int *more);
/* After the last level: skeleton, sepsets, per-level counts (all ranks), this rank's kernel time /
 * decision margin, orientation (as fbn_pc_stable).  Lifetime: the fbn_ci_ctx passed to
 * fbn_pc_dist_run / _pairs_import must stay alive until the last fbn_pc_dist_apply (the one that
 * reports no further level), which snapshots its margin log and drops its pair tables; result never
 * touches it, so the ctx may be destroyed before this call. */
int fbn_pc_dist_result(fbn_pc_dist *s, fbn_pc_result **out);
int fbn_pc_dist_destroy(fbn_pc_dist *s);
/* Roofline accounting: bytes of column data the CI kernels had to read for every launched test,
 * in the format they read (uint8 columns: N per variable; bit-sliced masks: N/8 per value). */
int fbn_pc_device_bytes(const fbn_pc_result *r, int64_t *bytes);
int fbn_pc_result_destroy(fbn_pc_result *r);

/* ------------------------------------------------------------------ parameter learning
 * The step between structure learning and inference: the count maps of every node of a DAG from
 * the column store a context already holds.  Replaces ParameterLearning::LearnParamsKnowStructCompData
 * (src/ParameterLearning.cpp:11-64), which calls DiscreteNode::AddInstanceOfVarVal / AddCount
 * (src/DiscreteNode.cpp:100-145) once per node per sample.  A graph is given as CSR parent lists:
 * node v's parents are parents[parent_off[v] .. parent_off[v+1]) in any order; node v's family table
 * is int64 counts[value of v][parent configuration], configurations over the parents in ASCENDING
 * index order, last fastest -- fbn_network_create's layout -- family after family in one array.
 *
 * Cap: one call counts at most FBN_PARAM_MAX_CELLS = 2^26 cells in all (256 MiB of 32-bit device
 * accumulators, 512 MiB of int64 on the host); a family's cell count, or the sum, beyond that (or
 * overflowing on the way there) is FBN_ERR_LIMIT, never a wrapped number. */
#define FBN_PARAM_MAX_CELLS ((int64_t)1 << 26)

/* Host-only sizing and validation of the families (the table shapes DiscreteNode::InitializeCPT
 * enumerates, src/DiscreteNode.cpp:114-130): family_off[v] = first cell of node v's table,
 * family_off[nvars] = *ncounts = total cells.  FBN_ERR_ARG for a parent out of range, a self parent
 * or a repeated parent (and dims outside 1..256); FBN_ERR_LIMIT past the cap above. */
int fbn_param_family_sizes(int nvars, const int32_t *dims, const int32_t *parent_off, const int32_t *parents,
                           int64_t *family_off /* [nvars+1] or NULL */, int64_t *ncounts);
/* Family counts of every node from the column store resident in c (AddCount over all samples,
 * src/DiscreteNode.cpp:132-145; the sample loop of src/ParameterLearning.cpp:40-58): one launch for
 * all families.  counts [cap] int64 on the host in the layout above; *ncounts = cells written.
 * counts == NULL: sizes only.  cap < *ncounts: FBN_ERR_ARG.  The graph is validated on the host
 * before anything is launched (errors as fbn_param_family_sizes); acyclicity is not required and
 * any state count the context accepts is counted.  FBN_ERR_LIMIT for >= 2^31 samples (32-bit device
 * accumulators).  Synchronous on the context's own stream; the device table is the context's and is
 * zeroed by every call.  Kernel time (table zeroing + counting): fbn_ci_last_kernel_ms. */
int fbn_param_counts(fbn_ci_ctx *c, const int32_t *parent_off, const int32_t *parents,
                     int64_t *counts, int64_t cap, int64_t *ncounts);
/* fbn_param_counts + fbn_network_create's BuildNetwork: the learned network (GetProbability's
 * (count + 1) / (total + dims[v]), src/DiscreteNode.cpp:152-164, as every network here).  parents in
 * the node's own order.  Inherits fbn_network_create's limits (1..127 states, the parent lists form
 * a DAG) and error codes.  Replaces LearnParamsKnowStructCompData (src/ParameterLearning.cpp:11-64). */
int fbn_param_learn(fbn_ci_ctx *c, const int32_t *parent_off, const int32_t *parents,
                    const char *const *names, fbn_network **out);
/* 0 = default.  Sample-slice length and the largest table counted in LDS (at most 8192 cells; larger
 * values are clamped, a negative one sends every family to the global path): an explicit
 * tuning/testing API (not an environment variable), so tests reach both paths and multi-slice
 * merging at small N.  Replaces no reference interface. */
int fbn_param_set_tuning(fbn_ci_ctx *c, int64_t samples_per_slice, int64_t lds_cells_max);
/* Host-only: a consistent DAG extension of a PDAG (Dor & Tarsi 1992) -- the reference has no such
 * step: its StructLearnCompData leaves the CPDAG of src/PCStable.cpp:576-843 and its parameter
 * learner is only ever given a network file's DAG.  triples [n][3] as fbn_pc_oriented_edges writes
 * them: (from, to, 1) arcs, (a, b, 0) undirected edges.  Repeatedly the lowest-index remaining node
 * with no arc to a remaining node and whose undirected neighbours are each adjacent to all its other
 * remaining neighbours takes its undirected edges as incoming and is removed (deterministic).
 * parent_off [nvars+1], parents [n] ascending per node.  FBN_ERR_ARG naming the remaining nodes when
 * none qualifies (no extension, or a directed cycle), and for a duplicate / contradictory edge. */
int fbn_pdag_to_dag(int nvars, const int32_t *triples, int n, int32_t *parent_off, int32_t *parents /* cap n */);

/* ------------------------------------------------------------------ sampling engine
 * Forward (ancestral) sampling and the two sampling inference algorithms the reference's CLI
 * advertises but only answers "under development" for: probabilistic logic sampling (-a 4) and
 * likelihood weighting (-a 5), -q samples per case (src/main.cpp:97-121, include/Parameter.h:16-17,30).
 * A sampler needs only a topological order and the CPTs, so it runs where fbn_jt_plan_create refuses
 * (a disconnected moral graph, e.g. the network PC-stable learns from ALARM-5000).
 *
 * Random stream: numpy's PCG64(seed); the draw of the k-th variable in topological order (Kahn, LIFO
 * stack, children ascending -- fbn_synth_forward_sample's order) for sample i sits at stream position
 *   k * n + i                                  forward sampling (n = the call's sample count),
 *   i * V + k,  i = (case_offset + c) * S + s  inference (case c of the call, sample s of S, V variables),
 * every variable consuming its position whether or not its draw is used.  Under the inference map a
 * case's result depends on (seed, case_offset + c, S) only: a batch split over calls or devices with
 * case_offset gives the same bits.  Values by fbn_synth_forward_sample's rule (x = u * cdf[d - 1],
 * value = min(#{q : x >= cdf[q]}, d - 1)) on fp64 cdf rows of the parent configuration.
 *
 * Limits: at most 2048 variables (one wave keeps its 64 samples' values as bytes [V][64] in LDS)
 * and FBN_PARAM_MAX_CELLS table cells in all, else FBN_ERR_LIMIT; a cyclic network is FBN_ERR_ARG. */
typedef struct fbn_sampler fbn_sampler;
/* Flatten the network (order, parent lists in GIVEN order, fp64 probability and cdf tables built
 * with the (count + 1) / (total + |dom|) convention) and upload it to `device` once.  device < 0: a
 * host-only sampler that runs the same algorithm, chunk for chunk, on CPU threads (bit-identical
 * values, weights and sums); its *_device entries return FBN_ERR_NODEV. */
int fbn_sampler_create(const fbn_network *net, int device, fbn_sampler **out);
int fbn_sampler_destroy(fbn_sampler *s);
/* n complete cases, cols [V][n] uint8 (the column store layout), bit-identical to
 * fbn_synth_forward_sample(net, n, seed, cols).  Replaces the reference's wall-clock seeded
 * SampleSetGenerator (src/SampleSetGenerator.cpp) as the workload generator; the _device form writes
 * a device buffer (e.g. the input of fbn_ci_dataset_from_device) and is asynchronous on hip_stream. */
int fbn_sample_forward(fbn_sampler *s, int64_t n, uint64_t seed, uint8_t *cols);
int fbn_sample_forward_device(fbn_sampler *s, int64_t n, uint64_t seed, uint8_t *d_cols, void *hip_stream);
/* Sampling inference of ncases evidence cases with S >= 1 samples each (the reference's -q).
 * evidence [ncases][V] int8, -1 = unobserved, every code -1 or < the node's state count (checked
 * before anything indexes with it: FBN_ERR_ARG naming the first bad case / node).
 * method 0, likelihood weighting (-a 5): in topological order an observed variable takes its evidence
 *   value and multiplies P(v = ev | parents) into the sample's weight, kept as a scaled pair (m, e)
 *   from (1.0, 0): (m, de) = frexp(m * P), e += de -- exact power-of-two scaling, so hundreds of
 *   observed variables do not underflow and (m, e) is reproducible bit for bit.
 * method 1, probabilistic logic sampling (-a 4): every variable is sampled; m becomes 0 when an
 *   observed variable's sample differs from its evidence, e stays 0.
 * Per case, with emax = max_s e_s, w_s = ldexp(m_s, e_s - emax) and sumw = sum_s w_s:
 *   marginals [ncases][sum_dom] fp64 (or NULL) = sum_s w_s [x_v = q] / sumw, zeros for an observed
 *     variable (fbn_jt_run's convention);
 *   labels [ncases] = arg-max of variable 0's row (strict '>' from state 0, as fbn_jt_run);
 *   stats [ncases][2] fp64 (or NULL) = log_evidence = log(sumw / S) + emax ln 2, and the effective
 *     sample size sumw^2 / sum_s w_s^2.
 * A case no sample of which is accepted (sumw == 0, method 1 only) gets a row of zeros, label -1,
 * log_evidence -inf and ess 0, never a NaN.  All sums are taken in one fixed order (64-sample
 * chunks of one wave, no floating-point atomics): two runs, and any split by case_offset, agree
 * bitwise.  Replaces the PLS / LW stubs of src/main.cpp:97-121.  Host arrays, synchronous. */
int fbn_lw_run(fbn_sampler *s, int method, const int8_t *evidence, int64_t ncases, int64_t S, uint64_t seed,
               int64_t case_offset, int32_t *labels, double *marginals, double *stats);
/* The same with device-resident buffers; asynchronous on hip_stream after the evidence check (one
 * stream sync, as fbn_jt_run_device's).  d_marginals == NULL: labels (and stats) only. */
int fbn_lw_run_device(fbn_sampler *s, int method, const int8_t *d_evidence, int64_t ncases, int64_t S, uint64_t seed,
                      int64_t case_offset, int32_t *d_labels, double *d_marginals, double *d_stats, void *hip_stream);
/* Testing interface (an explicit API, not an environment variable): the samples behind fbn_lw_run
 * for a small batch (ncases * S <= 2^22): values [V][ncases * S] uint8, mantissas fp64 and
 * exponents int32 [ncases * S], sample s of case c at index c * S + s.  Host arrays.  Replaces no
 * reference interface. */
int fbn_lw_debug_samples(fbn_sampler *s, int method, const int8_t *evidence, int64_t ncases, int64_t S, uint64_t seed,
                         int64_t case_offset, uint8_t *values, double *mantissas, int32_t *exponents);
/* Device kernel time (ms, hipEvent) of the sampler's last launch. */
int fbn_sampler_last_kernel_ms(const fbn_sampler *s, float *ms);
/* fbn_jt_score's sums (CalculateMSE / CalculateHellingerDistance with Round(., 7),
 * src/Inference.cpp:153-206) from the network's state counts alone: no plan needed, so marginals of
 * a network no junction tree can be built for are scored the same way, bit for bit. */
int fbn_score_marginals(const fbn_network *net, const double *marginals, const double *golden, int64_t ncases,
                        double *mse_sum, double *hd_sum);

/* ------------------------------------------------------------------ loopy belief propagation
 * The reference's -a 7 (ALGLBP), which only prints "LBP is under development" (src/main.cpp:136-147);
 * `iters` is its propagation length, -d (Parameter::propagation_length, include/Parameter.h:33,
 * src/Parameter.cpp:40, default 2).  Sum-product message passing on the factor graph of the families:
 * EXACT on a forest / polytree once the iterations reach its diameter, an APPROXIMATION on a graph with
 * loops (no JT-like accuracy: see DESIGN.md 5.6 for measured errors).  It needs only the families and
 * their CPTs, so it runs where fbn_jt_plan_create refuses (a disconnected moral graph, a plan past
 * the JT kernels' limits), does not sample and does not depend on a seed.
 *
 * Factor graph: one factor per node f over (f, GIVEN parents in the node's own order) with the table
 * P[pc * d + q] ((count + 1) / (total + |dom|); pc over the GIVEN parents, last fastest).  Edges
 * (f, slot), f ascending, slot ascending (slot 0 = f), carry a factor -> variable message m and a
 * variable -> factor message mu of dom(x) doubles each; M = the sum of dom(x) over the edges.
 * Start: every entry 1.0 / d; an observed x = e sends mu = indicator of e throughout.
 * One iteration (flooding): (1) for every edge on an unobserved variable and every q,
 *   raw(q) = sum over the cells c with x_slot(c) = q, ascending c, from 0.0, of
 *            ((P[c] * mu_u1[x_u1(c)]) * mu_u2[..]) ... over the other slots u in ascending order,
 *   Z = sum_q raw(q) in ascending q, new = raw / Z, with damping != 0: (1.0 - damping) * new + damping * old;
 * (2) for every unobserved x, every edge (f, s) on it and every q, raw(q) = the product from 1.0 of
 *   m_g(q) over the other edges on x in ascending order, normalised the same way, undamped.
 * The residual of an iteration is max |new - old| over every entry written.  The run stops after
 * `iters` iterations or after the first whose residual is <= tol.  The belief of an unobserved x is the
 * product from 1.0 of m_g(q) over all its edges, divided by its sum in ascending q.
 *   marginals [ncases][sum_dom] fp64 (or NULL), zeros for an observed variable (fbn_jt_run's convention);
 *   labels [ncases] = arg-max of variable 0's row (strict '>' from state 0, as fbn_jt_run);
 *   stats [ncases][2] fp64 (or NULL) = iterations used, last residual.
 * A case in which some Z is 0 or not finite (underflow of a product over very many neighbours) gets
 * a row of zeros, label -1 and residual +inf, never a NaN; other cases are unaffected.
 * Only +, *, /, fabs and comparisons in the stated order: host twin and device agree bit for bit, as
 * do two runs and any split of a batch.
 * Limits: FBN_PARAM_MAX_CELLS table cells in all, else FBN_ERR_LIMIT; a cyclic network is FBN_ERR_ARG.
 * iters < 1, tol < 0 or NaN, damping outside [0, 1): FBN_ERR_ARG. */
typedef struct fbn_lbp fbn_lbp;
/* Flatten the network and upload it to `device` once.  device < 0: a host-only handle that runs the
 * same algorithm on CPU threads (bit-identical); its *_device entry returns FBN_ERR_NODEV. */
int fbn_lbp_create(const fbn_network *net, int device, fbn_lbp **out);
int fbn_lbp_destroy(fbn_lbp *s);
/* edges E, message doubles M, bytes one case's messages take in LDS, and the path the next run
 * takes: 0 = messages in LDS, 1 = in a per-workgroup global workspace (sized by the grid). */
int fbn_lbp_info(const fbn_lbp *s, int64_t *edges, int64_t *msg_doubles, int64_t *lds_bytes, int *path /*0 LDS, 1 global*/);
/* evidence [ncases][V] int8, -1 = unobserved, every code -1 or < the node's state count (checked
 * before anything indexes with it: FBN_ERR_ARG naming the first bad case / node).  Host arrays,
 * synchronous.  Replaces the LBP stub of src/main.cpp:136-147. */
int fbn_lbp_run(fbn_lbp *s, const int8_t *evidence, int64_t ncases, int iters, double tol, double damping,
                int32_t *labels, double *marginals /*or NULL*/, double *stats /*[ncases][2] or NULL*/);
/* The same with device-resident buffers; asynchronous on hip_stream after the evidence check (one
 * stream sync, as fbn_jt_run_device's).  d_marginals / d_stats may be NULL. */
int fbn_lbp_run_device(fbn_lbp *s, const int8_t *d_evidence, int64_t ncases, int iters, double tol, double damping,
                       int32_t *d_labels, double *d_marginals, double *d_stats, void *hip_stream);
/* Testing interface: both message arrays [ncases][2][M] (m, then mu) after exactly `iters`
 * iterations (no tolerance), ncases * 2 * M <= 2^24.  Host arrays.  Replaces no reference interface. */
int fbn_lbp_debug_messages(fbn_lbp *s, const int8_t *evidence, int64_t ncases, int iters, double damping, double *messages);
/* Kernel tuning (an explicit API, not an environment variable).  lds_bytes_max: the most LDS a case's
 * messages may take before they go to the global workspace; 0 = default (64 KiB, also the maximum),
 * < 0 forces the global path.  max_groups: cap of the persistent grid, 0 = default.  Results do not
 * depend on either. */
int fbn_lbp_set_tuning(fbn_lbp *s, int64_t lds_bytes_max, int max_groups);
/* Device kernel time (ms, hipEvent) of the handle's last launch. */
int fbn_lbp_last_kernel_ms(const fbn_lbp *s, float *ms);

/* ------------------------------------------------------------------ EPIS-BN
 * The reference's -a 6 (ALGEPISBN, include/Parameter.h:18; its propagation length -d is "for epis-bn
 * and lbp", :33), which only prints "EPIS-BN is under development" (src/main.cpp:123-134).  Evidence
 * Pre-propagation Importance Sampling (Yuan & Druzdzel 2003): loopy belief propagation first, then
 * importance sampling whose proposal for every unobserved variable is its CPT row times the lambda
 * message LBP left on it.  Unbiased like likelihood weighting for any lambda, deterministic given the
 * seed, and it runs on every network the sampler takes (disconnected ones included); where LBP is
 * exact (forests in which every node has at most one parent) every sample carries the same weight.
 *
 * Pre-propagation: per evidence case, fbn_lbp_run's algorithm exactly (flooding, `iters` iterations,
 * stop at tol, damping).  lambda of an unobserved x is the variable -> factor message mu on edge
 * (f = x, slot 0) as the run leaves it: the normalised product of the factor -> variable messages from
 * every family in which x is a parent.  iters == 0: no pre-propagation, lambda = 1.0 exactly (the
 * draws are then likelihood weighting's).  A case whose LBP run fails (some Z zero or not finite)
 * also gets lambda = 1.0 and residual +inf in its stats, never a NaN.
 * One draw: stream positions, topological order, parent configuration and the selection rule are
 * fbn_lw_run's inference map (i * V + k, i = (case_offset + c) * S + s; every variable consumes its
 * position).  An observed variable is clamped and weighed as in likelihood weighting,
 * (m, de) = frexp(m * P(ev | pa)), e += de.  An unobserved variable of d states with table row P[0..d)
 * and lambda[0..d):
 *   g(q) = P[q] * lambda[q];  Z = sum_q g(q), ascending from 0.0;
 *   Z zero or not finite: this draw uses g' = P (a likelihood-weighting draw, no cutoff);
 *   else with cutoff eps > 0: g'(q) = max(g(q), eps * Z); else g' = g;
 *   c(q) = the running sum of g', ascending from 0.0;  x = u * c(d - 1);
 *   value = min(#{q : x >= c(q)}, d - 1);
 *   (m, de) = frexp(m * ((P[value] * c(d - 1)) / g'(value))), e += de
 *   (a value with g' = 0, reachable only by x == c(d - 1) through rounding, gives m = 0).
 * Cutoff: eps in [0, 1); eps < 0 selects the defaults by state count after Yuan & Druzdzel: 0.006
 * below 5 states, 0.001 for 5 to 8, 0.0005 above.  Raise-and-renormalise as written above is this
 * library's rule; the paper describes replacing small probabilities by the threshold and subtracting
 * the excess from the largest entry, which differs in form (the weights keep either one unbiased).
 * Only +, *, /, frexp and comparisons in the stated order: host twin and device agree bit for bit.
 * Outputs per case as fbn_lw_run (marginals with zeros for observed variables, label by the same
 * arg-max, emax rescaling, no floating-point atomics, one fixed summation order); stats
 * [ncases][4] = log_evidence, ess, LBP iterations used, LBP residual (+inf where the case fell back to
 * lambda = 1; 0, 0 with iters == 0).
 * Limits and errors are the sampler's and LBP's: 2048 variables, FBN_PARAM_MAX_CELLS table cells
 * (FBN_ERR_LIMIT), a cyclic network FBN_ERR_ARG, evidence codes checked first (FBN_ERR_ARG naming the
 * first bad case / node); S < 1, iters < 0, tol < 0 or NaN, damping outside [0, 1), eps >= 1 or NaN:
 * FBN_ERR_ARG. */
typedef struct fbn_epis fbn_epis;
/* Flatten the network for the sampler and for LBP and upload both to `device` once.  device < 0: a
 * host-only handle that runs the same algorithm on CPU threads (bit-identical); its *_device entry
 * returns FBN_ERR_NODEV. */
int fbn_epis_create(const fbn_network *net, int device, fbn_epis **out);
int fbn_epis_destroy(fbn_epis *s);
/* Host arrays, synchronous.  marginals / stats may be NULL.  Replaces the EPIS-BN stub of
 * src/main.cpp:123-134. */
int fbn_epis_run(fbn_epis *s, const int8_t *evidence, int64_t ncases, int64_t S, uint64_t seed, int64_t case_offset,
                 int iters, double tol, double damping, double eps, int32_t *labels, double *marginals,
                 double *stats /*[ncases][4]*/);
/* The same with device-resident buffers: two launches (LBP, then sampling) on hip_stream,
 * asynchronous after the evidence check (one stream sync, as fbn_jt_run_device's).  d_marginals /
 * d_stats may be NULL. */
int fbn_epis_run_device(fbn_epis *s, const int8_t *d_evidence, int64_t ncases, int64_t S, uint64_t seed,
                        int64_t case_offset, int iters, double tol, double damping, double eps, int32_t *d_labels,
                        double *d_marginals, double *d_stats, void *hip_stream);
/* Testing interface: the samples behind fbn_epis_run for a small batch (ncases * S <= 2^22) as
 * fbn_lw_debug_samples gives them (values [V][ncases * S], mantissas, exponents [ncases * S]), and the
 * lambda rows [ncases][sum_dom] the draws used (an observed variable's row is the indicator LBP keeps
 * for it and is not read).  Host arrays.  Replaces no reference interface. */
int fbn_epis_debug_samples(fbn_epis *s, const int8_t *evidence, int64_t ncases, int64_t S, uint64_t seed,
                           int64_t case_offset, int iters, double tol, double damping, double eps, uint8_t *values,
                           double *mantissas, int32_t *exponents, double *lambda);
/* Kernel tuning (an explicit API, not an environment variable).  lds_bytes_max: the most LDS the
 * values (64 V bytes) and the case's lambda row (8 sum_dom bytes) may take together with the row in
 * LDS; beyond it the row is read from global memory.  0 = default (64 KiB, also the maximum), < 0
 * forces the global placement.  Results do not depend on it.  fbn_epis_info: those bytes and the
 * placement the next run takes. */
int fbn_epis_set_tuning(fbn_epis *s, int64_t lds_bytes_max);
int fbn_epis_info(const fbn_epis *s, int64_t *lds_bytes, int *path /*0 lambda in LDS, 1 global*/);
/* Device kernel times (ms, hipEvent) of the handle's last run: the LBP launch (0 with iters == 0)
 * and the sampling launch. */
int fbn_epis_last_kernel_ms(const fbn_epis *s, float *lbp_ms, float *sample_ms);

/* ------------------------------------------------------------------ adaptive importance sampling
 * The reference's -a 10 (ALGAISBN) and -a 8 (ALGSIS, include/Parameter.h:20-22), which only print
 * "AIS-BN is under development" / "SIS is under development" (src/main.cpp:175-186, :149-160); -m is its
 * maximum number of updates (default 10), -l its updating interval (default 2,500).  AIS-BN (Cheng & Druzdzel 2000, method 0) and
 * self-importance sampling (after Shachter & Peot 1989, method 1) learn, per evidence case, an
 * importance CPT (ICPT) from the weighted family counts of their own samples: no LBP launch, every DAG
 * the sampler takes (disconnected ones included), unbiased, deterministic given the seed.  -a 9
 * ("SISv1") is not built: the reference defines it nowhere.
 *
 * Parameters: method, S >= 1 counted samples, m in [0, 1024] maximum updates, l >= 1 interval, eps
 * (fbn_epis_run's cutoff convention: negative = the defaults by state count), seed, case_offset.
 * Stages, per case: nupd learning stages of l samples, each followed by an update, then one stage of
 * `last` samples; T = nupd * l + last draws.  AIS-BN: nupd = m, last = S, only the last stage enters the
 * estimate.  SIS: every sample is counted, T = S; an update follows each full block of l samples while
 * samples remain, at most m times: nupd = min(m, (S - 1) / l), last = S - nupd * l.  A stage of n samples is
 * ceil(n / 64) chunks of 64; the lanes past n in a last chunk sample in bounds with weight 0.
 * Stream: position i * V + k with i = (case_offset + c) * T + t, t the sample's index within the case
 * over all stages, k the variable's topological index (every variable consumes its position).  A
 * case's result depends on (seed, global case index, method, S, m, l, eps) only.
 * Learnable set, per case: the unobserved variables with an observed descendant (only ancestors of
 * evidence need an importance function other than their CPT).  Every other unobserved variable is
 * drawn as in fbn_lw_run (cdf row, no weight factor); observed variables are clamped and weighed as
 * there.  A learnable variable with table row P[0..d) and ICPT row I[0..d) is drawn by fbn_epis_run's
 * rule with g(q) = I[q] in place of P[q] * lambda[q]: Z ascending from 0.0; Z zero or not finite: a
 * likelihood-weighting draw; with cutoff g' = max(g, eps * Z); the running sum of g' selects the value;
 * the weight takes (P[value] * c(d - 1)) / g'(value), or 0.0 when g'(value) is 0.
 * ICPT: `cells` doubles indexed like the CPTs (topological node order, parent configurations over the
 * GIVEN parents last fastest, states); it starts as the CPTs at the start of every case.
 * Counts N, `cells` doubles: zeroed at the start of each stage (AIS-BN) or once per case (SIS,
 * cumulative).  After a chunk of a learning stage, with w_s = ldexp(m_s, e_s - emax), every learnable
 * node x adds N[toff + pc_s * d + x_s] += w_s over the chunk's samples in ascending order (the lanes
 * past n excluded).  emax runs over the stage (AIS-BN) or the case (SIS); when it grows, N is rescaled
 * by the exact power of two, as the weight sums are.  No floating-point atomics, one order.
 * Update k = 0 .. nupd - 1, after learning stage k, for every row (x, pc) of a learnable node:
 * t = sum_q N[q] ascending from 0.0; t > 0 and finite: I[q] <- I[q] + eta_k * (N[q] / t - I[q]); else the
 * row is left alone (a stage whose weights are all 0 included).  Rows are not renormalised.
 * eta_k: AIS-BN 0.4 * (0.14 / 0.4)^(k / m), the paper's schedule; SIS 1.  The host computes the table
 * (fbn_ais_eta) and the kernel reads it.
 * Support: AIS-BN keeps I > 0 wherever P > 0, so any eps >= 0 is unbiased; SIS relies on the cutoff's
 * floor, so method 1 with eps == 0 is FBN_ERR_ARG.
 * This library's rules, where the papers differ: the raise-and-renormalise cutoff stands in for the
 * paper's own theta cutoff; AIS-BN's "uniform parents of unlikely evidence" initialisation is not built
 * (it needs prior marginals); SIS's update replaces a row by the cumulative weighted frequencies.
 * Outputs per case as fbn_lw_run over the counted samples (labels, marginals with zeros for observed
 * variables); stats [ncases][4] = log_evidence, ess, updates applied (those whose weights were not
 * all 0), ess / n of the first stage (likelihood weighting's figure: the ICPT is still the CPTs).  A
 * case whose counted weights are all 0 gives zeros, label -1, -inf, 0 and no NaN.
 * Errors: the sampler's limits; method not 0 / 1, S < 1, m outside [0, 1024], l < 1, eps >= 1 or NaN,
 * method 1 with eps == 0, a stream position ((case_offset + ncases) * T + 64) * V at or past 2^63:
 * FBN_ERR_ARG.  Evidence codes are checked first, as everywhere. */
typedef struct fbn_ais fbn_ais;
/* Flatten the network and upload it to `device` once.  device < 0: a host-only handle that runs the
 * same algorithm on CPU threads (bit-identical); its *_device entry returns FBN_ERR_NODEV. */
int fbn_ais_create(const fbn_network *net, int device, fbn_ais **out);
int fbn_ais_destroy(fbn_ais *s);
/* Host arrays, synchronous.  marginals / stats may be NULL.  Replaces the AIS-BN (method 0) and SIS
 * (method 1) stubs of src/main.cpp:175-186 and :149-160. */
int fbn_ais_run(fbn_ais *s, int method, const int8_t *evidence, int64_t ncases, int64_t S, int64_t m, int64_t l,
                uint64_t seed, int64_t case_offset, double eps, int32_t *labels, double *marginals,
                double *stats /*[ncases][4]*/);
/* The same with device-resident buffers: one launch on hip_stream, asynchronous after the evidence
 * check (one stream sync, as fbn_jt_run_device's).  d_marginals / d_stats may be NULL.  Replaces the
 * same stubs. */
int fbn_ais_run_device(fbn_ais *s, int method, const int8_t *d_evidence, int64_t ncases, int64_t S, int64_t m, int64_t l,
                       uint64_t seed, int64_t case_offset, double eps, int32_t *d_labels, double *d_marginals,
                       double *d_stats, void *hip_stream);
/* Testing interface: all T draws per case behind fbn_ais_run for a small batch (ncases * T and
 * ncases * cells <= 2^22): values [V][ncases * T], mantissas and exponents [ncases * T] (draw t of case c
 * at c * T + t), and the ICPT after the last update [ncases][cells].  Host arrays.  Replaces no
 * reference interface. */
int fbn_ais_debug_samples(fbn_ais *s, int method, const int8_t *evidence, int64_t ncases, int64_t S, int64_t m,
                          int64_t l, uint64_t seed, int64_t case_offset, double eps, uint8_t *values, double *mantissas,
                          int32_t *exponents, double *icpt);
/* Kernel tuning (an explicit API, not an environment variable).  lds_bytes_max: the most LDS a
 * workgroup may take with the state (ICPT and counts, 16 * cells bytes) in LDS behind the values (64 V
 * bytes), the weights (512) and the flags (V, padded to 8); beyond it the state lives in the workgroup's
 * slice of a global workspace sized by the grid.  0 = default (64 KiB, also the maximum), < 0 forces
 * the global home.  max_workgroups: cap of the persistent grid, 0 = default.  Results do not depend on
 * either.  fbn_ais_info: those LDS bytes, the state's bytes, and the home (0 LDS, 1 global) and grid a
 * run of ncases cases takes next.  Replace no reference interface. */
int fbn_ais_set_tuning(fbn_ais *s, int64_t lds_bytes_max, int max_workgroups);
int fbn_ais_info(const fbn_ais *s, int64_t ncases, int64_t *lds_bytes, int64_t *state_bytes, int *path, int *grid);
/* Device kernel time (ms, hipEvent) of the handle's last launch. */
int fbn_ais_last_kernel_ms(const fbn_ais *s, float *ms);
/* eta[0 .. m) of a method, as the runs use it (for restatements that must not depend on pow). */
int fbn_ais_eta(int method, int m, double *eta);

/* ------------------------------------------------------------------ most probable explanation
 * MPE: the complete assignment x* = argmax_x P(x, e) that agrees with the evidence e, and P(x*, e).
 * Exact, by max-product message passing on the junction forest of fbn_jt_forest_plan_create (any DAG).
 * The reference has no counterpart (its algorithms stop at marginals; its -a ends at 11).  The per-variable
 * arg-maxes of the posterior marginals are a different thing and can form an assignment of probability 0.
 *
 * Plan: the forest plan -- cliques with initial potentials init_c (plain products of CPT entries; the
 * product over all cliques is the joint), separators, clique_up / clique_down, levels, one root per
 * component.  Evidence is applied by masking: a clique entry that disagrees with an observed variable is
 * skipped.  Every CPT entry is > 0 -- (count + 1) / (total + |dom|), or a probability network's finite
 * entry, which may be as small as a subnormal -- and init_c is formed as a plain fp64 product, so
 * fbn_mpe_create returns FBN_ERR_LIMIT, naming the clique and one of its nodes, when an init_c[e] is below
 * DBL_MIN (zero or subnormal: the product underflowed).  Normal potentials do not make every v(e) below
 * normal: a message is scaled by its row's largest entry alone, so v(e) = init_c[e] times message entries
 * that lie far below their rows' largest can underflow with ordinary tables -- a potential of 2^-921 and a
 * single message entry 2^-300 below its row's largest are enough (four children that each cost one value of
 * their parent 2^-300 or 2^-920, all observed).  When every unmasked v(e) of a clique is 0 the case's value
 * comes out as {0, 0} although P(x*, e) > 0 and {m, ex} could hold it: fbn_mpe_run and
 * fbn_mpe_debug_messages read every case's value and return FBN_ERR_LIMIT naming the first such case, never
 * FBN_OK with m == 0.  fbn_mpe_run_device is asynchronous and leaves that check to the caller (m of d_value).
 * A v(e) that underflows while a larger one of its clique does not is a loss of relative accuracy below
 * 2^-1022 of the clique's largest, as in any fp64 table.  No zero-probability branch exists beyond a guard.
 * Collect: cliques deepest level first, plan order within a level.  For clique c scan its entries
 *   e = 0 .. T-1 ascending, skipping masked ones:
 *     v(e) = (((init_c[e] * M^_1[map_1(e)]) * M^_2[map_2(e)]) ...) over the children in clique_down order;
 *   a non-root keeps msg[up(e)] = max(msg[up(e)], v(e)) from 0.0 (up: the entry's configuration of the
 *   upstream separator); then mx = max_s msg[s], frexp(mx) = f * 2^k with f in [0.5, 1), the stored message
 *   is M^_c[s] = ldexp(msg[s], -k) and the clique's integer exponent E_c = k + sum over children E_child.
 *   Only powers of two rescale: every mantissa equals the unscaled product's, and nothing underflows on a
 *   deep tree (the maximum is never divided by).
 * Root and value: a root r takes the first strict maximum of v(e) over its unmasked entries (ascending e,
 *   '>', from the first unmasked entry): e*_r and best_r = f_r * 2^(k_r), total exponent k_r + sum E_child.
 *   The case's value is the product over the roots in ascending component order from (m, ex) = (1.0, 0):
 *   m = m * f_r, re-frexp after each multiply, exponents added.  value[case] = {m, ex}, m in [0.5, 1), ex
 *   integral, P(x*, e) = m * 2^ex -- representable where P itself is far below 2^-1074.  No log is
 *   evaluated; a caller forms log P = log(m) + ex * log 2.
 * Back-trace: cliques levels ascending, plan order within a level.  A root assigns its variables from
 *   e*_r.  A clique c with parent p takes s* = map_{p->c}(e*_p), recomputes v(e) exactly as in Collect for
 *   its unmasked entries with up(e) == s* (after the plan's table reorganisation: e = s* mod Ts), takes
 *   the first strict maximum in ascending e and assigns its variables from it.  Observed variables keep
 *   their evidence code; every variable is in a clique, so the row is complete.
 * Only *, comparisons, frexp and ldexp: two runs, any split of a batch, any grid size and the host twin
 * give identical bytes, the assignment under exact ties included.
 * Limits: a clique of more than 32 variables, tables beyond int32 indexing, or one wave's store
 * (store_rows * 512 bytes) past the handle's budget: FBN_ERR_LIMIT at create.  A cyclic network: FBN_ERR_ARG. */
typedef struct fbn_mpe fbn_mpe;
/* Build the forest plan, compile the max-product program and upload it to `device`.  device < 0: a
 * host-only handle that runs the same algorithm on CPU threads (bit-identical); its *_device entry returns
 * FBN_ERR_NODEV. */
int fbn_mpe_create(const fbn_network *net, int device, fbn_mpe **out);
int fbn_mpe_destroy(fbn_mpe *s);
/* cliques, the sum of their entries, the rows of one case's store (separator entries + separators +
 * cliques; never a clique table) and the forest's components. */
int fbn_mpe_info(const fbn_mpe *s, int64_t *cliques, int64_t *entries, int64_t *store_rows, int *components);
/* evidence [ncases][V] int8, -1 = unobserved, every code -1 or < the node's state count (checked before
 * anything indexes with it: FBN_ERR_ARG naming the first bad case / node).  assignment [ncases][V] int8,
 * value [ncases][2] fp64 = {m, ex}.  Host arrays, synchronous. */
int fbn_mpe_run(fbn_mpe *s, const int8_t *evidence, int64_t ncases, int8_t *assignment, double *value);
/* The same with device-resident buffers; asynchronous on hip_stream after the evidence check (one stream
 * sync, as fbn_jt_run_device's). */
int fbn_mpe_run_device(fbn_mpe *s, const int8_t *d_evidence, int64_t ncases, int8_t *d_assignment, double *d_value,
                       void *hip_stream);
/* Testing interface: the stored messages M^ [ncases][sum of separator entries] (separators in plan order)
 * and the exponents E of each separator's child clique [ncases][separators], as Collect leaves them;
 * at most 2^26 doubles.  Host arrays. */
int fbn_mpe_debug_messages(fbn_mpe *s, const int8_t *evidence, int64_t ncases, double *messages, int32_t *exponents);
/* Kernel tuning (an explicit API, not an environment variable).  max_workgroups: cap of the persistent
 * grid, 0 = default.  store_bytes_max: the budget of the message store, all waves together (0 = default,
 * 32 GiB, and never more than half of the free device memory); the grid shrinks to fit it, and a budget one wave's store does not fit is FBN_ERR_LIMIT (the
 * handle keeps its setting).  Results never depend on either. */
int fbn_mpe_set_tuning(fbn_mpe *s, int max_workgroups, int64_t store_bytes_max);
/* Device kernel time (ms, hipEvent) of the handle's last launch. */
int fbn_mpe_last_kernel_ms(const fbn_mpe *s, float *ms);

/* ------------------------------------------------------------------ expectation-maximisation
 * EM: the CPTs of a network of known structure from data with missing cells (a hidden variable is a column
 * of missing cells).  The reference has no counterpart: ParameterLearning.cpp assumes complete data.
 *
 * Data: int8 [ncases][V], -1 = missing, otherwise a state code -- the evidence format, validated as
 * fbn_mpe_run validates.  Plan: the forest plan of fbn_jt_forest_plan_create (any DAG); a data row is
 * applied as evidence by masking, as in MPE.  theta: the current parameters, fp64 [cells] in
 * fbn_param_counts' layout ([value][config of the ascending parents, last fastest], family after family,
 * offsets of fbn_param_family_sizes).  Every theta > 0, but init_c is a plain fp64 product of thetas and a
 * probability network's may be tiny: fbn_em_create and fbn_em_set_parameters return FBN_ERR_LIMIT, naming
 * the clique and one of its nodes, when an init_c[e] is below DBL_MIN (zero or subnormal), and
 * fbn_em_set_parameters then leaves the handle as it was.  A row's P(e) can still leave the range inside a
 * clique, with ordinary tables (as stated above fbn_mpe_create: normal potentials times message entries far
 * below their rows' largest): when every unmasked v(e) of a clique is 0 its value has m == 0 and its
 * posteriors are NaN.  fbn_em_estep, fbn_em_debug_posteriors and fbn_em_run read every case's value and
 * return FBN_ERR_LIMIT naming the first such case instead of FBN_OK; fbn_em_estep_device is asynchronous
 * and leaves that check to the caller (m of d_value).
 * Collect (sum-product): cliques deepest level first, plan order within a level.  For an unmasked entry
 *     v(e) = (((init_c[e] * M_1[map_1(e)]) * M_2[map_2(e)]) ...) over the children in clique_down order.
 *   A non-root keeps msg[s] = sum of v(e) over its unmasked entries with up(e) = s, in ascending e, from
 *   0.0; then mx = max_s msg[s], frexp(mx) = f * 2^k, the stored message is M_c[s] = ldexp(msg[s], -k) and
 *   the clique's integer exponent is E_c = k + sum over children E_child.  Only powers of two rescale.
 *   A root sums its unmasked v(e) in ascending e from 0.0: sum_r = f_r * 2^(k_r), total exponent
 *   k_r + sum E_child.  The case's evidence probability is the product over the roots in ascending
 *   component order from (m, ex) = (1.0, 0): m = m * f_r, re-frexp after each multiply, exponents added.
 *   value[case] = {m, ex}, m in [0.5, 1), P(e) = m * 2^ex.  No log is taken here.
 * Distribute: cliques levels ascending, plan order within a level.  For clique c with parent p the
 *   downward message on c's upstream separator is D_c[s] = sum over p's unmasked entries e with
 *   map_{p->c}(e) = s, in ascending e from 0.0, of
 *     t(e) = ((init_p[e] * M_j[map_j(e)]) ... over p's children j != c in clique_down order) * D_p[up_p(e)],
 *   the last factor only where p is not a root (for a root D_p = 1).  Then mx = max_s D_c[s], frexp(mx) gives
 *   k and the stored message is ldexp(D_c[s], -k); its exponent is not kept (a belief is normalised by its
 *   own clique's sum).  The message is division-free: nothing is ever divided by a message.
 * Family posteriors: node v's family {v} + parents is hosted by the first clique in plan order that
 *   contains it.  For a hosting clique the belief of an unmasked entry is b(e) = v(e) * D_c[up(e)] (b = v for
 *   a root), Z_c = the sum of b(e) in ascending e from 0.0, and the posterior of family cell f is the sum of
 *   b(e) / Z_c over the unmasked entries that map to f, in ascending e from 0.0: a true division by the
 *   clique's own sum, so a fully observed row contributes exactly 1.0 to one cell per family, and a cell the
 *   row rules out gets exactly 0.0.
 * E-step output: N[cell] = the sum over the cases of the posterior (fp64); value [ncases][2].  The host
 *   twin adds the cases in order.  The device adds the 64 cases of a block (cases 64 b .. 64 b + 63) in
 *   butterfly order (lane i adds lane i ^ off, off = 32 .. 1), then the blocks of a wave in order (blocks w,
 *   w + g, ... for wave w of g), then the waves in wave order: no atomics, so two runs with the same inputs
 *   and the same grid give identical bytes, while the counts of two grid sizes, and of the twin, may differ
 *   by the rounding of a sum of n non-negative terms (relative n * 2^-53).  Per-case posteriors and values are
 *   the twin's bytes at every grid size.
 * M-step: theta_v[q | pc] = (N[q, pc] + alpha) / (T[pc] + alpha * dims[v]), T[pc] = the sum of N[q, pc] in
 *   ascending q from 0.0.  alpha > 0 is the pseudo-count (1.0 is the project's own (count + 1) / (total + |dom|)).
 * Potentials of the next iteration: init_c[e] = ((1.0 * theta_a[..]) * theta_b[..]) ... over the families the
 *   clique hosts in ascending node order -- with theta a network's own CPTs, the plan's potentials to the byte.
 * Objective of iteration t, at the parameters its E-step ran with: log-likelihood L_t = the sum in case
 *   order of log(m) + ex * log(2), formed on the host; Q_t = L_t + alpha * (the sum over the cells in order of
 *   log theta[cell]).  EM with this M-step never decreases Q.
 * Stopping: an iteration is E-step, objective, M-step.  After max_iters iterations; or after the iteration
 *   t >= 1 with Q_t - Q_(t-1) <= tol * |Q_t| (its M-step is still taken).  tol = 0 never stops early.
 * Limits: as MPE's (a clique of more than 32 variables, tables beyond int32 indexing, one wave's state --
 *   store_rows * 512 + cells * 8 bytes -- past the handle's budget), or more than FBN_PARAM_MAX_CELLS cells:
 *   FBN_ERR_LIMIT at create.  A cyclic network: FBN_ERR_ARG. */
typedef struct fbn_em fbn_em;
/* `start` gives the structure and the starting parameters (its Prob: a count network's smoothed CPTs, or a
 * probability network's entries).  device < 0: a host-only handle running the host twin. */
int fbn_em_create(const fbn_network *start, int device, fbn_em **out);
int fbn_em_destroy(fbn_em *s);
/* cliques, the sum of their entries, the rows of one case's store (2 * separator entries + separators),
 * the family cells (a wave also owns an accumulator of one fp64 per cell) and the forest's components. */
int fbn_em_info(const fbn_em *s, int64_t *cliques, int64_t *entries, int64_t *store_rows, int64_t *cells,
                int *components);
/* One E-step at the current parameters.  Host arrays, synchronous; a bad code is FBN_ERR_ARG naming the
 * case and node. */
int fbn_em_estep(fbn_em *s, const int8_t *data, int64_t ncases, double *counts /* [cells] */,
                 double *value /* [ncases][2] or NULL */);
/* The same with device-resident buffers; asynchronous on hip_stream after the data check (one stream sync). */
int fbn_em_estep_device(fbn_em *s, const int8_t *d_data, int64_t ncases, double *d_counts, double *d_value,
                        void *hip_stream);
/* The loop, on the device for a device handle: the data is uploaded once; an iteration launches the E-step,
 * the cross-wave reduction and one kernel for the M-step and the potential rebuild; the per-case values
 * and theta (for the objective's logs) are all that comes back.  objective [max_iters][2] = {L_t, Q_t} for
 * the iterations done.  pseudo_count <= 0, max_iters < 1 or tol < 0: FBN_ERR_ARG.  Leaves the theta, byte for
 * byte, of a caller chaining fbn_em_estep, the stated M-step and fbn_em_set_parameters.
 * Range: after every M-step the host rebuilds the initial potentials from the theta that came back (the
 * products the device formed) and checks them as fbn_em_set_parameters does; before every objective it
 * checks the per-case values for m == 0.  Either failure is FBN_ERR_LIMIT: the handle keeps the last theta
 * that passed (the one before the refused M-step), *iters_done counts the M-steps kept, and no count, theta
 * or value of the refused step is reported. */
int fbn_em_run(fbn_em *s, const int8_t *data, int64_t ncases, int max_iters, double tol, double pseudo_count,
               double *objective, int *iters_done);
/* theta = net's probabilities; net must have the handle's structure (states, parent sets), else FBN_ERR_ARG. */
int fbn_em_set_parameters(fbn_em *s, const fbn_network *net);
/* The current theta as a probability network (fbn_network_create_cpt). */
int fbn_em_network(const fbn_em *s, fbn_network **out);
/* Testing interface: the per-case family posteriors [ncases][cells]; at most 2^26 doubles.  Host arrays. */
int fbn_em_debug_posteriors(fbn_em *s, const int8_t *data, int64_t ncases, double *post);
/* Kernel tuning, as fbn_mpe_set_tuning.  Per-case results never depend on either; the summed counts depend
 * on the grid within the rounding stated above. */
int fbn_em_set_tuning(fbn_em *s, int max_workgroups, int64_t store_bytes_max);
/* Device time (ms, hipEvent) of the handle's last E-step kernel. */
int fbn_em_last_kernel_ms(const fbn_em *s, float *ms);

/* ------------------------------------------------------------------ score-based structure learning
 * Greedy hill climbing over arc additions, deletions and reversals under a decomposable score (-a 14).
 * The reference learns structure by constraint tests only, so there is no reference output to match: the
 * device path is held bit for bit to a host twin in this library (fbn_hc_run_host, fbn_score_families_host).
 *
 * Score of a family (child v with r states, parents P with q joint configurations, counts N_jk in
 * fbn_param_counts' layout):  loglik = sum_jk L[N_jk] - sum_j L[N_j],  score = loglik - penalty (r - 1) q,
 * L[n] = n ln n.  L is a table of N + 1 doubles filled once on the host with the C library's log; both
 * sides gather from it and add in one fixed order (hc_score.h), so a family's score is a pure function of
 * (child, parent set, data): never of the batch, the chunk, the slices or the counting path.
 * The table costs 8 (N + 1) bytes: more than 2^24 samples is FBN_ERR_LIMIT. */
/* Host-only: the bytes of the score table of N samples; FBN_ERR_LIMIT past 2^24 samples, FBN_ERR_ARG for N < 1. */
int fbn_hc_table_bytes(int64_t nsamples, int64_t *bytes);
/* Host-only: the penalty of a named score for N samples: "bic" ln(N) / 2, "aic" 1, "loglik" 0; else FBN_ERR_ARG. */
int fbn_hc_penalty(const char *score, int64_t nsamples, double *penalty);
/* Scores of arbitrary families from the context's resident column store.  Family f is the columns
 * fam_cols[fam_off[f] .. fam_off[f+1]): the child first, then its parents in any order; fam_off[0] = 0.
 * loglik / score [nfam] doubles on the host (either may be NULL).  Validated on the host before any launch,
 * as fbn_param_family_sizes validates: FBN_ERR_ARG for an empty family, a column out of range, a self or
 * repeated parent, a negative or NaN penalty; FBN_ERR_LIMIT for a family above FBN_PARAM_MAX_CELLS.  A batch
 * whose tables exceed FBN_PARAM_MAX_CELLS in all is counted and reduced in chunks.  Counting is
 * fbn_param_counts' kernel under fbn_param_set_tuning; only 16 bytes per family return to the host.  Kernel
 * time (zeroing + counting + reduction, summed over the chunks): fbn_ci_last_kernel_ms. */
int fbn_score_families(fbn_ci_ctx *c, double penalty, int64_t nfam, const int64_t *fam_off, const int32_t *fam_cols,
                       double *loglik, double *score);
/* The host twin of fbn_score_families over a host column store (uint8 [nvars][nsamples]): same validation,
 * same values bit for bit.  No device. */
int fbn_score_families_host(int nvars, const int32_t *dims, const uint8_t *cols, int64_t nsamples, double penalty,
                            int64_t nfam, const int64_t *fam_off, const int32_t *fam_cols, double *loglik,
                            double *score);
/* 0 = default (FBN_PARAM_MAX_CELLS).  The most table cells counted per chunk of a batch (a larger family
 * sits alone in its chunk): a tuning/testing entry, so tests reach multi-chunk batches at small sizes. */
int fbn_hc_set_tuning(fbn_ci_ctx *c, int64_t chunk_cells_max);

typedef struct fbn_hc_options {
    double penalty;            /* >= 0 (fbn_hc_penalty); negative or NaN: FBN_ERR_ARG */
    int32_t max_parents;       /* most parents a node may be GIVEN; < 0: no limit */
    int32_t max_iter;          /* most operations applied; < 0: no limit */
    int64_t max_family_cells;  /* an operation whose new table would exceed it is inadmissible, never an
                                  error; <= 0 or above FBN_PARAM_MAX_CELLS: FBN_PARAM_MAX_CELLS */
    const uint8_t *allowed;    /* [nvars][nvars]: allowed[x * nvars + y] != 0 lets the search add x -> y
                                  (also by a reversal); NULL: every arc */
    int64_t allowed_len;       /* nvars * nvars when allowed != NULL, else FBN_ERR_ARG */
    const int32_t *start_off;  /* the starting DAG as CSR parent lists (fbn_param_counts' form); NULL: empty. */
    const int32_t *start_parents; /* A cyclic start is FBN_ERR_ARG; its arcs need not satisfy the limits above */
} fbn_hc_options;

typedef struct fbn_hc_info {
    int32_t nvars, narcs, iterations, pad;
    int64_t families_scored;   /* families handed to the scorer, over all batches */
    int64_t batches;           /* scorer calls: the first sweep, then one per operation */
    double score, loglik;      /* sums of the per-node values in node order */
    double kernel_ms;          /* device time of all batches (0 on the host twin) */
    double first_sweep_kernel_ms, first_sweep_wall_ms; /* the first batch: device time, host wall time */
    double score_wall_ms, wall_ms; /* wall time inside the scorer over all batches; of the whole search */
} fbn_hc_info;

typedef struct fbn_hc_result fbn_hc_result;

/* Hill climbing from options->start.  Every step applies the legal operation with the largest score delta,
 * provided it is > 0: add x -> y, delete x -> y, or reverse x -> y (delta = the delete delta in y's row plus
 * the add delta in x's row).  Legal: no directed cycle, max_parents, max_family_cells, allowed.  Exact ties
 * go to the lowest (type: add 0 < delete 1 < reverse 2, then the arc's head y, then its tail x; a reversal is
 * keyed by the arc it removes).  After a step only the rows of the nodes whose parent set changed are
 * rescored (one row, or two after a reversal), in one batch; the first sweep is one batch.  Stops when nothing improves, or at max_iter. */
int fbn_hc_run(fbn_ci_ctx *c, const fbn_hc_options *options, fbn_hc_result **out);
/* The same search over the host scorer (fbn_score_families_host): the host twin.  No device. */
int fbn_hc_run_host(int nvars, const int32_t *dims, const uint8_t *cols, int64_t nsamples,
                    const fbn_hc_options *options, fbn_hc_result **out);
int fbn_hc_result_info(const fbn_hc_result *r, fbn_hc_info *info);
/* parent_off [nvars+1], parents [narcs] ascending per node */
int fbn_hc_result_parents(const fbn_hc_result *r, int32_t *parent_off, int32_t *parents);
/* per-node family scores and log-likelihoods [nvars] (either may be NULL) */
int fbn_hc_result_node_scores(const fbn_hc_result *r, double *score, double *loglik);
/* the operation trace: ops [iterations][3] = (type, from, to) of the arc x -> y added, deleted or reversed
 * (from = x, to = y: the arc as it stood before a reversal), delta [iterations] */
int fbn_hc_result_trace(const fbn_hc_result *r, int32_t *ops, double *delta);
int fbn_hc_result_destroy(fbn_hc_result *r);

#ifdef __cplusplus
}
#endif

#endif /* FASTBN_H */
