// jt_em_program.h -- the expectation-maximisation program over the junction forest: compiled on the
// host from the forest plan (jt_em_plan.cpp), executed per data row by the host twin (jt_em_host.cpp)
// and by every lane of jt_em.hip.  Shared by host and device; plain C layout.  The algorithm is stated
// in include/fastbn.h above fbn_em_create.
//
// The sum-product program extends the max-product one (jt_mpe_program.h: cliques, maps, digit words,
// Collect and level orders are the same tables) by, per clique, the families it hosts and the two
// kinds of ascending lists that let every running sum live in a register: the parent's entries grouped
// by the entry of the separator they map to (the downward message), and the clique's own entries
// grouped by family cell (the posteriors).  Within a group the entries ascend, so a group's sum is
// the stated ascending-e sum restricted to it.
//
// State of one case ("the store", rows of one fp64 / int64 per case):
//   message rows   one per separator entry: the Collect message of the separator's child clique
//   exponent rows  one per separator: E of its child clique (an integer)
//   down rows      one per separator entry: the Distribute message D of the separator's child clique
// Clique tables are never stored: v(e) is recomputed wherever it is needed.  Beside its store a wave owns
// an accumulator of one fp64 per family cell (the posteriors summed over its cases).
#ifndef FBN_JT_EM_PROGRAM_H
#define FBN_JT_EM_PROGRAM_H

#include <stdint.h>

#include "jt_mpe_program.h"

struct JtEClique {
    int32_t nfam;       // families this clique hosts
    int32_t fam_off;    // eaux: nfam records {node, first cell, cells, cellmap_off (T int32: entry ->
                        //       cell of all families), group_off (T int32: entries by (cell, entry))}
    int32_t slot;       // this clique's index among its parent's children (clique_down order)
    int32_t pgroup_off; // eaux: the parent's entries by (entry of this clique's upstream separator, entry)
};
constexpr int kEmFamRec = 5;

// what fbn_em_estep_launch takes (launchers.h), filled by name in capi_em.hip
struct JtEmArgs {
    const JtMClique *cl;
    const JtEClique *ecl;
    const int32_t *aux, *eaux;
    const double *initv;
    const uint64_t *dig;
    const int32_t *collect;  // clique ids: deepest level first, plan order within a level
    const int32_t *trace;    // clique ids: levels ascending, plan order within a level
    const int8_t *data;      // [ncases][V]
    double *value;           // [ncases][2] or NULL
    double *dbg_post;        // testing (or NULL): [ncases][cells]
    double *store;           // [grid][store_rows][64]
    double *wacc;            // [grid][cells]: the waves' accumulators, zero at launch
    long long ncases;
    long long store_rows;
    int nc, V, msg_rows, nsep, cells;  // exponent rows at msg_rows, down rows at msg_rows + nsep
    int grid;
    int lds_acc;             // != 0: a wave accumulates in cells * 8 bytes of LDS and writes wacc when it retires
};
// the cross-wave reduction: counts[cell] from the accumulators of a->grid waves, in wave order
struct JtEmReduceArgs {
    const double *wacc;
    double *counts;
    int cells, grid;
};
// the M-step and the rebuild of the initial potentials, one launch
struct JtEmMstepArgs {
    const double *counts;
    double *theta;               // [cells]
    double *initv;               // [entries]
    const int32_t *cell_node;    // [cells]
    const int32_t *node_rec;     // [V] {first cell, parent configurations, states}
    const int32_t *entry_clique; // [entries]
    const JtMClique *cl;
    const JtEClique *ecl;
    const int32_t *eaux;
    double alpha;
    int cells, entries;
};

#include <vector>

namespace fbn {

struct JTPlanHost;
struct Network;

struct JTProgramEm {
    JTProgramMpe M;
    std::vector<JtEClique> ecl;
    std::vector<int32_t> eaux;
    std::vector<int32_t> cell_node, node_rec, entry_clique;
    std::vector<double> theta;  // [cells], fbn_param_counts' layout
    int64_t cells = 0;
    int64_t store_rows = 0;     // 2 * msg_rows + separators
};
// FBN_ERR_LIMIT as CompileJTProgramMpe's, and past FBN_PARAM_MAX_CELLS cells; theta = the network's CPTs
int CompileJTProgramEm(const Network &net, const JTPlanHost &plan, JTProgramEm &prog);
// theta[cell] = net.Prob(...) for a network of the program's structure, else FBN_ERR_ARG
int EmThetaFromNetwork(const JTProgramEm &P, const Network &structure, const Network &net, std::vector<double> &theta);
// init_c[e] = ((1.0 * theta_a[..]) * theta_b[..]) ... over the families the clique hosts, ascending node
void EmRebuildPotentials(const JTProgramEm &P, const double *theta, double *initv);
// CheckCliquePotential over rebuilt potentials: FBN_ERR_LIMIT for an entry below DBL_MIN
int EmCheckPotentials(const JTProgramEm &P, const double *initv);
// theta from counts: (N + alpha) / (T + alpha * states), T the sum over the states in ascending order
void EmMstep(const JTProgramEm &P, const double *counts, double alpha, double *theta);
// The host twin of the E-step: counts [cells] (or NULL) summed in case order, value [ncases][2] (or
// NULL), post [ncases][cells] (or NULL).  Cases spread over HostThreads() threads for value / post;
// the counts are then added in case order.
int HostEmEstep(const JTProgramEm &P, const int8_t *data, int64_t ncases, double *counts, double *value, double *post);

}  // namespace fbn

#endif
