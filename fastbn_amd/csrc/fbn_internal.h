// fbn_internal.h -- internal types of libfastbn (host side).  Not part of the ABI.
#ifndef FBN_INTERNAL_H
#define FBN_INTERNAL_H

#include <cstdint>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../include/fastbn.h"
#include "jt_program.h"
#include "knobs.h"

namespace fbn {

// thread-local error channel behind fbn_last_error()
int SetError(int code, const char *fmt, ...);
const char *LastError();

// ---------------------------------------------------------------------------------------------
// discrete Bayesian network (CustomNetwork + DiscreteNode state the hot paths read)
struct Network {
    std::vector<std::string> names;
    std::vector<int> dom;
    std::vector<std::vector<int>> given;        // parents in <GIVEN> order
    std::vector<std::vector<int>> parents_asc;  // parents in ascending index order
    std::vector<std::vector<int64_t>> counts;   // [v][q * npc + pc]
    std::vector<std::vector<int64_t>> totals;   // [v][pc], pc over parents_asc, last fastest
    std::vector<std::vector<double>> cpt;       // a probability network (else empty): [v][q * npc + pc]
    int n() const { return (int)dom.size(); }
    double Prob(int v, int q, const int *parent_vals_asc) const;
};
int LoadXmlbif(const std::string &path, Network &net);
int BuildNetwork(int n, const int32_t *dims, const int32_t *parent_off, const int32_t *parents, const int64_t *counts,
                 const char *const *names, Network &net);
int NodeCounts(const Network &net, int v, int32_t *parents_asc, int64_t *counts, int *nparents, int64_t *ncounts);
// a network that holds probabilities (BuildNetwork's validation; every entry finite and > 0, every
// column summing to 1 within 1e-9), and node v's table as Prob returns it, for either kind of network
int BuildNetworkCpt(int n, const int32_t *dims, const int32_t *parent_off, const int32_t *parents, const double *cpt,
                    const char *const *names, Network &net);
int NodeProbs(const Network &net, int v, int32_t *parents_asc, double *probs, int *nparents, int64_t *nprobs);

// parameter learning, host side (param_learn.cpp): family sizing / validation and the PDAG -> DAG
// extension behind fbn_param_family_sizes / fbn_pdag_to_dag (no device, no other part of the library)
int ParamFamilySizes(int nvars, const int32_t *dims, const int32_t *parent_off, const int32_t *parents,
                     int64_t *family_off, int64_t *ncounts);
int PdagToDag(int nvars, const int32_t *triples, int n, int32_t *parent_off, int32_t *parents);

struct Dataset {
    int nvars = 0;
    int64_t nsamples = 0;
    std::vector<std::string> names;
    std::vector<int32_t> dims;
    std::vector<uint8_t> cols;  // [var][sample]
};
int LoadCsv(const std::string &path, Dataset &ds);
// ev == nullptr: only *nrows; otherwise the first min(rows, cap) rows into ev [row][num_nodes] / labels
int LoadLibsvm(const std::string &path, int num_nodes, int8_t *ev, int32_t *labels, int64_t cap, int64_t *nrows);

// seeded generators (synth.cpp): numpy-PCG64-identical forward sampling and evidence cases, and
// writers of the reference's text formats
int ForwardSample(const Network &net, int64_t n, uint64_t seed, uint8_t *cols);
int EvidenceCases(const Network &net, int64_t n, int k, uint64_t seed, int query, int8_t *ev);
int WriteCsv(const std::string &path, const uint8_t *cols, int nvars, int64_t n, const std::vector<std::string> &names,
             const std::vector<std::vector<std::string>> &values);
int WriteLibsvm(const std::string &path, const int8_t *ev, int64_t n, int V, const int32_t *labels);
// the pieces of those generators the sampling engine (sample_host.cpp, sample.hip) is held to: the
// topological order (Kahn, LIFO stack, children ascending; shorter than n() for a cyclic graph) and
// numpy's PCG64(seed) after seeding, state and increment as (hi, lo) 64-bit halves
std::vector<int> TopoOrder(const Network &net);
void Pcg64Seed(uint64_t seed, uint64_t state[2], uint64_t inc[2]);

// ---------------------------------------------------------------------------------------------
// junction-tree static plan (host), container order as in JunctionTreeStructure
struct Table {
    std::vector<int> vars, dims, cum;  // row-major, left-most var most significant
    std::vector<double> pot;
    int64_t size() const { return (int64_t)pot.size(); }
    void Rebuild();
};

struct JTPlanHost {
    int num_nodes = 0;
    std::vector<int> dom;
    std::vector<Table> cliques, seps;  // initial potentials after ReorganizeTableStorage
    std::vector<int> clique_up;                 // upstream separator, -1 for a root
    std::vector<std::vector<int>> clique_down;  // downstream separators (MarkLevel order)
    std::vector<int> sep_up, sep_down;          // parent clique, child clique
    int root = -1;                              // = roots[0]
    std::vector<std::vector<int>> levels;       // even levels: cliques, odd levels: separators
    // junction forest: one tree per component of the moral graph (components numbered by their
    // lowest node), never joined -- roots[k] is the root of component k's tree, level i holds level i
    // of every tree.  A connected network has one component and roots = {root}.
    std::vector<int> roots;
    std::vector<int> component_of_node;
    int num_components = 0;
};
// forest = false: a disconnected moral graph is an error (FBN_ERR_ARG)
int BuildJTPlan(const Network &net, JTPlanHost &plan, bool forest = false);
// An initial clique potential is the plain fp64 product of the CPT entries of the families the clique
// hosts.  A count network's entries keep it far from the bottom of the range; a probability network's
// (any finite entry > 0) can take it to a subnormal or to zero, which every engine would then read as
// an impossible configuration.  FBN_ERR_LIMIT naming the clique and one of its nodes for an entry
// below DBL_MIN; the program compilers of every engine over the plan call it.
int CheckCliquePotential(int clique, const int *vars, int nvars, const double *pot, int64_t n);
int CheckPlanPotentials(const JTPlanHost &plan);

// device program (see jt_program.h) compiled from the host plan
struct JTProgram {
    std::vector<JtOp> ops;
    std::vector<int32_t> aux;
    std::vector<double> initv;
    std::vector<uint64_t> dig;
    int64_t state_entries = 0;  // NE: table entries + one pending denominator per clique
    int num_cliques = 0;
    int sum_dom = 0;
    int max_vars = 0;
};
int CompileJTProgram(const JTPlanHost &plan, JTProgram &prog);

// LDS-resident variant: per-wave global regions (entries of 64 lanes x fp64)
struct JTProgramLDS {
    std::vector<JtOp> ops;
    std::vector<int32_t> aux;
    std::vector<double> initv;
    std::vector<uint64_t> dig;
    int64_t store_entries = 0;  // parked collect tables (all cliques but plan.root)
    int64_t sep_entries = 0;    // separator messages
    int64_t max_table = 0;      // largest clique table (LDS rows needed for no spill)
    int num_cliques = 0;
    int sum_dom = 0;
};
int CompileJTProgramLDS(const JTPlanHost &plan, JTProgramLDS &prog);

// streamed ("virtual table") variant, see jt_program.h
struct JTProgramV {
    std::vector<JtVClique> cl;
    std::vector<int32_t> aux;
    std::vector<double> initv;
    std::vector<uint64_t> dig;
    std::vector<int32_t> order;  // clique ids of the schedule segments (see sched)
    std::vector<int32_t> sched;  // 2 * JT_V_WAVES + 3 segment offsets into order: Collect per wave,
                                 // Collect top, Distribute top, Distribute per wave, end
    double split_efficiency = 1.0;  // modelled parallel efficiency of the waves' tree split
    std::vector<int32_t> vsel;   // per variable {cand_off, ncand, out_off, dim} (candidates in aux)
    int64_t store_rows = 0;      // per-wave fp64 rows: Collect messages, Distribute messages, denominators,
    int64_t scratch_row = 0;     // then one scratch table per wave of the block
    int64_t scratch_rows = 0;    // rows per scratch table
    int num_cliques = 0;
    int sum_dom = 0;
};
// FBN_ERR_LIMIT when the plan does not fit the variant (a clique with > JT_V_MAX_CHILDREN children,
// more than 8 * JT_MAX_DIG_WORDS variables, or tables beyond int32 indexing)
int CompileJTProgramV(const JTPlanHost &plan, JTProgramV &prog);

// tiled variant (jt_tile.hip), see jt_program.h
struct JTProgramT {
    std::vector<JtTPass> passes;  // Collect (post-order), then Distribute (pre-order)
    std::vector<int32_t> tab;     // G / R / outer / bin-digit / marginal / variable / staging records
    std::vector<double> initv;
    int64_t scr_row = 0;          // wave store rows (JT_T_C fp64 each): messages, then partial bins,
    int64_t red_row = 0;          // then reduced bins
    int64_t store_rows = 0;
    int64_t lds_bytes = 0;        // per wave: the largest set of factors staged at once
    int64_t entry_visits = 0;     // clique entries summed over all passes (one case)
    int num_cliques = 0, sum_dom = 0;
    int waves = 1;                // waves per workgroup (one case group each) the passes' splits assume
};
// FBN_ERR_LIMIT when the plan does not fit (a domain > JT_T_MAXDIM states, > JT_T_MAXF - 1 children,
// > 32 digit bits in a clique, tables beyond int32 indexing).  lds_budget: bytes of factors per wave.
int CompileJTProgramT(const JTPlanHost &plan, JTProgramT &prog, int lds_budget);

// plan-specialized kernel source (jt_gen_*.cpp): eligibility and generation.  The generated
// kernel's per-wave workspace holds wave_entries rows of 64 fp64 lanes; initv is its constant input.
bool JTCodegenEligible(const JTPlanHost &plan, int64_t *entry_ops);
// message rows (64 lanes x fp64 each) of the generated kernel per place, [0] Collect, [1] Distribute
struct JTPlacement {
    int64_t global[2] = {0, 0}, lds[2] = {0, 0}, reg[2] = {0, 0};
    int64_t workspace_rows = 0;  // global rows per wave (a separator's two messages share theirs)
    int64_t lds_pool_rows = 0;   // LDS pool rows per wave (the most in use at one time)
};
struct JTKernelSpec {
    std::string src;
    std::vector<double> initv;
    int64_t wave_entries = 0, lds_bytes = 0;  // per wave: workspace rows, dynamic LDS
    JTPlacement place;
};
// fast: the fast arithmetic order (normalizations that cancel are left out; results within 1e-12 of
// the exact order, which repeats the reference's every multiply + Normalize); var_major: marginals
// stored variable-major [sum_dom][ncases] instead of case-major [ncases][sum_dom]
int GenerateJTKernel(const JTPlanHost &plan, bool fast, bool var_major, JTKernelSpec &out);

// compile + cache of the generated kernels (jt_jit.hip): the hiprtc options (part of the cache key),
// the cache file of a source, its code object (cache hit or compile)
extern const char *kJitOptions[];
extern const int kJitNumOptions;
std::string JitCachePath(const std::string &src);
int JitCodeObject(const std::string &src, std::vector<char> &code);

}  // namespace fbn

// C-ABI handles over the host model (capi.hip, synth.cpp)
struct fbn_network {
    fbn::Network net;
};
struct fbn_dataset {
    fbn::Dataset ds;
};

#endif
