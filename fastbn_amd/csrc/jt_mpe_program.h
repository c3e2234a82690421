// jt_mpe_program.h -- the max-product junction-forest program: compiled on the host from the forest
// plan (jt_mpe_plan.cpp), executed per evidence case by the host twin (jt_mpe_host.cpp) and by every
// lane of jt_mpe.hip.  Shared by host and device; plain C layout.  The algorithm is stated in
// include/fastbn.h above fbn_mpe_create.
//
// State of one case ("the store", rows of one fp64 / int64 per case):
//   message rows   one per separator entry: the Collect message M^ of the separator's child clique
//   exponent rows  one per separator: E of its child clique (an integer)
//   e* rows        one per clique: the entry the back-trace chose
// Clique tables are never stored: v(e) is recomputed from the initial potential and the children's
// messages wherever it is needed (Collect and back-trace), as the streamed sum-product variant does.
// Evidence is applied by masking, with CompileJTProgram's digit packing (8 bits per variable slot,
// 8 slots per 64-bit word, JT_MAX_DIG_WORDS words at most).
#ifndef FBN_JT_MPE_PROGRAM_H
#define FBN_JT_MPE_PROGRAM_H

#include <stdint.h>

#include "jt_program.h"

struct JtMClique {
    int32_t T, nv, k, nw;        // entries, variables, children, digit words per entry
    int32_t iv_off;              // initial potentials (fp64 index)
    int32_t dig_off;             // digit words (uint64 index), nw per entry
    int32_t vars_off;            // aux: the nv variable ids
    int32_t child_off;           // aux: k records {map_off (T int32: entry -> separator entry), message
                                 //      row, exponent row, child clique}, clique_down order
    int32_t up_Ts;               // entries of the upstream separator (0: a root)
    int32_t up_map_off;          // aux: T int32, entry -> upstream separator entry (= e % up_Ts)
    int32_t up_row, up_exp_row;  // the upstream separator's message rows and exponent row
    int32_t parent;              // parent clique (-1: a root)
    int32_t parent_map_off;      // aux: the parent's map onto the upstream separator (its T int32)
    int32_t estar_row;           // this clique's e* row
    int32_t nown;                // leading variables not in the upstream separator (the back-trace
                                 // assigns these; the separator's were assigned by the parent)
};

// what fbn_mpe_launch takes (launchers.h), filled by name in capi_mpe.hip
struct JtMpeArgs {
    const JtMClique *cl;
    const int32_t *aux;
    const double *initv;
    const uint64_t *dig;
    const int32_t *collect;  // clique ids: deepest level first, plan order within a level
    const int32_t *trace;    // clique ids: levels ascending, plan order within a level
    const int8_t *evid;      // [ncases][V]
    int8_t *assign;          // [ncases][V]
    double *value;           // [ncases][2]: mantissa in [0.5, 1), integral exponent
    double *dbg_msg;         // testing (or NULL): [ncases][msg_rows] after Collect
    int32_t *dbg_exp;        // testing (or NULL): [ncases][nsep]
    double *store;           // [grid][store_rows][64]
    long long ncases;
    long long store_rows;
    int nc, V, msg_rows, nsep;  // exponent rows start at msg_rows, e* rows at msg_rows + nsep
    int grid;
};

#include <vector>

namespace fbn {

struct JTPlanHost;

struct JTProgramMpe {
    std::vector<JtMClique> cl;
    std::vector<int32_t> aux;
    std::vector<double> initv;
    std::vector<uint64_t> dig;
    std::vector<int32_t> collect, trace;
    std::vector<int32_t> dom;
    int64_t msg_rows = 0;    // sum of the separator entries
    int64_t store_rows = 0;  // msg_rows + separators + cliques
    int64_t entries = 0;     // sum of the clique entries
    int nsep = 0, V = 0, components = 0;
};
// FBN_ERR_LIMIT for a clique of more than 8 * JT_MAX_DIG_WORDS variables or tables beyond int32 indexing
int CompileJTProgramMpe(const JTPlanHost &plan, JTProgramMpe &prog);
// FBN_ERR_ARG naming the first case / node whose code is neither -1 nor a state of the node
int CheckMpeEvidence(const JTProgramMpe &P, const int8_t *ev, int64_t ncases);
// value [ncases][2] = {m, ex} as MPE or the E-step reports it.  A case whose every unmasked v(e) of some
// clique underflowed to 0 has m == 0 (NaN posteriors in the E-step): the quantity is > 0 and {m, ex} could
// hold it, but a clique's potential times its messages is formed in plain fp64.  Normal potentials do not
// exclude it: messages are scaled by their row's largest entry, so a potential of 2^-920 beside one message
// entry 2^-300 below its row's largest is enough.  FBN_ERR_LIMIT naming the first such case.
int CheckCaseValues(const char *what, const double *value, int64_t ncases);
// The host twin: assignment [ncases][V], value [ncases][2]; messages [ncases][msg_rows] and exponents
// [ncases][nsep] (or NULL) as Collect leaves them.  Cases spread over HostThreads() threads.
int HostMpe(const JTProgramMpe &P, const int8_t *ev, int64_t ncases, int8_t *assign, double *value,
            double *messages, int32_t *exponents);

}  // namespace fbn

#endif
