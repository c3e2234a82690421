// jt_gen.h -- the records the three parts of the plan-specialized JT kernel generator share:
// options and per-variable tables (jt_gen_emit.cpp), the schedule (jt_gen_schedule.cpp) and the
// message placement (jt_gen_place.cpp).  Internal to the generator and its host check
// (tools/jt_codegen_host_check.cpp).
#ifndef FBN_JT_GEN_H
#define FBN_JT_GEN_H

#include <string>
#include <vector>

#include "fbn_internal.h"

namespace fbn {

// entry e of the clique in flight is a register value below kRegEntries, an LDS row of the clique
// tail from there on (round 5: 144 -- with the initial potentials as scalar loads, the LDS this frees
// holds the message pool: ALARM 0.165 -> 0.138 ms per 100k cases; 96 / 112 / 128 / 136 / 144 measured
// 0.151 / 0.142 / 0.141 / 0.140 / 0.138 ms)
constexpr int64_t kJtRegEntries = 144;
// register pool: fp64 values per lane of one wave per SIMD (512 registers), the part left to
// the compiler's temporaries, and the default cap on parked rows (FBN_JT_REG_POOL; 0 = off;
// kJtRegFile = bounded only by what the ops leave free).  ALARM, 100k cases, variable-major:
// slack 16 parks 123 rows, 231 -> 128 message rows in global memory, no spill, 0.1166 ->
// 0.1027 ms; slack 0 / 32 (42 / 2 spilled registers) 0.111 / 0.110 ms, caps 32 / 64 0.111 /
// 0.1026 ms.  The case-major kernel (64-bit output addresses: more registers of its own) spills
// at slack 16 (0.1218 -> 0.1272 ms); slack 28 / 32 / 36 / 48: 0.1179 / 0.1167 / 0.1176 / 0.1188 ms,
// but every one of them spills 42-44 SGPRs against 34 without the pool, so there the pool is
// opt-in
constexpr int64_t kJtRegFile = 256, kJtRegSlackVM = 16, kJtRegSlackCM = 32, kJtDefaultRegPool = kJtRegFile;

// the knobs and the two switches of the C-ABI, read once per generation
struct JtGenOptions {
    // fast arithmetic order: a clique's table is init * (product of its messages), never normalized
    // in between (the reference's per-step normalizations cancel in every normalized result);
    // messages are normalized once, marginals from a statically chosen clique
    bool fast = false;
    bool vmajor = false;   // marginals variable-major [SD][ncases] (fbn_jt_set_output_layout)
    // fp64 values per lane: table in flight + prefetched rows
    // (fast order: 260 -- round 5 sweep 150 / 200 / 260 / 320: 0.171 / 0.169 / 0.165 / 0.166 ms)
    int64_t budget = 200;
    // register pool: fast order only (the exact order's source is pinned); on by default for the
    // variable-major kernel only (the case-major one is faster with it too, but spills more SGPRs)
    int64_t reg_cap = 0;
    int64_t lds_pool = -1;  // FBN_JT_LDS_POOL: cap of the LDS message pool in rows (-1: what is left)
    bool leaf_rc = false;   // FBN_JT_LEAF_RC (JtGenSchedule::leaf_rc)
    bool sched = false;     // FBN_JT_SCHED: the load pipeline, on where the register pool is on
    // fast order: unbranched marginals with observed lanes stored as 0.0 and 16-byte stores of
    // adjacent values (FBN_JT_MARG_V2, default 1)
    bool marg_v2 = false;
    bool profile = false;   // FBN_JT_PROFILE: a cycle stamp per op category at the op boundaries
    bool place_debug = false;  // FBN_JT_PLACE_DEBUG: the chosen placement on stderr
    int64_t slack() const { return vmajor ? kJtRegSlackVM : kJtRegSlackCM; }
};
JtGenOptions JtGenReadOptions(bool fast, bool var_major);

// per-variable tables of the emitted text
struct JtGenTables {
    int SD = 0, nokw = 0, nobs = 0;
    // evidence: allowed-value bits of every variable packed into 32-bit words (okw<k>), observed
    // flags (obs<k>); var v owns bits [pos, pos + dom) of its word
    std::vector<int> okw_word, okw_pos, out_off;
    std::vector<int64_t> init_off;  // a clique's initial potential in the constant buffer
    std::vector<std::vector<int>> cand;  // the cliques holding a variable
    // fast order: the one clique each variable's evidence is entered in (its smallest holder): the
    // indicator of an observed value multiplies the joint once, so every calibrated clique still
    // holds P(clique, evidence) -- the other holders receive the zeros through their messages
    // (running intersection: the path to the home clique carries the variable)
    std::vector<int> home;
    // fast order: the separator a variable's marginal is summed from (its smallest holder when that
    // is smaller than its smallest clique; -1: the clique): the calibrated separator belief is the
    // parent's bin sums of its SepDis, P(separator, evidence) up to a per-case constant
    std::vector<int> msep;
    std::vector<int> mclq;  // fast order: the clique a variable's marginal is summed in when msep[v] < 0
    int64_t lds_rows = 0;   // LDS rows (64 lanes x fp64) per wave of the clique tail
};
JtGenTables JtGenBuildTables(const JTPlanHost &plan, bool fast);

// One op of the schedule: Collect of post[t] at time t < nc, Distribute of pre[t - nc] from nc on.
// Everything the placement charges and the emitter loads is decided here, once.
struct JtGenOp {
    int clique = -1;
    bool runs = true;    // false: the Collect of a forest root that sends no message (not emitted)
    bool early = false;  // Distribute: the children's Collect messages fit beside the table ("lb" at its start)
    std::vector<int> loads;     // separators loaded at the op's start: "la" (Collect), "lb" (Distribute, early)
    std::vector<int> prefetch;  // separators it may load for the next op under the same name,
    int prefetch_ld = -1;       // and the next op's parent message ("ld", -1: none)
    int64_t prefetch_rows = 0;  // rows of the candidates
    int64_t prefetch_cost = 0;  // table + rows held + candidates, without parked rows
    int64_t need = 0;           // the op's own register rows, the candidates included where they fit
    std::vector<int> touch;     // messages it holds anyway: 2 * separator + (Distribute message)
};
struct JtGenSchedule {
    std::vector<int> post, pre;  // Collect in DFS post-order, Distribute in DFS pre-order
    int cont_root = -1;          // the root collected last: it stays in registers for its Distribute
    std::vector<bool> md_reg;    // Distribute messages kept in registers (first child, if it fits)
    // fast order, opt-in (FBN_JT_LEAF_RC=1): Collect messages of small leaf cliques recomputed in the
    // parent's Distribute (initial potential x home indicators, bin sums: the same expression as in
    // Collect) instead of being parked from Collect to Distribute, stored only while the parent's
    // Collect needs them.  ALARM: 195 -> 151 global rows, but 0.137 -> 0.155 ms -- the recomputation
    // sits on the parent's critical path (round 5), so it is off by default
    std::vector<bool> leaf_rc, col_store;
    std::vector<JtGenOp> ops;    // 2 * nc
    int64_t peak_need = 0;       // the largest need of an op
    std::vector<int> qi, pi;     // a clique's time in Collect, in Distribute (less nc)
};
// visit: 0 = the plan's child order, 1 = heaviest subtree first, 2 = heaviest subtree last
std::vector<int> JtGenOrder(const JTPlanHost &plan, bool collect, int visit);
JtGenSchedule JtGenBuildSchedule(const JTPlanHost &plan, const JtGenOptions &opt, std::vector<int> post, std::vector<int> pre);

// one stored message: where its entries live over its interval [a, b] on the schedule's clock
struct JtGenMessage {
    int sep = -1;
    bool dist = false;  // the Distribute message (parent -> child), else the Collect one
    int a = 0, b = 0;
    int64_t n = 0, nreg = 0;  // entries, and the leading ones parked in registers
    bool in_lds = false;      // the others: LDS pool rows, else the per-wave rows in global memory
    std::vector<int64_t> rows;     // their rows (entry nreg + i in rows[i])
    std::vector<std::string> loc;  // per entry: a register name, "LP(row)" or "W(row)"
};
struct JtGenPlacement {
    std::vector<JtGenMessage> msgs;
    std::vector<int> col_of, dis_of;  // per separator: its entry in msgs, -1 when the message is not stored
    std::vector<int64_t> reg_extra;   // parked rows live at time t beyond what op t holds itself
    std::vector<int64_t> live;        // parked rows live at time t
    std::vector<int64_t> use;         // LDS pool rows in use at time t
    std::vector<std::string> reg_names;  // the parked entries' registers (declared per block)
    std::vector<int64_t> sep_row;     // first global row of a separator (both its messages share them)
    int64_t pool_rows = 0, pool_cap = 0;
    JTPlacement counts;
    // (a message that is not stored is never read from memory: the text of a place is "0.0")
    std::string Loc(int s, bool dist, int64_t j) const {
        const int i = dist ? dis_of[s] : col_of[s];
        return i < 0 ? std::string("0.0") : msgs[i].loc[j];
    }
};
JtGenPlacement JtGenPlace(const JTPlanHost &plan, const JtGenSchedule &sch, const JtGenOptions &opt, int64_t lds_rows);
int64_t JtGenWaveEntries(const JTPlanHost &plan, const JtGenPlacement &pl);  // rows of the per-wave workspace (FBN_WE)
void JtGenDescribe(const JTPlanHost &plan, const JtGenSchedule &sch, const JtGenPlacement &pl, const JtGenOptions &opt,
                   const JtGenTables &tab);

// tables, then the child orders the placement likes best (register pool on), their schedule and placement
int JtGenPlan(const JTPlanHost &plan, const JtGenOptions &opt, JtGenTables &tab, JtGenSchedule &sch, JtGenPlacement &pl);

}  // namespace fbn

#endif
