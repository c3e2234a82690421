// jt_codegen.cpp -- plan-specialized junction-tree kernel (HIP source, compiled with hiprtc for gfx950).
//
// For trees whose cliques are small (ALARM-class), the case-independent schedule is emitted as
// straight-line code: every table entry of the clique in flight is a named fp64 register value
// (lane = evidence case), every index map / digit / stride and every initial potential is a
// compile-time constant; the initial potentials are read with wave-uniform scalar loads from a
// constant buffer (iv_lds, off: from an LDS copy per wave).  No op dispatch, no index arrays;
// LDS holds the entries of a large clique past the register-resident ones and a pool of message
// rows (PlaceMessages).
//
// Schedule (values identical to the reference's level order -- a clique's Collect result depends
// only on its subtree and the fixed order of its child messages, its Distribute result only on its
// parent's -- so any children-first / parent-first traversal gives the same bits):
//  * Collect in DFS post-order: the last child's message stays in registers for its parent; other
//    messages are stored (they are needed again anyway as the "old" separator of Distribute) --
//    in registers the small cliques leave unused (fast order), in LDS pool rows when their live
//    interval fits, else in the per-wave rows in global memory (PlaceMessages).
//  * Distribute in DFS pre-order: a clique's Collect table is not parked and reloaded but
//    recomputed from its initial potential and its children's stored messages (which Distribute
//    loads anyway) -- ALU is cheap here, HBM round trips are not.  The message to the first child
//    stays in registers; the others go to LDS pool rows or overwrite their (now dead) Collect
//    message's global rows.
//  * Loads for the next clique are issued at the start of the current one (register budget
//    permitting) so their latency hides behind its arithmetic.
// Operation order per entry is exactly the interpreter's (= the reference's), so results are
// bit-identical; a lane whose normalization denominator leaves [2^-600, 2^600] flags its block,
// which the exact interpreter then recomputes (see capi_jt.hip).
#include <algorithm>
#include <map>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <sstream>
#include <string>

#include "fbn_internal.h"

namespace fbn {

namespace {

int LocOfT(const Table &t, int v) {
    for (size_t i = 0; i < t.vars.size(); ++i)
        if (t.vars[i] == v) return (int)i;
    return -1;
}

std::string Lit(double x) {  // exact decimal literal (%.17g round-trips)
    char b[64];
    snprintf(b, sizeof b, "%.17g", x);
    std::string s = b;
    if (s.find_first_of(".eEn") == std::string::npos) s += ".0";
    return s;
}

}  // namespace

bool JTCodegenEligible(const JTPlanHost &plan, int64_t *entry_ops) {
    int64_t tmax = 0, ops = 0;
    for (const auto &t : plan.cliques) {
        tmax = std::max<int64_t>(tmax, t.size());
        ops += t.size() * (4 + (int64_t)t.vars.size());
    }
    if (entry_ops) *entry_ops = ops;
    for (int d : plan.dom)
        if (d > 32) return false;  // evidence bit packing
    return tmax <= 256 && ops <= 40000;  // tails beyond 96 entries in LDS: <= 80 KB per wave
}

namespace {

class JTGen {
  public:
    JTGen(const JTPlanHost &p, bool fast_order, bool var_major) : plan(p), fast(fast_order), vmajor(var_major) {}
    int Run(std::string &src, int64_t *wave_entries, std::vector<double> &initv);
    int64_t lds_rows = 0;  // LDS rows (64 lanes x fp64) per wave: the clique tail
    int64_t pool_rows = 0;  // + LDS rows of the message pool (after the tail, before the initial potentials)
    JTPlacement place;  // message rows per place (PlaceMessages)
    // initial potentials: scalar loads from the constant buffer (round 5 default; 1 = an LDS copy per
    // wave, which takes LDS from the message pool: ALARM 0.163 vs 0.141 ms)
    bool iv_lds = false;

  private:
    const JTPlanHost &plan;
    // fast arithmetic order: a clique's table is init * (product of its messages), never normalized
    // in between (the reference's per-step normalizations cancel in every normalized result);
    // messages are normalized once, marginals from a statically chosen clique
    const bool fast;
    const bool vmajor;  // marginals variable-major [SD][ncases] (fbn_jt_set_output_layout)
    std::ostringstream o;
    std::vector<int> okw_word, okw_pos, out_off;
    std::vector<int64_t> sep_row, init_off;
    std::vector<std::vector<int>> cand;
    // fast order: the one clique each variable's evidence is entered in (its smallest holder): the
    // indicator of an observed value multiplies the joint once, so every calibrated clique still
    // holds P(clique, evidence) -- the other holders receive the zeros through their messages
    // (running intersection: the path to the home clique carries the variable)
    std::vector<int> home;
    // fast order: the separator a variable's marginal is summed from (its smallest holder when that
    // is smaller than its smallest clique; -1: the clique): the calibrated separator belief is the
    // parent's bin sums of its SepDis, P(separator, evidence) up to a per-case constant
    std::vector<int> msep;
    // fast order: the clique a variable's marginal is summed in when msep[v] < 0 (default: home[v])
    std::vector<int> mclq;
    // fast order: a marginal (and the label of variable 0) from the terms of each value
    void MargTerms(int v, const std::vector<std::vector<std::string>> &terms);
    int nobs = 0;
    // op boundary (+ diagnostic cycle stamp of op category k when FBN_JT_PROFILE is set)
    bool profile = false;
    static constexpr int64_t kInitBatch = 16;  // fast order: entries per software-pipelined batch of the fused product
    // Pipeline of the initial potentials' scalar loads, on where the register pool is on
    // (FBN_JT_SCHED, default 1; 0 = the loads as without the pool).  Values are untouched: only
    // where the loads stand changes.  Without it batch b + 1 is requested right before batch b's
    // first use, and as scalar loads return out of order that use's wait (lgkmcnt(0)) covers the
    // request just made: every second batch paid a whole scalar-cache round trip.  With it
    //  * batch b + 1 is requested after the first products of batch b, so behind their wait;
    //  * the first batch of fused product n + 1 (kSchedFirst entries: the SGPRs it holds across the
    //    sums of op n) is requested right after fused product n, the first product's in front of
    //    its op;
    //  * the loads are volatile vector loads (IvLoads), which keep their place.
    static constexpr int64_t kSchedFirst = 8;
    bool sched = false;
    int64_t BatchEnd(int64_t b0, int64_t T) const { return std::min(T, b0 + (b0 == 0 && sched ? kSchedFirst : kInitBatch)); }
    bool iv_issued = false;  // the next fused product's first batch is already requested
    // With the pipeline, the product trees of kSchedGroup entries of a fused product and the bin
    // sums of kSchedGroup bins of a Collect message are written level by level (every node over two
    // leaves first, then the nodes over those), one named temporary per inner node: the same trees
    // as prod / TreeSum, so the same operands and association.  No barrier between the levels: the
    // order is a hint to the compiler, which keeps enough of it.
    static constexpr int64_t kSchedGroup = 2;
    int64_t ntemp = 0;  // the temporaries' names
    struct LTree {  // one statement: head <balanced tree of the leaves> ; tail
        std::string head;
        std::vector<std::string> leaves;
        std::string tail;
    };
    std::vector<std::string> Levels(const std::vector<LTree> &trees, char op);  // the statements, by level
    bool in_leaf_rc = false;
    std::string IvLoads(const std::string &P, int c, int64_t b0);
    // the first batch of the next fused product: a marker in the text after each fused product,
    // which Run replaces at the end
    std::vector<std::string> iv_first;
    void IvFirst(const std::string &P, int c) {
        if (iv_first.empty()) o << IvLoads(P, c, 0);
        else iv_first.back() = IvLoads(P, c, 0);
        iv_issued = true;
    }
    static std::string IvMarker(size_t n) { return "/*@iv" + std::to_string(n) + "@*/"; }
    // fast order: a clique's SepDis ops and marginals share one op region (independent of each
    // other: their latencies overlap); inside it an op's closing boundary is left out
    bool in_merged = false;
    int min_waves = 1;
    // fast order: unbranched marginals with observed lanes stored as 0.0 and 16-byte stores of
    // adjacent values (FBN_JT_MARG_V2, default 1)
    bool marg_v2 = true;
    // where each stored message lives, per separator entry: "W(row)" (the per-wave workspace in
    // global memory) or "LP(row)" (the LDS message pool); the Collect message (child -> parent) and
    // the Distribute message (parent -> child) of a separator are placed separately
    std::vector<std::vector<std::string>> col_loc, dis_loc;
    std::vector<bool> md_reg;  // Distribute messages kept in registers (first child, if it fits)
    // fast order, opt-in (FBN_JT_LEAF_RC=1): Collect messages of small leaf cliques recomputed in the
    // parent's Distribute (initial potential x home indicators, bin sums: the same expression as in
    // Collect) instead of being parked from Collect to Distribute, stored only while the parent's
    // Collect needs them.  ALARM: 195 -> 151 global rows, but 0.137 -> 0.155 ms -- the recomputation
    // sits on the parent's critical path (gpurun_out/r05o), so it is off by default
    std::vector<bool> leaf_rc, col_store;
    void LoadCol(const std::string &name, int s) {
        if (!leaf_rc[s]) return Load(name, s);
        const int c = plan.sep_down[s];
        const int64_t Ts = plan.seps[s].size(), Q = plan.cliques[c].size() / Ts;
        for (int64_t j = 0; j < Ts; ++j) o << "        double " << name << s << "_" << j << ";\n";
        o << "        { // recompute the Collect message of leaf clique " << c << "\n";
        const std::string P = "r" + name;
        in_leaf_rc = true;  // (a scope of its own: no first batch of the next fused product in it)
        InitProd(P, c, {}, -1, "");
        in_leaf_rc = false;
        for (int64_t j = 0; j < Ts; ++j) {
            std::vector<std::string> terms;
            for (int64_t q = 0; q < Q; ++q) terms.push_back(N(P, c, q * Ts + j));
            o << "        " << name << s << "_" << j << " = " << TreeSum(terms) << ";\n";
        }
        o << "        }\n";
    }
    void PlaceMessages(const std::vector<int> &post, const std::vector<int> &pre, int64_t budget, int64_t reg_cap,
                       bool quiet);
    // register pool: fp64 values per lane of one wave per SIMD (512 registers), the part left to
    // the compiler's temporaries, and the default cap on parked rows (FBN_JT_REG_POOL; 0 = off;
    // kRegFile = bounded only by what the ops leave free).  ALARM, 100k cases, variable-major:
    // slack 16 parks 123 rows, 231 -> 128 message rows in global memory, no spill, 0.1166 ->
    // 0.1027 ms; slack 0 / 32 (42 / 2 spilled registers) 0.111 / 0.110 ms, caps 32 / 64 0.111 /
    // 0.1026 ms.  The case-major kernel (64-bit output addresses: more registers of its own) spills
    // at slack 16 (0.1218 -> 0.1272 ms); slack 28 / 32 / 36 / 48: 0.1179 / 0.1167 / 0.1176 / 0.1188 ms,
    // but every one of them spills 42-44 SGPRs against 34 without the pool, so there the pool is
    // opt-in
    static constexpr int64_t kRegFile = 256, kRegSlackVM = 16, kRegSlackCM = 32, kDefaultRegPool = kRegFile;
    int64_t peak_need = 0;  // the largest register need of an op itself, over the schedule
    std::vector<int64_t> reg_extra;  // parked rows live at time t beyond what op t holds itself
    std::vector<std::string> reg_names;  // the parked entries' registers (declared per block)
    std::string B(int k) const {
        return profile ? "        FBN_OP_BOUNDARY(); FBN_STAMP(" + std::to_string(k) + ");\n" : "        FBN_OP_BOUNDARY();\n";
    }

    std::string R(int c) const {  // number of unobserved variables of clique c
        std::vector<unsigned> m(nobs, 0u);
        for (int v : plan.cliques[c].vars) m[v / 32] |= 1u << (v % 32);
        std::ostringstream t;
        t << "(" << plan.cliques[c].vars.size();
        for (int k = 0; k < nobs; ++k)
            if (m[k]) t << " - __builtin_popcount(obs" << k << " & " << m[k] << "u)";
        t << ")";
        return t.str();
    }
    std::string observed(int v) const {
        std::ostringstream t;
        t << "((obs" << v / 32 << " >> " << v % 32 << ") & 1u)";
        return t.str();
    }
    int child(int s) const { return plan.sep_down[s]; }
    // separator index of clique entry e (the clique's digits of the separator's variables)
    int64_t SepIndex(const Table &t, const Table &sp, int64_t e) const {
        int64_t r = e, idx = 0;
        for (size_t j = 0; j < t.vars.size(); ++j) {
            const int64_t dgt = r / t.cum[j];
            r %= t.cum[j];
            const int l = LocOfT(sp, t.vars[j]);
            if (l >= 0) idx += dgt * sp.cum[l];
        }
        return idx;
    }
    void Init(const std::string &P, int c);
    // fast order: Init and every multiplication of the clique fused into one op (per entry the
    // initial potential x the home-evidence indicators x each message), ILP over all entries
    void InitProd(const std::string &P, int c, const std::vector<std::pair<int, std::string>> &kids, int up,
                  const std::string &upM);
    void Mul(const std::string &P, int c, int s, const std::string &M);
    void SepCol(const std::string &P, int c, int s, bool store);
    void DMul(const std::string &P, int c, int s, const std::string &M);
    void SepDis(const std::string &P, int c, int s, const std::string &old, bool store);
    void Marg(const std::string &P, int c);
    void Load(const std::string &name, int s) {  // "ld": the Distribute message, else the Collect one
        const auto &loc = name == "ld" ? dis_loc[s] : col_loc[s];
        for (int64_t j = 0; j < plan.seps[s].size(); ++j)
            o << "        const double " << name << s << "_" << j << " = " << loc[j] << ";\n";
    }
    // entry e of clique c's table: a register value, or (entries >= kRegEntries of a large table)
    // an LDS row [row][64 lanes] -- only one clique is in flight, so every table starts at row 0
    // (round 5: 144 -- with the initial potentials as scalar loads, the LDS this frees holds the
    // message pool: ALARM 0.165 -> 0.138 ms per 100k cases; 96 / 112 / 128 / 136 / 144 measured
    // 0.151 / 0.142 / 0.141 / 0.140 / 0.138 ms, gpurun_out/r05l, r05m)
    static constexpr int64_t kRegEntries = 144;
    std::string N(const std::string &P, int c, int64_t e) const {
        if (e >= kRegEntries) return "L(" + std::to_string(e - kRegEntries) + ")";
        return P + std::to_string(c) + "_" + std::to_string(e);
    }
    // value of entry e as the reference holds it: divided by the pending denominator unless the
    // table has been normalized eagerly (Normalize) since its last update
    bool normed = false;
    std::string Val(const std::string &P, int c, int64_t e) const {
        return (normed || fast) ? N(P, c, e) : "dv(" + N(P, c, e) + ", den, y)";
    }
    // fast order: a sum as a balanced tree of adds (depth log2 n instead of an n-long dependency
    // chain: a dependent fp64 add costs ~45 cycles at one wave per SIMD, an independent one ~5,
    // tools/micro/fp64_ilp.hip); the reference's left-to-right order is kept in the exact order
    static std::string TreeSum(const std::vector<std::string> &t, size_t b, size_t e) {
        if (e - b == 1) return t[b];
        const size_t m = b + (e - b) / 2;
        return "(" + TreeSum(t, b, m) + " + " + TreeSum(t, m, e) + ")";
    }
    static std::string TreeSum(const std::vector<std::string> &t) { return TreeSum(t, 0, t.size()); }
    void Normalize(const std::string &P, int c) {
        const Table &t = plan.cliques[c];
        for (int64_t e = 0; e < t.size(); ++e) o << (e % 8 ? " " : (e ? "\n        " : "        ")) << N(P, c, e) << " = dv(" << N(P, c, e) << ", den, y);";
        o << "\n" << B(6);
        normed = true;
    }
};

// masked initial potential + Normalize (lazy: values raw, den/y pending)
void JTGen::Init(const std::string &P, int c) {
    const Table &t = plan.cliques[c];
    const int nv = (int)t.vars.size();
    // per (variable, value) "allowed by the evidence" lane masks, then one AND chain per entry
    std::vector<bool> ev_here(nv, true);  // variables whose evidence this table carries
    for (int j = 0; j < nv; ++j) ev_here[j] = !fast || home[t.vars[j]] == c;
    for (int j = 0; j < nv; ++j) {
        const int v = t.vars[j];
        if (!ev_here[j]) continue;
        for (int d = 0; d < plan.dom[v]; ++d)
            o << (d ? " " : "        ") << "const bool k" << P << c << "_" << j << "_" << d << " = (okw" << okw_word[v] << " >> "
              << okw_pos[v] + d << ") & 1u;";
        o << "\n";
    }
    if (!fast) o << "        double s_" << P << c << " = 0.0;\n";
    // software-pipelined in batches: the LDS reads of batch b+1 are issued before batch b computes
    const int64_t kB = 16, T = t.size();
    auto loads = [&](int64_t b0) {
        if (b0 >= T) return;
        o << "       ";
        for (int64_t e = b0; e < std::min(T, b0 + kB); ++e)
            o << " const double w" << P << c << "_" << e << " = IV(" << init_off[c] + e << ");";
        o << "\n        __builtin_amdgcn_sched_barrier(0);\n";
    };
    loads(0);
    for (int64_t b0 = 0; b0 < T; b0 += kB) {
        loads(b0 + kB);
        for (int64_t e = b0; e < std::min(T, b0 + kB); ++e) {
            std::ostringstream cond;
            int64_t r = e;
            bool any = false;
            for (int j = 0; j < nv; ++j) {
                const int64_t dgt = r / t.cum[j];
                r %= t.cum[j];
                if (!ev_here[j]) continue;
                cond << (any ? " && " : "") << "k" << P << c << "_" << j << "_" << dgt;
                any = true;
            }
            o << "        " << (e < kRegEntries ? "double " : "") << N(P, c, e) << " = ";
            if (any) o << "sel(" << cond.str() << ", w" << P << c << "_" << e << ");";
            else o << "w" << P << c << "_" << e << ";";
            if (!fast) o << " s_" << P << c << " += " << N(P, c, e) << ";";
            o << "\n";
        }
        o << "        __builtin_amdgcn_sched_barrier(0);\n";
    }
    if (!fast) o << "        den = s_" << P << c << "; y = 1.0 / den; bad |= den_bad(den);\n";
    o << B(2);
    normed = false;
}

std::vector<std::string> JTGen::Levels(const std::vector<LTree> &trees, char op) {
    std::vector<std::string> lv;
    const std::string ops = std::string(" ") + op + " ";
    for (const LTree &t : trees) {
        // (name, height) of the node over the leaves [lo, hi), split like TreeSum
        std::function<std::pair<std::string, size_t>(size_t, size_t)> node = [&](size_t lo, size_t hi) -> std::pair<std::string, size_t> {
            if (hi - lo == 1) return {t.leaves[lo], 0};
            const size_t m = lo + (hi - lo) / 2;
            const auto a = node(lo, m), b = node(m, hi);
            const size_t h = 1 + std::max(a.second, b.second);
            if (lv.size() < h) lv.resize(h);
            if (lo == 0 && hi == t.leaves.size()) {
                lv[h - 1] += t.head + a.first + ops + b.first + ";" + t.tail;
                return {"", h};
            }
            const std::string nm = "x" + std::to_string(ntemp++);
            lv[h - 1] += "        const double " + nm + " = " + a.first + ops + b.first + ";\n";
            return {nm, h};
        };
        const auto r = node(0, t.leaves.size());
        if (t.leaves.size() == 1) {
            if (lv.empty()) lv.resize(1);
            lv[0] += t.head + r.first + ";" + t.tail;
        }
    }
    return lv;
}

std::string JTGen::IvLoads(const std::string &P, int c, int64_t b0) {
    const int64_t T = plan.cliques[c].size();
    std::ostringstream o;
    if (b0 >= T) return std::string();
    const int64_t b1 = BatchEnd(b0, T);
    if (sched && !iv_lds) {
        // Ordered loads: a plain load from the constant address space is tied to nothing, and
        // instruction selection places it next to its first use whatever the statement order (the
        // scheduling barriers bind the machine scheduler only).  A volatile load keeps its place
        // between the barriers; whole vectors, so a batch is still two 64-byte scalar loads.
        for (int64_t e = b0, n = 16; e < b1; e += n) {
            while (n > b1 - e) n /= 2;
            const std::string wv = "wv" + P + std::to_string(c) + "_" + std::to_string(e);
            o << "        const " << (n > 1 ? "fbn_w" + std::to_string(n) : std::string("double")) << " " << wv << " = *(const volatile "
              << (n > 1 ? "fbn_cw" + std::to_string(n) : std::string("cdouble")) << " *)&IV(" << init_off[c] + e << ");";
            for (int64_t k = 0; k < n; ++k)
                o << " const double w" << P << c << "_" << e + k << " = " << wv << (n > 1 ? "[" + std::to_string(k) + "]" : std::string()) << ";";
            o << "\n";
        }
        o << "        __builtin_amdgcn_sched_barrier(0);\n";
        return o.str();
    }
    o << "       ";
    for (int64_t e = b0; e < b1; ++e)
        o << " const double w" << P << c << "_" << e << " = IV(" << init_off[c] + e << ");";
    o << "\n        __builtin_amdgcn_sched_barrier(0);\n";
    return o.str();
}

void JTGen::InitProd(const std::string &P, int c, const std::vector<std::pair<int, std::string>> &kids, int up,
                     const std::string &upM) {
    const Table &t = plan.cliques[c];
    const int nv = (int)t.vars.size();
    // 0.0 / 1.0 indicators of the home variables' allowed values (x * 1.0 == x, x * 0.0 == 0 for the
    // finite potentials: the masking of the reference's reduction, one multiply instead of a select)
    std::vector<bool> ev_here(nv, false);
    for (int j = 0; j < nv; ++j) ev_here[j] = home[t.vars[j]] == c;
    for (int j = 0; j < nv; ++j) {
        if (!ev_here[j]) continue;
        const int v = t.vars[j];
        for (int d = 0; d < plan.dom[v]; ++d)
            o << (d ? " " : "        ") << "const double i" << P << c << "_" << j << "_" << d << " = (double)((okw"
              << okw_word[v] << " >> " << okw_pos[v] + d << ") & 1u);";
        o << "\n";
    }
    std::vector<std::vector<int64_t>> kidx(kids.size());
    for (size_t i = 0; i < kids.size(); ++i) {
        const Table &sp = plan.seps[kids[i].first];
        for (int64_t e = 0; e < t.size(); ++e) kidx[i].push_back(SepIndex(t, sp, e));
    }
    const int64_t Tup = up >= 0 ? plan.seps[up].size() : 0;
    const int64_t T = t.size();
    if (!iv_issued) o << IvLoads(P, c, 0);
    iv_issued = false;
    // the factors of entry e, in the order of the product tree
    auto factors = [&](int64_t e) {
        std::vector<std::string> f{"w" + P + std::to_string(c) + "_" + std::to_string(e)};
        int64_t r = e;
        for (int j = 0; j < nv; ++j) {
            const int64_t dgt = r / t.cum[j];
            r %= t.cum[j];
            if (ev_here[j]) f.push_back("i" + P + std::to_string(c) + "_" + std::to_string(j) + "_" + std::to_string(dgt));
        }
        for (size_t i = 0; i < kids.size(); ++i)
            f.push_back(kids[i].second + std::to_string(kids[i].first) + "_" + std::to_string(kidx[i][e]));
        if (up >= 0) f.push_back(upM + std::to_string(up) + "_" + std::to_string(e % Tup));
        return f;
    };
    const std::string wpre = "w" + P + std::to_string(c) + "_";
    for (int64_t b0 = 0, b1; b0 < T && sched; b0 = b1) {
        b1 = BatchEnd(b0, T);
        // the next batch is requested behind the first level that reads a potential of this one,
        // so behind its wait
        bool pending = b1 < T;
        for (int64_t e0 = b0; e0 < b1; e0 += kSchedGroup) {
            std::vector<LTree> trees;
            for (int64_t e = e0; e < std::min(b1, e0 + kSchedGroup); ++e)
                trees.push_back({"        " + std::string(e < kRegEntries ? "double " : "") + N(P, c, e) + " = ", factors(e), "\n"});
            for (const std::string &l : Levels(trees, '*')) {
                o << l;
                if (pending && l.find(wpre) != std::string::npos) {
                    o << "        __builtin_amdgcn_sched_barrier(0);\n" << IvLoads(P, c, b1);
                    pending = false;
                }
            }
        }
        o << "        __builtin_amdgcn_sched_barrier(0);\n";
    }
    for (int64_t b0 = 0, b1; b0 < T && !sched; b0 = b1) {
        b1 = BatchEnd(b0, T);
        o << IvLoads(P, c, b1);
        for (int64_t e = b0; e < b1; ++e) {
            const std::vector<std::string> f = factors(e);
            // a balanced product tree (depth log2 of the factor count)
            std::function<std::string(size_t, size_t)> prod = [&](size_t lo, size_t hi) -> std::string {
                if (hi - lo == 1) return f[lo];
                const size_t m = lo + (hi - lo) / 2;
                return "(" + prod(lo, m) + " * " + prod(m, hi) + ")";
            };
            o << "        " << (e < kRegEntries ? "double " : "") << N(P, c, e) << " = " << prod(0, f.size()) << ";\n";
        }
        o << "        __builtin_amdgcn_sched_barrier(0);\n";
    }
    o << B(2);
    if (sched && !in_leaf_rc) o << IvMarker(iv_first.size()) << "\n", iv_first.push_back(std::string());
    normed = false;
}

// CliqueLevelCollection: table *= extended child message (by separator entry), then Normalize
void JTGen::Mul(const std::string &P, int c, int s, const std::string &M) {
    const Table &t = plan.cliques[c], &sp = plan.seps[s];
    std::vector<std::vector<int64_t>> inv(sp.size());
    for (int64_t e = 0; e < t.size(); ++e) inv[SepIndex(t, sp, e)].push_back(e);
    for (int64_t j = 0; j < sp.size(); ++j) {
        o << "       ";
        for (int64_t e : inv[j]) o << " " << N(P, c, e) << " = " << Val(P, c, e) << " * " << M << s << "_" << j << ";";
        o << "\n";
    }
    if (!fast) {
        o << "        { double sm = 0.0;";
        for (int64_t e = 0; e < t.size(); ++e) o << " sm += " << N(P, c, e) << ";";
        o << " den = sm; y = 1.0 / den; bad |= den_bad(den); }\n";
    }
    o << B(3);
    normed = false;
}

// SeparatorLevelCollection: message[k % Ts] += table[k] / den  -> registers mc<s>_j (+ store)
void JTGen::SepCol(const std::string &P, int c, int s, bool store) {
    const Table &t = plan.cliques[c];
    const int64_t Ts = plan.seps[s].size(), Q = t.size() / Ts;
    if (fast) {
        // message = the raw bin sums (tree sums), never normalized: every later use is invariant to
        // a per-case scale of it (the Distribute ratio a / old, the normalized marginals), and its
        // values are likelihoods of the evidence below (<= 1); Marg range-checks the products
        for (int64_t j0 = 0; j0 < Ts && sched; j0 += kSchedGroup) {
            std::vector<LTree> trees;
            for (int64_t j = j0; j < std::min(Ts, j0 + kSchedGroup); ++j) {
                const std::string mc = "mc" + std::to_string(s) + "_" + std::to_string(j);
                std::vector<std::string> terms;
                for (int64_t q = 0; q < Q; ++q) terms.push_back(N(P, c, q * Ts + j));
                trees.push_back({"        const double " + mc + " = ", terms, (store ? " " + col_loc[s][j] + " = " + mc + ";" : std::string()) + "\n"});
            }
            for (const std::string &l : Levels(trees, '+')) o << l;
        }
        for (int64_t j = 0; j < Ts && !sched; ++j) {
            std::vector<std::string> terms;
            for (int64_t q = 0; q < Q; ++q) terms.push_back(N(P, c, q * Ts + j));
            o << "        const double mc" << s << "_" << j << " = " << TreeSum(terms) << ";";
            if (store) o << " " << col_loc[s][j] << " = mc" << s << "_" << j << ";";
            o << "\n";
        }
        if (!in_merged) o << B(4);
        return;
    }
    for (int64_t j = 0; j < Ts; ++j) {
        o << "        const double mc" << s << "_" << j << " = " << Val(P, c, j);
        for (int64_t q = 1; q < Q; ++q) o << " + " << Val(P, c, q * Ts + j);
        o << ";";
        if (store) o << " " << col_loc[s][j] << " = mc" << s << "_" << j << ";";
        o << "\n";
    }
    o << B(4);
}

// CliqueLevelDistribution: table *= parent message broadcast over k % Ts, then Normalize
void JTGen::DMul(const std::string &P, int c, int s, const std::string &M) {
    const Table &t = plan.cliques[c];
    const int64_t Ts = plan.seps[s].size();
    for (int64_t j = 0; j < Ts; ++j) {
        o << "       ";
        for (int64_t e = j; e < t.size(); e += Ts)
            o << " " << N(P, c, e) << " = " << Val(P, c, e) << " * " << M << s << "_" << j << ";";
        o << "\n";
    }
    if (!fast) {
        o << "        { double sm = 0.0;";
        for (int64_t e = 0; e < t.size(); ++e) o << " sm += " << N(P, c, e) << ";";
        o << " den = sm; y = 1.0 / den; bad |= den_bad(den); }\n";
    }
    o << B(5);
    normed = false;
}

// SeparatorLevelDistribution: tmp[map(k)] += table[k] / den; message = tmp / old (zero-guarded)
void JTGen::SepDis(const std::string &P, int c, int s, const std::string &old, bool store) {
    const Table &t = plan.cliques[c], &sp = plan.seps[s];
    std::vector<std::vector<int64_t>> lists(sp.size());
    for (int64_t e = 0; e < t.size(); ++e) lists[SepIndex(t, sp, e)].push_back(e);
    if (fast) {
        // bin sums a(j) as trees; md(j) = a(j) / old(j), 0 where old(j) == 0, with branch-free
        // reciprocals (v_rcp_f64 + one Newton step) so the Ts quotients overlap; no normalization
        // (the child's marginals are normalized at the end; values stay likelihoods <= 1)
        for (int64_t j = 0; j < sp.size(); ++j) {
            std::vector<std::string> terms;
            for (int64_t e : lists[j]) terms.push_back(N(P, c, e));
            const std::string sa = "sa" + std::to_string(s) + "_" + std::to_string(j);
            o << "        const double " << sa << " = " << TreeSum(terms) << ";";
            o << " double md" << s << "_" << j << "; { const double od = " << old << s << "_" << j
              << "; const double q = " << sa << " * frcp(od); md" << s << "_" << j << " = (od == 0.0) ? 0.0 : q; }";
            if (store) o << " " << dis_loc[s][j] << " = md" << s << "_" << j << ";";
            o << "\n";
        }
        // the marginals summed from this separator's calibrated belief (its bin sums)
        for (size_t l = 0; l < sp.vars.size(); ++l) {
            const int v = sp.vars[l];
            if (msep[v] != s) continue;
            std::vector<std::vector<std::string>> terms(plan.dom[v]);
            for (int64_t j = 0; j < sp.size(); ++j)
                terms[(j / sp.cum[l]) % sp.dims[l]].push_back("sa" + std::to_string(s) + "_" + std::to_string(j));
            MargTerms(v, terms);
        }
        if (!in_merged) o << B(7);
        return;
    }
    for (int64_t j = 0; j < sp.size(); ++j) {
        o << "        double md" << s << "_" << j << ";";
        o << " { double a = " << Val(P, c, lists[j][0]) << ";";
        for (size_t q = 1; q < lists[j].size(); ++q) o << " a += " << Val(P, c, lists[j][q]) << ";";
        o << " const double od = " << old << s << "_" << j << "; md" << s << "_" << j << " = (od == 0.0) ? 0.0 : a / od; }";
        if (store) o << " " << dis_loc[s][j] << " = md" << s << "_" << j << ";";
        o << "\n";
    }
    o << B(7);
}

void JTGen::MargTerms(int v, const std::vector<std::vector<std::string>> &terms) {
    const int dim = plan.dom[v];
    if (marg_v2) {
        // unbranched: computed for every lane, observed lanes store 0.0 (the reference's marginal of
        // an observed variable) in the same stores -- no divergent branch, no second store pass
        // (ALARM 0.137 -> 0.130 ms); adjacent values go out as one 16-byte store per lane (neutral).
        // (Measured and dropped: staging groups of 8 / 16 output values in LDS pool rows and writing
        // them out coalesced, 0.205 / 0.223 ms -- gpurun_out/r05q.)
        o << "        { // marginal of var " << v << "\n          const bool ob = " << observed(v) << " != 0u;\n";
        std::vector<std::string> ps;
        for (int d = 0; d < dim; ++d) {
            o << "          const double p" << d << " = " << TreeSum(terms[d]) << ";\n";
            ps.push_back("p" + std::to_string(d));
        }
        o << "          const double tot = " << TreeSum(ps) << "; const double yt = frcp(tot); bad |= ob ? 0u : den_bad(tot);\n";
        if (v == 0) {
            o << "          if (ACT && !ob) { int lab = 0; double mp = 0.0, m2 = 0.0;";
            for (int d = 0; d < dim; ++d)
                o << " { const double q = dv(p" << d << ", tot, yt); if (q > mp) { m2 = mp; mp = q; lab = " << d
                  << "; } else if (q > m2) m2 = q; }";
            o << " labels[CS] = lab; bad |= (mp - m2 <= 1e-12 * mp) ? 1u : 0u; }\n";
        }
        for (int d = 0; d < dim; ++d) {
            const int64_t k = out_off[v] + d;
            if (marg_v2 && d + 1 < dim) {
                o << "          if (ACT) OUTS2(" << k << ", ob ? 0.0 : dv(p" << d << ", tot, yt), ob ? 0.0 : dv(p" << d + 1 << ", tot, yt));\n";
                ++d;
            } else {
                o << "          if (ACT) OUTS(" << k << ", ob ? 0.0 : dv(p" << d << ", tot, yt));\n";
            }
        }
        o << "        }\n";
        return;
    }
    o << "        if (!" << observed(v) << ") { // marginal of var " << v << "\n";
    std::vector<std::string> ps;
    for (int d = 0; d < dim; ++d) {
        o << "          const double p" << d << " = " << TreeSum(terms[d]) << ";\n";
        ps.push_back("p" + std::to_string(d));
    }
    o << "          const double tot = " << TreeSum(ps) << "; const double yt = frcp(tot); bad |= den_bad(tot);\n";
    if (v == 0) {
        // a near-tie (top two within 1e-12 relative) may break differently from the reference's exact
        // values: the block is flagged for the exact pass
        o << "          if (ACT) { int lab = 0; double mp = 0.0, m2 = 0.0;";
        for (int d = 0; d < dim; ++d)
            o << " { const double q = dv(p" << d << ", tot, yt); if (q > mp) { m2 = mp; mp = q; lab = " << d
              << "; } else if (q > m2) m2 = q; }";
        o << " labels[CS] = lab; bad |= (mp - m2 <= 1e-12 * mp) ? 1u : 0u; }\n";
    }
    o << "          if (ACT) {";
    for (int d = 0; d < dim; ++d) o << " OUTS(" << out_off[v] + d << ", dv(p" << d << ", tot, yt));";
    o << " }\n        }\n";
}

// GetProbabilitiesOneNode for every variable whose selected clique (first with the fewest reduced
// variables) is c, and the label (ArgMax, strict '>' from 0; un-normalized if c reduces to one var)
void JTGen::Marg(const std::string &P, int c) {
    const Table &t = plan.cliques[c];
    for (size_t j = 0; j < t.vars.size(); ++j) {
        const int v = t.vars[j];
        const int dim = plan.dom[v];
        const int64_t cum = t.cum[j], bw = dim * cum, nhi = t.size() / bw;
        if (fast) {  // the smallest clique holding the variable (a calibrated tree: any gives the marginal)
            if (mclq[v] != c || msep[v] >= 0) continue;
            std::vector<std::vector<std::string>> terms(dim);
            for (int d = 0; d < dim; ++d)
                for (int64_t hi = 0; hi < nhi; ++hi)
                    for (int64_t l = 0; l < cum; ++l) terms[d].push_back(N(P, c, hi * bw + d * cum + l));
            MargTerms(v, terms);
            if (!in_merged) o << B(8);
            continue;
        } else {
            // selection: first candidate clique with the fewest reduced variables (recomputed here)
            o << "        { int b = " << R(cand[v][0]) << ", sl = " << cand[v][0] << ";";
            for (size_t k = 1; k < cand[v].size(); ++k)
                o << " { const int r = " << R(cand[v][k]) << "; if (r < b) { b = r; sl = " << cand[v][k] << "; } }";
            o << "\n        if (sl == " << c << " && !" << observed(v) << ") { // marginal of var " << v << "\n";
        }
        if (fast) {  // tree sums, branch-free reciprocal of the total
            std::vector<std::string> ps;
            for (int d = 0; d < dim; ++d) {
                std::vector<std::string> terms;
                for (int64_t hi = 0; hi < nhi; ++hi)
                    for (int64_t l = 0; l < cum; ++l) terms.push_back(N(P, c, hi * bw + d * cum + l));
                o << "          const double p" << d << " = " << TreeSum(terms) << ";\n";
                ps.push_back("p" + std::to_string(d));
            }
            o << "          const double tot = " << TreeSum(ps) << "; const double yt = frcp(tot); bad |= den_bad(tot);\n";
        } else {
            o << "          double tot = 0.0;";
            for (int d = 0; d < dim; ++d) o << " double p" << d << ";";
            o << "\n";
            for (int d = 0; d < dim; ++d) {
                bool first = true;
                o << "          { double a = ";
                for (int64_t hi = 0; hi < nhi; ++hi)
                    for (int64_t l = 0; l < cum; ++l) {
                        const int64_t e = hi * bw + d * cum + l;
                        o << (first ? "" : " a += ") << Val(P, c, e) << ";";
                        first = false;
                    }
                o << " p" << d << " = a; tot += a; }\n";
            }
            o << "          const double yt = 1.0 / tot; bad |= den_bad(tot);\n";
        }
        if (v == 0) {
            // (fast order: a near-tie, top two within 1e-12 relative, may break differently from the
            // reference's exact values -- the block is flagged for the exact pass)
            o << "          if (ACT) { int lab = 0; double mp = 0.0, m2 = 0.0;";
            for (int d = 0; d < dim; ++d)
                o << " { const double q = (b == 1) ? p" << d << " : dv(p" << d << ", tot, yt); if (q > mp) { m2 = mp; mp = q; lab = " << d
                  << "; } else if (q > m2) m2 = q; }";
            o << " labels[CS] = lab;" << (fast ? " bad |= (mp - m2 <= 1e-12 * mp) ? 1u : 0u;" : "") << " }\n";
        }
        o << "          if (ACT) {";
        for (int d = 0; d < dim; ++d) o << " OUTS(" << out_off[v] + d << ", dv(p" << d << ", tot, yt));";
        o << " }\n        } }\n" << (in_merged ? std::string() : B(8));
    }
}

// Message placement.  Every stored message has a live interval on the schedule's clock (Collect
// clique k of the post-order at time k, Distribute clique k of the pre-order at time nc + k): the
// Collect message of separator s from its child's Collect to its parent's Distribute, the
// Distribute message from the parent's Distribute to the child's.  The per-wave workspace of all
// of them (ALARM: 265 rows = 136 KB per wave, 139 MB for 1,024 waves) does not stay in L2, and each
// row written twice per block left L2 twice (PMC, round 5: 0.49 GB written per 100k cases, the
// kernel 20 % slower than with the workspace L2-resident).  So the LDS left over by the clique tail
// and the initial potentials (the budget of four waves per CU) holds a pool of rows, and messages
// get pool rows by interval: shortest intervals first while the pool has room at every time of
// the interval, rows then assigned in start order (an interval graph: the room suffices).  The
// rest keep global rows (Collect and Distribute message of a separator in the same rows, as
// before).  FBN_JT_LDS_POOL=n caps the pool at n rows (0: off).  Before the LDS pool, the fast order
// parks message entries in registers the small cliques leave unused (reg_cap rows at most, 0: off);
// a message may be split: its leading entries in registers, the others in one of the two memories.
void JTGen::PlaceMessages(const std::vector<int> &post, const std::vector<int> &pre, int64_t budget, int64_t reg_cap,
                          bool quiet) {
    const int nc = (int)plan.cliques.size(), ns = (int)plan.seps.size();
    auto tsize = [&](int c) { return plan.cliques[c].size(); };
    std::vector<int> pi(nc), qi(nc);
    for (int k = 0; k < nc; ++k) qi[post[k]] = k, pi[pre[k]] = k;
    md_reg.assign(ns, false);
    for (int c : pre)
        if (!plan.clique_down[c].empty()) {
            // the child Distribute visits first (the next clique of the pre-order)
            const int q = pre[pi[c] + 1], s = plan.clique_up[q];
            int64_t mk = 0;
            for (int s2 : plan.clique_down[q]) mk = std::max<int64_t>(mk, plan.seps[s2].size());
            md_reg[s] = tsize(q) + plan.seps[s].size() + mk <= budget;
        }
    const bool no_leaf_rc = KnobOr("FBN_JT_LEAF_RC", 0) == 0;
    leaf_rc.assign(ns, false);
    col_store.assign(ns, true);
    for (int s = 0; s < ns; ++s) {
        const int c = plan.sep_down[s], p = plan.sep_up[s];
        if (!fast || no_leaf_rc || !plan.clique_down[c].empty() || tsize(c) > 64) continue;
        leaf_rc[s] = true;
        // the parent's Collect takes the last child's message from registers when that child ran
        // just before it (Run's collect_loads)
        col_store[s] = !(qi[p] > 0 && post[qi[p] - 1] == c);
    }
    struct Item {
        int s;
        bool dist;
        int a, b;  // live interval [a, b]
        int64_t n;
    };
    std::vector<Item> items;
    for (int s = 0; s < ns; ++s) {
        const int c = plan.sep_down[s], p = plan.sep_up[s];
        if (!leaf_rc[s]) items.push_back({s, false, qi[c], nc + pi[p], plan.seps[s].size()});
        else if (col_store[s]) items.push_back({s, false, qi[c], qi[p], plan.seps[s].size()});
        if (!md_reg[s]) items.push_back({s, true, nc + pi[p], nc + pi[c], plan.seps[s].size()});
    }
    std::vector<int> order(items.size());
    for (size_t i = 0; i < items.size(); ++i) order[i] = (int)i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
        return items[x].b - items[x].a < items[y].b - items[y].a;
    });
    // Register pool (fast order, FBN_JT_REG_POOL): the leading nreg[i] entries of message i stay in
    // named registers for its whole interval.  An op needs its table (the register-resident part)
    // and the messages it loads, prefetches or keeps (need[t], the same rules Run emits by); what
    // is left of the 256 fp64 values per lane, less a slack for temporaries, may hold parked rows
    // at that time.  A message is checked at its producer (which would otherwise store each entry
    // as it is formed) and at every op before its consumer; an op that loads it on the way anyway
    // (the parent's Collect of a message parked until the parent's Distribute, a prefetch) pays
    // nothing extra for it.
    std::vector<int64_t> nreg(items.size(), 0);
    reg_extra.assign(2 * nc + 1, 0);
    if (reg_cap > 0) {
        auto kids_rows = [&](int c) {
            int64_t r = 0;
            for (int s : plan.clique_down[c]) r += plan.seps[s].size();
            return r;
        };
        auto early_lb = [&](int c) {
            const int64_t held = (plan.clique_up[c] >= 0) ? plan.seps[plan.clique_up[c]].size() : 0;
            return tsize(c) + kids_rows(c) + held <= budget;
        };
        std::vector<int64_t> need(2 * nc + 1, 0);
        std::vector<std::vector<int>> touch(2 * nc + 1);  // messages op t holds anyway: 2 * s + dist
        for (int k = 0; k < nc; ++k) {  // Collect
            const int c = post[k];
            need[k] = std::min<int64_t>(tsize(c), kRegEntries) + kids_rows(c);
            int64_t mine = 0;
            for (int s : plan.clique_down[c]) {
                touch[k].push_back(2 * s);
                if (!(k > 0 && child(s) == post[k - 1])) mine += plan.seps[s].size();
            }
            if (k + 1 < nc) {
                const int nx = post[k + 1];
                int64_t next = 0;
                for (int s : plan.clique_down[nx])
                    if (child(s) != c) next += plan.seps[s].size();
                if (tsize(c) + mine + next <= budget) {
                    need[k] += next;
                    for (int s : plan.clique_down[nx])
                        if (child(s) != c) touch[k].push_back(2 * s);
                }
            }
        }
        for (int k = 0; k < nc; ++k) {  // Distribute
            const int c = pre[k], up = plan.clique_up[c], t = nc + k;
            const bool early = early_lb(c);
            int64_t kmax = 0, pend = early ? kids_rows(c) : 0;
            for (int s : plan.clique_down[c]) {
                kmax = std::max<int64_t>(kmax, plan.seps[s].size());
                touch[t].push_back(2 * s);
                if (md_reg[s]) need[t] += plan.seps[s].size();
            }
            need[t] += std::min<int64_t>(tsize(c), kRegEntries) + (early ? kids_rows(c) : kmax);
            if (up >= 0) {
                need[t] += plan.seps[up].size();
                touch[t].push_back(2 * up + 1);
                if (md_reg[up]) pend += plan.seps[up].size();
            }
            if (k + 1 < nc) {
                const int nx = pre[k + 1], nup = plan.clique_up[nx];  // (nup < 0: the next tree's root)
                const bool ld_next = nup >= 0 && !md_reg[nup] && plan.sep_up[nup] != c;
                const int64_t nrows = (early_lb(nx) ? kids_rows(nx) : 0) + (ld_next ? plan.seps[nup].size() : 0);
                if (tsize(c) + pend + nrows <= budget) {
                    need[t] += nrows;
                    if (early_lb(nx))
                        for (int s : plan.clique_down[nx]) touch[t].push_back(2 * s);
                    if (ld_next) touch[t].push_back(2 * nup + 1);
                }
            }
        }
        peak_need = *std::max_element(need.begin(), need.end());
        const int64_t slack = vmajor ? kRegSlackVM : kRegSlackCM;
        std::vector<int64_t> live(2 * nc + 1, 0);  // parked rows by time (the cap)
        for (int i : order) {
            const Item &it = items[i];
            const int id = 2 * it.s + (it.dist ? 1 : 0);
            int64_t room = it.n;
            for (int t = it.a; t <= it.b; ++t) room = std::min(room, reg_cap - live[t]);
            std::vector<int> pay;  // the times this message costs registers of its own
            for (int t = it.a; t < it.b; ++t)
                if (t == it.a || std::find(touch[t].begin(), touch[t].end(), id) == touch[t].end()) pay.push_back(t);
            for (int t : pay) room = std::min(room, kRegFile - slack - need[t] - reg_extra[t]);
            if (room <= 0) continue;
            nreg[i] = room;
            for (int t = it.a; t <= it.b; ++t) live[t] += room;
            for (int t : pay) reg_extra[t] += room;
        }
        if (!quiet && KnobSet("FBN_JT_PLACE_DEBUG")) {
            std::string u;
            for (int t = 0; t < 2 * nc; ++t)
                u += std::to_string(need[t]) + "+" + std::to_string(reg_extra[t]) + (t == nc - 1 ? " | " : " ");
            fprintf(stderr, "register rows by time, the op's own + parked (Collect | Distribute): %s\n", u.c_str());
        }
    }
    // room: the LDS of four waves per CU (160 KB) less the clique tail and the initial potentials
    const int64_t per_wave = 160 * 1024 / 4 / 8;  // fp64 values
    int64_t ivn = 0;
    for (const auto &t : plan.cliques) ivn += t.size();
    int64_t cap = std::max<int64_t>(0, (per_wave - lds_rows * 64 - (iv_lds ? ivn : 0)) / 64);
    if (const char *e = KnobValue("FBN_JT_LDS_POOL")) cap = std::min<int64_t>(cap, std::max(0, atoi(e)));
    std::vector<int64_t> use(2 * nc + 1, 0);
    std::vector<bool> in_lds(items.size(), false);
    for (int i : order) {
        const Item &it = items[i];
        const int64_t n = it.n - nreg[i];  // (the rows not in registers)
        if (n == 0 || n > cap) continue;
        int64_t mx = 0;
        for (int t = it.a; t <= it.b; ++t) mx = std::max(mx, use[t]);
        if (mx + n > cap) continue;
        for (int t = it.a; t <= it.b; ++t) use[t] += n;
        in_lds[i] = true;
    }
    // concrete pool rows, in start order
    std::vector<int> byst;
    for (size_t i = 0; i < items.size(); ++i)
        if (in_lds[i]) byst.push_back((int)i);
    std::stable_sort(byst.begin(), byst.end(), [&](int x, int y) { return items[x].a < items[y].a; });
    std::vector<std::vector<int64_t>> rows_of(items.size());
    std::vector<int64_t> free_rows;
    for (int64_t r = cap - 1; r >= 0; --r) free_rows.push_back(r);  // (pop_back takes the lowest)
    std::vector<int> active;
    pool_rows = 0;
    for (int i : byst) {
        const Item &it = items[i];
        for (size_t k = 0; k < active.size();) {  // release intervals that ended before this one
            if (items[active[k]].b < it.a) {
                for (int64_t r : rows_of[active[k]]) free_rows.push_back(r);
                std::sort(free_rows.rbegin(), free_rows.rend());
                active.erase(active.begin() + k);
            } else {
                ++k;
            }
        }
        for (int64_t j = nreg[i]; j < it.n; ++j) {
            rows_of[i].push_back(free_rows.back());
            pool_rows = std::max<int64_t>(pool_rows, free_rows.back() + 1);
            free_rows.pop_back();
        }
        active.push_back(i);
    }
    col_loc.assign(ns, {});
    dis_loc.assign(ns, {});
    sep_row.assign(ns, -1);
    reg_names.clear();
    // global rows of a separator: shared by both its messages, entry j in row sep_row + j - sep_skip
    // (sep_skip: leading entries neither message keeps there)
    std::vector<int64_t> sep_skip(ns, 0);
    for (int s = 0; s < ns; ++s) sep_skip[s] = plan.seps[s].size();
    for (size_t i = 0; i < items.size(); ++i)
        if (!in_lds[i]) sep_skip[items[i].s] = std::min(sep_skip[items[i].s], nreg[i]);
    int64_t grow = 0;
    place = JTPlacement();
    for (size_t i = 0; i < items.size(); ++i) {
        const Item &it = items[i];
        auto &loc = it.dist ? dis_loc[it.s] : col_loc[it.s];
        loc.assign(it.n, std::string());
        for (int64_t j = 0; j < nreg[i]; ++j) {
            loc[j] = (it.dist ? "rd" : "rc") + std::to_string(it.s) + "_" + std::to_string(j);
            reg_names.push_back(loc[j]);
        }
        place.reg[it.dist] += nreg[i];
        if (in_lds[i]) {
            for (int64_t j = nreg[i]; j < it.n; ++j) loc[j] = "LP(" + std::to_string(rows_of[i][j - nreg[i]]) + ")";
            place.lds[it.dist] += it.n - nreg[i];
            continue;
        }
        if (nreg[i] == it.n) continue;
        if (sep_row[it.s] < 0) sep_row[it.s] = grow, grow += it.n - sep_skip[it.s];  // (shared by both messages)
        for (int64_t j = nreg[i]; j < it.n; ++j) loc[j] = "W(" + std::to_string(sep_row[it.s] + j - sep_skip[it.s]) + "LL)";
        place.global[it.dist] += it.n - nreg[i];
    }
    place.workspace_rows = grow;
    place.lds_pool_rows = pool_rows;
    for (int s = 0; s < ns; ++s) {
        if (sep_row[s] < 0) sep_row[s] = 0;
        if (dis_loc[s].empty()) dis_loc[s].assign(plan.seps[s].size(), "0.0");  // (in registers: never read)
        if (col_loc[s].empty()) col_loc[s].assign(plan.seps[s].size(), "0.0");  // (recomputed: never read)
    }
    if (!quiet && KnobSet("FBN_JT_PLACE_DEBUG")) {  // diagnostic: the placement's summary
        int64_t leaf = 0;
        for (int s = 0; s < ns; ++s)
            if (plan.clique_down[plan.sep_down[s]].empty()) leaf += plan.seps[s].size();
        fprintf(stderr, "placement: pool %lld of %lld rows; Collect rows LDS %lld global %lld; Distribute rows LDS %lld "
                        "global %lld (registers: the rest); global rows %lld; leaf-separator rows %lld\n",
                (long long)pool_rows, (long long)cap, (long long)place.lds[0], (long long)place.global[0],
                (long long)place.lds[1], (long long)place.global[1], (long long)grow, (long long)leaf);
        if (reg_cap > 0)
            fprintf(stderr, "register pool (cap %lld rows): Collect rows %lld, Distribute rows %lld\n", (long long)reg_cap,
                    (long long)place.reg[0], (long long)place.reg[1]);
        std::string u;
        for (int t = 0; t <= 2 * nc; ++t) u += std::to_string(use[t]) + (t == nc - 1 ? " | " : " ");
        fprintf(stderr, "pool rows in use by time (Collect | Distribute): %s\n", u.c_str());
        if (fast) {
            std::string m;
            for (int v = 0; v < (int)plan.dom.size(); ++v) {
                const int t = msep[v] >= 0 ? nc + pi[plan.sep_up[msep[v]]] : nc + pi[mclq[v]];
                m += std::to_string(v) + ":" + std::to_string(t) + " ";
            }
            fprintf(stderr, "marginal time per variable: %s\n", m.c_str());
        }
    }
}

int JTGen::Run(std::string &src, int64_t *wave_entries, std::vector<double> &initv) {
    const int nc = (int)plan.cliques.size(), ns = (int)plan.seps.size(), V = plan.num_nodes;
    profile = KnobOr("FBN_JT_PROFILE", 0) != 0;  // diagnostic build
    marg_v2 = fast && KnobOr("FBN_JT_MARG_V2", 1) != 0;
    lds_rows = 0;
    for (const auto &t : plan.cliques) lds_rows = std::max<int64_t>(lds_rows, t.size() - kRegEntries);
    // initial potentials: one constant buffer, read with wave-uniform (scalar) loads
    initv.clear();
    init_off.assign(nc, 0);
    for (int c = 0; c < nc; ++c) {
        init_off[c] = (int64_t)initv.size();
        initv.insert(initv.end(), plan.cliques[c].pot.begin(), plan.cliques[c].pot.end());
    }
    int SD = 0;
    out_off.assign(V, 0);
    for (int v = 0; v < V; ++v) out_off[v] = SD, SD += plan.dom[v];
    cand.assign(V, {});
    for (int c = 0; c < nc; ++c)
        for (int v : plan.cliques[c].vars) cand[v].push_back(c);
    home.assign(V, -1);
    for (int v = 0; v < V; ++v)
        for (int q : cand[v])
            if (home[v] < 0 || plan.cliques[q].size() < plan.cliques[home[v]].size()) home[v] = q;
    msep.assign(V, -1);
    if (fast)
        for (int sp = 0; sp < ns; ++sp)
            for (int v : plan.seps[sp].vars) {
                const int64_t have = msep[v] >= 0 ? plan.seps[msep[v]].size() : plan.cliques[home[v]].size();
                if (plan.seps[sp].size() < have) msep[v] = sp;
            }
    mclq = home;
    // traversal orders: Collect in post-order, Distribute in pre-order of a DFS.  Any child order
    // gives the same values (schedule freedom, section 4 of DESIGN.md).
    // With the register pool on, the child order of each phase is chosen by the placement itself:
    // the plan's, heaviest subtree (sum of clique entries) first, or heaviest last -- whichever
    // leaves the fewest message rows in global memory (a tie keeps the earlier candidate, the
    // plan's order first).  Products and sums keep the plan's child order whatever is visited first.
    std::vector<int64_t> weight(nc, 0);
    {
        std::function<int64_t(int)> w = [&](int c) {
            weight[c] = plan.cliques[c].size();
            for (int s : plan.clique_down[c]) weight[c] += w(child(s));
            return weight[c];
        };
        for (int r : plan.roots) w(r);
    }
    // visit: 0 = plan order, 1 = heaviest subtree first, 2 = heaviest subtree last
    auto dfs = [&](bool collect, int visit, std::vector<int> &post_o, std::vector<int> &pre_o) {
        std::vector<std::vector<int>> kids(nc);
        for (int c = 0; c < nc; ++c) {
            kids[c] = plan.clique_down[c];
            if (visit)
                std::stable_sort(kids[c].begin(), kids[c].end(), [&](int x, int y) {
                    return visit == 1 ? weight[child(x)] > weight[child(y)] : weight[child(x)] < weight[child(y)];
                });
        }
        // a forest: tree after tree -- Collect in component order, Distribute in the reverse, so the
        // root collected last is the one distributed first (it continues from its Collect registers)
        std::vector<int> roots = plan.roots;
        if (!collect) std::reverse(roots.begin(), roots.end());
        std::vector<std::pair<int, size_t>> st;
        size_t next_root = 0;
        while (!st.empty() || next_root < roots.size()) {  // iterative DFS
            if (st.empty()) st.push_back({roots[next_root++], 0});
            auto &top = st.back();
            const int c = top.first;
            if (top.second == 0) pre_o.push_back(c);
            if (top.second < kids[c].size()) {
                const int ch = child(kids[c][top.second++]);
                st.push_back({ch, 0});
            } else {
                post_o.push_back(c);
                st.pop_back();
            }
        }
    };
    std::vector<int> post, pre, unused;
    dfs(true, 0, post, unused);
    unused.clear();
    dfs(false, 0, unused, pre);
    if ((int)post.size() != nc) return SetError(FBN_ERR_LIMIT, "codegen: tree traversal covers %zu of %d cliques", post.size(), nc);
    // fp64 values per lane: table in flight + prefetched rows
    // (fast order: 260 -- round 5 sweep 150 / 200 / 260 / 320: 0.171 / 0.169 / 0.165 / 0.166 ms)
    const int64_t kBudget = fast ? 260 : 200;
    // register pool: fast order only (the exact order's source is pinned); on by default for the
    // variable-major kernel only (the case-major one is faster with it too, but spills more SGPRs)
    int64_t reg_cap = fast && vmajor ? kDefaultRegPool : 0;
    if (const char *e = KnobValue("FBN_JT_REG_POOL")) reg_cap = fast ? std::max(0, atoi(e)) : 0;
    sched = reg_cap > 0 && KnobOr("FBN_JT_SCHED", 1) != 0;
    if (reg_cap > 0) {
        int64_t best = -1, plan_peak = 0;
        int bvc = 0, bvd = 0;
        std::vector<int> bpost = post, bpre = pre;
        for (int vc = 0; vc < 3; ++vc)
            for (int vd = 0; vd < 3; ++vd) {
                std::vector<int> po, pr, un;
                dfs(true, vc, po, un);
                un.clear();
                dfs(false, vd, un, pr);
                PlaceMessages(po, pr, kBudget, reg_cap, true);
                // (an order whose ops themselves need more registers than the plan order's at their
                // peak is left out: the plan order's peak already fills the register file)
                if (best < 0) plan_peak = peak_need;
                else if (peak_need > plan_peak) continue;
                const int64_t g = place.global[0] + place.global[1];
                if (best < 0 || g < best) best = g, bpost = po, bpre = pr, bvc = vc, bvd = vd;
            }
        post = bpost, pre = bpre;
        if (KnobSet("FBN_JT_PLACE_DEBUG"))
            fprintf(stderr, "child order (0 plan, 1 heaviest subtree first, 2 last): Collect %d, Distribute %d\n", bvc, bvd);
    }
    PlaceMessages(post, pre, kBudget, reg_cap, false);
    int64_t rows = 0;
    for (int s = 0; s < ns; ++s) rows = std::max<int64_t>(rows, sep_row[s] + plan.seps[s].size());
    *wave_entries = std::max<int64_t>(rows, 1);

    o << "// generated by libfastbn (jt_codegen.cpp): " << nc << " cliques, " << ns << " separators, "
      << (fast ? "fast" : "exact") << " arithmetic order\n";
    o << "#define FBN_V " << V << "\n#define FBN_SD " << SD << "\n#define FBN_WE " << *wave_entries << "LL\n";
    o << "#define FBN_LP_BASE " << lds_rows << "\n";
    o << "#define FBN_IV_BASE " << (lds_rows + pool_rows) * 64 << "\n#define FBN_NIV " << initv.size() << "\n";
    o << "#define FBN_IV_LDS " << (iv_lds ? 1 : 0) << "\n#define FBN_MIN_WAVES " << min_waves << "\n";
    if (vmajor) o << "#define FBN_VMAJOR 1\n";
    // (FBN_NO_OUT and FBN_WS_FOLD below are never defined: two retired diagnostic builds whose
    // inert text stays, because the code-object cache key is a hash of this source and
    // tests/test_jt_regpool_codegen.py pins the keys)
    o << R"FBN(typedef signed char i8;
__device__ __forceinline__ double dv(double x, double den, double y) {  // x / den (Markstein, see jt_kernels.hip)
    const double q = x * y;
    const double r = __builtin_fma(-den, q, x);
    return __builtin_fma(r, y, q);
}
// row r of the per-wave workspace, this lane: uniform row base (SGPRs) + lane byte offset (VGPR)
typedef __attribute__((address_space(1))) double gdouble;
typedef __attribute__((address_space(1))) char gchar;
typedef __attribute__((address_space(4))) const double cdouble;
#define W(row) (*(gdouble *)((gchar *)(Wb + (row) * 64) + (unsigned long long)lo))
// LDS row of the clique in flight (entries beyond the register-resident part of large tables)
typedef __attribute__((address_space(3))) double ldouble;
extern __shared__ double fbn_lds[];
#define L(row) (ltail[(row) * 64])
// LDS message pool row (after the clique tail)
#define LP(row) (ltail[(FBN_LP_BASE + (row)) * 64])
// initial potentials: copied into LDS once per wave (wave-uniform address: broadcast reads), or
// read with scalar loads from the constant buffer
#if FBN_IV_LDS
#define IV(k) (ivl[k])
#else
#define IV(k) (ivc[k])
#endif
// unconditional (LDS broadcast) load + select: no branch per table entry
__device__ __forceinline__ double sel(bool c, double v) { return c ? v : 0.0; }
#define FBN_STAMP(k) do { unsigned long long t_; __asm__ volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); pacc[k] += t_ - tprev; tprev = t_; } while (0)
__device__ __forceinline__ unsigned den_bad(double d) { return (d >= 0x1p-600 && d <= 0x1p+600) ? 0u : 1u; }
// fast order: 1 / x as v_rcp_f64 + one Newton step (relative error <= 2.3e-15 over 2^-60..2^60,
// tools/micro/fp64_ilp.hip), branch-free, so independent reciprocals overlap; the operands are
// range-checked by den_bad (a block outside [2^-600, 2^600] goes to the exact pass)
__device__ __forceinline__ double frcp(double x) {
    const double r = __builtin_amdgcn_rcp(x);
    return __builtin_fma(r, __builtin_fma(-x, r, 1.0), r);
}
// this lane's case / output row, recomputed per segment from the (laundered) block index
#define CS (blkl * 64 + lane)
#define ACT (CS < ncases)
#ifdef FBN_VMAJOR
// variable-major output [SD][ncases]: value k of every case is one column, so a store instruction
// writes 64 consecutive cases = 512 contiguous bytes (4 full lines) instead of one value into 64
// lines.  Through a buffer resource: voffset = the lane's case (bytes), soffset = column k (bytes,
// one scalar multiply) -- 64-bit column addresses measured 10 % more instructions and SGPR spills.
// (The host takes this kernel only when ncases * SD * 8 < 2^31.)
typedef unsigned fbn_u2v __attribute__((ext_vector_type(2)));
#ifdef FBN_NO_OUT
#define OUTS(k, v) do { if (ncases < 0) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(fbn_u2v, (double)(v)), mrs, (int)(CS * 8), (int)(k) * mcb, 0); } while (0)
#else
#define OUTS(k, v) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(fbn_u2v, (double)(v)), mrs, (int)(CS * 8), (int)(k) * mcb, 0)
#endif
#else
#define OUT(k) (marg[CS * FBN_SD + (k)])
#ifdef FBN_NO_OUT  // diagnostic only (FBN_JT_NO_OUT=1): marginals computed, never stored
#define OUTS(k, v) do { if (ncases < 0) OUT(k) = (v); } while (0)
#else
#define OUTS(k, v) (OUT(k) = (v))  // (non-temporal stores measured 2.1x slower: partial lines)
#endif
#endif
#ifdef FBN_VMAJOR
#define OUTS2(k, a, b) do { OUTS(k, a); OUTS((k) + 1, b); } while (0)
#else
// two adjacent output values in one 16-byte store (8-byte aligned: the rows are 8 * FBN_SD bytes)
typedef double fbn_d2u __attribute__((ext_vector_type(2), aligned(8)));
#ifdef FBN_NO_OUT
#define OUTS2(k, a, b) do { if (ncases < 0) *(fbn_d2u *)&OUT(k) = (fbn_d2u){(a), (b)}; } while (0)
#else
#define OUTS2(k, a, b) (*(fbn_d2u *)&OUT(k) = (fbn_d2u){(a), (b)})
#endif
#endif
extern "C" __global__ void __launch_bounds__(64, FBN_MIN_WAVES)
fbn_jt_gen(const i8 *__restrict__ evid, double *__restrict__ marg, int *__restrict__ labels,
           double *__restrict__ ws, int *__restrict__ flags, const double *ivp, long long ncases,
           unsigned long long *__restrict__ prof) {
    const int lane = threadIdx.x;
    // LDS bases are laundered at every op boundary (so addresses fold into ds_* offsets instead of
    // being hoisted as loop-invariant constants)
    ldouble *ltail = (ldouble *)fbn_lds + lane;
#if FBN_IV_LDS
    ldouble *ivl = (ldouble *)fbn_lds + FBN_IV_BASE;
    for (int k = lane; k < FBN_NIV; k += 64) IV(k) = ivp[k];
    __syncthreads();
#else
    const cdouble *ivc = (const cdouble *)ivp;
    ldouble *ivl = (ldouble *)fbn_lds;  // unused (laundered at op boundaries)
#endif
    unsigned long long pacc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, tprev = __builtin_amdgcn_s_memtime();
#ifdef FBN_WS_FOLD
    gdouble *Wb = (gdouble *)ws + (unsigned long long)(blockIdx.x % FBN_WS_FOLD) * FBN_WE * 64;
#else
    gdouble *Wb = (gdouble *)ws + (unsigned long long)blockIdx.x * FBN_WE * 64;
#endif
    unsigned lo = (unsigned)lane * 8;
#ifdef FBN_VMAJOR
    const __amdgpu_buffer_rsrc_t mrs = __builtin_amdgcn_make_buffer_rsrc(marg, 0, 0x7FFFFFFF, 0x00020000);
    const int mcb = (int)ncases * 8;  // column stride, bytes
#endif
    for (long long blk = blockIdx.x; blk * 64 < ncases; blk += gridDim.x) {
        long long blkl = blk;
        const long long cs = blk * 64 + lane;
        const long long csr = cs < ncases ? cs : ncases - 1;
        const i8 *__restrict__ ev = evid + csr * FBN_V;
        unsigned bad = 0u;  // laundered at op boundaries: checked where computed, never deferred
        double den, y;
)FBN";
    // evidence: allowed-value bits of every variable packed into 32-bit words (okw<k>), observed
    // flags (obs<k>); var v owns bits [pos, pos + dom) of its word
    okw_word.assign(V, 0);
    okw_pos.assign(V, 0);
    int nokw = 0;
    {
        int pos = 32;
        for (int v = 0; v < V; ++v) {
            if (pos + plan.dom[v] > 32) ++nokw, pos = 0;
            okw_word[v] = nokw - 1, okw_pos[v] = pos, pos += plan.dom[v];
        }
    }
    nobs = (V + 31) / 32;
    // op boundary: no store->load forwarding, no hoisting of addresses, no scheduling across it,
    // and the evidence words are opaque per segment, so a Distribute recomputation is not merged
    // with (and kept live from) its Collect twin
    {
        std::vector<std::string> regs;
        for (int k = 0; k < nokw; ++k) regs.push_back("okw" + std::to_string(k));
        for (int k = 0; k < nobs; ++k) regs.push_back("obs" + std::to_string(k));
        o << "#define FBN_OP_BOUNDARY() do { __asm__ volatile(\"\" : \"+s\"(Wb), \"+v\"(lo), \"+v\"(ltail), \"+v\"(ivl), \"+v\"(bad), \"+s\"(blkl) :: \"memory\");";
        for (size_t i = 0; i < regs.size(); i += 16) {
            o << " __asm__ volatile(\"\" :";
            for (size_t k = i; k < std::min(regs.size(), i + 16); ++k) o << (k > i ? ", " : " ") << "\"+v\"(" << regs[k] << ")";
            o << ");";
        }
        o << " __builtin_amdgcn_sched_barrier(0); } while (0)\n";
    }
    if (sched)  // batches of initial potentials as vectors (IvLoads)
        for (int n = 2; n <= 16; n *= 2)
            o << "        typedef double fbn_w" << n << " __attribute__((ext_vector_type(" << n << "), aligned(8)));"
              << " typedef __attribute__((address_space(4))) fbn_w" << n << " fbn_cw" << n << ";\n";
    for (int k = 0; k < nokw; ++k) o << "        unsigned okw" << k << " = 0u;\n";
    for (int k = 0; k < nobs; ++k) o << "        unsigned obs" << k << " = 0u;\n";
    // message entries parked in registers: one per block iteration, assigned by the op that forms
    // the message before any op reads it; not in the boundaries' operand lists (free to sit in AGPRs)
    for (size_t i = 0; i < reg_names.size(); i += 8) {
        o << "        double";
        for (size_t k = i; k < std::min(reg_names.size(), i + 8); ++k) o << (k > i ? ", " : " ") << reg_names[k];
        o << ";\n";
    }
    for (int v = 0; v < V; ++v) {
        const unsigned full = (plan.dom[v] >= 32) ? 0xFFFFFFFFu : ((1u << plan.dom[v]) - 1u);
        o << "        { const int x = ev[" << v << "]; okw" << okw_word[v] << " |= (x < 0 ? " << full << "u : (1u << x)) << "
          << okw_pos[v] << "; obs" << v / 32 << " |= (x >= 0 ? 1u : 0u) << " << v % 32 << "; }\n";
    }
    o << B(0);

    auto tsize = [&](int c) { return plan.cliques[c].size(); };
    // ---------------- Collect, DFS post-order
    // loads of clique post[k]: its children's messages except a last child that is post[k-1]
    auto collect_loads = [&](size_t k, std::vector<int> &ls) {
        ls.clear();
        const int c = post[k];
        const auto &down = plan.clique_down[c];
        for (size_t i = 0; i < down.size(); ++i)
            if (!(k > 0 && child(down[i]) == post[k - 1])) ls.push_back(down[i]);  // (the child just collected: registers)
    };
    auto rows_of = [&](const std::vector<int> &ls) {
        int64_t r = 0;
        for (int s : ls) r += plan.seps[s].size();
        return r;
    };
    // The root collected last stays in registers for its Distribute.  Every other root of a forest
    // sends no message, so its Collect is left out; its Distribute recomputes the table like any
    // clique's, from the initial potential and the children's stored messages.
    const int cont_root = post.back() == pre.front() ? pre.front() : -1;
    std::vector<bool> loaded_a(ns, false);
    for (size_t k = 0; k < post.size(); ++k) {
        const int c = post[k];
        if (plan.clique_up[c] < 0 && c != cont_root) continue;
        std::vector<int> mine, next;
        collect_loads(k, mine);
        o << "        // ---- collect clique " << c << " (" << tsize(c) << " entries)\n";
        for (int s : mine)
            if (!loaded_a[s]) Load("la", s), loaded_a[s] = true;
        const bool next_runs = k + 1 < post.size() && (plan.clique_up[post[k + 1]] >= 0 || post[k + 1] == cont_root);
        if (next_runs) {  // prefetch for the next clique
            collect_loads(k + 1, next);
            int64_t pend = 0;
            for (int s : mine) pend += plan.seps[s].size();
            if (tsize(c) + pend + rows_of(next) + reg_extra[k] <= kBudget)  // (less the parked rows live now)
                for (int s : next)
                    if (!loaded_a[s]) Load("la", s), loaded_a[s] = true;
        }
        if (fast && sched) IvFirst("t", c);
        o << B(1);
        const auto &down = plan.clique_down[c];
        if (fast) {
            std::vector<std::pair<int, std::string>> kids;
            for (int s : down) kids.push_back({s, loaded_a[s] ? "la" : "mc"});
            InitProd("t", c, kids, -1, "");
        } else {
            Init("t", c);
            for (size_t i = 0; i < down.size(); ++i) {
                const int s = down[i];
                Mul("t", c, s, loaded_a[s] ? "la" : "mc");
            }
        }
        if (c != cont_root) SepCol("t", c, plan.clique_up[c], col_store[plan.clique_up[c]]);
    }
    // ---------------- Distribute, DFS pre-order (root continues from its Collect registers)
    // Register policy (kBudget fp64 values per lane):
    //  * the message to a first child stays in registers if that child's table, the message and
    //    its largest child message fit; otherwise it is stored and loaded ("ld") right before DMul
    //  * a clique's children's Collect messages ("lb") are loaded at its start (or prefetched by
    //    the previous clique) if they fit next to its table; otherwise each is loaded right before
    //    its Mul and loaded again ("lc") right before its SepDis
    auto kids_rows = [&](int c) {
        int64_t r = 0;
        for (int s : plan.clique_down[c]) r += plan.seps[s].size();
        return r;
    };
    auto early_lb = [&](int c) {
        const int up = plan.clique_up[c];
        const int64_t held = (up >= 0) ? plan.seps[up].size() : 0;  // in registers at DMul either way
        return tsize(c) + kids_rows(c) + held <= kBudget;
    };
    std::vector<bool> loaded_b(ns, false), loaded_d(ns, false);
    for (size_t k = 0; k < pre.size(); ++k) {
        const int c = pre[k];
        const int up = plan.clique_up[c];
        const bool early = early_lb(c);
        o << "        // ---- distribute clique " << c << " (" << tsize(c) << " entries)\n";
        int64_t pend = 0;
        if (early)
            for (int s : plan.clique_down[c]) {
                if (!loaded_b[s]) LoadCol("lb", s), loaded_b[s] = true;
                pend += plan.seps[s].size();
            }
        if (up >= 0 && md_reg[up]) pend += plan.seps[up].size();
        if (k + 1 < pre.size()) {  // prefetch for the next clique (before this clique's stores)
            const int nx = pre[k + 1], nup = plan.clique_up[nx];
            // its parent message, unless still in registers or produced by this clique (or it has
            // none: the next tree's root)
            const bool ld_next = nup >= 0 && !md_reg[nup] && plan.sep_up[nup] != c;
            const int64_t nrows = (early_lb(nx) ? kids_rows(nx) : 0) + (ld_next ? plan.seps[nup].size() : 0);
            if (tsize(c) + pend + nrows + reg_extra[nc + k] <= kBudget) {
                if (early_lb(nx))
                    for (int s : plan.clique_down[nx])
                        if (!loaded_b[s] && !leaf_rc[s]) Load("lb", s), loaded_b[s] = true;
                if (ld_next && !loaded_d[nup]) Load("ld", nup), loaded_d[nup] = true;
            }
        }
        if (c != cont_root && fast && early && sched) IvFirst("u", c);
        o << B(1);
        std::string P = "t";
        if (c != cont_root && fast && early) {  // all messages in registers: one fused op
            P = "u";
            if (up >= 0 && !md_reg[up] && !loaded_d[up]) Load("ld", up), loaded_d[up] = true, o << B(1);
            std::vector<std::pair<int, std::string>> kids;
            for (int s : plan.clique_down[c]) kids.push_back({s, "lb"});
            InitProd(P, c, kids, up, up < 0 ? "" : md_reg[up] ? "md" : "ld");
        } else if (c != cont_root) {
            P = "u";  // recompute the Collect table (same ops, same order -> same bits)
            Init(P, c);
            for (int s : plan.clique_down[c]) {
                if (!early) LoadCol("lb", s), o << B(1);
                Mul(P, c, s, "lb");
            }
            if (up >= 0) {
                if (!md_reg[up] && !loaded_d[up]) Load("ld", up), loaded_d[up] = true, o << B(1);
                DMul(P, c, up, md_reg[up] ? "md" : "ld");
            }
        }
        const auto &down = plan.clique_down[c];
        // consumers of the normalized table: one SepDis per child, one marginal per variable
        // (fast order: each SepDis takes the clique total from its own bin sums)
        if (!fast && down.size() + plan.cliques[c].vars.size() >= 2) Normalize(P, c);
        in_merged = fast && early;
        for (size_t i = 0; i < down.size(); ++i) {
            if (!early) LoadCol("lc", down[i]), o << B(1);
            SepDis(P, c, down[i], early ? "lb" : "lc", !md_reg[down[i]]);
        }
        Marg(P, c);
        if (in_merged) o << B(8);
        in_merged = false;
    }
    // an observed query: label 0, the ArgMax of its row of zeros (the unbranched marginals write the
    // label of the other lanes only; here, at the block's end, the store costs the ALARM kernel nothing)
    if (marg_v2) o << "        if (ACT && " << observed(0) << ") labels[CS] = 0;\n";
    for (int v = 0; v < V && !marg_v2; ++v) {  // (unbranched marginals store the zeros themselves)
        o << "        if (ACT && " << observed(v) << ") {";
        for (int d = 0; d < plan.dom[v]; ++d) o << " OUTS(" << out_off[v] + d << ", 0.0);";
        if (v == 0) o << " labels[CS] = 0;";  // an observed query: the ArgMax of its row of zeros
        o << " }\n";
    }
    o << R"(        const bool any_bad = __builtin_amdgcn_ballot_w64(bad != 0u) != 0ull;
        if (lane == 0) flags[blk] = any_bad ? 1 : 0;  // every block writes its flag: no clearing pass
    }
    if (prof && lane == 0)
        for (int k = 0; k < 10; ++k) prof[(unsigned long long)blockIdx.x * 16 + k] = pacc[k];
}
)";
    src = o.str();
    for (size_t n = 0; n < iv_first.size(); ++n) {
        const size_t at = src.find(IvMarker(n) + "\n");
        src.replace(at, IvMarker(n).size() + 1, iv_first[n]);
    }
    return FBN_OK;
}

}  // namespace

int GenerateJTKernel(const JTPlanHost &plan, std::string &src, int64_t *wave_entries, std::vector<double> &initv,
                     int64_t *lds_bytes, bool fast, bool var_major, JTPlacement *placement) {
    JTGen g(plan, fast, var_major);
    int rc = g.Run(src, wave_entries, initv);
    if (placement) *placement = g.place;
    if (lds_bytes) *lds_bytes = ((g.lds_rows + g.pool_rows) * 64 + (g.iv_lds ? (int64_t)initv.size() : 0)) * 8;
    return rc;
}

}  // namespace fbn
