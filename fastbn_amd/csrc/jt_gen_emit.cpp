// jt_gen_emit.cpp -- plan-specialized junction-tree kernel (HIP source, compiled with hiprtc for gfx950).
//
// For trees whose cliques are small (ALARM-class), the case-independent schedule is emitted as
// straight-line code: every table entry of the clique in flight is a named fp64 register value
// (lane = evidence case), every index map / digit / stride and every initial potential is a
// compile-time constant; the initial potentials are read with wave-uniform scalar loads from a
// constant buffer.  No op dispatch, no index arrays; LDS holds the entries of a large clique past
// the register-resident ones and a pool of message rows.
//
// Three parts (jt_gen.h): the schedule says what every op loads, prefetches and needs
// (jt_gen_schedule.cpp), the placement gives every stored message its registers, LDS rows or global
// rows (jt_gen_place.cpp), and the emitter here walks the schedule and writes the text.  The emitter
// keeps no mode between its functions: what an op's pieces must know is passed to them.
// Operation order per entry is exactly the interpreter's (= the reference's), so results are
// bit-identical; a lane whose normalization denominator leaves [2^-600, 2^600] flags its block,
// which the exact interpreter then recomputes (see capi_jt.hip).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <sstream>
#include <string>

#include "jt_gen.h"

namespace fbn {

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

JtGenOptions JtGenReadOptions(bool fast, bool var_major) {
    JtGenOptions opt;
    opt.fast = fast, opt.vmajor = var_major;
    opt.budget = fast ? 260 : 200;
    opt.reg_cap = fast && var_major ? kJtDefaultRegPool : 0;
    if (const char *e = KnobValue("FBN_JT_REG_POOL")) opt.reg_cap = fast ? std::max(0, atoi(e)) : 0;
    if (const char *e = KnobValue("FBN_JT_LDS_POOL")) opt.lds_pool = std::max(0, atoi(e));
    opt.leaf_rc = KnobOr("FBN_JT_LEAF_RC", 0) != 0;
    opt.sched = opt.reg_cap > 0 && KnobOr("FBN_JT_SCHED", 1) != 0;
    opt.marg_v2 = fast && KnobOr("FBN_JT_MARG_V2", 1) != 0;
    opt.profile = KnobOr("FBN_JT_PROFILE", 0) != 0;  // diagnostic build
    opt.place_debug = KnobSet("FBN_JT_PLACE_DEBUG");
    return opt;
}

JtGenTables JtGenBuildTables(const JTPlanHost &plan, bool fast) {
    const int nc = (int)plan.cliques.size(), ns = (int)plan.seps.size(), V = plan.num_nodes;
    JtGenTables tab;
    int64_t niv = 0;
    for (int c = 0; c < nc; ++c) {
        tab.lds_rows = std::max<int64_t>(tab.lds_rows, plan.cliques[c].size() - kJtRegEntries);
        tab.init_off.push_back(niv);
        niv += plan.cliques[c].size();
    }
    tab.out_off.assign(V, 0);
    for (int v = 0; v < V; ++v) tab.out_off[v] = tab.SD, tab.SD += plan.dom[v];
    tab.cand.assign(V, {});
    for (int c = 0; c < nc; ++c)
        for (int v : plan.cliques[c].vars) tab.cand[v].push_back(c);
    tab.home.assign(V, -1);
    for (int v = 0; v < V; ++v)
        for (int q : tab.cand[v])
            if (tab.home[v] < 0 || plan.cliques[q].size() < plan.cliques[tab.home[v]].size()) tab.home[v] = q;
    tab.msep.assign(V, -1);
    if (fast)
        for (int sp = 0; sp < ns; ++sp)
            for (int v : plan.seps[sp].vars) {
                const int64_t have = tab.msep[v] >= 0 ? plan.seps[tab.msep[v]].size() : plan.cliques[tab.home[v]].size();
                if (plan.seps[sp].size() < have) tab.msep[v] = sp;
            }
    tab.mclq = tab.home;
    tab.okw_word.assign(V, 0);
    tab.okw_pos.assign(V, 0);
    for (int v = 0, pos = 32; v < V; ++v) {
        if (pos + plan.dom[v] > 32) ++tab.nokw, pos = 0;
        tab.okw_word[v] = tab.nokw - 1, tab.okw_pos[v] = pos, pos += plan.dom[v];
    }
    tab.nobs = (V + 31) / 32;
    return tab;
}

namespace {

int LocOfT(const Table &t, int v) {
    for (size_t i = 0; i < t.vars.size(); ++i)
        if (t.vars[i] == v) return (int)i;
    return -1;
}

// The fixed text in front of the ops.  FBN_IV_LDS (always 0), FBN_MIN_WAVES (always 1), FBN_NO_OUT and
// FBN_WS_FOLD (never defined) belong to retired builds; their inert text stays byte for byte,
// because the code-object cache key is a hash of this source and tests/test_jt_regpool_codegen.py
// and tests/test_jt_codegen_pinned.py pin the keys.
const char kPrelude[] = R"FBN(typedef signed char i8;
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

const char kEpilogue[] = R"(        const bool any_bad = __builtin_amdgcn_ballot_w64(bad != 0u) != 0ull;
        if (lane == 0) flags[blk] = any_bad ? 1 : 0;  // every block writes its flag: no clearing pass
    }
    if (prof && lane == 0)
        for (int k = 0; k < 10; ++k) prof[(unsigned long long)blockIdx.x * 16 + k] = pacc[k];
}
)";

// a balanced tree over [lo, hi) splits here: sums, products and their level-wise forms alike
size_t Split(size_t lo, size_t hi) { return lo + (hi - lo) / 2; }

// fast order: a sum (product) as a balanced tree (depth log2 n instead of an n-long dependency
// chain: a dependent fp64 add costs ~45 cycles at one wave per SIMD, an independent one ~5,
// tools/micro/fp64_ilp.hip); the reference's left-to-right order is kept in the exact order
std::string Tree(const std::vector<std::string> &t, const char *op, size_t lo, size_t hi) {
    if (hi - lo == 1) return t[lo];
    const size_t m = Split(lo, hi);
    return "(" + Tree(t, op, lo, m) + op + Tree(t, op, m, hi) + ")";
}
std::string TreeSum(const std::vector<std::string> &t) { return Tree(t, " + ", 0, t.size()); }

class Emitter {
  public:
    Emitter(const JTPlanHost &p, const JtGenOptions &op, const JtGenTables &tb, const JtGenSchedule &sc, const JtGenPlacement &pc)
        : plan(p), opt(op), tab(tb), sch(sc), pl(pc), fast(op.fast), nc((int)p.cliques.size()) {
        // the fused products of the pipeline, in schedule order (FirstBatch)
        fused_at.assign(2 * nc, -1);
        for (int t = 0; t < 2 * nc && opt.sched; ++t) {
            const JtGenOp &o2 = sch.ops[t];
            if (t < nc ? o2.runs : (o2.clique != sch.cont_root && o2.early)) fused_at[t] = (int)fused.size(), fused.push_back(t);
        }
    }
    std::string Run(int64_t wave_entries, int64_t niv) {
        Prelude(wave_entries, niv);
        Collect();
        Distribute();
        Epilogue();
        return o.str();
    }

  private:
    const JTPlanHost &plan;
    const JtGenOptions &opt;
    const JtGenTables &tab;
    const JtGenSchedule &sch;
    const JtGenPlacement &pl;
    const bool fast;
    const int nc;
    std::ostringstream o;  // the text
    int64_t ntemp = 0;     // the names of Levels' temporaries
    std::vector<int> fused, fused_at;  // times of the fused products; a time's index among them (-1: none)

    static constexpr int64_t kInitBatch = 16;  // entries per software-pipelined batch of initial potentials
    // Pipeline of the initial potentials' scalar loads, on where the register pool is on
    // (FBN_JT_SCHED, default 1; 0 = the loads as without the pool).  Values are untouched: only
    // where the loads stand changes.  Without it batch b + 1 is requested right before batch b's
    // first use, and as scalar loads return out of order that use's wait (lgkmcnt(0)) covers the
    // request just made: every second batch paid a whole scalar-cache round trip.  With it
    //  * batch b + 1 is requested after the first products of batch b, so behind their wait;
    //  * the first batch of fused product n + 1 (kSchedFirst entries: the SGPRs it holds across the
    //    sums of op n) is requested right after fused product n, the first product's in front of
    //    its op (FirstBatch: the schedule knows which product comes next);
    //  * the loads are volatile vector loads (IvLoads), which keep their place.
    static constexpr int64_t kSchedFirst = 8;
    static int64_t BatchEnd(int64_t b0, int64_t T, bool pipelined) {
        return std::min(T, b0 + (b0 == 0 && pipelined ? kSchedFirst : kInitBatch));
    }
    // With the pipeline, the product trees of kSchedGroup entries of a fused product and the bin
    // sums of kSchedGroup bins of a Collect message are written level by level (every node over two
    // leaves first, then the nodes over those), one named temporary per inner node: the same trees
    // as Tree, so the same operands and association.  No barrier between the levels: the
    // order is a hint to the compiler, which keeps enough of it.
    static constexpr int64_t kSchedGroup = 2;
    struct LTree {  // one statement: head <balanced tree of the leaves> ; tail
        std::string head;
        std::vector<std::string> leaves;
        std::string tail;
    };
    std::vector<std::string> Levels(const std::vector<LTree> &trees, char op);  // the statements, by level
    std::string IvLoads(const std::string &P, int c, int64_t b0, bool pipelined) const;
    // the first batch of the fused product at time t ("" where t has none)
    std::string FirstBatch(int t) const { return IvLoads(t < nc ? "t" : "u", sch.ops[t].clique, 0, true); }
    std::string NextFirstBatch(int t) const {
        const size_t i = (size_t)fused_at[t] + 1;
        return fused_at[t] >= 0 && i < fused.size() ? FirstBatch(fused[i]) : std::string();
    }
    // op boundary (+ diagnostic cycle stamp of op category k when FBN_JT_PROFILE is set)
    std::string B(int k) const {
        return opt.profile ? "        FBN_OP_BOUNDARY(); FBN_STAMP(" + std::to_string(k) + ");\n" : "        FBN_OP_BOUNDARY();\n";
    }
    std::string R(int c) const {  // number of unobserved variables of clique c
        std::vector<unsigned> m(tab.nobs, 0u);
        for (int v : plan.cliques[c].vars) m[v / 32] |= 1u << (v % 32);
        std::ostringstream t;
        t << "(" << plan.cliques[c].vars.size();
        for (int k = 0; k < tab.nobs; ++k)
            if (m[k]) t << " - __builtin_popcount(obs" << k << " & " << m[k] << "u)";
        t << ")";
        return t.str();
    }
    std::string observed(int v) const {
        std::ostringstream t;
        t << "((obs" << v / 32 << " >> " << v % 32 << ") & 1u)";
        return t.str();
    }
    // separator index of clique entry e (the clique's digits of the separator's variables)
    static int64_t SepIndex(const Table &t, const Table &sp, int64_t e) {
        int64_t r = e, idx = 0;
        for (size_t j = 0; j < t.vars.size(); ++j) {
            const int64_t dgt = r / t.cum[j];
            r %= t.cum[j];
            const int l = LocOfT(sp, t.vars[j]);
            if (l >= 0) idx += dgt * sp.cum[l];
        }
        return idx;
    }
    // entry e of clique c's table: a register value, or (entries >= kJtRegEntries of a large table)
    // an LDS row [row][64 lanes] -- only one clique is in flight, so every table starts at row 0
    static std::string N(const std::string &P, int c, int64_t e) {
        if (e >= kJtRegEntries) return "L(" + std::to_string(e - kJtRegEntries) + ")";
        return P + std::to_string(c) + "_" + std::to_string(e);
    }
    // value of entry e as the reference holds it: divided by the pending denominator unless the
    // table has been normalized eagerly (Normalize) since its last update
    std::string Val(const std::string &P, int c, int64_t e, bool normed) const {
        return (normed || fast) ? N(P, c, e) : "dv(" + N(P, c, e) + ", den, y)";
    }
    void Init(const std::string &P, int c);
    // fast order: Init and every multiplication of the clique fused into one op (per entry the
    // initial potential x the home-evidence indicators x each message), ILP over all entries.
    // own_first: it requests its first batch itself (no pipeline, or a recompute scope);
    // next_first: the first batch of the fused product after it
    void InitProd(const std::string &P, int c, const std::vector<std::pair<int, std::string>> &kids, int up,
                  const std::string &upM, bool own_first, const std::string &next_first);
    void Mul(const std::string &P, int c, int s, const std::string &M, bool up = false);
    void SepCol(const std::string &P, int c, int s, bool store);
    // normed: the table was normalized eagerly (exact order).  merged (fast order): a clique's
    // SepDis ops and marginals share one op region (independent of each other: their latencies
    // overlap); inside it an op's closing boundary is left out
    void SepDis(const std::string &P, int c, int s, const std::string &old, bool store, bool normed, bool merged);
    void Marg(const std::string &P, int c, bool normed, bool merged);
    // fast order: a marginal (and the label of variable 0) from the terms of each value
    void MargTerms(int v, const std::vector<std::vector<std::string>> &terms);
    void Load(const std::string &name, int s) {  // "ld": the Distribute message, else the Collect one
        for (int64_t j = 0; j < plan.seps[s].size(); ++j)
            o << "        const double " << name << s << "_" << j << " = " << pl.Loc(s, name == "ld", j) << ";\n";
    }
    void LoadCol(const std::string &name, int s) {
        if (!sch.leaf_rc[s]) return Load(name, s);
        const int c = plan.sep_down[s];
        const int64_t Ts = plan.seps[s].size(), Q = plan.cliques[c].size() / Ts;
        for (int64_t j = 0; j < Ts; ++j) o << "        double " << name << s << "_" << j << ";\n";
        o << "        { // recompute the Collect message of leaf clique " << c << "\n";
        const std::string P = "r" + name;
        InitProd(P, c, {}, -1, "", true, "");  // (a scope of its own: no first batch of the next fused product in it)
        for (int64_t j = 0; j < Ts; ++j) {
            std::vector<std::string> terms;
            for (int64_t q = 0; q < Q; ++q) terms.push_back(N(P, c, q * Ts + j));
            o << "        " << name << s << "_" << j << " = " << TreeSum(terms) << ";\n";
        }
        o << "        }\n";
    }
    void Normalize(const std::string &P, int c) {
        const Table &t = plan.cliques[c];
        for (int64_t e = 0; e < t.size(); ++e) o << (e % 8 ? " " : (e ? "\n        " : "        ")) << N(P, c, e) << " = dv(" << N(P, c, e) << ", den, y);";
        o << "\n" << B(6);
    }
    void Prelude(int64_t wave_entries, int64_t niv);
    void Collect();
    void Distribute();
    void Epilogue();
};

// masked initial potential + Normalize (lazy: values raw, den/y pending)
void Emitter::Init(const std::string &P, int c) {
    const Table &t = plan.cliques[c];
    const int nv = (int)t.vars.size();
    // per (variable, value) "allowed by the evidence" lane masks, then one AND chain per entry
    std::vector<bool> ev_here(nv, true);  // variables whose evidence this table carries
    for (int j = 0; j < nv; ++j) ev_here[j] = !fast || tab.home[t.vars[j]] == c;
    for (int j = 0; j < nv; ++j) {
        const int v = t.vars[j];
        if (!ev_here[j]) continue;
        for (int d = 0; d < plan.dom[v]; ++d)
            o << (d ? " " : "        ") << "const bool k" << P << c << "_" << j << "_" << d << " = (okw" << tab.okw_word[v] << " >> "
              << tab.okw_pos[v] + d << ") & 1u;";
        o << "\n";
    }
    if (!fast) o << "        double s_" << P << c << " = 0.0;\n";
    // software-pipelined in batches: the loads of batch b+1 are issued before batch b computes
    const int64_t T = t.size();
    o << IvLoads(P, c, 0, false);
    for (int64_t b0 = 0; b0 < T; b0 += kInitBatch) {
        o << IvLoads(P, c, b0 + kInitBatch, false);
        for (int64_t e = b0; e < std::min(T, b0 + kInitBatch); ++e) {
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
            o << "        " << (e < kJtRegEntries ? "double " : "") << N(P, c, e) << " = ";
            if (any) o << "sel(" << cond.str() << ", w" << P << c << "_" << e << ");";
            else o << "w" << P << c << "_" << e << ";";
            if (!fast) o << " s_" << P << c << " += " << N(P, c, e) << ";";
            o << "\n";
        }
        o << "        __builtin_amdgcn_sched_barrier(0);\n";
    }
    if (!fast) o << "        den = s_" << P << c << "; y = 1.0 / den; bad |= den_bad(den);\n";
    o << B(2);
}

std::vector<std::string> Emitter::Levels(const std::vector<LTree> &trees, char op) {
    std::vector<std::string> lv;
    const std::string ops = std::string(" ") + op + " ";
    for (const LTree &t : trees) {
        // (name, height) of the node over the leaves [lo, hi), split like Tree
        std::function<std::pair<std::string, size_t>(size_t, size_t)> node = [&](size_t lo, size_t hi) -> std::pair<std::string, size_t> {
            if (hi - lo == 1) return {t.leaves[lo], 0};
            const size_t m = Split(lo, hi);
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

// the loads of the batch of clique c's initial potentials that starts at entry b0 ("" past the end)
std::string Emitter::IvLoads(const std::string &P, int c, int64_t b0, bool pipelined) const {
    const int64_t T = plan.cliques[c].size();
    std::ostringstream o;
    if (b0 >= T) return std::string();
    const int64_t b1 = BatchEnd(b0, T, pipelined);
    if (pipelined) {
        // Ordered loads: a plain load from the constant address space is tied to nothing, and
        // instruction selection places it next to its first use whatever the statement order (the
        // scheduling barriers bind the machine scheduler only).  A volatile load keeps its place
        // between the barriers; whole vectors, so a batch is still two 64-byte scalar loads.
        for (int64_t e = b0, n = 16; e < b1; e += n) {
            while (n > b1 - e) n /= 2;
            const std::string wv = "wv" + P + std::to_string(c) + "_" + std::to_string(e);
            o << "        const " << (n > 1 ? "fbn_w" + std::to_string(n) : std::string("double")) << " " << wv << " = *(const volatile "
              << (n > 1 ? "fbn_cw" + std::to_string(n) : std::string("cdouble")) << " *)&IV(" << tab.init_off[c] + e << ");";
            for (int64_t k = 0; k < n; ++k)
                o << " const double w" << P << c << "_" << e + k << " = " << wv << (n > 1 ? "[" + std::to_string(k) + "]" : std::string()) << ";";
            o << "\n";
        }
        o << "        __builtin_amdgcn_sched_barrier(0);\n";
        return o.str();
    }
    o << "       ";
    for (int64_t e = b0; e < b1; ++e)
        o << " const double w" << P << c << "_" << e << " = IV(" << tab.init_off[c] + e << ");";
    o << "\n        __builtin_amdgcn_sched_barrier(0);\n";
    return o.str();
}

void Emitter::InitProd(const std::string &P, int c, const std::vector<std::pair<int, std::string>> &kids, int up,
                       const std::string &upM, bool own_first, const std::string &next_first) {
    const Table &t = plan.cliques[c];
    const int nv = (int)t.vars.size();
    const bool sched = opt.sched;
    // 0.0 / 1.0 indicators of the home variables' allowed values (x * 1.0 == x, x * 0.0 == 0 for the
    // finite potentials: the masking of the reference's reduction, one multiply instead of a select)
    std::vector<bool> ev_here(nv, false);
    for (int j = 0; j < nv; ++j) ev_here[j] = tab.home[t.vars[j]] == c;
    for (int j = 0; j < nv; ++j) {
        if (!ev_here[j]) continue;
        const int v = t.vars[j];
        for (int d = 0; d < plan.dom[v]; ++d)
            o << (d ? " " : "        ") << "const double i" << P << c << "_" << j << "_" << d << " = (double)((okw"
              << tab.okw_word[v] << " >> " << tab.okw_pos[v] + d << ") & 1u);";
        o << "\n";
    }
    std::vector<std::vector<int64_t>> kidx(kids.size());
    for (size_t i = 0; i < kids.size(); ++i) {
        const Table &sp = plan.seps[kids[i].first];
        for (int64_t e = 0; e < t.size(); ++e) kidx[i].push_back(SepIndex(t, sp, e));
    }
    const int64_t Tup = up >= 0 ? plan.seps[up].size() : 0;
    const int64_t T = t.size();
    if (own_first) o << IvLoads(P, c, 0, sched);
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
        b1 = BatchEnd(b0, T, true);
        // the next batch is requested behind the first level that reads a potential of this one,
        // so behind its wait
        bool pending = b1 < T;
        for (int64_t e0 = b0; e0 < b1; e0 += kSchedGroup) {
            std::vector<LTree> trees;
            for (int64_t e = e0; e < std::min(b1, e0 + kSchedGroup); ++e)
                trees.push_back({"        " + std::string(e < kJtRegEntries ? "double " : "") + N(P, c, e) + " = ", factors(e), "\n"});
            for (const std::string &l : Levels(trees, '*')) {
                o << l;
                if (pending && l.find(wpre) != std::string::npos) {
                    o << "        __builtin_amdgcn_sched_barrier(0);\n" << IvLoads(P, c, b1, true);
                    pending = false;
                }
            }
        }
        o << "        __builtin_amdgcn_sched_barrier(0);\n";
    }
    for (int64_t b0 = 0, b1; b0 < T && !sched; b0 = b1) {
        b1 = BatchEnd(b0, T, false);
        o << IvLoads(P, c, b1, false);
        for (int64_t e = b0; e < b1; ++e) {
            const std::vector<std::string> f = factors(e);  // a balanced product tree (depth log2 of the factor count)
            o << "        " << (e < kJtRegEntries ? "double " : "") << N(P, c, e) << " = " << Tree(f, " * ", 0, f.size()) << ";\n";
        }
        o << "        __builtin_amdgcn_sched_barrier(0);\n";
    }
    o << B(2) << next_first;
}

// CliqueLevelCollection: table *= extended child message (by separator entry), then Normalize;
// up: CliqueLevelDistribution, the parent's message broadcast over k % Ts
void Emitter::Mul(const std::string &P, int c, int s, const std::string &M, bool up) {
    const Table &t = plan.cliques[c], &sp = plan.seps[s];
    std::vector<std::vector<int64_t>> inv(sp.size());
    for (int64_t e = 0; e < t.size(); ++e) inv[up ? e % sp.size() : SepIndex(t, sp, e)].push_back(e);
    for (int64_t j = 0; j < sp.size(); ++j) {
        o << "       ";
        for (int64_t e : inv[j]) o << " " << N(P, c, e) << " = " << Val(P, c, e, false) << " * " << M << s << "_" << j << ";";
        o << "\n";
    }
    if (!fast) {
        o << "        { double sm = 0.0;";
        for (int64_t e = 0; e < t.size(); ++e) o << " sm += " << N(P, c, e) << ";";
        o << " den = sm; y = 1.0 / den; bad |= den_bad(den); }\n";
    }
    o << B(up ? 5 : 3);
}

// SeparatorLevelCollection: message[k % Ts] += table[k] / den  -> registers mc<s>_j (+ store)
void Emitter::SepCol(const std::string &P, int c, int s, bool store) {
    const Table &t = plan.cliques[c];
    const int64_t Ts = plan.seps[s].size(), Q = t.size() / Ts;
    auto stored = [&](int64_t j) {
        const std::string mc = "mc" + std::to_string(s) + "_" + std::to_string(j);
        return store ? " " + pl.Loc(s, false, j) + " = " + mc + ";" : std::string();
    };
    // fast order: message = the raw bin sums (tree sums), never normalized: every later use is
    // invariant to a per-case scale of it (the Distribute ratio a / old, the normalized marginals),
    // and its values are likelihoods of the evidence below (<= 1); Marg range-checks the products
    for (int64_t j0 = 0; j0 < Ts && fast && opt.sched; j0 += kSchedGroup) {
        std::vector<LTree> trees;
        for (int64_t j = j0; j < std::min(Ts, j0 + kSchedGroup); ++j) {
            std::vector<std::string> terms;
            for (int64_t q = 0; q < Q; ++q) terms.push_back(N(P, c, q * Ts + j));
            trees.push_back({"        const double mc" + std::to_string(s) + "_" + std::to_string(j) + " = ", terms, stored(j) + "\n"});
        }
        for (const std::string &l : Levels(trees, '+')) o << l;
    }
    for (int64_t j = 0; j < Ts && !(fast && opt.sched); ++j) {
        o << "        const double mc" << s << "_" << j << " = ";
        if (fast) {
            std::vector<std::string> terms;
            for (int64_t q = 0; q < Q; ++q) terms.push_back(N(P, c, q * Ts + j));
            o << TreeSum(terms);
        } else {
            o << Val(P, c, j, false);
            for (int64_t q = 1; q < Q; ++q) o << " + " << Val(P, c, q * Ts + j, false);
        }
        o << ";" << stored(j) << "\n";
    }
    o << B(4);
}

// SeparatorLevelDistribution: tmp[map(k)] += table[k] / den; message = tmp / old (zero-guarded)
void Emitter::SepDis(const std::string &P, int c, int s, const std::string &old, bool store, bool normed, bool merged) {
    const Table &t = plan.cliques[c], &sp = plan.seps[s];
    std::vector<std::vector<int64_t>> lists(sp.size());
    for (int64_t e = 0; e < t.size(); ++e) lists[SepIndex(t, sp, e)].push_back(e);
    for (int64_t j = 0; j < sp.size(); ++j) {
        if (fast) {
            // bin sums a(j) as trees; md(j) = a(j) / old(j), 0 where old(j) == 0, with branch-free
            // reciprocals (v_rcp_f64 + one Newton step) so the Ts quotients overlap; no normalization
            // (the child's marginals are normalized at the end; values stay likelihoods <= 1)
            std::vector<std::string> terms;
            for (int64_t e : lists[j]) terms.push_back(N(P, c, e));
            const std::string sa = "sa" + std::to_string(s) + "_" + std::to_string(j);
            o << "        const double " << sa << " = " << TreeSum(terms) << ";";
            o << " double md" << s << "_" << j << "; { const double od = " << old << s << "_" << j
              << "; const double q = " << sa << " * frcp(od); md" << s << "_" << j << " = (od == 0.0) ? 0.0 : q; }";
        } else {
            o << "        double md" << s << "_" << j << ";";
            o << " { double a = " << Val(P, c, lists[j][0], normed) << ";";
            for (size_t q = 1; q < lists[j].size(); ++q) o << " a += " << Val(P, c, lists[j][q], normed) << ";";
            o << " const double od = " << old << s << "_" << j << "; md" << s << "_" << j << " = (od == 0.0) ? 0.0 : a / od; }";
        }
        if (store) o << " " << pl.Loc(s, true, j) << " = md" << s << "_" << j << ";";
        o << "\n";
    }
    // fast order: the marginals summed from this separator's calibrated belief (its bin sums)
    for (size_t l = 0; l < sp.vars.size() && fast; ++l) {
        const int v = sp.vars[l];
        if (tab.msep[v] != s) continue;
        std::vector<std::vector<std::string>> terms(plan.dom[v]);
        for (int64_t j = 0; j < sp.size(); ++j)
            terms[(j / sp.cum[l]) % sp.dims[l]].push_back("sa" + std::to_string(s) + "_" + std::to_string(j));
        MargTerms(v, terms);
    }
    if (!merged) o << B(7);
}

void Emitter::MargTerms(int v, const std::vector<std::vector<std::string>> &terms) {
    const int dim = plan.dom[v];
    // FBN_JT_MARG_V2 (v2), unbranched: computed for every lane, observed lanes store 0.0 (the
    // reference's marginal of an observed variable) in the same stores -- no divergent branch, no
    // second store pass (ALARM 0.137 -> 0.130 ms); adjacent values go out as one 16-byte store per
    // lane (neutral).  (Measured and dropped: staging groups of 8 / 16 output values in LDS pool rows
    // and writing them out coalesced, 0.205 / 0.223 ms, round 5.)
    const bool v2 = opt.marg_v2;
    if (v2) o << "        { // marginal of var " << v << "\n          const bool ob = " << observed(v) << " != 0u;\n";
    else o << "        if (!" << observed(v) << ") { // marginal of var " << v << "\n";
    std::vector<std::string> ps;
    for (int d = 0; d < dim; ++d) {
        o << "          const double p" << d << " = " << TreeSum(terms[d]) << ";\n";
        ps.push_back("p" + std::to_string(d));
    }
    o << "          const double tot = " << TreeSum(ps) << "; const double yt = frcp(tot); bad |= "
      << (v2 ? "ob ? 0u : den_bad(tot)" : "den_bad(tot)") << ";\n";
    if (v == 0) {
        // a near-tie (top two within 1e-12 relative) may break differently from the reference's exact
        // values: the block is flagged for the exact pass
        o << "          if (" << (v2 ? "ACT && !ob" : "ACT") << ") { int lab = 0; double mp = 0.0, m2 = 0.0;";
        for (int d = 0; d < dim; ++d)
            o << " { const double q = dv(p" << d << ", tot, yt); if (q > mp) { m2 = mp; mp = q; lab = " << d
              << "; } else if (q > m2) m2 = q; }";
        o << " labels[CS] = lab; bad |= (mp - m2 <= 1e-12 * mp) ? 1u : 0u; }\n";
    }
    if (!v2) o << "          if (ACT) {";
    for (int d = 0; d < dim; ++d) {
        const int64_t k = tab.out_off[v] + d;
        if (!v2) {
            o << " OUTS(" << k << ", dv(p" << d << ", tot, yt));";
        } else if (d + 1 < dim) {
            o << "          if (ACT) OUTS2(" << k << ", ob ? 0.0 : dv(p" << d << ", tot, yt), ob ? 0.0 : dv(p" << d + 1 << ", tot, yt));\n";
            ++d;
        } else {
            o << "          if (ACT) OUTS(" << k << ", ob ? 0.0 : dv(p" << d << ", tot, yt));\n";
        }
    }
    o << (v2 ? "        }\n" : " }\n        }\n");
}

// GetProbabilitiesOneNode for every variable whose selected clique (first with the fewest reduced
// variables) is c, and the label (ArgMax, strict '>' from 0; un-normalized if c reduces to one var)
void Emitter::Marg(const std::string &P, int c, bool normed, bool merged) {
    const Table &t = plan.cliques[c];
    for (size_t j = 0; j < t.vars.size(); ++j) {
        const int v = t.vars[j];
        const int dim = plan.dom[v];
        const int64_t cum = t.cum[j], bw = dim * cum, nhi = t.size() / bw;
        if (fast) {  // the smallest clique holding the variable (a calibrated tree: any gives the marginal)
            if (tab.mclq[v] != c || tab.msep[v] >= 0) continue;
            std::vector<std::vector<std::string>> terms(dim);
            for (int d = 0; d < dim; ++d)
                for (int64_t hi = 0; hi < nhi; ++hi)
                    for (int64_t l = 0; l < cum; ++l) terms[d].push_back(N(P, c, hi * bw + d * cum + l));
            MargTerms(v, terms);
            if (!merged) o << B(8);
            continue;
        }
        // selection: first candidate clique with the fewest reduced variables (recomputed here)
        const std::vector<int> &cand = tab.cand[v];
        o << "        { int b = " << R(cand[0]) << ", sl = " << cand[0] << ";";
        for (size_t k = 1; k < cand.size(); ++k)
            o << " { const int r = " << R(cand[k]) << "; if (r < b) { b = r; sl = " << cand[k] << "; } }";
        o << "\n        if (sl == " << c << " && !" << observed(v) << ") { // marginal of var " << v << "\n";
        o << "          double tot = 0.0;";
        for (int d = 0; d < dim; ++d) o << " double p" << d << ";";
        o << "\n";
        for (int d = 0; d < dim; ++d) {
            bool first = true;
            o << "          { double a = ";
            for (int64_t hi = 0; hi < nhi; ++hi)
                for (int64_t l = 0; l < cum; ++l) {
                    const int64_t e = hi * bw + d * cum + l;
                    o << (first ? "" : " a += ") << Val(P, c, e, normed) << ";";
                    first = false;
                }
            o << " p" << d << " = a; tot += a; }\n";
        }
        o << "          const double yt = 1.0 / tot; bad |= den_bad(tot);\n";
        if (v == 0) {
            o << "          if (ACT) { int lab = 0; double mp = 0.0, m2 = 0.0;";
            for (int d = 0; d < dim; ++d)
                o << " { const double q = (b == 1) ? p" << d << " : dv(p" << d << ", tot, yt); if (q > mp) { m2 = mp; mp = q; lab = " << d
                  << "; } else if (q > m2) m2 = q; }";
            o << " labels[CS] = lab; }\n";
        }
        o << "          if (ACT) {";
        for (int d = 0; d < dim; ++d) o << " OUTS(" << tab.out_off[v] + d << ", dv(p" << d << ", tot, yt));";
        o << " }\n        } }\n" << (merged ? std::string() : B(8));
    }
}

void Emitter::Prelude(int64_t wave_entries, int64_t niv) {
    const int V = plan.num_nodes;
    o << "// generated by libfastbn (jt_codegen.cpp): " << nc << " cliques, " << plan.seps.size() << " separators, "
      << (fast ? "fast" : "exact") << " arithmetic order\n";
    o << "#define FBN_V " << V << "\n#define FBN_SD " << tab.SD << "\n#define FBN_WE " << wave_entries << "LL\n";
    o << "#define FBN_LP_BASE " << tab.lds_rows << "\n";
    o << "#define FBN_IV_BASE " << (tab.lds_rows + pl.pool_rows) * 64 << "\n#define FBN_NIV " << niv << "\n";
    o << "#define FBN_IV_LDS 0\n#define FBN_MIN_WAVES 1\n";
    if (opt.vmajor) o << "#define FBN_VMAJOR 1\n";
    o << kPrelude;
    // op boundary: no store->load forwarding, no hoisting of addresses, no scheduling across it,
    // and the evidence words are opaque per segment, so a Distribute recomputation is not merged
    // with (and kept live from) its Collect twin
    std::vector<std::string> regs;
    for (int k = 0; k < tab.nokw; ++k) regs.push_back("okw" + std::to_string(k));
    for (int k = 0; k < tab.nobs; ++k) regs.push_back("obs" + std::to_string(k));
    o << "#define FBN_OP_BOUNDARY() do { __asm__ volatile(\"\" : \"+s\"(Wb), \"+v\"(lo), \"+v\"(ltail), \"+v\"(ivl), \"+v\"(bad), \"+s\"(blkl) :: \"memory\");";
    for (size_t i = 0; i < regs.size(); i += 16) {
        o << " __asm__ volatile(\"\" :";
        for (size_t k = i; k < std::min(regs.size(), i + 16); ++k) o << (k > i ? ", " : " ") << "\"+v\"(" << regs[k] << ")";
        o << ");";
    }
    o << " __builtin_amdgcn_sched_barrier(0); } while (0)\n";
    if (opt.sched)  // batches of initial potentials as vectors (IvLoads)
        for (int n = 2; n <= 16; n *= 2)
            o << "        typedef double fbn_w" << n << " __attribute__((ext_vector_type(" << n << "), aligned(8)));"
              << " typedef __attribute__((address_space(4))) fbn_w" << n << " fbn_cw" << n << ";\n";
    for (const std::string &r : regs) o << "        unsigned " << r << " = 0u;\n";
    // message entries parked in registers: one per block iteration, assigned by the op that forms
    // the message before any op reads it; not in the boundaries' operand lists (free to sit in AGPRs)
    for (size_t i = 0; i < pl.reg_names.size(); i += 8) {
        o << "        double";
        for (size_t k = i; k < std::min(pl.reg_names.size(), i + 8); ++k) o << (k > i ? ", " : " ") << pl.reg_names[k];
        o << ";\n";
    }
    for (int v = 0; v < V; ++v) {
        const unsigned full = (plan.dom[v] >= 32) ? 0xFFFFFFFFu : ((1u << plan.dom[v]) - 1u);
        o << "        { const int x = ev[" << v << "]; okw" << tab.okw_word[v] << " |= (x < 0 ? " << full << "u : (1u << x)) << "
          << tab.okw_pos[v] << "; obs" << v / 32 << " |= (x >= 0 ? 1u : 0u) << " << v % 32 << "; }\n";
    }
    o << B(0);
}

// Collect, DFS post-order
void Emitter::Collect() {
    std::vector<bool> loaded(plan.seps.size(), false);
    auto load = [&](int s) {
        if (!loaded[s]) Load("la", s), loaded[s] = true;
    };
    for (int k = 0; k < nc; ++k) {
        const JtGenOp &op = sch.ops[k];
        if (!op.runs) continue;
        const int c = op.clique;
        o << "        // ---- collect clique " << c << " (" << plan.cliques[c].size() << " entries)\n";
        for (int s : op.loads) load(s);
        // prefetch for the next clique, less the parked rows live now (kept asymmetry 1) and only
        // when its Collect is emitted (kept asymmetry 2)
        if (k + 1 < nc && sch.ops[k + 1].runs && op.prefetch_cost + pl.reg_extra[k] <= opt.budget)
            for (int s : op.prefetch) load(s);
        if (fused_at[k] == 0) o << FirstBatch(k);  // (the kernel's first fused product: in front of its own boundary)
        o << B(1);
        const auto &down = plan.clique_down[c];
        if (fast) {
            std::vector<std::pair<int, std::string>> kids;
            for (int s : down) kids.push_back({s, loaded[s] ? "la" : "mc"});
            InitProd("t", c, kids, -1, "", fused_at[k] < 0, NextFirstBatch(k));
        } else {
            Init("t", c);
            for (int s : down) Mul("t", c, s, loaded[s] ? "la" : "mc");
        }
        if (c != sch.cont_root) SepCol("t", c, plan.clique_up[c], sch.col_store[plan.clique_up[c]]);
    }
}

// Distribute, DFS pre-order (the root continues from its Collect registers)
void Emitter::Distribute() {
    const std::vector<bool> &md_reg = sch.md_reg;
    std::vector<bool> loaded_b(plan.seps.size(), false), loaded_d(plan.seps.size(), false);
    auto load_ld = [&](int s, bool boundary) {
        if (s < 0 || md_reg[s] || loaded_d[s]) return;
        Load("ld", s), loaded_d[s] = true;
        if (boundary) o << B(1);
    };
    for (int t = nc; t < 2 * nc; ++t) {
        const JtGenOp &op = sch.ops[t];
        const int c = op.clique, up = plan.clique_up[c];
        const bool early = op.early, recompute = c != sch.cont_root, fused = recompute && fast && early;
        const auto &down = plan.clique_down[c];
        o << "        // ---- distribute clique " << c << " (" << plan.cliques[c].size() << " entries)\n";
        for (int s : op.loads)
            if (!loaded_b[s]) LoadCol("lb", s), loaded_b[s] = true;
        if (op.prefetch_cost + pl.reg_extra[t] <= opt.budget) {  // prefetch for the next clique (kept asymmetry 1)
            for (int s : op.prefetch)
                if (!loaded_b[s] && !sch.leaf_rc[s]) Load("lb", s), loaded_b[s] = true;  // (kept asymmetry 3)
            if (op.prefetch_ld >= 0) load_ld(op.prefetch_ld, false);
        }
        if (fused_at[t] == 0) o << FirstBatch(t);
        o << B(1);
        const std::string P = recompute ? "u" : "t";
        if (fused) {  // all messages in registers: one fused op
            load_ld(up, true);
            std::vector<std::pair<int, std::string>> kids;
            for (int s : down) kids.push_back({s, "lb"});
            InitProd(P, c, kids, up, up < 0 ? "" : md_reg[up] ? "md" : "ld", fused_at[t] < 0, NextFirstBatch(t));
        } else if (recompute) {  // recompute the Collect table (same ops, same order -> same bits)
            Init(P, c);
            for (int s : down) {
                if (!early) LoadCol("lb", s), o << B(1);
                Mul(P, c, s, "lb");
            }
            if (up >= 0) {
                load_ld(up, true);
                Mul(P, c, up, md_reg[up] ? "md" : "ld", true);
            }
        }
        // consumers of the normalized table: one SepDis per child, one marginal per variable
        // (fast order: each SepDis takes the clique total from its own bin sums)
        const bool normed = !fast && down.size() + plan.cliques[c].vars.size() >= 2;
        if (normed) Normalize(P, c);
        const bool merged = fast && early;
        for (int s : down) {
            if (!early) LoadCol("lc", s), o << B(1);
            SepDis(P, c, s, early ? "lb" : "lc", !md_reg[s], normed, merged);
        }
        Marg(P, c, normed, merged);
        if (merged) o << B(8);
    }
}

void Emitter::Epilogue() {
    // an observed query: label 0, the ArgMax of its row of zeros (the unbranched marginals write the
    // label of the other lanes only; here, at the block's end, the store costs the ALARM kernel nothing)
    if (opt.marg_v2) o << "        if (ACT && " << observed(0) << ") labels[CS] = 0;\n";
    for (int v = 0; v < plan.num_nodes && !opt.marg_v2; ++v) {  // (unbranched marginals store the zeros themselves)
        o << "        if (ACT && " << observed(v) << ") {";
        for (int d = 0; d < plan.dom[v]; ++d) o << " OUTS(" << tab.out_off[v] + d << ", 0.0);";
        if (v == 0) o << " labels[CS] = 0;";  // an observed query: the ArgMax of its row of zeros
        o << " }\n";
    }
    o << kEpilogue;
}

}  // namespace

int GenerateJTKernel(const JTPlanHost &plan, bool fast, bool var_major, JTKernelSpec &out) {
    const JtGenOptions opt = JtGenReadOptions(fast, var_major);
    JtGenTables tab;
    JtGenSchedule sch;
    JtGenPlacement pl;
    if (int rc = JtGenPlan(plan, opt, tab, sch, pl)) return rc;
    // initial potentials: one constant buffer, read with wave-uniform (scalar) loads
    out.initv.clear();
    for (const Table &t : plan.cliques) out.initv.insert(out.initv.end(), t.pot.begin(), t.pot.end());
    out.wave_entries = JtGenWaveEntries(plan, pl);
    out.lds_bytes = (tab.lds_rows + pl.pool_rows) * 64 * 8;
    out.place = pl.counts;
    out.src = Emitter(plan, opt, tab, sch, pl).Run(out.wave_entries, (int64_t)out.initv.size());
    return FBN_OK;
}

}  // namespace fbn
