// jt_codegen_host_check.cpp -- stand-alone driver of the plan-specialized JT kernel generator
// (fastbn_amd/csrc/jt_gen_*.cpp) for host sanitizer runs (no device, no libfastbn, no Python):
// one command line:
//   c++ -std=c++17 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude
//       tools/jt_codegen_host_check.cpp fastbn_amd/csrc/jt_gen_schedule.cpp fastbn_amd/csrc/jt_gen_place.cpp
//       fastbn_amd/csrc/jt_gen_emit.cpp fastbn_amd/csrc/jt_plan.cpp fastbn_amd/csrc/io.cpp
//       fastbn_amd/csrc/synth.cpp -pthread -o jt_codegen_host_check
//   ./jt_codegen_host_check [tests/golden/alarm/alarm.xml [more.xml ...]]
// Networks: ALARM and any further XMLBIF files named, and two seeded networks built here from counts (the
// library has no network generator of its own: fastbn_amd/synth.py draws the tests' random networks) --
// a connected 60-node one with parents from a window of 6, and a 120-node forest whose nodes may have
// no parent.  Each in both output layouts and both arithmetic orders under the 15 knob settings of
// tools/jt_codegen_digest.py.  Checked on the schedule and placement values, per case:
//  (a) every stored message has one entry and every entry of it exactly one place; a message that is
//      not stored (kept in registers, or a leaf-recomputed Collect message nobody loads) has none;
//  (b) two messages whose live intervals overlap (touching counts) share no LDS pool row;
//  (c) global rows of different separators are disjoint and below wave_entries;
//  (d) pool on: an op's need + the parked rows it pays for <= register file - slack, and the parked
//      rows live at any time <= the cap.  The first half does NOT hold as stated and is reported apart
//      (exit status 1): the schedule's budget (260 rows in the fast order) lets an op's own need pass
//      the limit (240 variable-major, 224 case-major), e.g. ALARM Distribute clique 24: need 264 +
//      parked 0 > 240; Distribute clique 25, case-major: 261 + 0 > 224.  What the placement itself
//      promises holds and is checked: nothing is parked at such an op's expense (parked 0 in every
//      miss), and wherever rows are parked the sum is within the limit;
//  (e) clique tail + pool stay within 40 KB of LDS per wave (networks whose cliques stay below 224
//      entries: a longer tail alone passes 40 KB and the kernel runs fewer waves per CU);
//  (f) an op's loads and prefetches name only stored messages whose producer ran earlier;
//  (g) two generations give the same source.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../fastbn_amd/csrc/jt_gen.h"

static int g_fail = 0;
static std::string g_case;
static int g_d_miss = 0;
static std::set<std::string> g_d_lines;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            printf("FAIL %s:%d [%s]: %s\n", __FILE__, __LINE__, g_case.c_str(), #cond);   \
            ++g_fail;                                                                     \
        }                                                                                 \
    } while (0)

static const char *kKnobs[] = {"REG_POOL", "SCHED", "LEAF_RC", "LDS_POOL", "MARG_V2", "PROFILE"};
static const char *kEnvs[15] = {"", "REG_POOL=0", "REG_POOL=256", "REG_POOL=64", "SCHED=0", "REG_POOL=256,SCHED=0", "LEAF_RC=1",
                                "LEAF_RC=1,REG_POOL=256", "LEAF_RC=1,REG_POOL=256,SCHED=0", "LDS_POOL=0",
                                "LDS_POOL=0,REG_POOL=256", "LDS_POOL=16", "MARG_V2=0", "MARG_V2=0,REG_POOL=256", "PROFILE=1"};

static void SetEnv(const std::string &env) {
    for (const char *k : kKnobs) unsetenv((std::string("FBN_JT_") + k).c_str());
    for (size_t at = 0; at < env.size();) {
        const size_t end = std::min(env.find(',', at), env.size()), eq = env.find('=', at);
        setenv(("FBN_JT_" + env.substr(at, eq - at)).c_str(), env.substr(eq + 1, end - eq - 1).c_str(), 1);
        at = end + 1;
    }
}

// node v > 0 draws kmin..2 parents from the `window` nodes before it; seeded counts in 1..9
static fbn::Network SeededNetwork(int n, unsigned seed, int window, int kmin) {
    std::mt19937 rng(seed);
    std::vector<int32_t> dims(n), off(n + 1, 0), par;
    std::vector<int64_t> counts;
    for (int v = 0; v < n; ++v) {
        dims[v] = 2 + (int)(rng() % 2);
        std::set<int> ps;
        const int lo = std::max(0, v - window), k = std::min(v - lo, kmin + (int)(rng() % (3 - kmin)));
        while ((int)ps.size() < k) ps.insert(lo + (int)(rng() % (v - lo)));
        int64_t cfg = dims[v];
        for (int p : ps) par.push_back(p), cfg *= dims[p];
        off[v + 1] = (int32_t)par.size();
        for (int64_t i = 0; i < cfg; ++i) counts.push_back(1 + (int64_t)(rng() % 9));
    }
    fbn::Network net;
    CHECK(fbn::BuildNetwork(n, dims.data(), off.data(), par.data(), counts.data(), nullptr, net) == FBN_OK);
    return net;
}

static void CheckPlaces(const fbn::JTPlanHost &plan, const fbn::JtGenOptions &opt, const fbn::JtGenTables &tab,
                        const fbn::JtGenSchedule &sch, const fbn::JtGenPlacement &pl, int64_t wave_entries) {
    const int nc = (int)plan.cliques.size(), ns = (int)plan.seps.size();
    // (a)
    std::vector<int> seen(2 * ns, 0);
    for (const fbn::JtGenMessage &m : pl.msgs) {
        ++seen[2 * m.sep + m.dist];
        CHECK(m.a <= m.b && m.n == plan.seps[m.sep].size() && m.nreg >= 0 && m.nreg <= m.n);
        CHECK((int64_t)m.rows.size() == m.n - m.nreg && (int64_t)m.loc.size() == m.n);
        for (int64_t j = 0; j < m.n; ++j)
            CHECK(m.loc[j].rfind(j < m.nreg ? (m.dist ? "rd" : "rc") : (m.in_lds ? "LP(" : "W("), 0) == 0);
    }
    for (int s = 0; s < ns; ++s) {
        CHECK(seen[2 * s] == (sch.leaf_rc[s] && !sch.col_store[s] ? 0 : 1) && (seen[2 * s] == 1) == (pl.col_of[s] >= 0));
        CHECK(seen[2 * s + 1] == (sch.md_reg[s] ? 0 : 1) && (seen[2 * s + 1] == 1) == (pl.dis_of[s] >= 0));
    }
    // (b), (c)
    std::vector<int> owner(wave_entries, -1);
    for (size_t i = 0; i < pl.msgs.size(); ++i) {
        const fbn::JtGenMessage &x = pl.msgs[i];
        for (int64_t r : x.rows) {
            CHECK(r >= 0 && r < (x.in_lds ? pl.pool_rows : wave_entries));
            if (x.in_lds || r < 0 || r >= wave_entries) continue;
            CHECK(owner[r] < 0 || owner[r] == x.sep);
            owner[r] = x.sep;
        }
        for (size_t k = i + 1; k < pl.msgs.size() && x.in_lds; ++k) {
            const fbn::JtGenMessage &y = pl.msgs[k];
            if (!y.in_lds || x.b < y.a || y.b < x.a) continue;
            for (int64_t r : x.rows) CHECK(std::find(y.rows.begin(), y.rows.end(), r) == y.rows.end());
        }
    }
    // (d), (e)
    for (int t = 0; t < 2 * nc && opt.reg_cap > 0; ++t) {
        const int64_t need = sch.ops[t].need, limit = fbn::kJtRegFile - opt.slack();
        if (need + pl.reg_extra[t] > limit) {  // (d) as stated: counted apart, one line per distinct miss
            char line[160];
            snprintf(line, sizeof line, "%s clique %d: need %lld + parked %lld > %lld", t < nc ? "Collect" : "Distribute",
                     sch.ops[t].clique, (long long)need, (long long)pl.reg_extra[t], (long long)limit);
            const std::string miss = g_case.substr(0, g_case.find('|')) + " " + line;
            if (g_d_lines.insert(miss).second) printf("(d) %s\n", miss.c_str());
            ++g_d_miss;
        }
        CHECK(pl.reg_extra[t] == 0 || need + pl.reg_extra[t] <= limit);  // (what the placement adds always fits)
        CHECK(pl.live[t] <= opt.reg_cap);
    }
    CHECK((tab.lds_rows + pl.pool_rows) * 512 <= 40 * 1024);
    // (f)
    for (int t = 0; t < 2 * nc; ++t) {
        const fbn::JtGenOp &op = sch.ops[t];
        std::vector<int> cols = op.loads;
        cols.insert(cols.end(), op.prefetch.begin(), op.prefetch.end());
        for (int s : cols) {
            const int made = sch.qi[plan.sep_down[s]];
            CHECK(made < t && sch.ops[made].runs);
            CHECK(pl.col_of[s] >= 0 || (t >= nc && sch.leaf_rc[s]));  // (a recomputed message needs no place)
        }
        if (op.prefetch_ld >= 0)
            CHECK(t >= nc && nc + sch.pi[plan.sep_up[op.prefetch_ld]] < t && pl.dis_of[op.prefetch_ld] >= 0);
    }
}

static int CheckNetwork(const char *name, const fbn::Network &net) {
    fbn::JTPlanHost plan;
    g_case = name;
    CHECK(fbn::BuildJTPlan(net, plan, /*forest=*/true) == FBN_OK);
    CHECK(fbn::JTCodegenEligible(plan, nullptr));
    int cases = 0;
    for (const char *env : kEnvs)
        for (int vm = 0; vm < 2; ++vm)
            for (int fast = 0; fast < 2; ++fast, ++cases) {
                g_case = std::string(name) + (vm ? "|vmajor|" : "|cmajor|") + (fast ? "fast|" : "exact|") + env;
                SetEnv(env);
                const fbn::JtGenOptions opt = fbn::JtGenReadOptions(fast, vm);
                fbn::JtGenTables tab;
                fbn::JtGenSchedule sch;
                fbn::JtGenPlacement pl;
                CHECK(fbn::JtGenPlan(plan, opt, tab, sch, pl) == FBN_OK);
                fbn::JTKernelSpec a, b;
                CHECK(fbn::GenerateJTKernel(plan, fast, vm, a) == FBN_OK && fbn::GenerateJTKernel(plan, fast, vm, b) == FBN_OK);
                CHECK(a.src == b.src && !a.src.empty() && a.wave_entries == fbn::JtGenWaveEntries(plan, pl));  // (g)
                CheckPlaces(plan, opt, tab, sch, pl, a.wave_entries);
            }
    printf("%s: %d cliques, %d cases\n", name, (int)plan.cliques.size(), cases);
    return cases;
}

int main(int argc, char **argv) {
    int cases = 0;
    for (int i = 1; i < std::max(argc, 2); ++i) {
        const char *xml = argc > 1 ? argv[i] : "tests/golden/alarm/alarm.xml";
        fbn::Network net;
        if (fbn::LoadXmlbif(xml, net) != FBN_OK) {
            printf("FAIL: %s: %s\n", xml, fbn::LastError());
            return 1;
        }
        cases += CheckNetwork(xml, net);
    }
    cases += CheckNetwork("seeded60", SeededNetwork(60, 5, 6, 1));
    cases += CheckNetwork("forest120", SeededNetwork(120, 13, 6, 0));
    if (g_fail || g_d_miss) {
        printf("%d cases, %d check(s) failed; (d) as stated missed %d times, at ops whose own need exceeds the limit\n", cases,
               g_fail, g_d_miss);
        return 1;
    }
    printf("jt_codegen_host_check: %d cases ok\n", cases);
    return 0;
}
