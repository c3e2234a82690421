// capi_state.h -- the handles behind include/fastbn.h that own device state (the junction-tree plan,
// the CI-test context) and the helpers of capi_ci.hip that capi_pc.hip also calls.  Internal to
// libfastbn; included by capi_jt.hip, capi_ci.hip and capi_pc.hip.
#ifndef FBN_CAPI_STATE_H
#define FBN_CAPI_STATE_H

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "fbn_device.h"
#include "fbn_internal.h"

namespace fbn {
struct PcSmallOut;    // pc_small.h
struct CiBatchStats;  // pc_internal.h
}
using fbn::DevBuf;

// device (host-only plans: < 0, runs fail with FBN_ERR_NODEV), events, kernel timing
// (fbn_jt_set_kernel_timing), caller streams and the evidence check are DeviceHandle's (fbn_device.h)
struct fbn_jt_plan : fbn::DeviceHandle {
    fbn::JTPlanHost host;
    // One group per kernel variant: its host program, whether the plan is eligible, its device tables.
    struct Interp {  // variant 1: whole case state in a global workspace
        fbn::JTProgram prog;
        DevBuf ops, aux, initv, dig;
    } interp;
    struct Lds {  // variants 0 (default interpreter) / 2, and the exact fixup of 3-5: clique in flight resident in LDS
        fbn::JTProgramLDS prog;
        DevBuf ops, aux, initv, dig;
    } lds;
    struct Streamed {  // variant 4: streamed (virtual) tables, large trees
        fbn::JTProgramV prog;
        bool ok = false;
        DevBuf cl, aux, initv, dig, order, sched, sel;
    } streamed;
    struct Tiled {  // variant 5: tiled, JT_T_C cases x JT_T_L entry slots per wave (fast order)
        fbn::JTProgramT prog;
        bool ok = false;
        DevBuf passes, tab, initv;
    } tiled;
    struct Gen {  // variant 3: plan-specialized kernel
        bool eligible = false;
        // one loaded module (and initial-potential buffer) per arithmetic order, [0] exact, [1] fast:
        // switching the order never unloads a module or rewrites a buffer a queued run may still use
        struct Kernel {
            int state = 0;  // 0 not tried, 1 loaded, -1 failed
            hipModule_t mod = nullptr;
            hipFunction_t fn = nullptr;
            int64_t we = 0, lds = 0;
            DevBuf iv;
        } k[4];  // [fast + 2 * variable-major output]
    } gen;

    // switches (the fbn_jt_set_* entries)
    int waves_per_cu = 0, variant = -1;
    // arithmetic order of the specialized / streamed kernels: 1 = the reference's (bit-identical),
    // 0 = fast (normalizations that cancel left out, within 1e-12), -1 = auto (fast)
    int exact = -1;
    // fbn_jt_set_output_layout: 1 = d_marginals variable-major [SD][ncases]; kernels without a
    // variable-major store path (4, 5) write case-major into mtmp, transposed into place after
    int out_layout = 0;
    bool ev_check = true;  // fbn_jt_set_evidence_check
    bool force_fixup = false;
    // outputs and staging of fbn_jt_run; default outputs of fbn_jt_run_device
    DevBuf evid, labels, marg, mtmp;
    DevBuf ws;             // the main kernel's per-wave workspace
    DevBuf ws_fix, flags;  // the fixup's workspace; one flag per 64-case block (variants 3-5)
    // the last run
    int last_variant = -1;
    int64_t last_nblk = 0;  // its 64-case blocks (flags of variants 3-5)
    DevBuf prof;            // diagnostic per-op-type cycle counters
    bool prof_on = false;
    int last_grid = 0;
    ~fbn_jt_plan() {
        for (auto &k : gen.k)
            if (k.mod) (void)hipModuleUnload(k.mod);
    }
};

// per-slot state of the CI launches: the PC driver keeps two batches in flight (one per half of
// the level's edges) on the ctx stream, so every buffer a launch (re)sizes or writes is per slot
struct CiSlot {
    DevBuf items, indep, df, bcounts, scratch;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, done = nullptr;  // kernel start / end, batch results ready
    int64_t last_bytes = 0;  // input bytes of the last launch in the kernel's own format (roofline)
    // pinned host staging of the driver's batches
    void *h_items = nullptr, *h_res = nullptr;
    size_t h_items_bytes = 0, h_res_bytes = 0;
    int64_t n = 0;  // batch in flight
    bool zc = false, want_df = false;
    ~CiSlot() {
        if (h_items) (void)hipHostFree(h_items);
        if (h_res) (void)hipHostFree(h_res);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (done) (void)hipEventDestroy(done);
    }
};

struct fbn_ci_ctx {
    int device = 0, num_cu = 0, nvars = 0;
    int64_t N = 0;
    std::vector<int32_t> dims;
    DevBuf cols, ddims, g2, p, counts;
    DevBuf stats;  // decision-margin log: {min |p - alpha| bits, #tests within 1e-9 of alpha}
    // bit-sliced columns for marginal tests (ci_bits_count.hip), built on first use
    DevBuf bits, brow, browcnt;  // masks, first row of each variable, sample count per row
    DevBuf pack2;                // 2-bit packed columns (every state count <= 4), built on first use
    bool pack2_ready = false;
    int64_t pack2_W = 0;
    // pair tables of every (i < j), 16 counts each, recorded by level 0 of a PC run and used by its
    // level-1 tests (pair_mode: 0 off, 1 record at the next marginal batch, 2 use if recorded)
    DevBuf pairtab;
    // register-blocked level-0 tasks (ci_bits_pairs_tiled) of the pair range [ptask_t0, ptask_t1)
    DevBuf ptasks;
    int64_t ptask_t0 = -1, ptask_t1 = -1, ptask_n = 0;
    int pair_mode = 0;
    bool pairs_recorded = false;
    // row Grams (ci_bits_gram.hip ci_bits_gram): leading rows = values 0..d-2 of every variable;
    // lead0[v] = v's first leading row, leadrows[r] = the bits row of leading row r
    std::vector<int32_t> row0_host, lead0_host, leadrows_host;
    DevBuf lead0, leadrows;
    bool lead_ready = false;
    // level 0: the Gram of all leading rows (ld = leading-row count) and its tile tasks for the
    // pair range [g0_t0, g0_t1)
    DevBuf gram0, g0tasks;
    int64_t g0_t0 = -1, g0_t1 = -1, g0_ntasks = 0;
    // device-resident level-1 search (CiLevel1Device): edge state, round buffers, per-round open
    // counts (pinned mirror), round events
    DevBuf l1pairs, l1adj, l1adjoff, l1ed, l1pos, l1st, l1sep, l1cnt, l1len, l1off, l1scal, l1open;
    DevBuf l1items, l1counts, l1df, l1indep, l1sstat;  // l1sstat: the offset scan's per-tile status words
    // the level-1 information screen (ci_l1.hip): pairwise I of the complete graph, the kept
    // candidates' positions, the screen's scan status words
    DevBuf l1mi, l1pcnt, l1plist, l1sstat2;
    // level 0's G^2 of every pair written into l1mi by the recording batches (pairs [0, covered) in
    // order; == all pairs: the screen needs no recomputation from the pair tables)
    int64_t l1mi_covered = 0;
    DevBuf keptidx, kepttmp;  // level-0 kept pair indices (CiAllPairsKept)
    // level 0 -> level 1 on the device (CiL0L1Device): per-variable kept counts, upper-part offsets,
    // (E, candidate sets); the side stream copies the flags / edge list to the host meanwhile
    DevBuf kcnt, kupoff, kscal, l1part;
    hipStream_t side = nullptr;
    hipEvent_t side_ev = nullptr, main_ev = nullptr;
    void *h_pairs = nullptr;
    size_t h_pairs_bytes = 0;
    // level-0 Gram on the matrix cores (ci_gram_mfma.hip): FP4 one-hot store (Rp x Kb bytes, built
    // once, stage-major), the tile list of row range [g4_r0, g4_r1), split-K slabs
    DevBuf onehot4, g4tasks, g4slab;
    int64_t g4_r0 = -1, g4_r1 = -1;
    int g4_nt = 0;
    bool onehot4_ready = false;
    // fbn_ci_level0_info: the last level-0 all-pairs launch -- path (1 popcount Gram, 2 MFMA Gram,
    // 3 tiled pairs kernel, 0 none yet), R, Rp, KS, nt, S, shortest / longest slice in stages
    int64_t l0_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int *h_kept = nullptr;
    unsigned *h_open = nullptr;
    void *h_xfer = nullptr;  // pinned staging of level-0 kept pairs / level-1 results (read-back)
    size_t h_xfer_bytes = 0;
    unsigned long long *h_margin = nullptr;  // pinned: reset value, read-back (CiResetMargin)
    hipEvent_t l1ev[2] = {nullptr, nullptr};
    // device-resident skeleton search of small graphs (pc_small.hip): scratch (barrier counters +
    // first-independent words, zeroed once; statistics slots; level-0 pair tables) and the
    // pinned result record the kernel writes
    DevBuf small_scr;
    void *small_zeroed = nullptr;       // scratch whose barrier / first[] words are zeroed (and its size)
    size_t small_zeroed_bytes = 0;
    unsigned small_epoch = 0, small_phase = 0;  // launches so far, grid-barrier phases so far
    fbn::PcSmallOut *h_small = nullptr;
    // fbn_ci_debug_counts: the histogram kernel writes every test's table (stride in ints), 0 off
    int64_t counts_stride = 0;
    // decision band of the bit-sliced G^2 kernel for alpha = band_alpha (ci_chisq.h fbn_chisq_band):
    // [lo, hi] per df 1..kBandDf, then delta; host copy kept alive for the async upload
    DevBuf band;
    std::vector<double> band_host;
    double band_alpha = -1.0;
    int band_n = 0;
    bool bits_ready = false;
    int64_t bits_W = 0;
    CiSlot slot[2];
    hipStream_t stream = nullptr;  // the PC driver's rounds (pinned staging, one sync per round)
    std::vector<hipStream_t> streams_used;  // caller streams of fbn_ci_run (drained by fbn_ci_ctx_destroy)
    float last_ms = 0.f;
    bool timing = true;  // HIP events around every CI kernel (fbn_ci_set_kernel_timing)
    // parameter learning (param_counts.hip): family descriptors, their columns / key strides, the
    // 32-bit family tables (zeroed by every fbn_param_counts), fbn_param_set_tuning (0 = default)
    DevBuf par_fam, par_col, par_str, par_tab;
    int64_t par_slice = 0, par_lds = 0;
    // score-based structure learning (capi_hc.hip, hc_score.hip): L[n] = n ln n for n <= N (built on the
    // host and uploaded by the first scoring call), the penalty terms and the two results per family of a
    // chunk, fbn_hc_set_tuning's chunk cap (0 = FBN_PARAM_MAX_CELLS)
    DevBuf hc_L, hc_pen, hc_out;
    bool hc_table_ready = false;
    int64_t hc_chunk = 0;
    ~fbn_ci_ctx() {
        if (h_open) (void)hipHostFree(h_open);
        if (h_margin) (void)hipHostFree(h_margin);
        if (h_kept) (void)hipHostFree(h_kept);
        if (h_xfer) (void)hipHostFree(h_xfer);
        if (h_small) (void)hipHostFree(h_small);
        for (auto &e : l1ev)
            if (e) (void)hipEventDestroy(e);
        if (h_pairs) (void)hipHostFree(h_pairs);
        if (side_ev) (void)hipEventDestroy(side_ev);
        if (main_ev) (void)hipEventDestroy(main_ev);
        if (side) (void)hipStreamDestroy(side);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// helpers of capi_ci.hip that the PC-stable seam (capi_pc.hip) calls too
namespace fbn {

// df <= 36 covers every bit-sliced test (<= 4 states, <= 1 conditioning variable: 4 * 3 * 3)
constexpr int kBandDf = 36;
constexpr int kBandDfMax = 256;  // larger df (few tests, deep levels): p evaluated

// the bit-sliced path's sample threshold (CiBitsEligible, pc_internal.h)
constexpr int64_t kCiBitsMinSamples = 4096;

int CiBand(fbn_ci_ctx *c, double alpha, hipStream_t s, const double **out, int *nband, int want_df = 0);
int CiResetMargin(fbn_ci_ctx *c);
int CiReadMargin(fbn_ci_ctx *c, double *min_margin, int64_t *near_alpha, bool own_stream_only = false);
int CiLeadEnsure(fbn_ci_ctx *c, hipStream_t s);
int CiBitsEnsure(fbn_ci_ctx *c, hipStream_t s);
int CiPack2Ensure(fbn_ci_ctx *c, hipStream_t s);
// One batch of n tests with d conditioning variables for CiLaunchDevice (filled by name).
struct CiBatchReq {
    const int32_t *items = nullptr;  // host copy [n][2 + d] (validated unless pre); null with all_pairs
    int64_t n = 0;
    int d = 0;
    double alpha = 0.05;  // (the count-only callers, fbn_ci_counts / fbn_ci_debug_counts, leave it)
    bool want_g2p = false;          // G^2 and p into c->g2 / c->p (else decisions only, through the band)
    int32_t *counts_dev = nullptr;  // optional: test 0's table (every test's with c->counts_stride)
    int k = 0;                      // the slot whose buffers and events the batch uses
    // optional device-visible (pinned, mapped) host buffers the kernels read the items from and write
    // the decisions to directly -- no staging copies for the small batches of a latency-bound round
    const int32_t *zc_items = nullptr;
    uint8_t *zc_indep = nullptr;
    int32_t *zc_df = nullptr;
    const CiBatchStats *pre = nullptr;  // the items' statistics, from a caller that generated them: no validation
    bool all_pairs = false;  // no items: test t is pair pair0 + t of the complete graph (bit-sliced path only)
    int64_t pair0 = 0;
};
int CiLaunchDevice(fbn_ci_ctx *c, const CiBatchReq &q, hipStream_t s);

}  // namespace fbn

#endif
