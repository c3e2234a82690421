// capi_jt.hip -- the junction-tree entries of include/fastbn.h: plan creation and upload, the switches,
// the specialized kernel's build, and the run path: JtRunDevice chooses the variant and hands a JtRun
// record to that variant's one function (RunLds, RunInterp, RunSpecialized, RunStreamed, RunTiled);
// scoring.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "capi_state.h"
#include "launchers.h"
#include "sample_model.h"

using fbn::SetError;
using fbn::Upload;

extern "C" {

// ------------------------------------------------------------------ junction tree
static int JtUpload(fbn_jt_plan *p) {
    auto &g = p->interp;
    auto &l = p->lds;
    int rc;
    if ((rc = Upload(g.ops, g.prog.ops)) || (rc = Upload(g.aux, g.prog.aux)) || (rc = Upload(g.initv, g.prog.initv)) ||
        (rc = Upload(g.dig, g.prog.dig)) || (rc = Upload(l.ops, l.prog.ops)) || (rc = Upload(l.aux, l.prog.aux)) ||
        (rc = Upload(l.initv, l.prog.initv)) || (rc = Upload(l.dig, l.prog.dig)))
        return rc;
    auto &v = p->streamed;
    if (v.ok && ((rc = Upload(v.cl, v.prog.cl)) || (rc = Upload(v.aux, v.prog.aux)) ||
                 (rc = Upload(v.initv, v.prog.initv)) || (rc = Upload(v.dig, v.prog.dig)) ||
                 (rc = Upload(v.order, v.prog.order)) || (rc = Upload(v.sched, v.prog.sched)) ||
                 (rc = Upload(v.sel, v.prog.vsel))))
        return rc;
    auto &t = p->tiled;
    if (t.ok && ((rc = Upload(t.passes, t.prog.passes)) || (rc = Upload(t.tab, t.prog.tab)) ||
                 (rc = Upload(t.initv, t.prog.initv))))
        return rc;
    return p->evidence.Attach(p->host.dom);  // (fbn_jt_score_terms_device reads the same state counts)
}

// forest: a disconnected moral graph gives one tree per component (fbn_jt_forest_plan_create)
static int JtPlanCreate(const fbn_network *net, int device, bool forest, fbn_jt_plan **out) {
    if (!net || !out) return SetError(FBN_ERR_ARG, "null pointer");
    auto p = std::unique_ptr<fbn_jt_plan>(new (std::nothrow) fbn_jt_plan());
    if (!p) return SetError(FBN_ERR_NOMEM, "out of memory");
    static const bool ptime = fbn::KnobSet("FBN_PLAN_TIMING");  // diagnostic: plan phases
    auto tp0 = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (!ptime) return;
        const auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "plan %s: %.1f ms\n", what, std::chrono::duration<double, std::milli>(t - tp0).count());
        tp0 = t;
    };
    int rc = fbn::BuildJTPlan(net->net, p->host, forest);
    if (rc) return rc;
    lap("structure");
    rc = fbn::CompileJTProgram(p->host, p->interp.prog);
    if (rc) return rc;
    rc = fbn::CompileJTProgramLDS(p->host, p->lds.prog);
    if (rc) return rc;
    lap("interpreter programs");
    rc = fbn::CompileJTProgramV(p->host, p->streamed.prog);
    if (rc && rc != FBN_ERR_LIMIT) return rc;
    p->streamed.ok = rc == FBN_OK;
    if (!p->streamed.ok) p->streamed.prog = fbn::JTProgramV();
    lap("streamed program");
    // tiled variant: factors of a clique phase staged in LDS up to this many bytes per wave
    // LDS factor budget per workgroup: 6016 B + the bin and total rows = 10 KB, so 16 one-wave
    // workgroups fit a CU's 160 KB
    constexpr int kTileLdsBytes = 6016;
    rc = fbn::CompileJTProgramT(p->host, p->tiled.prog, kTileLdsBytes);
    if (rc && rc != FBN_ERR_LIMIT) return rc;
    p->tiled.ok = rc == FBN_OK;
    if (!p->tiled.ok) p->tiled.prog = fbn::JTProgramT();
    lap("tiled program");
    p->gen.eligible = fbn::JTCodegenEligible(p->host, nullptr);
    p->device = device;  // device < 0: host-only plan (info / dump), runs fail with FBN_ERR_NODEV
    if (device >= 0 && ((rc = p->Attach(device)) || (rc = JtUpload(p.get())))) return rc;
    *out = p.release();
    return FBN_OK;
}

int fbn_jt_plan_create(const fbn_network *net, int device, fbn_jt_plan **out) {
    return JtPlanCreate(net, device, false, out);
}

int fbn_jt_forest_plan_create(const fbn_network *net, int device, fbn_jt_plan **out) {
    return JtPlanCreate(net, device, true, out);
}

int fbn_jt_plan_components(const fbn_jt_plan *p, int32_t *component_of_node, int32_t *num_components) {
    if (!p || !num_components) return SetError(FBN_ERR_ARG, "null pointer");
    *num_components = p->host.num_components;
    if (component_of_node) std::copy(p->host.component_of_node.begin(), p->host.component_of_node.end(), component_of_node);
    return FBN_OK;
}

int fbn_jt_plan_info_get(const fbn_jt_plan *p, fbn_jt_plan_info *info) {
    if (!p || !info) return SetError(FBN_ERR_ARG, "null pointer");
    memset(info, 0, sizeof *info);
    info->num_nodes = p->host.num_nodes;
    info->num_cliques = (int32_t)p->host.cliques.size();
    info->num_separators = (int32_t)p->host.seps.size();
    info->num_levels = (int32_t)p->host.levels.size();
    info->root = p->host.root;
    info->sum_dom = p->interp.prog.sum_dom;
    for (auto &t : p->host.cliques) info->clique_entries += t.size();
    for (auto &t : p->host.seps) info->separator_entries += t.size();
    info->algorithmic_bytes_per_case =
        16 * (info->clique_entries + info->separator_entries) + 8 * (int64_t)info->sum_dom + info->num_nodes;
    info->num_ops = (int32_t)p->interp.prog.ops.size();
    info->max_vars_per_table = p->interp.prog.max_vars;
    info->specialized_eligible = p->gen.eligible ? 1 : 0;
    info->variant = p->variant >= 0 ? p->variant : p->last_variant;
    info->streamed_eligible = p->streamed.ok ? 1 : 0;
    info->streamed_waves = JT_V_WAVES;
    info->streamed_split_efficiency = p->streamed.ok ? p->streamed.prog.split_efficiency : 0.0;
    const auto &t = p->tiled.prog;
    info->tiled_eligible = p->tiled.ok ? 1 : 0;
    info->tiled_passes = (int32_t)t.passes.size();
    info->tiled_entry_visits = t.entry_visits;
    info->tiled_lds_bytes = t.lds_bytes;
    info->tiled_table_bytes = (int64_t)t.tab.size() * 4;
    return FBN_OK;
}

int fbn_jt_stream_schedule(const fbn_jt_plan *p, int32_t *order, int64_t order_cap, int32_t *sched,
                           int64_t sched_cap, int64_t *n_order, int64_t *n_sched) {
    if (!p) return SetError(FBN_ERR_ARG, "null pointer");
    if (!p->streamed.ok) return SetError(FBN_ERR_LIMIT, "plan not eligible for the streamed kernel");
    const auto &v = p->streamed.prog;
    if (n_order) *n_order = (int64_t)v.order.size();
    if (n_sched) *n_sched = (int64_t)v.sched.size();
    if (order) {
        if (order_cap < (int64_t)v.order.size()) return SetError(FBN_ERR_ARG, "order buffer too small");
        std::copy(v.order.begin(), v.order.end(), order);
    }
    if (sched) {
        if (sched_cap < (int64_t)v.sched.size()) return SetError(FBN_ERR_ARG, "sched buffer too small");
        std::copy(v.sched.begin(), v.sched.end(), sched);
    }
    return FBN_OK;
}

int fbn_jt_tile_program(const fbn_jt_plan *p, int32_t *passes, int32_t *tab, double *initv, int64_t *geometry) {
    if (!p) return SetError(FBN_ERR_ARG, "null pointer");
    if (!p->tiled.ok) return SetError(FBN_ERR_LIMIT, "plan not eligible for the tiled kernel");
    static_assert(sizeof(JtTPass) == 33 * 4, "JtTPass = 33 int32");
    const auto &t = p->tiled.prog;
    if (passes) memcpy(passes, t.passes.data(), t.passes.size() * sizeof(JtTPass));
    if (tab) memcpy(tab, t.tab.data(), t.tab.size() * 4);
    if (initv) memcpy(initv, t.initv.data(), t.initv.size() * 8);
    if (geometry) {
        const int64_t g[8] = {(int64_t)t.passes.size(), (int64_t)t.tab.size(), (int64_t)t.initv.size(), t.scr_row,
                              t.red_row, t.store_rows, JT_T_C, JT_T_L};
        memcpy(geometry, g, sizeof g);
    }
    return FBN_OK;
}

int fbn_jt_plan_dump(const fbn_jt_plan *p, const char *plan_path, const char *init_path) {
    if (!p || !plan_path || !init_path) return SetError(FBN_ERR_ARG, "null pointer");
    const auto &h = p->host;
    FILE *f = fopen(plan_path, "w");
    if (!f) return SetError(FBN_ERR_IO, "cannot write %s", plan_path);
    fprintf(f, "cliques %zu\n", h.cliques.size());
    for (size_t i = 0; i < h.cliques.size(); ++i) {
        const auto &t = h.cliques[i];
        fprintf(f, "c %zu %zu %lld", i, t.vars.size(), (long long)t.size());
        for (int v : t.vars) fprintf(f, " %d", v);
        fprintf(f, " | up %d | down", h.clique_up[i]);
        for (int d : h.clique_down[i]) fprintf(f, " %d", d);
        fprintf(f, "\n");
    }
    fprintf(f, "seps %zu\n", h.seps.size());
    for (size_t i = 0; i < h.seps.size(); ++i) {
        const auto &t = h.seps[i];
        fprintf(f, "s %zu %zu %lld", i, t.vars.size(), (long long)t.size());
        for (int v : t.vars) fprintf(f, " %d", v);
        fprintf(f, " | up %d | down %d\n", h.sep_up[i], h.sep_down[i]);
    }
    fprintf(f, "root %d\n", h.root);
    if (h.roots.size() > 1) {  // a forest: the roots of all trees, in component order
        fprintf(f, "roots %zu", h.roots.size());
        for (int r : h.roots) fprintf(f, " %d", r);
        fprintf(f, "\n");
    }
    fprintf(f, "levels %zu\n", h.levels.size());
    for (size_t l = 0; l < h.levels.size(); ++l) {
        fprintf(f, "level %zu %c", l, (l % 2) ? 's' : 'c');
        for (int x : h.levels[l]) fprintf(f, " %d", x);
        fprintf(f, "\n");
    }
    fclose(f);
    f = fopen(init_path, "w");
    if (!f) return SetError(FBN_ERR_IO, "cannot write %s", init_path);
    for (size_t i = 0; i < h.cliques.size(); ++i) {
        fprintf(f, "c %zu %lld", i, (long long)h.cliques[i].size());
        for (double v : h.cliques[i].pot) fprintf(f, " %.17g", v);
        fprintf(f, "\n");
    }
    fclose(f);
    return FBN_OK;
}

constexpr int kJtVFast = 1 << 12;  // jt_virt.hip kVFast
// auto (-1) = the fast arithmetic order for every kernel that has one; exact (1) on request
static bool JtFast(const fbn_jt_plan *p) { return p->exact != 1; }

int fbn_jt_set_waves_per_cu(fbn_jt_plan *p, int waves) {
    if (!p || waves < 0 || waves > 32) return SetError(FBN_ERR_ARG, "waves per CU must be 0..32");
    p->waves_per_cu = waves;
    return FBN_OK;
}

int fbn_jt_set_variant(fbn_jt_plan *p, int variant) {
    if (!p || variant < -1 || variant > 5)
        return SetError(FBN_ERR_ARG, "variant must be -1 (auto), 0 (LDS), 1 (global), 2 (LDS, IEEE division), "
                                     "3 (specialized), 4 (streamed) or 5 (tiled)");
    if (variant == 3 && !p->gen.eligible) return SetError(FBN_ERR_ARG, "plan not eligible for the specialized kernel");
    if (variant == 4 && !p->streamed.ok) return SetError(FBN_ERR_ARG, "plan not eligible for the streamed kernel");
    if (variant == 5 && !p->tiled.ok) return SetError(FBN_ERR_ARG, "plan not eligible for the tiled kernel");
    p->variant = variant;
    return FBN_OK;
}

// the plan-specialized kernel of the current arithmetic order, loaded (cache) or compiled (hiprtc)
// once per plan and order; both orders stay loaded
static fbn_jt_plan::Gen::Kernel &GenCur(fbn_jt_plan *p, bool vm) { return p->gen.k[(JtFast(p) ? 1 : 0) + (vm ? 2 : 0)]; }
// source, constant input and launch facts of the specialized kernel of the plan's current order
static int GenSpec(const fbn_jt_plan *p, bool vm, fbn::JTKernelSpec &spec) {
    if (!p->gen.eligible) return SetError(FBN_ERR_ARG, "plan not eligible for codegen");
    return fbn::GenerateJTKernel(p->host, JtFast(p), vm, spec);
}
static int GenSpec(const fbn_jt_plan *p, fbn::JTKernelSpec &spec) { return GenSpec(p, p->out_layout == 1, spec); }

static int GenEnsure(fbn_jt_plan *p, bool vm) {
    auto &k = GenCur(p, vm);
    if (k.state == 1) return FBN_OK;
    if (k.state == -1) return FBN_ERR_HIP;
    k.state = -1;
    fbn::JTKernelSpec spec;
    int rc = GenSpec(p, vm, spec);
    if (rc) return rc;
    k.we = spec.wave_entries, k.lds = spec.lds_bytes;
    std::vector<char> code;
    if ((rc = fbn::JitCodeObject(spec.src, code))) return rc;
    FBN_HIP(hipModuleLoadData(&k.mod, code.data()));
    FBN_HIP(hipModuleGetFunction(&k.fn, k.mod, "fbn_jt_gen"));
    if ((rc = Upload(k.iv, spec.initv))) return rc;  // (a new buffer: no run uses it yet)
    k.state = 1;
    return FBN_OK;
}

// diagnostic: per-op-type cycle totals of the LDS variant (s_memtime, summed over waves)
int fbn_jt_debug_op_cycles(fbn_jt_plan *p, int enable, unsigned long long *cycles /* [10] or NULL */) {
    if (!p) return SetError(FBN_ERR_ARG, "null pointer");
    if (cycles && p->prof_on && p->last_grid > 0) {
        std::vector<unsigned long long> h((size_t)p->last_grid * 16);
        FBN_HIP(hipDeviceSynchronize());
        FBN_HIP(hipMemcpy(h.data(), p->prof.p, h.size() * 8, hipMemcpyDeviceToHost));
        for (int k = 0; k < 10; ++k) {
            cycles[k] = 0;
            for (int w = 0; w < p->last_grid; ++w) cycles[k] += h[(size_t)w * 16 + k];
        }
    }
    p->prof_on = enable != 0;
    return FBN_OK;
}

int fbn_jt_kernel_source(const fbn_jt_plan *p, char *buf, int64_t cap, int64_t *len) {
    if (!p) return SetError(FBN_ERR_ARG, "null pointer");
    fbn::JTKernelSpec spec;
    if (int rc = GenSpec(p, spec)) return rc;
    const std::string &src = spec.src;
    if (len) *len = (int64_t)src.size() + 1;
    if (buf && cap > 0) {
        const size_t n = std::min<size_t>((size_t)cap - 1, src.size());
        memcpy(buf, src.data(), n);
        buf[n] = 0;
    }
    return FBN_OK;
}

int fbn_jt_kernel_cache_path(const fbn_jt_plan *p, char *buf, int64_t cap) {
    if (!p || !buf || cap <= 0) return SetError(FBN_ERR_ARG, "bad argument");
    fbn::JTKernelSpec spec;
    if (int rc = GenSpec(p, spec)) return rc;
    snprintf(buf, (size_t)cap, "%s", fbn::JitCachePath(spec.src).c_str());
    return FBN_OK;
}

int fbn_jt_kernel_placement(const fbn_jt_plan *p, int64_t *rows) {
    if (!p || !rows) return SetError(FBN_ERR_ARG, "null pointer");
    fbn::JTKernelSpec spec;
    if (int rc = GenSpec(p, spec)) return rc;
    const fbn::JTPlacement &pl = spec.place;
    const int64_t r[8] = {pl.global[0], pl.global[1], pl.lds[0], pl.lds[1],
                          pl.reg[0], pl.reg[1], pl.workspace_rows, pl.lds_pool_rows};
    std::copy(r, r + 8, rows);
    return FBN_OK;
}

int fbn_jt_set_exact(fbn_jt_plan *p, int exact) {
    if (!p || exact < -1 || exact > 1) return SetError(FBN_ERR_ARG, "exact must be -1 (auto), 0 (fast) or 1 (exact)");
    p->exact = exact;
    return FBN_OK;
}

int fbn_jt_debug_force_fixup(fbn_jt_plan *p, int enable) {
    if (!p) return SetError(FBN_ERR_ARG, "null pointer");
    p->force_fixup = enable != 0;
    return FBN_OK;
}

int fbn_jt_debug_flagged_blocks(fbn_jt_plan *p, int64_t *count) {
    if (!p || !count) return SetError(FBN_ERR_ARG, "null pointer");
    *count = 0;
    if (p->last_nblk <= 0 || !p->flags.p) return FBN_OK;
    std::vector<int> h((size_t)p->last_nblk);
    FBN_HIP(hipDeviceSynchronize());
    FBN_HIP(hipMemcpy(h.data(), p->flags.p, h.size() * 4, hipMemcpyDeviceToHost));
    for (int f : h) *count += f != 0;
    return FBN_OK;
}

int fbn_jt_kernel_build(const fbn_jt_plan *p) {
    if (!p) return SetError(FBN_ERR_ARG, "null pointer");
    fbn::JTKernelSpec spec;
    if (int rc = GenSpec(p, spec)) return rc;
    std::vector<char> code;
    return fbn::JitCodeObject(spec.src, code);
}

int fbn_jt_kernel_options(char *buf, int64_t cap) {
    if (!buf || cap <= 0) return SetError(FBN_ERR_ARG, "bad argument");
    std::string o;
    for (int i = 0; i < fbn::kJitNumOptions; ++i) o += std::string(fbn::kJitOptions[i]) + "\n";
    snprintf(buf, (size_t)cap, "%s", o.c_str());
    return FBN_OK;
}

// ------------------------------------------------------------------ the run path
// One run on the device, filled by name by JtRunDevice for the function of the chosen variant.
struct JtRun {
    int variant = 0;
    const int8_t *evid = nullptr;  // [ncases][V]
    int64_t ncases = 0, nblk = 0;  // nblk: 64-case blocks
    int32_t *labels = nullptr;
    double *marg = nullptr;  // where the kernels store: the caller's buffer, or the scratch transposed after
    hipStream_t s = nullptr;
    bool vm = false;  // the kernels store marg variable-major themselves (never with the scratch)
};

// diagnostic cycle counters of a launch (fbn_jt_debug_op_cycles): rows of 16, zeroed on the stream; NULL when off
static int ProfileRows(fbn_jt_plan *p, int rows, hipStream_t s, unsigned long long **out) {
    *out = nullptr;
    if (!p->prof_on) return FBN_OK;
    if (int rc = p->prof.ensure((size_t)rows * 16 * 8)) return rc;
    FBN_HIP(hipMemsetAsync(p->prof.p, 0, (size_t)rows * 16 * 8, s));
    p->last_grid = rows;
    *out = p->prof.as<unsigned long long>();
    return FBN_OK;
}

// LDS variant geometry: waves per CU and the number of LDS table rows (64 lanes x 8 B each)
static void LdsGeometry(const fbn_jt_plan *p, int *waves, int *cap) {
    const int64_t row = 64 * 8, tmax = std::max<int64_t>(1, p->lds.prog.max_table);
    int w = p->waves_per_cu;
    if (w <= 0) w = (int)std::max<int64_t>(1, std::min<int64_t>(8, fbn::kCuLdsBytes / (tmax * row)));
    int64_t c = std::min<int64_t>(tmax, (fbn::kCuLdsBytes / w) / row);
    *waves = w;
    *cap = (int)std::max<int64_t>(1, c);
}

// LDS interpreter launch with workspace ws: the whole run (flags == NULL), or in fixup mode only the
// 64-case blocks whose flag is set
static int LaunchLds(fbn_jt_plan *p, const JtRun &r, DevBuf &ws, const int *flags, bool force_exact) {
    const auto &l = p->lds.prog;
    const int V = p->host.num_nodes, SD = l.sum_dom, nc = l.num_cliques;
    int wpc, cap, rc;
    LdsGeometry(p, &wpc, &cap);
    const bool spill = cap < l.max_table;
    // fixup mode: flagged blocks are rare; one wave per CU scans the flags 64 at a time (the launch
    // follows every specialized / tiled launch: ~3 us per call on ALARM, grids of 4 / 16 / 256 waves
    // measured alike)
    int grid = (int)std::min<int64_t>(r.nblk, flags ? (int64_t)p->num_cu : (int64_t)p->num_cu * wpc);
    const int64_t store_off = 0, den_off = l.store_entries, sep_off = den_off + nc, spill_off = sep_off + l.sep_entries;
    const int64_t wave_entries = spill_off + (spill ? l.max_table - cap : 0);
    if (flags)  // fixup mode: at most ~2 GiB of workspace (large trees need ~100 MB per wave)
        grid = (int)std::max<int64_t>(1, std::min<int64_t>(grid, ((int64_t)2 << 30) / (wave_entries * 64 * 8 + nc * 64 * 4)));
    const size_t ws_d = (size_t)grid * wave_entries * 64 * 8;
    const size_t ws_i = (size_t)grid * nc * 64 * 4;
    if ((rc = ws.ensure(ws_d + ws_i))) return rc;
    unsigned long long *prof = nullptr;
    if (!flags && (rc = ProfileRows(p, grid, r.s, &prof))) return rc;
    JtLdsArgs a{};
    a.par.ncases = r.ncases, a.par.wave_entries = wave_entries;
    a.par.store_off = store_off, a.par.den_off = den_off, a.par.sep_off = sep_off, a.par.spill_off = spill_off;
    a.par.nops = (int)l.ops.size(), a.par.V = V, a.par.SD = SD, a.par.nc = nc, a.par.cap = cap;
    a.par.force_exact = force_exact, a.par.vmajor = r.vm ? 1 : 0;
    a.par.flags = flags;
    a.ops = p->lds.ops.as<JtOp>(), a.aux = p->lds.aux.as<int32_t>();
    a.initv = p->lds.initv.as<double>(), a.dig = p->lds.dig.as<uint64_t>();
    a.evid = r.evid, a.marg = r.marg, a.labels = r.labels;
    a.ws = ws.as<double>(), a.wsi = reinterpret_cast<int32_t *>(ws.as<char>() + ws_d);
    a.spill = spill, a.grid = grid;
    a.prof = prof;
    hipError_t e = fbn_jt_lds_launch(&a, r.s);
    if (e != hipSuccess) return SetError(FBN_ERR_HIP, "jt kernel launch: %s", hipGetErrorString(e));
    return FBN_OK;
}

// The tail of variants 3-5, after their kernel: the blocks it flagged (denominators or pass totals that
// left the range the fast arithmetic is checked for) recomputed exactly by the LDS interpreter.  The
// flags are ensured by the variant, before its kernel.  recompute = false: the flags only.
static int FixupTail(fbn_jt_plan *p, const JtRun &r, bool recompute = true) {
    if (p->force_fixup) FBN_HIP(hipMemsetAsync(p->flags.p, 1, (size_t)r.nblk * 4, r.s));  // testing only
    return recompute ? LaunchLds(p, r, p->ws_fix, p->flags.as<int>(), false) : FBN_OK;
}

// Each variant: size the persistent grid, allocate, open the timed interval (Begin), enqueue.

// variants 0 / 2: LDS interpreter (2: IEEE division)
static int RunLds(fbn_jt_plan *p, const JtRun &r) {
    if (int rc = p->Begin(r.s)) return rc;
    return LaunchLds(p, r, p->ws, nullptr, r.variant == 2);
}

// variant 1: global interpreter
static int RunInterp(fbn_jt_plan *p, const JtRun &r) {
    const auto &g = p->interp.prog;
    const int nc = g.num_cliques;
    const int wpc = p->waves_per_cu > 0 ? p->waves_per_cu : 8;
    // persistent waves: cap the per-wave workspaces at 80 % of the free HBM (more resident waves
    // = more memory-level parallelism: this variant is latency bound on large plans)
    const size_t per_wave = (size_t)g.state_entries * 64 * 8 + (size_t)nc * 64 * 4;
    const int grid = (int)fbn::ClampGridToFreeMemory(std::min<int64_t>(r.nblk, (int64_t)p->num_cu * wpc), per_wave,
                                                     p->ws.bytes, fbn::kMemShare80);
    const size_t ws_d = (size_t)grid * g.state_entries * 64 * 8;
    const size_t ws_i = (size_t)grid * nc * 64 * 4;
    int rc;
    if ((rc = p->ws.ensure(ws_d + ws_i)) || (rc = p->Begin(r.s))) return rc;
    JtArgs a{};
    a.ops = p->interp.ops.as<JtOp>(), a.aux = p->interp.aux.as<int32_t>();
    a.initv = p->interp.initv.as<double>(), a.dig = p->interp.dig.as<uint64_t>();
    a.evid = r.evid, a.marg = r.marg, a.labels = r.labels;
    a.ws = p->ws.as<double>(), a.wsi = reinterpret_cast<int32_t *>(p->ws.as<char>() + ws_d);
    a.ncases = r.ncases, a.NE = g.state_entries;
    a.nops = (int)g.ops.size(), a.V = p->host.num_nodes, a.SD = g.sum_dom, a.nc = nc;
    a.vmajor = r.vm ? 1 : 0;
    hipError_t e = fbn_jt_launch(&a, grid, r.s);
    if (e != hipSuccess) return SetError(FBN_ERR_HIP, "jt kernel launch: %s", hipGetErrorString(e));
    return FBN_OK;
}

// variant 3: plan-specialized kernel; one wave (64 cases) per SIMD: the clique in flight occupies the
// register file (+ LDS tail)
static int RunSpecialized(fbn_jt_plan *p, const JtRun &r) {
    const auto &gk = GenCur(p, r.vm);  // (the kernel JtChooseVariant ensured: a run of variant 3 has vm == vm3)
    int wpc = p->waves_per_cu > 0 ? p->waves_per_cu : 4;
    if (gk.lds > 0) wpc = std::max<int>(1, std::min<int64_t>(wpc, fbn::kCuLdsBytes / gk.lds));
    const int grid = (int)std::min<int64_t>(r.nblk, (int64_t)p->num_cu * wpc);
    int rc;
    if ((rc = p->ws.ensure((size_t)grid * gk.we * 64 * 8)) || (rc = p->flags.ensure((size_t)r.nblk * 4)) ||
        (rc = p->Begin(r.s)))
        return rc;
    const int8_t *a_ev = r.evid;
    double *a_marg = r.marg, *a_ws = p->ws.as<double>();
    int32_t *a_lab = r.labels;
    int *a_flags = p->flags.as<int>();
    const double *a_iv = gk.iv.as<double>();
    long long a_n = r.ncases;
    unsigned long long *a_prof = nullptr;  // diagnostic: only kernels generated with FBN_JT_PROFILE=1 write it
    if ((rc = ProfileRows(p, grid, r.s, &a_prof))) return rc;
    void *args[] = {&a_ev, &a_marg, &a_lab, &a_ws, &a_flags, &a_iv, &a_n, &a_prof};
    FBN_HIP(hipModuleLaunchKernel(gk.fn, grid, 1, 1, 64, 1, 1, (unsigned)gk.lds, r.s, args, nullptr));
    return FixupTail(p, r);
}

// variant 4: streamed tables: small register footprint, many resident waves; the per-wave store holds
// only separator messages and denominators.  Workgroups of JT_V_WAVES waves, one 64-case block per
// workgroup (persistent).
static int RunStreamed(fbn_jt_plan *p, const JtRun &r) {
    const auto &v = p->streamed.prog;
    const int V = p->host.num_nodes, nc = p->interp.prog.num_cliques;
    const int wpc = p->waves_per_cu > 0 ? p->waves_per_cu : 16;
    const size_t per_blk_d = (size_t)v.store_rows * 64 * 8, per_blk_i = (size_t)(nc + V) * 64 * 4;
    const int grid = (int)fbn::ClampGridToFreeMemory(
        std::min<int64_t>(r.nblk, std::max<int64_t>(1, (int64_t)p->num_cu * wpc / JT_V_WAVES)), per_blk_d + per_blk_i,
        p->ws.bytes, fbn::kMemShare80);
    const size_t ws_d = (size_t)grid * per_blk_d;
    int rc;
    if ((rc = p->ws.ensure(ws_d + (size_t)grid * per_blk_i)) || (rc = p->flags.ensure((size_t)r.nblk * 4)) ||
        (rc = p->Begin(r.s)))
        return rc;
    // diagnostic ablation only (tools/): skip pass types, wrong results, no fixup
    const char *vdebug_env = fbn::KnobValue("FBN_JT_VDEBUG");
    const int vdebug = vdebug_env ? atoi(vdebug_env) : 0;
    auto &d = p->streamed;
    hipError_t e = fbn_jt_virt_launch(d.cl.as<JtVClique>(), d.aux.as<int32_t>(), d.initv.as<double>(),
                                      d.dig.as<uint64_t>(), d.order.as<int32_t>(), d.sched.as<int32_t>(),
                                      d.sel.as<int32_t>(), r.evid, r.marg, r.labels, p->ws.as<double>(),
                                      reinterpret_cast<int32_t *>(p->ws.as<char>() + ws_d), p->flags.as<int>(),
                                      r.ncases, v.store_rows, v.scratch_row, v.scratch_rows, nc, V,
                                      p->interp.prog.sum_dom, grid, vdebug | (JtFast(p) ? kJtVFast : 0), r.s);
    if (e != hipSuccess) return SetError(FBN_ERR_HIP, "jt kernel launch: %s", hipGetErrorString(e));
    return FixupTail(p, r, !vdebug_env);
}

// variant 5: tiled; workgroups of t.waves waves, one case group (JT_T_C cases) each, persistent; per
// workgroup its message store
static int RunTiled(fbn_jt_plan *p, const JtRun &r) {
    const auto &t = p->tiled.prog;
    const int64_t ncg = (r.ncases + JT_T_C - 1) / JT_T_C;
    const int wpc = p->waves_per_cu > 0 ? p->waves_per_cu : 16;
    const size_t per_wg = (size_t)t.store_rows * JT_T_C * 8;
    const int grid = (int)fbn::ClampGridToFreeMemory(
        std::min<int64_t>(ncg, std::max<int64_t>(1, (int64_t)p->num_cu * wpc / t.waves)), per_wg, p->ws.bytes,
        fbn::kMemShare80);
    int rc;
    if ((rc = p->ws.ensure((size_t)grid * per_wg)) || (rc = p->flags.ensure((size_t)r.nblk * 4))) return rc;
    // (this variant alone zeroes the flags before its kernel; the memsets here come before ev0)
    FBN_HIP(hipMemsetAsync(p->flags.p, 0, (size_t)r.nblk * 4, r.s));
    unsigned long long *tprof = nullptr;  // diagnostic: per-phase cycles, one row
    if ((rc = ProfileRows(p, 1, r.s, &tprof)) || (rc = p->Begin(r.s))) return rc;
    hipError_t e = fbn_jt_tile_launch(p->tiled.passes.as<JtTPass>(), (int)t.passes.size(), p->tiled.tab.as<int32_t>(),
                                      p->tiled.initv.as<double>(), r.evid, r.marg, r.labels, p->ws.as<double>(),
                                      p->flags.as<int>(), r.ncases, t.store_rows, t.scr_row, t.red_row,
                                      p->host.num_nodes, p->interp.prog.sum_dom, (int)t.lds_bytes, grid, t.waves,
                                      tprof, r.s);
    if (e != hipSuccess) return SetError(FBN_ERR_HIP, "jt kernel launch: %s", hipGetErrorString(e));
    return FixupTail(p, r);
}

// vm3: the run wants variable-major marginals and the specialized kernel can store them (GenCur's index)
static int JtChooseVariant(fbn_jt_plan *p, bool vm3, int *variant) {
    *variant = p->variant;
    if (*variant == 3) return GenEnsure(p, vm3);
    if (*variant != -1) return FBN_OK;
    // specialized kernel when eligible; else the streamed kernel (1.5-2x the interpreters on
    // ALARM and the Munin-like network); the interpreters only for plans it cannot take
    if (p->gen.eligible && GenEnsure(p, vm3) == FBN_OK) *variant = 3;
    else if (p->tiled.ok && JtFast(p)) *variant = 5;  // (fast arithmetic order only)
    else if (p->streamed.ok) *variant = 4;
    else *variant = (p->lds.prog.max_table * 64 * 8 * 2 <= fbn::kCuLdsBytes) ? 0 : 1;
    return FBN_OK;
}

// check: range-check the evidence first; vm: d_marginals is variable-major [SD][ncases]
static int JtRunDevice(fbn_jt_plan *p, const int8_t *d_evidence, int64_t ncases, int32_t *d_labels,
                       double *d_marginals, hipStream_t s, bool check, bool vm) {
    int rc;
    if (check && (rc = p->evidence.Run(d_evidence, ncases, s))) return rc;
    const int SD = p->interp.prog.sum_dom;
    JtRun r;
    r.evid = d_evidence, r.ncases = ncases, r.nblk = (ncases + 63) / 64, r.s = s;
    r.marg = d_marginals, r.labels = d_labels;
    if (!r.marg) {
        if ((rc = p->marg.ensure((size_t)ncases * SD * 8))) return rc;
        r.marg = p->marg.as<double>();
    }
    if (!r.labels) {
        if ((rc = p->labels.ensure((size_t)ncases * 4))) return rc;
        r.labels = p->labels.as<int32_t>();
    }
    // the specialized kernel stores variable-major columns with 32-bit byte offsets
    const bool vm3 = vm && (int64_t)ncases * SD * 8 < INT32_MAX;
    if ((rc = JtChooseVariant(p, vm3, &r.variant))) return rc;
    p->last_variant = r.variant;
    // variable-major output: kernels 0-3 store it directly; 4 and 5 write case-major scratch that is
    // transposed into the caller's buffer at the end (same values)
    double *const marg_out = r.marg;
    // (the specialized kernel addresses columns with 32-bit byte offsets: larger batches transpose too)
    const bool vm_scratch = vm && (r.variant == 4 || r.variant == 5 || (r.variant == 3 && !vm3));
    if (vm_scratch) {
        if ((rc = p->mtmp.ensure((size_t)ncases * SD * 8))) return rc;
        r.marg = p->mtmp.as<double>();
    }
    r.vm = vm && !vm_scratch;
    p->last_nblk = r.variant >= 3 ? r.nblk : 0;
    // (each variant records ev0 itself: after its allocations, and where its first timed work is enqueued)
    switch (r.variant) {
        case 1: rc = RunInterp(p, r); break;
        case 3: rc = RunSpecialized(p, r); break;
        case 4: rc = RunStreamed(p, r); break;
        case 5: rc = RunTiled(p, r); break;
        default: rc = RunLds(p, r);
    }
    if (rc) return rc;
    if (vm_scratch) {
        hipError_t e = fbn_jt_marg_transpose(r.marg, marg_out, ncases, SD, s);
        if (e != hipSuccess) return SetError(FBN_ERR_HIP, "jt marginal transpose: %s", hipGetErrorString(e));
    }
    return p->End(s);
}

// the public entries' common opening: a device plan, its device current, the caller's stream noted
static int JtOpen(fbn_jt_plan *p, hipStream_t s) {
    if (p->device < 0) return SetError(FBN_ERR_NODEV, "host-only plan (created with device < 0)");
    FBN_HIP(hipSetDevice(p->device));
    p->Note(s);
    return FBN_OK;
}

int fbn_jt_evidence_validate(fbn_jt_plan *p, const int8_t *d_evidence, int64_t ncases, void *hip_stream) {
    if (!p || (!d_evidence && ncases > 0) || ncases < 0) return SetError(FBN_ERR_ARG, "bad argument");
    if (ncases == 0) return FBN_OK;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (int rc = JtOpen(p, s)) return rc;
    return p->evidence.Run(d_evidence, ncases, s);
}

int fbn_jt_set_kernel_timing(fbn_jt_plan *p, int enable) {
    if (!p) return SetError(FBN_ERR_ARG, "null pointer");
    p->timing = enable != 0;
    return FBN_OK;
}

int fbn_jt_set_evidence_check(fbn_jt_plan *p, int enable) {
    if (!p) return SetError(FBN_ERR_ARG, "null pointer");
    p->ev_check = enable != 0;
    return FBN_OK;
}

int fbn_jt_run_device(fbn_jt_plan *p, const int8_t *d_evidence, int64_t ncases, int32_t *d_labels,
                      double *d_marginals, void *hip_stream) {
    if (!p || (!d_evidence && ncases > 0) || ncases < 0) return SetError(FBN_ERR_ARG, "bad argument");
    if (ncases == 0) return FBN_OK;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (int rc = JtOpen(p, s)) return rc;
    return JtRunDevice(p, d_evidence, ncases, d_labels, d_marginals, s, p->ev_check, p->out_layout == 1 && d_marginals);
}

int fbn_jt_run(fbn_jt_plan *p, const int8_t *evidence, int64_t ncases, int32_t *labels_out, double *marginals_out,
               void *hip_stream) {
    if (!p || (!evidence && ncases > 0) || ncases < 0 || (!labels_out && ncases > 0))
        return SetError(FBN_ERR_ARG, "bad argument");
    if (ncases == 0) return FBN_OK;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    int rc;
    // (the stream is noted before anything is queued on it: an error return below leaves work that destroy drains)
    if ((rc = JtOpen(p, s))) return rc;
    const int V = p->host.num_nodes, SD = p->interp.prog.sum_dom;
    if ((rc = p->evid.ensure((size_t)ncases * V))) return rc;
    if ((rc = p->labels.ensure((size_t)ncases * 4))) return rc;
    if ((rc = p->marg.ensure((size_t)ncases * SD * 8))) return rc;
    FBN_HIP(hipMemcpyAsync(p->evid.p, evidence, (size_t)ncases * V, hipMemcpyHostToDevice, s));
    rc = JtRunDevice(p, p->evid.as<int8_t>(), ncases, p->labels.as<int32_t>(), p->marg.as<double>(), s, true, false);
    if (rc) return rc;
    FBN_HIP(hipMemcpyAsync(labels_out, p->labels.p, (size_t)ncases * 4, hipMemcpyDeviceToHost, s));
    if (marginals_out)
        FBN_HIP(hipMemcpyAsync(marginals_out, p->marg.p, (size_t)ncases * SD * 8, hipMemcpyDeviceToHost, s));
    FBN_HIP(hipStreamSynchronize(s));
    return FBN_OK;
}

int fbn_jt_score(const fbn_jt_plan *p, const double *marginals, const double *golden, int64_t ncases, double *mse_sum,
                 double *hd_sum) {
    if (!p || !marginals || !golden || !mse_sum || !hd_sum) return SetError(FBN_ERR_ARG, "null pointer");
    return fbn::ScoreMarginals(p->host.dom, marginals, golden, ncases, mse_sum, hd_sum);  // sample_host.cpp
}

int fbn_jt_set_output_layout(fbn_jt_plan *p, int layout) {
    if (!p || layout < 0 || layout > 1)
        return SetError(FBN_ERR_ARG, "layout must be 0 (case-major) or 1 (variable-major)");
    p->out_layout = layout;
    return FBN_OK;
}

int fbn_jt_score_terms_device(fbn_jt_plan *p, const double *d_marginals, const double *d_golden, int64_t ncases,
                              double *d_terms, void *hip_stream) {
    if (!p || ncases < 0 || (ncases > 0 && (!d_marginals || !d_golden || !d_terms)))
        return SetError(FBN_ERR_ARG, "bad argument");
    if (ncases == 0) return FBN_OK;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (int rc = JtOpen(p, s)) return rc;
    hipError_t e = fbn_jt_score_terms(d_marginals, d_golden, ncases, p->interp.prog.sum_dom, p->out_layout == 1 ? 1 : 0,
                                      p->evidence.dom.as<int32_t>(), p->host.num_nodes, d_terms, s);
    if (e != hipSuccess) return SetError(FBN_ERR_HIP, "jt score terms: %s", hipGetErrorString(e));
    return FBN_OK;
}

int fbn_jt_last_kernel_ms(const fbn_jt_plan *p, float *ms) {
    if (!p) return SetError(FBN_ERR_ARG, "no timed launch");
    return p->LastKernelMs(ms);
}

int fbn_jt_plan_destroy(fbn_jt_plan *p) { return fbn::DestroyHandle(p); }

}  // extern "C"
