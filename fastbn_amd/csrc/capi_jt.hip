// capi_jt.hip -- the junction-tree entries of include/fastbn.h: plan creation and upload, kernel
// variant choice and launch, evidence check, scoring.
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

extern "C" {

// ------------------------------------------------------------------ junction tree
static int JtUpload(fbn_jt_plan *p) {
    auto up = [](DevBuf &b, const void *src, size_t bytes) -> int {
        int rc = b.ensure(std::max<size_t>(bytes, 8));
        if (rc) return rc;
        if (bytes) FBN_HIP(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
        return FBN_OK;
    };
    const auto &g = p->prog;
    int rc;
    if ((rc = up(p->ops, g.ops.data(), g.ops.size() * sizeof(JtOp)))) return rc;
    if ((rc = up(p->aux, g.aux.data(), g.aux.size() * 4))) return rc;
    if ((rc = up(p->initv, g.initv.data(), g.initv.size() * 8))) return rc;
    if ((rc = up(p->dig, g.dig.data(), g.dig.size() * 8))) return rc;
    const auto &l = p->lprog;
    if ((rc = up(p->lops, l.ops.data(), l.ops.size() * sizeof(JtOp)))) return rc;
    if ((rc = up(p->laux, l.aux.data(), l.aux.size() * 4))) return rc;
    if ((rc = up(p->linitv, l.initv.data(), l.initv.size() * 8))) return rc;
    if ((rc = up(p->ldig, l.dig.data(), l.dig.size() * 8))) return rc;
    if (p->v_ok) {
        const auto &v = p->vprog;
        if ((rc = up(p->vcl, v.cl.data(), v.cl.size() * sizeof(JtVClique)))) return rc;
        if ((rc = up(p->vaux, v.aux.data(), v.aux.size() * 4))) return rc;
        if ((rc = up(p->viv, v.initv.data(), v.initv.size() * 8))) return rc;
        if ((rc = up(p->vdig, v.dig.data(), v.dig.size() * 8))) return rc;
        if ((rc = up(p->vorder, v.order.data(), v.order.size() * 4))) return rc;
        if ((rc = up(p->vsched, v.sched.data(), v.sched.size() * 4))) return rc;
        if ((rc = up(p->vsel, v.vsel.data(), v.vsel.size() * 4))) return rc;
    }
    if (p->t_ok) {
        const auto &t = p->tprog;
        if ((rc = up(p->tpass, t.passes.data(), t.passes.size() * sizeof(JtTPass)))) return rc;
        if ((rc = up(p->ttab, t.tab.data(), t.tab.size() * 4))) return rc;
        if ((rc = up(p->tiv, t.initv.data(), t.initv.size() * 8))) return rc;
    }
    return FBN_OK;
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
    rc = fbn::CompileJTProgram(p->host, p->prog);
    if (rc) return rc;
    rc = fbn::CompileJTProgramLDS(p->host, p->lprog);
    if (rc) return rc;
    lap("interpreter programs");
    rc = fbn::CompileJTProgramV(p->host, p->vprog);
    if (rc && rc != FBN_ERR_LIMIT) return rc;
    p->v_ok = rc == FBN_OK;
    if (!p->v_ok) p->vprog = fbn::JTProgramV();
    lap("streamed program");
    // tiled variant: factors of a clique phase staged in LDS up to this many bytes per wave
    // LDS factor budget per workgroup: 6016 B + the bin and total rows = 10 KB, so 16 one-wave
    // workgroups fit a CU's 160 KB
    constexpr int kTileLdsBytes = 6016;
    rc = fbn::CompileJTProgramT(p->host, p->tprog, kTileLdsBytes);
    if (rc && rc != FBN_ERR_LIMIT) return rc;
    p->t_ok = rc == FBN_OK;
    if (!p->t_ok) p->tprog = fbn::JTProgramT();
    lap("tiled program");
    p->gen_eligible = fbn::JTCodegenEligible(p->host, nullptr);
    p->device = device;
    if (device >= 0) {  // device < 0: host-only plan (info / dump), runs fail with FBN_ERR_NODEV
        rc = fbn::CheckDevice(device, &p->num_cu);
        if (rc) return rc;
        rc = JtUpload(p.get());
        if (rc) return rc;
        FBN_HIP(hipEventCreate(&p->ev0));
        FBN_HIP(hipEventCreate(&p->ev1));
    }
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
    info->sum_dom = p->prog.sum_dom;
    for (auto &t : p->host.cliques) info->clique_entries += t.size();
    for (auto &t : p->host.seps) info->separator_entries += t.size();
    info->algorithmic_bytes_per_case =
        16 * (info->clique_entries + info->separator_entries) + 8 * (int64_t)info->sum_dom + info->num_nodes;
    info->num_ops = (int32_t)p->prog.ops.size();
    info->max_vars_per_table = p->prog.max_vars;
    info->specialized_eligible = p->gen_eligible ? 1 : 0;
    info->variant = p->variant >= 0 ? p->variant : p->last_variant;
    info->streamed_eligible = p->v_ok ? 1 : 0;
    info->streamed_waves = JT_V_WAVES;
    info->streamed_split_efficiency = p->v_ok ? p->vprog.split_efficiency : 0.0;
    info->tiled_eligible = p->t_ok ? 1 : 0;
    info->tiled_passes = (int32_t)p->tprog.passes.size();
    info->tiled_entry_visits = p->tprog.entry_visits;
    info->tiled_lds_bytes = p->tprog.lds_bytes;
    info->tiled_table_bytes = (int64_t)p->tprog.tab.size() * 4;
    return FBN_OK;
}

int fbn_jt_stream_schedule(const fbn_jt_plan *p, int32_t *order, int64_t order_cap, int32_t *sched,
                           int64_t sched_cap, int64_t *n_order, int64_t *n_sched) {
    if (!p) return SetError(FBN_ERR_ARG, "null pointer");
    if (!p->v_ok) return SetError(FBN_ERR_LIMIT, "plan not eligible for the streamed kernel");
    const auto &v = p->vprog;
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
    if (!p->t_ok) return SetError(FBN_ERR_LIMIT, "plan not eligible for the tiled kernel");
    static_assert(sizeof(JtTPass) == 33 * 4, "JtTPass = 33 int32");
    const auto &t = p->tprog;
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
    if (variant == 3 && !p->gen_eligible) return SetError(FBN_ERR_ARG, "plan not eligible for the specialized kernel");
    if (variant == 4 && !p->v_ok) return SetError(FBN_ERR_ARG, "plan not eligible for the streamed kernel");
    if (variant == 5 && !p->t_ok) return SetError(FBN_ERR_ARG, "plan not eligible for the tiled kernel");
    p->variant = variant;
    return FBN_OK;
}

// the plan-specialized kernel of the current arithmetic order, loaded (cache) or compiled (hiprtc)
// once per plan and order; both orders stay loaded
static fbn_jt_plan::GenKernel &GenCur(fbn_jt_plan *p, bool vm) { return p->gen[(JtFast(p) ? 1 : 0) + (vm ? 2 : 0)]; }
// source, constant input and launch facts of the specialized kernel of the plan's current order
static int GenSpec(const fbn_jt_plan *p, bool vm, fbn::JTKernelSpec &spec) {
    if (!p->gen_eligible) return SetError(FBN_ERR_ARG, "plan not eligible for codegen");
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
    const std::vector<double> &iv = spec.initv;
    std::vector<char> code;
    if ((rc = fbn::JitCodeObject(spec.src, code))) return rc;
    FBN_HIP(hipModuleLoadData(&k.mod, code.data()));
    FBN_HIP(hipModuleGetFunction(&k.fn, k.mod, "fbn_jt_gen"));
    if ((rc = k.iv.ensure(std::max<size_t>(iv.size() * 8, 8)))) return rc;
    FBN_HIP(hipMemcpy(k.iv.p, iv.data(), iv.size() * 8, hipMemcpyHostToDevice));  // (a new buffer: no run uses it yet)
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

static const size_t kLdsBytes = 160 * 1024;

// LDS variant geometry: waves per CU and the number of LDS table rows (64 lanes x 8 B each)
static void LdsGeometry(const fbn_jt_plan *p, int *waves, int *cap) {
    const int64_t row = 64 * 8, tmax = std::max<int64_t>(1, p->lprog.max_table);
    int w = p->waves_per_cu;
    if (w <= 0) w = (int)std::max<int64_t>(1, std::min<int64_t>(8, (int64_t)kLdsBytes / (tmax * row)));
    int64_t c = std::min<int64_t>(tmax, (int64_t)(kLdsBytes / w) / row);
    *waves = w;
    *cap = (int)std::max<int64_t>(1, c);
}

// LDS interpreter launch (variants 0/2, and the exact fixup of variant 3 when flags != NULL)
static int LaunchLds(fbn_jt_plan *p, DevBuf &ws, const int8_t *d_evidence, int64_t ncases, int32_t *labels,
                     double *marg, const int *flags, bool force_exact, hipStream_t s, bool vm = false) {
    const auto &l = p->lprog;
    const int V = p->host.num_nodes, SD = l.sum_dom, nc = l.num_cliques;
    const int64_t nblk = (ncases + 63) / 64;
    int wpc, cap, rc;
    LdsGeometry(p, &wpc, &cap);
    const bool spill = cap < l.max_table;
    // fixup mode: flagged blocks are rare; one wave per CU scans the flags 64 at a time (the launch
    // follows every specialized / tiled launch: ~3 us per call on ALARM, grids of 4 / 16 / 256 waves
    // measured alike)
    int grid = (int)std::min<int64_t>(nblk, flags ? (int64_t)p->num_cu : (int64_t)p->num_cu * wpc);
    const int64_t store_off = 0, den_off = l.store_entries, sep_off = den_off + nc, spill_off = sep_off + l.sep_entries;
    const int64_t wave_entries = spill_off + (spill ? l.max_table - cap : 0);
    if (flags)  // fixup mode: at most ~2 GiB of workspace (large trees need ~100 MB per wave)
        grid = (int)std::max<int64_t>(1, std::min<int64_t>(grid, ((int64_t)2 << 30) / (wave_entries * 64 * 8 + nc * 64 * 4)));
    const size_t ws_d = (size_t)grid * wave_entries * 64 * 8;
    const size_t ws_i = (size_t)grid * nc * 64 * 4;
    if ((rc = ws.ensure(ws_d + ws_i))) return rc;
    const bool prof = p->prof_on && !flags;
    if (prof) {
        if ((rc = p->prof.ensure((size_t)grid * 16 * 8))) return rc;
        FBN_HIP(hipMemsetAsync(p->prof.p, 0, (size_t)grid * 16 * 8, s));
        p->last_grid = grid;
    }
    JtLdsArgs a{};
    a.par.ncases = ncases, a.par.wave_entries = wave_entries;
    a.par.store_off = store_off, a.par.den_off = den_off, a.par.sep_off = sep_off, a.par.spill_off = spill_off;
    a.par.nops = (int)l.ops.size(), a.par.V = V, a.par.SD = SD, a.par.nc = nc, a.par.cap = cap;
    a.par.force_exact = force_exact, a.par.vmajor = vm ? 1 : 0;
    a.par.flags = flags;
    a.ops = p->lops.as<JtOp>(), a.aux = p->laux.as<int32_t>();
    a.initv = p->linitv.as<double>(), a.dig = p->ldig.as<uint64_t>();
    a.evid = d_evidence, a.marg = marg, a.labels = labels;
    a.ws = ws.as<double>(), a.wsi = reinterpret_cast<int32_t *>(ws.as<char>() + ws_d);
    a.spill = spill, a.grid = grid;
    a.prof = prof ? p->prof.as<unsigned long long>() : nullptr;
    hipError_t e = fbn_jt_lds_launch(&a, s);
    if (e != hipSuccess) return SetError(FBN_ERR_HIP, "jt kernel launch: %s", hipGetErrorString(e));
    return FBN_OK;
}

// the evidence range check (fbn_device.h) against the plan's domains, uploaded at its first use
static int JtCheckEvidence(fbn_jt_plan *p, const int8_t *d_ev, int64_t ncases, hipStream_t s) {
    const int V = p->host.num_nodes;
    int rc;
    if (!p->ddom.p) {
        if ((rc = p->ddom.ensure((size_t)V * 4))) return rc;
        if ((rc = p->evcheck.ensure(8))) return rc;
        FBN_HIP(hipMemcpy(p->ddom.p, p->host.dom.data(), (size_t)V * 4, hipMemcpyHostToDevice));
    }
    return fbn::EvidenceCheckDevice(d_ev, ncases, V, p->ddom.as<int32_t>(), p->host.dom.data(),
                                    p->evcheck.as<unsigned long long>(), s);
}

int fbn_jt_evidence_validate(fbn_jt_plan *p, const int8_t *d_evidence, int64_t ncases, void *hip_stream) {
    if (!p || (!d_evidence && ncases > 0) || ncases < 0) return SetError(FBN_ERR_ARG, "bad argument");
    if (ncases == 0) return FBN_OK;
    if (p->device < 0) return SetError(FBN_ERR_NODEV, "host-only plan (created with device < 0)");
    FBN_HIP(hipSetDevice(p->device));
    p->note_stream(static_cast<hipStream_t>(hip_stream));
    return JtCheckEvidence(p, d_evidence, ncases, static_cast<hipStream_t>(hip_stream));
}

int fbn_jt_set_kernel_timing(fbn_jt_plan *p, int enable) {
    if (!p) return SetError(FBN_ERR_ARG, "null pointer");
    p->ktiming = enable != 0;
    return FBN_OK;
}

int fbn_jt_set_evidence_check(fbn_jt_plan *p, int enable) {
    if (!p) return SetError(FBN_ERR_ARG, "null pointer");
    p->ev_check = enable != 0;
    return FBN_OK;
}

static int JtRunDevice(fbn_jt_plan *p, const int8_t *d_evidence, int64_t ncases, int32_t *d_labels,
                       double *d_marginals, hipStream_t s, bool check, bool vm);

int fbn_jt_run_device(fbn_jt_plan *p, const int8_t *d_evidence, int64_t ncases, int32_t *d_labels,
                      double *d_marginals, void *hip_stream) {
    if (!p || (!d_evidence && ncases > 0) || ncases < 0) return SetError(FBN_ERR_ARG, "bad argument");
    if (ncases == 0) return FBN_OK;
    if (p->device < 0) return SetError(FBN_ERR_NODEV, "host-only plan (created with device < 0)");
    FBN_HIP(hipSetDevice(p->device));
    p->note_stream(static_cast<hipStream_t>(hip_stream));
    return JtRunDevice(p, d_evidence, ncases, d_labels, d_marginals, static_cast<hipStream_t>(hip_stream),
                       p->ev_check, p->out_layout == 1 && d_marginals);
}

static int JtRunDevice(fbn_jt_plan *p, const int8_t *d_evidence, int64_t ncases, int32_t *d_labels,
                       double *d_marginals, hipStream_t s, bool check, bool vm) {
    if (check)
        if (int rc = JtCheckEvidence(p, d_evidence, ncases, s)) return rc;
    const auto &g = p->prog;
    const int V = p->host.num_nodes, SD = g.sum_dom, nc = g.num_cliques;
    const int64_t nblk = (ncases + 63) / 64;
    int rc;
    double *marg = d_marginals;
    if (!marg) {
        if ((rc = p->marg.ensure((size_t)ncases * SD * 8))) return rc;
        marg = p->marg.as<double>();
    }
    int32_t *labels = d_labels;
    if (!labels) {
        if ((rc = p->labels.ensure((size_t)ncases * 4))) return rc;
        labels = p->labels.as<int32_t>();
    }
    int variant = p->variant;
    // the specialized kernel stores variable-major columns with 32-bit byte offsets
    const bool vm3 = vm && (int64_t)ncases * SD * 8 < INT32_MAX;
    if (variant == -1) {
        // specialized kernel when eligible; else the streamed kernel (1.5-2x the interpreters on
        // ALARM and the Munin-like network); the interpreters only for plans it cannot take
        if (p->gen_eligible && GenEnsure(p, vm3) == FBN_OK) variant = 3;
        else if (p->t_ok && JtFast(p)) variant = 5;  // (fast arithmetic order only)
        else if (p->v_ok) variant = 4;
        else variant = (p->lprog.max_table * 64 * 8 * 2 <= (int64_t)kLdsBytes) ? 0 : 1;
    }
    else if (variant == 3 && (rc = GenEnsure(p, vm3))) return rc;
    p->last_variant = variant;
    // variable-major output: kernels 0-3 store it directly; 4 and 5 write case-major scratch that is
    // transposed into the caller's buffer at the end (same values)
    double *const marg_out = marg;
    // (the specialized kernel addresses columns with 32-bit byte offsets: larger batches transpose too)
    const bool vm_scratch = vm && (variant == 4 || variant == 5 || (variant == 3 && !vm3));
    if (vm_scratch) {
        if ((rc = p->mtmp.ensure((size_t)ncases * SD * 8))) return rc;
        marg = p->mtmp.as<double>();
    }
    const bool vm_direct = vm && !vm_scratch;
    p->last_nblk = variant >= 3 ? nblk : 0;

    if (variant == 1) {
        const int wpc = p->waves_per_cu > 0 ? p->waves_per_cu : 8;
        int grid = (int)std::min<int64_t>(nblk, (int64_t)p->num_cu * wpc);
        // persistent waves: cap the per-wave workspaces at 80 % of the free HBM (more resident waves
        // = more memory-level parallelism: this variant is latency bound on large plans)
        const size_t per_wave = (size_t)g.state_entries * 64 * 8 + (size_t)nc * 64 * 4;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && per_wave > 0) {
            const size_t have = free_b / 10 * 8 + (p->ws.bytes);
            grid = (int)std::max<int64_t>(1, std::min<int64_t>(grid, (int64_t)(have / per_wave)));
        }
        const size_t ws_d = (size_t)grid * g.state_entries * 64 * 8;
        const size_t ws_i = (size_t)grid * nc * 64 * 4;
        if ((rc = p->ws.ensure(ws_d + ws_i))) return rc;
        if (p->ktiming) FBN_HIP(hipEventRecord(p->ev0, s));
        JtArgs a{};
        a.ops = p->ops.as<JtOp>(), a.aux = p->aux.as<int32_t>();
        a.initv = p->initv.as<double>(), a.dig = p->dig.as<uint64_t>();
        a.evid = d_evidence, a.marg = marg, a.labels = labels;
        a.ws = p->ws.as<double>(), a.wsi = reinterpret_cast<int32_t *>(p->ws.as<char>() + ws_d);
        a.ncases = ncases, a.NE = g.state_entries;
        a.nops = (int)g.ops.size(), a.V = V, a.SD = SD, a.nc = nc;
        a.vmajor = vm_direct ? 1 : 0;
        hipError_t e = fbn_jt_launch(&a, grid, s);
        if (e != hipSuccess) return SetError(FBN_ERR_HIP, "jt kernel launch: %s", hipGetErrorString(e));
    } else if (variant == 4) {
        // streamed tables: small register footprint, many resident waves; the per-wave store holds
        // only separator messages and denominators
        // workgroups of JT_V_WAVES waves, one 64-case block per workgroup (persistent)
        const int W = JT_V_WAVES;
        const int wpc = p->waves_per_cu > 0 ? p->waves_per_cu : 16;
        int grid = (int)std::min<int64_t>(nblk, std::max<int64_t>(1, (int64_t)p->num_cu * wpc / W));
        const auto &v = p->vprog;
        const size_t per_blk_d = (size_t)v.store_rows * 64 * 8, per_blk_i = (size_t)(nc + V) * 64 * 4;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const size_t have = free_b / 10 * 8 + p->ws.bytes;
            grid = (int)std::max<int64_t>(1, std::min<int64_t>(grid, (int64_t)(have / (per_blk_d + per_blk_i))));
        }
        const size_t ws_d = (size_t)grid * per_blk_d;
        if ((rc = p->ws.ensure(ws_d + (size_t)grid * per_blk_i))) return rc;
        if ((rc = p->flags.ensure((size_t)nblk * 4))) return rc;
        if (p->ktiming) FBN_HIP(hipEventRecord(p->ev0, s));
        const char *vdebug_env = fbn::KnobValue("FBN_JT_VDEBUG");
        const int vdebug = vdebug_env ? atoi(vdebug_env) : 0;
        hipError_t e = fbn_jt_virt_launch(p->vcl.as<JtVClique>(), p->vaux.as<int32_t>(), p->viv.as<double>(),
                                          p->vdig.as<uint64_t>(), p->vorder.as<int32_t>(), p->vsched.as<int32_t>(),
                                          p->vsel.as<int32_t>(), d_evidence, marg, labels, p->ws.as<double>(),
                                          reinterpret_cast<int32_t *>(p->ws.as<char>() + ws_d), p->flags.as<int>(),
                                          ncases, v.store_rows, v.scratch_row, v.scratch_rows, nc, V, SD, grid,
                                          // diagnostic ablation only (tools/): skip pass types, wrong results
                                          vdebug | (JtFast(p) ? kJtVFast : 0),
                                          s);
        if (e != hipSuccess) return SetError(FBN_ERR_HIP, "jt kernel launch: %s", hipGetErrorString(e));
        if (p->force_fixup) FBN_HIP(hipMemsetAsync(p->flags.p, 1, (size_t)nblk * 4, s));  // testing only
        // exact recomputation of the blocks whose denominators left the fast-division range
        if (!vdebug_env &&
            (rc = LaunchLds(p, p->ws_fix, d_evidence, ncases, labels, marg, p->flags.as<int>(), false, s)))
            return rc;
    } else if (variant == 5) {
        const auto &t = p->tprog;
        // workgroups of JT_T_W waves, one case group (JT_T_C cases) each, persistent; per workgroup
        // its message store
        const int64_t ncg = (ncases + JT_T_C - 1) / JT_T_C;
        const int wpc = p->waves_per_cu > 0 ? p->waves_per_cu : 16;
        int grid = (int)std::min<int64_t>(ncg, std::max<int64_t>(1, (int64_t)p->num_cu * wpc / t.waves));
        const size_t per_wg = (size_t)t.store_rows * JT_T_C * 8;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const size_t have = free_b / 10 * 8 + p->ws.bytes;
            grid = (int)std::max<int64_t>(1, std::min<int64_t>(grid, (int64_t)(have / per_wg)));
        }
        if ((rc = p->ws.ensure((size_t)grid * per_wg))) return rc;
        if ((rc = p->flags.ensure((size_t)nblk * 4))) return rc;
        FBN_HIP(hipMemsetAsync(p->flags.p, 0, (size_t)nblk * 4, s));
        unsigned long long *tprof = nullptr;  // diagnostic: per-phase cycles (fbn_jt_debug_op_cycles)
        if (p->prof_on) {
            if ((rc = p->prof.ensure(16 * 8))) return rc;
            FBN_HIP(hipMemsetAsync(p->prof.p, 0, 16 * 8, s));
            p->last_grid = 1;
            tprof = p->prof.as<unsigned long long>();
        }
        if (p->ktiming) FBN_HIP(hipEventRecord(p->ev0, s));
        hipError_t e = fbn_jt_tile_launch(p->tpass.as<JtTPass>(), (int)t.passes.size(), p->ttab.as<int32_t>(),
                                          p->tiv.as<double>(), d_evidence, marg, labels, p->ws.as<double>(),
                                          p->flags.as<int>(), ncases, t.store_rows, t.scr_row, t.red_row, V, SD,
                                          (int)t.lds_bytes, grid, t.waves, tprof, s);
        if (e != hipSuccess) return SetError(FBN_ERR_HIP, "jt kernel launch: %s", hipGetErrorString(e));
        if (p->force_fixup) FBN_HIP(hipMemsetAsync(p->flags.p, 1, (size_t)nblk * 4, s));  // testing only
        // exact recomputation of the blocks holding a case group whose pass totals left the checked range
        if ((rc = LaunchLds(p, p->ws_fix, d_evidence, ncases, labels, marg, p->flags.as<int>(), false, s)))
            return rc;
    } else if (variant == 3) {
        // one wave (64 cases) per SIMD: the clique in flight occupies the register file (+ LDS tail)
        const auto &gk = GenCur(p, vm3);
        int wpc = p->waves_per_cu > 0 ? p->waves_per_cu : 4;
        if (gk.lds > 0) wpc = std::max<int>(1, std::min<int64_t>(wpc, (int64_t)kLdsBytes / gk.lds));
        const int grid = (int)std::min<int64_t>(nblk, (int64_t)p->num_cu * wpc);
        if ((rc = p->ws.ensure((size_t)grid * gk.we * 64 * 8))) return rc;
        if ((rc = p->flags.ensure((size_t)nblk * 4))) return rc;
        if (p->ktiming) FBN_HIP(hipEventRecord(p->ev0, s));

        const int8_t *a_ev = d_evidence;
        double *a_marg = marg, *a_ws = p->ws.as<double>();
        int32_t *a_lab = labels;
        int *a_flags = p->flags.as<int>();
        const double *a_iv = gk.iv.as<double>();
        long long a_n = ncases;
        unsigned long long *a_prof = nullptr;
        if (p->prof_on) {  // diagnostic: only kernels generated with FBN_JT_PROFILE=1 write it
            if ((rc = p->prof.ensure((size_t)grid * 16 * 8))) return rc;
            FBN_HIP(hipMemsetAsync(p->prof.p, 0, (size_t)grid * 16 * 8, s));
            p->last_grid = grid;
            a_prof = p->prof.as<unsigned long long>();
        }
        void *args[] = {&a_ev, &a_marg, &a_lab, &a_ws, &a_flags, &a_iv, &a_n, &a_prof};
        FBN_HIP(hipModuleLaunchKernel(gk.fn, grid, 1, 1, 64, 1, 1, (unsigned)gk.lds, s, args, nullptr));
        if (p->force_fixup) FBN_HIP(hipMemsetAsync(p->flags.p, 1, (size_t)nblk * 4, s));  // testing only
        // exact recomputation of the blocks whose denominators left the fast-division range
        if ((rc = LaunchLds(p, p->ws_fix, d_evidence, ncases, labels, marg, p->flags.as<int>(), false, s, vm_direct)))
            return rc;
    } else {
        if (p->ktiming) FBN_HIP(hipEventRecord(p->ev0, s));
        if ((rc = LaunchLds(p, p->ws, d_evidence, ncases, labels, marg, nullptr, variant == 2, s, vm_direct))) return rc;
    }
    if (vm_scratch) {
        hipError_t e = fbn_jt_marg_transpose(marg, marg_out, ncases, SD, s);
        if (e != hipSuccess) return SetError(FBN_ERR_HIP, "jt marginal transpose: %s", hipGetErrorString(e));
    }
    if (p->ktiming) FBN_HIP(hipEventRecord(p->ev1, s));
    p->timed = p->ktiming;
    return FBN_OK;
}

int fbn_jt_run(fbn_jt_plan *p, const int8_t *evidence, int64_t ncases, int32_t *labels_out, double *marginals_out,
               void *hip_stream) {
    if (!p || (!evidence && ncases > 0) || ncases < 0 || (!labels_out && ncases > 0))
        return SetError(FBN_ERR_ARG, "bad argument");
    if (ncases == 0) return FBN_OK;
    if (p->device < 0) return SetError(FBN_ERR_NODEV, "host-only plan (created with device < 0)");
    const int V = p->host.num_nodes, SD = p->prog.sum_dom;
    FBN_HIP(hipSetDevice(p->device));
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    int rc;
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
    if (p->device < 0) return SetError(FBN_ERR_NODEV, "host-only plan (created with device < 0)");
    FBN_HIP(hipSetDevice(p->device));
    const int V = p->host.num_nodes;
    int rc;
    if (!p->ddom.p) {
        if ((rc = p->ddom.ensure((size_t)V * 4))) return rc;
        if ((rc = p->evcheck.ensure(8))) return rc;
        FBN_HIP(hipMemcpy(p->ddom.p, p->host.dom.data(), (size_t)V * 4, hipMemcpyHostToDevice));
    }
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    p->note_stream(s);
    hipError_t e = fbn_jt_score_terms(d_marginals, d_golden, ncases, p->prog.sum_dom, p->out_layout == 1 ? 1 : 0,
                                      p->ddom.as<int32_t>(), V, d_terms, s);
    if (e != hipSuccess) return SetError(FBN_ERR_HIP, "jt score terms: %s", hipGetErrorString(e));
    return FBN_OK;
}

int fbn_jt_last_kernel_ms(const fbn_jt_plan *p, float *ms) {
    if (!p || !ms || !p->timed) return SetError(FBN_ERR_ARG, "no timed launch");
    FBN_HIP(hipEventSynchronize(p->ev1));
    FBN_HIP(hipEventElapsedTime(ms, p->ev0, p->ev1));
    return FBN_OK;
}

int fbn_jt_plan_destroy(fbn_jt_plan *p) {
    if (!p) return FBN_OK;
    if (p->device >= 0) {  // runs are queued on caller streams: drain those before the buffers go
        (void)hipSetDevice(p->device);
        for (hipStream_t s : p->streams_used) (void)hipStreamSynchronize(s);
    }
    delete p;
    return FBN_OK;
}

}  // extern "C"
