// gci_ctx.h -- the Gaussian context (fbn_gci_ctx) for the files that queue work on it: capi_gci.hip, which
// creates it and keeps R resident, and capi_gscore.hip, the family scorer over that R.  Internal to libfastbn.
#ifndef FBN_GCI_CTX_H
#define FBN_GCI_CTX_H

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "fbn_device.h"

using fbn::DevBuf;

struct fbn_gci_ctx {
    int device = 0, num_cu = 0, nvars = 0;
    int64_t N = 0;
    DevBuf X, mean, bad, slab, R, var, stats;
    int want_split = 0, want_tile = 0;  // fbn_gci_set_tuning, 0 = automatic
    int split_k = 0, tile = 0;          // what the resident R was computed with
    hipStream_t stream = nullptr;
    hipEvent_t cev[4] = {nullptr, nullptr, nullptr, nullptr};  // around means, Gram, reduce
    float corr_ms[3] = {0.f, 0.f, 0.f};
    float last_ms = 0.f;
    bool timed = false;
    struct Slot {
        DevBuf items, indep, r;
        void *h_items = nullptr, *h_res = nullptr;
        size_t h_items_bytes = 0, h_res_bytes = 0;
        hipEvent_t ev0 = nullptr, ev1 = nullptr, done = nullptr;  // kernel start / end, results in pinned memory
        int64_t n = 0;
        bool want_r = false;
        ~Slot() {
            if (h_items) (void)hipHostFree(h_items);
            if (h_res) (void)hipHostFree(h_res);
            if (ev0) (void)hipEventDestroy(ev0);
            if (ev1) (void)hipEventDestroy(ev1);
            if (done) (void)hipEventDestroy(done);
        }
    } slot[2];
    unsigned long long *h_stats = nullptr;  // pinned: [0..2] the reset value, [3..5] the read-back
    int64_t last_degenerate = 0;
    // the family scorer (capi_gscore.hip): S_vv on the host (GciCompute leaves it), the per-variable tables, the
    // bucketed records and the two outputs on the device, their pinned staging, the degenerate counter
    std::vector<double> h_ss;
    DevBuf gs_lss, gs_tq, gs_rec, gs_out, gs_cnt;
    void *gs_h_rec = nullptr, *gs_h_out = nullptr;
    size_t gs_h_rec_bytes = 0, gs_h_out_bytes = 0;
    int64_t gs_info[3] = {0, 0, 0};  // of the last batch: families, kernel launches, degenerate families
    ~fbn_gci_ctx() {
        if (h_stats) (void)hipHostFree(h_stats);
        if (gs_h_rec) (void)hipHostFree(gs_h_rec);
        if (gs_h_out) (void)hipHostFree(gs_h_out);
        for (auto &e : cev)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

#endif
