// learner_device.h -- what the device entries of the score-based learners (capi_hc.hip, capi_exact.hip,
// capi_bma.hip, capi_omcmc.hip) share around their kernels: a pinned staging block, the timed phase on a CI
// context's stream, and the lattice learners' scaffold (the refusals ahead of the lattices and phase 1, the
// local scores up).  The scorer itself is hc_search.h's HcDeviceScorer.  Internal to libfastbn.
#ifndef FBN_LEARNER_DEVICE_H
#define FBN_LEARNER_DEVICE_H

#include <hip/hip_runtime.h>

#include "capi_state.h"
#include "exact_dp.h"
#include "hc_search.h"

namespace fbn {

// pinned host memory that lives for one run
struct Pinned {
    void *p = nullptr;
    int alloc(size_t bytes) {
        const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
        if (e != hipSuccess) return SetError(FBN_ERR_NOMEM, "hipHostMalloc(%zu): %s", bytes, hipGetErrorString(e));
        return FBN_OK;
    }
    ~Pinned() {
        if (p) (void)hipHostFree(p);
    }
};

// One phase on the context's stream: launches() between the context's two events, then tail() (the copies that
// bring the phase's results back, outside the events), then one synchronise.  Kernel ms (left as it is with
// timing off) and wall ms out.
template <class Launches, class Tail>
int Phase(fbn_ci_ctx *c, double *kernel_ms, double *wall_ms, Launches launches, Tail tail) {
    CiSlot &S = c->slot[0];
    const auto t0 = Clock::now();
    if (c->timing) FBN_HIP(hipEventRecord(S.ev0, c->stream));
    if (int rc = launches()) return rc;
    if (c->timing) FBN_HIP(hipEventRecord(S.ev1, c->stream));
    if (int rc = tail()) return rc;
    FBN_HIP(hipStreamSynchronize(c->stream));
    if (c->timing) {
        float f = 0.f;
        FBN_HIP(hipEventElapsedTime(&f, S.ev0, S.ev1));
        *kernel_ms = f;
    }
    *wall_ms = MsSince(t0);
    return FBN_OK;
}
template <class Launches>
int Phase(fbn_ci_ctx *c, double *kernel_ms, double *wall_ms, Launches launches) {
    return Phase(c, kernel_ms, wall_ms, launches, [] { return (int)FBN_OK; });
}

// The lattice learners' scaffold (capi_exact.hip defines it; capi_bma.hip runs it too).  Three steps, since the
// two learners order them differently around their own allocations: the exact search allocates, uploads and
// then plans; the arc posteriors plan, allocate and then upload.
// 1: FBN_ERR_LIMIT where the state does not fit the free device memory; what = "subset" or "posterior"
int LatticeFits(int n, int64_t state_bytes, const char *what);
// 2: the transform's passes of tile_bits bits over n - 1 for a kernel whose tile holds 2^lds_bits entries;
//    FBN_ERR_LIMIT where one of them needs more workgroups than a launch has.  Returns their number in *passes.
int LatticePasses(int n, int tile_bits, int lds_bits, ExactPass *pass, int32_t *passes);
// 3: phase 1 -- the local scores of one variable at a time (ExactLocalScores, size_prior as there) into pinned
//    memory, then up into d_ls [n][2^(n-1)]; the copies' wall time is added to *upload_wall_ms.  stage is the
//    caller's and allocated here: it is freed when the run returns, after its wall clock has stopped
int LatticeLocalScores(fbn_ci_ctx *c, const fbn_exact_options &opt, const HcScorer &scorer, const double *size_prior, Pinned &stage,
                       double *d_ls, fbn_exact_info *xi, double *upload_wall_ms);

}  // namespace fbn

#endif
