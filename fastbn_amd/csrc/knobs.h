// knobs.h -- every environment variable libfastbn reads: one table, one accessor, and the library's
// only getenv.  None is needed in production: a test seam forces a path the defaults do not take on
// the tests' small inputs, a diagnostic only prints or records.  DESIGN.md lists the same rows.
// Internal to libfastbn (header only, so the host files also build stand-alone).
#ifndef FBN_KNOBS_H
#define FBN_KNOBS_H

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <thread>

namespace fbn {

enum KnobKind { kSeam, kDiagnostic, kLocation };
// kPerCall: read wherever the path is chosen (tests set these inside a running process);
// kOnce: read once per process, at first use; kOutside: read by the CLI or the Python package only
enum KnobRead { kPerCall, kOnce, kOutside };

struct Knob {
    const char *name;
    const char *dflt;  // what holds when the variable is unset
    KnobKind kind;
    KnobRead read;
};

inline constexpr Knob kKnobs[] = {
    // CI tests: counting paths (capi_ci.hip, capi_pc.hip)
    {"FBN_CI_BITSN", "off: levels >= 2 count from byte columns", kSeam, kPerCall},
    {"FBN_CI_FORCE_BITS", "off: bit-sliced columns from 4096 samples", kSeam, kPerCall},
    {"FBN_CI_GRAM4_SPLITS", "CUs / tiles", kSeam, kPerCall},
    {"FBN_CI_GRAM_NO_MFMA", "off: FP4 MFMA Gram where it pays", kSeam, kPerCall},
    {"FBN_CI_NO_BAND", "off: the G^2 decision band is built", kSeam, kPerCall},
    {"FBN_CI_NO_BITS", "off", kSeam, kPerCall},
    {"FBN_CI_NO_DER2", "off", kSeam, kPerCall},
    {"FBN_CI_NO_GRAM", "off", kSeam, kPerCall},
    {"FBN_CI_NO_PACK2", "off", kSeam, kPerCall},
    {"FBN_CI_NO_PAIRS", "off", kSeam, kPerCall},
    {"FBN_CI_NO_ZEROCOPY", "off", kSeam, kPerCall},
    {"FBN_CI_PACK2", "off: packed columns from 65536 samples", kSeam, kPerCall},
    // JT: plan and code generation (jt_codegen.cpp, jt_tile_plan.cpp), read when a plan is built
    {"FBN_JT_LDS_POOL", "the LDS left beside the kernel's own", kSeam, kPerCall},
    {"FBN_JT_LEAF_RC", "0", kSeam, kPerCall},
    {"FBN_JT_MARG_V2", "1", kSeam, kPerCall},
    {"FBN_JT_REG_POOL", "the registers left under the budget", kSeam, kPerCall},
    {"FBN_JT_SCHED", "1: the potentials' load pipeline and level-wise products (read only with the register pool on)", kSeam, kPerCall},
    {"FBN_JT_TILING", "0", kSeam, kPerCall},
    {"FBN_JT_TW", "1", kSeam, kPerCall},
    // PC-stable: drivers (pc_driver.cpp, pc_dist.cpp, capi_pc.hip)
    {"FBN_PC_DIST_FORCE_EXCHANGE", "off", kSeam, kOutside},
    {"FBN_PC_FULLSPEC", "16384", kSeam, kPerCall},
    {"FBN_PC_GEN_GENERAL", "off", kSeam, kPerCall},
    {"FBN_PC_GROWTH", "4 (host rounds), 2 (device level 1)", kSeam, kPerCall},
    {"FBN_PC_HOST_L0L1", "off", kSeam, kPerCall},
    {"FBN_PC_HOST_L1", "off", kSeam, kPerCall},
    {"FBN_PC_L0CHUNK", "4194304", kSeam, kPerCall},
    {"FBN_PC_L1CAP", "524288", kSeam, kPerCall},
    {"FBN_PC_L1_MAXCHUNK", "65536", kSeam, kPerCall},
    {"FBN_PC_NO_MISCREEN", "off", kSeam, kPerCall},
    {"FBN_PC_NO_SMALL", "off", kSeam, kPerCall},
    {"FBN_PC_PIPELINE_EDGES", "kPipelineEdges", kSeam, kPerCall},
    {"FBN_PC_ROUND0", "8192", kSeam, kPerCall},
    {"FBN_PC_SMALL_COOP", "unset: cooperative launch where it fits", kSeam, kPerCall},
    {"FBN_PC_SMALL_FAIL", "unset", kSeam, kPerCall},
    // diagnostics: print or record only
    {"FBN_JT_PLACE_DEBUG", "off", kDiagnostic, kPerCall},
    {"FBN_JT_PROFILE", "0", kDiagnostic, kPerCall},
    {"FBN_JT_VDEBUG", "0", kDiagnostic, kPerCall},
    {"FBN_PC_SMALL_TRACE", "off", kDiagnostic, kOnce},
    {"FBN_PC_TIMING", "off", kDiagnostic, kOnce},
    {"FBN_PLAN_TIMING", "off", kDiagnostic, kOnce},
    // locations and limits
    {"FBN_KERNEL_CACHE", "fastbn_amd/kcache beside the library", kLocation, kPerCall},
    {"FBN_LIB_PATH", "libfastbn.so beside the package", kLocation, kOutside},
    {"OMP_NUM_THREADS", "min(16, hardware threads)", kLocation, kPerCall},
};

// the value of a knob of the table, nullptr when unset
inline const char *KnobValue(const char *name) {
    for (const Knob &k : kKnobs)
        if (!strcmp(k.name, name)) return getenv(name);
    abort();  // a read of a name the table does not list
}

inline bool KnobSet(const char *name) { return KnobValue(name) != nullptr; }

inline int64_t KnobOr(const char *name, int64_t dflt) {
    const char *v = KnobValue(name);
    return v ? atoll(v) : dflt;
}

// diagnostic: host phase times of the PC drivers on stderr
inline bool PcTiming() {
    static const bool on = KnobSet("FBN_PC_TIMING");
    return on;
}

// threads of the host twins and the loaders: at most 16, at most OMP_NUM_THREADS
inline int HostThreads() {
    const unsigned hc = std::thread::hardware_concurrency();
    int t = (int)std::max(1u, std::min(16u, hc ? hc : 1u));
    if (const char *e = KnobValue("OMP_NUM_THREADS")) t = std::max(1, std::min(t, atoi(e)));
    return t;
}

}  // namespace fbn

#endif
