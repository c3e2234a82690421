// order_mcmc.h -- what the order-MCMC sampler's kernels (order_mcmc.hip), its device entry (capi_omcmc.hip) and
// its host twin (order_mcmc_host.cpp) share: the family-list entry, the limits, the stream positions of a
// chain, the proposal and the start permutation, the options' checks, the list builder and the result record.
// The arithmetic is exact_lse.h's (fbn_lse_exp) and hc_bd.h's (fbn_bd_ln); the generator is sample_model.h's
// PCG64.  include/fastbn.h ("order MCMC") states the definitions.  Internal to libfastbn.
#ifndef FBN_ORDER_MCMC_H
#define FBN_ORDER_MCMC_H

#include <cstdint>
#include <vector>

#include "exact_lse.h"
#include "hc_search.h"
#include "sample_model.h"

constexpr int kOmcmcMaxVars = 64;                         // a parent set is one 64-bit mask, an arc row one wave
constexpr int64_t kOmcmcMaxFamilies = (int64_t)1 << 26;   // list entries in all: 1 GiB of (mask, score) pairs
constexpr int kOmcmcChainBits = 40;                       // stream positions a chain owns: 2^40
constexpr int kOmcmcStartDraws = 64;                      // positions [0, 64) of a chain: its start permutation
constexpr int64_t kOmcmcMaxSteps = ((int64_t)1 << 38) - 64;  // 64 + 3 steps stays below 2^40
constexpr int64_t kOmcmcMaxChains = (int64_t)1 << 23;     // chain_offset + chains: positions stay below 2^63
constexpr int kOmcmcGroupMax = 16;                        // chains (waves) per workgroup, fbn_omcmc_set_tuning
constexpr int kOmcmcGroupDefault = 4;

// one candidate parent set of a node: the variables as bits, the local score with the prior's term added
struct alignas(16) OmcmcEntry {
    uint64_t mask;
    double score;
};

// ---- the stream of chain g (= chain_offset + c): position (g << 40) + k for draw k of the start permutation,
// (g << 40) + 64 + 3 t for the three draws of step t (0-based).  A draw at position p is the output after p + 1
// steps of the seeded generator.
FBN_HD uint64_t OmcmcStartPos(uint64_t g) { return g << kOmcmcChainBits; }
FBN_HD uint64_t OmcmcStepPos(uint64_t g, uint64_t t) { return (g << kOmcmcChainBits) + (uint64_t)kOmcmcStartDraws + 3u * t; }

// the start permutation: Fisher-Yates from the top, draw k (k = n - 1 .. 1) picks j = floor(r k' / 2^64), k' = k + 1;
// s is the state at OmcmcStartPos(g)
template <class Bytes>
FBN_HD void OmcmcStartOrder(fbn::U128 s, fbn::U128 inc, int n, Bytes order) {
    for (int p = 0; p < n; ++p) order[p] = (uint8_t)p;
    for (int k = n - 1; k >= 1; --k) {
        s = fbn::PcgStep(s, inc);
        const int j = (int)fbn::MulHi64(fbn::PcgOutput(s), (uint64_t)(k + 1));
        const uint8_t t = order[k];
        order[k] = order[j];
        order[j] = t;
    }
}

// the proposal of one step from its first two draws: two distinct positions i < j, uniform over the pairs
FBN_HD void OmcmcProposal(uint64_t r1, uint64_t r2, int n, int *i, int *j) {
    const int a = (int)fbn::MulHi64(r1, (uint64_t)n);
    int b = (int)fbn::MulHi64(r2, (uint64_t)(n - 1));
    if (b >= a) ++b;
    *i = a < b ? a : b;
    *j = a < b ? b : a;
}

// Metropolis-Hastings with a symmetric proposal: accept iff delta >= 0 or u < e^delta
FBN_HD bool OmcmcAccept(double delta, double u) { return delta >= 0.0 || u < fbn_lse_exp(delta); }

// ---- host side
struct fbn_omcmc_result {
    fbn_omcmc_info info{};
    std::vector<double> arc_prob, chain_arc_prob, log_score;  // [n][n], [chains][n][n], [chains][samples]
    std::vector<int32_t> orders;                              // [chains][n]
    std::vector<int64_t> accepted;                            // [chains]
};

namespace fbn {

// the family lists of all nodes: node v owns ent[off[v] .. off[v + 1]), the empty set first
struct OmcmcLists {
    std::vector<int64_t> off;
    std::vector<OmcmcEntry> ent;
};

// prior 0 / 1, 1 .. 64 variables (FBN_ERR_LIMIT past that), state counts, penalty and the allowed mask's length
int OmcmcCheck(int nvars, const int32_t *dims, const fbn_exact_options &opt, int prior);
// chains, samples, thin >= 1, burn_in, chain_offset, max_families >= 0 (FBN_ERR_ARG); chain_offset + chains and the
// steps within the stream's layout (FBN_ERR_LIMIT)
int OmcmcCheckRun(const fbn_omcmc_options &m);
// orders [k][n]: k >= 1 permutations of 0 .. n - 1, else FBN_ERR_ARG naming the first bad one
int OmcmcCheckOrders(int n, const int32_t *orders, int64_t k);
// Counts the candidates of every node first (FBN_ERR_LIMIT with the count past `cap`, 0 = kOmcmcMaxFamilies, before
// anything is scored), then scores them through `scorer` in the shared enumerator's batches.
int OmcmcBuildLists(int n, const int32_t *dims, const fbn_exact_options &opt, int prior, const HcScorer &scorer, int64_t cap,
                    OmcmcLists *out, fbn_exact_info *xi);
// the result's shape and the run's counters from the options and the scorer's record
void OmcmcStartResult(int n, int prior, const fbn_omcmc_options &m, const OmcmcLists &L, const fbn_exact_info &xi,
                      fbn_omcmc_result *res);
// From the chains' raw outputs -- acc [chains][n][64] (acc[c][v][u] = the sum over samples of P(u -> v | order)),
// last orders as bytes [chains][64] -- the per-chain means, their mean in chain order, the orders as int32.
void OmcmcFinish(int n, const fbn_omcmc_options &m, const double *acc, const uint8_t *orders, fbn_omcmc_result *res);
// the twin of the chain kernel and of the scan kernel (order_mcmc_host.cpp)
void OmcmcHostChains(int n, const OmcmcLists &L, const fbn_omcmc_options &m, double *acc, uint8_t *orders, double *trace,
                     int64_t *accepted);
void OmcmcHostTerms(int n, const OmcmcLists &L, const int32_t *orders, int64_t k, double *term, double *arcs);

}  // namespace fbn

#if defined(__HIPCC__)
namespace fbn {

// omcmc_chain_kernel's arguments (order_mcmc.hip; filled by capi_omcmc.hip): the steps [t0, t1) of chains
// [0, chains), chain c being chain chain0 + c of the seed.  t0 == 0 starts the chains (start order, zeroed
// accumulators); a later launch resumes from the parked orders.
struct OmcmcDeviceArgs {
    const OmcmcEntry *ent;
    const long long *off;  // [n + 1]
    int n, group;          // group: chains (waves) per workgroup
    U128 state, inc;
    uint64_t jump[256];    // this seed's 2^j jump pairs (PcgStream::jump), read from the kernel arguments
    long long chains, chain0, burn_in, thin, samples, t0, t1;
    uint8_t *orders;       // [chains][64]: parked between launches, the last orders after the final one
    double *acc;           // [chains][n][64]: acc[c][v][u], the sum over samples of P(u -> v | order)
    double *trace;         // [chains][samples]
    long long *accepted;   // [chains]
};
// omcmc_terms_kernel's: the scan of k given orders
struct OmcmcTermsArgs {
    const OmcmcEntry *ent;
    const long long *off;
    int n, group;
    const int32_t *orders;  // [k][n], checked
    long long k;
    double *term, *arcs;    // [k][n], [k][n][n]
};

}  // namespace fbn
#endif

#endif
