// jt_psample_program.h -- exact posterior sampling on the junction forest: what the host twin
// (jt_psample_host.cpp), the kernel (jt_psample.hip) and the handle (capi_psample.hip) share.  The program
// is the max-product program of jt_mpe_program.h unchanged (CompileJTProgramMpe); only the store of one
// wave differs.  The algorithm is stated in include/fastbn.h above fbn_psample_create.
//
// The store of one wave, rows of one fp64 / int64 per column [row][64]:
//   message rows   one per separator entry: the sum-product Collect message of the separator's child clique
//   exponent rows  one per separator
//   e* rows        kPsampleU per clique: the entry each of a lane's kPsampleU draws in flight chose
// Message and exponent rows are indexed by the case's column (case 64 b + j of block b in column j); the e*
// rows by the lane that draws.
#ifndef FBN_JT_PSAMPLE_PROGRAM_H
#define FBN_JT_PSAMPLE_PROGRAM_H

#include <stdint.h>

#include "jt_mpe_program.h"
#include "sample_model.h"

// independent draws a lane keeps in flight (measured against the other two of {1, 2, 4}: DESIGN.md 5.12)
constexpr int kPsampleU = 4;

// what fbn_psample_launch takes (launchers.h), filled by name in capi_psample.hip; passed to the kernel by value
struct JtPsampleArgs {
    const JtMClique *cl;
    const int32_t *aux;
    const double *initv;
    const uint64_t *dig;
    const int32_t *collect;  // clique ids: deepest level first, plan order within a level
    const int32_t *trace;    // clique ids: levels ascending, plan order within a level
    const int8_t *evid;      // [ncases][V], checked
    int8_t *samples;         // [ncases][S][V]
    double *value;           // [ncases][2]: P(e) = m * 2^ex
    double *store;           // [grid][store_rows][64]
    long long ncases, S, case0;
    long long chunk;         // samples per unit (1 .. S); a unit is (64-case block, chunk)
    long long store_rows;    // msg_rows + nsep + kPsampleU * nc
    int nc, V, msg_rows, nsep;
    int grid;
    fbn::U128 state, inc;  // PCG64(seed) after seeding
    uint64_t jump[256];    // this seed's 2^j jump pairs (PcgStream::jump)
};

namespace fbn {

// nsamples >= 1, at most 2^31 - 1 samples per call, stream positions (case_offset + ncases) * S * nc below 2^63
int CheckPsampleShape(const JTProgramMpe &P, int64_t ncases, int64_t S, int64_t case_offset);
// The host twin: samples [ncases][S][V], value [ncases][2].  Cases spread over HostThreads() threads.
int HostPsample(const JTProgramMpe &P, const int8_t *ev, int64_t ncases, int64_t S, uint64_t seed, int64_t case_offset,
                int8_t *samples, double *value);

}  // namespace fbn

#endif
