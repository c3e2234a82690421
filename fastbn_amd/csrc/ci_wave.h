// ci_wave.h -- the wave-level idioms of the CI kernels (ci_bits_*.hip, ci_l1.hip, ci_kernels.hip),
// written once: the butterfly sum, the store of a per-lane-replicated table (lane c writes cell c)
// and the dispatch over the 4 x 4 state-count classes.  Device-inline; internal to libfastbn.
#ifndef FBN_CI_WAVE_H
#define FBN_CI_WAVE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

// the sum of v over the wave's 64 lanes, in every lane
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// a[lane] of an array every lane holds in registers (static indices only: a select chain)
template <class T, int N>
__device__ __forceinline__ T lane_select(int lane, const T (&a)[N]) {
    T v = 0;
#pragma unroll
    for (int c = 0; c < N; ++c) v = lane == c ? a[c] : v;
    return v;
}

// out[c] (and out2[c], if given) = full[c] for the N cells of a table every lane holds: lane c stores cell c
template <int N>
__device__ __forceinline__ void lane_store(int lane, const int32_t (&full)[N], int32_t *__restrict__ out,
                                           int32_t *__restrict__ out2 = nullptr) {
    if (lane < N) {
        const int32_t v = lane_select(lane, full);
        out[lane] = v;
        if (out2) out2[lane] = v;
    }
}

// M(dx, dy) for every state-count class of a pair on the bit-sliced store (dims 1..4): the cases of a
// `switch (dx * 8 + dy)` whose M expands to `case dx * 8 + dy: ...; break;`
#define FBN_DIMS_4x4(M)                                                                              \
    M(1, 1) M(1, 2) M(1, 3) M(1, 4) M(2, 1) M(2, 2) M(2, 3) M(2, 4) M(3, 1) M(3, 2) M(3, 3) M(3, 4) \
    M(4, 1) M(4, 2) M(4, 3) M(4, 4)

#endif
