// The descending bitonic network over 64-bit keys, shared by its two users: vt_get_confidence (decoder.hip: rows = images, keys = tags) and
// the evaluator's per-class ranking (eval_metrics.hip: rows = classes, keys = samples).  Keys in, keys out; what a key means is the caller's.
//
// The network is the single-direction ("flip") bitonic sort: stage k compares i with i ^ (k - 1) first and then i ^ j for j = k/4 .. 1,
// every exchange in the same direction, so elements beyond n are virtual minimum keys that never move and n needs no power-of-two
// padding.  Up to VT_SORT_CH keys a whole row sorts in LDS in one launch; beyond that each VT_SORT_CH-block is sorted in LDS, the
// j >= VT_SORT_CH steps of the later stages run as global-memory passes and each stage's tail (j < VT_SORT_CH) runs in LDS again.
#pragma once
#include <hip/hip_runtime.h>

constexpr int VT_SORT_CH = 16384;                            // keys of one LDS pass (128 KB of the 160 KB)

// high word of a key: the fp32 score mapped to an unsigned whose order is the score's (NaN -> 1: after every real value, -inf
// included; -0.0 ties with +0.0, as in a comparison sort)
__device__ __forceinline__ unsigned vt_sort_key_hi(float f) {
    unsigned u = __float_as_uint(f);
    if (u == 0x80000000u) u = 0u;
    return (f != f) ? 1u : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));
}
__device__ __forceinline__ float vt_sort_key_score(unsigned u) {
    if (u == 1u) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// one compare-exchange step over the np LDS slots of a block that holds n real keys (workgroup of 1024 threads)
__device__ __forceinline__ void vt_sort_lds_step(unsigned long long* key, int n, int np, int j, bool flip, int kk) {
    for (int i = threadIdx.x; i < np; i += 1024) {
        const int l = flip ? (i ^ (kk - 1)) : (i ^ j);
        if (l > i && l < n) {
            const unsigned long long a = key[i], c = key[l];
            if (a < c) { key[i] = c; key[l] = a; }           // descending
        }
    }
    __syncthreads();
}
// every stage k = 2 .. np: sorts the block
__device__ __forceinline__ void vt_sort_lds_full(unsigned long long* key, int n, int np) {
    for (int k = 2; k <= np; k <<= 1) {
        vt_sort_lds_step(key, n, np, 0, true, k);
        for (int j = k >> 2; j > 0; j >>= 1) vt_sort_lds_step(key, n, np, j, false, 0);
    }
}
// the steps j = VT_SORT_CH / 2 .. 1 of a stage k > VT_SORT_CH
__device__ __forceinline__ void vt_sort_lds_tail(unsigned long long* key, int n, int np) {
    for (int j = VT_SORT_CH >> 1; j > 0; j >>= 1) vt_sort_lds_step(key, n, np, j, false, 0);
}
// one global-memory step of stage k for pair number t of a row of N keys: flip (partner i ^ (k - 1)) or plain (partner i ^ j);
// pairs with a partner >= N stay.  I is the index type (int up to 2^30 keys per row, long long beyond).
template <typename I>
__device__ __forceinline__ void vt_sort_global_step(unsigned long long* __restrict__ kb, I N, I k, I j, int flip, I t) {
    const I half = flip ? (k >> 1) : j;
    const I i = ((t / half) * 2) * half + (t % half);        // lower element of pair t
    const I l = flip ? (i ^ (k - 1)) : (i ^ j);
    if (l >= N || i >= N) return;
    const unsigned long long a = kb[i], c = kb[l];
    if (a < c) { kb[i] = c; kb[l] = a; }
}
