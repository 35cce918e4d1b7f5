// Classifier-head trainer: layout of the caller-owned state block and of the per-call workspace, and the dropout generator
// (train_head.hip; mirrored by vae_tagger_amd/train.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "vt_decoder.h"
#include "vt_eval.h"

constexpr int VT_HEAD_RING = 256;           // per-step loss values kept: slot = step % VT_HEAD_RING
constexpr int VT_HEAD_MAX_B = 4096;
constexpr int VT_HEAD_ROWS_LAST = 32;       // output rows of one backward workgroup, last layer / hidden layers
constexpr int VT_HEAD_ROWS_HIDDEN = 16;
constexpr int VT_HEAD_TENSORS = 14;         // at most 3 x (weight, bias, ln weight, ln bias) + (weight, bias)

// Parameter tensors in state order: per hidden layer i  classifier.{4i}.weight [d(i+1)][d(i)], classifier.{4i}.bias,
// classifier.{4i+1}.weight (LayerNorm), classifier.{4i+1}.bias; then classifier.{4 hidden}.weight [N][d(hidden)] and its bias.
// Every tensor starts on a multiple of 64 floats; the padding stays zero in all four arrays.
struct HeadTensor { int module; int is_bias; size_t off, numel; };      // name = classifier.<module>.<weight|bias>

// One block, every section 256-B aligned:
//   params fp32 [P] | grads fp32 [P] | adam m fp32 [P] | adam v fp32 [P] | scalars { fp64 squared norm, fp32 norm, fp32 clip coefficient } |
//   loss ring fp64 [VT_HEAD_RING] | squared-norm partials fp64 [norm_parts]: one per workgroup of the kernels that write gradients
struct HeadLayout {
    DecHeadShape shape;
    int ntensors;
    HeadTensor t[VT_HEAD_TENSORS];
    size_t P;                                // floats of one parameter array (padded)
    size_t params, grads, m, v, scalars, ring, normpart, total;
    int groups[4], kblocks[4], part_base[4]; // backward grid of linear layer l and its first squared-norm partial
    int norm_parts;
};

inline int vt_head_rows(const DecHeadShape& s, int l) { return l == s.hidden ? VT_HEAD_ROWS_LAST : VT_HEAD_ROWS_HIDDEN; }

inline HeadLayout vt_head_layout(const DecHeadShape& s) {
    HeadLayout l;
    l.shape = s;
    size_t off = 0;
    int n = 0;
    auto add = [&](int module, int is_bias, size_t numel) {
        l.t[n].module = module; l.t[n].is_bias = is_bias; l.t[n].off = off; l.t[n].numel = numel;
        off += (numel + 63) / 64 * 64;
        ++n;
    };
    for (int i = 0; i <= s.hidden; ++i) {
        add(4 * i, 0, (size_t)s.dims[i + 1] * s.dims[i]);
        add(4 * i, 1, (size_t)s.dims[i + 1]);
        if (i < s.hidden) { add(4 * i + 1, 0, (size_t)s.dims[i + 1]); add(4 * i + 1, 1, (size_t)s.dims[i + 1]); }
    }
    l.ntensors = n;
    l.P = off;
    l.norm_parts = 0;
    for (int i = 0; i <= s.hidden; ++i) {
        const int rows = vt_head_rows(s, i);
        l.groups[i] = (s.dims[i + 1] + rows - 1) / rows;
        l.kblocks[i] = s.dims[i] / 256;
        l.part_base[i] = l.norm_parts;
        l.norm_parts += l.groups[i] * l.kblocks[i];
    }
    l.params = 0;
    l.grads = l.params + vt_eval_align(4 * l.P);
    l.m = l.grads + vt_eval_align(4 * l.P);
    l.v = l.m + vt_eval_align(4 * l.P);
    l.scalars = l.v + vt_eval_align(4 * l.P);
    l.ring = l.scalars + 256;
    l.normpart = l.ring + vt_eval_align(sizeof(double) * VT_HEAD_RING);
    l.total = l.normpart + vt_eval_align(sizeof(double) * (size_t)l.norm_parts);
    return l;
}

// Workspace of one forward / forward_backward call (floats unless noted), every section 256-B aligned:
//   per hidden layer i: z (the linear's output), a (after LayerNorm, activation, dropout), dt (grad of the LayerNorm output),
//   xh (normalised z), dz (grad of z), each [B][d(i+1)] | logits [B][N] | dy [B][N] | dX partials [max groups][B][K] |
//   loss partials fp64 [ceil(N / 64)]
struct HeadWorkspace { size_t z[3], a[3], dt[3], xh[3], dz[3], logits, dy, part, losspart, total; };
inline HeadWorkspace vt_head_workspace(const HeadLayout& l, int B) {
    const DecHeadShape& s = l.shape;
    HeadWorkspace w;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += vt_eval_align(bytes); return o; };
    for (int i = 0; i < s.hidden; ++i) {
        const size_t n = 4 * (size_t)B * s.dims[i + 1];
        w.z[i] = take(n); w.a[i] = take(n); w.dt[i] = take(n); w.xh[i] = take(n); w.dz[i] = take(n);
    }
    const size_t N = (size_t)s.dims[s.hidden + 1];
    w.logits = take(4 * (size_t)B * N);
    w.dy = take(4 * (size_t)B * N);
    size_t part = 0;
    for (int i = 1; i <= s.hidden; ++i) {                      // (layer 0 reads the frozen features: no dX)
        const size_t p = (size_t)l.groups[i] * B * s.dims[i];
        if (p > part) part = p;
    }
    w.part = take(4 * part);
    w.losspart = take(sizeof(double) * ((N + 63) / 64));
    w.total = off;
    return w;
}

// Dropout: a counter-based generator, no stored state.  Element `idx` of hidden layer `layer` at (seed, step) is KEPT when the top 24
// bits of two rounds of the splitmix64 finaliser over (seed, step) and (layer, idx), as a fraction of 2^24, are >= p.
#if defined(__HIPCC__)
#define VT_TRAIN_HD __host__ __device__
#else
#define VT_TRAIN_HD
#endif
VT_TRAIN_HD inline uint64_t vt_head_mix64(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
VT_TRAIN_HD inline bool vt_head_keep(uint64_t seed, uint64_t step, int layer, uint64_t idx, float p) {
    uint64_t x = vt_head_mix64(seed + 0x9E3779B97F4A7C15ull * (step + 1));
    x = vt_head_mix64(x ^ ((uint64_t)(layer + 1) << 56) ^ idx);
    return (float)(uint32_t)(x >> 40) * (1.0f / 16777216.0f) >= p;
}
