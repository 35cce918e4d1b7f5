// Streaming validation-loss accumulator: layout of the caller-owned state block (eval_loss.hip; mirrored by vae_tagger_amd/losses.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "vt_eval.h"

constexpr int VT_LOSS_TC = 64;              // classes of one workgroup: one partial of the batch scalars per workgroup
constexpr int VT_LOSS_MAX_N = 1 << 24;

// One block, every section 256-B aligned:
//   params { fp64 alpha, fp64 gamma, uint64 has_weights, uint64 N } | totals { fp64 [3] sums of per-batch means (bce, focal, weighted bce),
//   uint64 [3] steps, elements, non-finite logits } | class weights fp64 [N] (1.0 without weights) | class sums fp64 [N][2] (bce, focal) |
//   partials of the last update, per workgroup of 64 classes { fp64 [3], uint64 non-finite }
struct LossLayout {
    size_t params, totals, weights, sums, partials, total;
    int groups;                              // workgroups of one update = ceil(N / 64): a function of N alone
};
inline LossLayout vt_loss_layout(int N) {
    LossLayout l;
    l.groups = (N + VT_LOSS_TC - 1) / VT_LOSS_TC;
    l.params = 0;
    l.totals = l.params + vt_eval_align(32);
    l.weights = l.totals + vt_eval_align(48);
    l.sums = l.weights + vt_eval_align(sizeof(double) * (size_t)N);
    l.partials = l.sums + vt_eval_align(sizeof(double) * 2 * (size_t)N);
    l.total = l.partials + vt_eval_align(32 * (size_t)l.groups);
    return l;
}
