// Per-image (example-based) precision / recall / F1: layout of the caller-owned state block (eval_samples.hip; mirrored by
// vae_tagger_amd/sample_metrics.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "vt_eval.h"

constexpr int VT_SAMPLE_MAX_T = VT_EVAL_MAX_T;     // thresholds per state
constexpr int VT_SAMPLE_MAX_B = VT_EVAL_MAX_B;     // rows of one update
constexpr int VT_SAMPLE_HEADER_WORDS = 32;         // uint64 words in front of the non-finite slots

// One block, every section 256-B aligned:
//   thresholds fp64 [32] | totals { uint64 header [32] = (rule, T, 0...), uint32 nonfinite [VT_SAMPLE_MAX_B] } |
//   true uint32 [capacity] | rows uint32 [capacity][T][2] = (tp, predicted)
// nonfinite[b] = non-finite probabilities seen in row b of every update (owned by that row's workgroup: no atomics); their sum is the
// total.  A merge of shards concatenates `true` and `rows` and adds the slots.
struct SampleLayout {
    size_t thr, totals, nonfinite, true_at, rows, head_bytes /* thresholds + totals */, total;
};
inline SampleLayout vt_sample_layout(int T, long long capacity) {
    SampleLayout l;
    l.thr = 0;
    l.totals = l.thr + vt_eval_align(sizeof(double) * VT_SAMPLE_MAX_T);
    l.nonfinite = l.totals + sizeof(uint64_t) * VT_SAMPLE_HEADER_WORDS;
    l.true_at = l.totals + vt_eval_align(sizeof(uint64_t) * VT_SAMPLE_HEADER_WORDS + sizeof(uint32_t) * VT_SAMPLE_MAX_B);
    l.head_bytes = l.true_at;
    l.rows = l.true_at + vt_eval_align(sizeof(uint32_t) * (size_t)capacity);
    l.total = l.rows + vt_eval_align(sizeof(uint32_t) * 2 * (size_t)T * (size_t)capacity);
    return l;
}

// vt_sample_finish's output: fp64 sums [T][3] = (precision, recall, F1) | uint64 [T][2] = (exact matches, images with no prediction) |
// uint64 [2] = (images with no true tag, non-finite probabilities)
inline size_t vt_sample_out_bytes(int T) { return (size_t)T * (3 * sizeof(double) + 2 * sizeof(uint64_t)) + 2 * sizeof(uint64_t); }
