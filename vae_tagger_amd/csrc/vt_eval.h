// Streaming multi-label evaluator: layout of the caller-owned state block + launch entry points, shared by eval_metrics.hip and capi.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

constexpr int VT_EVAL_MAX_T = 32;          // thresholds per state
constexpr int VT_EVAL_MAX_B = 4096;        // rows of one update (the per-row mismatch scratch)
constexpr long long VT_EVAL_MAX_N_SEEN = 0x7fffffffLL;    // the sample index is 31 bits of the key's low word
constexpr int VT_EVAL_MAX_MERGE = 64;       // sources of one merge (their descriptors travel as a kernel argument)
constexpr long long VT_EVAL_MICRO_LIMIT = 0x7fffffffLL;   // micro AP on the device while n_seen * N < 2^31

// One block, every section 256-B aligned:
//   thresholds fp64 [32] | row_stats uint64 [3] | row_scratch uint32 [VT_EVAL_MAX_B] | support uint32 [N] | counts uint32 [N][T][2] |
//   keys uint64 [N][capacity]
struct EvalLayout {
    size_t thr, row_stats, row_scratch, support, counts, keys, head_bytes /* everything but the keys */, total;
};
inline size_t vt_eval_align(size_t x) { return (x + 255) / 256 * 256; }
inline EvalLayout vt_eval_layout(int N, int T, long long capacity) {
    EvalLayout l;
    l.thr = 0;
    l.row_stats = l.thr + vt_eval_align(sizeof(double) * VT_EVAL_MAX_T);
    l.row_scratch = l.row_stats + vt_eval_align(sizeof(uint64_t) * 3);
    l.support = l.row_scratch + vt_eval_align(sizeof(uint32_t) * VT_EVAL_MAX_B);
    l.counts = l.support + vt_eval_align(sizeof(uint32_t) * (size_t)N);
    l.keys = l.counts + vt_eval_align(sizeof(uint32_t) * 2 * (size_t)N * (size_t)T);
    l.head_bytes = l.keys;
    l.total = l.keys + vt_eval_align(sizeof(uint64_t) * (size_t)N * (size_t)capacity);
    return l;
}

struct EvalThresholds { double v[VT_EVAL_MAX_T]; };

hipError_t vt_eval_launch_reset(void* state, const EvalLayout& l, const EvalThresholds& thr, hipStream_t s);
hipError_t vt_eval_launch_update(void* state, const EvalLayout& l, const float* probs, const void* labels, int labels_u8, int B, int N,
                                 int T, int t_main, long long capacity, long long n_seen, hipStream_t s);
// sorts the first n_seen keys of every class row in place (descending), writes ap[N]; with micro_ap != nullptr also flattens the store
// into `flat` (n_seen * N keys), sorts it and writes micro_ap[0]
hipError_t vt_eval_launch_ap(void* state, const EvalLayout& l, int N, long long capacity, long long n_seen, double* ap, double* micro_ap,
                             unsigned long long* flat, hipStream_t s);

// One source of the export / merge key kernel: the first n keys of every class row (row pitch `pitch`) of the block at `base` go to
// destination columns [off, off + n) with off << 1 subtracted from each key (the sample index moves by off); columns [n, fill) are
// zero-filled.  The head sections and the start of the keys sit at the destination's offsets: they do not depend on the capacity.
struct EvalMergeSrc { const char* base; long long pitch, n, fill, off; };
struct EvalMergeArg { EvalMergeSrc src[VT_EVAL_MAX_MERGE]; int W; };

// copies a state into a block of capacity out_capacity (>= n_seen, or 0: head only): head copied, row scratch zeroed, the first n_seen
// key columns copied, the padding columns and the key section's alignment tail zero-filled.  vec: 16-B accesses on the aligned part.
hipError_t vt_eval_launch_export(const void* state, const EvalLayout& l, void* out, const EvalLayout& lo, int N, long long capacity,
                                 long long n_seen, long long out_capacity, int vec, hipStream_t s);
// adds the sources' support / counts / row_stats into dst and (dst_capacity > 0) appends their keys: two launches whatever a.W is
hipError_t vt_eval_launch_merge(void* dst, const EvalLayout& l, int N, long long dst_capacity, const EvalMergeArg& a, int vec, hipStream_t s);

// recount under one threshold per class (DEVICE thr [N], fp64) from the first n_seen keys of every class row; the state is only read.
// counts_out [N][2] = (tp, fp), row_stats_out [3] = (exactly matching rows, mismatching elements, non-finite probabilities); the
// workspace (vt_eval_recount_ws_bytes) holds the accumulators and the per-sample mismatch tally, zeroed by the call itself.
size_t vt_eval_recount_ws_bytes(int N, long long n_seen);
hipError_t vt_eval_launch_recount(const void* state, const EvalLayout& l, int N, long long capacity, long long n_seen, const double* thr,
                                  uint32_t* counts_out, unsigned long long* row_stats_out, void* ws, hipStream_t s);
