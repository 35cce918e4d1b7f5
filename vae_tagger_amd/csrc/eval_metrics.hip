// Streaming multi-label evaluator on the device (evaluation.py's MultiLabelEvaluator / find_optimal_threshold without an n x c host
// matrix): per batch one launch folds the probabilities into integer confusion counts for up to 32 thresholds and appends one sort key
// per (class, sample); at the end the class rows are ranked with the shared bitonic network (vt_sort_network.h) and one workgroup per
// class sums the average precision in fp64 in a fixed order.  Every counter is an integer owned by one thread or reached by integer
// atomics only, so the state is bit-reproducible whatever the launch timing.
// Sharded evaluation: a state is exported as a compact block and several blocks are merged into one state (a head kernel adding the
// integers, a key kernel appending the class rows with the sample index rebased) -- no atomics, no LDS.
// Recount: a read-only pass over the stored keys re-decides every prediction under one threshold per class (vt_eval_recount): the
// metrics at another operating point, or under per-class thresholds, without feeding the samples again.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "vt_common.h"
#include "vt_eval.h"
#include "vt_sort_network.h"

namespace {

constexpr int EV_TC = 64;      // classes of one workgroup's tile: one wave = the 64 classes of one threshold group
constexpr int EV_RB = 64;      // rows staged per LDS pass
constexpr int EV_TS = VT_EVAL_MAX_T / 4;   // thresholds per thread (4 waves share the 32)

struct ThrArg { EvalThresholds t; };

__global__ __launch_bounds__(64) void eval_init_kernel(double* __restrict__ thr, ThrArg a) {
    if (threadIdx.x < VT_EVAL_MAX_T) thr[threadIdx.x] = a.t.v[threadIdx.x];
}

// One call per batch.  Workgroup = 64 classes x every row of the batch, staged 64 rows at a time through LDS:
//   * wave g owns, for each of its 64 classes, the thresholds g, g + 4, ...: (tp, fp) live in registers over the whole batch and are
//     added to counts[class][t] by that one thread at the end;
//   * the wave that owns t_main counts each row's mismatching classes with one ballot and adds it to row_scratch[row] (integer atomic:
//     157 workgroups meet there at N = 10000); eval_fold_rows_kernel turns the scratch into row_stats afterwards;
//   * the tile is written out transposed, so that the rows' keys of one class leave as one contiguous run of the class-major store.
// The comparison is (double)p > thr[t], strict: what numpy computes for float32_array > float64_scalar.
template <typename L>
__global__ __launch_bounds__(256) void eval_accumulate_kernel(const float* __restrict__ probs, const L* __restrict__ labels, int B, int N,
                                                              int T, int t_main, const double* __restrict__ thr,
                                                              uint32_t* __restrict__ counts, uint32_t* __restrict__ support,
                                                              unsigned long long* __restrict__ row_stats, uint32_t* __restrict__ row_scratch,
                                                              unsigned long long* __restrict__ keys, long long capacity, long long n_seen) {
    __shared__ float sp[EV_RB][EV_TC + 1];
    __shared__ unsigned char sy[EV_RB][EV_TC + 4];
    const int tid = threadIdx.x, c = tid & 63, g = tid >> 6;
    const int c0 = blockIdx.x * EV_TC, cls = c0 + c;
    const bool valid = cls < N;
    double th[EV_TS];
    uint32_t tp[EV_TS], fp[EV_TS];
#pragma unroll
    for (int s = 0; s < EV_TS; ++s) {
        const int t = g + 4 * s;
        th[s] = t < T ? thr[t] : __longlong_as_double(0x7ff0000000000000LL);     // +inf: never exceeded
        tp[s] = 0; fp[s] = 0;
    }
    const double th_main = thr[t_main];
    const bool main_wave = g == (t_main & 3);
    uint32_t sup = 0, bad = 0;
    for (int b0 = 0; b0 < B; b0 += EV_RB) {
        const int rows = min(EV_RB, B - b0);
        for (int i = tid; i < rows * EV_TC; i += 256) {
            const int r = i >> 6, cc = i & 63;
            float p = 0.f;
            unsigned char y = 0;
            if (r < rows && c0 + cc < N) {
                const long long o = (long long)(b0 + r) * N + c0 + cc;
                p = probs[o];
                y = labels[o] > 0 ? 1 : 0;
            }
            sp[r][cc] = p; sy[r][cc] = y;
        }
        __syncthreads();
        for (int r = 0; r < rows; ++r) {
            const float p = sp[r][c];
            const uint32_t y = sy[r][c];
            const double dp = (double)p;
#pragma unroll
            for (int s = 0; s < EV_TS; ++s) {
                const uint32_t pred = dp > th[s] ? 1u : 0u;
                tp[s] += pred & y;
                fp[s] += pred & (y ^ 1u);
            }
            if (main_wave) {                                 // wave-uniform
                const uint32_t pred = dp > th_main ? 1u : 0u;
                const unsigned long long m = __ballot(valid && pred != y);
                if (c == 0 && m) atomicAdd(&row_scratch[b0 + r], (uint32_t)__popcll(m));
            }
            if (g == 0) {
                sup += y;
                bad += (valid && !(fabsf(p) <= 3.0e38f)) ? 1u : 0u;
            }
        }
        if (keys) {
            int rsh = 0;
            while ((1 << rsh) < rows) ++rsh;                 // rows rounded up to a power of two: 16 keys = one 128-B line per class at batch 16
            for (int i = tid; i < (EV_TC << rsh); i += 256) {
                const int cc = i >> rsh, r = i & ((1 << rsh) - 1);   // consecutive lanes = consecutive samples of one class
                if (r < rows && c0 + cc < N) {
                    const long long col = n_seen + b0 + r;
                    const unsigned lo = ((~(unsigned)col) << 1) | (unsigned)sy[r][cc];
                    keys[(long long)(c0 + cc) * capacity + col] = ((unsigned long long)vt_sort_key_hi(sp[r][cc]) << 32) | lo;
                }
            }
        }
        __syncthreads();
    }
    if (valid) {
#pragma unroll
        for (int s = 0; s < EV_TS; ++s) {
            const int t = g + 4 * s;
            if (t < T) {
                uint32_t* o = counts + ((long long)cls * T + t) * 2;
                o[0] += tp[s]; o[1] += fp[s];
            }
        }
        if (g == 0) support[cls] += sup;
    }
    if (g == 0) {
        for (int d = 32; d > 0; d >>= 1) bad += __shfl_down(bad, d);
        if (c == 0 && bad) atomicAdd(&row_stats[2], (unsigned long long)bad);
    }
}

// row_scratch[b] = mismatching classes of row b at t_main -> row_stats (exactly matching rows, mismatching elements); clears the scratch
__global__ __launch_bounds__(256) void eval_fold_rows_kernel(uint32_t* __restrict__ row_scratch, int B, unsigned long long* __restrict__ row_stats) {
    __shared__ unsigned s_exact;
    __shared__ unsigned long long s_mis;
    if (threadIdx.x == 0) { s_exact = 0; s_mis = 0; }
    __syncthreads();
    unsigned exact = 0;
    unsigned long long mis = 0;
    for (int b = threadIdx.x; b < B; b += 256) {
        const uint32_t m = row_scratch[b];
        exact += m == 0;
        mis += m;
        row_scratch[b] = 0;
    }
    atomicAdd(&s_exact, exact);
    atomicAdd(&s_mis, mis);
    __syncthreads();
    if (threadIdx.x == 0) { row_stats[0] += s_exact; row_stats[1] += s_mis; }
}

// ---- descending sort of `rows` rows of n prepared keys at row pitch `pitch` (the network of vt_sort_network.h) ---------------------
// MODE 0: sort every VT_SORT_CH-block; MODE 1: the LDS tail of a later stage.  blockIdx.x = row * chunks + chunk.
template <int MODE>
__global__ __launch_bounds__(1024) void eval_sort_local_kernel(unsigned long long* __restrict__ keys, long long pitch, long long n_row, int chunks) {
    extern __shared__ __attribute__((aligned(16))) char sm[];
    unsigned long long* key = (unsigned long long*)sm;
    const long long row = blockIdx.x / chunks, base = (long long)(blockIdx.x % chunks) * VT_SORT_CH;
    const long long left = n_row - base;
    const int n = left < VT_SORT_CH ? (int)left : VT_SORT_CH;
    int np = 2;
    while (np < n) np <<= 1;
    unsigned long long* kb = keys + row * pitch + base;
    for (int i = threadIdx.x; i < np; i += 1024) key[i] = i < n ? kb[i] : 0ull;
    __syncthreads();
    if (MODE == 0) vt_sort_lds_full(key, n, np);
    else vt_sort_lds_tail(key, n, np);
    for (int i = threadIdx.x; i < n; i += 1024) kb[i] = key[i];
}

__global__ __launch_bounds__(256) void eval_sort_global_kernel(unsigned long long* __restrict__ keys, long long pitch, long long n_row,
                                                               long long k, long long j, int flip, long long pair_blocks) {
    const long long row = blockIdx.x / pair_blocks;
    const long long t = (long long)(blockIdx.x % pair_blocks) * 256 + threadIdx.x;
    vt_sort_global_step<long long>(keys + row * pitch, n_row, k, j, flip, t);
}

// ---- average precision of one sorted row ---------------------------------------------------------------------------------------------
constexpr int AP_ITEMS = 8;                  // consecutive keys per thread
constexpr int AP_CHUNK = 1024 * AP_ITEMS;

struct OpAdd { __device__ static unsigned f(unsigned a, unsigned b) { return a + b; } };
struct OpMax { __device__ static unsigned f(unsigned a, unsigned b) { return a > b ? a : b; } };

// exclusive scan of one value per thread over the 1024-thread workgroup (identity 0); *total = the reduction of all
template <typename Op>
__device__ __forceinline__ unsigned ap_block_scan(unsigned v, unsigned* lds /* [16] */, unsigned* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(inc, d);
        if (lane >= d) inc = Op::f(inc, o);
    }
    __syncthreads();                          // the previous use of lds is over
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    unsigned before = 0, all = 0;
    for (int i = 0; i < 16; ++i) {
        const unsigned x = lds[i];
        if (i < w) before = Op::f(before, x);
        all = Op::f(all, x);
    }
    *total = all;
    unsigned excl = __shfl_up(inc, 1);
    if (lane == 0) excl = 0;
    return Op::f(before, excl);
}

// One workgroup per row.  A tie group is a run of equal high words; with TP_g, K_g the cumulative positives / elements at the end of
// group g:  AP = sum_g (TP_g / npos - TP_{g-1} / npos) * (TP_g / K_g)  -- scikit-learn's definition, term for term what evaluation.py's
// _average_precision computes (no fused multiply-add); summed in fp64 in a fixed order (thread-sequential, wave tree, 16 wave partials in order, chunks in order).
// A row without a positive gives NaN.  n < 2^31 (the counters are 32-bit).
__global__ __launch_bounds__(1024) void eval_ap_kernel(const unsigned long long* __restrict__ keys, long long pitch, long long n,
                                                       double* __restrict__ out) {
#pragma clang fp contract(off)                // every term rounds as numpy's does: product, then sum (the Makefile contracts by default)
    __shared__ unsigned s_u[16];
    __shared__ double s_d[16];
    const unsigned long long* kb = keys + (long long)blockIdx.x * pitch;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    unsigned cnt = 0;
    for (long long i = tid; i < n; i += 1024) cnt += (unsigned)kb[i] & 1u;
    unsigned npos_u;
    ap_block_scan<OpAdd>(cnt, s_u, &npos_u);
    if (npos_u == 0) {
        if (tid == 0) out[blockIdx.x] = __longlong_as_double(0x7ff8000000000000LL);
        return;
    }
    const double npos = (double)npos_u;
    double ap = 0.0;
    unsigned carry_tp = 0, carry_last = 0;    // positives before this chunk; TP at the end of the last complete tie group before it
    for (long long base = 0; base < n; base += AP_CHUNK) {
        const long long i0 = base + (long long)tid * AP_ITEMS;
        unsigned hi[AP_ITEMS + 1], tpl[AP_ITEMS];
        unsigned run = 0;
#pragma unroll
        for (int e = 0; e <= AP_ITEMS; ++e) {
            const unsigned long long k = i0 + e < n ? kb[i0 + e] : 0ull;
            hi[e] = (unsigned)(k >> 32);
            if (e < AP_ITEMS) { run += (unsigned)k & 1u; tpl[e] = run; }
        }
        unsigned total, total_last;
        const unsigned off = carry_tp + ap_block_scan<OpAdd>(run, s_u, &total);
        unsigned lmax = 0;
#pragma unroll
        for (int e = 0; e < AP_ITEMS; ++e) {
            const long long i = i0 + e;
            const bool last = i < n && (i == n - 1 || hi[e + 1] != hi[e]);
            if (last) lmax = off + tpl[e];                   // TP never decreases: the latest group end is the maximum
        }
        unsigned prev = ap_block_scan<OpMax>(lmax, s_u, &total_last);
        prev = prev > carry_last ? prev : carry_last;
        double acc = 0.0;
#pragma unroll
        for (int e = 0; e < AP_ITEMS; ++e) {
            const long long i = i0 + e;
            const bool last = i < n && (i == n - 1 || hi[e + 1] != hi[e]);
            if (last) {
                const unsigned tpg = off + tpl[e];
                acc += ((double)tpg / npos - (double)prev / npos) * ((double)tpg / (double)(i + 1));
                prev = tpg;
            }
        }
        for (int d = 32; d > 0; d >>= 1) acc += __shfl_down(acc, d);
        __syncthreads();
        if (lane == 0) s_d[w] = acc;
        __syncthreads();
        if (tid == 0) {
            double c = 0.0;
            for (int i = 0; i < 16; ++i) c += s_d[i];
            ap += c;
        }
        carry_tp += total;
        carry_last = total_last > carry_last ? total_last : carry_last;
    }
    if (tid == 0) out[blockIdx.x] = ap;
}

// class-major store at pitch `capacity` -> one dense row of N * n keys for the micro average; the sample index is dropped (ties need no
// tie-break for AP), the label bit stays
__global__ __launch_bounds__(256) void eval_flatten_kernel(const unsigned long long* __restrict__ keys, long long capacity, long long n,
                                                           long long total, unsigned long long* __restrict__ flat) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long c = i / n, s = i - c * n;
    flat[i] = keys[c * capacity + s] & 0xffffffff00000001ull;
}

// ---- export / merge of state blocks (sharded evaluation) ---------------------------------------------------------------------------
// Key kernel: a strided copy with one integer op per key.  Per class row, source w's first n keys go to destination columns
// [off, off + n) with `sub` = off << 1 subtracted: the low word is (~i << 1) | label = 2^32 - 2 - 2 i + label, so the subtraction
// turns sample i into sample i + off and stays inside the low word while i + off < 2^31 (the host checks the total).  Columns
// [n, fill) of the destination are zero-filled (the export's padding; fill == n in a merge).  blockIdx.x = row * chunks + chunk,
// blockIdx.y = source; a chunk is MERGE_CH keys of one row: consecutive lanes touch consecutive keys (VEC = 1: 8 B per lane) or
// consecutive pairs (VEC = 2: 16 B per lane on the 16-B aligned part of the DESTINATION run, whose first key may sit at an odd
// index; the source pair is read as one 16-B access when it has the same parity and as two 8-B ones when not).
constexpr int MERGE_CH = 2048;

template <int VEC>
__global__ __launch_bounds__(256) void eval_merge_keys_kernel(EvalMergeArg a, size_t keys_at, unsigned long long* __restrict__ dst,
                                                              long long dst_pitch, long long chunks) {
    const EvalMergeSrc s = a.src[blockIdx.y];
    const long long row = blockIdx.x / chunks, c0 = (long long)(blockIdx.x % chunks) * MERGE_CH;
    if (c0 >= s.fill) return;
    const unsigned long long sub = (unsigned long long)s.off << 1;
    const unsigned long long* __restrict__ sk = (const unsigned long long*)(s.base + keys_at) + row * s.pitch;
    unsigned long long* __restrict__ dk = dst + row * dst_pitch + s.off;
    const int tid = threadIdx.x;
    if (VEC == 1) {
#pragma unroll
        for (int k = 0; k < MERGE_CH / 256; ++k) {
            const long long col = c0 + k * 256 + tid;
            if (col < s.fill) dk[col] = col < s.n ? sk[col] - sub : 0ull;
        }
    } else {
        const long long lead = (row * dst_pitch + s.off) & 1;           // keys in front of the first 16-B aligned destination pair
        const bool src_pairs = ((row * s.pitch + lead) & 1) == 0;       // block-uniform: the source pairs are 16-B aligned too
        if (c0 == 0 && lead && tid == 0) dk[0] = 0 < s.n ? sk[0] - sub : 0ull;
#pragma unroll
        for (int k = 0; k < MERGE_CH / 512; ++k) {
            const long long col = lead + c0 + 2 * (k * 256 + tid);
            if (col + 1 < s.fill) {
                ulonglong2 v = make_ulonglong2(0ull, 0ull);
                if (col + 1 < s.n) {
                    if (src_pairs) v = *(const ulonglong2*)(sk + col);
                    else { v.x = sk[col]; v.y = sk[col + 1]; }
                    v.x -= sub; v.y -= sub;
                } else if (col < s.n) {
                    v.x = sk[col] - sub;
                }
                *(ulonglong2*)(dk + col) = v;
            } else if (col < s.fill) {
                dk[col] = col < s.n ? sk[col] - sub : 0ull;
            }
        }
    }
}

// Head kernel: support and counts (one run of uint32 from the support section to the end of the head, the sections' zero padding
// included) and row_stats of W sources added into the destination; every element is owned by one thread, sources in the order given.
__global__ __launch_bounds__(256) void eval_merge_head_kernel(EvalMergeArg a, char* __restrict__ dst, size_t support, size_t row_stats,
                                                              long long quads) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < quads) {
        uint4* d = (uint4*)(dst + support) + i;
        uint4 v = *d;
        for (int w = 0; w < a.W; ++w) {
            const uint4 x = ((const uint4*)(a.src[w].base + support))[i];
            v.x += x.x; v.y += x.y; v.z += x.z; v.w += x.w;
        }
        *d = v;
    }
    if (blockIdx.x == 0 && threadIdx.x < 3) {
        unsigned long long* d = (unsigned long long*)(dst + row_stats) + threadIdx.x;
        unsigned long long v = *d;
        for (int w = 0; w < a.W; ++w) v += ((const unsigned long long*)(a.src[w].base + row_stats))[threadIdx.x];
        *d = v;
    }
}

// ---- recount under a per-class threshold vector, from the stored keys ---------------------------------------------------------------
// A read-only pass over the first n keys of every class row.  blockIdx.x = row * chunks + chunk, a chunk is RC_CH keys of one row read
// 16 B per lane on the 16-B aligned part of the row (a row's first key sits at an odd index when row * pitch is odd: lane 0 of chunk 0
// takes it on its own).  Per key: the probability comes back from the high word (the inverse of vt_sort_key_hi), label and sample index
// from the low word; prediction = (double)p > thr[row], strict, as eval_accumulate_kernel decides.  tp / fp / non-finite are summed per
// workgroup and leave as one integer atomic each into the workspace head; a mismatching element adds 1 to tally[sample] (integer vector
// atomic) -- indexed by the sample the key names, not by its column, so a row that vt_eval_average_precision has sorted counts the same.
constexpr int RC_CH = 4096;

struct RecountAcc { unsigned tp, fp, bad; };

__device__ __forceinline__ void recount_key(unsigned long long k, double th, long long n, uint32_t* __restrict__ tally, RecountAcc& a) {
    const float p = vt_sort_key_score((unsigned)(k >> 32));
    const unsigned lo = (unsigned)k;
    const unsigned y = lo & 1u;
    const unsigned sample = (~lo) >> 1;
    const unsigned pred = (double)p > th ? 1u : 0u;
    a.tp += pred & y;
    a.fp += pred & (y ^ 1u);
    a.bad += !(fabsf(p) <= 3.0e38f) ? 1u : 0u;
    if (pred != y && (long long)sample < n) atomicAdd(&tally[sample], 1u);      // (a key of a valid state never names a sample >= n)
}

__global__ __launch_bounds__(256) void eval_recount_kernel(const unsigned long long* __restrict__ keys, long long pitch, long long n,
                                                           long long chunks, const double* __restrict__ thr,
                                                           uint32_t* __restrict__ tally, uint32_t* __restrict__ acc_counts,
                                                           unsigned long long* __restrict__ acc_bad) {
    __shared__ unsigned s_red[4][3];
    const long long row = blockIdx.x / chunks, c0 = (long long)(blockIdx.x % chunks) * RC_CH;
    const unsigned long long* __restrict__ kb = keys + row * pitch;
    const double th = thr[row];
    const int tid = threadIdx.x;
    const long long lead = (row * pitch) & 1;
    RecountAcc a{0u, 0u, 0u};
    if (c0 == 0 && lead && tid == 0 && n > 0) recount_key(kb[0], th, n, tally, a);
#pragma unroll
    for (int k = 0; k < RC_CH / 512; ++k) {
        const long long col = lead + c0 + 2 * (k * 256 + tid);
        if (col + 1 < n) {
            const ulonglong2 v = *(const ulonglong2*)(kb + col);
            recount_key(v.x, th, n, tally, a);
            recount_key(v.y, th, n, tally, a);
        } else if (col < n) {
            recount_key(kb[col], th, n, tally, a);
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        a.tp += __shfl_down(a.tp, d); a.fp += __shfl_down(a.fp, d); a.bad += __shfl_down(a.bad, d);
    }
    if ((tid & 63) == 0) { s_red[tid >> 6][0] = a.tp; s_red[tid >> 6][1] = a.fp; s_red[tid >> 6][2] = a.bad; }
    __syncthreads();
    if (tid < 3) {
        const unsigned v = s_red[0][tid] + s_red[1][tid] + s_red[2][tid] + s_red[3][tid];
        if (v) {
            if (tid < 2) atomicAdd(&acc_counts[row * 2 + tid], v);
            else atomicAdd(acc_bad, (unsigned long long)v);
        }
    }
}

// tally[sample] = mismatching classes of that sample -> acc_rows = (exactly matching rows, mismatching elements)
__global__ __launch_bounds__(256) void eval_recount_fold_kernel(const uint32_t* __restrict__ tally, long long n,
                                                                unsigned long long* __restrict__ acc_rows) {
    __shared__ unsigned long long s_red[4][2];
    unsigned long long exact = 0, mis = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const uint32_t m = tally[i];
        exact += m == 0;
        mis += m;
    }
    for (int d = 32; d > 0; d >>= 1) { exact += __shfl_down(exact, d); mis += __shfl_down(mis, d); }
    if ((threadIdx.x & 63) == 0) { s_red[threadIdx.x >> 6][0] = exact; s_red[threadIdx.x >> 6][1] = mis; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const unsigned long long v = s_red[0][threadIdx.x] + s_red[1][threadIdx.x] + s_red[2][threadIdx.x] + s_red[3][threadIdx.x];
        if (v) atomicAdd(&acc_rows[threadIdx.x], v);
    }
}

// workspace accumulators -> the caller's outputs (device or pinned host memory: plain stores only)
__global__ __launch_bounds__(256) void eval_recount_emit_kernel(const uint32_t* __restrict__ acc_counts, const unsigned long long* __restrict__ acc_stats,
                                                                long long n2, uint32_t* __restrict__ counts_out,
                                                                unsigned long long* __restrict__ row_stats_out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n2) counts_out[i] = acc_counts[i];
    if (blockIdx.x == 0 && threadIdx.x < 3) row_stats_out[threadIdx.x] = acc_stats[threadIdx.x];
}

#define CK(e) do { hipError_t _e = (e); if (_e != hipSuccess) return _e; } while (0)
#define CKL() CK(hipGetLastError())

hipError_t sort_rows(unsigned long long* keys, long long rows, long long pitch, long long n, hipStream_t s) {
    static std::atomic<unsigned long long> attr_done{0};
    CK(vt_dynamic_smem_once(attr_done, VT_SORT_CH * 8, eval_sort_local_kernel<0>, eval_sort_local_kernel<1>));
    const long long chunks = (n + VT_SORT_CH - 1) / VT_SORT_CH;
    long long top = VT_SORT_CH;
    while (top < n) top <<= 1;
    const long long pair_blocks = (top / 2 + 255) / 256;
    if (rows * chunks > 0x7fffffffLL || (chunks > 1 && rows * pair_blocks > 0x7fffffffLL)) return hipErrorInvalidValue;
    int np = 2;
    while (np < (n < VT_SORT_CH ? n : VT_SORT_CH)) np <<= 1;
    hipLaunchKernelGGL(eval_sort_local_kernel<0>, dim3((unsigned)(rows * chunks)), dim3(1024), (size_t)np * 8, s, keys, pitch, n, (int)chunks); CKL();
    if (chunks == 1) return hipSuccess;
    for (long long k = 2LL * VT_SORT_CH; k <= top; k <<= 1) {
        hipLaunchKernelGGL(eval_sort_global_kernel, dim3((unsigned)(rows * pair_blocks)), dim3(256), 0, s, keys, pitch, n, k, 0LL, 1, pair_blocks); CKL();
        for (long long j = k >> 2; j >= VT_SORT_CH; j >>= 1) {
            hipLaunchKernelGGL(eval_sort_global_kernel, dim3((unsigned)(rows * pair_blocks)), dim3(256), 0, s, keys, pitch, n, k, j, 0, pair_blocks); CKL();
        }
        hipLaunchKernelGGL(eval_sort_local_kernel<1>, dim3((unsigned)(rows * chunks)), dim3(1024), (size_t)VT_SORT_CH * 8, s, keys, pitch, n, (int)chunks); CKL();
    }
    return hipSuccess;
}

}  // namespace

hipError_t vt_eval_launch_reset(void* state, const EvalLayout& l, const EvalThresholds& thr, hipStream_t s) {
    CK(hipMemsetAsync(state, 0, l.head_bytes, s));
    ThrArg a; a.t = thr;
    hipLaunchKernelGGL(eval_init_kernel, dim3(1), dim3(64), 0, s, (double*)((char*)state + l.thr), a); CKL();
    return hipSuccess;
}

hipError_t vt_eval_launch_update(void* state, const EvalLayout& l, const float* probs, const void* labels, int labels_u8, int B, int N,
                                 int T, int t_main, long long capacity, long long n_seen, hipStream_t s) {
    char* st = (char*)state;
    const double* thr = (const double*)(st + l.thr);
    uint32_t* counts = (uint32_t*)(st + l.counts);
    uint32_t* support = (uint32_t*)(st + l.support);
    unsigned long long* row_stats = (unsigned long long*)(st + l.row_stats);
    uint32_t* row_scratch = (uint32_t*)(st + l.row_scratch);
    unsigned long long* keys = capacity > 0 ? (unsigned long long*)(st + l.keys) : nullptr;
    const dim3 grid((N + EV_TC - 1) / EV_TC);
    if (labels_u8)
        hipLaunchKernelGGL(eval_accumulate_kernel<unsigned char>, grid, dim3(256), 0, s, probs, (const unsigned char*)labels, B, N, T, t_main, thr,
                           counts, support, row_stats, row_scratch, keys, capacity, n_seen);
    else
        hipLaunchKernelGGL(eval_accumulate_kernel<float>, grid, dim3(256), 0, s, probs, (const float*)labels, B, N, T, t_main, thr, counts,
                           support, row_stats, row_scratch, keys, capacity, n_seen);
    CKL();
    hipLaunchKernelGGL(eval_fold_rows_kernel, dim3(1), dim3(256), 0, s, row_scratch, B, row_stats); CKL();
    return hipSuccess;
}

hipError_t vt_eval_launch_ap(void* state, const EvalLayout& l, int N, long long capacity, long long n_seen, double* ap, double* micro_ap,
                             unsigned long long* flat, hipStream_t s) {
    unsigned long long* keys = (unsigned long long*)((char*)state + l.keys);
    CK(sort_rows(keys, N, capacity, n_seen, s));
    hipLaunchKernelGGL(eval_ap_kernel, dim3(N), dim3(1024), 0, s, keys, capacity, n_seen, ap); CKL();
    if (micro_ap) {
        const long long total = n_seen * N;
        hipLaunchKernelGGL(eval_flatten_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, keys, capacity, n_seen, total, flat); CKL();
        CK(sort_rows(flat, 1, total, total, s));
        hipLaunchKernelGGL(eval_ap_kernel, dim3(1), dim3(1024), 0, s, flat, total, total, micro_ap); CKL();
    }
    return hipSuccess;
}

namespace {
hipError_t launch_merge_keys(const EvalMergeArg& a, size_t keys_at, unsigned long long* dst, long long dst_pitch, int N, int vec, hipStream_t s) {
    long long widest = 0;
    for (int w = 0; w < a.W; ++w) widest = a.src[w].fill > widest ? a.src[w].fill : widest;
    if (widest == 0) return hipSuccess;
    const long long chunks = (widest + MERGE_CH - 1) / MERGE_CH;
    if ((long long)N * chunks > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((long long)N * chunks), (unsigned)a.W);
    if (vec) hipLaunchKernelGGL(eval_merge_keys_kernel<2>, grid, dim3(256), 0, s, a, keys_at, dst, dst_pitch, chunks);
    else hipLaunchKernelGGL(eval_merge_keys_kernel<1>, grid, dim3(256), 0, s, a, keys_at, dst, dst_pitch, chunks);
    CKL();
    return hipSuccess;
}
}  // namespace

hipError_t vt_eval_launch_export(const void* state, const EvalLayout& l, void* out, const EvalLayout& lo, int N, long long capacity,
                                 long long n_seen, long long out_capacity, int vec, hipStream_t s) {
    CK(hipMemcpyAsync(out, state, l.head_bytes, hipMemcpyDeviceToDevice, s));
    CK(hipMemsetAsync((char*)out + lo.row_scratch, 0, sizeof(uint32_t) * VT_EVAL_MAX_B, s));
    if (out_capacity <= 0) return hipSuccess;
    EvalMergeArg a;
    a.W = 1;
    a.src[0] = EvalMergeSrc{(const char*)state, capacity, n_seen, out_capacity, 0};
    CK(launch_merge_keys(a, l.keys, (unsigned long long*)((char*)out + lo.keys), out_capacity, N, vec, s));
    const size_t used = lo.keys + sizeof(uint64_t) * (size_t)N * (size_t)out_capacity;
    if (lo.total > used) CK(hipMemsetAsync((char*)out + used, 0, lo.total - used, s));    // the section's alignment tail
    return hipSuccess;
}

hipError_t vt_eval_launch_merge(void* dst, const EvalLayout& l, int N, long long dst_capacity, const EvalMergeArg& a, int vec, hipStream_t s) {
    const long long quads = (long long)((l.head_bytes - l.support) / 16);
    hipLaunchKernelGGL(eval_merge_head_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, s, a, (char*)dst, l.support, l.row_stats, quads); CKL();
    if (dst_capacity > 0) CK(launch_merge_keys(a, l.keys, (unsigned long long*)((char*)dst + l.keys), dst_capacity, N, vec, s));
    return hipSuccess;
}

size_t vt_eval_recount_ws_bytes(int N, long long n_seen) {
    return vt_eval_align(sizeof(uint64_t) * 3) + vt_eval_align(sizeof(uint32_t) * 2 * (size_t)N) + vt_eval_align(sizeof(uint32_t) * (size_t)n_seen);
}

hipError_t vt_eval_launch_recount(const void* state, const EvalLayout& l, int N, long long capacity, long long n_seen, const double* thr,
                                  uint32_t* counts_out, unsigned long long* row_stats_out, void* ws, hipStream_t s) {
    // workspace: stats uint64 [3] = (exact rows, mismatching elements, non-finite) | counts uint32 [N][2] | tally uint32 [n_seen]
    char* w = (char*)ws;
    unsigned long long* acc_stats = (unsigned long long*)w;
    uint32_t* acc_counts = (uint32_t*)(w + vt_eval_align(sizeof(uint64_t) * 3));
    uint32_t* tally = acc_counts + vt_eval_align(sizeof(uint32_t) * 2 * (size_t)N) / sizeof(uint32_t);
    CK(hipMemsetAsync(ws, 0, vt_eval_recount_ws_bytes(N, n_seen), s));
    if (n_seen > 0) {
        const long long chunks = (n_seen + RC_CH - 1) / RC_CH;
        if ((long long)N * chunks > 0x7fffffffLL) return hipErrorInvalidValue;
        const unsigned long long* keys = (const unsigned long long*)((const char*)state + l.keys);
        hipLaunchKernelGGL(eval_recount_kernel, dim3((unsigned)((long long)N * chunks)), dim3(256), 0, s, keys, capacity, n_seen, chunks, thr, tally,
                           acc_counts, acc_stats + 2); CKL();
        long long fold_blocks = (n_seen + 255) / 256;
        if (fold_blocks > 1024) fold_blocks = 1024;
        hipLaunchKernelGGL(eval_recount_fold_kernel, dim3((unsigned)fold_blocks), dim3(256), 0, s, tally, n_seen, acc_stats); CKL();
    }
    const long long n2 = 2LL * N;
    hipLaunchKernelGGL(eval_recount_emit_kernel, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, s, acc_counts, acc_stats, n2, counts_out,
                       row_stats_out); CKL();
    return hipSuccess;
}
