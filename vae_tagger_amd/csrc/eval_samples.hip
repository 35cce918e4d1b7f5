// Per-image (example-based) precision / recall / F1 on the device: what the reference's batch_inference_test.py computes per picture
// (batch_inference_test.py:87-104) -- precision_i = |true & pred| / |pred|, recall_i = |true & pred| / |true|, F1_i, exact match --
// accumulated in one caller-owned state block that is fed the [B][N] probabilities batch by batch in stream order.  The evaluator of
// eval_metrics.hip reduces the same matrix along the samples (per class); this unit reduces it along the classes (per image):
//   * vt_sample_update: one workgroup per row, one pass over the row with loads coalesced over N, every threshold decided from the same
//     load (staged in LDS; a thread owns one threshold); a row's tallies are integers combined through LDS -- no atomics, one launch;
//   * vt_sample_from_keys: the same tallies under ONE THRESHOLD PER CLASS from an evaluator's key store (a read-only pass over the keys;
//     the sample is the one the key names, so ranked rows and merged states count the same), through integer vector atomics;
//   * vt_sample_finish: per threshold one workgroup turns (tp, predicted, true) into fp64 P, R, F1 and sums them in image order, the
//     order of the reference's loop: no floating-point atomics, the same bits every run -- and the host route's bits.
#include <math.h>
#include <string.h>

#include "vt_context.h"
#include "vt_samples.h"
#include "vt_sort_network.h"

using namespace vt;

namespace {

struct SampleThresholds { double v[VT_SAMPLE_MAX_T]; };

__global__ __launch_bounds__(64) void sample_init_kernel(double* __restrict__ thr, unsigned long long* __restrict__ header, SampleThresholds a,
                                                         int rule, int T) {
    if (threadIdx.x < VT_SAMPLE_MAX_T) thr[threadIdx.x] = a.v[threadIdx.x];
    if (threadIdx.x == 0) { header[0] = (unsigned long long)rule; header[1] = (unsigned long long)T; }
}

// One workgroup per row b of the batch, one pass over the row.  Per pass thread j loads element j0 + j (a wave reads 256 contiguous
// bytes) and stages (probability, label) in LDS; the tail of the row is masked, not padded: an out-of-row slot holds NaN, which fails
// both > and >=, and label 0.  The counting step turns the work round: thread (t, g) owns threshold t = tid & 31 and walks the staged
// elements g, g + 8, ... (the 32 lanes of a threshold group read one LDS address: a broadcast), so a thread keeps ONE threshold and two
// counters in registers whatever T is, and the eight groups' counters are added through LDS at the end -- integers, no atomics.
constexpr int SM_G = 256 / VT_SAMPLE_MAX_T;        // element groups: 8

template <typename L>
__global__ __launch_bounds__(256) void sample_rows_kernel(const float* __restrict__ probs, const L* __restrict__ labels,
                                                          const uint32_t* __restrict__ true_extra, int N, int T,
                                                          const double* __restrict__ thr, const unsigned long long* __restrict__ header,
                                                          uint32_t* __restrict__ nonfinite, uint32_t* __restrict__ true_out,
                                                          uint32_t* __restrict__ rows, long long n_seen) {
    __shared__ uint2 s_e[256];                               // (probability bits, label) of the pass
    __shared__ uint32_t s_cnt[SM_G][2 * VT_SAMPLE_MAX_T];
    __shared__ uint32_t s_pb[4][2];
    const int b = blockIdx.x, tid = threadIdx.x, t = tid & (VT_SAMPLE_MAX_T - 1), g = tid / VT_SAMPLE_MAX_T;
    const bool ge = header[0] == (unsigned long long)VT_SAMPLE_GE;
    const float* __restrict__ prow = probs + (long long)b * N;
    const L* __restrict__ lrow = labels + (long long)b * N;
    const double th = thr[t];                                // (NaN beyond T: never reached under either rule)
    uint32_t tp = 0, pr = 0, pos = 0, bad = 0;
    for (int j0 = 0; j0 < N; j0 += 256) {
        const int j = j0 + tid;
        const bool in = j < N;
        const float p = in ? prow[j] : __uint_as_float(0x7fc00000u);
        const uint32_t y = (in && lrow[j] > 0) ? 1u : 0u;
        pos += y;
        bad += (in && !(fabsf(p) <= 3.0e38f)) ? 1u : 0u;
        s_e[tid] = make_uint2(__float_as_uint(p), y);
        __syncthreads();
        const int n = min(256, N - j0);
        for (int e = g; e < n; e += SM_G) {
            const uint2 v = s_e[e];
            const double dp = (double)__uint_as_float(v.x);
            const uint32_t pd = (ge ? dp >= th : dp > th) ? 1u : 0u;
            pr += pd;
            tp += pd & v.y;
        }
        __syncthreads();
    }
    for (int d = 32; d > 0; d >>= 1) { pos += __shfl_down(pos, d); bad += __shfl_down(bad, d); }
    s_cnt[g][2 * t] = tp; s_cnt[g][2 * t + 1] = pr;
    if ((tid & 63) == 0) { s_pb[tid >> 6][0] = pos; s_pb[tid >> 6][1] = bad; }
    __syncthreads();
    const long long s = n_seen + b;
    if (tid < 2 * T) {
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < SM_G; ++k) v += s_cnt[k][tid];
        rows[s * 2 * T + tid] = v;
    }
    if (tid == 64) true_out[s] = s_pb[0][0] + s_pb[1][0] + s_pb[2][0] + s_pb[3][0] + (true_extra ? true_extra[b] : 0u);
    if (tid == 65) {
        const uint32_t v = s_pb[0][1] + s_pb[1][1] + s_pb[2][1] + s_pb[3][1];
        if (v) nonfinite[b] += v;                            // slot b belongs to row b's workgroup in every launch; launches are in stream order
    }
}

// ---- the same tallies from an evaluator's key store, one threshold per class -----------------------------------------------------
// true[i] <- true_extra[i] (or 0) for the n samples; the rows are zeroed by a memset
__global__ __launch_bounds__(256) void sample_seed_true_kernel(uint32_t* __restrict__ true_out, const uint32_t* __restrict__ true_extra, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) true_out[i] = true_extra ? true_extra[i] : 0u;
}

// The walk of eval_recount_kernel: blockIdx.x = row * chunks + chunk, SK_CH keys of one class row per workgroup, 16 B per lane on the
// 16-B aligned part of the row.  Per key the probability comes back from the high word (vt_sort_key_score), label and sample index from
// the low word.  A positive label adds 1 to true[sample]; a prediction adds (tp, 1) to rows[sample] as ONE 64-bit integer atomic (tp is
// the low word and never carries: it stays below N).  In a store that has not been ranked consecutive lanes name consecutive samples.
constexpr int SK_CH = 4096;

__device__ __forceinline__ void sample_key(unsigned long long k, double th, bool ge, long long n, uint32_t* __restrict__ true_out,
                                           unsigned long long* __restrict__ rows, unsigned& bad) {
    const float p = vt_sort_key_score((unsigned)(k >> 32));
    const unsigned lo = (unsigned)k;
    const unsigned y = lo & 1u;
    const unsigned sample = (~lo) >> 1;
    const double dp = (double)p;
    const bool pred = ge ? dp >= th : dp > th;
    bad += !(fabsf(p) <= 3.0e38f) ? 1u : 0u;
    if ((long long)sample < n) {                             // (a key of a valid state never names a sample >= n)
        if (y) atomicAdd(&true_out[sample], 1u);
        if (pred) atomicAdd(&rows[sample], (1ull << 32) | (unsigned long long)y);
    }
}

__global__ __launch_bounds__(256) void sample_from_keys_kernel(const unsigned long long* __restrict__ keys, long long pitch, long long n,
                                                               long long chunks, const double* __restrict__ thr, int ge,
                                                               uint32_t* __restrict__ true_out, unsigned long long* __restrict__ rows,
                                                               uint32_t* __restrict__ nonfinite) {
    __shared__ unsigned s_red[4];
    const long long row = blockIdx.x / chunks, c0 = (long long)(blockIdx.x % chunks) * SK_CH;
    const unsigned long long* __restrict__ kb = keys + row * pitch;
    const double th = thr[row];
    const int tid = threadIdx.x;
    const long long lead = (row * pitch) & 1;
    unsigned bad = 0;
    if (c0 == 0 && lead && tid == 0 && n > 0) sample_key(kb[0], th, ge != 0, n, true_out, rows, bad);
#pragma unroll
    for (int k = 0; k < SK_CH / 512; ++k) {
        const long long col = lead + c0 + 2 * (k * 256 + tid);
        if (col + 1 < n) {
            const ulonglong2 v = *(const ulonglong2*)(kb + col);
            sample_key(v.x, th, ge != 0, n, true_out, rows, bad);
            sample_key(v.y, th, ge != 0, n, true_out, rows, bad);
        } else if (col < n) {
            sample_key(kb[col], th, ge != 0, n, true_out, rows, bad);
        }
    }
    for (int d = 32; d > 0; d >>= 1) bad += __shfl_down(bad, d);
    if ((tid & 63) == 0) s_red[tid >> 6] = bad;
    __syncthreads();
    if (tid == 0) {
        const unsigned v = s_red[0] + s_red[1] + s_red[2] + s_red[3];
        if (v) atomicAdd(&nonfinite[blockIdx.x % VT_SAMPLE_MAX_B], v);      // (a workgroup adds at most SK_CH: a slot cannot wrap below 2^44 keys)
    }
}

// ---- finish: one workgroup per threshold ------------------------------------------------------------------------------------------
// The reference's conventions (batch_inference_test.py:87-104): precision 0 when nothing is predicted, recall 1 when the image has no
// true tag, F1 = 2 P R / (P + R) evaluated as Python does, ((2 P) R) / (P + R), or 0 when P + R = 0; exact match: tp == predicted == true.
// The three sums run in IMAGE ORDER, the order of the reference's loop and of sample_metrics_host: 1024 images at a time are evaluated
// by the workgroup and staged in LDS, then one thread per quantity (in three different waves) adds its 1024 values one after the other.
// The result is therefore the host's, bit for bit, at the price of a dependent chain of n fp64 adds (about 4 us per 1024 images).
__global__ __launch_bounds__(1024) void sample_finish_kernel(const uint32_t* __restrict__ true_in, const uint32_t* __restrict__ rows,
                                                             const uint32_t* __restrict__ nonfinite, int T, long long n,
                                                             double* __restrict__ out_sums, unsigned long long* __restrict__ out_counts,
                                                             unsigned long long* __restrict__ out_once) {
#pragma clang fp contract(off)                // every value rounds as the host's does (the Makefile contracts by default)
    __shared__ double s_v[3][1024];
    __shared__ unsigned long long s_u[16][4];
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int q = tid >> 6;                   // threads 0, 64, 128 own the sums of P, R, F1
    double acc = 0.0;
    unsigned long long exact = 0, nopred = 0, notrue = 0, bad = 0;
    for (long long base = 0; base < n; base += 1024) {
        const long long i = base + tid;
        if (i < n) {
            const uint32_t tr = true_in[i];
            const uint32_t tp = rows[(i * T + t) * 2], pr = rows[(i * T + t) * 2 + 1];
            const double P = pr > 0 ? (double)tp / (double)pr : 0.0;
            const double R = tr > 0 ? (double)tp / (double)tr : 1.0;
            const double F = P + R > 0.0 ? 2.0 * P * R / (P + R) : 0.0;
            s_v[0][tid] = P; s_v[1][tid] = R; s_v[2][tid] = F;
            exact += (tp == pr && pr == tr) ? 1u : 0u;
            nopred += pr == 0;
            notrue += tr == 0;
        }
        __syncthreads();
        if (lane == 0 && q < 3) {
            const int cnt = n - base < 1024 ? (int)(n - base) : 1024;
            for (int k = 0; k < cnt; ++k) acc += s_v[q][k];
        }
        __syncthreads();
    }
    if (lane == 0 && q < 3) out_sums[t * 3 + q] = acc;
    if (t == 0)
        for (int i = tid; i < VT_SAMPLE_MAX_B; i += 1024) bad += nonfinite[i];
    for (int d = 32; d > 0; d >>= 1) {
        exact += __shfl_down(exact, d); nopred += __shfl_down(nopred, d); notrue += __shfl_down(notrue, d); bad += __shfl_down(bad, d);
    }
    if (lane == 0) { s_u[w][0] = exact; s_u[w][1] = nopred; s_u[w][2] = notrue; s_u[w][3] = bad; }
    __syncthreads();
    if (tid < 4) {
        unsigned long long c = 0;
        for (int i = 0; i < 16; ++i) c += s_u[i][tid];
        if (tid < 2) out_counts[t * 2 + tid] = c;
        else if (t == 0) out_once[tid - 2] = c;
    }
}

bool sample_misaligned(const void* p) { return ((uintptr_t)p & (ALIGN - 1)) != 0; }
bool sample_dims_ok(int T, long long capacity) {
    return T > 0 && T <= VT_SAMPLE_MAX_T && capacity > 0 && capacity <= VT_EVAL_MAX_N_SEEN;
}
int sample_check_state(vt_context* c, const char* who, const void* state, size_t state_bytes, int T, long long capacity) {
    if (!sample_dims_ok(T, capacity))
        return c->fail(VT_ERR_INVALID, "%s: bad dimensions (T = %d of at most %d, capacity = %lld)", who, T, VT_SAMPLE_MAX_T, capacity);
    if (!state || sample_misaligned(state)) return c->fail(VT_ERR_INVALID, "%s: state is null or not 256-B aligned", who);
    const size_t need = vt_sample_layout(T, capacity).total;
    if (state_bytes < need) return c->fail(VT_ERR_WORKSPACE, "%s: state holds %zu bytes, %zu needed", who, state_bytes, need);
    return VT_OK;
}
bool sample_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

#define SCKL(c, what) HIPCK(c, hipGetLastError(), what)

}  // namespace

extern "C" {

size_t vt_sample_state_bytes(int T, long long capacity) { return sample_dims_ok(T, capacity) ? vt_sample_layout(T, capacity).total : 0; }

int vt_sample_reset(vt_context* c, void* state, size_t state_bytes, int T, const double* thresholds, int rule, long long capacity, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (int r = sample_check_state(c, "vt_sample_reset", state, state_bytes, T, capacity)) return r;
    if (!thresholds || (rule != VT_SAMPLE_GT && rule != VT_SAMPLE_GE))
        return c->fail(VT_ERR_INVALID, "vt_sample_reset: null thresholds or rule = %d (VT_SAMPLE_GT or VT_SAMPLE_GE)", rule);
    const SampleLayout l = vt_sample_layout(T, capacity);
    hipStream_t s = (hipStream_t)stream;
    char* st = (char*)state;
    SampleThresholds th;
    for (int i = 0; i < VT_SAMPLE_MAX_T; ++i) th.v[i] = i < T ? thresholds[i] : NAN;       // (NaN: never reached under either rule)
    HIPCK(c, hipMemsetAsync(state, 0, l.head_bytes, s), "sample_reset clear");
    hipLaunchKernelGGL(sample_init_kernel, dim3(1), dim3(64), 0, s, (double*)(st + l.thr), (unsigned long long*)(st + l.totals), th, rule, T);
    SCKL(c, "sample_reset init");
    return VT_OK;
}

int vt_sample_update(vt_context* c, void* state, size_t state_bytes, int T, long long capacity, const float* probs, const void* labels,
                     int labels_dtype, const uint32_t* true_extra, int B, int N, long long n_seen, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (int r = sample_check_state(c, "vt_sample_update", state, state_bytes, T, capacity)) return r;
    if (!probs || !labels || ((uintptr_t)probs & 3) || (labels_dtype == VT_F32 && ((uintptr_t)labels & 3)) ||
        (labels_dtype != VT_F32 && labels_dtype != VT_U8) || ((uintptr_t)true_extra & 3))
        return c->fail(VT_ERR_INVALID, "vt_sample_update: null or misaligned input, or labels neither VT_F32 nor VT_U8");
    if (N <= 0 || B <= 0 || B > VT_SAMPLE_MAX_B || n_seen < 0 || n_seen + B > capacity)
        return c->fail(VT_ERR_INVALID, "vt_sample_update: N = %d, B = %d outside [1, %d] or n_seen + B = %lld exceeds the capacity %lld", N, B,
                       VT_SAMPLE_MAX_B, n_seen + B, capacity);
    const SampleLayout l = vt_sample_layout(T, capacity);
    hipStream_t s = (hipStream_t)stream;
    char* st = (char*)state;
    const double* thr = (const double*)(st + l.thr);
    const unsigned long long* header = (const unsigned long long*)(st + l.totals);
    uint32_t* nonfinite = (uint32_t*)(st + l.nonfinite);
    uint32_t* true_out = (uint32_t*)(st + l.true_at);
    uint32_t* rows = (uint32_t*)(st + l.rows);
    if (labels_dtype == VT_U8)
        hipLaunchKernelGGL(sample_rows_kernel<unsigned char>, dim3(B), dim3(256), 0, s, probs, (const unsigned char*)labels, true_extra, N, T, thr,
                           header, nonfinite, true_out, rows, n_seen);
    else
        hipLaunchKernelGGL(sample_rows_kernel<float>, dim3(B), dim3(256), 0, s, probs, (const float*)labels, true_extra, N, T, thr, header,
                           nonfinite, true_out, rows, n_seen);
    SCKL(c, "sample_update");
    return VT_OK;
}

int vt_sample_from_keys(vt_context* c, const void* eval_state, size_t eval_state_bytes, int N, int T_eval, long long capacity, long long n_seen,
                        const double* class_thresholds, int rule, const uint32_t* true_extra, void* sample_state, size_t sample_state_bytes,
                        long long sample_capacity, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (N <= 0 || T_eval <= 0 || T_eval > VT_EVAL_MAX_T || capacity <= 0 || capacity > VT_EVAL_MAX_N_SEEN ||
        (unsigned long long)N * (unsigned long long)capacity >= (1ull << 40))
        return c->fail(VT_ERR_INVALID, "vt_sample_from_keys: bad evaluator dimensions (N = %d, T = %d, capacity = %lld: a key store is needed)", N,
                       T_eval, capacity);
    if (!eval_state || sample_misaligned(eval_state)) return c->fail(VT_ERR_INVALID, "vt_sample_from_keys: eval_state is null or not 256-B aligned");
    const EvalLayout le = vt_eval_layout(N, T_eval, capacity);
    if (eval_state_bytes < le.total)
        return c->fail(VT_ERR_WORKSPACE, "vt_sample_from_keys: eval_state holds %zu bytes, %zu needed", eval_state_bytes, le.total);
    if (int r = sample_check_state(c, "vt_sample_from_keys", sample_state, sample_state_bytes, 1, sample_capacity)) return r;
    if (n_seen < 0 || n_seen > capacity || n_seen > sample_capacity)
        return c->fail(VT_ERR_INVALID, "vt_sample_from_keys: n_seen = %lld outside [0, min(capacity = %lld, sample capacity = %lld)]", n_seen, capacity,
                       sample_capacity);
    if (!class_thresholds || ((uintptr_t)class_thresholds & 7) || ((uintptr_t)true_extra & 3) ||
        (rule != VT_SAMPLE_GT && rule != VT_SAMPLE_GE))
        return c->fail(VT_ERR_INVALID, "vt_sample_from_keys: class_thresholds null or misaligned, true_extra misaligned, or rule = %d", rule);
    const SampleLayout l = vt_sample_layout(1, sample_capacity);
    if (sample_overlap(eval_state, le.total, sample_state, l.total)) return c->fail(VT_ERR_INVALID, "vt_sample_from_keys: the two states overlap");
    const long long chunks = (n_seen + SK_CH - 1) / SK_CH;
    if ((long long)N * chunks > 0x7fffffffLL) return c->fail(VT_ERR_INVALID, "vt_sample_from_keys: N x n_seen too large for one launch");
    hipStream_t s = (hipStream_t)stream;
    char* st = (char*)sample_state;
    SampleThresholds th;
    for (int i = 0; i < VT_SAMPLE_MAX_T; ++i) th.v[i] = NAN;                               // (one threshold per class: the table is unused)
    HIPCK(c, hipMemsetAsync(st, 0, l.head_bytes, s), "sample_from_keys clear");
    hipLaunchKernelGGL(sample_init_kernel, dim3(1), dim3(64), 0, s, (double*)(st + l.thr), (unsigned long long*)(st + l.totals), th, rule, 1);
    SCKL(c, "sample_from_keys init");
    if (n_seen == 0) return VT_OK;
    uint32_t* true_out = (uint32_t*)(st + l.true_at);
    HIPCK(c, hipMemsetAsync(st + l.rows, 0, sizeof(uint32_t) * 2 * (size_t)n_seen, s), "sample_from_keys rows");
    hipLaunchKernelGGL(sample_seed_true_kernel, dim3((unsigned)((n_seen + 255) / 256)), dim3(256), 0, s, true_out, true_extra, n_seen);
    SCKL(c, "sample_from_keys seed");
    hipLaunchKernelGGL(sample_from_keys_kernel, dim3((unsigned)((long long)N * chunks)), dim3(256), 0, s,
                       (const unsigned long long*)((const char*)eval_state + le.keys), capacity, n_seen, chunks, class_thresholds,
                       rule == VT_SAMPLE_GE ? 1 : 0, true_out, (unsigned long long*)(st + l.rows), (uint32_t*)(st + l.nonfinite));
    SCKL(c, "sample_from_keys");
    return VT_OK;
}

size_t vt_sample_finish_bytes(int T) { return T > 0 && T <= VT_SAMPLE_MAX_T ? vt_sample_out_bytes(T) : 0; }

int vt_sample_finish(vt_context* c, const void* state, size_t state_bytes, int T, long long capacity, long long n_seen, void* out,
                     size_t out_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (int r = sample_check_state(c, "vt_sample_finish", state, state_bytes, T, capacity)) return r;
    if (n_seen < 0 || n_seen > capacity) return c->fail(VT_ERR_INVALID, "vt_sample_finish: n_seen = %lld outside [0, capacity = %lld]", n_seen, capacity);
    if (!out || ((uintptr_t)out & 7)) return c->fail(VT_ERR_INVALID, "vt_sample_finish: out is null or misaligned");
    const size_t need = vt_sample_out_bytes(T);
    if (out_bytes < need) return c->fail(VT_ERR_WORKSPACE, "vt_sample_finish: out holds %zu bytes, %zu needed", out_bytes, need);
    const SampleLayout l = vt_sample_layout(T, capacity);
    if (sample_overlap(state, l.total, out, need)) return c->fail(VT_ERR_INVALID, "vt_sample_finish: out overlaps the state");
    const char* st = (const char*)state;
    double* sums = (double*)out;
    unsigned long long* counts = (unsigned long long*)(sums + 3 * (size_t)T);
    hipLaunchKernelGGL(sample_finish_kernel, dim3(T), dim3(1024), 0, (hipStream_t)stream, (const uint32_t*)(st + l.true_at),
                       (const uint32_t*)(st + l.rows), (const uint32_t*)(st + l.nonfinite), T, n_seen, sums, counts, counts + 2 * (size_t)T);
    SCKL(c, "sample_finish");
    return VT_OK;
}

int vt_sample_read_rows(vt_context* c, const void* state, size_t state_bytes, int T, long long capacity, long long n_seen, uint32_t* true_out,
                        size_t true_bytes, uint32_t* rows_out, size_t rows_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (int r = sample_check_state(c, "vt_sample_read_rows", state, state_bytes, T, capacity)) return r;
    if (n_seen < 0 || n_seen > capacity) return c->fail(VT_ERR_INVALID, "vt_sample_read_rows: n_seen = %lld outside [0, capacity = %lld]", n_seen, capacity);
    if (!true_out || !rows_out || ((uintptr_t)true_out & 3) || ((uintptr_t)rows_out & 3))
        return c->fail(VT_ERR_INVALID, "vt_sample_read_rows: an output is null or misaligned");
    const size_t nt = sizeof(uint32_t) * (size_t)n_seen, nr = nt * 2 * (size_t)T;
    if (true_bytes < nt || rows_bytes < nr)
        return c->fail(VT_ERR_WORKSPACE, "vt_sample_read_rows: outputs hold %zu / %zu bytes, %zu / %zu needed", true_bytes, rows_bytes, nt, nr);
    if (n_seen == 0) return VT_OK;
    const SampleLayout l = vt_sample_layout(T, capacity);
    const char* st = (const char*)state;
    hipStream_t s = (hipStream_t)stream;
    HIPCK(c, hipMemcpyAsync(true_out, st + l.true_at, nt, hipMemcpyDefault, s), "sample_read true");
    HIPCK(c, hipMemcpyAsync(rows_out, st + l.rows, nr, hipMemcpyDefault, s), "sample_read rows");
    return VT_OK;
}

}  // extern "C"
