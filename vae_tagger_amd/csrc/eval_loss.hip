// Streaming validation loss on the device: what train_decoder.py's validation loop (train_decoder.py:218-241) computes per batch with
// nn.BCEWithLogitsLoss, FocalLoss or ClassBalancedLoss (improved_losses.py:39-72), accumulated in one caller-owned state block that is
// fed the decoder's LOGITS batch by batch in stream order.  Forward only.  Everything is evaluated in fp64 from the fp32 inputs:
//   bce   = max(x, 0) - x y + log1p(exp(-|x|))
//   focal = alpha (1 - exp(-bce))^gamma bce
// No floating-point atomics and no atomics at all: per update every class is owned by one thread, the rows of a class are walked by four
// lanes in a fixed interleave and combined in lane order, the 64 classes of a workgroup are combined by a wave tree, and a second, one-wave
// launch adds the workgroups' partials in workgroup order -- the order of every sum is a function of (B, N) alone, so the state after a
// given call sequence is the same bits on every run.
#include <math.h>
#include <string.h>

#include "vt_context.h"
#include "vt_loss.h"

using namespace vt;

namespace {

constexpr int LS_RL = 4;                    // row lanes: lane g of a class walks rows g, g + 4, ...
constexpr int LS_WCHUNK = 256;              // class weights travel as kernel arguments, this many per launch

struct LossWeightChunk { double v[LS_WCHUNK]; };
struct LossMergeArg { const char* src[VT_EVAL_MAX_MERGE]; int W; };

__global__ __launch_bounds__(64) void loss_init_kernel(double* __restrict__ params, double alpha, double gamma, unsigned long long has_weights,
                                                       unsigned long long N) {
    if (threadIdx.x == 0) {
        params[0] = alpha; params[1] = gamma;
        ((unsigned long long*)params)[2] = has_weights; ((unsigned long long*)params)[3] = N;
    }
}

__global__ __launch_bounds__(256) void loss_fill_weights_kernel(double* __restrict__ w, int N) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N) w[i] = 1.0;
}

__global__ __launch_bounds__(LS_WCHUNK) void loss_set_weights_kernel(double* __restrict__ w, int base, int N, LossWeightChunk c) {
    const int i = base + threadIdx.x;
    if (i < N) w[i] = c.v[threadIdx.x];
}

__device__ __forceinline__ double label_value(float y) { return (double)y; }                 // VT_F32: used as its value
__device__ __forceinline__ double label_value(unsigned char y) { return y ? 1.0 : 0.0; }     // VT_U8: 0 or 1

// (1 - pt)^gamma with the results of pow(): gamma == 0 gives 1 whatever the base, NaN included
__device__ __forceinline__ double focal_factor(double base, double gamma) {
    if (gamma == 2.0) return base * base;
    if (gamma == 0.0) return 1.0;
    if (gamma == 1.0) return base;
    return pow(base, gamma);
}

// Workgroup = 64 classes x 4 row lanes.  sums[class] is read and written by one thread; partials[blockIdx.x] by one thread.
template <typename L>
__global__ __launch_bounds__(256) void loss_accumulate_kernel(const float* __restrict__ logits, const L* __restrict__ labels, int B, int N,
                                                              const double* __restrict__ params, const double* __restrict__ weights,
                                                              double* __restrict__ sums, double* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ double s_part[LS_RL][VT_LOSS_TC][2];
    __shared__ unsigned s_bad[LS_RL];
    const int tid = threadIdx.x, c = tid & 63, g = tid >> 6;
    const int cls = blockIdx.x * VT_LOSS_TC + c;
    const bool valid = cls < N;
    const double alpha = params[0], gamma = params[1];
    double sb = 0.0, sf = 0.0;
    unsigned bad = 0;
    if (valid) {
        for (int r = g; r < B; r += LS_RL) {
            const long long o = (long long)r * N + cls;
            const float xf = logits[o];
            const double x = (double)xf, y = label_value(labels[o]);
            const double bce = fmax(x, 0.0) - x * y + log1p(exp(-fabs(x)));
            const double f = alpha * focal_factor(1.0 - exp(-bce), gamma) * bce;
            sb += bce; sf += f;
            bad += !(fabsf(xf) <= 3.0e38f) ? 1u : 0u;
        }
    }
    s_part[g][c][0] = sb; s_part[g][c][1] = sf;
    for (int d = 32; d > 0; d >>= 1) bad += __shfl_down(bad, d);
    if (c == 0) s_bad[g] = bad;
    __syncthreads();
    if (g != 0) return;
    double tb = s_part[0][c][0], tf = s_part[0][c][1];
#pragma unroll
    for (int k = 1; k < LS_RL; ++k) { tb += s_part[k][c][0]; tf += s_part[k][c][1]; }
    double tw = 0.0;
    if (valid) {
        sums[2 * (long long)cls] += tb; sums[2 * (long long)cls + 1] += tf;
        tw = weights[cls] * tb;
    }
    for (int d = 32; d > 0; d >>= 1) { tb += __shfl_down(tb, d); tf += __shfl_down(tf, d); tw += __shfl_down(tw, d); }
    if (c == 0) {
        double* p = partials + 4 * (long long)blockIdx.x;
        p[0] = tb; p[1] = tf; p[2] = tw;
        ((unsigned long long*)p)[3] = (unsigned long long)s_bad[0] + s_bad[1] + s_bad[2] + s_bad[3];
    }
}

// one wave: the workgroups' partials in workgroup order (lane l takes l, l + 64, ...; then the wave tree) -> the per-batch means and counters
__global__ __launch_bounds__(64) void loss_fold_kernel(const double* __restrict__ partials, int groups, int B, int N, double* __restrict__ totals) {
#pragma clang fp contract(off)
    const int l = threadIdx.x;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    unsigned long long bad = 0;
    for (int i = l; i < groups; i += 64) {
        const double* p = partials + 4 * (long long)i;
        a0 += p[0]; a1 += p[1]; a2 += p[2];
        bad += ((const unsigned long long*)p)[3];
    }
    for (int d = 32; d > 0; d >>= 1) {
        a0 += __shfl_down(a0, d); a1 += __shfl_down(a1, d); a2 += __shfl_down(a2, d); bad += __shfl_down(bad, d);
    }
    if (l == 0) {
        const double denom = (double)B * (double)N;
        totals[0] += a0 / denom; totals[1] += a1 / denom; totals[2] += a2 / denom;
        unsigned long long* u = (unsigned long long*)totals + 3;
        u[0] += 1ull; u[1] += (unsigned long long)B * (unsigned long long)N; u[2] += bad;
    }
}

// dst += source 0, then source 1, ...: every element is owned by one thread
__global__ __launch_bounds__(256) void loss_merge_kernel(LossMergeArg a, char* __restrict__ dst, size_t sums_at, size_t totals_at, long long n2) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n2) {
        double* d = (double*)(dst + sums_at) + i;
        double v = *d;
        for (int w = 0; w < a.W; ++w) v += ((const double*)(a.src[w] + sums_at))[i];
        *d = v;
    }
    if (blockIdx.x == 0 && threadIdx.x < 3) {
        double* d = (double*)(dst + totals_at) + threadIdx.x;
        double v = *d;
        for (int w = 0; w < a.W; ++w) v += ((const double*)(a.src[w] + totals_at))[threadIdx.x];
        *d = v;
    } else if (blockIdx.x == 0 && threadIdx.x < 6) {
        unsigned long long* d = (unsigned long long*)(dst + totals_at) + threadIdx.x;
        unsigned long long v = *d;
        for (int w = 0; w < a.W; ++w) v += ((const unsigned long long*)(a.src[w] + totals_at))[threadIdx.x];
        *d = v;
    }
}

bool loss_misaligned(const void* p) { return ((uintptr_t)p & (ALIGN - 1)) != 0; }
bool loss_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}
int loss_check_state(vt_context* c, const char* who, const void* state, size_t state_bytes, int N) {
    if (N <= 0 || N > VT_LOSS_MAX_N) return c->fail(VT_ERR_INVALID, "%s: N = %d outside [1, %d]", who, N, VT_LOSS_MAX_N);
    if (!state || loss_misaligned(state)) return c->fail(VT_ERR_INVALID, "%s: state is null or not 256-B aligned", who);
    const size_t need = vt_loss_layout(N).total;
    if (state_bytes < need) return c->fail(VT_ERR_WORKSPACE, "%s: state holds %zu bytes, %zu needed", who, state_bytes, need);
    return VT_OK;
}
bool loss_params_ok(double alpha, double gamma) { return isfinite(alpha) && isfinite(gamma) && gamma >= 0.0; }
bool loss_same_params(int N, double a0, double g0, const double* w0, double a1, double g1, const double* w1) {
    if (memcmp(&a0, &a1, sizeof(double)) || memcmp(&g0, &g1, sizeof(double)) || (w0 == nullptr) != (w1 == nullptr)) return false;
    return !w0 || w0 == w1 || memcmp(w0, w1, sizeof(double) * (size_t)N) == 0;
}

#define LCKL(c, what) HIPCK(c, hipGetLastError(), what)

}  // namespace

extern "C" {

size_t vt_loss_state_bytes(int N) { return N > 0 && N <= VT_LOSS_MAX_N ? vt_loss_layout(N).total : 0; }

int vt_loss_reset(vt_context* c, void* state, size_t state_bytes, int N, double alpha, double gamma, const double* class_weights, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (int r = loss_check_state(c, "vt_loss_reset", state, state_bytes, N)) return r;
    if (!loss_params_ok(alpha, gamma)) return c->fail(VT_ERR_INVALID, "vt_loss_reset: alpha = %g must be finite, gamma = %g finite and >= 0", alpha, gamma);
    if (class_weights)
        for (int i = 0; i < N; ++i)
            if (class_weights[i] != class_weights[i]) return c->fail(VT_ERR_INVALID, "vt_loss_reset: class weight %d is NaN", i);
    const LossLayout l = vt_loss_layout(N);
    hipStream_t s = (hipStream_t)stream;
    char* st = (char*)state;
    HIPCK(c, hipMemsetAsync(state, 0, l.total, s), "loss_reset clear");
    hipLaunchKernelGGL(loss_init_kernel, dim3(1), dim3(64), 0, s, (double*)(st + l.params), alpha, gamma, class_weights ? 1ull : 0ull,
                       (unsigned long long)N); LCKL(c, "loss_reset init");
    double* w = (double*)(st + l.weights);
    if (!class_weights) {
        hipLaunchKernelGGL(loss_fill_weights_kernel, dim3((N + 255) / 256), dim3(256), 0, s, w, N); LCKL(c, "loss_reset weights");
        return VT_OK;
    }
    for (int base = 0; base < N; base += LS_WCHUNK) {           // as kernel arguments: the host array is free when the call returns
        LossWeightChunk ch;
        const int n = N - base < LS_WCHUNK ? N - base : LS_WCHUNK;
        memcpy(ch.v, class_weights + base, sizeof(double) * (size_t)n);
        for (int i = n; i < LS_WCHUNK; ++i) ch.v[i] = 0.0;
        hipLaunchKernelGGL(loss_set_weights_kernel, dim3(1), dim3(LS_WCHUNK), 0, s, w, base, N, ch); LCKL(c, "loss_reset weights");
    }
    return VT_OK;
}

int vt_loss_update(vt_context* c, void* state, size_t state_bytes, int N, const float* logits, const void* labels, int labels_dtype, int B,
                   void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (int r = loss_check_state(c, "vt_loss_update", state, state_bytes, N)) return r;
    if (!logits || !labels || ((uintptr_t)logits & 3) || (labels_dtype == VT_F32 && ((uintptr_t)labels & 3)) ||
        (labels_dtype != VT_F32 && labels_dtype != VT_U8))
        return c->fail(VT_ERR_INVALID, "vt_loss_update: null or misaligned input, or labels neither VT_F32 nor VT_U8");
    if (B <= 0 || B > VT_EVAL_MAX_B) return c->fail(VT_ERR_INVALID, "vt_loss_update: B = %d outside [1, %d]", B, VT_EVAL_MAX_B);
    const LossLayout l = vt_loss_layout(N);
    hipStream_t s = (hipStream_t)stream;
    char* st = (char*)state;
    const double* params = (const double*)(st + l.params);
    const double* weights = (const double*)(st + l.weights);
    double* sums = (double*)(st + l.sums);
    double* partials = (double*)(st + l.partials);
    if (labels_dtype == VT_U8)
        hipLaunchKernelGGL(loss_accumulate_kernel<unsigned char>, dim3(l.groups), dim3(256), 0, s, logits, (const unsigned char*)labels, B, N, params,
                           weights, sums, partials);
    else
        hipLaunchKernelGGL(loss_accumulate_kernel<float>, dim3(l.groups), dim3(256), 0, s, logits, (const float*)labels, B, N, params, weights, sums,
                           partials);
    LCKL(c, "loss_update");
    hipLaunchKernelGGL(loss_fold_kernel, dim3(1), dim3(64), 0, s, partials, l.groups, B, N, (double*)(st + l.totals)); LCKL(c, "loss_update fold");
    return VT_OK;
}

int vt_loss_read(vt_context* c, const void* state, size_t state_bytes, int N, void* out, size_t out_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (int r = loss_check_state(c, "vt_loss_read", state, state_bytes, N)) return r;
    if (!out || ((uintptr_t)out & 7)) return c->fail(VT_ERR_INVALID, "vt_loss_read: out is null or misaligned");
    const size_t need = vt_loss_layout(N).total;
    if (out_bytes < need) return c->fail(VT_ERR_WORKSPACE, "vt_loss_read: out holds %zu bytes, %zu needed", out_bytes, need);
    if (loss_overlap(state, need, out, need)) return c->fail(VT_ERR_INVALID, "vt_loss_read: out overlaps the state");
    HIPCK(c, hipMemcpyAsync(out, state, need, hipMemcpyDefault, (hipStream_t)stream), "loss_read");
    return VT_OK;
}

int vt_loss_merge(vt_context* c, void* dst, size_t dst_bytes, int N, double alpha, double gamma, const double* class_weights,
                  const vt_loss_source* sources, int W, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (int r = loss_check_state(c, "vt_loss_merge (dst)", dst, dst_bytes, N)) return r;
    if (!sources || W < 1 || W > VT_EVAL_MAX_MERGE) return c->fail(VT_ERR_INVALID, "vt_loss_merge: null sources or W = %d outside [1, %d]", W, VT_EVAL_MAX_MERGE);
    const LossLayout l = vt_loss_layout(N);
    LossMergeArg a;
    a.W = W;
    for (int w = 0; w < W; ++w) {
        const vt_loss_source& s = sources[w];
        if (int r = loss_check_state(c, "vt_loss_merge (source)", s.state, s.state_bytes, N)) return r;
        if (loss_overlap(dst, l.total, s.state, l.total)) return c->fail(VT_ERR_INVALID, "vt_loss_merge: source %d is dst or overlaps it", w);
        if (!loss_same_params(N, alpha, gamma, class_weights, s.alpha, s.gamma, s.class_weights))
            return c->fail(VT_ERR_INVALID, "vt_loss_merge: source %d was taken with another alpha, gamma or class weights than dst", w);
        a.src[w] = (const char*)s.state;
    }
    const long long n2 = 2LL * N;
    hipLaunchKernelGGL(loss_merge_kernel, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, (char*)dst, l.sums, l.totals, n2);
    LCKL(c, "loss_merge");
    return VT_OK;
}

}  // extern "C"
