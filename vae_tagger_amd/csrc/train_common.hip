// What the trainers share (vt_train.h: TrainBlock): the kernels that work on any block -- the gradient norm and clip coefficient, the
// gradient scale, AdamW, the in-order merge of K ranks' gradients -- and one host implementation of the state check, clip, step, the kind -> byte range dispatch of the four
// parameter arrays and the scalars, and the read / write copies.  train_head.hip, train_front.hip and train_cross.hip call these with their own layout
// and the name of the entry point they were reached through.  The conventions are theirs: fp32 storage, fp64 reductions in an order
// fixed by the shapes, no atomics, nothing synchronises the host.
#include <math.h>

#include "vt_common.h"
#include "vt_context.h"
#include "vt_train.h"

using namespace vt;

namespace {

// one workgroup: the squared-norm partials of block 0 in index order, then block 1's, ... (an unused entry has n = 0: t + 0.0 has t's
// bits, t >= 0) -> one norm and coef = min(1, max_norm / (norm + 1e-6))  (clip_grad_norm_), written to every block
struct ClipBlocks { const double* part[VT_CLIP_MAX_BLOCKS]; int n[VT_CLIP_MAX_BLOCKS]; TrainScalars* sc[VT_CLIP_MAX_BLOCKS]; int count; };
__global__ __launch_bounds__(256) void train_clip_kernel(ClipBlocks blocks, float max_norm) {
#pragma clang fp contract(off)
    __shared__ double red[4];
    double total = 0.0;
#pragma unroll
    for (int k = 0; k < VT_CLIP_MAX_BLOCKS; ++k) {
        const double* __restrict__ part = blocks.part[k];
        double a = 0.0;
        for (int i = threadIdx.x; i < blocks.n[k]; i += 256) a += part[i];
        const double t = block_sum_256d(a, red);
        total = k ? total + t : t;
    }
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(total);
        const float coef = max_norm / (norm + 1e-6f);
        TrainScalars v;
        v.sq = total; v.norm = norm; v.coef = coef < 1.0f ? coef : 1.0f;
#pragma unroll
        for (int k = 0; k < VT_CLIP_MAX_BLOCKS; ++k)
            if (k < blocks.count) *blocks.sc[k] = v;
    }
}

// g *= coef when coef < 1 (a gradient inside the bound keeps its bits: nothing is written)
__global__ __launch_bounds__(256) VT_NO_PACKED_F32 void train_scale_kernel(float4* __restrict__ g, long long n4, const TrainScalars* __restrict__ sc) {
    const float coef = sc->coef;
    if (!(coef < 1.0f)) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    float4 v = g[i];
    v.x *= coef; v.y *= coef; v.z *= coef; v.w *= coef;
    g[i] = v;
}

// (VT_NO_PACKED_F32: the compiler would pair these float4 lanes into packed fp32 ops with a source op_sel -- vt_common.h)
// the per-element arithmetic is adamw_one of vt_train.h (shared with vae_optim.hip)
__global__ __launch_bounds__(256) VT_NO_PACKED_F32 void train_adamw_kernel(float4* __restrict__ P, float4* __restrict__ G, float4* __restrict__ M, float4* __restrict__ V,
                                                          long long n4, float decay, float w1, float beta2, float w2, float step_size, float rbc2,
                                                          float eps) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    float4 p = P[i], g = G[i], m = M[i], v = V[i];
    adamw_one(p.x, g.x, m.x, v.x, decay, w1, beta2, w2, step_size, rbc2, eps);
    adamw_one(p.y, g.y, m.y, v.y, decay, w1, beta2, w2, step_size, rbc2, eps);
    adamw_one(p.z, g.z, m.z, v.z, decay, w1, beta2, w2, step_size, rbc2, eps);
    adamw_one(p.w, g.w, m.w, v.w, decay, w1, beta2, w2, step_size, rbc2, eps);
    P[i] = p; G[i] = g; M[i] = m; V[i] = v;
}

// The gradient exchange of a sharded run: grads[e] = (float) sum over r = 0 .. K-1, in that order, of w[r] * (double)src[r * stride + e],
// in fp64 with the multiply and the add rounded separately (a rank whose weight is 0 is still read).  Workgroup b owns chunk b of the
// block's float4s (vt_train_merge_chunk4) and rewrites squared-norm partial b from the fp32 values it stored, so clip and step follow
// as after a backward; a workgroup whose chunk is empty writes 0.0.
struct MergeWeights { double w[VT_MERGE_MAX_RANKS]; };
__global__ __launch_bounds__(256) VT_NO_PACKED_F32 void train_merge_kernel(const float4* __restrict__ src, long long stride4, int K, MergeWeights w,
                                                                           float4* __restrict__ grads, long long n4, long long chunk4,
                                                                           double* __restrict__ normpart) {
#pragma clang fp contract(off)
    __shared__ double red[4];
    const long long lo = (long long)blockIdx.x * chunk4;
    const long long hi = lo + chunk4 < n4 ? lo + chunk4 : n4;
    double sq = 0.0;
    for (long long i = lo + threadIdx.x; i < hi; i += 256) {
        double ax = 0.0, ay = 0.0, az = 0.0, aw = 0.0;
        for (int r = 0; r < K; ++r) {
            const float4 v = src[(long long)r * stride4 + i];
            const double wr = w.w[r];
            double px = wr * (double)v.x, py = wr * (double)v.y, pz = wr * (double)v.z, pw = wr * (double)v.w;
            // the products are pinned in registers: with -ffp-contract=fast on the command line the backend fuses a multiply into
            // the add that follows whatever the pragma says, and w[r] x has more than 53 bits, so the fused sum has other bits
            asm volatile("" : "+v"(px), "+v"(py), "+v"(pz), "+v"(pw));
            ax = ax + px;
            ay = ay + py;
            az = az + pz;
            aw = aw + pw;
        }
        float4 o;
        o.x = (float)ax; o.y = (float)ay; o.z = (float)az; o.w = (float)aw;
        grads[i] = o;
        sq = sq + (double)o.x * (double)o.x;
        sq = sq + (double)o.y * (double)o.y;
        sq = sq + (double)o.z * (double)o.z;
        sq = sq + (double)o.w * (double)o.w;
    }
    const double t = block_sum_256d(sq, red);
    if (threadIdx.x == 0) normpart[blockIdx.x] = t;
}

}  // namespace

int vt_train_check(vt_context* c, const char* who, const TrainBlock& b, const void* state, size_t state_bytes) {
    if (!state || ((uintptr_t)state & (ALIGN - 1))) return c->fail(VT_ERR_INVALID, "%s: state is null or not 256-B aligned", who);
    if (state_bytes < b.total) return c->fail(VT_ERR_WORKSPACE, "%s: state holds %zu bytes, %zu needed", who, state_bytes, b.total);
    return VT_OK;
}

int vt_train_clip_blocks(vt_context* c, const char* who, const TrainBlockRef* blocks, int n, float max_norm, hipStream_t s) {
    if (!(max_norm > 0.f)) return c->fail(VT_ERR_INVALID, "%s: max_norm = %g must be positive", who, max_norm);
    if (n < 1 || n > VT_CLIP_MAX_BLOCKS) return c->fail(VT_ERR_INVALID, "%s: %d blocks, 1 to %d expected", who, n, VT_CLIP_MAX_BLOCKS);
    ClipBlocks k;
    for (int i = 0; i < VT_CLIP_MAX_BLOCKS; ++i) {
        const TrainBlockRef& b = blocks[i < n ? i : 0];
        k.part[i] = (const double*)((char*)b.state + b.layout->normpart);
        k.n[i] = i < n ? b.layout->norm_parts : 0;
        k.sc[i] = (TrainScalars*)((char*)b.state + b.layout->scalars);
    }
    k.count = n;
    hipLaunchKernelGGL(train_clip_kernel, dim3(1), dim3(256), 0, s, k, max_norm);
    HIPCK(c, hipGetLastError(), who);
    return vt_train_scale_blocks(c, who, blocks, n, s);
}

int vt_train_scale_blocks(vt_context* c, const char* who, const TrainBlockRef* blocks, int n, hipStream_t s) {
    for (int i = 0; i < n; ++i) {
        const long long n4 = (long long)(blocks[i].layout->P / 4);
        hipLaunchKernelGGL(train_scale_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s,
                           (float4*)((char*)blocks[i].state + blocks[i].layout->grads), n4,
                           (const TrainScalars*)((char*)blocks[i].state + blocks[i].layout->scalars));
        HIPCK(c, hipGetLastError(), who);
    }
    return VT_OK;
}

int vt_train_step(vt_context* c, const char* who, const TrainBlock& b, void* state, double lr, double beta1, double beta2, double eps,
                  double weight_decay, long long t, hipStream_t s) {
    if (t < 1 || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !isfinite(lr) || !isfinite(weight_decay))
        return c->fail(VT_ERR_INVALID, "%s: t >= 1, betas in [0, 1), eps >= 0 and finite lr / weight_decay expected", who);
    char* st = (char*)state;
    const long long n4 = (long long)(b.P / 4);
    const double bc1 = 1.0 - pow(beta1, (double)t), bc2 = 1.0 - pow(beta2, (double)t);
    hipLaunchKernelGGL(train_adamw_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, (float4*)(st + b.params), (float4*)(st + b.grads),
                       (float4*)(st + b.m), (float4*)(st + b.v), n4, (float)(1.0 - lr * weight_decay), (float)(1.0 - beta1), (float)beta2,
                       (float)(1.0 - beta2), (float)(lr / bc1), (float)sqrt(bc2), (float)eps);
    HIPCK(c, hipGetLastError(), who);
    return VT_OK;
}

int vt_train_grads_export(vt_context* c, const char* who, const TrainBlock& b, const void* state, void* dst, size_t dst_bytes, hipStream_t s) {
    if (!dst || ((uintptr_t)dst & 15)) return c->fail(VT_ERR_INVALID, "%s: dst is null or not 16-B aligned", who);
    if (dst_bytes < 4 * b.P) return c->fail(VT_ERR_WORKSPACE, "%s: dst holds %zu bytes, %zu needed", who, dst_bytes, 4 * b.P);
    HIPCK(c, hipMemcpyAsync(dst, (const char*)state + b.grads, 4 * b.P, hipMemcpyDeviceToDevice, s), who);
    return VT_OK;
}

int vt_train_grads_merge(vt_context* c, const char* who, const TrainBlock& b, void* state, const void* src, size_t stride_floats, int K,
                         const double* weights, hipStream_t s) {
    if (K < 1 || K > VT_MERGE_MAX_RANKS) return c->fail(VT_ERR_INVALID, "%s: K = %d ranks, 1 to %d expected", who, K, VT_MERGE_MAX_RANKS);
    if (!src || ((uintptr_t)src & 15)) return c->fail(VT_ERR_INVALID, "%s: src is null or not 16-B aligned", who);
    if (stride_floats % 4 || stride_floats < b.P)
        return c->fail(VT_ERR_INVALID, "%s: stride of %zu floats, a multiple of 4 that is at least %zu expected", who, stride_floats, b.P);
    if (!weights) return c->fail(VT_ERR_INVALID, "%s: weights is null", who);
    MergeWeights w;
    for (int r = 0; r < VT_MERGE_MAX_RANKS; ++r) {
        w.w[r] = r < K ? weights[r] : 0.0;
        if (!isfinite(w.w[r]) || w.w[r] < 0.0) return c->fail(VT_ERR_INVALID, "%s: weight %d = %g must be finite and non-negative", who, r, w.w[r]);
    }
    char* st = (char*)state;
    const long long n4 = (long long)(b.P / 4);
    hipLaunchKernelGGL(train_merge_kernel, dim3((unsigned)b.norm_parts), dim3(256), 0, s, (const float4*)src, (long long)(stride_floats / 4), K, w,
                       (float4*)(st + b.grads), n4, vt_train_merge_chunk4(b.P, b.norm_parts), (double*)(st + b.normpart));
    HIPCK(c, hipGetLastError(), who);
    return VT_OK;
}

int vt_train_section(vt_context* c, const char* who, const TrainBlock& b, int kind, size_t toff, size_t numel, size_t* off, size_t* bytes) {
    if (kind >= VT_HEAD_PARAM && kind <= VT_HEAD_ADAM_V) {
        const size_t base = kind == VT_HEAD_PARAM ? b.params : kind == VT_HEAD_GRAD ? b.grads : kind == VT_HEAD_ADAM_M ? b.m : b.v;
        *off = base + 4 * toff; *bytes = 4 * numel;
        return VT_OK;
    }
    if (kind == VT_HEAD_NORM) { *off = b.scalars; *bytes = sizeof(TrainScalars); return VT_OK; }
    return c->fail(VT_ERR_INVALID, "%s: unknown kind %d", who, kind);
}

int vt_train_read(vt_context* c, const char* who, const void* state, size_t off, size_t bytes, void* out, size_t out_bytes, hipStream_t s) {
    if (!out || out_bytes < bytes) return c->fail(VT_ERR_WORKSPACE, "%s: out is null or holds %zu bytes, %zu needed", who, out_bytes, bytes);
    HIPCK(c, hipMemcpyAsync(out, (const char*)state + off, bytes, hipMemcpyDefault, s), who);
    return VT_OK;
}

int vt_train_write(vt_context* c, const char* who, void* state, size_t off, size_t bytes, const void* src, size_t src_bytes, hipStream_t s) {
    if (!src || src_bytes != bytes) return c->fail(VT_ERR_INVALID, "%s: src is null or holds %zu bytes, %zu expected", who, src_bytes, bytes);
    HIPCK(c, hipMemcpyAsync((char*)state + off, src, bytes, hipMemcpyDefault, s), who);
    return VT_OK;
}
