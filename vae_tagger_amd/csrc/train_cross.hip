// Training of the attention decoder's CROSS-ATTENTION on the device: query_generator.* and cross_attention.* of
// AttentionClassificationDecoder (modules.py:105-124, :451-459), the piece between the front's rows x [B][512] (train_front.hip) and the
// feature rows the head reads (train_head.hip).  One caller-owned state block (vt_train.h: CrossLayout), the other trainers'
// conventions: fp32 storage; fp64 accumulation and norm partials; no atomics; every sum in an order fixed by the shapes; nothing
// synchronises the host.  State check, clip, AdamW step and read / write are train_common.hip's.  There is no dropout and no
// normalisation layer in this piece, so training and eval forward are one function.
//   forward    decoder.hip's launches (vt_dec_cross) on the state's tensors: the inference bits.  q = Wg x + bg, u = Wq q + bq and the
//              attention output o stay in the workspace for the backward.
//   backward   y = x + mean(a) 1, a = Wo o + bo + q, so every entry of d a is g = sum_f dY[f] / 512:
//              1. colsum(Wo) once, then g and d o = g colsum(Wo)                  (one workgroup per image)
//              2. attention: one workgroup per image, one lane per key token, everything recomputed in fp64.  Scores and d p are
//                 linear in the token: s_j = a0_h + A_h . t_j with A_h = scale sum_{e in h} u_e Wk[e][:], d p_j = b0_h + Bv_h . t_j with
//                 Bv_h = sum_{e in h} d o_e Wv[e][:], so a head costs 8-vectors per token whatever its width.  d s = p (d p - sum p d p)
//                 is a cancelling sum (fp64); d t_j = d s_j A_h + p_j Bv_h; the image's partial row of d Wk, d bk, d Wv, d bv and
//                 d u come from the wave sums sum_j p_j t_j, sum_j d s_j t_j, sum_j d s_j, sum_j p_j of each head
//              3. d q = g + Wq^T d u, then d X = d Y + d t + Wg^T d q             ([B]-row transposed mat-vecs, 8 images per pass)
//              4. d Wg += sum_b d q (x) x, d Wq += sum_b d u (x) q, d Wo += sum_b g (x) o and their biases: a workgroup owns a tile of
//                 8 rows x 256 columns, loops b in ascending order, adds into the gradients and writes its squared-norm partial
//              5. the per-image partial rows of k_proj / v_proj are added in image order into the gradients
#include <math.h>
#include <string.h>

#include "vt_common.h"
#include "vt_context.h"
#include "vt_train.h"

using namespace vt;

namespace {

#define CROSS_KERNEL(n) __global__ __launch_bounds__(n) VT_NO_PACKED_F32

constexpr int GEMV_BT = 8;                   // images per pass of the transposed mat-vec
constexpr int OUTER_BT = 64;                 // images staged per pass of the outer-product kernel

// butterfly reductions: every lane ends with the same bits (a + b and b + a round alike)
__device__ __forceinline__ double wave_all_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_all_max_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// colsum[e] = sum_f Wo[f][e]: the same for every image, so once per backward
CROSS_KERNEL(256) void cross_colsum_kernel(const float* __restrict__ wo, double* __restrict__ colsum) {
    const int t = threadIdx.x;
    double cs = 0.0;
    for (int f = 0; f < 512; ++f) cs += (double)wo[f * 256 + t];
    colsum[t] = cs;
}

// g[b] = sum_f dY[b][f] / 512;  d_o[b][e] = g[b] colsum[e]
CROSS_KERNEL(256) void cross_do_kernel(const float* dy, const double* __restrict__ colsum, double* __restrict__ g, float* __restrict__ d_o) {
    __shared__ double red[4];
    const int b = blockIdx.x, t = threadIdx.x;
    const double a = (double)dy[(long long)b * 512 + t] + (double)dy[(long long)b * 512 + 256 + t];
    const double gs = block_sum_256d(a, red) / 512.0;
    if (t == 0) g[b] = gs;
    d_o[(long long)b * 256 + t] = (float)(gs * colsum[t]);
}

// the attention backward of image b (see the head of the file).  x [B][512] with token j, channel c at c 64 + j; u, d_o [B][256];
// writes du [B][256], dt [B][512] (x's layout) and part[b][VT_CROSS_KV_ROW]
CROSS_KERNEL(64) void cross_attn_bwd_kernel(const float* __restrict__ x, const float* __restrict__ params, const float* __restrict__ u,
                                            const float* __restrict__ d_o, int heads, float* __restrict__ du, float* __restrict__ dt_out,
                                            float* __restrict__ part) {
    __shared__ double s_u[256], s_do[256];
    __shared__ double s_A[8][8], s_Bv[8][8], s_a0[8], s_b0[8];
    __shared__ double s_pt[8][8], s_st[8][8], s_sds[8], s_sp[8];
    const float* wk = params + VT_CROSS_TABLE[VT_CT_KW].off;
    const float* bk = params + VT_CROSS_TABLE[VT_CT_KB].off;
    const float* wv = params + VT_CROSS_TABLE[VT_CT_VW].off;
    const float* bv = params + VT_CROSS_TABLE[VT_CT_VB].off;
    const int b = blockIdx.x, l = threadIdx.x;
    const int hd = 256 / heads;
    const double scale = 1.0 / sqrt((double)hd);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = l + 64 * i;
        s_u[e] = (double)u[(long long)b * 256 + e];
        s_do[e] = (double)d_o[(long long)b * 256 + e];
    }
    __syncthreads();
    {   // lane = (head, channel): the head's 8-vectors
        const int h = l >> 3, c = l & 7;
        if (h < heads) {
            double A = 0.0, Bv = 0.0, a0 = 0.0, b0 = 0.0;
            for (int d = 0; d < hd; ++d) {
                const int e = h * hd + d;
                A += (double)wk[e * 8 + c] * s_u[e];
                Bv += (double)wv[e * 8 + c] * s_do[e];
                a0 += (double)bk[e] * s_u[e];
                b0 += (double)bv[e] * s_do[e];
            }
            s_A[h][c] = A * scale; s_Bv[h][c] = Bv;
            if (c == 0) { s_a0[h] = a0 * scale; s_b0[h] = b0; }
        }
    }
    __syncthreads();
    // lane = key token
    double t[8], dt[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) { t[c] = (double)x[(long long)b * 512 + c * 64 + l]; dt[c] = 0.0; }
    for (int h = 0; h < heads; ++h) {
        double s = s_a0[h], dp = s_b0[h];
#pragma unroll
        for (int c = 0; c < 8; ++c) { s += s_A[h][c] * t[c]; dp += s_Bv[h][c] * t[c]; }
        const double m = wave_all_max_d(s);
        double p = exp(s - m);
        p /= wave_all_sum_d(p);
        const double row = wave_all_sum_d(p * dp);
        const double ds = p * (dp - row);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            dt[c] += ds * s_A[h][c] + p * s_Bv[h][c];
            const double pt = wave_all_sum_d(p * t[c]), st = wave_all_sum_d(ds * t[c]);
            if (l == 0) { s_pt[h][c] = pt; s_st[h][c] = st; }
        }
        const double sds = wave_all_sum_d(ds), sp = wave_all_sum_d(p);
        if (l == 0) { s_sds[h] = sds; s_sp[h] = sp; }
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) dt_out[(long long)b * 512 + c * 64 + l] = (float)dt[c];
    __syncthreads();
    // lane = embedding entries e = l + 64 i: the image's partial row and d u
    float* row = part + (long long)b * VT_CROSS_KV_ROW;
    constexpr int KB = 2048, VW = 2304, VB = 2304 + 2048;         // k_proj.bias, v_proj.weight, v_proj.bias inside the row
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = l + 64 * i, h = e / hd;
        const double ue = s_u[e] * scale, de = s_do[e];
        double a = (double)bk[e] * s_sds[h];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            row[e * 8 + c] = (float)(ue * s_st[h][c]);
            row[VW + e * 8 + c] = (float)(de * s_pt[h][c]);
            a += (double)wk[e * 8 + c] * s_st[h][c];
        }
        row[KB + e] = (float)(ue * s_sds[h]);
        row[VB + e] = (float)(de * s_sp[h]);
        du[(long long)b * 256 + e] = (float)(a * scale);
    }
}
static_assert(VT_CROSS_TABLE[VT_CT_KB].off - VT_CROSS_TABLE[VT_CT_KW].off == 2048 && VT_CROSS_TABLE[VT_CT_VW].off - VT_CROSS_TABLE[VT_CT_KW].off == 2304 &&
              VT_CROSS_TABLE[VT_CT_VB].off - VT_CROSS_TABLE[VT_CT_KW].off == 2304 + 2048, "the partial row follows the table from k_proj.weight on");

// out[b][i] = base + sum_k W[k][i] v[b][k] for GEMV_BT images per workgroup, one column i per thread (W [K][N], K <= 512).
// MODE 0: base = g[b] (d q);  MODE 1: base = add0[b][i] + add1[b][i] (d X = d Y + d t + ...; out may be add0)
template <int MODE>
CROSS_KERNEL(256) void cross_gemv_t_kernel(const float* __restrict__ w, const float* __restrict__ v, int K, int N, int B, const double* __restrict__ g,
                                           const float* add0, const float* __restrict__ add1, float* out) {
    __shared__ float sv[GEMV_BT][512];
    const int b0 = blockIdx.y * GEMV_BT, t = threadIdx.x;
    for (int idx = t; idx < GEMV_BT * K; idx += 256) {
        const int bi = idx / K, k = idx - bi * K;
        sv[bi][k] = b0 + bi < B ? v[(long long)(b0 + bi) * K + k] : 0.f;
    }
    __syncthreads();
    const int i = blockIdx.x * 256 + t;
    double acc[GEMV_BT];
#pragma unroll
    for (int bi = 0; bi < GEMV_BT; ++bi) acc[bi] = 0.0;
    for (int k = 0; k < K; ++k) {
        const double wv = (double)w[(long long)k * N + i];
#pragma unroll
        for (int bi = 0; bi < GEMV_BT; ++bi) acc[bi] += wv * (double)sv[bi][k];
    }
#pragma unroll
    for (int bi = 0; bi < GEMV_BT; ++bi) {
        if (b0 + bi >= B) break;
        const long long o = (long long)(b0 + bi) * N + i;
        const double base = MODE == 0 ? g[b0 + bi] : (double)add0[o] + (double)add1[o];
        out[o] = (float)(base + acc[bi]);
    }
}

// G[r][col] += sum_b L[b][r] R[b][col] over a tile of VT_CROSS_TILE_ROWS rows x 256 columns, b ascending; the workgroups of column tile 0
// also add sum_b L[b][r] into the bias gradient Gb[r].  BCAST: L[b][r] = g[b] for every r (d a).  normpart[tile] = the sum of squares of
// what this workgroup wrote.
template <bool BCAST>
CROSS_KERNEL(256) void cross_outer_kernel(const float* __restrict__ L, const double* __restrict__ g, int M, const float* __restrict__ R, int N, int B,
                                          float* __restrict__ G, float* __restrict__ Gb, double* __restrict__ normpart) {
    constexpr int TR = VT_CROSS_TILE_ROWS;
    __shared__ double sl[OUTER_BT][TR];
    __shared__ double red[4];
    const int t = threadIdx.x, row0 = blockIdx.y * TR, col = blockIdx.x * 256 + t;
    const bool bias = blockIdx.x == 0 && t < TR;
    double acc[TR], bacc = 0.0;
#pragma unroll
    for (int r = 0; r < TR; ++r) acc[r] = 0.0;
    for (int b0 = 0; b0 < B; b0 += OUTER_BT) {
        __syncthreads();
        for (int idx = t; idx < OUTER_BT * TR; idx += 256) {
            const int bb = idx / TR, r = idx - bb * TR;
            double v = 0.0;
            if (b0 + bb < B) v = BCAST ? g[b0 + bb] : (double)L[(long long)(b0 + bb) * M + row0 + r];
            sl[bb][r] = v;
        }
        __syncthreads();
        const int nb = B - b0 < OUTER_BT ? B - b0 : OUTER_BT;
        for (int bb = 0; bb < nb; ++bb) {
            const double rv = (double)R[(long long)(b0 + bb) * N + col];
#pragma unroll
            for (int r = 0; r < TR; ++r) acc[r] += sl[bb][r] * rv;
        }
        if (bias)
            for (int bb = 0; bb < nb; ++bb) bacc += sl[bb][t];
    }
    double sq = 0.0;
#pragma unroll
    for (int r = 0; r < TR; ++r) {
        float* gp = G + (long long)(row0 + r) * N + col;
        const float gv = *gp + (float)acc[r];
        *gp = gv;
        sq += (double)gv * (double)gv;
    }
    if (bias) {
        const float gv = Gb[row0 + t] + (float)bacc;
        Gb[row0 + t] = gv;
        sq += (double)gv * (double)gv;
    }
    const double total = block_sum_256d(sq, red);
    if (t == 0) normpart[blockIdx.y * gridDim.x + blockIdx.x] = total;
}

// G[i] += sum over the images' partial rows in image order (fp64); normpart[blockIdx.x] = the sum of squares of what was written
CROSS_KERNEL(256) void cross_reduce_kernel(const float* __restrict__ part, int B, float* __restrict__ G, double* __restrict__ normpart) {
    __shared__ double red[4];
    const int i = blockIdx.x * 256 + threadIdx.x;             // (the grid covers VT_CROSS_KV_ROW exactly)
    double a = 0.0;
    for (int r = 0; r < B; ++r) a += (double)part[(long long)r * VT_CROSS_KV_ROW + i];
    const float gv = G[i] + (float)a;
    G[i] = gv;
    const double total = block_sum_256d((double)gv * (double)gv, red);
    if (threadIdx.x == 0) normpart[blockIdx.x] = total;
}
static_assert(VT_CROSS_KV_ROW % 256 == 0, "cross_reduce_kernel's grid covers the row exactly");

#define TCKL(c, what) HIPCK(c, hipGetLastError(), what)

int cross_check(vt_context* c, const char* who, const void* state, size_t state_bytes, CrossLayout* out) {
    if (!c->dec_finalized) return c->fail(VT_ERR_STATE, "%s: decoder weights not finalized", who);
    if (!vt_cross_trainable(c->dec))
        return c->fail(VT_ERR_INVALID, "%s: this decoder has no cross-attention that can be trained on the device (attention decoder with "
                                       "cross-attention, latent_channels 16, heads in {1, 2, 4, 8} expected)", who);
    *out = vt_cross_layout(c->dec);
    return vt_train_check(c, who, *out, state, state_bytes);
}

int cross_check_batch(vt_context* c, const char* who, const void* rows, const char* rows_name, int B, const void* ws, size_t ws_bytes) {
    if (!rows || ((uintptr_t)rows & 3)) return c->fail(VT_ERR_INVALID, "%s: %s is null or misaligned", who, rows_name);
    if (B <= 0 || B > VT_FRONT_MAX_B) return c->fail(VT_ERR_INVALID, "%s: B = %d outside [1, %d]", who, B, VT_FRONT_MAX_B);
    if (!ws || ((uintptr_t)ws & (ALIGN - 1))) return c->fail(VT_ERR_INVALID, "%s: workspace is null or not 256-B aligned", who);
    const size_t need = vt_cross_workspace(B).total;
    if (ws_bytes < need) return c->fail(VT_ERR_WORKSPACE, "%s: workspace holds %zu bytes, %zu needed", who, ws_bytes, need);
    return VT_OK;
}

// the context's table entry of tensor t
const float** cross_ctx_slot(DecoderWeights& d, int t) {
    switch (t) {
        case VT_CT_GW: return &d.qg_w; case VT_CT_GB: return &d.qg_b; case VT_CT_QW: return &d.cx_q_w; case VT_CT_QB: return &d.cx_q_b;
        case VT_CT_KW: return &d.cx_k_w; case VT_CT_KB: return &d.cx_k_b; case VT_CT_VW: return &d.cx_v_w; case VT_CT_VB: return &d.cx_v_b;
        case VT_CT_OW: return &d.cx_o_w; default: return &d.cx_o_b;
    }
}

int cross_section(vt_context* c, const char* who, const CrossLayout& l, int kind, const char* name, size_t* off, size_t* bytes) {
    if (kind < VT_HEAD_PARAM || kind > VT_HEAD_ADAM_V) return vt_train_section(c, who, l, kind, 0, 0, off, bytes);    // no tensor is meant
    for (int i = 0; i < VT_CROSS_TENSORS; ++i)
        if (name && strcmp(VT_CROSS_TABLE[i].name, name) == 0)
            return vt_train_section(c, who, l, kind, VT_CROSS_TABLE[i].off, VT_CROSS_TABLE[i].numel, off, bytes);
    return c->fail(VT_ERR_INVALID, "%s: no cross-attention parameter named %s", who, name ? name : "(null)");
}

}  // namespace

extern "C" {

size_t vt_cross_state_bytes(const vt_context* c) {
    if (!c || !c->dec_configured || !vt_cross_trainable(c->dec)) return 0;
    return vt_cross_layout(c->dec).total;
}

size_t vt_cross_workspace_bytes(const vt_context* c, int B) {
    if (!c || !c->dec_configured || !vt_cross_trainable(c->dec) || B <= 0 || B > VT_FRONT_MAX_B) return 0;
    return vt_cross_workspace(B).total;
}

int vt_cross_init(vt_context* c, void* state, size_t state_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    CrossLayout l;
    VTCK(cross_check(c, "vt_cross_init", state, state_bytes, &l));
    hipStream_t s = (hipStream_t)stream;
    char* st = (char*)state;
    HIPCK(c, hipMemsetAsync(state, 0, l.total, s), "cross_init clear");
    for (int i = 0; i < VT_CROSS_TENSORS; ++i)
        HIPCK(c, hipMemcpyAsync((float*)(st + l.params) + VT_CROSS_TABLE[i].off, *cross_ctx_slot(c->dec, i), 4 * (size_t)VT_CROSS_TABLE[i].numel,
                                hipMemcpyDeviceToDevice, s), "cross_init copy");
    const TrainBlockRef blocks[1] = {{&l, st}};
    return vt_train_clip_blocks(c, "vt_cross_init", blocks, 1, 1.0f, s);        // over the zeroed block: norm 0, coefficient 1
}

int vt_cross_commit(vt_context* c, const void* state, size_t state_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    CrossLayout l;
    VTCK(cross_check(c, "vt_cross_commit", state, state_bytes, &l));
    const char* st = (const char*)state;
    for (int i = 0; i < VT_CROSS_TENSORS; ++i)
        HIPCK(c, hipMemcpyAsync(const_cast<float*>(*cross_ctx_slot(c->dec, i)), (const float*)(st + l.params) + VT_CROSS_TABLE[i].off,
                                4 * (size_t)VT_CROSS_TABLE[i].numel, hipMemcpyDeviceToDevice, (hipStream_t)stream), "cross_commit copy");
    return VT_OK;
}

int vt_cross_forward(vt_context* c, void* state, size_t state_bytes, const float* x_in, int B, float* features_out, void* ws, size_t ws_bytes,
                     void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    CrossLayout l;
    VTCK(cross_check(c, "vt_cross_forward", state, state_bytes, &l));
    VTCK(cross_check_batch(c, "vt_cross_forward", x_in, "x_in", B, ws, ws_bytes));
    if (!features_out || ((uintptr_t)features_out & 3) || features_out == x_in)
        return c->fail(VT_ERR_INVALID, "vt_cross_forward: features_out is null, misaligned or x_in itself");
    const CrossWorkspace k = vt_cross_workspace(B);
    hipStream_t s = (hipStream_t)stream;
    char* wsb = (char*)ws;
    const float* P = (const float*)((const char*)state + l.params);
    DecoderWeights d = c->dec;
    for (int i = 0; i < VT_CROSS_TENSORS; ++i) *cross_ctx_slot(d, i) = P + VT_CROSS_TABLE[i].off;
    HIPCK(c, hipMemcpyAsync(features_out, x_in, 4 * (size_t)B * 512, hipMemcpyDeviceToDevice, s), "cross_forward copy");
    HIPCK(c, vt_dec_cross(d, x_in, B, (float*)(wsb + k.q), (float*)(wsb + k.u), (float*)(wsb + k.o), (float*)(wsb + k.a), features_out, s),
          "decoder cross-attention");
    return VT_OK;
}

int vt_cross_backward(vt_context* c, void* state, size_t state_bytes, const float* x_in, const float* d_features, int B, float* d_x_out, void* ws,
                      size_t ws_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    CrossLayout l;
    VTCK(cross_check(c, "vt_cross_backward", state, state_bytes, &l));
    VTCK(cross_check_batch(c, "vt_cross_backward", x_in, "x_in", B, ws, ws_bytes));
    if (!d_features || ((uintptr_t)d_features & 3) || !d_x_out || ((uintptr_t)d_x_out & 3))
        return c->fail(VT_ERR_INVALID, "vt_cross_backward: d_features or d_x_out is null or misaligned");
    const CrossWorkspace k = vt_cross_workspace(B);
    hipStream_t s = (hipStream_t)stream;
    char* st = (char*)state;
    char* wsb = (char*)ws;
    const float* P = (const float*)(st + l.params);
    float* G = (float*)(st + l.grads);
    double* normpart = (double*)(st + l.normpart);
    auto T = [&](int t) { return P + VT_CROSS_TABLE[t].off; };
    auto GT = [&](int t) { return G + VT_CROSS_TABLE[t].off; };
    const float* q = (const float*)(wsb + k.q); const float* u = (const float*)(wsb + k.u); const float* o = (const float*)(wsb + k.o);
    double* g = (double*)(wsb + k.g);
    float* d_o = (float*)(wsb + k.d_o); float* du = (float*)(wsb + k.du); float* dq = (float*)(wsb + k.dq); float* dt = (float*)(wsb + k.dt);
    float* part = (float*)(wsb + k.part);
    const int passes = (B + GEMV_BT - 1) / GEMV_BT;
    double* colsum = (double*)(wsb + k.colsum);
    hipLaunchKernelGGL(cross_colsum_kernel, dim3(1), dim3(256), 0, s, T(VT_CT_OW), colsum); TCKL(c, "cross colsum");
    hipLaunchKernelGGL(cross_do_kernel, dim3(B), dim3(256), 0, s, d_features, (const double*)colsum, g, d_o); TCKL(c, "cross d o");
    hipLaunchKernelGGL(cross_attn_bwd_kernel, dim3(B), dim3(64), 0, s, x_in, P, u, (const float*)d_o, l.heads, du, dt, part); TCKL(c, "cross attention backward");
    hipLaunchKernelGGL(cross_gemv_t_kernel<0>, dim3(2, passes), dim3(256), 0, s, T(VT_CT_QW), (const float*)du, 256, 512, B, (const double*)g,
                       (const float*)nullptr, (const float*)nullptr, dq); TCKL(c, "cross d q");
    hipLaunchKernelGGL(cross_gemv_t_kernel<1>, dim3(2, passes), dim3(256), 0, s, T(VT_CT_GW), (const float*)dq, 512, 512, B, (const double*)g,
                       d_features, (const float*)dt, d_x_out); TCKL(c, "cross d x");
    constexpr int TR = VT_CROSS_TILE_ROWS;
    hipLaunchKernelGGL(cross_outer_kernel<false>, dim3(2, 512 / TR), dim3(256), 0, s, (const float*)dq, (const double*)g, 512, x_in, 512, B,
                       GT(VT_CT_GW), GT(VT_CT_GB), normpart + VT_CROSS_SLOT_G); TCKL(c, "cross d Wg");
    hipLaunchKernelGGL(cross_outer_kernel<false>, dim3(2, 256 / TR), dim3(256), 0, s, (const float*)du, (const double*)g, 256, q, 512, B,
                       GT(VT_CT_QW), GT(VT_CT_QB), normpart + VT_CROSS_SLOT_Q); TCKL(c, "cross d Wq");
    hipLaunchKernelGGL(cross_outer_kernel<true>, dim3(1, 512 / TR), dim3(256), 0, s, (const float*)nullptr, (const double*)g, 512, o, 256, B,
                       GT(VT_CT_OW), GT(VT_CT_OB), normpart + VT_CROSS_SLOT_O); TCKL(c, "cross d Wo");
    hipLaunchKernelGGL(cross_reduce_kernel, dim3(VT_CROSS_KV_ROW / 256), dim3(256), 0, s, (const float*)part, B, GT(VT_CT_KW), normpart + VT_CROSS_SLOT_KV);
    TCKL(c, "cross k / v reduce");
    return VT_OK;
}

int vt_cross_step(vt_context* c, void* state, size_t state_bytes, double lr, double beta1, double beta2, double eps, double weight_decay, long long t,
                  void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    CrossLayout l;
    VTCK(cross_check(c, "vt_cross_step", state, state_bytes, &l));
    return vt_train_step(c, "vt_cross_step", l, state, lr, beta1, beta2, eps, weight_decay, t, (hipStream_t)stream);
}

// the gradient exchange of a sharded run (vt_train.h)
size_t vt_cross_grads_floats(const vt_context* c) {
    return vt_cross_state_bytes(c) ? vt_cross_layout(c->dec).P : 0;
}

int vt_cross_grads_export(vt_context* c, const void* state, size_t state_bytes, void* dst, size_t dst_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    CrossLayout l;
    VTCK(cross_check(c, "vt_cross_grads_export", state, state_bytes, &l));
    return vt_train_grads_export(c, "vt_cross_grads_export", l, state, dst, dst_bytes, (hipStream_t)stream);
}

int vt_cross_grads_merge(vt_context* c, void* state, size_t state_bytes, const float* src, size_t stride_floats, int K, const double* weights,
                         void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    CrossLayout l;
    VTCK(cross_check(c, "vt_cross_grads_merge", state, state_bytes, &l));
    return vt_train_grads_merge(c, "vt_cross_grads_merge", l, state, src, stride_floats, K, weights, (hipStream_t)stream);
}

int vt_cross_read(vt_context* c, const void* state, size_t state_bytes, int kind, const char* name, void* out, size_t out_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    CrossLayout l;
    VTCK(cross_check(c, "vt_cross_read", state, state_bytes, &l));
    size_t off = 0, bytes = 0;
    VTCK(cross_section(c, "vt_cross_read", l, kind, name, &off, &bytes));
    return vt_train_read(c, "vt_cross_read", state, off, bytes, out, out_bytes, (hipStream_t)stream);
}

int vt_cross_write(vt_context* c, void* state, size_t state_bytes, int kind, const char* name, const void* src, size_t src_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    CrossLayout l;
    VTCK(cross_check(c, "vt_cross_write", state, state_bytes, &l));
    if (kind < VT_HEAD_PARAM || kind > VT_HEAD_ADAM_V) return c->fail(VT_ERR_INVALID, "vt_cross_write: kind %d is not a parameter array", kind);
    size_t off = 0, bytes = 0;
    VTCK(cross_section(c, "vt_cross_write", l, kind, name, &off, &bytes));
    return vt_train_write(c, "vt_cross_write", state, off, bytes, src, src_bytes, (hipStream_t)stream);
}

}  // extern "C"
