// Training of the attention decoder's FRONT on the device: spatial_attention.*, feature_compress.* and self_attention_post.* of
// AttentionClassificationDecoder (modules.py:36-47, :66-91, :377-382) at latent_channels = 16, heads in {1, 2, 4, 8}, each of spatial
// and self attention on or off.  On a decoder with cross-attention the front ends in the rows cross-attention reads (modules.py:448),
// in both modes; query_generator.* and cross_attention.* are train_cross.hip's.  One caller-owned state block
// (vt_train.h), the head trainer's conventions: fp32 storage; fp64 statistics and norm partials; no atomics; every sum in an order
// fixed by the shapes; nothing synchronises the host.  The gradient with respect to the latent is not computed (the encoder is frozen).
// State check, AdamW step, the parameter kinds of read / write and the scalars are train_common.hip's; this file keeps the front's
// kernels and its own kinds (the BatchNorm buffers and the re-fold after a write).
//   forward, train = 0   vt_decoder_front on the state's tensors: the inference kernels, BatchNorm folded from the running statistics
//   forward, train != 0  pool / gate / sgate (decoder.hip's launches: same bits) and spmap (SpatialAttention) -> xs = (x gate) sgate
//                        -> conv3x3 -> z; batch statistics of z
//                        (fp64 partials per 256 pixels, finished in chunk order; running statistics updated as nn.BatchNorm2d does);
//                        BatchNorm + ReLU + adaptive pool 8x8; self-attention with dropout on the softmax weights (vt_head_keep,
//                        layer VT_FRONT_DROPOUT_LAYER, element ((b heads + head) 64 + query) 64 + key)
//   backward             self-attention (one workgroup per image, everything recomputed from the pooled rows) -> pool / ReLU /
//                        BatchNorm (a gather per pixel over the pool windows that contain it) -> conv dW / db (LDS tiles, per-tile
//                        partials) -> the spatial gate's 7x7 weight, the channel max to the arg-max channel (lowest index on a tie),
//                        the channel gate's MLP.  Weight gradients: partials per image / tile, then front_reduce_kernel adds them in
//                        index order into the gradients and writes the squared-norm partial of what it wrote.
#include <math.h>
#include <string.h>

#include "vt_common.h"
#include "vt_context.h"
#include "vt_train.h"

using namespace vt;

namespace {

#define FRONT_KERNEL(n) __global__ __launch_bounds__(n) VT_NO_PACKED_F32

// float offset of tensor T inside the partial row of its gradient group (a row starts at the group's first float)
template <int T> constexpr int SA_ROW = VT_FRONT_TABLE[T].off - VT_FG_START[VT_FG_SA];
template <int T> constexpr int MLP_ROW = VT_FRONT_TABLE[T].off - VT_FG_START[VT_FG_MLP];

// ---- SpatialAttention forward: pool, channel gate and spatial gate are decoder.hip's launches (vt_dec_pool / _gate / _sgate) ----------
// mean / max over channels of x gate -> sp[b][2][HW]; am[b][p] = the channel of the max, the lowest on a tie.  Not dec_spmap_kernel:
// it records the arg-max channel, and its `if (v > m)` is not fmaxf on a tie of +0 and -0 (fmaxf may return either zero)
FRONT_KERNEL(256) void front_spmap_kernel(const float* __restrict__ x, const float* __restrict__ gate, int HW, float* __restrict__ sp,
                                          unsigned char* __restrict__ am) {
    const int b = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    float s = 0.f, m = -INFINITY;
    int a = 0;
    for (int c = 0; c < 16; ++c) {
        const float v = x[((long long)b * 16 + c) * HW + p] * gate[b * 16 + c];
        s += v;
        if (v > m) { m = v; a = c; }
    }
    sp[((long long)b * 2) * HW + p] = s / 16.0f;
    sp[((long long)b * 2 + 1) * HW + p] = m;
    am[(long long)b * HW + p] = (unsigned char)a;
}

// xs = (x gate[c]) sg[p]: the conv's input, kept for the backward
FRONT_KERNEL(256) void front_xs_kernel(const float* __restrict__ x, const float* __restrict__ gate, const float* __restrict__ sg, int HW,
                                       float* __restrict__ xs) {
    const int bc = blockIdx.y;                               // b * 16 + c
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    xs[(long long)bc * HW + p] = (x[(long long)bc * HW + p] * gate[bc]) * sg[(long long)(bc >> 4) * HW + p];
}

// ---- feature_compress forward ------------------------------------------------------------------------------------------------------
// z = conv3x3(xs, pad 1) + bias, one thread per pixel and all 8 outputs
FRONT_KERNEL(256) void front_conv_kernel(const float* __restrict__ xs, const float* __restrict__ w, const float* __restrict__ bias, int H, int W,
                                         float* __restrict__ z) {
    __shared__ float sw[1152];
    for (int i = threadIdx.x; i < 1152; i += 256) sw[i] = w[i];
    __syncthreads();
    const int b = blockIdx.y, HW = H * W;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const int y = p / W, x = p - y * W;
    float v[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) v[o] = bias[o];
    for (int c = 0; c < 16; ++c)
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = y + ky - 1;
            if (iy < 0 || iy >= H) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = x + kx - 1;
                if (ix < 0 || ix >= W) continue;
                const float in = xs[((long long)b * 16 + c) * HW + iy * W + ix];
#pragma unroll
                for (int o = 0; o < 8; ++o) v[o] = fmaf(sw[(o * 16 + c) * 9 + ky * 3 + kx], in, v[o]);
            }
        }
#pragma unroll
    for (int o = 0; o < 8; ++o) z[((long long)b * 8 + o) * HW + p] = v[o];
}

// 16 block sums of one chunk (256 pixels of one image): part[chunk][16] = s[0..15], waves added in wave order
__device__ __forceinline__ void chunk_sums_16(const double* v, double* __restrict__ part) {
    __shared__ double red[4][16];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const double s = wave_sum_d(v[i]);
        if (lane == 0) red[wv][i] = s;
    }
    __syncthreads();
    if (threadIdx.x < 16) part[threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// per chunk and channel: sum z, sum z^2 (fp64)
FRONT_KERNEL(256) void front_bn_stats_kernel(const float* __restrict__ z, int HW, double* __restrict__ part) {
    const int b = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
    double v[16];
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        const double t = p < HW ? (double)z[((long long)b * 8 + o) * HW + p] : 0.0;
        v[o] = t; v[8 + o] = t * t;
    }
    chunk_sums_16(v, part + ((long long)b * gridDim.x + blockIdx.x) * 16);
}

// eval-mode fold of BatchNorm, as vt_decoder_finalize computes it on the host (fp32): scale = gamma / sqrt(var + eps), shift = beta - mean scale.
// The host rounds the product mean scale before it subtracts.  The pragma alone does not keep the device from fusing the two into one
// multiply-add (the build's -ffp-contract=fast lets the backend fuse whatever the source says), which made the shift differ by an ulp
// from the one a decoder loaded from the trainer's checkpoint computes; the empty asm pins the rounded product in a register.
__device__ __forceinline__ void bn_fold_one(const float* __restrict__ params, float* __restrict__ bn, int o) {
#pragma clang fp contract(off)
    const float inv = 1.0f / sqrtf(bn[8 + o] + 1e-5f);
    const float sc = params[VT_FRONT_TABLE[VT_FT_BNW].off + o] * inv;
    float prod = bn[o] * sc;
    asm volatile("" : "+v"(prod));
    bn[16 + o] = sc;
    bn[24 + o] = params[VT_FRONT_TABLE[VT_FT_BNB].off + o] - prod;
}
FRONT_KERNEL(64) void front_bn_fold_kernel(const float* __restrict__ params, float* __restrict__ bn) {
    if (threadIdx.x < 8) bn_fold_one(params, bn, threadIdx.x);
}

// chunks in order -> mean, rstd of the batch (biased variance); running statistics with momentum 0.1 and the unbiased variance;
// num_batches_tracked + 1; the eval fold of the new running statistics
FRONT_KERNEL(64) void front_bn_finish_kernel(const double* __restrict__ part, int chunks, double M, const float* __restrict__ params,
                                             float* __restrict__ bn, double* __restrict__ stat) {
#pragma clang fp contract(off)
    const int o = threadIdx.x;
    if (o < 8) {
        double s = 0.0, ss = 0.0;
        for (int i = 0; i < chunks; ++i) { s += part[(long long)i * 16 + o]; ss += part[(long long)i * 16 + 8 + o]; }
        const double mean = s / M;
        double var = ss / M - mean * mean;
        if (var < 0.0) var = 0.0;
        stat[o * 4] = mean;
        stat[o * 4 + 1] = 1.0 / sqrt(var + 1e-5);
        const float unbiased = (float)(var * (M / (M - 1.0)));
        bn[o] = 0.9f * bn[o] + 0.1f * (float)mean;
        bn[8 + o] = 0.9f * bn[8 + o] + 0.1f * unbiased;
        bn_fold_one(params, bn, o);
    }
    if (o == 0) *(long long*)(bn + 32) += 1;
}

// y = relu(gamma xhat + beta), xhat = (z - mean) rstd: the training-mode BatchNorm output, the same expression in forward and backward
__device__ __forceinline__ float bn_xhat(float z, float mean, float rstd) { return (z - mean) * rstd; }

// BatchNorm (batch statistics) + ReLU + AdaptiveAvgPool(8, 8): one wave per (cell, image)
FRONT_KERNEL(64) void front_bn_pool_kernel(const float* __restrict__ z, const double* __restrict__ stat, const float* __restrict__ gamma,
                                           const float* __restrict__ beta, int H, int W, float* __restrict__ pooled) {
    const int cell = blockIdx.x, b = blockIdx.y, HW = H * W;
    const int cy = cell >> 3, cx = cell & 7;
    const int y0 = (cy * H) / 8, y1 = ((cy + 1) * H + 7) / 8;
    const int x0 = (cx * W) / 8, x1 = ((cx + 1) * W + 7) / 8;
    const int cw = x1 - x0, n = (y1 - y0) * cw;
    double acc[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) acc[o] = 0.0;
    for (int i = threadIdx.x; i < n; i += 64) {
        const int p = (y0 + i / cw) * W + x0 + i % cw;
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            const float xh = bn_xhat(z[((long long)b * 8 + o) * HW + p], (float)stat[o * 4], (float)stat[o * 4 + 1]);
            acc[o] += (double)fmaxf(fmaf(xh, gamma[o], beta[o]), 0.f);
        }
    }
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        const double s = wave_sum_d(acc[o]);
        if (threadIdx.x == 0) pooled[((long long)b * 8 + o) * 64 + cell] = (float)(s / (double)n);
    }
}

// ---- self-attention, training mode -------------------------------------------------------------------------------------------------
struct SaParams { const float *ln_w, *ln_b, *q_w, *q_b, *k_w, *k_b, *v_w, *v_b, *o_w, *o_b; };
__host__ __device__ inline SaParams sa_params(const float* base) {
    SaParams p;
    p.ln_w = base + VT_FRONT_TABLE[VT_FT_LNW].off; p.ln_b = base + VT_FRONT_TABLE[VT_FT_LNB].off;
    p.q_w = base + VT_FRONT_TABLE[VT_FT_QW].off; p.q_b = base + VT_FRONT_TABLE[VT_FT_QB].off;
    p.k_w = base + VT_FRONT_TABLE[VT_FT_KW].off; p.k_b = base + VT_FRONT_TABLE[VT_FT_KB].off;
    p.v_w = base + VT_FRONT_TABLE[VT_FT_VW].off; p.v_b = base + VT_FRONT_TABLE[VT_FT_VB].off;
    p.o_w = base + VT_FRONT_TABLE[VT_FT_OW].off; p.o_b = base + VT_FRONT_TABLE[VT_FT_OB].off;
    return p;
}

// token `tok` of image b: LayerNorm (fp64 statistics) and the three projections; k and v go to LDS
__device__ __forceinline__ void sa_project(const float* __restrict__ t, const SaParams& w, int b, int tok, float* xin, float* xh, float* xn,
                                           float* q, float (*sk)[8], float (*sv)[8], double* rstd_out) {
    double mean = 0.0;
#pragma unroll
    for (int e = 0; e < 8; ++e) { xin[e] = t[((long long)b * 8 + e) * 64 + tok]; mean += (double)xin[e]; }
    mean *= 0.125;
    double var = 0.0;
#pragma unroll
    for (int e = 0; e < 8; ++e) { const double d = (double)xin[e] - mean; var += d * d; }
    var *= 0.125;
    const double rstd = 1.0 / sqrt(var + 1e-5);
    *rstd_out = rstd;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        xh[e] = (float)(((double)xin[e] - mean) * rstd);
        xn[e] = fmaf(xh[e], w.ln_w[e], w.ln_b[e]);
    }
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        float aq = w.q_b[o], ak = w.k_b[o], av = w.v_b[o];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            aq = fmaf(w.q_w[o * 8 + e], xn[e], aq);
            ak = fmaf(w.k_w[o * 8 + e], xn[e], ak);
            av = fmaf(w.v_w[o * 8 + e], xn[e], av);
        }
        q[o] = aq; sk[tok][o] = ak; sv[tok][o] = av;
    }
}

template <int HD>
__device__ __forceinline__ float sa_score(const float* q, const float* k, float scale) {
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < HD; ++d) s = fmaf(q[d], k[d], s);
    return s * scale;
}
// the softmax denominator of one query row, summed in fp64 and rounded once: the weights then add up to 1 within an ulp
template <int HD>
__device__ __forceinline__ float sa_denominator(const float* q, const float (*sk)[8], int h, float scale, float m) {
    double den = 0.0;
    for (int j = 0; j < 64; ++j) den += (double)expf(sa_score<HD>(q, &sk[j][h * HD], scale) - m);
    return (float)den;
}
__device__ __forceinline__ bool sa_keep(unsigned long long seed, unsigned long long step, int b, int heads, int h, int i, int j, float p) {
    if (!(p > 0.f)) return true;
    return vt_head_keep(seed, step, VT_FRONT_DROPOUT_LAYER, (((unsigned long long)b * heads + h) * 64 + i) * 64 + j, p);
}

// out[b][e][tok] = out_proj(dropout(softmax(q k^T / sqrt(hd))) v) + t: one token per lane, one workgroup per image
template <int HEADS>
FRONT_KERNEL(64) void front_sa_fwd_kernel(const float* __restrict__ t, const float* __restrict__ params, float p, unsigned long long seed,
                                          unsigned long long step, float* __restrict__ out, unsigned char* __restrict__ mask) {
    constexpr int HD = 8 / HEADS;
    __shared__ float sk[64][8], sv[64][8];
    const SaParams w = sa_params(params);
    const int b = blockIdx.x, tok = threadIdx.x;
    float xin[8], xh[8], xn[8], q[8], att[8];
    double rstd;
    sa_project(t, w, b, tok, xin, xh, xn, q, sk, sv, &rstd);
    __syncthreads();
    const float scale = 1.0f / sqrtf((float)HD), ds = 1.0f / (1.0f - p);
#pragma unroll
    for (int h = 0; h < HEADS; ++h) {
        float m = -INFINITY;
        for (int j = 0; j < 64; ++j) m = fmaxf(m, sa_score<HD>(q + h * HD, &sk[j][h * HD], scale));
        const float den = sa_denominator<HD>(q + h * HD, sk, h, scale, m);
        float o[HD];
#pragma unroll
        for (int d = 0; d < HD; ++d) o[d] = 0.f;
        for (int j = 0; j < 64; ++j) {
            const float pr = expf(sa_score<HD>(q + h * HD, &sk[j][h * HD], scale) - m) / den;
            const bool keep = sa_keep(seed, step, b, HEADS, h, tok, j, p);
            const float pd = keep ? pr * ds : 0.f;
            if (mask) mask[((((long long)b * HEADS + h) * 64 + tok) * 64) + j] = keep ? 1 : 0;
#pragma unroll
            for (int d = 0; d < HD; ++d) o[d] = fmaf(pd, sv[j][h * HD + d], o[d]);
        }
#pragma unroll
        for (int d = 0; d < HD; ++d) att[h * HD + d] = o[d];
    }
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        float a = w.o_b[o];
#pragma unroll
        for (int e = 0; e < 8; ++e) a = fmaf(w.o_w[o * 8 + e], att[e], a);
        out[((long long)b * 8 + o) * 64 + tok] = a + xin[o];
    }
}

// Backward of the above for image b.  dy = d out [b][8][64].  Writes dt[b][8][64] (the gradient of the pooled rows) and the image's row
// of weight-gradient partials part[b][640] (offsets of the self-attention group).  Everything is recomputed from the pooled rows in
// fp64 (the gradients are sums of cancelling terms: softmax rows, LayerNorm, the token sums).  Per head: phase A, lane = query token i,
// fills row i of the 64 x 64 weight matrix P in LDS (row stride 65: lanes hit different banks), its d q and attention output; phase B,
// lane = key token j, reads column j of P for d k and d v, summed over i in ascending order.
template <int HEADS>
FRONT_KERNEL(64) void front_sa_bwd_kernel(const float* __restrict__ t, const float* __restrict__ params, const float* __restrict__ dy, float p,
                                          unsigned long long seed, unsigned long long step, float* __restrict__ dt, float* __restrict__ part) {
    constexpr int HD = 8 / HEADS;
    __shared__ double sk[64][8], sv[64][8], sq[64][8], sda[64][8];
    __shared__ double sP[64 * 65];
    __shared__ double s_row[64];
    const SaParams w = sa_params(params);
    const int b = blockIdx.x, tok = threadIdx.x;
    double xin[8], xh[8], xn[8], q[8], att[8], dout[8], datt[8], dq[8], dk[8], dv[8];
    double mean = 0.0;
#pragma unroll
    for (int e = 0; e < 8; ++e) { xin[e] = (double)t[((long long)b * 8 + e) * 64 + tok]; mean += xin[e]; }
    mean *= 0.125;
    double var = 0.0;
#pragma unroll
    for (int e = 0; e < 8; ++e) { const double d = xin[e] - mean; var += d * d; }
    var *= 0.125;
    const double rstd = 1.0 / sqrt(var + 1e-5);
#pragma unroll
    for (int e = 0; e < 8; ++e) { xh[e] = (xin[e] - mean) * rstd; xn[e] = xh[e] * (double)w.ln_w[e] + (double)w.ln_b[e]; }
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        double aq = (double)w.q_b[o], ak = (double)w.k_b[o], av = (double)w.v_b[o];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            aq += (double)w.q_w[o * 8 + e] * xn[e];
            ak += (double)w.k_w[o * 8 + e] * xn[e];
            av += (double)w.v_w[o * 8 + e] * xn[e];
        }
        q[o] = aq; sq[tok][o] = aq; sk[tok][o] = ak; sv[tok][o] = av;
        dout[o] = (double)dy[((long long)b * 8 + o) * 64 + tok];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        double a = 0.0;
#pragma unroll
        for (int o = 0; o < 8; ++o) a += (double)w.o_w[o * 8 + e] * dout[o];
        datt[e] = a; sda[tok][e] = a; dq[e] = 0.0; dk[e] = 0.0; dv[e] = 0.0; att[e] = 0.0;
    }
    const double scale = 1.0 / sqrt((double)HD), ds = 1.0 / (1.0 - (double)p);
    for (int h = 0; h < HEADS; ++h) {
        __syncthreads();                     // k, v, q, d att are in LDS; the previous head's phase B has read P
        // phase A: row `tok` of P
        double m = -INFINITY;
        for (int j = 0; j < 64; ++j) {
            double sc = 0.0;
#pragma unroll
            for (int d = 0; d < HD; ++d) sc += q[h * HD + d] * sk[j][h * HD + d];
            sc *= scale;
            sP[tok * 65 + j] = sc;
            m = fmax(m, sc);
        }
        double den = 0.0;
        for (int j = 0; j < 64; ++j) { const double e = exp(sP[tok * 65 + j] - m); sP[tok * 65 + j] = e; den += e; }
        double row = 0.0;
        for (int j = 0; j < 64; ++j) {
            const double pr = sP[tok * 65 + j] / den;
            sP[tok * 65 + j] = pr;
            const bool keep = sa_keep(seed, step, b, HEADS, h, tok, j, p);
            double dpd = 0.0;
#pragma unroll
            for (int d = 0; d < HD; ++d) dpd += datt[h * HD + d] * sv[j][h * HD + d];
            if (keep) {
                row += pr * dpd * ds;
#pragma unroll
                for (int d = 0; d < HD; ++d) att[h * HD + d] += pr * ds * sv[j][h * HD + d];
            }
        }
        for (int j = 0; j < 64; ++j) {
            const bool keep = sa_keep(seed, step, b, HEADS, h, tok, j, p);
            double dpd = 0.0;
#pragma unroll
            for (int d = 0; d < HD; ++d) dpd += datt[h * HD + d] * sv[j][h * HD + d];
            const double dsc = sP[tok * 65 + j] * ((keep ? dpd * ds : 0.0) - row) * scale;
#pragma unroll
            for (int d = 0; d < HD; ++d) dq[h * HD + d] += dsc * sk[j][h * HD + d];
        }
        s_row[tok] = row;
        __syncthreads();
        // phase B: column `tok` of P
        for (int i = 0; i < 64; ++i) {
            const double pr = sP[i * 65 + tok];
            const bool keep = sa_keep(seed, step, b, HEADS, h, i, tok, p);
            double dpd = 0.0;
#pragma unroll
            for (int d = 0; d < HD; ++d) dpd += sda[i][h * HD + d] * sv[tok][h * HD + d];
            const double dsc = pr * ((keep ? dpd * ds : 0.0) - s_row[i]) * scale;
            const double pd = keep ? pr * ds : 0.0;
#pragma unroll
            for (int d = 0; d < HD; ++d) {
                dk[h * HD + d] += dsc * sq[i][h * HD + d];
                dv[h * HD + d] += pd * sda[i][h * HD + d];
            }
        }
    }
    // back through the projections and LayerNorm
    double dxn[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        double a = 0.0;
#pragma unroll
        for (int o = 0; o < 8; ++o) a += (double)w.q_w[o * 8 + e] * dq[o] + (double)w.k_w[o * 8 + e] * dk[o] + (double)w.v_w[o * 8 + e] * dv[o];
        dxn[e] = a;
    }
    double m1 = 0.0, m2 = 0.0;
#pragma unroll
    for (int e = 0; e < 8; ++e) { const double tg = dxn[e] * (double)w.ln_w[e]; m1 += tg; m2 += tg * xh[e]; }
    m1 *= 0.125; m2 *= 0.125;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const double tg = dxn[e] * (double)w.ln_w[e];
        dt[((long long)b * 8 + e) * 64 + tok] = (float)(dout[e] + rstd * (tg - m1 - xh[e] * m2));
    }
    // weight-gradient partials of this image: sums over its 64 tokens
    float* row = part + (long long)b * 640;
    const bool lead = tok == 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const double a = wave_sum_d(dxn[e] * xh[e]), c = wave_sum_d(dxn[e]);
        const double sqb = wave_sum_d(dq[e]), skb = wave_sum_d(dk[e]), svb = wave_sum_d(dv[e]), sob = wave_sum_d(dout[e]);
        if (lead) {
            row[SA_ROW<VT_FT_LNW> + e] = (float)a; row[SA_ROW<VT_FT_LNB> + e] = (float)c; row[SA_ROW<VT_FT_QB> + e] = (float)sqb; row[SA_ROW<VT_FT_KB> + e] = (float)skb;
            row[SA_ROW<VT_FT_VB> + e] = (float)svb; row[SA_ROW<VT_FT_OB> + e] = (float)sob;
        }
    }
#pragma unroll
    for (int o = 0; o < 8; ++o)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const double a = wave_sum_d(dq[o] * xn[e]), c = wave_sum_d(dk[o] * xn[e]), d = wave_sum_d(dv[o] * xn[e]), f = wave_sum_d(dout[o] * att[e]);
            if (lead) {
                row[SA_ROW<VT_FT_QW> + o * 8 + e] = (float)a; row[SA_ROW<VT_FT_KW> + o * 8 + e] = (float)c; row[SA_ROW<VT_FT_VW> + o * 8 + e] = (float)d;
                row[SA_ROW<VT_FT_OW> + o * 8 + e] = (float)f;
            }
        }
}

// ---- pool / ReLU / BatchNorm backward ----------------------------------------------------------------------------------------------
// g[o] = d(BatchNorm output) at pixel (y, x): every pool window [floor(i H / 8), ceil((i + 1) H / 8)) that contains the pixel gives
// dpool / (window size); ReLU passes it where the output is > 0 (derivative 0 at exactly 0).  xh[o] = the normalised z.
__device__ __forceinline__ void bn_out_grad(const float* __restrict__ dpool, const float* __restrict__ z, const double* __restrict__ stat,
                                            const float* __restrict__ gamma, const float* __restrict__ beta, int b, int y, int x, int H, int W,
                                            float* g, float* xh) {
    const int HW = H * W;
#pragma unroll
    for (int o = 0; o < 8; ++o) g[o] = 0.f;
    for (int cy = 0; cy < 8; ++cy) {
        const int y0 = (cy * H) / 8, y1 = ((cy + 1) * H + 7) / 8;
        if (y < y0 || y >= y1) continue;
        for (int cx = 0; cx < 8; ++cx) {
            const int x0 = (cx * W) / 8, x1 = ((cx + 1) * W + 7) / 8;
            if (x < x0 || x >= x1) continue;
            const float n = (float)((y1 - y0) * (x1 - x0));
#pragma unroll
            for (int o = 0; o < 8; ++o) g[o] += dpool[((long long)b * 8 + o) * 64 + cy * 8 + cx] / n;
        }
    }
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        xh[o] = bn_xhat(z[((long long)b * 8 + o) * HW + y * W + x], (float)stat[o * 4], (float)stat[o * 4 + 1]);
        if (!(fmaf(xh[o], gamma[o], beta[o]) > 0.f)) g[o] = 0.f;
    }
}

// per chunk and channel: sum g, sum g xhat (fp64)
FRONT_KERNEL(256) void front_bn_bwd_stats_kernel(const float* __restrict__ dpool, const float* __restrict__ z, const double* __restrict__ stat,
                                                 const float* __restrict__ gamma, const float* __restrict__ beta, int H, int W,
                                                 double* __restrict__ part) {
    const int b = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
    double v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = 0.0;
    if (p < H * W) {
        float g[8], xh[8];
        bn_out_grad(dpool, z, stat, gamma, beta, b, p / W, p % W, H, W, g, xh);
#pragma unroll
        for (int o = 0; o < 8; ++o) { v[o] = (double)g[o]; v[8 + o] = (double)g[o] * (double)xh[o]; }
    }
    chunk_sums_16(v, part + ((long long)b * gridDim.x + blockIdx.x) * 16);
}

// chunks in order -> stat[o][2] = sum g (d beta), stat[o][3] = sum g xhat (d gamma); both ADDED to the gradients; the group's norm partial
FRONT_KERNEL(64) void front_bn_bwd_finish_kernel(const double* __restrict__ part, int chunks, double* __restrict__ stat, float* __restrict__ grads,
                                                 double* __restrict__ normpart) {
    __shared__ double sq[8];
    const int o = threadIdx.x;
    if (o < 8) {
        double s1 = 0.0, s2 = 0.0;
        for (int i = 0; i < chunks; ++i) { s1 += part[(long long)i * 16 + o]; s2 += part[(long long)i * 16 + 8 + o]; }
        stat[o * 4 + 2] = s1; stat[o * 4 + 3] = s2;
        const float gw = grads[VT_FRONT_TABLE[VT_FT_BNW].off + o] + (float)s2, gb = grads[VT_FRONT_TABLE[VT_FT_BNB].off + o] + (float)s1;
        grads[VT_FRONT_TABLE[VT_FT_BNW].off + o] = gw; grads[VT_FRONT_TABLE[VT_FT_BNB].off + o] = gb;
        sq[o] = (double)gw * (double)gw + (double)gb * (double)gb;
    }
    __syncthreads();
    if (o == 0) {
        double a = 0.0;
        for (int i = 0; i < 8; ++i) a += sq[i];
        normpart[VT_FG_SLOT[VT_FG_BN]] = a;
    }
}

// dz = gamma rstd (g - mean(g) - xhat mean(g xhat)), means over the batch's M = B h w pixels
FRONT_KERNEL(256) void front_bn_bwd_dz_kernel(const float* __restrict__ dpool, const float* __restrict__ z, const double* __restrict__ stat,
                                              const float* __restrict__ gamma, const float* __restrict__ beta, int H, int W, double M,
                                              float* __restrict__ dz) {
    const int b = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x, HW = H * W;
    if (p >= HW) return;
    float g[8], xh[8];
    bn_out_grad(dpool, z, stat, gamma, beta, b, p / W, p % W, H, W, g, xh);
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        const double m1 = stat[o * 4 + 2] / M, m2 = stat[o * 4 + 3] / M;
        dz[((long long)b * 8 + o) * HW + p] = (float)((double)gamma[o] * stat[o * 4 + 1] * ((double)g[o] - m1 - (double)xh[o] * m2));
    }
}

// ---- conv3x3 backward ----------------------------------------------------------------------------------------------------------------
// One workgroup per tile of VT_FRONT_CONV_ROWS rows x 64 columns of one image; thread = gradient entries tid + 256 j of
// { dW[o][c][ky][kx] (1152), db[o] (8) }; each row of the tile is staged in LDS (dz, and xs with its halo), accumulated in registers.
// part[tile][1216]
FRONT_KERNEL(256) void front_conv_dw_kernel(const float* __restrict__ dz, const float* __restrict__ xs, int H, int W, float* __restrict__ part) {
    __shared__ float s_x[16][3][66];
    __shared__ float s_dz[8][64];
    const int tid = threadIdx.x, b = blockIdx.z, HW = H * W;
    const int x0 = blockIdx.x * VT_FRONT_CONV_COLS, yb = blockIdx.y * VT_FRONT_CONV_ROWS;
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};  // (fp64: up to 1024 cancelling terms per entry and tile)
    for (int y = yb; y < yb + VT_FRONT_CONV_ROWS && y < H; ++y) {
        __syncthreads();
        for (int i = tid; i < 8 * 64; i += 256) {
            const int o = i >> 6, xx = x0 + (i & 63);
            s_dz[o][i & 63] = xx < W ? dz[((long long)b * 8 + o) * HW + y * W + xx] : 0.f;
        }
        for (int i = tid; i < 16 * 3 * 66; i += 256) {
            const int c = i / 198, r = (i / 66) % 3, xl = i % 66;
            const int yy = y + r - 1, xx = x0 + xl - 1;
            s_x[c][r][xl] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? xs[((long long)b * 16 + c) * HW + yy * W + xx] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int e = tid + 256 * j;
            if (e < 1152) {
                const int o = e / 144, c = (e / 9) % 16, k = e % 9, ky = k / 3, kx = k % 3;
                double a = acc[j];
                for (int xl = 0; xl < 64; ++xl) a += (double)s_dz[o][xl] * (double)s_x[c][ky][xl + kx];
                acc[j] = a;
            } else if (e < 1160) {
                double a = acc[j];
                for (int xl = 0; xl < 64; ++xl) a += (double)s_dz[e - 1152][xl];
                acc[j] = a;
            }
        }
    }
    const long long tile = ((long long)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int e = tid + 256 * j;
        if (e < 1160) part[tile * 1216 + e] = (float)acc[j];
    }
}

// d xs[c][q] = sum_{o, k} w[o][c][k] dz[o][q - offset(k)]; d sgate = sum_c d xs[c] (x gate[c]); dpre = d sgate sg (1 - sg)
FRONT_KERNEL(256) void front_conv_dx_kernel(const float* __restrict__ dz, const float* __restrict__ w, const float* __restrict__ x,
                                            const float* __restrict__ gate, const float* __restrict__ sg, int H, int W, float* __restrict__ dxs,
                                            float* __restrict__ dpre) {
    __shared__ float sw[1152];
    for (int i = threadIdx.x; i < 1152; i += 256) sw[i] = w[i];
    __syncthreads();
    const int b = blockIdx.y, HW = H * W;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const int y = p / W, xq = p - y * W;
    double d[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) d[c] = 0.0;
    for (int ky = 0; ky < 3; ++ky) {
        const int oy = y - (ky - 1);
        if (oy < 0 || oy >= H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int ox = xq - (kx - 1);
            if (ox < 0 || ox >= W) continue;
            for (int o = 0; o < 8; ++o) {
                const double g = (double)dz[((long long)b * 8 + o) * HW + oy * W + ox];
#pragma unroll
                for (int c = 0; c < 16; ++c) d[c] += (double)sw[(o * 16 + c) * 9 + ky * 3 + kx] * g;
            }
        }
    }
    double dsg = 0.0;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        dxs[((long long)b * 16 + c) * HW + p] = (float)d[c];
        dsg += d[c] * (double)(x[((long long)b * 16 + c) * HW + p] * gate[b * 16 + c]);
    }
    const double s = (double)sg[(long long)b * HW + p];
    dpre[(long long)b * HW + p] = (float)(dsg * s * (1.0 - s));
}

// ---- SpatialAttention backward -----------------------------------------------------------------------------------------------------
// d sp[c2][q] = sum_k w7[c2][k] dpre[q - offset(k)]
FRONT_KERNEL(256) void front_dsp_kernel(const float* __restrict__ dpre, const float* __restrict__ w, int H, int W, float* __restrict__ dsp) {
    __shared__ float sw[98];
    if (threadIdx.x < 98) sw[threadIdx.x] = w[threadIdx.x];
    __syncthreads();
    const int b = blockIdx.y, HW = H * W;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const int y = p / W, x = p - y * W;
    double a0 = 0.0, a1 = 0.0;
    for (int ky = 0; ky < 7; ++ky) {
        const int oy = y - (ky - 3);
        if (oy < 0 || oy >= H) continue;
        for (int kx = 0; kx < 7; ++kx) {
            const int ox = x - (kx - 3);
            if (ox < 0 || ox >= W) continue;
            const double g = (double)dpre[(long long)b * HW + oy * W + ox];
            a0 += (double)sw[ky * 7 + kx] * g;
            a1 += (double)sw[49 + ky * 7 + kx] * g;
        }
    }
    dsp[((long long)b * 2) * HW + p] = (float)a0;
    dsp[((long long)b * 2 + 1) * HW + p] = (float)a1;
}

// d w7[c2][ky][kx] over VT_FRONT_SP_ROWS rows of one image: part[tile][128], thread = one of the 98 entries
FRONT_KERNEL(128) void front_sp7_dw_kernel(const float* __restrict__ dpre, const float* __restrict__ sp, int H, int W, float* __restrict__ part) {
    const int e = threadIdx.x, b = blockIdx.y, HW = H * W;
    if (e >= 98) return;
    const int c2 = e / 49, ky = (e % 49) / 7, kx = e % 7;
    double a = 0.0;
    for (int y = blockIdx.x * VT_FRONT_SP_ROWS; y < (blockIdx.x + 1) * VT_FRONT_SP_ROWS && y < H; ++y) {
        const int iy = y + ky - 3;
        if (iy < 0 || iy >= H) continue;
        const int xa = max(0, 3 - kx), xb = min(W, W + 3 - kx);       // 0 <= x + kx - 3 < W
        for (int x = xa; x < xb; ++x) a += (double)dpre[(long long)b * HW + y * W + x] * (double)sp[((long long)b * 2 + c2) * HW + iy * W + x + kx - 3];
    }
    part[((long long)b * gridDim.x + blockIdx.x) * 128 + e] = (float)a;
}

// d gate[b][c] = sum_q d xc[c][q] x[c][q],  d xc = d xs sg + d sp[0] / 16 + (arg-max channel == c) d sp[1]
FRONT_KERNEL(256) void front_dgate_kernel(const float* __restrict__ dxs, const float* __restrict__ sg, const float* __restrict__ dsp,
                                          const unsigned char* __restrict__ am, const float* __restrict__ x, int HW, double* __restrict__ dgate) {
    __shared__ double red[4];
    const int c = blockIdx.x, b = blockIdx.y;
    double a = 0.0;
    for (int q = threadIdx.x; q < HW; q += 256) {
        float d = dxs[((long long)b * 16 + c) * HW + q] * sg[(long long)b * HW + q] + dsp[((long long)b * 2) * HW + q] * (1.0f / 16.0f);
        if (am[(long long)b * HW + q] == c) d += dsp[((long long)b * 2 + 1) * HW + q];
        a += (double)d * (double)x[((long long)b * 16 + c) * HW + q];
    }
    const double total = block_sum_256d(a, red);
    if (threadIdx.x == 0) dgate[b * 16 + c] = total;
}

// the channel gate's MLP (bias-free 16 -> 2 -> 16, applied to the average and to the max pool) for image b: part[b][128],
// w0[r][i] at r 16 + i, w2[c][r] at its table offset in the group + c 2 + r
FRONT_KERNEL(64) void front_mlp_bwd_kernel(const float* __restrict__ pool, const float* __restrict__ gate, const double* __restrict__ dgate,
                                           const float* __restrict__ w0, const float* __restrict__ w2, float* __restrict__ part) {
    __shared__ double s_h[2][2], s_do[16], s_dh[2];
    const int b = blockIdx.x, t = threadIdx.x;
    if (t < 4) {
        const int which = t >> 1, r = t & 1;
        double h = 0.0;
        for (int i = 0; i < 16; ++i) h += (double)w0[r * 16 + i] * (double)pool[(b * 16 + i) * 2 + which];
        s_h[which][r] = h;                                   // pre-activation
    }
    if (t < 16) { const double g = (double)gate[b * 16 + t]; s_do[t] = dgate[b * 16 + t] * g * (1.0 - g); }
    __syncthreads();
    if (t < 2) {
        double a = 0.0;
        for (int c = 0; c < 16; ++c) a += (double)w2[c * 2 + t] * s_do[c];
        s_dh[t] = a;
    }
    __syncthreads();
    float* row = part + (long long)b * 128;
    if (t < 32) {
        const int r = t >> 4, i = t & 15;
        double a = 0.0;
        for (int which = 0; which < 2; ++which)
            if (s_h[which][r] > 0.0) a += s_dh[r] * (double)pool[(b * 16 + i) * 2 + which];
        row[MLP_ROW<VT_FT_CA0> + t] = (float)a;
    } else {
        const int c = (t - 32) >> 1, r = (t - 32) & 1;
        row[MLP_ROW<VT_FT_CA2> + (t - 32)] = (float)(s_do[c] * (fmax(s_h[0][r], 0.0) + fmax(s_h[1][r], 0.0)));
    }
}

// ---- partials -> gradients ----------------------------------------------------------------------------------------------------------
// grads[e0 + i] += sum over the partial rows in index order (fp64) for the n floats of one group; normpart[slot + blockIdx.x] = the
// sum of squares of what this workgroup wrote
FRONT_KERNEL(256) void front_reduce_kernel(const float* __restrict__ part, int nparts, int stride, int e0, int n, float* __restrict__ grads,
                                           double* __restrict__ normpart, int slot) {
    __shared__ double red[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    double sq = 0.0;
    if (i < n && vt_front_real(e0 + i)) {
        double a = 0.0;
        for (int r = 0; r < nparts; ++r) a += (double)part[(long long)r * stride + i];
        const float g = grads[e0 + i] + (float)a;
        grads[e0 + i] = g;
        sq = (double)g * (double)g;
    }
    const double total = block_sum_256d(sq, red);
    if (threadIdx.x == 0) normpart[slot + blockIdx.x] = total;
}

#define TCKL(c, what) HIPCK(c, hipGetLastError(), what)

int front_check(vt_context* c, const char* who, const void* state, size_t state_bytes, FrontLayout* out) {
    if (!c->dec_finalized) return c->fail(VT_ERR_STATE, "%s: decoder weights not finalized", who);
    if (!vt_front_trainable(c->dec))
        return c->fail(VT_ERR_INVALID, "%s: the front of this decoder cannot be trained on the device (attention decoder at latent_channels 16, "
                                       "heads in {1, 2, 4, 8} expected)", who);
    *out = vt_front_layout(c->dec);
    return vt_train_check(c, who, *out, state, state_bytes);
}

int front_check_batch(vt_context* c, const char* who, const FrontLayout& l, const void* latent, int B, int h, int w, const void* ws, size_t ws_bytes) {
    if (!latent || ((uintptr_t)latent & 3)) return c->fail(VT_ERR_INVALID, "%s: latent is null or misaligned", who);
    if (B <= 0 || B > VT_FRONT_MAX_B || h <= 0 || w <= 0 || (long long)h * w > (1 << 24))
        return c->fail(VT_ERR_INVALID, "%s: B = %d, h = %d, w = %d out of range", who, B, h, w);
    if (!ws || ((uintptr_t)ws & (ALIGN - 1))) return c->fail(VT_ERR_INVALID, "%s: workspace is null or not 256-B aligned", who);
    const size_t need = vt_front_workspace(l, B, h, w).total;
    if (ws_bytes < need) return c->fail(VT_ERR_WORKSPACE, "%s: workspace holds %zu bytes, %zu needed", who, ws_bytes, need);
    return VT_OK;
}

// the context's table entry of tensor t
const float** front_ctx_slot(DecoderWeights& d, int t) {
    switch (t) {
        case VT_FT_CA0: return &d.ca_w0; case VT_FT_CA2: return &d.ca_w2; case VT_FT_SP7: return &d.sa_w;
        case VT_FT_FCW: return &d.fc_w; case VT_FT_FCB: return &d.fc_b; case VT_FT_BNW: return &d.bn_w; case VT_FT_BNB: return &d.bn_b;
        case VT_FT_LNW: return &d.sa.ln_w; case VT_FT_LNB: return &d.sa.ln_b; case VT_FT_QW: return &d.sa.q_w; case VT_FT_QB: return &d.sa.q_b;
        case VT_FT_KW: return &d.sa.k_w; case VT_FT_KB: return &d.sa.k_b; case VT_FT_VW: return &d.sa.v_w; case VT_FT_VB: return &d.sa.v_b;
        case VT_FT_OW: return &d.sa.o_w; default: return &d.sa.o_b;
    }
}

int front_find(vt_context* c, const char* who, const FrontLayout& l, const char* name) {
    for (int i = 0; i < VT_FRONT_TENSORS; ++i)
        if (l.present(i) && name && strcmp(VT_FRONT_TABLE[i].name, name) == 0) return i;
    c->fail(VT_ERR_INVALID, "%s: no front parameter named %s", who, name ? name : "(null)");
    return -1;
}

int front_fold(vt_context* c, const FrontLayout& l, char* st, hipStream_t s) {
    hipLaunchKernelGGL(front_bn_fold_kernel, dim3(1), dim3(64), 0, s, (const float*)(st + l.params), (float*)(st + l.bn)); TCKL(c, "front fold");
    return VT_OK;
}

template <class... A>
void launch_sa_fwd(int heads, dim3 g, hipStream_t s, A... a) {
    switch (heads) {
        case 1: hipLaunchKernelGGL(front_sa_fwd_kernel<1>, g, dim3(64), 0, s, a...); break;
        case 2: hipLaunchKernelGGL(front_sa_fwd_kernel<2>, g, dim3(64), 0, s, a...); break;
        case 4: hipLaunchKernelGGL(front_sa_fwd_kernel<4>, g, dim3(64), 0, s, a...); break;
        default: hipLaunchKernelGGL(front_sa_fwd_kernel<8>, g, dim3(64), 0, s, a...); break;
    }
}
template <class... A>
void launch_sa_bwd(int heads, dim3 g, hipStream_t s, A... a) {
    switch (heads) {
        case 1: hipLaunchKernelGGL(front_sa_bwd_kernel<1>, g, dim3(64), 0, s, a...); break;
        case 2: hipLaunchKernelGGL(front_sa_bwd_kernel<2>, g, dim3(64), 0, s, a...); break;
        case 4: hipLaunchKernelGGL(front_sa_bwd_kernel<4>, g, dim3(64), 0, s, a...); break;
        default: hipLaunchKernelGGL(front_sa_bwd_kernel<8>, g, dim3(64), 0, s, a...); break;
    }
}

}  // namespace

extern "C" {

size_t vt_front_state_bytes(const vt_context* c) {
    if (!c || !c->dec_configured || !vt_front_trainable(c->dec)) return 0;
    return vt_front_layout(c->dec).total;
}

size_t vt_front_workspace_bytes(const vt_context* c, int B, int h, int w) {
    if (!c || !c->dec_configured || !vt_front_trainable(c->dec) || B <= 0 || B > VT_FRONT_MAX_B || h <= 0 || w <= 0 || (long long)h * w > (1 << 24)) return 0;
    return vt_front_workspace(vt_front_layout(c->dec), B, h, w).total;
}

int vt_front_init(vt_context* c, void* state, size_t state_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    FrontLayout l;
    VTCK(front_check(c, "vt_front_init", state, state_bytes, &l));
    hipStream_t s = (hipStream_t)stream;
    char* st = (char*)state;
    HIPCK(c, hipMemsetAsync(state, 0, l.total, s), "front_init clear");
    for (int i = 0; i < VT_FRONT_TENSORS; ++i)
        if (l.present(i))
            HIPCK(c, hipMemcpyAsync((float*)(st + l.params) + VT_FRONT_TABLE[i].off, *front_ctx_slot(c->dec, i), 4 * (size_t)VT_FRONT_TABLE[i].numel,
                                    hipMemcpyDeviceToDevice, s), "front_init copy");
    float* bn = (float*)(st + l.bn);
    HIPCK(c, hipMemcpyAsync(bn, c->dec.bn_mean, 32, hipMemcpyDeviceToDevice, s), "front_init copy");
    HIPCK(c, hipMemcpyAsync(bn + 8, c->dec.bn_var, 32, hipMemcpyDeviceToDevice, s), "front_init copy");
    HIPCK(c, hipMemcpyAsync(bn + 16, c->dec.bn_scale, 32, hipMemcpyDeviceToDevice, s), "front_init copy");
    HIPCK(c, hipMemcpyAsync(bn + 24, c->dec.bn_shift, 32, hipMemcpyDeviceToDevice, s), "front_init copy");
    const TrainBlockRef blocks[1] = {{&l, st}};
    return vt_train_clip_blocks(c, "vt_front_init", blocks, 1, 1.0f, s);     // over the zeroed block: norm 0, coefficient 1
}

int vt_front_commit(vt_context* c, const void* state, size_t state_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    FrontLayout l;
    VTCK(front_check(c, "vt_front_commit", state, state_bytes, &l));
    hipStream_t s = (hipStream_t)stream;
    const char* st = (const char*)state;
    for (int i = 0; i < VT_FRONT_TENSORS; ++i)
        if (l.present(i))
            HIPCK(c, hipMemcpyAsync(const_cast<float*>(*front_ctx_slot(c->dec, i)), (const float*)(st + l.params) + VT_FRONT_TABLE[i].off,
                                    4 * (size_t)VT_FRONT_TABLE[i].numel, hipMemcpyDeviceToDevice, s), "front_commit copy");
    const float* bn = (const float*)(st + l.bn);       // the running statistics and the fold dec_compress_kernel reads
    HIPCK(c, hipMemcpyAsync(const_cast<float*>(c->dec.bn_mean), bn, 32, hipMemcpyDeviceToDevice, s), "front_commit copy");
    HIPCK(c, hipMemcpyAsync(const_cast<float*>(c->dec.bn_var), bn + 8, 32, hipMemcpyDeviceToDevice, s), "front_commit copy");
    HIPCK(c, hipMemcpyAsync(const_cast<float*>(c->dec.bn_scale), bn + 16, 32, hipMemcpyDeviceToDevice, s), "front_commit copy");
    HIPCK(c, hipMemcpyAsync(const_cast<float*>(c->dec.bn_shift), bn + 24, 32, hipMemcpyDeviceToDevice, s), "front_commit copy");
    return VT_OK;
}

int vt_front_forward(vt_context* c, void* state, size_t state_bytes, const float* latent, int B, int h, int w, int train, float attention_dropout,
                     unsigned long long seed, unsigned long long step, float* features_out, unsigned char* mask_out, void* ws, size_t ws_bytes,
                     void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    FrontLayout l;
    VTCK(front_check(c, "vt_front_forward", state, state_bytes, &l));
    VTCK(front_check_batch(c, "vt_front_forward", l, latent, B, h, w, ws, ws_bytes));
    if (!features_out) return c->fail(VT_ERR_INVALID, "vt_front_forward: features_out is null");
    if (!(attention_dropout >= 0.f && attention_dropout < 1.f)) return c->fail(VT_ERR_INVALID, "vt_front_forward: dropout rate %g outside [0, 1)", attention_dropout);
    const FrontWorkspace k = vt_front_workspace(l, B, h, w);
    hipStream_t s = (hipStream_t)stream;
    char* st = (char*)state;
    char* wsb = (char*)ws;
    const float* P = (const float*)(st + l.params);
    float* bn = (float*)(st + l.bn);
    auto T = [&](int t) { return P + VT_FRONT_TABLE[t].off; };
    if (!train) {
        // the inference front on the state's tensors
        DecoderWeights d = c->dec;
        for (int i = 0; i < VT_FRONT_TENSORS; ++i)
            if (l.present(i)) *front_ctx_slot(d, i) = T(i);
        d.bn_scale = bn + 16; d.bn_shift = bn + 24;
        d.use_cross = 0;                              // the front ends in front of cross-attention (vt_cross_forward runs that piece)
        HIPCK(c, vt_decoder_front(d, latent, B, h, w, (float*)(wsb + k.eval), features_out, s), "decoder_front");
        return VT_OK;
    }
    const int HW = h * w;
    const double M = (double)B * (double)HW;
    if (B * (long long)HW < 2) return c->fail(VT_ERR_INVALID, "vt_front_forward: batch statistics need more than one value per channel");
    const dim3 px((HW + 255) / 256, B);
    const float* xs = latent;
    if (l.use_spatial) {
        float* pool = (float*)(wsb + k.pool); float* gate = (float*)(wsb + k.gate); float* sp = (float*)(wsb + k.sp); float* sg = (float*)(wsb + k.sg);
        HIPCK(c, vt_dec_pool(latent, B, 16, HW, pool, s), "front pool");
        HIPCK(c, vt_dec_gate(pool, T(VT_FT_CA0), T(VT_FT_CA2), B, 16, 2, gate, s), "front gate");
        hipLaunchKernelGGL(front_spmap_kernel, px, dim3(256), 0, s, latent, gate, HW, sp, (unsigned char*)(wsb + k.am)); TCKL(c, "front spmap");
        HIPCK(c, vt_dec_sgate(sp, T(VT_FT_SP7), B, h, w, sg, s), "front sgate");
        hipLaunchKernelGGL(front_xs_kernel, dim3((HW + 255) / 256, B * 16), dim3(256), 0, s, latent, gate, sg, HW, (float*)(wsb + k.xs)); TCKL(c, "front xs");
        xs = (const float*)(wsb + k.xs);
    }
    float* z = (float*)(wsb + k.z);
    double* stat = (double*)(wsb + k.bnstat);
    hipLaunchKernelGGL(front_conv_kernel, px, dim3(256), 0, s, xs, T(VT_FT_FCW), T(VT_FT_FCB), h, w, z); TCKL(c, "front conv");
    hipLaunchKernelGGL(front_bn_stats_kernel, px, dim3(256), 0, s, z, HW, (double*)(wsb + k.bnpart)); TCKL(c, "front bn stats");
    hipLaunchKernelGGL(front_bn_finish_kernel, dim3(1), dim3(64), 0, s, (const double*)(wsb + k.bnpart), k.chunks, M, P, bn, stat); TCKL(c, "front bn finish");
    float* pooled = l.use_self ? (float*)(wsb + k.tin) : features_out;
    hipLaunchKernelGGL(front_bn_pool_kernel, dim3(64, B), dim3(64), 0, s, z, stat, T(VT_FT_BNW), T(VT_FT_BNB), h, w, pooled); TCKL(c, "front bn pool");
    if (l.use_self) {
        launch_sa_fwd(l.heads, dim3(B), s, (const float*)pooled, P, attention_dropout, seed, step, features_out, mask_out); TCKL(c, "front self-attention");
    }
    return VT_OK;
}

int vt_front_backward(vt_context* c, void* state, size_t state_bytes, const float* latent, const float* d_features, int B, int h, int w,
                      float attention_dropout, unsigned long long seed, unsigned long long step, void* ws, size_t ws_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    FrontLayout l;
    VTCK(front_check(c, "vt_front_backward", state, state_bytes, &l));
    VTCK(front_check_batch(c, "vt_front_backward", l, latent, B, h, w, ws, ws_bytes));
    if (!d_features || ((uintptr_t)d_features & 3)) return c->fail(VT_ERR_INVALID, "vt_front_backward: d_features is null or misaligned");
    if (!(attention_dropout >= 0.f && attention_dropout < 1.f)) return c->fail(VT_ERR_INVALID, "vt_front_backward: dropout rate %g outside [0, 1)", attention_dropout);
    const FrontWorkspace k = vt_front_workspace(l, B, h, w);
    hipStream_t s = (hipStream_t)stream;
    char* st = (char*)state;
    char* wsb = (char*)ws;
    const float* P = (const float*)(st + l.params);
    float* G = (float*)(st + l.grads);
    double* normpart = (double*)(st + l.normpart);
    auto T = [&](int t) { return P + VT_FRONT_TABLE[t].off; };
    const int HW = h * w;
    const double M = (double)B * (double)HW;
    const dim3 px((HW + 255) / 256, B);
    auto reduce = [&](int group, const float* part, int nparts, int stride) {
        const int n = VT_FG_END[group] - VT_FG_START[group];
        hipLaunchKernelGGL(front_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, s, part, nparts, stride, VT_FG_START[group], n, G, normpart,
                           VT_FG_SLOT[group]);
    };
    const float* dpool = d_features;
    if (l.use_self) {
        float* psa = (float*)(wsb + k.p_sa);
        launch_sa_bwd(l.heads, dim3(B), s, (const float*)(wsb + k.tin), P, d_features, attention_dropout, seed, step, (float*)(wsb + k.dpool), psa);
        TCKL(c, "front self-attention backward");
        reduce(VT_FG_SA, psa, B, 640); TCKL(c, "front self-attention reduce");
        dpool = (const float*)(wsb + k.dpool);
    }
    const float* z = (const float*)(wsb + k.z);
    double* stat = (double*)(wsb + k.bnstat);
    double* bpart = (double*)(wsb + k.bnpart);
    float* dz = (float*)(wsb + k.dz);
    hipLaunchKernelGGL(front_bn_bwd_stats_kernel, px, dim3(256), 0, s, dpool, z, stat, T(VT_FT_BNW), T(VT_FT_BNB), h, w, bpart); TCKL(c, "front bn backward stats");
    hipLaunchKernelGGL(front_bn_bwd_finish_kernel, dim3(1), dim3(64), 0, s, (const double*)bpart, k.chunks, stat, G, normpart); TCKL(c, "front bn backward finish");
    hipLaunchKernelGGL(front_bn_bwd_dz_kernel, px, dim3(256), 0, s, dpool, z, stat, T(VT_FT_BNW), T(VT_FT_BNB), h, w, M, dz); TCKL(c, "front bn backward");
    const float* xs = l.use_spatial ? (const float*)(wsb + k.xs) : latent;
    float* pconv = (float*)(wsb + k.p_conv);
    const dim3 tiles((w + VT_FRONT_CONV_COLS - 1) / VT_FRONT_CONV_COLS, (h + VT_FRONT_CONV_ROWS - 1) / VT_FRONT_CONV_ROWS, B);
    hipLaunchKernelGGL(front_conv_dw_kernel, tiles, dim3(256), 0, s, (const float*)dz, xs, h, w, pconv); TCKL(c, "front conv backward");
    reduce(VT_FG_CONV, pconv, k.conv_parts, 1216); TCKL(c, "front conv reduce");
    if (l.use_spatial) {
        const float* gate = (const float*)(wsb + k.gate); const float* sg = (const float*)(wsb + k.sg); const float* sp = (const float*)(wsb + k.sp);
        const float* pool = (const float*)(wsb + k.pool);
        float* dxs = (float*)(wsb + k.dxs); float* dpre = (float*)(wsb + k.dpre); float* dsp = (float*)(wsb + k.dsp); double* dgate = (double*)(wsb + k.dgate);
        float* psp = (float*)(wsb + k.p_sp7); float* pmlp = (float*)(wsb + k.p_mlp);
        hipLaunchKernelGGL(front_conv_dx_kernel, px, dim3(256), 0, s, (const float*)dz, T(VT_FT_FCW), latent, gate, sg, h, w, dxs, dpre); TCKL(c, "front conv dx");
        const int rows = (h + VT_FRONT_SP_ROWS - 1) / VT_FRONT_SP_ROWS;
        hipLaunchKernelGGL(front_sp7_dw_kernel, dim3(rows, B), dim3(128), 0, s, (const float*)dpre, sp, h, w, psp); TCKL(c, "front 7x7 backward");
        reduce(VT_FG_SP7, psp, k.sp_parts, 128); TCKL(c, "front 7x7 reduce");
        hipLaunchKernelGGL(front_dsp_kernel, px, dim3(256), 0, s, (const float*)dpre, T(VT_FT_SP7), h, w, dsp); TCKL(c, "front dsp");
        hipLaunchKernelGGL(front_dgate_kernel, dim3(16, B), dim3(256), 0, s, (const float*)dxs, sg, (const float*)dsp,
                           (const unsigned char*)(wsb + k.am), latent, HW, dgate); TCKL(c, "front dgate");
        hipLaunchKernelGGL(front_mlp_bwd_kernel, dim3(B), dim3(64), 0, s, pool, gate, (const double*)dgate, T(VT_FT_CA0), T(VT_FT_CA2), pmlp); TCKL(c, "front mlp backward");
        reduce(VT_FG_MLP, pmlp, B, 128); TCKL(c, "front mlp reduce");
    }
    return VT_OK;
}

int vt_front_step(vt_context* c, void* state, size_t state_bytes, double lr, double beta1, double beta2, double eps, double weight_decay, long long t,
                  void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    FrontLayout l;
    VTCK(front_check(c, "vt_front_step", state, state_bytes, &l));
    VTCK(vt_train_step(c, "vt_front_step", l, state, lr, beta1, beta2, eps, weight_decay, t, (hipStream_t)stream));
    return front_fold(c, l, (char*)state, (hipStream_t)stream);
}

// the gradient exchange of a sharded run (vt_train.h)
size_t vt_front_grads_floats(const vt_context* c) {
    return vt_front_state_bytes(c) ? vt_front_layout(c->dec).P : 0;
}

int vt_front_grads_export(vt_context* c, const void* state, size_t state_bytes, void* dst, size_t dst_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    FrontLayout l;
    VTCK(front_check(c, "vt_front_grads_export", state, state_bytes, &l));
    return vt_train_grads_export(c, "vt_front_grads_export", l, state, dst, dst_bytes, (hipStream_t)stream);
}

int vt_front_grads_merge(vt_context* c, void* state, size_t state_bytes, const float* src, size_t stride_floats, int K, const double* weights,
                         void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    FrontLayout l;
    VTCK(front_check(c, "vt_front_grads_merge", state, state_bytes, &l));
    return vt_train_grads_merge(c, "vt_front_grads_merge", l, state, src, stride_floats, K, weights, (hipStream_t)stream);
}

// the front's own kinds (the BatchNorm buffers); the parameter arrays of a named tensor and the scalars are the common layer's
static int front_section(vt_context* c, const char* who, const FrontLayout& l, int kind, const char* name, size_t* off, size_t* bytes) {
    if (kind == VT_FRONT_BN_MEAN) { *off = l.bn; *bytes = 32; return VT_OK; }
    if (kind == VT_FRONT_BN_VAR) { *off = l.bn + 32; *bytes = 32; return VT_OK; }
    if (kind == VT_FRONT_BN_TRACKED) { *off = l.bn + 128; *bytes = 8; return VT_OK; }
    if (kind < VT_HEAD_PARAM || kind > VT_HEAD_ADAM_V) return vt_train_section(c, who, l, kind, 0, 0, off, bytes);    // no tensor is meant
    const int i = front_find(c, who, l, name);
    if (i < 0) return VT_ERR_INVALID;
    return vt_train_section(c, who, l, kind, VT_FRONT_TABLE[i].off, VT_FRONT_TABLE[i].numel, off, bytes);
}

int vt_front_read(vt_context* c, const void* state, size_t state_bytes, int kind, const char* name, void* out, size_t out_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    FrontLayout l;
    VTCK(front_check(c, "vt_front_read", state, state_bytes, &l));
    size_t off = 0, bytes = 0;
    VTCK(front_section(c, "vt_front_read", l, kind, name, &off, &bytes));
    return vt_train_read(c, "vt_front_read", state, off, bytes, out, out_bytes, (hipStream_t)stream);
}

int vt_front_write(vt_context* c, void* state, size_t state_bytes, int kind, const char* name, const void* src, size_t src_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    FrontLayout l;
    VTCK(front_check(c, "vt_front_write", state, state_bytes, &l));
    if (kind == VT_HEAD_NORM) return c->fail(VT_ERR_INVALID, "vt_front_write: kind %d cannot be written", kind);
    size_t off = 0, bytes = 0;
    VTCK(front_section(c, "vt_front_write", l, kind, name, &off, &bytes));
    VTCK(vt_train_write(c, "vt_front_write", state, off, bytes, src, src_bytes, (hipStream_t)stream));
    if (kind == VT_HEAD_PARAM || kind == VT_FRONT_BN_MEAN || kind == VT_FRONT_BN_VAR) return front_fold(c, l, (char*)state, (hipStream_t)stream);
    return VT_OK;
}

}  // extern "C"
