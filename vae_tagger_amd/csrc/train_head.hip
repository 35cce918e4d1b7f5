// Training of the decoder's classifier head on the device: what train_decoder.py's loop body (train_decoder.py:173-216) does to
// `classifier.*` -- forward with dropout, BCE / Focal / class-balanced loss (improved_losses.py:39-72), backward, clip_grad_norm_
// and AdamW -- on one caller-owned state block (vt_train.h) fed FEATURE ROWS [B][F]: the output of the decoder's front
// (vt_decode_features).  Alone, this unit leaves the front frozen (its rows are the same every epoch); the attention decoder's front
// is trained by train_front.hip, which takes d loss / d features from vt_head_forward_backward_dx here.  What the two trainers have in
// common -- the state check, clip over one or both blocks, the AdamW step, the parameter kinds of read / write -- is train_common.hip;
// this file keeps the head's forward, loss and backward and its own kind (the loss ring).  Cross-attention has no backward anywhere.
// fp32 parameters, gradients and moments; fp64 for the loss elements and every scalar reduction.  No atomics: every gradient element
// is owned by one thread, sums over the batch run in ascending row order, sums over workgroups are written as partials and added in
// workgroup order by a later launch -- the order of every sum is a function of the shapes alone, so a given call sequence leaves the
// same bits on every run.  Nothing synchronises the host.
//   forward    vt_dec_linear / vt_dec_ln_act, the launches of vt_decoder_forward (eval mode: the same bits), + the dropout pass
//   loss       head_loss_kernel: loss elements and d loss / d logits, one partial per 64 classes; head_loss_fold_kernel -> ring
//   backward   head_linear_bwd_kernel per linear layer: reads each weight row once for dW (a rank-B update) AND the dX partials, adds
//              into the gradient and takes the squared norm of what it wrote; head_ln_bwd_kernel per hidden layer: adds the dX
//              partials, backs through dropout (same generator), activation and LayerNorm
//   clip, step train_common.hip: partials -> norm, coefficient, scale in place when the coefficient is below 1; decoupled AdamW as
//              torch.optim.AdamW, zeroing the gradients in the same pass
#include <math.h>
#include <string.h>

#include "vt_common.h"
#include "vt_context.h"
#include "vt_train.h"

using namespace vt;

namespace {

constexpr int HB_BT = 16;                   // batch rows of one pass of the backward kernel over its weight rows

// in place: a = keep ? a / (1 - p) : 0   (nn.Dropout in training mode); optionally the mask bytes
__global__ __launch_bounds__(256) void head_dropout_kernel(float* __restrict__ a, long long n, float p, float scale, unsigned long long seed,
                                                           unsigned long long step, int layer, unsigned char* __restrict__ mask) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool keep = vt_head_keep(seed, step, layer, (unsigned long long)i, p);
    a[i] = keep ? a[i] * scale : 0.f;
    if (mask) mask[i] = keep ? 1 : 0;
}

__global__ __launch_bounds__(256) void head_fill_u8_kernel(unsigned char* __restrict__ m, long long n, unsigned char v) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) m[i] = v;
}

__device__ __forceinline__ double label_value(float y) { return (double)y; }
__device__ __forceinline__ double label_value(unsigned char y) { return y ? 1.0 : 0.0; }

// Workgroup = 64 classes x 4 row lanes (eval_loss.hip's shape).  kind 0: bce; 1: alpha (1 - e^-bce)^gamma bce; 2: w[class] bce.
// dy[r][c] = d(mean loss)/d(logit) * gscale, gscale = loss_scale / (B N); partials[blockIdx.x] = the workgroup's sum of loss elements.
template <typename L>
__global__ __launch_bounds__(256) void head_loss_kernel(const float* __restrict__ logits, const L* __restrict__ labels, int B, int N, int kind,
                                                        double alpha, double gamma, const float* __restrict__ cw, double gscale,
                                                        float* __restrict__ dy, double* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ double s_part[4][64];
    const int tid = threadIdx.x, c = tid & 63, g = tid >> 6;
    const int cls = blockIdx.x * 64 + c;
    double sl = 0.0;
    if (cls < N) {
        const double w = kind == 2 ? (double)cw[cls] : 1.0;
        for (int r = g; r < B; r += 4) {
            const long long o = (long long)r * N + cls;
            const double x = (double)logits[o], y = label_value(labels[o]);
            const double e = exp(-fabs(x));
            const double bce = fmax(x, 0.0) - x * y + log1p(e);
            const double sig = x >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
            double l, dl;                    // loss element and d l / d bce
            if (kind == 1) {
                const double pt = exp(-bce), u = 1.0 - pt;
                double ug, ug1;              // u^gamma, gamma u^(gamma - 1)
                if (gamma == 2.0) { ug = u * u; ug1 = 2.0 * u; }
                else if (gamma == 1.0) { ug = u; ug1 = 1.0; }
                else if (gamma == 0.0) { ug = 1.0; ug1 = 0.0; }
                else { ug = pow(u, gamma); ug1 = gamma * pow(u, gamma - 1.0); }
                l = alpha * ug * bce;
                // (u == 0 only where bce == 0: the term's limit is 0 for every gamma; gamma < 1 would give inf x 0 there)
                dl = alpha * ((u > 0.0 ? ug1 * pt * bce : 0.0) + ug);
            } else {
                l = w * bce; dl = w;
            }
            sl += l;
            dy[o] = (float)(dl * (sig - y) * gscale);
        }
    }
    s_part[g][c] = sl;
    __syncthreads();
    if (g != 0) return;
    double t = ((s_part[0][c] + s_part[1][c]) + s_part[2][c]) + s_part[3][c];
    t = wave_sum_d(t);
    if (c == 0) partials[blockIdx.x] = t;
}

// one wave: the partials in workgroup order -> ring[slot] = loss_scale * mean
__global__ __launch_bounds__(64) void head_loss_fold_kernel(const double* __restrict__ partials, int groups, double scale, double* __restrict__ slot) {
#pragma clang fp contract(off)
    double a = 0.0;
    for (int i = threadIdx.x; i < groups; i += 64) a += partials[i];
    a = wave_sum_d(a);
    if (threadIdx.x == 0) *slot = a * scale;
}

// Backward of y = x W^T + b for output rows [g rows, (g + 1) rows) and input columns [256 kb, 256 kb + 256): thread = one column.
//   gW[o][k] += sum_b dz[b][o] x[b][k]         (b ascending, in passes of HB_BT rows)
//   dxpart[g][b][k] = sum_{o in group} dz[b][o] W[o][k]      (o ascending; nullptr: the input needs no gradient)
//   column block 0 also owns the row vectors: gb[o] += sum_b dz[b][o]; with dt: ggam[o] += sum_b dt[b][o] xh[b][o], gbeta[o] += sum_b dt[b][o]
//   normpart[blockIdx.x * gridDim.y + blockIdx.y] = sum of squares (fp64) of every gradient value this workgroup wrote
__global__ __launch_bounds__(256) void head_linear_bwd_kernel(const float* __restrict__ dz, const float* __restrict__ x, const float* __restrict__ W,
                                                              float* __restrict__ gW, float* __restrict__ gb, const float* __restrict__ dt,
                                                              const float* __restrict__ xh, float* __restrict__ ggam, float* __restrict__ gbeta,
                                                              float* __restrict__ dxpart, double* __restrict__ normpart, int B, int K, int OUT,
                                                              int rows) {
    __shared__ double red[4];
    const int tid = threadIdx.x, g = blockIdx.x, k = blockIdx.y * 256 + tid;
    const int o0 = g * rows, o1 = min(OUT, o0 + rows);
    double sq = 0.0;
    for (int b0 = 0; b0 < B; b0 += HB_BT) {
        const int nb = min(HB_BT, B - b0);
        const bool last = b0 + HB_BT >= B;
        float xr[HB_BT], dx[HB_BT];
#pragma unroll
        for (int i = 0; i < HB_BT; ++i) { xr[i] = i < nb ? x[(long long)(b0 + i) * K + k] : 0.f; dx[i] = 0.f; }
        for (int o = o0; o < o1; ++o) {
            const long long wi = (long long)o * K + k;
            const float w = W[wi];
            float dw = 0.f;
#pragma unroll
            for (int i = 0; i < HB_BT; ++i) {
                if (i < nb) {
                    const float d = dz[(long long)(b0 + i) * OUT + o];
                    dx[i] = fmaf(d, w, dx[i]);
                    dw = fmaf(d, xr[i], dw);
                }
            }
            const float gn = gW[wi] + dw;
            gW[wi] = gn;
            if (last) sq += (double)gn * (double)gn;
        }
        if (dxpart) {
#pragma unroll
            for (int i = 0; i < HB_BT; ++i)
                if (i < nb) dxpart[((long long)g * B + b0 + i) * K + k] = dx[i];
        }
    }
    if (blockIdx.y == 0 && tid < o1 - o0) {
        const int o = o0 + tid;
        float sb = 0.f, sg = 0.f, st = 0.f;
        for (int b = 0; b < B; ++b) {
            sb += dz[(long long)b * OUT + o];
            if (dt) { const float t = dt[(long long)b * OUT + o]; sg = fmaf(t, xh[(long long)b * OUT + o], sg); st += t; }
        }
        const float nb_ = gb[o] + sb;
        gb[o] = nb_;
        sq += (double)nb_ * (double)nb_;
        if (dt) {
            const float ng = ggam[o] + sg, nt = gbeta[o] + st;
            ggam[o] = ng; gbeta[o] = nt;
            sq += (double)ng * (double)ng + (double)nt * (double)nt;
        }
    }
    const double total = block_sum_256d(sq, red);
    if (tid == 0) normpart[(long long)blockIdx.x * gridDim.y + blockIdx.y] = total;
}

// One workgroup per batch row of a hidden layer of width D <= 1024: dA = sum of the G dX partials (g ascending), back through dropout
// (the forward's mask, regenerated), the activation (sign of the stored output) and LayerNorm (statistics recomputed from z).
//   dt = grad of the LayerNorm output, xh = (z - mean) rstd, dzo = rstd (dt gamma - mean(dt gamma) - xh mean(dt gamma xh))
__global__ __launch_bounds__(256) void head_ln_bwd_kernel(const float* __restrict__ part, int G, const float* __restrict__ z,
                                                          const float* __restrict__ a, const float* __restrict__ gamma, int B, int D, float slope,
                                                          float p, float scale, unsigned long long seed, unsigned long long step, int layer,
                                                          float* __restrict__ dt, float* __restrict__ xh, float* __restrict__ dzo) {
    __shared__ double red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    float zv[4], tv[4];
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = tid + 256 * j;
        zv[j] = 0.f; tv[j] = 0.f;
        if (k < D) {
            const long long e = (long long)b * D + k;
            float da = 0.f;
            for (int g = 0; g < G; ++g) da += part[((long long)g * B + b) * D + k];
            if (p > 0.f) da = vt_head_keep(seed, step, layer, (unsigned long long)e, p) ? da * scale : 0.f;
            tv[j] = a[e] > 0.f ? da : slope * da;
            zv[j] = z[e];
            s += (double)zv[j];
        }
    }
    const double mean = block_sum_256d(s, red) / (double)D;
    double v = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (tid + 256 * j < D) { const double d = (double)zv[j] - mean; v += d * d; }
    const double var = block_sum_256d(v, red) / (double)D;
    const double rstd = 1.0 / sqrt(var + 1e-5);
    double s1 = 0.0, s2 = 0.0;
    float hv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = tid + 256 * j;
        hv[j] = 0.f;
        if (k < D) {
            hv[j] = (float)(((double)zv[j] - mean) * rstd);
            const double tg = (double)tv[j] * (double)gamma[k];
            s1 += tg; s2 += tg * (double)hv[j];
        }
    }
    const double m1 = block_sum_256d(s1, red) / (double)D;
    const double m2 = block_sum_256d(s2, red) / (double)D;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = tid + 256 * j;
        if (k < D) {
            const long long e = (long long)b * D + k;
            dt[e] = tv[j]; xh[e] = hv[j];
            dzo[e] = (float)(rstd * ((double)tv[j] * (double)gamma[k] - m1 - (double)hv[j] * m2));
        }
    }
}

// d_features[b][k] = sum of the first layer's G dX partials, g ascending
__global__ __launch_bounds__(256) void head_dx_sum_kernel(const float* __restrict__ part, int G, long long n, float* __restrict__ dx) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float a = 0.f;
    for (int g = 0; g < G; ++g) a += part[(long long)g * n + i];
    dx[i] = a;
}

#define TCKL(c, what) HIPCK(c, hipGetLastError(), what)

int head_check(vt_context* c, const char* who, const void* state, size_t state_bytes, HeadLayout* out) {
    if (!c->dec_finalized) return c->fail(VT_ERR_STATE, "%s: decoder weights not finalized", who);
    const DecHeadShape s = vt_decoder_head_shape(c->dec);
    for (int i = 0; i <= s.hidden; ++i)
        if (s.dims[i] % 256) return c->fail(VT_ERR_INVALID, "%s: the head's input widths must be multiples of 256 (one backward thread per column of a 256-column block); this head has %d", who, s.dims[i]);
    *out = vt_head_layout(s);
    return vt_train_check(c, who, *out, state, state_bytes);
}

// the context's table entry of tensor t (a device pointer the context owns)
const float* head_ctx_tensor(const DecoderWeights& d, const HeadTensor& t) {
    const int i = t.module / 4;
    if (t.module % 4 == 0) return t.is_bias ? d.cls_b[i] : d.cls_w[i];
    return t.is_bias ? d.cls_ln_b[i] : d.cls_ln_w[i];
}

DecHeadParams head_params(const HeadLayout& l, const float* base) {
    DecHeadParams p{};
    int n = 0;
    for (int i = 0; i <= l.shape.hidden; ++i) {
        p.w[i] = base + l.t[n++].off; p.b[i] = base + l.t[n++].off;
        if (i < l.shape.hidden) { p.ln_w[i] = base + l.t[n++].off; p.ln_b[i] = base + l.t[n++].off; }
    }
    return p;
}

int head_find(vt_context* c, const char* who, const HeadLayout& l, const char* name) {
    for (int i = 0; i < l.ntensors; ++i) {
        char k[64];
        snprintf(k, sizeof k, "classifier.%d.%s", l.t[i].module, l.t[i].is_bias ? "bias" : "weight");
        if (name && strcmp(k, name) == 0) return i;
    }
    c->fail(VT_ERR_INVALID, "%s: no head parameter named %s", who, name ? name : "(null)");
    return -1;
}

// forward through the head: logits in ws.logits; train: dropout with the given rates (masks optionally written)
int head_forward(vt_context* c, const HeadLayout& l, const char* st, const float* features, int B, const HeadWorkspace& w, char* ws, bool train,
                 const float* drop, unsigned long long seed, unsigned long long step, unsigned char* masks, bool keep_z, hipStream_t s) {
    const DecHeadShape& sh = l.shape;
    const DecHeadParams p = head_params(l, (const float*)(st + l.params));
    const float* x = features;
    for (int i = 0; i < sh.hidden; ++i) {
        const int D = sh.dims[i + 1];
        float* z = (float*)(ws + w.z[i]);
        float* a = (float*)(ws + w.a[i]);
        const long long n = (long long)B * D;
        if (keep_z) {
            HIPCK(c, vt_dec_linear(x, p.w[i], p.b[i], z, B, sh.dims[i], D, s), "head linear");
            HIPCK(c, hipMemcpyAsync(a, z, 4 * (size_t)n, hipMemcpyDeviceToDevice, s), "head copy");
        } else {
            HIPCK(c, vt_dec_linear(x, p.w[i], p.b[i], a, B, sh.dims[i], D, s), "head linear");
        }
        HIPCK(c, vt_dec_ln_act(a, p.ln_w[i], p.ln_b[i], B, D, sh.act, s), "head layer norm");
        const float pd = train && drop ? drop[i] : 0.f;
        if (pd > 0.f) {
            hipLaunchKernelGGL(head_dropout_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, n, pd, 1.0f / (1.0f - pd), seed, step, i, masks);
            TCKL(c, "head dropout");
        } else if (masks) {
            hipLaunchKernelGGL(head_fill_u8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, masks, n, (unsigned char)1); TCKL(c, "head masks");
        }
        if (masks) masks += n;
        x = a;
    }
    HIPCK(c, vt_dec_linear(x, p.w[sh.hidden], p.b[sh.hidden], (float*)(ws + w.logits), B, sh.dims[sh.hidden], sh.dims[sh.hidden + 1], s), "head linear");
    return VT_OK;
}

int head_check_batch(vt_context* c, const char* who, const HeadLayout& l, const void* features, int B, const void* ws, size_t ws_bytes) {
    if (!features || ((uintptr_t)features & 3)) return c->fail(VT_ERR_INVALID, "%s: features are null or misaligned", who);
    if (B <= 0 || B > VT_HEAD_MAX_B) return c->fail(VT_ERR_INVALID, "%s: B = %d outside [1, %d]", who, B, VT_HEAD_MAX_B);
    if (!ws || ((uintptr_t)ws & (ALIGN - 1))) return c->fail(VT_ERR_INVALID, "%s: workspace is null or not 256-B aligned", who);
    const size_t need = vt_head_workspace(l, B).total;
    if (ws_bytes < need) return c->fail(VT_ERR_WORKSPACE, "%s: workspace holds %zu bytes, %zu needed", who, ws_bytes, need);
    return VT_OK;
}

}  // namespace

// vt_train.h: the context's decoder-side blocks in clip order, checked as vt_head_clip / vt_train_clip / vt_train_clip3 check them
int vt_train_decoder_blocks(vt_context* c, const char* who, void* head_state, size_t head_bytes, void* front_state, size_t front_bytes,
                            void* cross_state, size_t cross_bytes, DecoderBlocks* out) {
    VTCK(head_check(c, who, head_state, head_bytes, &out->head));
    out->ref[0] = {&out->head, head_state};
    out->n = 1;
    const bool has_front = front_state || front_bytes, has_cross = cross_state || cross_bytes;
    if (has_cross && !has_front) return c->fail(VT_ERR_INVALID, "%s: a cross-attention block comes with the front's", who);
    if (has_front) {
        if (!vt_front_trainable(c->dec)) return c->fail(VT_ERR_INVALID, "%s: this decoder's front is not trainable", who);
        out->front = vt_front_layout(c->dec);
        VTCK(vt_train_check(c, who, out->front, front_state, front_bytes));
        out->ref[out->n++] = {&out->front, front_state};
    }
    if (has_cross) {
        if (!vt_cross_trainable(c->dec)) return c->fail(VT_ERR_INVALID, "%s: this decoder has no trainable cross-attention", who);
        out->cross = vt_cross_layout(c->dec);
        VTCK(vt_train_check(c, who, out->cross, cross_state, cross_bytes));
        out->ref[out->n++] = {&out->cross, cross_state};
    }
    return VT_OK;
}

extern "C" {

int vt_decoder_feature_dim(const vt_context* c) {
    if (!c || !c->dec_configured) return 0;
    return vt_decoder_head_shape(c->dec).dims[0];
}

int vt_decode_features(vt_context* c, const float* latent, int B, int h, int w, float* features, void* ws, size_t ws_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (!c->dec_finalized) return c->fail(VT_ERR_STATE, "decoder weights not finalized");
    if (!latent || !features || !ws || B <= 0 || h <= 0 || w <= 0) return c->fail(VT_ERR_INVALID, "vt_decode_features: bad argument");
    if (ws_bytes < vt_decode_workspace_bytes(c, B, h, w)) return c->fail(VT_ERR_WORKSPACE, "vt_decode_features: workspace too small");
    HIPCK(c, vt_decoder_front(c->dec, latent, B, h, w, (float*)ws, features, (hipStream_t)stream), "decoder_front");
    return VT_OK;
}

size_t vt_head_state_bytes(const vt_context* c) {
    if (!c || !c->dec_configured) return 0;
    const DecHeadShape s = vt_decoder_head_shape(c->dec);
    for (int i = 0; i <= s.hidden; ++i)
        if (s.dims[i] % 256) return 0;
    return vt_head_layout(s).total;
}

size_t vt_head_workspace_bytes(const vt_context* c, int B) {
    if (!c || !c->dec_configured || B <= 0 || B > VT_HEAD_MAX_B) return 0;
    return vt_head_workspace(vt_head_layout(vt_decoder_head_shape(c->dec)), B).total;
}

int vt_head_init(vt_context* c, void* state, size_t state_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    HeadLayout l;
    VTCK(head_check(c, "vt_head_init", state, state_bytes, &l));
    hipStream_t s = (hipStream_t)stream;
    char* st = (char*)state;
    HIPCK(c, hipMemsetAsync(state, 0, l.total, s), "head_init clear");
    for (int i = 0; i < l.ntensors; ++i)
        HIPCK(c, hipMemcpyAsync((float*)(st + l.params) + l.t[i].off, head_ctx_tensor(c->dec, l.t[i]), 4 * l.t[i].numel, hipMemcpyDeviceToDevice, s),
              "head_init copy");
    const TrainBlockRef blocks[1] = {{&l, st}};
    return vt_train_clip_blocks(c, "vt_head_init", blocks, 1, 1.0f, s);      // over the zeroed block: norm 0, coefficient 1
}

int vt_head_commit(vt_context* c, const void* state, size_t state_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    HeadLayout l;
    VTCK(head_check(c, "vt_head_commit", state, state_bytes, &l));
    const char* st = (const char*)state;
    for (int i = 0; i < l.ntensors; ++i)
        HIPCK(c, hipMemcpyAsync(const_cast<float*>(head_ctx_tensor(c->dec, l.t[i])), (const float*)(st + l.params) + l.t[i].off, 4 * l.t[i].numel,
                                hipMemcpyDeviceToDevice, (hipStream_t)stream), "head_commit copy");
    return VT_OK;
}

int vt_head_forward(vt_context* c, const void* state, size_t state_bytes, const float* features, int B, float* logits_out, void* ws, size_t ws_bytes,
                    void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    HeadLayout l;
    VTCK(head_check(c, "vt_head_forward", state, state_bytes, &l));
    VTCK(head_check_batch(c, "vt_head_forward", l, features, B, ws, ws_bytes));
    if (!logits_out) return c->fail(VT_ERR_INVALID, "vt_head_forward: logits_out is null");
    const HeadWorkspace w = vt_head_workspace(l, B);
    hipStream_t s = (hipStream_t)stream;
    VTCK(head_forward(c, l, (const char*)state, features, B, w, (char*)ws, false, nullptr, 0, 0, nullptr, false, s));
    HIPCK(c, hipMemcpyAsync(logits_out, (char*)ws + w.logits, 4 * (size_t)B * l.shape.dims[l.shape.hidden + 1], hipMemcpyDeviceToDevice, s), "head logits");
    return VT_OK;
}

// vt_head_forward_backward, and with d_features its _dx form: the first layer's dX partials are kept and added in workgroup order
static int head_forward_backward(vt_context* c, void* state, size_t state_bytes, const float* features, const void* labels, int labels_dtype, int B,
                                 int loss_kind, double alpha, double gamma, const float* class_weights, double loss_scale, int train,
                                 const float* dropout_p, unsigned long long seed, unsigned long long step, float* logits_out,
                                 unsigned char* masks_out, float* d_features, void* ws, size_t ws_bytes, void* stream) {
    DeviceGuard guard(c);
    HeadLayout l;
    VTCK(head_check(c, "vt_head_forward_backward", state, state_bytes, &l));
    VTCK(head_check_batch(c, "vt_head_forward_backward", l, features, B, ws, ws_bytes));
    if (!labels || (labels_dtype != VT_F32 && labels_dtype != VT_U8) || (labels_dtype == VT_F32 && ((uintptr_t)labels & 3)))
        return c->fail(VT_ERR_INVALID, "vt_head_forward_backward: labels are null, misaligned, or neither VT_F32 nor VT_U8");
    if (loss_kind < 0 || loss_kind > 2 || (loss_kind == 2 && !class_weights))
        return c->fail(VT_ERR_INVALID, "vt_head_forward_backward: loss_kind %d (0 bce, 1 focal, 2 class-balanced: needs class_weights)", loss_kind);
    if (!isfinite(alpha) || !isfinite(gamma) || gamma < 0.0 || !isfinite(loss_scale))
        return c->fail(VT_ERR_INVALID, "vt_head_forward_backward: alpha, gamma >= 0 and loss_scale must be finite");
    const DecHeadShape& sh = l.shape;
    float drop[3] = {0.f, 0.f, 0.f};
    if (train && dropout_p)
        for (int i = 0; i < sh.hidden; ++i) {
            drop[i] = dropout_p[i];
            if (!(drop[i] >= 0.f && drop[i] < 1.f)) return c->fail(VT_ERR_INVALID, "vt_head_forward_backward: dropout rate %g outside [0, 1)", drop[i]);
        }
    const HeadWorkspace w = vt_head_workspace(l, B);
    hipStream_t s = (hipStream_t)stream;
    char* st = (char*)state;
    char* wsb = (char*)ws;
    const int N = sh.dims[sh.hidden + 1];
    VTCK(head_forward(c, l, st, features, B, w, wsb, train != 0, drop, seed, step, masks_out, true, s));
    float* logits = (float*)(wsb + w.logits);
    if (logits_out) HIPCK(c, hipMemcpyAsync(logits_out, logits, 4 * (size_t)B * N, hipMemcpyDeviceToDevice, s), "head logits");
    // loss and its gradient
    float* dy = (float*)(wsb + w.dy);
    double* lpart = (double*)(wsb + w.losspart);
    const int lgroups = (N + 63) / 64;
    const double denom = (double)B * (double)N;
    if (labels_dtype == VT_U8)
        hipLaunchKernelGGL(head_loss_kernel<unsigned char>, dim3(lgroups), dim3(256), 0, s, logits, (const unsigned char*)labels, B, N, loss_kind, alpha,
                           gamma, class_weights, loss_scale / denom, dy, lpart);
    else
        hipLaunchKernelGGL(head_loss_kernel<float>, dim3(lgroups), dim3(256), 0, s, logits, (const float*)labels, B, N, loss_kind, alpha, gamma,
                           class_weights, loss_scale / denom, dy, lpart);
    TCKL(c, "head loss");
    hipLaunchKernelGGL(head_loss_fold_kernel, dim3(1), dim3(64), 0, s, lpart, lgroups, loss_scale / denom,
                       (double*)(st + l.ring) + (step % VT_HEAD_RING)); TCKL(c, "head loss fold");
    // backward, last layer first
    const DecHeadParams p = head_params(l, (const float*)(st + l.params));
    const DecHeadParams g = head_params(l, (const float*)(st + l.grads));
    double* normpart = (double*)(st + l.normpart);
    float* part = (float*)(wsb + w.part);
    const float* dzl = dy;
    for (int i = sh.hidden; i >= 0; --i) {
        const float* x = i == 0 ? features : (const float*)(wsb + w.a[i - 1]);
        const bool hid = i < sh.hidden;
        hipLaunchKernelGGL(head_linear_bwd_kernel, dim3(l.groups[i], l.kblocks[i]), dim3(256), 0, s, dzl, x, p.w[i], const_cast<float*>(g.w[i]),
                           const_cast<float*>(g.b[i]), hid ? (const float*)(wsb + w.dt[i]) : nullptr, hid ? (const float*)(wsb + w.xh[i]) : nullptr,
                           hid ? const_cast<float*>(g.ln_w[i]) : nullptr, hid ? const_cast<float*>(g.ln_b[i]) : nullptr, i > 0 || d_features ? part : nullptr,
                           normpart + l.part_base[i], B, sh.dims[i], sh.dims[i + 1], vt_head_rows(sh, i)); TCKL(c, "head linear backward");
        if (i == 0) break;
        const int j = i - 1, D = sh.dims[i];            // hidden layer j produced this linear's input
        hipLaunchKernelGGL(head_ln_bwd_kernel, dim3(B), dim3(256), 0, s, part, l.groups[i], (const float*)(wsb + w.z[j]), (const float*)(wsb + w.a[j]),
                           p.ln_w[j], B, D, sh.act == 0 ? 0.f : 0.2f, drop[j], 1.0f / (1.0f - drop[j]), seed, step, j, (float*)(wsb + w.dt[j]),
                           (float*)(wsb + w.xh[j]), (float*)(wsb + w.dz[j])); TCKL(c, "head layer norm backward");
        dzl = (const float*)(wsb + w.dz[j]);
    }
    if (d_features) {
        const long long n = (long long)B * sh.dims[0];
        hipLaunchKernelGGL(head_dx_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, l.groups[0], n, d_features); TCKL(c, "head d features");
    }
    return VT_OK;
}

int vt_head_forward_backward(vt_context* c, void* state, size_t state_bytes, const float* features, const void* labels, int labels_dtype, int B,
                             int loss_kind, double alpha, double gamma, const float* class_weights, double loss_scale, int train,
                             const float* dropout_p, unsigned long long seed, unsigned long long step, float* logits_out, unsigned char* masks_out,
                             void* ws, size_t ws_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    return head_forward_backward(c, state, state_bytes, features, labels, labels_dtype, B, loss_kind, alpha, gamma, class_weights, loss_scale, train,
                                 dropout_p, seed, step, logits_out, masks_out, nullptr, ws, ws_bytes, stream);
}

int vt_head_forward_backward_dx(vt_context* c, void* state, size_t state_bytes, const float* features, const void* labels, int labels_dtype, int B,
                                int loss_kind, double alpha, double gamma, const float* class_weights, double loss_scale, int train,
                                const float* dropout_p, unsigned long long seed, unsigned long long step, float* logits_out,
                                unsigned char* masks_out, float* d_features, void* ws, size_t ws_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    if (!d_features || ((uintptr_t)d_features & 3)) return c->fail(VT_ERR_INVALID, "vt_head_forward_backward_dx: d_features is null or misaligned");
    return head_forward_backward(c, state, state_bytes, features, labels, labels_dtype, B, loss_kind, alpha, gamma, class_weights, loss_scale, train,
                                 dropout_p, seed, step, logits_out, masks_out, d_features, ws, ws_bytes, stream);
}

// clip_grad_norm_ over the head's and the front's gradients together
int vt_train_clip(vt_context* c, void* head_state, size_t head_bytes, void* front_state, size_t front_bytes, float max_norm, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    HeadLayout l;
    VTCK(head_check(c, "vt_train_clip", head_state, head_bytes, &l));
    if (!vt_front_trainable(c->dec)) return c->fail(VT_ERR_INVALID, "vt_train_clip: this decoder's front is not trainable");
    const FrontLayout f = vt_front_layout(c->dec);
    VTCK(vt_train_check(c, "vt_train_clip (front)", f, front_state, front_bytes));
    const TrainBlockRef blocks[2] = {{&l, head_state}, {&f, front_state}};
    return vt_train_clip_blocks(c, "vt_train_clip", blocks, 2, max_norm, (hipStream_t)stream);
}

// the same over the head's, the front's and the cross-attention's gradients
int vt_train_clip3(vt_context* c, void* head_state, size_t head_bytes, void* front_state, size_t front_bytes, void* cross_state, size_t cross_bytes,
                   float max_norm, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    HeadLayout l;
    VTCK(head_check(c, "vt_train_clip3", head_state, head_bytes, &l));
    if (!vt_cross_trainable(c->dec)) return c->fail(VT_ERR_INVALID, "vt_train_clip3: this decoder has no trainable cross-attention");
    const FrontLayout f = vt_front_layout(c->dec);
    const CrossLayout x = vt_cross_layout(c->dec);
    VTCK(vt_train_check(c, "vt_train_clip3 (front)", f, front_state, front_bytes));
    VTCK(vt_train_check(c, "vt_train_clip3 (cross)", x, cross_state, cross_bytes));
    const TrainBlockRef blocks[3] = {{&l, head_state}, {&f, front_state}, {&x, cross_state}};
    return vt_train_clip_blocks(c, "vt_train_clip3", blocks, 3, max_norm, (hipStream_t)stream);
}

int vt_head_clip(vt_context* c, void* state, size_t state_bytes, float max_norm, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    HeadLayout l;
    VTCK(head_check(c, "vt_head_clip", state, state_bytes, &l));
    const TrainBlockRef blocks[1] = {{&l, state}};
    return vt_train_clip_blocks(c, "vt_head_clip", blocks, 1, max_norm, (hipStream_t)stream);
}

int vt_head_step(vt_context* c, void* state, size_t state_bytes, double lr, double beta1, double beta2, double eps, double weight_decay, long long t,
                 void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    HeadLayout l;
    VTCK(head_check(c, "vt_head_step", state, state_bytes, &l));
    return vt_train_step(c, "vt_head_step", l, state, lr, beta1, beta2, eps, weight_decay, t, (hipStream_t)stream);
}

// the gradient exchange of a sharded run (vt_train.h): the floats of the grads section, its copy out, the in-order merge of K ranks'
size_t vt_head_grads_floats(const vt_context* c) {
    return vt_head_state_bytes(c) ? vt_head_layout(vt_decoder_head_shape(c->dec)).P : 0;
}

int vt_head_grads_export(vt_context* c, const void* state, size_t state_bytes, void* dst, size_t dst_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    HeadLayout l;
    VTCK(head_check(c, "vt_head_grads_export", state, state_bytes, &l));
    return vt_train_grads_export(c, "vt_head_grads_export", l, state, dst, dst_bytes, (hipStream_t)stream);
}

int vt_head_grads_merge(vt_context* c, void* state, size_t state_bytes, const float* src, size_t stride_floats, int K, const double* weights,
                        void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    HeadLayout l;
    VTCK(head_check(c, "vt_head_grads_merge", state, state_bytes, &l));
    return vt_train_grads_merge(c, "vt_head_grads_merge", l, state, src, stride_floats, K, weights, (hipStream_t)stream);
}

// the head's own kind (the loss ring); the parameter arrays of a named tensor and the scalars are the common layer's
static int head_section(vt_context* c, const char* who, const HeadLayout& l, int kind, const char* name, size_t* off, size_t* bytes) {
    if (kind == VT_HEAD_LOSS_RING) { *off = l.ring; *bytes = sizeof(double) * VT_HEAD_RING; return VT_OK; }
    if (kind < VT_HEAD_PARAM || kind > VT_HEAD_ADAM_V) return vt_train_section(c, who, l, kind, 0, 0, off, bytes);    // no tensor is meant
    const int i = head_find(c, who, l, name);
    if (i < 0) return VT_ERR_INVALID;
    return vt_train_section(c, who, l, kind, l.t[i].off, l.t[i].numel, off, bytes);
}

int vt_head_read(vt_context* c, const void* state, size_t state_bytes, int kind, const char* name, void* out, size_t out_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    HeadLayout l;
    VTCK(head_check(c, "vt_head_read", state, state_bytes, &l));
    size_t off = 0, bytes = 0;
    VTCK(head_section(c, "vt_head_read", l, kind, name, &off, &bytes));
    return vt_train_read(c, "vt_head_read", state, off, bytes, out, out_bytes, (hipStream_t)stream);
}

int vt_head_write(vt_context* c, void* state, size_t state_bytes, int kind, const char* name, const void* src, size_t src_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    HeadLayout l;
    VTCK(head_check(c, "vt_head_write", state, state_bytes, &l));
    if (kind < VT_HEAD_PARAM || kind > VT_HEAD_ADAM_V) return c->fail(VT_ERR_INVALID, "vt_head_write: kind %d is not a parameter array", kind);
    size_t off = 0, bytes = 0;
    VTCK(head_section(c, "vt_head_write", l, kind, name, &off, &bytes));
    return vt_train_write(c, "vt_head_write", state, off, bytes, src, src_bytes, (hipStream_t)stream);
}

}  // extern "C"
