// The trainers: what every caller-owned state block has and the host layer over it (train_common.hip), then the layouts of the
// classifier head's block and per-call workspace and the dropout generator (train_head.hip), then the front's (train_front.hip) and
// the cross-attention's (train_cross.hip).
// These tables are the only place a layout is written: vae_tagger_amd/train.py goes through vt_*_read / vt_*_write by kind and name
// and mirrors nothing but the 16 bytes of TrainScalars (grad_norm).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "vt_decoder.h"
#include "vt_eval.h"

struct vt_context;

// ---- what every trainer block has ---------------------------------------------------------------------------------------------------
// the scalars of the last clip: fp64 squared norm, fp32 norm, fp32 clip coefficient
struct TrainScalars { double sq; float norm; float coef; };
// byte offsets of the sections (each 256-B aligned) that the shared layer touches, the floats of one parameter array (padded) and the
// number of squared-norm partials (fp64, one per workgroup of the kernels that write gradients)
struct TrainBlock {
    size_t P;
    size_t params, grads, m, v, scalars, normpart, total;
    int norm_parts;
};
// Host layer of train_common.hip; `who` is the entry point the caller was reached through (error messages name it).
int vt_train_check(vt_context* c, const char* who, const TrainBlock& b, const void* state, size_t state_bytes);   // null, alignment, size
// clip_grad_norm_ over n blocks together (1 <= n <= VT_CLIP_MAX_BLOCKS): the squared-norm partials of block 0 in index order, then
// block 1's, ...; one norm and one coefficient, written to every block
constexpr int VT_CLIP_MAX_BLOCKS = 3;
struct TrainBlockRef { const TrainBlock* layout; void* state; };
int vt_train_clip_blocks(vt_context* c, const char* who, const TrainBlockRef* blocks, int n, float max_norm, hipStream_t s);
// the second half of vt_train_clip_blocks on its own: every block's gradients *= the coefficient in its scalars when that is < 1
// (vae_optim.hip's joint clip writes the scalars itself, from the VAE's partials and the blocks')
int vt_train_scale_blocks(vt_context* c, const char* who, const TrainBlockRef* blocks, int n, hipStream_t s);
int vt_train_step(vt_context* c, const char* who, const TrainBlock& b, void* state, double lr, double beta1, double beta2, double eps,
                  double weight_decay, long long t, hipStream_t s);
// The gradient exchange of a sharded run.  export: the block's `grads` section (P floats, padding included) -> dst, device to device.
// merge: grads[e] = (float) sum over ranks r = 0 .. K-1, in that order, of weights[r] * (double)src[r * stride_floats + e] (fp64, multiply
// and add rounded separately; `weights` is a HOST array of K finite, non-negative values; src is 16-B aligned device memory that does
// not overlap the state, stride_floats a multiple of 4 and >= P), and ALL norm_parts squared-norm partials are rewritten from the merged
// fp32 values, so vt_train_clip_blocks and vt_train_step follow unchanged.  The partition of P behind those partials is written here,
// once: partial i is the fp64 sum of squares of float4s [i * chunk4, min((i + 1) * chunk4, P / 4)), chunk4 = ceil((P / 4) / norm_parts);
// a partial whose range is empty is 0.0.
constexpr int VT_MERGE_MAX_RANKS = 64;
inline long long vt_train_merge_chunk4(size_t P, int norm_parts) { return (long long)((P / 4 + (size_t)norm_parts - 1) / (size_t)norm_parts); }
int vt_train_grads_export(vt_context* c, const char* who, const TrainBlock& b, const void* state, void* dst, size_t dst_bytes, hipStream_t s);
int vt_train_grads_merge(vt_context* c, const char* who, const TrainBlock& b, void* state, const void* src, size_t stride_floats, int K,
                         const double* weights, hipStream_t s);
// The per-element AdamW of train_common.hip's block step and of vae_optim.hip's multi-tensor step: one source, so both units compile the
// same arithmetic.  torch.optim.AdamW (single-tensor path): p *= 1 - lr wd; m = lerp(m, g, 1 - beta1); v = beta2 v + (1 - beta2) g g;
// p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps); g = 0
#if defined(__HIPCC__)
__device__ __forceinline__ void adamw_one(float& p, float& g, float& m, float& v, float decay, float w1, float beta2, float w2, float step_size,
                                          float rbc2, float eps) {
#pragma clang fp contract(off)
    p = p * decay;
    m = m + w1 * (g - m);
    v = v * beta2 + w2 * (g * g);
    const float denom = sqrtf(v) / rbc2 + eps;
    p = p - step_size * (m / denom);
    g = 0.f;
}
#endif
// VT_HEAD_PARAM .. VT_HEAD_ADAM_V of the tensor at float offset `toff` with `numel` floats, or VT_HEAD_NORM -> byte range of the block
int vt_train_section(vt_context* c, const char* who, const TrainBlock& b, int kind, size_t toff, size_t numel, size_t* off, size_t* bytes);
int vt_train_read(vt_context* c, const char* who, const void* state, size_t off, size_t bytes, void* out, size_t out_bytes, hipStream_t s);
int vt_train_write(vt_context* c, const char* who, void* state, size_t off, size_t bytes, const void* src, size_t src_bytes, hipStream_t s);

// ---- head trainer (train_head.hip) ----------------------------------------------------------------------------------------------------

constexpr int VT_HEAD_RING = 256;           // per-step loss values kept: slot = step % VT_HEAD_RING
constexpr int VT_HEAD_MAX_B = 4096;
constexpr int VT_HEAD_ROWS_LAST = 32;       // output rows of one backward workgroup, last layer / hidden layers
constexpr int VT_HEAD_ROWS_HIDDEN = 16;
constexpr int VT_HEAD_TENSORS = 14;         // at most 3 x (weight, bias, ln weight, ln bias) + (weight, bias)

// Parameter tensors in state order: per hidden layer i  classifier.{4i}.weight [d(i+1)][d(i)], classifier.{4i}.bias,
// classifier.{4i+1}.weight (LayerNorm), classifier.{4i+1}.bias; then classifier.{4 hidden}.weight [N][d(hidden)] and its bias.
// Every tensor starts on a multiple of 64 floats; the padding stays zero in all four arrays.
struct HeadTensor { int module; int is_bias; size_t off, numel; };      // name = classifier.<module>.<weight|bias>

// One block, every section 256-B aligned:
//   params fp32 [P] | grads fp32 [P] | adam m fp32 [P] | adam v fp32 [P] | scalars { fp64 squared norm, fp32 norm, fp32 clip coefficient } |
//   loss ring fp64 [VT_HEAD_RING] | squared-norm partials fp64 [norm_parts]: one per workgroup of the kernels that write gradients
struct HeadLayout : TrainBlock {
    DecHeadShape shape;
    int ntensors;
    HeadTensor t[VT_HEAD_TENSORS];
    size_t ring;
    int groups[4], kblocks[4], part_base[4]; // backward grid of linear layer l and its first squared-norm partial
};

inline int vt_head_rows(const DecHeadShape& s, int l) { return l == s.hidden ? VT_HEAD_ROWS_LAST : VT_HEAD_ROWS_HIDDEN; }

inline HeadLayout vt_head_layout(const DecHeadShape& s) {
    HeadLayout l;
    l.shape = s;
    size_t off = 0;
    int n = 0;
    auto add = [&](int module, int is_bias, size_t numel) {
        l.t[n].module = module; l.t[n].is_bias = is_bias; l.t[n].off = off; l.t[n].numel = numel;
        off += (numel + 63) / 64 * 64;
        ++n;
    };
    for (int i = 0; i <= s.hidden; ++i) {
        add(4 * i, 0, (size_t)s.dims[i + 1] * s.dims[i]);
        add(4 * i, 1, (size_t)s.dims[i + 1]);
        if (i < s.hidden) { add(4 * i + 1, 0, (size_t)s.dims[i + 1]); add(4 * i + 1, 1, (size_t)s.dims[i + 1]); }
    }
    l.ntensors = n;
    l.P = off;
    l.norm_parts = 0;
    for (int i = 0; i <= s.hidden; ++i) {
        const int rows = vt_head_rows(s, i);
        l.groups[i] = (s.dims[i + 1] + rows - 1) / rows;
        l.kblocks[i] = s.dims[i] / 256;
        l.part_base[i] = l.norm_parts;
        l.norm_parts += l.groups[i] * l.kblocks[i];
    }
    l.params = 0;
    l.grads = l.params + vt_eval_align(4 * l.P);
    l.m = l.grads + vt_eval_align(4 * l.P);
    l.v = l.m + vt_eval_align(4 * l.P);
    l.scalars = l.v + vt_eval_align(4 * l.P);
    l.ring = l.scalars + 256;
    l.normpart = l.ring + vt_eval_align(sizeof(double) * VT_HEAD_RING);
    l.total = l.normpart + vt_eval_align(sizeof(double) * (size_t)l.norm_parts);
    return l;
}

// Workspace of one forward / forward_backward call (floats unless noted), every section 256-B aligned:
//   per hidden layer i: z (the linear's output), a (after LayerNorm, activation, dropout), dt (grad of the LayerNorm output),
//   xh (normalised z), dz (grad of z), each [B][d(i+1)] | logits [B][N] | dy [B][N] | dX partials [max groups][B][K] |
//   loss partials fp64 [ceil(N / 64)]
struct HeadWorkspace { size_t z[3], a[3], dt[3], xh[3], dz[3], logits, dy, part, losspart, total; };
inline HeadWorkspace vt_head_workspace(const HeadLayout& l, int B) {
    const DecHeadShape& s = l.shape;
    HeadWorkspace w;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += vt_eval_align(bytes); return o; };
    for (int i = 0; i < s.hidden; ++i) {
        const size_t n = 4 * (size_t)B * s.dims[i + 1];
        w.z[i] = take(n); w.a[i] = take(n); w.dt[i] = take(n); w.xh[i] = take(n); w.dz[i] = take(n);
    }
    const size_t N = (size_t)s.dims[s.hidden + 1];
    w.logits = take(4 * (size_t)B * N);
    w.dy = take(4 * (size_t)B * N);
    size_t part = 0;
    for (int i = 0; i <= s.hidden; ++i) {                      // (layer 0's are read by vt_head_forward_backward_dx only)
        const size_t p = (size_t)l.groups[i] * B * s.dims[i];
        if (p > part) part = p;
    }
    w.part = take(4 * part);
    w.losspart = take(sizeof(double) * ((N + 63) / 64));
    w.total = off;
    return w;
}

// Dropout: a counter-based generator, no stored state.  Element `idx` of hidden layer `layer` at (seed, step) is KEPT when the top 24
// bits of two rounds of the splitmix64 finaliser over (seed, step) and (layer, idx), as a fraction of 2^24, are >= p.
#if defined(__HIPCC__)
#define VT_TRAIN_HD __host__ __device__
#else
#define VT_TRAIN_HD
#endif
VT_TRAIN_HD inline uint64_t vt_head_mix64(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
VT_TRAIN_HD inline bool vt_head_keep(uint64_t seed, uint64_t step, int layer, uint64_t idx, float p) {
    uint64_t x = vt_head_mix64(seed + 0x9E3779B97F4A7C15ull * (step + 1));
    x = vt_head_mix64(x ^ ((uint64_t)(layer + 1) << 56) ^ idx);
    return (float)(uint32_t)(x >> 40) * (1.0f / 16777216.0f) >= p;
}

// ---- front trainer (train_front.hip): spatial_attention.*, feature_compress.* and self_attention_post.* of the attention decoder ----
// Parameter tensors at FIXED float offsets in each of the four arrays (a tensor of a piece that is switched off keeps its slot, all
// zero); every tensor starts on a multiple of 64 floats and the padding stays zero.  Gradient GROUPS are reduced by one launch each.
constexpr int VT_FRONT_TENSORS = 17;
constexpr int VT_FRONT_P = 2240;            // floats of one parameter array
constexpr int VT_FRONT_NORM_PARTS = 16;     // squared-norm partials: mlp 0 | 7x7 1 | conv 2..6 | batch norm 7 | self-attention 8..10 | 5 spare
constexpr int VT_FRONT_MAX_B = 1024;        // (grids carry B, and B x 16, in their y dimension)
constexpr int VT_FRONT_DROPOUT_LAYER = 8;   // the attention dropout's layer id in vt_head_keep (the head's are 0..2)
struct FrontTensor { const char* name; int off, numel, piece; };     // piece 0: spatial attention, 1: feature_compress, 2: self-attention
constexpr FrontTensor VT_FRONT_TABLE[VT_FRONT_TENSORS] = {
    {"spatial_attention.channel_att.0.weight", 0, 32, 0},   {"spatial_attention.channel_att.2.weight", 64, 32, 0},
    {"spatial_attention.spatial_att.0.weight", 128, 98, 0}, {"feature_compress.0.weight", 256, 1152, 1},
    {"feature_compress.0.bias", 1408, 8, 1},                {"feature_compress.1.weight", 1472, 8, 1},
    {"feature_compress.1.bias", 1536, 8, 1},                {"self_attention_post.norm.weight", 1600, 8, 2},
    {"self_attention_post.norm.bias", 1664, 8, 2},          {"self_attention_post.q_proj.weight", 1728, 64, 2},
    {"self_attention_post.q_proj.bias", 1792, 8, 2},        {"self_attention_post.k_proj.weight", 1856, 64, 2},
    {"self_attention_post.k_proj.bias", 1920, 8, 2},        {"self_attention_post.v_proj.weight", 1984, 64, 2},
    {"self_attention_post.v_proj.bias", 2048, 8, 2},        {"self_attention_post.out_proj.weight", 2112, 64, 2},
    {"self_attention_post.out_proj.bias", 2176, 8, 2},
};
enum { VT_FT_CA0 = 0, VT_FT_CA2, VT_FT_SP7, VT_FT_FCW, VT_FT_FCB, VT_FT_BNW, VT_FT_BNB, VT_FT_LNW, VT_FT_LNB, VT_FT_QW, VT_FT_QB, VT_FT_KW,
       VT_FT_KB, VT_FT_VW, VT_FT_VB, VT_FT_OW, VT_FT_OB };
enum { VT_FG_MLP = 0, VT_FG_SP7 = 1, VT_FG_CONV = 2, VT_FG_BN = 3, VT_FG_SA = 4 };
constexpr int VT_FG_FIRST[5] = {VT_FT_CA0, VT_FT_SP7, VT_FT_FCW, VT_FT_BNW, VT_FT_LNW};     // first tensor of each group
constexpr int VT_FG_START[5] = {0, 128, 256, 1472, 1600};       // first float of each group; the group ends where the next starts
constexpr int VT_FG_END[5] = {128, 256, 1472, 1600, 2240};
constexpr int VT_FG_SLOT[5] = {0, 1, 2, 7, 8};                  // first squared-norm partial of each group
// is float `e` of a parameter array an element of a tensor (not padding)?  always_inline: the kernels that call it carry
// VT_NO_PACKED_F32, a target attribute, and the compiler does not inline a callee whose target attributes differ from its caller's
// unless the callee is always_inline -- without it the kernel makes a real function call per thread.  Inlined, the loop unrolls over
// the constant table into a chain of comparisons against literals.
VT_TRAIN_HD constexpr __attribute__((always_inline)) bool vt_front_real(int e) {
    for (int t = 0; t < VT_FRONT_TENSORS; ++t)
        if (e >= VT_FRONT_TABLE[t].off && e < VT_FRONT_TABLE[t].off + VT_FRONT_TABLE[t].numel) return true;
    return false;
}
// the literals above against the table: a changed offset that they do not follow does not compile
constexpr int vt_fg_blocks(int g) { return (VT_FG_END[g] - VT_FG_START[g] + 255) / 256; }   // workgroups of the group's reduce launch
constexpr bool vt_fg_starts_ok() {
    for (int g = 0; g < 5; ++g)
        if (VT_FG_START[g] != VT_FRONT_TABLE[VT_FG_FIRST[g]].off || VT_FG_END[g] != (g < 4 ? VT_FG_START[g + 1] : VT_FRONT_P)) return false;
    return true;
}
constexpr bool vt_fg_slots_ok() {
    for (int g = 0; g < 5; ++g)
        if (VT_FG_SLOT[g] != (g ? VT_FG_SLOT[g - 1] + vt_fg_blocks(g - 1) : 0)) return false;
    return VT_FG_SLOT[4] + vt_fg_blocks(4) <= VT_FRONT_NORM_PARTS;
}
static_assert(vt_fg_starts_ok(), "a gradient group starts at its first tensor's offset and ends where the next group starts");
static_assert(VT_FRONT_P == VT_FRONT_TABLE[VT_FRONT_TENSORS - 1].off + (VT_FRONT_TABLE[VT_FRONT_TENSORS - 1].numel + 63) / 64 * 64,
              "VT_FRONT_P is the end of the last tensor's 64-float slot");
static_assert(vt_fg_slots_ok(), "VT_FG_SLOT counts one squared-norm partial per reduce workgroup, all inside VT_FRONT_NORM_PARTS");

// One block, every section 256-B aligned:
//   params fp32 [P] | grads | adam m | adam v | batch norm buffers { running_mean fp32 [8], running_var fp32 [8], eval scale fp32 [8],
//   eval shift fp32 [8] (the fold vt_decoder_finalize makes, redone whenever its inputs change), int64 num_batches_tracked at byte 128 } |
//   scalars { fp64 squared norm, fp32 norm, fp32 clip coefficient } | squared-norm partials fp64 [VT_FRONT_NORM_PARTS]
struct FrontLayout : TrainBlock {
    int use_spatial, use_self, heads;
    size_t bn;
    bool present(int t) const { const int p = VT_FRONT_TABLE[t].piece; return p == 1 || (p == 0 ? use_spatial != 0 : use_self != 0); }
};
inline FrontLayout vt_front_layout(const DecoderWeights& d) {
    FrontLayout l;
    l.use_spatial = d.use_spatial; l.use_self = d.use_self; l.heads = d.heads;
    l.P = VT_FRONT_P; l.norm_parts = VT_FRONT_NORM_PARTS;
    const size_t a = vt_eval_align(4 * (size_t)VT_FRONT_P);
    l.params = 0; l.grads = a; l.m = 2 * a; l.v = 3 * a; l.bn = 4 * a;
    l.scalars = l.bn + 256;
    l.normpart = l.scalars + 256;
    l.total = l.normpart + vt_eval_align(sizeof(double) * VT_FRONT_NORM_PARTS);
    return l;
}
// the front can be trained: the attention decoder at latent_channels 16, heads in {1, 2, 4, 8} (with cross-attention the front ends
// in the rows cross-attention reads; that piece is the cross block's, below)
inline bool vt_front_trainable(const DecoderWeights& d) {
    if (d.plain || d.latent_channels != 16) return false;
    return !d.use_self || d.heads == 1 || d.heads == 2 || d.heads == 4 || d.heads == 8;
}

// Workspace of a forward / backward pair (the backward reads what the training-mode forward of the same batch left), every section
// 256-B aligned.  Pixel chunks: 256 pixels of one image (batch-norm partials); conv tiles: 16 rows x 64 columns; 7x7 tiles: 2 rows.
constexpr int VT_FRONT_CONV_ROWS = 16, VT_FRONT_CONV_COLS = 64, VT_FRONT_SP_ROWS = 2;
struct FrontWorkspace {
    size_t eval;                                                     // vt_decoder_front's scratch (train = 0)
    size_t pool, gate, sp, am, sg, xs, z, bnpart, bnstat, tin;      // forward
    size_t dpool, dz, dxs, dpre, dsp, dgate, p_sa, p_conv, p_sp7, p_mlp;   // backward
    int chunks, conv_parts, sp_parts;
    size_t total;
};
inline FrontWorkspace vt_front_workspace(const FrontLayout& l, int B, int H, int W) {
    FrontWorkspace w;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += vt_eval_align(bytes); return o; };
    const size_t HW = (size_t)H * W, b = (size_t)B;
    w.chunks = B * (int)((HW + 255) / 256);
    w.conv_parts = B * ((H + VT_FRONT_CONV_ROWS - 1) / VT_FRONT_CONV_ROWS) * ((W + VT_FRONT_CONV_COLS - 1) / VT_FRONT_CONV_COLS);
    w.sp_parts = B * ((H + VT_FRONT_SP_ROWS - 1) / VT_FRONT_SP_ROWS);
    w.eval = take(4 * vt_decoder_workspace_floats(B, 16, H, W));
    w.pool = take(4 * b * 32); w.gate = take(4 * b * 16); w.sp = take(4 * b * 2 * HW); w.am = take(b * HW); w.sg = take(4 * b * HW);
    w.xs = take(l.use_spatial ? 4 * b * 16 * HW : 0);
    w.z = take(4 * b * 8 * HW);
    w.bnpart = take(sizeof(double) * (size_t)w.chunks * 16);
    w.bnstat = take(sizeof(double) * 32);                            // per channel: mean, rstd, sum dy, sum dy xhat
    w.tin = take(4 * b * 512);
    w.dpool = take(4 * b * 512); w.dz = take(4 * b * 8 * HW);
    w.dxs = take(l.use_spatial ? 4 * b * 16 * HW : 0);
    w.dpre = take(4 * b * HW); w.dsp = take(4 * b * 2 * HW); w.dgate = take(sizeof(double) * b * 16);
    w.p_sa = take(4 * b * 640);
    w.p_conv = take(4 * (size_t)w.conv_parts * 1216);
    w.p_sp7 = take(4 * (size_t)w.sp_parts * 128);
    w.p_mlp = take(4 * b * 128);
    w.total = off;
    return w;
}

// ---- cross-attention trainer (train_cross.hip): query_generator.* and cross_attention.* of the attention decoder ---------------------
// Ten tensors at fixed float offsets in each of the four arrays; every numel is a multiple of 64, so there is no padding.  The weight
// gradients of the three large layers are written by tiles of VT_CROSS_TILE_ROWS rows x VT_CROSS_TILE_COLS columns, one workgroup and
// one squared-norm partial each (the workgroups of column tile 0 also own the bias entries of their rows); k_proj / v_proj (one
// contiguous range of 4608 floats) are reduced from one partial row per image by 256-float workgroups.
constexpr int VT_CROSS_TENSORS = 10;
constexpr int VT_CROSS_P = 530176;          // floats of one parameter array
constexpr int VT_CROSS_TILE_ROWS = 8, VT_CROSS_TILE_COLS = 256;
struct CrossTensor { const char* name; int off, numel; };
constexpr CrossTensor VT_CROSS_TABLE[VT_CROSS_TENSORS] = {
    {"query_generator.weight", 0, 262144},             {"query_generator.bias", 262144, 512},
    {"cross_attention.q_proj.weight", 262656, 131072}, {"cross_attention.q_proj.bias", 393728, 256},
    {"cross_attention.k_proj.weight", 393984, 2048},   {"cross_attention.k_proj.bias", 396032, 256},
    {"cross_attention.v_proj.weight", 396288, 2048},   {"cross_attention.v_proj.bias", 398336, 256},
    {"cross_attention.out_proj.weight", 398592, 131072}, {"cross_attention.out_proj.bias", 529664, 512},
};
enum { VT_CT_GW = 0, VT_CT_GB, VT_CT_QW, VT_CT_QB, VT_CT_KW, VT_CT_KB, VT_CT_VW, VT_CT_VB, VT_CT_OW, VT_CT_OB };
constexpr int VT_CROSS_KV_ROW = 4608;       // floats of one image's partial row: k_proj.weight | k_proj.bias | v_proj.weight | v_proj.bias
constexpr int vt_cross_tiles(int rows, int cols) { return (rows / VT_CROSS_TILE_ROWS) * (cols / VT_CROSS_TILE_COLS); }
// first squared-norm partial of: query_generator [512 x 512] | q_proj [256 x 512] | out_proj [512 x 256] | the k / v range
constexpr int VT_CROSS_SLOT_G = 0;
constexpr int VT_CROSS_SLOT_Q = VT_CROSS_SLOT_G + vt_cross_tiles(512, 512);
constexpr int VT_CROSS_SLOT_O = VT_CROSS_SLOT_Q + vt_cross_tiles(256, 512);
constexpr int VT_CROSS_SLOT_KV = VT_CROSS_SLOT_O + vt_cross_tiles(512, 256);
constexpr int VT_CROSS_NORM_PARTS = VT_CROSS_SLOT_KV + VT_CROSS_KV_ROW / 256;
constexpr bool vt_cross_table_ok() {
    int off = 0;
    for (int t = 0; t < VT_CROSS_TENSORS; ++t) {
        if (VT_CROSS_TABLE[t].off != off || VT_CROSS_TABLE[t].numel % 64) return false;
        off += VT_CROSS_TABLE[t].numel;
    }
    return off == VT_CROSS_P;
}
static_assert(vt_cross_table_ok(), "the cross tensors follow each other without padding and end at VT_CROSS_P");
static_assert(VT_CROSS_TABLE[VT_CT_VB].off + VT_CROSS_TABLE[VT_CT_VB].numel - VT_CROSS_TABLE[VT_CT_KW].off == VT_CROSS_KV_ROW,
              "k_proj and v_proj are one contiguous range of VT_CROSS_KV_ROW floats");
static_assert(VT_CROSS_NORM_PARTS == 274, "one squared-norm partial per workgroup that writes gradients: 128 + 64 + 64 tiles + 18");

// One block, every section 256-B aligned: params fp32 [P] | grads | adam m | adam v | scalars | squared-norm partials fp64
struct CrossLayout : TrainBlock { int heads; };
inline CrossLayout vt_cross_layout(const DecoderWeights& d) {
    CrossLayout l;
    l.heads = d.heads;
    l.P = VT_CROSS_P; l.norm_parts = VT_CROSS_NORM_PARTS;
    const size_t a = vt_eval_align(4 * (size_t)VT_CROSS_P);
    l.params = 0; l.grads = a; l.m = 2 * a; l.v = 3 * a;
    l.scalars = 4 * a;
    l.normpart = l.scalars + 256;
    l.total = l.normpart + vt_eval_align(sizeof(double) * VT_CROSS_NORM_PARTS);
    return l;
}
inline bool vt_cross_trainable(const DecoderWeights& d) { return vt_front_trainable(d) && d.use_cross && (d.heads == 1 || d.heads == 2 || d.heads == 4 || d.heads == 8); }

// Workspace of a forward / backward pair, every section 256-B aligned (floats unless noted).  The forward leaves q (query_generator's
// output), u (q_proj's) and o (the attention output) for the backward of the same batch.
struct CrossWorkspace { size_t q, u, o, a, g, colsum, d_o, du, dq, dt, part, total; };
inline CrossWorkspace vt_cross_workspace(int B) {
    CrossWorkspace w;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += vt_eval_align(bytes); return o; };
    const size_t b = (size_t)B;
    w.q = take(4 * b * 512); w.u = take(4 * b * 256); w.o = take(4 * b * 256); w.a = take(4 * b * 512);
    w.g = take(sizeof(double) * b);                 // fp64 g[b] = sum_f dY[b][f] / 512: every entry of d a
    w.colsum = take(sizeof(double) * 256);          // fp64 column sums of out_proj.weight (one per backward, whatever B)
    w.d_o = take(4 * b * 256); w.du = take(4 * b * 256); w.dq = take(4 * b * 512); w.dt = take(4 * b * 512);
    w.part = take(4 * b * VT_CROSS_KV_ROW);
    w.total = off;
    return w;
}

// ---- the decoder-side blocks of one context, in the order a clip sums them: head, then front, then cross-attention ----------------------
// (train_head.hip) A null pointer with size 0 means the block is absent: the plain decoder has only the head, and the cross-attention's
// block comes with the front's.  Every present block is checked as vt_head_clip / vt_train_clip / vt_train_clip3 check theirs.
struct DecoderBlocks {
    HeadLayout head; FrontLayout front; CrossLayout cross;
    TrainBlockRef ref[VT_CLIP_MAX_BLOCKS];
    int n;
};
int vt_train_decoder_blocks(vt_context* c, const char* who, void* head_state, size_t head_bytes, void* front_state, size_t front_bytes,
                            void* cross_state, size_t cross_bytes, DecoderBlocks* out);
