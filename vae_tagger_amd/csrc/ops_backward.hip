// The vt_op_* backward operators (and vt_op_conv_thin_forward, the data gradient of conv_out): host code over the kernels of conv_wgrad.hip,
// conv_thin_wgrad.hip, conv3x3_s2_dgrad.hip, conv3x3_up2_dgrad.hip and backward_kernels.hip, on caller-owned buffers.
#include "vt_ops.h"

using namespace vt;

extern "C" {

// ---- backward of the resnet block's layers: bf16 operands whatever flag 18 says, fp32 results, no atomics ----

size_t vt_op_cast_bias_grad_workspace_bytes(long long rows, int C) {
    const int chunks = vt_cast_bias_chunks(rows, C);
    return chunks > 0 ? align_up((size_t)chunks * C * sizeof(double)) : 0;
}

int vt_op_cast_bias_grad(vt_context* c, const float* dy, void* dy16, float* dbias, long long rows, int C, void* ws, size_t ws_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (!dy || (!dy16 && !dbias)) return c->fail(VT_ERR_INVALID, "vt_op_cast_bias_grad: null buffer");
    if (rows <= 0 || !vt_cast_bias_supported(C) || vt_cast_bias_chunks(rows, C) <= 0)
        return c->fail(VT_ERR_INVALID, "vt_op_cast_bias_grad: needs rows > 0 and C a multiple of 4, at most 1024 (got rows %lld, C %d)", rows, C);
    if (dbias) VTCK(check_workspace(c, "vt_op_cast_bias_grad", ws, ws_bytes, vt_op_cast_bias_grad_workspace_bytes(rows, C), 16));
    HIPCK(c, vt_launch_cast_bias_grad(dy, (bf16_t*)dy16, dbias, rows, C, (double*)ws, (hipStream_t)stream), "vt_op_cast_bias_grad");
    return VT_OK;
}

// dx = conv(dy16, W'), W'[ci][ky'][kx'][co] = bf16(W[co][ci][2 - ky'][2 - kx']): the forward conv with Cout input and Cin output channels.  The packed
// weights go to the operator scratch behind `keep` bytes the caller has its own use for (the literal routes of the resampling layers).
static int conv_dgrad_launch(vt_context* c, const void* dy16, const float* w_oihw, const float* dx_add, float* dx, int B, int H, int W, int Cin, int Cout,
                             int ksize, size_t keep, hipStream_t s, const char* what) {
    const int taps = ksize * ksize;
    const size_t w_bytes = align_up((size_t)Cin * taps * Cout * 2);
    const bool halo = c->use_halo_conv && ksize == 3 && vt_conv3x3_halo_supported(Cout, Cin);
    VTCK(c->ensure_op_scratch(keep + w_bytes * (halo ? 2 : 1)));
    bf16_t* wt = (bf16_t*)((char*)c->op_scratch + keep);
    HIPCK(c, vt_launch_pack_dgrad_weights(w_oihw, wt, Cin, Cout, ksize, s), "pack_dgrad_weights");
    if (halo) {
        bf16_t* wp = (bf16_t*)((char*)wt + w_bytes);
        HIPCK(c, vt_launch_repack_ohwi_to_halo(wt, wp, Cout, Cin, s), "repack");
        Conv3x3Args h{};
        h.X = (const bf16_t*)dy16; h.Wp = wp; h.res = dx_add; h.out_f32 = dx; h.zeros = c->zeros; h.batch = B; h.H = H; h.W = W; h.Cin = Cout; h.Cout = Cin;
        return launch_halo(c, h, s, what);
    }
    ConvGemmArgs a{};
    a.X = (const bf16_t*)dy16; a.W = wt; a.res = dx_add; a.out_f32 = dx; a.zeros = c->zeros;
    a.Hin = H; a.Win = W; a.Hout = H; a.Wout = W; a.Cin = Cout; a.Cout = Cin; a.Wrows = Cin; a.ksize = ksize; a.stride = 1; a.pad = ksize / 2;
    a.ldx = Cout; a.ldw = taps * Cout; a.ldo = Cin; a.ldr = Cin;
    a.x_bs = (long long)H * W * Cout; a.o_bs = (long long)H * W * Cin; a.r_bs = a.o_bs; a.batch = B; a.alpha = 1.f; a.bias_mode = 0;
    return launch_gemm(c, a, s, what);
}

int vt_op_conv_backward_data(vt_context* c, const void* dy16, const float* w_oihw, const float* dx_add, float* dx, int B, int H, int W, int Cin, int Cout,
                             int ksize, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (!dy16 || !w_oihw || !dx) return c->fail(VT_ERR_INVALID, "vt_op_conv_backward_data: null buffer");
    if (ksize != 1 && ksize != 3) return c->fail(VT_ERR_INVALID, "vt_op_conv_backward_data: ksize must be 1 or 3 (stride 1, pad ksize / 2), got %d", ksize);
    if (B <= 0 || H <= 0 || W <= 0 || Cin < 8 || (Cin % 8) || Cout < 8 || (Cout % 8))
        return c->fail(VT_ERR_INVALID, "vt_op_conv_backward_data: Cin and Cout must be multiples of 8 and B, H, W >= 1 (got %d -> %d, %d x %d x %d)", Cin, Cout, B, H, W);
    return conv_dgrad_launch(c, dy16, w_oihw, dx_add, dx, B, H, W, Cin, Cout, ksize, 0, (hipStream_t)stream, "vt_op_conv_backward_data");
}

size_t vt_op_conv_backward_weight_workspace_bytes(int B, int H, int W, int Cin, int Cout, int ksize, int splits) {
    if (!vt_conv_wgrad_supported(Cin, Cout, ksize) || vt_conv_wgrad_steps(B, H, W) <= 0) return 0;
    const int sp = slice_count(splits, vt_conv_wgrad_steps(B, H, W), vt_conv_wgrad_auto_splits(B, H, W, Cin, Cout));
    return align_up((size_t)sp * Cout * Cin * ksize * ksize * sizeof(float));
}

int vt_op_conv_backward_weight(vt_context* c, const void* dy16, const void* a16, float* dw, int B, int H, int W, int Cin, int Cout, int ksize, int splits,
                               void* ws, size_t ws_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (!dy16 || !a16 || !dw) return c->fail(VT_ERR_INVALID, "vt_op_conv_backward_weight: null buffer");
    if (!vt_conv_wgrad_supported(Cin, Cout, ksize))
        return c->fail(VT_ERR_INVALID, "vt_op_conv_backward_weight: Cin and Cout must be multiples of 64 and ksize 1 or 3 (got %d -> %d, ksize %d)", Cin, Cout, ksize);
    if (B <= 0 || H <= 0 || W <= 0 || vt_conv_wgrad_steps(B, H, W) <= 0) return c->fail(VT_ERR_INVALID, "vt_op_conv_backward_weight: B, H, W must be >= 1");
    if (splits < 0) return c->fail(VT_ERR_INVALID, "vt_op_conv_backward_weight: splits must be >= 0 (0 = chosen from the shape)");
    if ((uintptr_t)dw % 16) return c->fail(VT_ERR_INVALID, "vt_op_conv_backward_weight: dw must be 16-byte aligned");
    VTCK(check_workspace(c, "vt_op_conv_backward_weight", ws, ws_bytes, vt_op_conv_backward_weight_workspace_bytes(B, H, W, Cin, Cout, ksize, splits), 16));
    ConvWgradArgs a{};
    a.dy = (const bf16_t*)dy16; a.a = (const bf16_t*)a16; a.dw = dw; a.ws = (float*)ws; a.batch = B; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.ksize = ksize;
    a.splits = slice_count(splits, vt_conv_wgrad_steps(B, H, W), vt_conv_wgrad_auto_splits(B, H, W, Cin, Cout));
    HIPCK(c, vt_launch_conv_wgrad(a, (hipStream_t)stream), "vt_op_conv_backward_weight");
    return VT_OK;
}

// ---- backward of the two resampling layers: Downsample2D's stride-2 conv and Upsample2D ----

// Downsample2D: y = conv3x3(pad(x, (0,1,0,1)), W), stride 2.  dy16 [B][H/2][W/2][Cout] -> dx [B][H][W][Cin].  The scatter kernel, or with
// vt_set_flag(ctx, 23, 1) / channel counts it refuses the literal route: dy16 scattered to the odd positions of a zeroed H x W tensor, then
// vt_op_conv_backward_data's launch.
int vt_op_conv_s2_backward_data(vt_context* c, const void* dy16, const float* w_oihw, const float* dx_add, float* dx, int B, int H, int W, int Cin, int Cout,
                                void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (!dy16 || !w_oihw || !dx) return c->fail(VT_ERR_INVALID, "vt_op_conv_s2_backward_data: null buffer");
    if (B <= 0 || H < 2 || W < 2 || Cin < 8 || (Cin % 8) || Cout < 8 || (Cout % 8))
        return c->fail(VT_ERR_INVALID, "vt_op_conv_s2_backward_data: Cin and Cout must be multiples of 8, B >= 1 and H, W >= 2 (got %d -> %d, %d x %d x %d)", Cin, Cout,
                       B, H, W);
    if ((long long)H * W * std::max(Cin, Cout) >= (1LL << 31)) return c->fail(VT_ERR_INVALID, "vt_op_conv_s2_backward_data: image too large (32-bit per-image offsets)");
    hipStream_t s = (hipStream_t)stream;
    if (!c->s2_dgrad_literal && vt_conv3x3_s2_dgrad_supported(Cin, Cout) && (Cout % 64) == 0) {
        VTCK(c->ensure_op_scratch(align_up((size_t)Cout * 9 * Cin * 2)));
        HIPCK(c, vt_launch_pack_s2_dgrad(w_oihw, (bf16_t*)c->op_scratch, Cin, Cout, s), "pack_s2_dgrad");
        ConvS2DgradArgs a{};
        a.dy = (const bf16_t*)dy16; a.Wp = (const bf16_t*)c->op_scratch; a.dx_add = dx_add; a.dx = dx; a.zeros = c->zeros;
        a.batch = B; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout;
        HIPCK(c, vt_launch_conv3x3_s2_dgrad(a, s), "conv3x3_s2_dgrad");
        return VT_OK;
    }
    const size_t keep = align_up((size_t)B * H * W * Cout * 2);
    VTCK(c->ensure_op_scratch(keep + 2 * align_up((size_t)Cin * 9 * Cout * 2)));      // (sized once: the launch below must not move the buffer)
    HIPCK(c, vt_launch_scatter_odd_nhwc16(dy16, c->op_scratch, B, H, W, Cout, s), "scatter_odd");
    return conv_dgrad_launch(c, c->op_scratch, w_oihw, dx_add, dx, B, H, W, Cin, Cout, 3, keep, s, "vt_op_conv_s2_backward_data(literal)");
}

static size_t rs_wgrad_ws_bytes(int mode, int B, int Hdy, int Wdy, int Cin, int Cout, int splits) {
    if (splits < 0 || !vt_conv_wgrad_supported(Cin, Cout, 3) || vt_conv_wgrad_rs_steps(mode, B, Hdy, Wdy) <= 0) return 0;
    const int sp = slice_count(splits, vt_conv_wgrad_rs_steps(mode, B, Hdy, Wdy), vt_conv_wgrad_rs_auto_splits(mode, B, Hdy, Wdy, Cin, Cout));
    return align_up((size_t)sp * Cout * Cin * 9 * sizeof(float));
}

static int rs_wgrad(vt_context* c, const char* name, int mode, const void* dy16, const void* a16, float* dw, int B, int Hdy, int Wdy, int aH, int aW, int Cin, int Cout,
                    int splits, void* ws, size_t ws_bytes, void* stream) {
    if (!dy16 || !a16 || !dw) return c->fail(VT_ERR_INVALID, "%s: null buffer", name);
    if (!vt_conv_wgrad_supported(Cin, Cout, 3)) return c->fail(VT_ERR_INVALID, "%s: channel counts must be multiples of 64 (got %d -> %d)", name, Cin, Cout);
    if (B <= 0 || aH < (mode == 1 ? 2 : 1) || aW < (mode == 1 ? 2 : 1) || vt_conv_wgrad_rs_steps(mode, B, Hdy, Wdy) <= 0)
        return c->fail(VT_ERR_INVALID, "%s: B must be >= 1 and the layer's input at least %s (got %d x %d x %d)", name, mode == 1 ? "2 x 2" : "1 x 1", B, aH, aW);
    if (splits < 0) return c->fail(VT_ERR_INVALID, "%s: splits must be >= 0 (0 = chosen from the shape)", name);
    if ((uintptr_t)dw % 16) return c->fail(VT_ERR_INVALID, "%s: dw must be 16-byte aligned", name);
    VTCK(check_workspace(c, name, ws, ws_bytes, rs_wgrad_ws_bytes(mode, B, Hdy, Wdy, Cin, Cout, splits), 16));
    ConvWgradArgs a{};
    a.dy = (const bf16_t*)dy16; a.a = (const bf16_t*)a16; a.dw = dw; a.ws = (float*)ws; a.batch = B; a.H = Hdy; a.W = Wdy; a.aH = aH; a.aW = aW; a.Cin = Cin; a.Cout = Cout;
    a.ksize = 3; a.splits = slice_count(splits, vt_conv_wgrad_rs_steps(mode, B, Hdy, Wdy), vt_conv_wgrad_rs_auto_splits(mode, B, Hdy, Wdy, Cin, Cout));
    HIPCK(c, vt_launch_conv_wgrad_rs(a, mode, (hipStream_t)stream), name);
    return VT_OK;
}

size_t vt_op_conv_s2_backward_weight_workspace_bytes(int B, int H, int W, int Cin, int Cout, int splits) {
    if (H < 2 || W < 2) return 0;
    return rs_wgrad_ws_bytes(1, B, H / 2, W / 2, Cin, Cout, splits);
}

int vt_op_conv_s2_backward_weight(vt_context* c, const void* dy16, const void* a16, float* dw, int B, int H, int W, int Cin, int Cout, int splits, void* ws,
                                  size_t ws_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    return rs_wgrad(c, "vt_op_conv_s2_backward_weight", 1, dy16, a16, dw, B, H / 2, W / 2, H, W, Cin, Cout, splits, ws, ws_bytes, stream);
}

// Upsample2D: y = conv3x3(nearest2x(x), W).  dy16 [B][2h][2w][C] -> dx [B][h][w][C].  The route follows the forward's: the gather kernel on the
// transposed folded matrices, or with vt_set_flag(ctx, 22, 1) / a C it refuses the literal one on bf16(W): vt_op_conv_backward_data's launch at
// 2h x 2w into scratch, then the 2x2 sum.
int vt_op_upsample2x_conv3x3_backward_data(vt_context* c, const void* dy16, const float* w_oihw, const float* dx_add, float* dx, int B, int h, int wd, int C,
                                           void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (!dy16 || !w_oihw || !dx) return c->fail(VT_ERR_INVALID, "vt_op_upsample2x_conv3x3_backward_data: null buffer");
    if (B <= 0 || h <= 0 || wd <= 0 || C < 8 || (C % 8))
        return c->fail(VT_ERR_INVALID, "vt_op_upsample2x_conv3x3_backward_data: C must be a multiple of 8 and B, h, w >= 1 (got %d, %d x %d x %d)", C, B, h, wd);
    if ((long long)B * h * wd * C >= (1LL << 29)) return c->fail(VT_ERR_INVALID, "vt_op_upsample2x_conv3x3_backward_data: tensor too large for the operator entry");
    hipStream_t s = (hipStream_t)stream;
    if (!c->up2_literal && vt_conv3x3_up2_dgrad_supported(C)) {
        VTCK(c->ensure_op_scratch(align_up((size_t)C * 16 * C * 2)));
        HIPCK(c, vt_launch_pack_up2_dgrad(w_oihw, (bf16_t*)c->op_scratch, C, s), "pack_up2_dgrad");
        ConvUp2DgradArgs a{};
        a.dy = (const bf16_t*)dy16; a.Wp = (const bf16_t*)c->op_scratch; a.dx_add = dx_add; a.dx = dx; a.zeros = c->zeros; a.batch = B; a.H = h; a.W = wd; a.C = C;
        HIPCK(c, vt_launch_conv3x3_up2_dgrad(a, s), "conv3x3_up2_dgrad");
        return VT_OK;
    }
    const size_t keep = align_up((size_t)B * 4 * h * wd * C * sizeof(float));
    VTCK(c->ensure_op_scratch(keep + 2 * align_up((size_t)C * 9 * C * 2)));
    float* t = (float*)c->op_scratch;
    VTCK(conv_dgrad_launch(c, dy16, w_oihw, nullptr, t, B, 2 * h, 2 * wd, C, C, 3, keep, s, "vt_op_upsample2x_conv3x3_backward_data(literal)"));
    HIPCK(c, vt_launch_sum2x2_f32(t, dx_add, dx, B, h, wd, C, s), "sum2x2");
    return VT_OK;
}

size_t vt_op_upsample2x_conv3x3_backward_weight_workspace_bytes(int B, int h, int w, int C, int splits) {
    if (h < 1 || w < 1 || h >= (1 << 29) || w >= (1 << 29)) return 0;
    return rs_wgrad_ws_bytes(2, B, 2 * h, 2 * w, C, C, splits);
}

int vt_op_upsample2x_conv3x3_backward_weight(vt_context* c, const void* dy16, const void* x16, float* dw, int B, int h, int w, int C, int splits, void* ws,
                                             size_t ws_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (h >= (1 << 29) || w >= (1 << 29)) return c->fail(VT_ERR_INVALID, "vt_op_upsample2x_conv3x3_backward_weight: shape too large");
    return rs_wgrad(c, "vt_op_upsample2x_conv3x3_backward_weight", 2, dy16, x16, dw, B, 2 * h, 2 * w, h, w, C, C, splits, ws, ws_bytes, stream);
}

// ---- the full-resolution end convs, 3 channels on one side ----

size_t vt_op_conv_thin_backward_weight_workspace_bytes(int B, int H, int W, int Cw, int splits) {
    if (splits < 0 || !vt_conv_thin_wgrad_supported(Cw) || vt_conv_thin_wgrad_steps(B, H, W) <= 0) return 0;
    return align_up(vt_conv_thin_wgrad_ws_bytes(Cw, slice_count(splits, vt_conv_thin_wgrad_steps(B, H, W), vt_conv_thin_wgrad_auto_splits(B, H, W, Cw))));
}

int vt_op_conv_thin_backward_weight(vt_context* c, const float* thin, const void* wide16, int thin_is_input, float* dw, float* thin_sums, int B, int H, int W,
                                    int Cw, int splits, void* ws, size_t ws_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    VTCK(vt_op_backward_operands_check(c));
    if (!thin || !wide16 || !dw) return c->fail(VT_ERR_INVALID, "vt_op_conv_thin_backward_weight: null buffer");
    if (!vt_conv_thin_wgrad_supported(Cw))
        return c->fail(VT_ERR_INVALID, "vt_op_conv_thin_backward_weight: Cw must be a multiple of 64, at most 512 (got %d)", Cw);
    if (B <= 0 || H <= 0 || W <= 0 || vt_conv_thin_wgrad_steps(B, H, W) <= 0) return c->fail(VT_ERR_INVALID, "vt_op_conv_thin_backward_weight: B, H, W must be >= 1");
    if (splits < 0) return c->fail(VT_ERR_INVALID, "vt_op_conv_thin_backward_weight: splits must be >= 0 (0 = chosen from the shape)");
    VTCK(check_workspace(c, "vt_op_conv_thin_backward_weight", ws, ws_bytes, vt_op_conv_thin_backward_weight_workspace_bytes(B, H, W, Cw, splits), 16));
    ConvThinWgradArgs a{};
    a.thin = thin; a.wide = (const bf16_t*)wide16; a.dw = dw; a.thin_sums = thin_sums; a.ws = ws; a.batch = B; a.H = H; a.W = W; a.Cw = Cw;
    a.thin_is_input = thin_is_input; a.splits = slice_count(splits, vt_conv_thin_wgrad_steps(B, H, W), vt_conv_thin_wgrad_auto_splits(B, H, W, Cw));
    HIPCK(c, vt_launch_conv_thin_wgrad(a, (hipStream_t)stream), "vt_op_conv_thin_backward_weight");
    return VT_OK;
}

// packed weights (the larger of the two layouts), then C zeros for the bias
static size_t thin_forward_pack_bytes(int C) { return align_up(std::max((size_t)27 * C * sizeof(float), (size_t)2 * 128 * 32 * 2)); }

size_t vt_op_conv_thin_forward_workspace_bytes(int C) {
    if (C < 8 || (C % 8)) return 0;
    return thin_forward_pack_bytes(C) + align_up((size_t)C * sizeof(float));
}

int vt_op_conv_thin_forward(vt_context* c, const float* x, const float* w, const float* bias, int transpose_rotate, float* o32, void* o16, int B, int H, int W,
                            int C, void* ws, size_t ws_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    VTCK(vt_op_backward_operands_check(c));
    if (!x || !w || (!o32 && !o16)) return c->fail(VT_ERR_INVALID, "vt_op_conv_thin_forward: null buffer");
    if (B <= 0 || H <= 0 || W <= 0 || C < 8 || (C % 8) || C > 256)
        return c->fail(VT_ERR_INVALID, "vt_op_conv_thin_forward: C must be a multiple of 8, at most 256, and B, H, W >= 1 (got %d, %d x %d x %d)", C, B, H, W);
    VTCK(check_workspace(c, "vt_op_conv_thin_forward", ws, ws_bytes, vt_op_conv_thin_forward_workspace_bytes(C), 16));
    hipStream_t s = (hipStream_t)stream;
    const bool mfma = C == 128 && c->conv_in_mfma;
    float* zero_bias = (float*)((char*)ws + thin_forward_pack_bytes(C));
    if (transpose_rotate) bias = nullptr;
    HIPCK(c, vt_launch_pack_conv_thin(w, bias, transpose_rotate != 0, mfma, ws, zero_bias, C, s), "pack_conv_thin");
    const float* b = bias ? bias : zero_bias;
    if (mfma) HIPCK(c, vt_launch_conv_in_mfma(x, (const bf16_t*)ws, b, o32, (bf16_t*)o16, nullptr, nullptr, nullptr, B, H, W, s), "vt_op_conv_thin_forward");
    else HIPCK(c, vt_launch_conv_in(x, (const float*)ws, b, o32, (bf16_t*)o16, nullptr, nullptr, 0, nullptr, B, H, W, C, s), "vt_op_conv_thin_forward");
    return VT_OK;
}

// The block functions (vae_backward.py) mix these operators with the forward ones, which follow flag 18: they ask here first.
int vt_op_backward_operands_check(vt_context* c) {
    if (!c) return VT_ERR_INVALID;
    if (c->f16_ops) return c->fail(VT_ERR_INVALID, "the resnet block's backward runs on bf16 operands: fp16-operand mode (vt_set_flag 18) must be off");
    return VT_OK;
}

// ---- GroupNorm: the fp64 (mean, rstd) the backward reads, and the backward with and without SiLU (DESIGN.md sections 4.19 and 4.20) ----

// what the three GroupNorm operators accept, under the name of the one that asks
static int check_gn_backward_shape(vt_context* c, const char* op, int B, int HW, int C, int groups) {
    if (B <= 0 || HW <= 0 || groups > 64 || !vt_gn_silu_bwd_supported(C, groups))
        return c->fail(VT_ERR_INVALID, "%s: channels per group must be 2, 4, 8 or 16 and C a power of two from 16 to 1024 (got C %d, %d groups)", op, C, groups);
    return VT_OK;
}

size_t vt_op_groupnorm_stats_workspace_bytes(int B, int HW, int C) {
    const size_t n = vt_gn_stats64_ws_bytes(B, HW, C);
    return n ? align_up(n) : 0;
}

int vt_op_groupnorm_stats(vt_context* c, const float* x, int B, int HW, int C, int groups, float eps, float* stats, void* ws, size_t ws_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (!x || !stats) return c->fail(VT_ERR_INVALID, "vt_op_groupnorm_stats: null buffer");
    VTCK(check_gn_backward_shape(c, "vt_op_groupnorm_stats", B, HW, C, groups));
    VTCK(check_workspace(c, "vt_op_groupnorm_stats", ws, ws_bytes, vt_op_groupnorm_stats_workspace_bytes(B, HW, C), 16));
    HIPCK(c, vt_launch_gn_stats64(x, B, HW, C, groups, eps, stats, ws, (hipStream_t)stream), "vt_op_groupnorm_stats");
    return VT_OK;
}

size_t vt_op_groupnorm_silu_backward_workspace_bytes(int B, int HW, int C) {
    const size_t n = vt_gn_silu_bwd_ws_bytes(B, HW, C);
    return n ? align_up(n) : 0;
}

size_t vt_op_groupnorm_backward_workspace_bytes(int B, int HW, int C) { return vt_op_groupnorm_silu_backward_workspace_bytes(B, HW, C); }

// the two backward operators differ in the launcher (du = da silu'(u), or du = da) and in the name their messages carry
static int gn_backward(vt_context* c, const char* op, decltype(&vt_launch_gn_backward) launch, const float* x, const float* stats, const float* gamma,
                       const float* beta, const float* da, const float* dx_add, float* dx, void* dx16, float* dgamma, float* dbeta, int B, int HW, int C, int groups,
                       void* ws, size_t ws_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (!x || !stats || !gamma || !beta || !da || !dx) return c->fail(VT_ERR_INVALID, "%s: null buffer", op);
    VTCK(check_gn_backward_shape(c, op, B, HW, C, groups));
    VTCK(check_workspace(c, op, ws, ws_bytes, vt_op_groupnorm_silu_backward_workspace_bytes(B, HW, C), 16));
    HIPCK(c, launch(x, stats, gamma, beta, da, dx_add, dx, (bf16_t*)dx16, dgamma, dbeta, B, HW, C, groups, ws, (hipStream_t)stream), op);
    return VT_OK;
}

int vt_op_groupnorm_silu_backward(vt_context* c, const float* x, const float* stats, const float* gamma, const float* beta, const float* da,
                                  const float* dx_add, float* dx, void* dx16, float* dgamma, float* dbeta, int B, int HW, int C, int groups, void* ws,
                                  size_t ws_bytes, void* stream) {
    return gn_backward(c, "vt_op_groupnorm_silu_backward", vt_launch_gn_silu_backward, x, stats, gamma, beta, da, dx_add, dx, dx16, dgamma, dbeta, B, HW, C, groups, ws,
                       ws_bytes, stream);
}

int vt_op_groupnorm_backward(vt_context* c, const float* x, const float* stats, const float* gamma, const float* beta, const float* dh, const float* dx_add,
                             float* dx, void* dx16, float* dgamma, float* dbeta, int B, int HW, int C, int groups, void* ws, size_t ws_bytes, void* stream) {
    return gn_backward(c, "vt_op_groupnorm_backward", vt_launch_gn_backward, x, stats, gamma, beta, dh, dx_add, dx, dx16, dgamma, dbeta, B, HW, C, groups, ws, ws_bytes,
                       stream);
}

}  // extern "C"
