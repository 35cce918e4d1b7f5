// The vt_op_* forward single-layer entry points: one kernel (or one conv of the encoder's schedule) on caller-owned buffers, and the synchronising
// test entries (vt_op_conv3x3_block, vt_op_conv3x3_fp8, vt_op_conv_in).  The backward operators are ops_backward.hip.
#include "vt_ops.h"

using namespace vt;

namespace {

template <class V>
hipError_t to_device(void* dst, const std::vector<V>& v) { return hipMemcpy(dst, v.data(), v.size() * sizeof(V), hipMemcpyHostToDevice); }

}  // namespace

extern "C" {

int vt_op_conv2d(vt_context* c, const void* x, const void* w, const float* bias, const float* res, float* o32, void* o16,
                 int B, int Hin, int Win, int Cin, int Cout, int ksize, int stride, int pad_lo, int pad_hi, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (!x || !w || (!o32 && !o16)) return c->fail(VT_ERR_INVALID, "vt_op_conv2d: null buffer");
    if (stride < 1 || pad_lo < 0 || pad_hi < 0) return c->fail(VT_ERR_INVALID, "vt_op_conv2d: bad stride/pad");
    const int Hout = (Hin + pad_lo + pad_hi - ksize) / stride + 1, Wout = (Win + pad_lo + pad_hi - ksize) / stride + 1;
    if (Hout < 1 || Wout < 1) return c->fail(VT_ERR_INVALID, "vt_op_conv2d: empty output");
    hipStream_t s = (hipStream_t)stream;
    if (c->use_halo_conv && ksize == 3 && stride == 1 && pad_lo == 1 && pad_hi == 1 && vt_conv3x3_halo_supported(Cin, Cout)) {
        Conv3x3Args h{};
        VTCK(repack_halo(c, w, Cin, Cout, s, &h.Wp));
        h.X = (const bf16_t*)x; h.bias = bias; h.res = res; h.out_f32 = o32;
        h.out_bf16 = (bf16_t*)o16; h.zeros = c->zeros; h.batch = B; h.H = Hin; h.W = Win; h.Cin = Cin; h.Cout = Cout;
        return launch_halo(c, h, s, "vt_op_conv2d(halo)");
    }
    if (c->s2_halo && ksize == 3 && stride == 2 && pad_lo == 0 && pad_hi == 1 && Hin >= 2 && Win >= 2 && vt_conv3x3_s2_supported(Cin, Cout)) {
        VTCK(c->ensure_op_scratch((size_t)Cout * 9 * Cin * 2));
        HIPCK(c, vt_launch_repack_ohwi_to_s2((const bf16_t*)w, (bf16_t*)c->op_scratch, Cin, Cout, s), "repack");
        ConvW cw; cw.cin = Cin; cw.cout = Cout; cw.k = 3; cw.wp2 = (const bf16_t*)c->op_scratch; cw.b = bias;
        return run_conv(c, cw, (const bf16_t*)x, B, Hin, Win, 2, 0, Hout, Wout, res, o32, (bf16_t*)o16, s);
    }
    ConvGemmArgs a{};
    a.X = (const bf16_t*)x; a.W = (const bf16_t*)w; a.bias = bias; a.res = res; a.out_f32 = o32; a.out_bf16 = (bf16_t*)o16;
    a.zeros = c->zeros; a.Hin = Hin; a.Win = Win; a.Hout = Hout; a.Wout = Wout; a.Cin = Cin; a.Cout = Cout; a.Wrows = Cout;
    a.ksize = ksize; a.stride = stride; a.pad = pad_lo; a.ldx = Cin; a.ldw = ksize * ksize * Cin; a.ldo = Cout; a.ldr = Cout;
    a.x_bs = (long long)Hin * Win * Cin; a.o_bs = (long long)Hout * Wout * Cout; a.r_bs = a.o_bs; a.batch = B;
    a.alpha = 1.f; a.bias_mode = bias ? 1 : 0;
    return launch_gemm(c, a, s, "vt_op_conv2d");
}

// conv3x3(silu(x*scale + shift)), stride 1, pad 1, with the affine + SiLU fused into the conv's halo staging
int vt_op_norm_silu_conv3x3(vt_context* c, const void* x, int x_dtype, const float* scale_shift, const void* w,
                            const float* bias, const float* res, float* o32, void* o16, int B, int H, int W, int Cin,
                            int Cout, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (!x || !scale_shift || !w || (!o32 && !o16)) return c->fail(VT_ERR_INVALID, "vt_op_norm_silu_conv3x3: null buffer");
    if (x_dtype != VT_F32 && x_dtype != VT_BF16) return c->fail(VT_ERR_INVALID, "vt_op_norm_silu_conv3x3: x must be f32 or bf16");
    if (!vt_conv3x3_halo_supported(Cin, Cout) || Cin * 8 > 8192) return c->fail(VT_ERR_INVALID, "vt_op_norm_silu_conv3x3: unsupported channel counts %d -> %d", Cin, Cout);
    hipStream_t s = (hipStream_t)stream;
    Conv3x3Args h{};
    VTCK(repack_halo(c, w, Cin, Cout, s, &h.Wp));
    h.X = x_dtype == VT_BF16 ? (const bf16_t*)x : nullptr; h.Xf32 = x_dtype == VT_F32 ? (const float*)x : nullptr;
    h.scale_shift = scale_shift; h.bias = bias; h.res = res; h.out_f32 = o32;
    h.out_bf16 = (bf16_t*)o16; h.zeros = c->zeros; h.batch = B; h.H = H; h.W = W; h.Cin = Cin; h.Cout = Cout;
    return launch_halo(c, h, s, "vt_op_norm_silu_conv3x3");
}

size_t vt_op_conv2d_gn_workspace_bytes(int B, int Hout, int Wout, int Cout) {
    if (B <= 0 || Hout <= 0 || Wout <= 0 || Cout <= 0) return 0;
    int parts = vt_conv_gemm_ptiles(Hout * Wout, Cout);
    const int t2 = vt_conv3x3_halo_tiles_max(Hout, Wout);
    if (t2 > parts) parts = t2;
    return align_up((size_t)B * parts * 64 * 3 * 4);
}

// conv + the GroupNorm (scale, shift) of its OUTPUT from the epilogue partials (no extra pass over the output)
int vt_op_conv2d_gn(vt_context* c, const void* x, const void* w, const float* bias, const float* res, float* o32, void* o16,
                    int B, int Hin, int Win, int Cin, int Cout, int ksize, int stride, int pad_lo, int pad_hi, int groups,
                    float eps, const float* gamma, const float* beta, float* scale_shift, void* ws, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    // ---- every refusal of this function comes before its first launch (run_conv makes its own before it launches)
    if (!ws) return c->fail(VT_ERR_INVALID, "vt_op_conv2d_gn: bad argument");
    VTCK(check_gn_epilogue(c, "vt_op_conv2d_gn", gamma, beta, scale_shift, Cout, groups));
    if (!bias) return c->fail(VT_ERR_INVALID, "vt_op_conv2d_gn: bias required");
    const int Hout = (Hin + pad_lo + pad_hi - ksize) / stride + 1, Wout = (Win + pad_lo + pad_hi - ksize) / stride + 1;
    ConvW cw; cw.cin = Cin; cw.cout = Cout; cw.k = ksize; cw.w = (const bf16_t*)w; cw.b = bias;
    hipStream_t s = (hipStream_t)stream;
    if (c->use_halo_conv && ksize == 3 && stride == 1 && pad_lo == 1 && pad_hi == 1 && vt_conv3x3_halo_supported(Cin, Cout))
        VTCK(repack_halo(c, w, Cin, Cout, s, &cw.wp));
    GnState gn; gn.partial = (float*)ws;
    ConvOpts o; o.gn = &gn; o.groups = groups;
    FuseGnStats stats_on(c);
    VTCK(run_conv(c, cw, (const bf16_t*)x, B, Hin, Win, stride, pad_lo, Hout, Wout, res, o32, (bf16_t*)o16, s, o));
    return finish_gn_stats(c, "vt_op_conv2d_gn", gn, B, Cout, groups, eps, gamma, beta, scale_shift, s);
}

// Upsample2D (nearest 2x + conv3x3) of the low-resolution x: the folded kernel, or with vt_set_flag(ctx, 22, 1) / a shape it refuses the
// literal route (upsample pass + the stride-1 conv).  Scratch comes from the context's operator buffer.
static int op_upsample2x_conv3x3(vt_context* c, const void* x, const float* w, const float* bias, float* o32, int B, int h, int wd, int C,
                                 int groups, float eps, const float* gamma, const float* beta, float* scale_shift, hipStream_t s) {
    if (!x || !w || !o32) return c->fail(VT_ERR_INVALID, "vt_op_upsample2x_conv3x3: null buffer");
    if (B <= 0 || h <= 0 || wd <= 0 || C < 8 || (C % 8)) return c->fail(VT_ERR_INVALID, "vt_op_upsample2x_conv3x3: bad shape");
    if ((long long)B * h * wd * C >= (1LL << 29)) return c->fail(VT_ERR_INVALID, "vt_op_upsample2x_conv3x3: tensor too large for the operator entry");
    const bool f16 = c->f16_ops != 0;
    const bool want_gn = scale_shift != nullptr;
    const bool folded = !c->up2_literal && vt_conv3x3_up2_supported(C, C);
    const int cpg = want_gn ? C / groups : 0;
    const int parts_max = std::max({vt_conv3x3_up2_tiles(h, wd), vt_conv3x3_halo_tiles_max(2 * h, 2 * wd), vt_conv_gemm_ptiles(4 * h * wd, C)});
    const size_t gn_bytes = want_gn ? align_up((size_t)B * parts_max * groups * 3 * 4) : 0;
    const size_t w_bytes = align_up((size_t)C * C * 16 * 2), up_bytes = align_up((size_t)B * 4 * h * wd * C * 2);
    VTCK(c->ensure_op_scratch(gn_bytes + w_bytes + (folded ? 0 : up_bytes)));
    char* p = (char*)c->op_scratch;
    GnState gn; gn.partial = (float*)p; p += gn_bytes;
    bf16_t* wp = (bf16_t*)p; p += w_bytes;
    if (folded) {
        HIPCK(c, vt_launch_pack_up2(w, f16 ? nullptr : wp, f16 ? (f16_t*)wp : nullptr, C, C, s), "pack_up2");
        ConvUp2Args a{};
        a.X = (const bf16_t*)x; a.Wp = wp; a.bias = bias; a.out_f32 = o32; a.zeros = c->zeros; a.batch = B; a.H = h; a.W = wd; a.Cin = C; a.Cout = C; a.f16 = f16;
        if (want_gn) { a.gn_partial = gn.partial; a.gn_cpg = cpg; gn.parts = vt_conv3x3_up2_tiles(h, wd); }
        HIPCK(c, vt_launch_conv3x3_up2(a, s), "conv3x3_up2");
    } else {
        bf16_t* up = (bf16_t*)p;
        const bool halo = c->use_halo_conv && vt_conv3x3_halo_supported(C, C);
        if (f16 && !(halo && vt_conv3x3_halo_f16_supported(C, c->halo_occ2, 0)))
            return c->fail(VT_ERR_INVALID, "vt_op_upsample2x_conv3x3: the literal route has no fp16-operand kernel for %d channels", C);
        HIPCK(c, vt_launch_upsample2x_nhwc16(x, up, B, h, wd, C, s), "upsample2x");
        HIPCK(c, vt_launch_pack_f32_oihw(w, wp, C, C, halo ? 1 : 0, f16, s), "pack_f32_oihw");
        ConvW cw; cw.cin = C; cw.cout = C; cw.k = 3; cw.b = bias;
        if (halo) { cw.wp = wp; cw.wp16 = wp; } else cw.w = wp;
        ConvOpts o; o.x_f16 = f16; o.groups = want_gn ? groups : 32; o.gn = want_gn ? &gn : nullptr;
        FuseGnStats stats_on(c);
        VTCK(run_conv(c, cw, up, B, 2 * h, 2 * wd, 1, 1, 2 * h, 2 * wd, nullptr, o32, nullptr, s, o));
    }
    return want_gn ? finish_gn_stats(c, "vt_op_upsample2x_conv3x3_gn", gn, B, C, groups, eps, gamma, beta, scale_shift, s) : VT_OK;
}

int vt_op_upsample2x_conv3x3(vt_context* c, const void* x, const float* w_oihw, const float* bias, float* o32, int B, int h, int w, int C,
                             void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    return op_upsample2x_conv3x3(c, x, w_oihw, bias, o32, B, h, w, C, 0, 0.f, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

int vt_op_upsample2x_conv3x3_gn(vt_context* c, const void* x, const float* w_oihw, const float* bias, float* o32, int B, int h, int w, int C,
                                int groups, float eps, const float* gamma, const float* beta, float* scale_shift, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (!bias) return c->fail(VT_ERR_INVALID, "vt_op_upsample2x_conv3x3_gn: bad argument");
    VTCK(check_gn_epilogue(c, "vt_op_upsample2x_conv3x3_gn", gamma, beta, scale_shift, C, groups));
    return op_upsample2x_conv3x3(c, x, w_oihw, bias, o32, B, h, w, C, groups, eps, gamma, beta, scale_shift, (hipStream_t)stream);
}

size_t vt_op_conv3x3_fp8_workspace_bytes(int B, int H, int W, int Cin, int Cout) {
    if (B <= 0 || H <= 0 || W <= 0 || !vt_conv3x3_halo_fp8_supported(Cin, Cout)) return 0;
    return align_up((size_t)B * H * W * Cin) + align_up((size_t)B * Cin * 8) + align_up((size_t)Cout * 9 * Cin) + align_up((size_t)Cout * 4) + ALIGN;
}

// 3x3 stride-1 pad-1 conv on fp8 operands, as the encoder runs it with vt_set_flag(ctx, 11, 1): x (fp32 NHWC, device) is quantised
// to e4m3(8 x) by the GroupNorm-apply kernel (identity affine, no SiLU), w (fp32 OIHW, DEVICE; copied to the host, packed to e4m3
// with per-cout scales and written into the workspace: synchronises).  out = conv(deq(x8), deq(w8)) + bias (+ residual), fp32 NHWC.
int vt_op_conv3x3_fp8(vt_context* c, const float* x_nhwc, const float* w_oihw, const float* bias, const float* res, float* o32,
                      int B, int H, int W, int Cin, int Cout, int stride, void* ws, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (!x_nhwc || !w_oihw || !o32 || !ws || ((uintptr_t)ws % ALIGN)) return c->fail(VT_ERR_INVALID, "vt_op_conv3x3_fp8: bad buffer");
    if (vt_op_conv3x3_fp8_workspace_bytes(B, H, W, Cin, Cout) == 0 || (stride != 1 && stride != 2)) return c->fail(VT_ERR_INVALID, "vt_op_conv3x3_fp8: unsupported shape");
    hipStream_t s = (hipStream_t)stream;
    char* p = (char*)ws;
    unsigned char* x8 = (unsigned char*)p; p += align_up((size_t)B * H * W * Cin);
    float* ss = (float*)p; p += align_up((size_t)B * Cin * 8);
    unsigned char* w8 = (unsigned char*)p; p += align_up((size_t)Cout * 9 * Cin);
    float* mult = (float*)p;
    std::vector<float> hw((size_t)Cout * 9 * Cin), hss((size_t)B * Cin * 2);
    HIPCK(c, hipMemcpy(hw.data(), w_oihw, hw.size() * 4, hipMemcpyDeviceToHost), "vt_op_conv3x3_fp8 copy");
    const bool s2_kernel = stride == 2 && c->s2_halo && vt_conv3x3_s2_fp8_supported(Cin, Cout);
    const ConvE4m3 pk = pack_conv_e4m3(hw.data(), Cout, Cin, s2_kernel);
    for (size_t i = 0; i < hss.size(); i += 2) { hss[i] = 1.f; hss[i + 1] = 0.f; }
    HIPCK(c, to_device(ss, hss), "vt_op_conv3x3_fp8 copy");
    if (stride == 2) {
        // Downsample2D's conv: pad (0,1,0,1), stride 2, on the generic GEMM's fp8 variant -- or the phase-plane kernel's packing
        // instead (same scales); x is quantised as e4m3(x) (scale 1)
        HIPCK(c, to_device(w8, s2_kernel ? pk.wp8s2 : pk.w8g), "vt_op_conv3x3_fp8 copy");
        HIPCK(c, to_device(mult, pk.mult8g), "vt_op_conv3x3_fp8 copy");
        HIPCK(c, vt_launch_gn_apply(x_nhwc, 1, ss, x8, B, H * W, Cin, 0, s, FP8_RES_SCALE), "vt_op_conv3x3_fp8 quantise");
        ConvW cw; cw.cin = Cin; cw.cout = Cout; cw.k = 3; cw.w8g = w8; cw.mult8g = mult; cw.b = bias;
        if (s2_kernel) cw.wp8s2 = w8;
        ConvOpts o; o.x_fp8 = true;
        return run_conv(c, cw, (const bf16_t*)x8, B, H, W, 2, 0, H / 2, W / 2, res, o32, nullptr, s, o);
    }
    HIPCK(c, to_device(w8, pk.wp8), "vt_op_conv3x3_fp8 copy");
    HIPCK(c, to_device(mult, pk.mult8), "vt_op_conv3x3_fp8 copy");
    HIPCK(c, vt_launch_gn_apply(x_nhwc, 1, ss, x8, B, H * W, Cin, 0, s, FP8_ACT_SCALE), "vt_op_conv3x3_fp8 quantise");
    Conv3x3Fp8Args h{};
    h.X = x8; h.Wp = w8; h.mult = mult; h.bias = bias; h.res = res; h.out_f32 = o32; h.zeros = c->zeros;
    h.batch = B; h.H = H; h.W = W; h.Cin = Cin; h.Cout = Cout;
    h.shape = (Cin <= 128 || (c->fp8_tile & 4)) ? (c->fp8_tile & 3) : 0;
    return launch_halo_fp8(c, h, s, "vt_op_conv3x3_fp8");
}

size_t vt_op_conv3x3_block_workspace_bytes(int B, int H, int W, int Cout, int stride) {
    if (stride != 1 && stride != 2) return 0;
    return vt_op_conv2d_gn_workspace_bytes(B, stride == 2 ? H / 2 : H, stride == 2 ? W / 2 : W, Cout);
}

// One conv of a resnet block / Downsample2D in the forms the schedules launch: fused shortcut, fp16 residual stream, 16-bit operand copy
// (bf16 / fp16 bits, NHWC / chunk-planar), GroupNorm partials -- through run_conv and the finalizers' packers (header: the contract).
int vt_op_conv3x3_block(vt_context* c, const void* x, int x_planar, const float* w_oihw, const float* bias, const void* sc_x, const float* sc_w,
                        int sc_cin, const void* res, int res_dtype, void* out, int out_dtype, void* o16, int out16_f16, int out16_planar, int B,
                        int H, int W, int Cin, int Cout, int stride, int groups, float eps, const float* gamma, const float* beta,
                        float* scale_shift, void* ws, size_t ws_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    // ---- everything that can be refused is refused here or inside run_conv, before the first launch
    if (!x || !w_oihw || !bias || (!out && !o16)) return c->fail(VT_ERR_INVALID, "vt_op_conv3x3_block: null buffer (x, w, bias and one of out / out16 are required)");
    if (stride != 1 && stride != 2) return c->fail(VT_ERR_INVALID, "vt_op_conv3x3_block: stride must be 1 (pad 1) or 2 (pad (0,1,0,1)), got %d", stride);
    if (B <= 0 || H < stride || W < stride) return c->fail(VT_ERR_INVALID, "vt_op_conv3x3_block: bad shape %d x %d x %d", B, H, W);
    if (!vt_conv3x3_halo_supported(Cin, Cout) || !vt_conv3x3_s2_supported(Cin, Cout))
        return c->fail(VT_ERR_INVALID, "vt_op_conv3x3_block: the halo kernels take Cin %% 32 == 0 and Cout %% 128 == 0 (got %d -> %d)", Cin, Cout);
    if ((long long)B * H * W * std::max(Cin, Cout) >= (1LL << 31)) return c->fail(VT_ERR_INVALID, "vt_op_conv3x3_block: tensor too large for the operator entry");
    if ((res && res_dtype != VT_F32 && res_dtype != VT_F16) || (out && out_dtype != VT_F32 && out_dtype != VT_F16))
        return c->fail(VT_ERR_INVALID, "vt_op_conv3x3_block: residual / out must be VT_F32 or VT_F16");
    if (res && out && res_dtype != out_dtype)
        return c->fail(VT_ERR_INVALID, "vt_op_conv3x3_block: the residual stream has one type: an %s residual with an %s output is not a form the kernels have",
                       res_dtype == VT_F16 ? "fp16" : "fp32", out_dtype == VT_F16 ? "fp16" : "fp32");
    const int rdt = (out ? out_dtype : (res ? res_dtype : VT_F32)) == VT_F16 ? 2 : 1;
    const bool has_sc = sc_x || sc_w;
    if (has_sc) {
        if (!sc_x || !sc_w || sc_cin <= 0 || (sc_cin % 32)) return c->fail(VT_ERR_INVALID, "vt_op_conv3x3_block: the fused shortcut needs sc_x, sc_w and sc_cin %% 32 == 0");
        if (stride != 1) return c->fail(VT_ERR_INVALID, "vt_op_conv3x3_block: the stride-2 kernel has no fused shortcut");
        if (res) return c->fail(VT_ERR_INVALID, "vt_op_conv3x3_block: a fused shortcut replaces the residual (ConvOpts::sc): give one of them");
        if ((long long)B * H * W * sc_cin >= (1LL << 31)) return c->fail(VT_ERR_INVALID, "vt_op_conv3x3_block: tensor too large for the operator entry");
    }
    if (x_planar && stride == 1) return c->fail(VT_ERR_INVALID, "vt_op_conv3x3_block: the stride-1 kernels read NHWC input only (chunk-planar x is the stride-2 kernel's)");
    if (out16_planar && stride == 2) return c->fail(VT_ERR_INVALID, "vt_op_conv3x3_block: the stride-2 kernel writes no chunk-planar copy");
    if ((out16_f16 || out16_planar) && !o16) return c->fail(VT_ERR_INVALID, "vt_op_conv3x3_block: out16_f16 / out16_planar without out16");
    const bool want_gn = scale_shift != nullptr;
    const int Ho = stride == 2 ? H / 2 : H, Wo = stride == 2 ? W / 2 : W;
    if (want_gn) {
        VTCK(check_gn_epilogue(c, "vt_op_conv3x3_block", gamma, beta, scale_shift, Cout, groups));
        VTCK(check_workspace(c, "vt_op_conv3x3_block", ws, ws_bytes, vt_op_conv3x3_block_workspace_bytes(B, H, W, Cout, stride), ALIGN, VT_ERR_WORKSPACE));
        // the generic GEMM (flag 0 / 13 off, or a stride-2 conv with an fp16 residual) has a stats epilogue on whole 128- / 256-cout tiles only
        const bool gemm = stride == 1 ? !c->use_halo_conv : !(c->s2_halo && !(res && rdt == 2));
        if (gemm && Cout > 128 && (Cout % 256)) return c->fail(VT_ERR_INVALID, "vt_op_conv3x3_block: the generic GEMM has no stats epilogue for %d couts", Cout);
    }
    hipStream_t s = (hipStream_t)stream;
    // ---- pack: the weights come to the host and go through pack_conv / pack_fused_shortcut, as in vt_encoder_finalize (synchronises)
    std::vector<float> hw((size_t)Cout * Cin * 9), hb(Cout), hsw(has_sc ? (size_t)Cout * sc_cin : 0);
    HIPCK(c, hipStreamSynchronize(s), "vt_op_conv3x3_block sync");
    HIPCK(c, hipMemcpy(hw.data(), w_oihw, hw.size() * 4, hipMemcpyDeviceToHost), "vt_op_conv3x3_block copy");
    HIPCK(c, hipMemcpy(hb.data(), bias, hb.size() * 4, hipMemcpyDeviceToHost), "vt_op_conv3x3_block copy");
    if (has_sc) HIPCK(c, hipMemcpy(hsw.data(), sc_w, hsw.size() * 4, hipMemcpyDeviceToHost), "vt_op_conv3x3_block copy");
    // the packed tensors live in a list of this call (not in a model's), without the e4m3 forms, and are freed when it returns
    struct Uploads {
        vt_context* c; std::vector<void*> list; std::vector<void*>* saved; bool fp8;
        explicit Uploads(vt_context* c_) : c(c_), saved(c_->cur_allocs), fp8(c_->pack_fp8) { c->cur_allocs = &list; c->pack_fp8 = false; }
        ~Uploads() { c->cur_allocs = saved; c->pack_fp8 = fp8; (void)hipDeviceSynchronize(); c->free_allocs(list); }
    } uploads(c);
    ConvW cw;
    VTCK(pack_conv(c, "vt_op_conv3x3_block", hw.data(), hb.data(), Cout, Cin, 3, &cw, stride == 2));
    ScFuse scf{};
    if (has_sc) {
        VTCK(pack_fused_shortcut(c, "vt_op_conv3x3_block shortcut", hsw.data(), hb.data(), Cout, sc_cin, &scf.wp, &scf.bias, &scf.wp16));
        scf.x = (const bf16_t*)sc_x; scf.cin = sc_cin;
    }
    // fp16-operand mode: x (and sc_x) carry fp16 bits exactly when the schedules would have written them so for this conv
    const bool f16 = c->f16_ops != 0;
    if (f16 && !conv_f16(c, cw, stride, has_sc))
        return c->fail(VT_ERR_INVALID, "vt_op_conv3x3_block: fp16-operand mode (flag 18) is on, but under the current flags this conv has no fp16-operand kernel");
    scf.x_f16 = f16;
    GnState gn; gn.partial = (float*)ws;
    ConvOpts o;
    o.x_f16 = f16; o.o16_f16 = out16_f16 != 0; o.planar = stride == 1 ? out16_planar != 0 : x_planar != 0; o.rdt = rdt;
    o.sc = has_sc ? &scf : nullptr; o.gn = want_gn ? &gn : nullptr; o.groups = want_gn ? groups : 32;
    FuseGnStats stats_on(c);
    VTCK(run_conv(c, cw, (const bf16_t*)x, B, H, W, stride, stride == 1 ? 1 : 0, Ho, Wo, res, out, (bf16_t*)o16, s, o));
    if (want_gn) VTCK(finish_gn_stats(c, "vt_op_conv3x3_block", gn, B, Cout, groups, eps, gamma, beta, scale_shift, s));
    HIPCK(c, hipStreamSynchronize(s), "vt_op_conv3x3_block sync");
    return VT_OK;
}

int vt_op_gemm_nt(vt_context* c, const void* A, const void* Bm, const float* bias, float* o32, void* o16, int batch, int M,
                  int N, int K, int lda, int ldb, int ldo, long long a_bs, long long b_bs, long long o_bs, float alpha,
                  int bias_per_row, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (!A || !Bm || (!o32 && !o16)) return c->fail(VT_ERR_INVALID, "vt_op_gemm_nt: null buffer");
    ConvGemmArgs a{};
    a.X = (const bf16_t*)A; a.W = (const bf16_t*)Bm; a.bias = bias; a.out_f32 = o32; a.out_bf16 = (bf16_t*)o16; a.zeros = c->zeros;
    a.Hin = a.Hout = 1; a.Win = a.Wout = M; a.Cin = K; a.Cout = N; a.Wrows = N; a.ksize = 1; a.stride = 1; a.pad = 0;
    a.ldx = lda; a.ldw = ldb; a.ldo = ldo; a.x_bs = a_bs; a.w_bs = b_bs; a.o_bs = o_bs; a.batch = batch; a.alpha = alpha;
    a.bias_mode = bias ? (bias_per_row ? 2 : 1) : 0;
    return launch_gemm(c, a, (hipStream_t)stream, "vt_op_gemm_nt");
}

int vt_op_conv_in(vt_context* c, const float* x, const float* w_oihw, const float* bias, float* o32, void* o16, int B,
                  int H, int W, int Cout, void* ws, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (!x || !w_oihw || !bias || !ws) return c->fail(VT_ERR_INVALID, "vt_op_conv_in: null buffer");
    // device-side repack is not worth a kernel for a test entry point: weights arrive on the DEVICE in OIHW,
    // are copied to the host, packed [27][Cout] and written into `ws` (>= 27*Cout*4 bytes).  Synchronises.
    std::vector<float> hw((size_t)Cout * 27);
    HIPCK(c, hipMemcpy(hw.data(), w_oihw, hw.size() * 4, hipMemcpyDeviceToHost), "vt_op_conv_in copy");
    if (Cout == 128 && c->conv_in_mfma) {            // the matrix-core variant the encoder uses (vt_set_flag 5); ws >= 16 KB
        std::vector<float> hb(128);
        HIPCK(c, hipMemcpy(hb.data(), bias, 128 * 4, hipMemcpyDeviceToHost), "vt_op_conv_in copy");
        HIPCK(c, to_device(ws, pack_conv_in_mfma(hw.data(), hb.data())), "vt_op_conv_in copy");
        HIPCK(c, vt_launch_conv_in_mfma(x, (const bf16_t*)ws, bias, o32, (bf16_t*)o16, nullptr, nullptr, nullptr, B, H, W, (hipStream_t)stream), "vt_op_conv_in");
        return VT_OK;
    }
    HIPCK(c, to_device(ws, pack_conv_in(hw.data(), Cout)), "vt_op_conv_in copy");
    HIPCK(c, vt_launch_conv_in(x, (const float*)ws, bias, o32, (bf16_t*)o16, nullptr, nullptr, 0, nullptr, B, H, W, Cout, (hipStream_t)stream), "vt_op_conv_in");
    return VT_OK;
}

size_t vt_op_groupnorm_workspace_bytes(int B, int HW, int C) {
    if (B <= 0 || HW <= 0 || C < 8 || (C % 8)) return 0;
    return align_up((size_t)B * vt_gn_max_chunks(HW, C) * 64 * 3 * 4) + align_up((size_t)B * C * 2 * 4);
}

int vt_op_groupnorm(vt_context* c, const void* x, int x_dtype, int B, int HW, int C, int groups, float eps,
                    const float* gamma, const float* beta, int silu, void* y, void* ws, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (!x || !gamma || !beta || !y || !ws) return c->fail(VT_ERR_INVALID, "vt_op_groupnorm: null buffer");
    if (x_dtype != VT_F32 && x_dtype != VT_BF16 && x_dtype != VT_F16) return c->fail(VT_ERR_INVALID, "vt_op_groupnorm: dtype must be f32, bf16 or f16");
    if (groups > 64) return c->fail(VT_ERR_INVALID, "vt_op_groupnorm: groups > 64");
    hipStream_t s = (hipStream_t)stream;
    float* partial = (float*)ws;
    float* ss = (float*)((char*)ws + align_up((size_t)B * vt_gn_max_chunks(HW, C) * 64 * 3 * 4));
    int nchunks = 0;
    const int f = x_dtype == VT_F32 ? 1 : (x_dtype == VT_F16 ? 2 : 0);
    HIPCK(c, vt_launch_gn_stats(x, f, B, HW, C, groups, partial, &nchunks, s), "gn_stats");
    HIPCK(c, vt_launch_gn_finalize(partial, nchunks, B, C, groups, eps, gamma, beta, ss, s), "gn_finalize");
    HIPCK(c, vt_launch_gn_apply(x, f, ss, (bf16_t*)y, B, HW, C, silu, s), "gn_apply");
    return VT_OK;
}

int vt_op_softmax_rows(vt_context* c, const float* scores, void* probs, int rows, int n, int lds, int ldp, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    HIPCK(c, vt_launch_softmax_rows(scores, 0, (bf16_t*)probs, rows, n, lds, ldp, (hipStream_t)stream), "vt_op_softmax_rows");
    return VT_OK;
}

}  // extern "C"
