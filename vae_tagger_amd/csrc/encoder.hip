// The conv / GroupNorm launch helpers of both VAE schedules (host code): which conv kernel runs for which shape and flag set, GroupNorm
// bookkeeping (run_conv, run_gn, run_norm_conv) -- and the encoder's schedule over the shared run layer (vt_vae_run.h): its plan, conv_in,
// the down stages, vt_encode, vt_encode_tag.  No host synchronisation, caller-owned buffers.
#include <algorithm>

#include "vt_vae_run.h"

namespace vt {

// ---- launch helpers -------------------------------------------------------------------------------
int launch_gemm(vt_context* c, const ConvGemmArgs& a_in, hipStream_t s, const char* what) {
    ConvGemmArgs a = a_in;
    a.short_tiles = c->gemm_short;
    if (!c->profiling || a.gate) { HIPCK(c, vt_launch_conv_gemm(a, s), what); return VT_OK; }       // gated launches may be no-ops: not counted
    const int n = a.Cout < a.Wrows ? a.Cout : a.Wrows;
    return profiled(c, s, vt_conv_gemm_config(a), 2.0 * a.batch * (double)a.Hout * a.Wout * n * (double)(a.ksize * a.ksize) * a.Cin, what,
                    [&] { return vt_launch_conv_gemm(a, s); });
}

int launch_halo(vt_context* c, const Conv3x3Args& a_in, hipStream_t s, const char* what) {
    Conv3x3Args a = a_in;
    a.occ2 = c->halo_occ2;
    if (!c->profiling) { HIPCK(c, vt_launch_conv3x3_halo(a, s), what); return VT_OK; }
    return profiled(c, s, vt_conv3x3_halo_config(a), 2.0 * a.batch * (double)a.H * a.W * a.Cout * (9.0 * a.Cin + (a.scX ? a.scCin : 0)), what,
                    [&] { return vt_launch_conv3x3_halo(a, s); });
}

int launch_halo_fp8(vt_context* c, const Conv3x3Fp8Args& a, hipStream_t s, const char* what) {
    return profiled(c, s, a.Cin <= 128 ? VT_PROF_HALO_FP8_C128 : VT_PROF_HALO_FP8,
                    2.0 * a.batch * (double)a.H * a.W * a.Cout * (9.0 * a.Cin + (a.scX ? a.scCin : 0)), what, [&] { return vt_launch_conv3x3_halo_fp8(a, s); });
}

// (run_gn, conv_f16 and run_norm_conv serve the shared run layer, vae_run.hip, and the image decoder's schedule: declared in vt_context.h)

// y = act(GroupNorm(x)) as bf16 rows.  Uses epilogue-produced partials when present.
int run_gn(vt_context* c, const void* x, int xdt /*0 bf16, 1 fp32, 2 fp16*/, int B, int HW, const NormW& n, int groups, int silu, bf16_t* y,
           GnState& g, hipStream_t s, bool out_fp8, bool out_f16 /* y holds fp16 bits: the consumer conv runs on fp16 operands */) {
    const float o8 = out_fp8 ? FP8_ACT_SCALE : 0.f;       // y then holds e4m3(8 y), one byte per element
    int parts = g.parts;
    if (parts == 0) HIPCK(c, vt_launch_gn_stats(x, xdt, B, HW, n.c, groups, g.partial, &parts, s), "gn_stats");
    g.parts = 0;
    HIPCK(c, vt_launch_gn_finalize(g.partial, parts, B, n.c, groups, 1e-6f, n.g, n.b, g.ss, s, c->status), "gn_finalize");
    dbg_sum(c, g.partial, (size_t)B * parts * groups * 3 * 4, s);          // (diagnostics: the partials this norm consumed, then its table)
    dbg_sum(c, g.ss, (size_t)B * n.c * 2 * 4, s);
    const double bytes = (double)B * HW * n.c * ((xdt == 1 ? 4.0 : 2.0) + (out_fp8 ? 1.0 : 2.0));     // algorithmic bytes: one read + one bf16 / fp8 write
    return profiled(c, s, VT_PROF_GN_APPLY, bytes, "gn_apply", [&] { return vt_launch_gn_apply(x, xdt, g.ss, y, B, HW, n.c, silu, s, o8, c->status, out_f16); });
}

// fp16-operand mode (vt_set_flag 18): does THIS conv multiply fp16 operands?  A 16-bit operand tensor carries fp16 bits exactly when its
// consumer says yes here, so producer and consumer sites ask the same question.  Not in fp8 mode; the kernels that have an fp16 form are the
// default halo tile (plain input), the stride-2 phase-plane kernel and the 32-cout GEMM tile (conv_out).
bool conv_f16(const vt_context* c, const ConvW& w, int stride, bool has_sc) {
    if (!c->f16_ops || c->fp8 || w.k != 3) return false;
    if (stride == 2) return c->s2_halo && w.wp2_16 != nullptr;
    return c->use_halo_conv && w.wp && w.wp16 && !c->fuse_gn_apply && vt_conv3x3_halo_f16_supported(w.cout, c->halo_occ2, has_sc ? 1 : 0);
}   // (conv_out, the one conv on the 32-cout GEMM tile, is decided where it is launched)

namespace {

// One run_conv call with the residual-stream pointers resolved by type: what each kernel family below fills its arguments from.
struct ConvCall {
    const ConvW& w; const bf16_t* x; int B, Hin, Win, stride, pad, Hout, Wout; bf16_t* o16; hipStream_t s; const ConvOpts& o;
    const float* res32; const f16_t* res16; float* o32; f16_t* oh16;
    int cpg; bool fuse;                 // fuse: the epilogue writes the GroupNorm partials of the output into o.gn
    double flops() const { return 2.0 * B * (double)Hout * Wout * w.cout * 9.0 * w.cin; }
};

// stride-2 conv on e4m3 operands (x = e4m3(FP8_RES_SCALE * h)), phase-plane kernel
int conv_s2_fp8(vt_context* c, const ConvCall& k) {
    const ConvW& w = k.w;
    Conv3x3S2Fp8Args h{};
    h.X = (const unsigned char*)k.x; h.Wp = w.wp8s2; h.mult = w.mult8g; h.bias = w.b; h.res = k.res32;
    h.out_f32 = k.o32; h.out_f16 = k.oh16; h.out_bf16 = k.o16; h.zeros = c->zeros;
    h.batch = k.B; h.H = k.Hin; h.W = k.Win; h.Cin = w.cin; h.Cout = w.cout; h.x_planar = k.o.planar;
    if (k.fuse) { h.gn_partial = k.o.gn->partial; h.gn_cpg = k.cpg; k.o.gn->parts = vt_conv3x3_s2_fp8_tiles(k.Hout, k.Wout); }
    return profiled(c, k.s, VT_PROF_S2_HALO_FP8, k.flops(), "conv3x3_s2_fp8", [&] { return vt_launch_conv3x3_s2_fp8(h, k.s); });
}

// ... or the generic implicit GEMM with the fp8 MFMA
int conv_gemm_fp8(vt_context* c, const ConvCall& k) {
    const ConvW& w = k.w;
    ConvGemmArgs a{};
    a.X = k.x; a.W = (const bf16_t*)w.w8g; a.f8 = 1; a.col_scale = w.mult8g;
    a.bias = w.b; a.res = k.res32; a.res_f16 = k.res16; a.out_f32 = k.o32; a.out_f16 = k.oh16; a.out_bf16 = k.o16; a.zeros = c->zeros;
    a.Hin = k.Hin; a.Win = k.Win; a.Hout = k.Hout; a.Wout = k.Wout; a.Cin = w.cin; a.Cout = w.cout; a.Wrows = w.cout;
    a.ksize = 3; a.stride = 2; a.pad = k.pad;
    a.ldx = w.cin; a.ldw = 9 * w.cin; a.ldo = w.cout; a.ldr = w.cout;
    a.x_bs = (long long)k.Hin * k.Win * w.cin; a.w_bs = 0; a.o_bs = (long long)k.Hout * k.Wout * w.cout; a.r_bs = a.o_bs;
    a.batch = k.B; a.alpha = 1.f; a.bias_mode = 1; a.out_mode = 0; a.short_tiles = c->gemm_short;
    if (k.fuse && w.cout > 32 && (w.cout % (w.cout <= 128 ? 128 : 256)) == 0) {
        a.gn_partial = k.o.gn->partial; a.gn_cpg = k.cpg; k.o.gn->parts = vt_conv_gemm_ptiles_of(a);
    }
    return profiled(c, k.s, VT_PROF_GEMM_FP8, k.flops(), "conv_gemm_fp8", [&] { return vt_launch_conv_gemm(a, k.s); });
}

// stride-1 conv on e4m3 operands (conv3x3_halo_fp8.hip)
int conv_halo_fp8(vt_context* c, const ConvCall& k) {
    const ConvW& w = k.w; const ScFuse* sc = k.o.sc;
    Conv3x3Fp8Args h{};
    h.X = (const unsigned char*)k.x; h.Wp = w.wp8; h.mult = w.mult8; h.bias = w.b; h.res = k.res32; h.res_f16 = k.res16;
    h.out_f32 = k.o32; h.out_f16 = k.oh16; h.out_bf16 = k.o.o16_e4m3 ? nullptr : k.o16; h.zeros = c->zeros;
    if (k.o.o16_e4m3) { h.out_e4m3 = (unsigned char*)k.o16; h.out_e4m3_scale = FP8_RES_SCALE; h.status = c->status; h.out8_planar = k.o.planar; }
    else if (k.o.planar) return c->fail(VT_ERR_STATE, "internal: planar bf16 copy requested from the fp8 conv");
    h.batch = k.B; h.H = k.Hin; h.W = k.Win; h.Cin = w.cin; h.Cout = w.cout;
    if (sc) { h.scX = sc->x; h.scW = sc->wp8; h.scCin = sc->cin; h.bias = sc->bias; }
    h.shape = (w.cin <= 128 || (c->fp8_tile & 4)) ? (c->fp8_tile & 3) : 0;
    if (k.fuse) { h.gn_partial = k.o.gn->partial; h.gn_cpg = k.cpg; k.o.gn->parts = vt_conv3x3_halo_fp8_tiles_shape(k.Hin, k.Win, h.shape); }
    return launch_halo_fp8(c, h, k.s, "conv3x3_halo_fp8");
}

// stride-2 conv on 16-bit operands, phase-plane kernel (conv3x3_s2_halo.hip)
int conv_s2(vt_context* c, const ConvCall& k) {
    const ConvW& w = k.w;
    Conv3x3S2Args h{};
    h.X = k.x; h.Wp = k.o.x_f16 ? w.wp2_16 : w.wp2; h.bias = w.b; h.res = k.res32; h.out_f32 = k.o32; h.out_f16 = k.oh16; h.out_bf16 = k.o16; h.zeros = c->zeros;
    h.batch = k.B; h.H = k.Hin; h.W = k.Win; h.Cin = w.cin; h.Cout = w.cout; h.f16 = k.o.x_f16; h.out16_f16 = k.o.o16_f16; h.x_planar = k.o.planar;
    if (k.fuse) { h.gn_partial = k.o.gn->partial; h.gn_cpg = k.cpg; k.o.gn->parts = vt_conv3x3_s2_tiles(k.Hout, k.Wout); }
    return profiled(c, k.s, VT_PROF_S2_HALO, k.flops(), "conv3x3_s2", [&] { return vt_launch_conv3x3_s2(h, k.s); });
}

// the default: stride-1 3x3 on the halo kernel (conv3x3_halo.hip), optionally with the norm or the shortcut fused in
int conv_halo(vt_context* c, const ConvCall& k) {
    const ConvW& w = k.w; const ConvOpts& o = k.o;
    Conv3x3Args h{};
    h.X = o.xnorm_f32 ? nullptr : k.x; h.Xf32 = o.xnorm_f32; h.scale_shift = o.ss;
    h.Wp = o.x_f16 ? w.wp16 : w.wp; h.bias = w.b; h.res = k.res32; h.res_f16 = k.res16; h.out_f32 = k.o32; h.out_f16 = k.oh16; h.out_bf16 = k.o16; h.zeros = c->zeros;
    h.batch = k.B; h.H = k.Hin; h.W = k.Win; h.Cin = w.cin; h.Cout = w.cout; h.f16 = o.x_f16; h.out16_f16 = o.o16_f16; h.out16_planar = o.planar;
    if (o.sc) { h.scX = o.sc->x; h.scW = o.x_f16 ? o.sc->wp16 : o.sc->wp; h.scCin = o.sc->cin; h.bias = o.sc->bias; }
    if (k.fuse) { h.gn_partial = o.gn->partial; h.gn_cpg = k.cpg; o.gn->parts = vt_conv3x3_halo_tiles(k.Hin, k.Win, w.cout, o.ss ? (o.xnorm_f32 ? 1 : 2) : 0, c->halo_occ2, o.sc != nullptr); }
    VTCK(launch_halo(c, h, k.s, "conv3x3_halo"));
    if (c->dbg_on) {                                           // diagnostics: the conv's stored output (whichever type the stream has)
        const size_t ne = (size_t)k.B * k.Hin * k.Win * w.cout;
        if (k.oh16) dbg_sum(c, k.oh16, ne * 2, k.s); else if (k.o32) dbg_sum(c, k.o32, ne * 4, k.s); else if (k.o16) dbg_sum(c, k.o16, ne * 2, k.s);
    }
    return VT_OK;
}

// everything else: the generic implicit GEMM (conv_gemm.hip)
int conv_gemm(vt_context* c, const ConvCall& k) {
    const ConvW& w = k.w;
    ConvGemmArgs a{};
    a.X = k.x; a.W = w.w; a.bias = w.b; a.res = k.res32; a.res_f16 = k.res16; a.out_f32 = k.o32; a.out_f16 = k.oh16; a.out_bf16 = k.o16; a.zeros = c->zeros;
    a.Hin = k.Hin; a.Win = k.Win; a.Hout = k.Hout; a.Wout = k.Wout; a.Cin = w.cin; a.Cout = w.cout; a.Wrows = w.cout;
    a.ksize = w.k; a.stride = k.stride; a.pad = k.pad;
    a.ldx = w.cin; a.ldw = w.k * w.k * w.cin; a.ldo = w.cout; a.ldr = w.cout;
    a.x_bs = (long long)k.Hin * k.Win * w.cin; a.w_bs = 0; a.o_bs = (long long)k.Hout * k.Wout * w.cout; a.r_bs = a.o_bs;
    a.batch = k.B; a.alpha = 1.f; a.bias_mode = 1; a.out_mode = 0;
    if (k.fuse && w.cout > 32 && (w.cout % (w.cout <= 128 ? 128 : 256)) == 0) {
        a.short_tiles = c->gemm_short;
        a.gn_partial = k.o.gn->partial; a.gn_cpg = k.cpg; k.o.gn->parts = vt_conv_gemm_ptiles_of(a);
    }
    return launch_gemm(c, a, k.s, "conv_gemm");
}

}  // namespace

// One conv of the encoder on whichever kernel takes it; the conditions are tested in this order.
int run_conv(vt_context* c, const ConvW& w, const bf16_t* x, int B, int Hin, int Win, int stride, int pad, int Hout, int Wout,
             const void* res, void* oh, bf16_t* o16, hipStream_t s, const ConvOpts& o) {
    const int cpg = w.cout / o.groups;
    const ConvCall k{w, x, B, Hin, Win, stride, pad, Hout, Wout, o16, s, o,
                     o.rdt == 1 ? (const float*)res : nullptr, o.rdt == 2 ? (const f16_t*)res : nullptr, o.rdt == 1 ? (float*)oh : nullptr, o.rdt == 2 ? (f16_t*)oh : nullptr,
                     cpg, o.gn && c->fuse_gn_stats && (cpg == 4 || cpg == 8 || cpg == 16)};
    if (o.gn) o.gn->parts = 0;
    if (o.x_fp8 && stride == 2) {
        if (!w.w8g || w.k != 3 || o.ss || o.sc || o.o16_e4m3) return c->fail(VT_ERR_STATE, "internal: fp8 operands requested for a conv the fp8 GEMM cannot run");
        if (c->s2_halo && w.wp8s2 && pad == 0 && Hout == Hin / 2 && Wout == Win / 2 && !k.res16) return conv_s2_fp8(c, k);
        return conv_gemm_fp8(c, k);
    }
    if (o.x_fp8) {
        if (!w.wp8 || w.k != 3 || stride != 1 || pad != 1 || o.ss || (o.sc && !o.sc->wp8)) return c->fail(VT_ERR_STATE, "internal: fp8 operands requested for a conv the fp8 kernel cannot run");
        return conv_halo_fp8(c, k);
    }
    if (c->s2_halo && w.wp2 && w.k == 3 && stride == 2 && pad == 0 && Hout == Hin / 2 && Wout == Win / 2 && !k.res16 && !o.ss && !o.sc && !o.xnorm_f32) return conv_s2(c, k);
    if (c->use_halo_conv && w.wp && w.k == 3 && stride == 1 && pad == 1 && Hout == Hin && Wout == Win) return conv_halo(c, k);
    if (o.ss || o.sc) return c->fail(VT_ERR_STATE, "internal: fused norm / shortcut requested for a conv the halo kernel cannot run");
    if (o.x_f16 || o.o16_f16 || o.planar) return c->fail(VT_ERR_STATE, "internal: fp16 operands / a planar layout requested for a conv on the generic GEMM");
    return conv_gemm(c, k);
}

static bool norm_conv_fusable(const vt_context* c, const ConvW& w, int cin) {
    return c->fuse_gn_apply && c->use_halo_conv && w.wp && w.k == 3 && cin * 8 <= 8192;
}

// conv3x3(silu(GroupNorm(x))) with x fp32 (x32) or bf16 (x16).  Statistics come from the producer's epilogue
// when available (gn.parts > 0); the normalise+SiLU runs inside the conv's halo staging when the halo kernel
// applies, otherwise as the standalone pass into `act`.
// x: the tensor to normalise (xdt 0 = bf16 conv output, 1 = fp32 / 2 = fp16 residual stream); res / oh: residual in / out (rdt).
int run_norm_conv(vt_context* c, const NormW& n, const ConvW& w, const void* x, int xdt, int B, int H, int W,
                  int groups, bf16_t* act, const void* res, void* oh, bf16_t* o16, GnState& gn, bool want_stats,
                  hipStream_t s, int rdt, const NormConvOpts& nc) {
    const ScFuse* sc = nc.sc;
    const bool f8 = c->fp8 && w.wp8 && w.k == 3 && (!sc || sc->wp8);      // fp8 operands: the GroupNorm-apply pass writes e4m3, the conv reads it
    if (nc.o16_e4m3 && !f8) return c->fail(VT_ERR_STATE, "internal: e4m3 output requested from a bf16 conv");
    ConvOpts o;
    o.gn = want_stats ? &gn : nullptr; o.groups = groups; o.rdt = rdt;
    if (f8 || xdt == 2 || !norm_conv_fusable(c, w, n.c)) {   // (the fused staging reads fp32 or bf16 only)
        // fp16-operand mode: the pass writes fp16, the conv multiplies fp16 -- a fused shortcut's input must then carry fp16 bits too
        const bool h16 = !f8 && conv_f16(c, w, 1, sc != nullptr) && (!sc || sc->x_f16);
        if (sc && sc->x_f16 && !h16) return c->fail(VT_ERR_STATE, "internal: fp16 shortcut input for a bf16 conv");
        VTCK(run_gn(c, x, xdt, B, H * W, n, groups, 1, act, gn, s, f8, h16));
        o.sc = sc; o.x_fp8 = f8; o.o16_e4m3 = nc.o16_e4m3; o.x_f16 = h16; o.o16_f16 = nc.o16_f16; o.planar = nc.o16_planar;
        return run_conv(c, w, act, B, H, W, 1, 1, H, W, res, oh, o16, s, o);
    }
    if (nc.o16_planar) return c->fail(VT_ERR_STATE, "internal: planar copy requested from the fused-norm staging path");
    if (sc) return c->fail(VT_ERR_STATE, "internal: fused shortcut with the fused-norm staging");
    int parts = gn.parts;
    if (parts == 0) HIPCK(c, vt_launch_gn_stats(x, xdt, B, H * W, n.c, groups, gn.partial, &parts, s), "gn_stats");
    gn.parts = 0;
    HIPCK(c, vt_launch_gn_finalize(gn.partial, parts, B, n.c, groups, 1e-6f, n.g, n.b, gn.ss, s, c->status), "gn_finalize");
    // (x_f16 / o16_f16 are not forwarded here: fp16 operands with vt_set_flag 2 -- the open advisor finding, a follow-up of its own)
    o.xnorm_f32 = xdt == 1 ? (const float*)x : nullptr; o.ss = gn.ss;
    return run_conv(c, w, xdt == 0 ? (const bf16_t*)x : nullptr, B, H, W, 1, 1, H, W, res, oh, o16, s, o);
}

namespace {

// ---- encoder plan ---------------------------------------------------------------------------------
struct EncPlan : VaePlan {
    int hl = 0, wl = 0;        // latent spatial size
};

EncPlan plan_encoder(const EncoderW& e, int B, int H, int W) {
    EncPlan p;
    int h = H, w = W;
    // the producers of GroupNorm partials that only the encoder has: both conv_in kernels, the fp8 halo conv, the stride-2 kernels
    auto note = [&](int hh, int ww, int ch) {
        p.note(hh, ww, ch, std::max({vt_conv_in_parts(hh, ww), vt_conv_in_mfma_parts(hh, ww), vt_conv3x3_halo_fp8_tiles(hh, ww),
                                     vt_conv3x3_s2_tiles(hh, ww), vt_conv3x3_s2_fp8_tiles(hh, ww)}));
    };
    note(h, w, e.block_out[0]);
    for (size_t i = 0; i < e.block_out.size(); ++i) {
        note(h, w, e.block_out[i]);
        if (i + 1 < e.block_out.size()) { h /= 2; w /= 2; note(h, w, e.block_out[i]); }
    }
    p.hl = h; p.wl = w;
    p.finish(B, e.groups, h * w, e.block_out.back());
    return p;
}

// One vt_encode call: the shared run plus what only the encoder has, conv_in and the down stages.
struct EncRun : VaeRun {
    const EncoderW& e;

    EncRun(vt_context* c_, const EncPlan& p, int B_, int H, int W, void* ws, hipStream_t s_) : VaeRun(c_, c_->enc.groups, B_, H, W, s_), e(c_->enc) {
        carve(p, ws);
    }

    int conv_in(const float* x) {
        const int cpg0 = e.block_out[0] / e.groups;
        const bool fuse0 = c->fuse_gn_stats && (cpg0 % 4) == 0;
        int parts = 0;
        float* o32 = rdt == 1 ? (float*)f32[cur] : nullptr;
        f16_t* oh = rdt == 2 ? (f16_t*)f32[cur] : nullptr;
        if (c->conv_in_mfma && e.conv_in_wpk) {
            HIPCK(c, vt_launch_conv_in_mfma(x, e.conv_in_wpk, e.conv_in_b, o32, nullptr, oh, fuse0 ? gn.partial : nullptr, &parts,
                                            B, h, w, s), "conv_in_mfma");
        } else {
            HIPCK(c, vt_launch_conv_in(x, e.conv_in_w, e.conv_in_b, o32, nullptr, oh, fuse0 ? gn.partial : nullptr, cpg0, &parts,
                                       B, h, w, e.block_out[0], s), "conv_in");
        }
        gn.parts = fuse0 ? parts : 0;
        return VT_OK;
    }

    // the resnet blocks of one stage and, unless it is the last, its Downsample2D
    int stage(size_t i) {
        const StageW& st = e.stages[i];
        BlockOut hbo;                                  // how the last block wrote `hb`
        for (size_t j = 0; j < st.res.size(); ++j) {
            const ResnetW& rw = st.res[j];
            const bool last = j + 1 == st.res.size();
            BlockOut out;
            out.only16 = last && st.has_down;
            // fp8 mode: the last block of a stage hands its output to the stride-2 conv as e4m3 when both run on fp8 operands
            out.e4m3 = out.only16 && c->fp8 && st.down.w8g && rw.c2.wp8 && !rw.has_sc;
            // fp16-operand mode: the block output for the stride-2 conv carries fp16 bits when that conv multiplies fp16 (conv_f16)
            out.f16 = out.only16 && !out.e4m3 && conv_f16(c, st.down, 2, false);
            // the copy is chunk-planar when the stride-2 conv that reads it runs on a phase-plane kernel (and the producer is a halo kernel that can write it so)
            out.planar = out.only16 && c->s2_planar && c->s2_halo && !c->fuse_gn_apply &&
                         (out.e4m3 ? st.down.wp8s2 != nullptr : (st.down.wp2 != nullptr && c->use_halo_conv && rw.c2.wp && !(c->fp8 && rw.c2.wp8)));
            VTCK(resnet(rw, out));
            if (last) hbo = out;
            if (out.only16) h16 = hb;
        }
        if (!st.has_down) return VT_OK;
        // Downsample2D(padding=0): F.pad(x,(0,1,0,1)) then conv3x3 stride 2 -> out = floor(in/2)
        const int ho = h / 2, wo = w / 2;
        const int nxt = (cur + 1) % 3;
        const ResnetW* next = (i + 1 < e.stages.size() && e.stages[i + 1].res[0].has_sc) ? &e.stages[i + 1].res[0] : nullptr;
        // the bf16 copy of the new h for the next block's shortcut: in tmid when a separate shortcut conv consumes it
        // before conv1 overwrites tmid; when the shortcut is fused into conv2 it must outlive conv1, so it goes to the
        // third rotating buffer (the block's `scb`, free now that no shortcut tensor is written)
        bf16_t* copy = !next ? nullptr : (fuse_sc(*next) ? (bf16_t*)f32[(nxt + 2) % 3] : tmid);
        // ... and the bf16 copy for the next block's FUSED shortcut carries fp16 bits when that block's conv2 does
        // (only the phase-plane kernel can write them; on the generic GEMM the copy stays bf16 and that conv2 keeps bf16 operands)
        const bool copy16 = copy && fuse_sc(*next) && conv_f16(c, next->c2, 1, true) && c->s2_halo && st.down.wp2 && !hbo.e4m3;
        ConvOpts o;
        o.gn = &gn; o.groups = groups; o.rdt = rdt; o.x_fp8 = hbo.e4m3; o.x_f16 = hbo.f16; o.o16_f16 = copy16; o.planar = hbo.planar;
        VTCK(run_conv(c, st.down, hb, B, h, w, 2, 0, ho, wo, nullptr, f32[nxt], copy, s, o));
        h16 = copy; h16_is_f16 = copy16;
        cur = nxt; h = ho; w = wo;
        return VT_OK;
    }
};

}  // namespace
}  // namespace vt

using namespace vt;

extern "C" {

int vt_encoder_configure(vt_context* c, int in_ch, int latent, const int* block_out, int n_blocks, int layers,
                         int groups, float scaling, int has_scaling, float shift, int has_shift) {
    if (!c) return VT_ERR_INVALID;
    if (in_ch != 3) return c->fail(VT_ERR_INVALID, "in_channels must be 3 (got %d)", in_ch);
    if (!block_out || n_blocks < 1 || n_blocks > 8 || layers < 1 || layers > 8 || latent < 1 || groups < 1)
        return c->fail(VT_ERR_INVALID, "bad encoder configuration");
    EncoderW& e = c->enc;
    { DeviceGuard guard(c); c->free_allocs(c->enc_allocs); }       // a re-upload (load_state_dict / .to()) replaces the packed weights
    e = EncoderW();
    e.in_ch = in_ch; e.latent = latent; e.layers = layers; e.groups = groups;
    e.block_out.assign(block_out, block_out + n_blocks);
    VTCK(check_block_out(c, block_out, n_blocks, groups));
    if (2 * latent > 32 || (2 * latent) % 4) return c->fail(VT_ERR_INVALID, "latent_channels must be <= 16 and even");
    e.scaling = scaling; e.has_scaling = has_scaling != 0; e.shift = shift; e.has_shift = has_shift != 0;
    e.configured = true;
    return VT_OK;
}

size_t vt_encode_workspace_bytes(const vt_context* c, int B, int H, int W) {
    if (!c || !c->enc.configured || B <= 0 || H < 8 || W < 8) return 0;
    return plan_encoder(c->enc, B, H, W).total;
}

double vt_encoder_flops(const vt_context* c, int H, int W) {
    if (!c || !c->enc.configured) return 0.0;
    const EncoderW& e = c->enc;
    double f = 2.0 * H * W * 27 * e.block_out[0];
    int h = H, w = W, ci = e.block_out[0];
    for (size_t i = 0; i < e.block_out.size(); ++i) {
        const int co = e.block_out[i];
        for (int j = 0; j < e.layers; ++j) {
            f += 2.0 * h * w * 9 * ci * co + 2.0 * h * w * 9 * co * co;
            if (ci != co) f += 2.0 * h * w * ci * co;
            ci = co;
        }
        if (i + 1 < e.block_out.size()) { h /= 2; w /= 2; f += 2.0 * h * w * 9 * co * co; }
    }
    const double s = (double)h * w, C = ci;
    f += 4 * (2.0 * s * 9 * C * C) + 4 * (2.0 * s * C * C) + 2 * (2.0 * s * s * C) + 2.0 * s * 9 * C * 2 * e.latent;
    return f;
}

int vt_encode(vt_context* c, const float* x, int B, int H, int W, int mode, float* latent, void* ws, size_t ws_bytes,
              void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    const EncoderW& e = c->enc;
    if (!e.finalized) return c->fail(VT_ERR_STATE, "encoder weights not finalized");
    if (!x || !latent || !ws || B <= 0) return c->fail(VT_ERR_INVALID, "vt_encode: null buffer or B <= 0");
    if (mode < 0 || mode > 2) return c->fail(VT_ERR_INVALID, "vt_encode: mode must be 0 (moments), 1 (mode) or 2 (mode*scale+shift)");
    const int nd = (int)e.block_out.size() - 1;
    if ((H >> nd) < 1 || (W >> nd) < 1) return c->fail(VT_ERR_INVALID, "vt_encode: image %dx%d too small", H, W);
    const EncPlan p = plan_encoder(e, B, H, W);
    if (ws_bytes < p.total) return c->fail(VT_ERR_WORKSPACE, "vt_encode: workspace %zu < required %zu", ws_bytes, p.total);
    if (((uintptr_t)ws) % ALIGN) return c->fail(VT_ERR_INVALID, "vt_encode: workspace must be 256-B aligned");
    EncRun run(c, p, B, H, W, ws, (hipStream_t)stream);
    VTCK(run.conv_in(x));
    for (size_t i = 0; i < e.stages.size(); ++i) VTCK(run.stage(i));
    VTCK(run.resnet(e.mid0));
    VTCK(run.mid_attention(e.attn));
    VTCK(run.resnet(e.mid1));
    // conv_norm_out + conv_out -> moments (mode 0) / mode() = mean = the first `latent` channels (mode 1) / * scaling + shift (mode 2)
    return run.conv_out(e.conv_out, e.norm_out, mode == 0 ? 2 * e.latent : e.latent, (mode == 2 && e.has_scaling) ? e.scaling : 1.f,
                        (mode == 2 && e.has_shift) ? e.shift : 0.f, latent);
}

size_t vt_encode_tag_workspace_bytes(const vt_context* c, int B, int H, int W) {
    if (!c || !c->enc.configured || !c->dec_configured || B <= 0 || H < 8 || W < 8) return 0;
    const EncPlan p = plan_encoder(c->enc, B, H, W);
    const size_t lat_bytes = align_up((size_t)B * c->enc.latent * p.hl * p.wl * 4);
    const size_t dec_bytes = vt_decode_workspace_bytes(c, B, p.hl, p.wl);
    return lat_bytes + (p.total > dec_bytes ? p.total : dec_bytes) + ALIGN;
}

int vt_encode_tag(vt_context* c, const float* x, int B, int H, int W, float* latent_out, float* logits, void* ws,
                  size_t ws_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    if (!c->enc.finalized || !c->dec_finalized) return c->fail(VT_ERR_STATE, "weights not finalized");
    if (!ws || ((uintptr_t)ws % ALIGN)) return c->fail(VT_ERR_INVALID, "vt_encode_tag: workspace must be 256-B aligned");
    const size_t need = vt_encode_tag_workspace_bytes(c, B, H, W);
    if (need == 0 || ws_bytes < need) return c->fail(VT_ERR_WORKSPACE, "vt_encode_tag: workspace %zu < required %zu", ws_bytes, need);
    const EncPlan p = plan_encoder(c->enc, B, H, W);
    const size_t lat_bytes = align_up((size_t)B * c->enc.latent * p.hl * p.wl * 4);
    // layout: [latent][encoder scratch, reused as decoder scratch once the encoder is done (same stream)]
    float* lat = latent_out ? latent_out : (float*)ws;
    char* rest = (char*)ws + lat_bytes;
    VTCK(vt_encode(c, x, B, H, W, 2, lat, rest, ws_bytes - lat_bytes, stream));
    return vt_decode_logits(c, lat, B, p.hl, p.wl, logits, rest, ws_bytes - lat_bytes, stream);
}

}  // extern "C"
