// The run layer shared by the VAE encoder's and the image decoder's launch schedules (host code; vt_vae_run.h): workspace plan and carve,
// the ResnetBlock2D / mid-attention / conv_out steps over the rotating buffers, the block_out validation of both configure entries.
#include <algorithm>

#include "vt_vae_run.h"

namespace vt {

void VaePlan::note(int h, int w, int ch, int own_parts) {
    max_elems = std::max(max_elems, (size_t)h * w * ch);
    max_c = std::max(max_c, ch);
    // GroupNorm partials: the most triples per (image, group) that any producer of this tensor writes
    max_chunks = std::max({max_chunks, vt_gn_max_chunks(h * w, ch), vt_conv_gemm_ptiles(h * w, ch), vt_conv3x3_halo_tiles_max(h, w), own_parts});
}

void VaePlan::finish(int B, int groups, int S_, int C_, size_t extra) {
    S = S_; C = C_;
    max_chunks = std::max(max_chunks, vt_attn_linear_parts(S));     // to_out's GroupNorm partials: one per 32-token slab (attn_qk.hip, mode 5)
    total = 3 * align_up(max_elems * B * 4 + SLACK) + 3 * align_up(max_elems * B * 2 + SLACK) +
            align_up((size_t)B * max_chunks * groups * 3 * 4) + align_up((size_t)B * max_c * 2 * 4) + extra +
            attn_scratch_bytes(B, S, C) + ALIGN;
}

int check_block_out(vt_context* c, const int* block_out, int n, int groups) {
    for (int i = 0; i < n; ++i) {
        const int ch = block_out[i];
        if (ch % groups || ch % 64 || ch > 2048) return c->fail(VT_ERR_INVALID, "block_out_channels entries must be multiples of 64 and of norm_num_groups (got %d)", ch);
        const int cpg = ch / groups;
        if (cpg < 2 || (cpg & (cpg - 1)) || (256 % (ch / 8))) return c->fail(VT_ERR_INVALID, "unsupported channels/groups combination %d/%d", ch, groups);
    }
    return VT_OK;
}

char* VaeRun::carve(const VaePlan& p, void* ws, size_t extra) {
    char* q = (char*)ws;
    for (int i = 0; i < 3; ++i) { f32[i] = (void*)q; q += align_up(p.max_elems * B * 4 + SLACK); }
    for (int i = 0; i < 3; ++i) { b16[i] = (bf16_t*)q; q += align_up(p.max_elems * B * 2 + SLACK); }
    gn.partial = (float*)q; q += align_up((size_t)B * p.max_chunks * groups * 3 * 4);
    gn.ss = (float*)q; q += align_up((size_t)B * p.max_c * 2 * 4);
    as = carve_attn(q + extra, B, p.S, p.C);
    act = b16[0]; tmid = b16[1]; hb = b16[2];
    return q;
}

bool VaeRun::fuse_sc(const ResnetW& rw) const {
    return c->fuse_shortcut && rw.sc_wp && c->use_halo_conv && rw.c2.wp && !c->fuse_gn_apply && (!(c->fp8 && rw.c2.wp8) || rw.sc_wp8);
}

int VaeRun::resnet(const ResnetW& rw, const BlockOut& out) {
    const int nxt = (cur + 1) % 3, scb = (cur + 2) % 3;
    const void* res = f32[cur];
    if (rw.has_sc && !h16) return c->fail(VT_ERR_STATE, "internal: shortcut conv without a 16-bit input");
    const ScFuse scf{h16, rw.sc_wp, rw.b_c2sc, rw.cin, rw.sc_wp8, rw.sc_wp16, h16_is_f16};
    NormConvOpts c2;
    if (rw.has_sc) {
        if (fuse_sc(rw)) {
            // conv_shortcut rides in conv2's launch (extra K-steps on the 16-bit copy of the block input, which the stride-2 /
            // Upsample2D conv left in f32[scb]): no shortcut tensor is written or read back
            c2.sc = &scf; res = nullptr;
        } else {
            ConvOpts o; o.rdt = rdt;
            VTCK(run_conv(c, rw.sc, h16, B, h, w, 1, 0, h, w, nullptr, f32[scb], nullptr, s, o));
            res = f32[scb];
        }
    }
    // conv1's output is only ever read by norm2: with the fp16 storage mode it is kept as fp16 too (11 significand
    // bits instead of bf16's 8 at the same 2 B: one of the three 8-bit roundings per resnet block disappears)
    const bool c1h = rdt == 2;
    const int c1dt = c1h ? 2 : 0;
    VTCK(run_norm_conv(c, rw.n1, rw.c1, f32[cur], rdt, B, h, w, groups, act, nullptr, c1h ? (void*)tmid : nullptr,
                       c1h ? nullptr : tmid, gn, true, s, rdt));
    h16 = nullptr; h16_is_f16 = false;
    if (out.only16) {
        c2.o16_e4m3 = out.e4m3; c2.o16_f16 = out.f16; c2.o16_planar = out.planar;
        return run_norm_conv(c, rw.n2, rw.c2, tmid, c1dt, B, h, w, groups, act, res, nullptr, hb, gn, false, s, rdt, c2);
    }
    VTCK(run_norm_conv(c, rw.n2, rw.c2, tmid, c1dt, B, h, w, groups, act, res, f32[nxt], nullptr, gn, true, s, rdt, c2));
    cur = nxt;
    return VT_OK;
}

int VaeRun::mid_attention(const AttnW& attn) {
    const int S = h * w, nxt = (cur + 1) % 3;
    const bool tok8 = attn_proj_is_fp8(c, attn, S, attn.c);       // the tokens leave the GroupNorm pass as e4m3(8 x): the projections' operand
    VTCK(run_gn(c, f32[cur], rdt, B, S, attn.gn, groups, 0, act, gn, s, tok8));
    VTCK(run_attention(c, attn, act, f32[cur], f32[nxt], B, S, as, s, &gn, groups, rdt, tok8));
    cur = nxt;
    return VT_OK;
}

int VaeRun::conv_out(const ConvW& cw, const NormW& norm, int keep, float post_scale, float post_shift, float* out) {
    const bool out16 = cw.cout <= 32 && cw.w16 && c->f16_ops && !c->fp8;      // fp16-operand mode: conv_out multiplies fp16 too (both of its kernels have the form)
    VTCK(run_gn(c, f32[cur], rdt, B, h * w, norm, groups, 1, act, gn, s, false, out16));
    if (c->conv_out_halo && cw.wpo && cw.k == 3 && keep <= cw.cout) {
        // on its 32-cout halo tile
        ConvOutArgs o{};
        o.X = act; o.Wp = out16 ? cw.wpo16 : cw.wpo; o.f16 = out16; o.bias = cw.b; o.out = out; o.zeros = c->zeros;
        o.batch = B; o.H = h; o.W = w; o.Cin = cw.cin; o.Cout = cw.cout; o.keep = keep;
        o.post_scale = post_scale; o.post_shift = post_shift;
        return profiled(c, s, VT_PROF_CONV_OUT, 2.0 * B * (double)h * w * cw.cout * 9.0 * cw.cin, "conv_out_halo", [&] { return vt_launch_conv_out_halo(o, s); });
    }
    ConvGemmArgs a{};
    a.X = act; a.W = out16 ? cw.w16 : cw.w; a.f16 = out16; a.bias = cw.b; a.out_f32 = out; a.zeros = c->zeros;
    a.Hin = a.Hout = h; a.Win = a.Wout = w; a.Cin = cw.cin; a.Cout = cw.cout; a.Wrows = cw.cout;
    a.ksize = 3; a.stride = 1; a.pad = 1; a.ldx = cw.cin; a.ldw = 9 * cw.cin; a.ldo = cw.cout;
    a.cout_keep = keep;
    a.x_bs = (long long)h * w * cw.cin; a.o_bs = (long long)a.cout_keep * h * w; a.batch = B; a.alpha = 1.f;
    a.bias_mode = 1; a.out_mode = 1;
    a.post_scale = post_scale; a.post_shift = post_shift;
    return launch_gemm(c, a, s, "conv_out");
}

}  // namespace vt
