// Training-mode forward and the core backward of the mid-block attention (host code; kernels: attn_qk.hip, attn_pv.hip, attn_bwd.hip).
// DESIGN.md section 4.20.
#include <math.h>

#include "vt_ops.h"

namespace vt {
namespace {

constexpr int AC = 512;                                       // the only channel count the dedicated kernels take
size_t round64(int S) { return (size_t)(S + 63) / 64 * 64; }

// ---- training forward: workspace = packed weights | GroupNorm scratch | (mean, rstd) scratch | run_attention's scratch
struct FwdWs { bf16_t *wqk, *wv, *wo; float* bqk; char* gn; char* st; char* attn; size_t total; };
FwdWs carve_fwd(char* p, int B, int S, int C) {
    FwdWs w;
    char* p0 = p;
    w.wqk = (bf16_t*)p; p += align_up((size_t)2 * C * C * 2);
    w.wv = (bf16_t*)p; p += align_up((size_t)C * C * 2);
    w.wo = (bf16_t*)p; p += align_up((size_t)C * C * 2);
    w.bqk = (float*)p; p += align_up((size_t)2 * C * 4);
    w.gn = p; p += align_up((size_t)B * vt_gn_max_chunks(S, C) * 64 * 3 * 4) + align_up((size_t)B * C * 2 * 4);
    w.st = p; p += align_up(vt_gn_stats64_ws_bytes(B, S, C));
    w.attn = p; p += attn_scratch_bytes(B, S, C);
    w.total = (size_t)(p - p0);
    return w;
}

// ---- core backward: workspace = small tensors of the whole batch | two fragment-ordered S x S buffers per image of a group
struct BwdWs { bf16_t *do16, *v16, *kT, *qT, *doT, *ofwd; float *dvec, *rinv, *coff, *sums; bf16_t *p0, *p1; size_t total; };
BwdWs carve_bwd(char* p, int B, int S, int C) {
    BwdWs w;
    char* base = p;
    const size_t lp = attn_pitch_of(S), G = (size_t)attn_group_of(B, S), Sp = round64(S);
    w.do16 = (bf16_t*)p; p += align_up((size_t)B * S * C * 2);
    w.v16 = (bf16_t*)p; p += align_up((size_t)B * S * C * 2);
    w.kT = (bf16_t*)p; p += align_up((size_t)B * C * lp * 2);
    w.qT = (bf16_t*)p; p += align_up((size_t)B * C * lp * 2);
    w.doT = (bf16_t*)p; p += align_up((size_t)B * C * lp * 2);
    w.ofwd = (bf16_t*)p; p += align_up((size_t)B * S * C * 2);      // (the stage entry's forward P.V, a measurement aid, writes here)
    w.dvec = (float*)p; p += align_up((size_t)B * Sp * 4);
    w.rinv = (float*)p; p += align_up((size_t)B * Sp * 4);
    w.coff = (float*)p; p += align_up((size_t)B * Sp * 4);
    w.sums = (float*)p; p += align_up((size_t)4 * G * S * 4);
    w.p0 = (bf16_t*)p; p += align_up(G * (size_t)vt_attn_pt_elems(S) * 2);
    w.p1 = (bf16_t*)p; p += align_up(G * (size_t)vt_attn_pt_elems(S) * 2);
    w.total = (size_t)(p - base);
    return w;
}

}  // namespace
}  // namespace vt

using namespace vt;

extern "C" {

int vt_op_attention_vt_pitch(int S) { return S > 0 ? (int)attn_pitch_of(S) : 0; }

size_t vt_op_attention_forward_train_workspace_bytes(int B, int S, int C) {
    if (B <= 0 || S <= 0 || C != AC) return 0;
    return carve_fwd(nullptr, B, S, C).total + ALIGN;
}

int vt_op_attention_forward_train(vt_context* c, const float* x, const float* gn_w, const float* gn_b, const float* wq, const float* bq, const float* wk,
                                  const float* bk, const float* wv, const float* bv, const float* wo, const float* bo, float* y, void* h16, void* qk16, void* vT16,
                                  void* o16, float* o, float* shift, float* sums, float* stats, int B, int S, int C, void* ws, size_t ws_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (C != AC) return c->fail(VT_ERR_INVALID, "vt_op_attention_forward_train: the attention kernels take C = 512 only (got %d)", C);
    if (B <= 0 || S <= 0) return c->fail(VT_ERR_INVALID, "vt_op_attention_forward_train: B and S must be >= 1");
    if (!x || !gn_w || !gn_b || !wq || !bq || !wk || !bk || !wv || !bv || !wo || !bo || !y || !h16 || !qk16 || !vT16 || !o16 || !o || !shift || !sums || !stats)
        return c->fail(VT_ERR_INVALID, "vt_op_attention_forward_train: null buffer");
    if (c->f16_ops || c->fp8 || c->attn_mode != 0 || !c->attn_qk_kernel || !c->attn_pv_kernel || !c->attn_proj_kernel)
        return c->fail(VT_ERR_INVALID, "vt_op_attention_forward_train: runs the default bf16 launches only (flags 7, 9, 11, 12, 17 and 18 at their defaults)");
    VTCK(check_workspace(c, "vt_op_attention_forward_train", ws, ws_bytes, vt_op_attention_forward_train_workspace_bytes(B, S, C), ALIGN));
    hipStream_t s = (hipStream_t)stream;
    const FwdWs w = carve_fwd((char*)ws, B, S, C);
    // weights -> the bf16 operands of the encoder's packing ([Wq; Wk], Wv, Wo row-major; bq | bk), on the stream
    HIPCK(c, vt_launch_cast_bias_grad(wq, w.wqk, nullptr, C, C, nullptr, s), "pack to_q");
    HIPCK(c, vt_launch_cast_bias_grad(wk, w.wqk + (size_t)C * C, nullptr, C, C, nullptr, s), "pack to_k");
    HIPCK(c, vt_launch_cast_bias_grad(wv, w.wv, nullptr, C, C, nullptr, s), "pack to_v");
    HIPCK(c, vt_launch_cast_bias_grad(wo, w.wo, nullptr, C, C, nullptr, s), "pack to_out");
    HIPCK(c, hipMemcpyAsync(w.bqk, bq, (size_t)C * 4, hipMemcpyDeviceToDevice, s), "pack bq");
    HIPCK(c, hipMemcpyAsync(w.bqk + C, bk, (size_t)C * 4, hipMemcpyDeviceToDevice, s), "pack bk");
    // h16 = GroupNorm32(x), eps 1e-6, no SiLU: vt_op_groupnorm's three launches; (mean, rstd) for the backward
    constexpr int GROUPS = 32;
    constexpr float EPS = 1e-6f;
    float* partial = (float*)w.gn;
    float* ss = (float*)(w.gn + align_up((size_t)B * vt_gn_max_chunks(S, C) * 64 * 3 * 4));
    int nchunks = 0;
    HIPCK(c, vt_launch_gn_stats(x, 1, B, S, C, GROUPS, partial, &nchunks, s), "gn_stats");
    HIPCK(c, vt_launch_gn_finalize(partial, nchunks, B, C, GROUPS, EPS, gn_w, gn_b, ss, s), "gn_finalize");
    HIPCK(c, vt_launch_gn_apply(x, 1, ss, (bf16_t*)h16, B, S, C, 0, s), "gn_apply");
    HIPCK(c, vt_launch_gn_stats64(x, B, S, C, GROUPS, EPS, stats, w.st, s), "gn_stats64");
    // the inference schedule on caller-owned operands: q | k, v^T, o and the shift land in the caller's buffers
    AttnW aw;
    aw.wqk = w.wqk; aw.wv = w.wv; aw.wo = w.wo; aw.bqk = w.bqk; aw.bv = bv; aw.bo = bo; aw.c = C;
    AttnScratch sc = carve_attn(w.attn, B, S, C);
    sc.qk = (bf16_t*)qk16; sc.vt = (bf16_t*)vT16; sc.o = (bf16_t*)o16; sc.shift = shift; sc.save_sums = sums;
    VTCK(run_attention(c, aw, (const bf16_t*)h16, x, y, B, S, sc, s));
    HIPCK(c, vt_launch_bf16_to_f32((const bf16_t*)o16, o, (long long)B * S * C, s), "o -> fp32");
    return VT_OK;
}

size_t vt_op_attention_core_backward_workspace_bytes(int B, int S, int C) {
    if (B <= 0 || S <= 0 || C != AC) return 0;
    return carve_bwd(nullptr, B, S, C).total + ALIGN;
}

int vt_op_attention_core_backward(vt_context* c, const void* qk16, const void* vT16, const float* o, const float* dout, const float* shift, const float* sums,
                                  float* dq, float* dk, float* dv, void* dq16, void* dk16, void* dv16, int B, int S, int C, int group, int nsplit, void* ws,
                                  size_t ws_bytes, void* stream) {
    return vt_op_attention_core_backward_stages(c, qk16, vT16, o, dout, shift, sums, dq, dk, dv, dq16, dk16, dv16, B, S, C, group, nsplit, ws, ws_bytes, stream, 0xffu);
}

// bit 0: layout passes; 1: numerators; 2: ds; 3: dq; 4: p^T; 5: dv; 6: ds^T; 7: dk; 8 (not part of the backward): the forward's P.V on whatever the
// first fragment buffer holds
int vt_op_attention_core_backward_stages(vt_context* c, const void* qk16, const void* vT16, const float* o, const float* dout, const float* shift,
                                         const float* sums, float* dq, float* dk, float* dv, void* dq16, void* dk16, void* dv16, int B, int S, int C, int group,
                                         int nsplit, void* ws, size_t ws_bytes, void* stream, unsigned stages) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (C != AC) return c->fail(VT_ERR_INVALID, "vt_op_attention_core_backward: the attention kernels take C = 512 only (got %d)", C);
    if (B <= 0 || S <= 0) return c->fail(VT_ERR_INVALID, "vt_op_attention_core_backward: B and S must be >= 1");
    if (!qk16 || !vT16 || !o || !dout || !shift || !sums || !dq || !dk || !dv) return c->fail(VT_ERR_INVALID, "vt_op_attention_core_backward: null buffer");
    if (group < 0 || nsplit < 0) return c->fail(VT_ERR_INVALID, "vt_op_attention_core_backward: group and nsplit must be >= 0 (0 = chosen from the shape)");
    VTCK(check_workspace(c, "vt_op_attention_core_backward", ws, ws_bytes, vt_op_attention_core_backward_workspace_bytes(B, S, C), ALIGN));
    hipStream_t s = (hipStream_t)stream;
    const BwdWs w = carve_bwd((char*)ws, B, S, C);
    const int lp = (int)attn_pitch_of(S), ld8 = (S + 7) / 8 * 8, Sp = (int)round64(S);
    const int G = attn_group_of(B, S);
    const int grp = group > 0 && group < G ? group : G;            // (the workspace holds G images' buffers)
    const float alpha = 1.0f / sqrtf((float)C);
    const long long pt = vt_attn_pt_elems(S);
    const bf16_t* qk = (const bf16_t*)qk16;
    // ---- layout passes over the whole batch: do16, D, 1 / sum, the key direction's exponent offset; v16 from v^T; k^T, q^T, do^T
    const auto on = [&](int bit) { return (stages >> bit) & 1u; };
    if (on(0)) {
    HIPCK(c, vt_launch_attn_bwd_rows(dout, o, shift, sums, (long long)B * S, w.do16, w.dvec, w.rinv, w.coff, B, S, Sp, s), "attn bwd rows");
    HIPCK(c, vt_launch_transpose16((const bf16_t*)vT16, w.v16, C, S, C, lp, C, (long long)C * lp, (long long)S * C, B, s), "attn bwd v16");
    HIPCK(c, vt_launch_transpose16(qk, w.qT, S, C, ld8, 2 * C, lp, (long long)S * 2 * C, (long long)C * lp, B, s), "attn bwd q^T");
    HIPCK(c, vt_launch_transpose16(qk + C, w.kT, S, C, ld8, 2 * C, lp, (long long)S * 2 * C, (long long)C * lp, B, s), "attn bwd k^T");
    HIPCK(c, vt_launch_transpose16(w.do16, w.doT, S, C, ld8, C, lp, (long long)S * C, (long long)C * lp, B, s), "attn bwd do^T");
    }
    const int nkt = (S + 63) / 64;
    for (int b0 = 0; b0 < B; b0 += grp) {
        const int nb = B - b0 < grp ? B - b0 : grp;
        const int qblocks = nb * ((S + 255) / 256);
        int nsp = nsplit > 0 ? nsplit : attn_sweep_nsplit(qblocks, nkt, 8);
        if (nsp > nkt) nsp = nkt;
        const int nsp_seg = nsp >= 4 ? 4 : nsp >= 2 ? 2 : 1;      // the numerator sweep spreads whole segments: 1, 2 or 4 workgroups
        const bf16_t* qg = qk + (long long)b0 * S * 2 * C;
        // 1. the numerators the forward multiplied: same launch, same shift (its segment sums go to scratch; the forward's are the input)
        AttnQkArgs k{};
        k.q = qg; k.k = qg + C; k.S = S; k.C = C; k.ldq = 2 * C; k.qk_bs = (long long)S * 2 * C; k.row_bs = S; k.alpha = alpha; k.batch = nb; k.zeros = c->zeros;
        k.mode = 2; k.P = w.p0; k.p_frag = 1; k.p_bs = pt; k.rowin = shift + (long long)b0 * S; k.rowout = w.sums; k.split_stride = (long long)nb * S; k.nsplit = nsp_seg;
        if (on(1)) HIPCK(c, vt_launch_attn_qk(k, s), "attn bwd numerators");
        // 2. query direction: ds = alpha p (dp - D), dq = ds k
        AttnBwdQkArgs g{};
        g.S = S; g.C = C; g.batch = nb; g.p_bs = pt; g.vec_bs = Sp; g.alpha = alpha; g.nsplit = nsp; g.zeros = c->zeros;
        g.mode = 0; g.rows = w.do16 + (long long)b0 * S * C; g.ldr = C; g.r_bs = (long long)S * C; g.str = w.v16 + (long long)b0 * S * C; g.lds = C; g.s_bs = (long long)S * C;
        g.Pin = w.p0; g.Pout = w.p1; g.rowscale = w.rinv + (long long)b0 * Sp; g.rowd = w.dvec + (long long)b0 * Sp;
        if (on(2)) HIPCK(c, vt_launch_attn_bwd_qk(g, s), "attn bwd ds");
        AttnBwdPvArgs v{};
        v.S = S; v.C = C; v.batch = nb; v.pt_bs = pt; v.ldx = lp; v.xt_bs = (long long)C * lp; v.ldo = C; v.o_bs = (long long)S * C; v.zeros = c->zeros;
        v.Pt = w.p1; v.xt = w.kT + (long long)b0 * C * lp; v.out = dq + (long long)b0 * S * C; v.out16 = dq16 ? (bf16_t*)dq16 + (long long)b0 * S * C : nullptr;
        if (on(3)) HIPCK(c, vt_launch_attn_bwd_pv(v, s), "attn bwd dq");
        // 3. key direction, roles swapped: p^T, dv = p^T do; ds^T, dk = ds^T q
        g.mode = 1; g.rows = qg + C; g.ldr = 2 * C; g.r_bs = (long long)S * 2 * C; g.str = qg; g.lds = 2 * C; g.s_bs = (long long)S * 2 * C;
        g.Pin = nullptr; g.Pout = w.p0; g.rowscale = nullptr; g.rowd = nullptr; g.colv = w.coff + (long long)b0 * Sp;
        if (on(4)) HIPCK(c, vt_launch_attn_bwd_qk(g, s), "attn bwd p^T");
        v.Pt = w.p0; v.xt = w.doT + (long long)b0 * C * lp; v.out = dv + (long long)b0 * S * C; v.out16 = dv16 ? (bf16_t*)dv16 + (long long)b0 * S * C : nullptr;
        if (on(5)) HIPCK(c, vt_launch_attn_bwd_pv(v, s), "attn bwd dv");
        g.mode = 2; g.rows = w.v16 + (long long)b0 * S * C; g.ldr = C; g.r_bs = (long long)S * C; g.str = w.do16 + (long long)b0 * S * C; g.lds = C; g.s_bs = (long long)S * C;
        g.Pin = w.p0; g.Pout = w.p1; g.colv = w.dvec + (long long)b0 * Sp;
        if (on(6)) HIPCK(c, vt_launch_attn_bwd_qk(g, s), "attn bwd ds^T");
        v.Pt = w.p1; v.xt = w.qT + (long long)b0 * C * lp; v.out = dk + (long long)b0 * S * C; v.out16 = dk16 ? (bf16_t*)dk16 + (long long)b0 * S * C : nullptr;
        if (on(7)) HIPCK(c, vt_launch_attn_bwd_pv(v, s), "attn bwd dk");
        if (on(8)) {
            AttnPvArgs f{};
            f.Pt = w.p0; f.pt_bs = pt; f.vt = (const bf16_t*)vT16 + (long long)b0 * C * lp; f.ldv = lp; f.vt_bs = (long long)C * lp; f.rsum = w.sums;
            f.split_stride = (long long)nb * S; f.row_bs = S; f.o = w.ofwd + (long long)b0 * S * C; f.ldo = C; f.o_bs = (long long)S * C; f.S = S; f.C = C; f.batch = nb;
            f.zeros = c->zeros;
            HIPCK(c, vt_launch_attn_pv(f, s), "attn fwd pv");
        }
    }
    return VT_OK;
}

}  // extern "C"
