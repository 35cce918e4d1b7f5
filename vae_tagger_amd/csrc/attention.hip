// The mid-block attention's launch schedule (host code): scratch layout, projections, Q.K^T / softmax numerators / P.V per
// group of images, output projection.
#include <math.h>

#include "vt_context.h"

namespace vt {
namespace {

// Row stride (elements) of the S x S score / probability matrices and of v^T: S rounded up to 8, plus 2112 (4 KB + 128 B) when that would
// make the row pitch a multiple of 2 KB -- 16 rows of one store instruction (or 256 rows of one tile's K-step) at a
// power-of-two pitch all fall on the same HBM channel (measured: the P write of attn_qk.hip cost as much as its MFMAs).
size_t attn_pitch(int S) {
    const size_t ld = (size_t)(S + 7) / 8 * 8;
    return (ld * 2) % 2048 == 0 ? ld + 2048 + 64 : ld;   // consecutive rows: a different 4-KB block AND a different 256-B sub-block
}
// row pitch (bytes) of the e4m3 v^T: S rounded up to 16, off the power-of-two pitches as above
size_t attn_pitch8(int S) {
    const size_t ld = (size_t)(S + 15) / 16 * 16;
    return ld % 2048 == 0 ? ld + 2048 + 64 : ld;
}
constexpr float FP8_QK_SCALE = 8.0f;       // q8 | k8 = e4m3(8 q | 8 k), v8 = e4m3(8 v): |values| up to 56 before saturation (status bit 1)
constexpr float FP8_P_SCALE_LOG2 = 8.0f;   // P8 = e4m3(256 exp(s - max)): numerators <= 256 < 448, e4m3's normal range reaches 6e-5 of the row maximum
constexpr float FP8_P_SCALE_SAMPLED_LOG2 = 5.0f;   // ... e4m3(32 exp(s - sampled max)): 2.6 nats of head room above the sampled maximum, 5e-4 below
// Probabilities (and, on the three-pass path, scores) are materialised for `group` images at a time (one batched launch
// each for Q.K^T and P.V): as many images as fit a 9.25 GiB budget (1.13 GiB per image at S = 16384), in equal launches.
int attn_group(int B, int S) {
    const size_t ld = attn_pitch(S);
    const size_t per_img = (size_t)S * ld * 4;                      // fp16 scores + bf16 probs
    size_t g = ((size_t)37 << 28) / (per_img ? per_img : 1);       // 9.25 GiB: eight images at S = 16384 with the padded pitch
    if (g < 1) g = 1;
    if (g > (size_t)B) g = (size_t)B;
    const size_t ngroups = ((size_t)B + g - 1) / g;                // equal launches rather than a small last one
    return (int)(((size_t)B + ngroups - 1) / ngroups);
}
// (row, column slot) partials per row: every tile configuration gives a wave 64 columns (the 32-column one has one slot)
size_t attn_slots_bound(int S) { return (size_t)(S + 7) / 8 * 8 / 64 + 4; }
// elements of one image's probabilities: the [S][pitch] matrix or its fragment-ordered form (attn_pv.hip), whichever is larger
size_t attn_p_elems(int S) {
    const size_t rowmajor = (size_t)S * attn_pitch(S), frag = (size_t)vt_attn_pt_elems(S);
    return rowmajor > frag ? rowmajor : frag;
}

}  // namespace

size_t attn_pitch_of(int S) { return attn_pitch(S); }
int attn_group_of(int B, int S) { return attn_group(B, S); }

size_t attn_scratch_bytes(int B, int S, int C) {
    const size_t ld = attn_pitch(S), G = (size_t)attn_group(B, S);
    return align_up((size_t)B * S * 2 * C * 2) + align_up((size_t)B * C * ld * 2) + align_up(G * S * ld * 2) +
           align_up(G * attn_p_elems(S) * 2) + align_up((size_t)B * S * C * 2) + 5 * align_up((size_t)B * S * 4) +
           align_up(G * attn_slots_bound(S) * S * 4) + align_up((size_t)B * 4) + align_up((size_t)B * S * 2 * C) +
           align_up((size_t)B * C * attn_pitch8(S)) + align_up((size_t)B * S * C) + align_up((size_t)B * C * 2 * 4);
}
AttnScratch carve_attn(char* p, int B, int S, int C) {
    const size_t ld = attn_pitch(S), G = (size_t)attn_group(B, S);
    AttnScratch a;
    a.group = (int)G;
    a.qk = (bf16_t*)p; p += align_up((size_t)B * S * 2 * C * 2);
    a.vt = (bf16_t*)p; p += align_up((size_t)B * C * ld * 2);
    a.scores = (f16_t*)p; p += align_up(G * S * ld * 2);
    a.probs = (bf16_t*)p; p += align_up(G * attn_p_elems(S) * 2);
    a.o = (bf16_t*)p; p += align_up((size_t)B * S * C * 2);
    a.qn = (float*)p; p += align_up((size_t)B * S * 4);
    a.kn = (float*)p; p += align_up((size_t)B * S * 4);
    a.sd = (float*)p; p += align_up((size_t)B * S * 4);
    a.shift = (float*)p; p += align_up((size_t)B * S * 4);
    a.rinv = (float*)p; p += align_up((size_t)B * S * 4);
    a.part = (float*)p; p += align_up(G * attn_slots_bound(S) * S * 4);
    a.flags = (int*)p; p += align_up((size_t)B * 4);
    a.qk8 = (unsigned char*)p; p += align_up((size_t)B * S * 2 * C);
    a.vt8 = (unsigned char*)p; p += align_up((size_t)B * C * attn_pitch8(S));
    a.x8 = (unsigned char*)p; p += align_up((size_t)B * S * C);
    a.ident = (float*)p;
    return a;
}

namespace {
// does the attention of this context take the e4m3 kernels (attn_fp8.hip) at this size -- and its projections too?
bool attn_is_fp8(const vt_context* c, int S, int C) {
    return c->fp8 && c->attn_fp8 && c->attn_mode != 2 && c->attn_qk_kernel && vt_attn_qk_supported(S, C) && vt_attn_fp8_supported(S, C) &&
           (size_t)vt_attn_p8_bytes(S) <= attn_p_elems(S) * 2;
}
}  // namespace
bool attn_proj_is_fp8(const vt_context* c, const AttnW& w, int S, int C) { return attn_is_fp8(c, S, C) && c->proj_fp8 && w.wqk8 && w.wv8; }

namespace {

// key-tile splits of a launch on attn_qk.hip's skeleton: enough workgroups to fill the device (512) from few query blocks
int split_for(long long qblocks, int nkt) { int n = 1; while (n < nkt && qblocks * n < 512) n *= 2; return n < nkt ? n : nkt; }
// ... and of the key sweeps whose row sums leave as segment sums: a small grid (batch 1 at 1024^2: 64 query blocks on 256 CUs)
// spreads a query block's segments over 2 or 4 workgroups of at least `min_tiles` key tiles each -- same bits either way
int sweep_nsplit(int qblocks, int ktiles, int min_tiles) { int n = qblocks > 128 ? 1 : qblocks > 64 ? 2 : 4; while (n > 1 && ktiles / n < min_tiles) n >>= 1; return n; }

// One run_attention call: sizes, the kernels it takes, and what every stage reads.
struct AttnRun {
    vt_context* c; const AttnW& w; const AttnScratch& sc; int B, S, C; hipStream_t s;
    int ld;                 // K extent of P.V (columns [S, ld) of P are zero)
    int lp;                 // row pitch of scores / P / v^T
    int ld8, kext8;         // the same for the e4m3 v^T
    bool f8, p8;            // attn_is_fp8(), attn_proj_is_fp8()
    float scale;
    int mode;               // 0: exponent shift from operand norms, exact row maximum if flagged;
                            // 1: always the exact row maximum; 2: scores -> softmax pass -> P
    bool qk_kernel() const { return c->attn_qk_kernel && vt_attn_qk_supported(S, C); }
    ConvGemmArgs gemm() const {       // a 1x1 "conv" over tokens: the generic GEMM's view of every product here
        ConvGemmArgs a{};
        a.zeros = c->zeros; a.ksize = 1; a.stride = 1; a.pad = 0; a.Hin = a.Hout = 1; a.alpha = 1.f;
        return a;
    }
};

// Stage 1: q | k and v^T from the group-normed tokens.
int attn_project(const AttnRun& r, const bf16_t* x16, bool x_e4m3) {
    vt_context* c = r.c; const AttnW& w = r.w; const AttnScratch& sc = r.sc; hipStream_t s = r.s;
    const int B = r.B, S = r.S, C = r.C, lp = r.lp;
    if (r.p8) {
        // fp8 mode: q8 | k8 = e4m3(8 (x Wqk^T + bqk)) and v8^T = e4m3(8 (Wv x^T + bv)) straight from e4m3 operands (proj_fp8_kernel): no bf16
        // q | k / v^T tensors, no conversion passes.  One scale per weight matrix (e4m3's normal range spans 2^15).
        const unsigned char* x8 = (const unsigned char*)x16;
        if (!x_e4m3) {
            std::vector<float> id((size_t)B * C * 2);
            for (size_t i = 0; i < id.size(); i += 2) { id[i] = 1.f; id[i + 1] = 0.f; }
            HIPCK(c, hipMemcpyAsync(sc.ident, id.data(), id.size() * 4, hipMemcpyHostToDevice, s), "attn tokens -> e4m3");
            HIPCK(c, hipStreamSynchronize(s), "attn tokens -> e4m3");                       // (`id` leaves scope; op-level entry only)
            HIPCK(c, vt_launch_gn_apply(x16, 0, sc.ident, sc.x8, B, S, C, 0, s, FP8_ACT_SCALE, c->status), "attn tokens -> e4m3");
            x8 = sc.x8;
        }
        ProjFp8Args pq{};
        pq.q8 = x8; pq.ldq = C; pq.q_bs = (long long)S * C; pq.nq = S;
        pq.k8 = w.wqk8; pq.ldk = C; pq.k_bs = 0; pq.nk = 2 * C;
        pq.out8 = sc.qk8; pq.ldo = 2 * C; pq.o_bs = (long long)S * 2 * C; pq.kext = 2 * C;
        pq.kbias = w.bqk; pq.alpha = w.sqk / FP8_ACT_SCALE; pq.oscale = FP8_QK_SCALE; pq.status = c->status;
        pq.C = C; pq.batch = B; pq.zeros = c->zeros;
        pq.nsplit = split_for((long long)B * ((S + 255) / 256), (2 * C + 127) / 128);
        ProjFp8Args pv{};
        pv.q8 = w.wv8; pv.ldq = C; pv.q_bs = 0; pv.nq = C;
        pv.k8 = x8; pv.ldk = C; pv.k_bs = (long long)S * C; pv.nk = S;
        pv.out8 = sc.vt8; pv.ldo = r.ld8; pv.o_bs = (long long)C * r.ld8; pv.kext = r.kext8;
        pv.qbias = w.bv; pv.alpha = w.sv / FP8_ACT_SCALE; pv.oscale = FP8_QK_SCALE; pv.status = c->status;
        pv.C = C; pv.batch = B; pv.zeros = c->zeros;
        pv.nsplit = split_for((long long)B * ((C + 255) / 256), (S + 127) / 128);
        VTCK(profiled(c, s, VT_PROF_PROJ_FP8, 2.0 * B * (double)S * 2 * C * C, "attn qk proj fp8", [&] { return vt_launch_proj_fp8(pq, s); }));
        return profiled(c, s, VT_PROF_PROJ_FP8, 2.0 * B * (double)S * C * C, "attn v proj fp8", [&] { return vt_launch_proj_fp8(pv, s); });
    }
    if (c->attn_proj_kernel && r.qk_kernel() && (lp % 8) == 0) {
        // bf16 projections on attn_qk.hip's skeleton (mode 4: rows of one operand in registers, the other's rows streamed through LDS):
        // q | k = x [Wq; Wk]^T + bqk -> [B][S][2C];  v^T = Wv x^T + bv -> [B][C][lp] (keys [S, round8(S)) zero)
        AttnQkArgs pq{};
        pq.mode = 4; pq.q = x16; pq.ldq = C; pq.qk_bs = (long long)S * C; pq.S = S; pq.C = C;
        pq.k = w.wqk; pq.ldk = C; pq.k_bs = 0; pq.nk = 2 * C; pq.kbias = w.bqk;
        pq.P = sc.qk; pq.ldp = 2 * C; pq.p_bs = (long long)S * 2 * C; pq.alpha = 1.f; pq.batch = B; pq.zeros = c->zeros; pq.row_bs = S;
        pq.nsplit = split_for((long long)B * ((S + 255) / 256), (2 * C + 63) / 64);
        AttnQkArgs pv{};
        pv.mode = 4; pv.q = w.wv; pv.ldq = C; pv.qk_bs = 0; pv.S = C; pv.C = C; pv.qbias = w.bv;
        pv.k = x16; pv.ldk = C; pv.k_bs = (long long)S * C; pv.nk = S;
        pv.P = sc.vt; pv.ldp = lp; pv.p_bs = (long long)C * lp; pv.alpha = 1.f; pv.batch = B; pv.zeros = c->zeros; pv.row_bs = C;
        pv.nsplit = split_for((long long)B * ((C + 255) / 256), (S + 63) / 64);
        VTCK(profiled(c, s, VT_PROF_PROJ_BF16, 2.0 * B * (double)S * 2 * C * C, "attn qk proj", [&] { return vt_launch_attn_qk(pq, s); }));
        return profiled(c, s, VT_PROF_PROJ_BF16, 2.0 * B * (double)S * C * C, "attn v proj", [&] { return vt_launch_attn_qk(pv, s); });
    }
    // q | k = x Wqk^T + bqk  -> [B][S][2C]
    ConvGemmArgs a = r.gemm();
    a.X = x16; a.W = w.wqk; a.bias = w.bqk; a.bias_mode = 1; a.out_bf16 = sc.qk;
    a.Win = a.Wout = S; a.Cin = C; a.Cout = 2 * C; a.Wrows = 2 * C; a.ldx = C; a.ldw = C; a.ldo = 2 * C;
    a.x_bs = (long long)S * C; a.w_bs = 0; a.o_bs = (long long)S * 2 * C; a.batch = B;
    VTCK(launch_gemm(c, a, s, "attn qk proj"));
    // v^T = Wv x^T + bv -> [B][C][ld]   (Wv rows are the "pixel" operand, tokens the "cout" operand)
    a.X = w.wv; a.W = x16; a.bias = w.bv; a.bias_mode = 2; a.out_bf16 = sc.vt;
    a.Win = a.Wout = C; a.Cin = C; a.Cout = r.ld; a.Wrows = S; a.ldx = C; a.ldw = C; a.ldo = lp;
    a.x_bs = 0; a.w_bs = (long long)S * C; a.o_bs = (long long)C * lp; a.batch = B;
    return launch_gemm(c, a, s, "attn v proj");
}

// Stage 2, fp8 mode, images [b0, b0 + nb): both contractions on e4m3 operands.  The exponent shift is the exact row maximum of the e4m3
// scores (a first sweep of the same kernel without exp / convert / store): numerators <= 1, stored as e4m3(256 x)
int attn_group_fp8(const AttnRun& r, int b0, int nb) {
    vt_context* c = r.c; const AttnScratch& sc = r.sc; hipStream_t s = r.s;
    const int S = r.S, C = r.C;
    AttnQk8Args q8{};
    q8.qk8 = sc.qk8 + (long long)b0 * S * 2 * C; q8.ldq = 2 * C; q8.qk_bs = (long long)S * 2 * C; q8.S = S; q8.C = C;
    float* shift = sc.shift + (long long)b0 * S;
    q8.P8 = (unsigned char*)sc.probs; q8.p_bs = vt_attn_p8_bytes(S); q8.rowin = shift;
    q8.row_bs = S; q8.alpha = r.scale / (FP8_QK_SCALE * FP8_QK_SCALE); q8.batch = nb; q8.zeros = c->zeros;
    const int ktiles = (S + 127) / 128;
    const int nsplit8 = sweep_nsplit(nb * ((S + 255) / 256), ktiles, 4);
    // The shift must be (close to) the row maximum: e4m3's range is too short for the bound from operand norms.  A full first
    // sweep costs 1.5 ms per step; instead the first sweep takes every kstride-th key tile -- a SAMPLED maximum m <= max -- and the
    // numerators are stored as e4m3(32 exp(s - m)): exact while the true maximum is within ln(448 / 32) = 2.6 of the sampled one
    // (thousands of keys per row: always, on the weights seen so far).  A numerator beyond 448 raises the group's flag, and the two
    // launches gated on it redo the group with the exact maximum and e4m3(256 x) -- no host round trip.  vt_set_flag(7, 1):
    // always exact.
    const int kstride = (r.mode == 1) ? 1 : ktiles >= 64 ? 8 : ktiles >= 16 ? 4 : 1;
    int* flag8 = sc.flags + b0 / sc.group;
    q8.mode = 1; q8.rowout = shift; q8.nsplit = 1; q8.kstride = kstride;
    HIPCK(c, vt_launch_attn_qk_fp8(q8, s), "attn row max fp8");
    AttnQk8Args redo = q8;
    q8.mode = 3; q8.rowout = nullptr; q8.kstride = 0; q8.nsplit = nsplit8;
    q8.pscale_log2 = kstride > 1 ? FP8_P_SCALE_SAMPLED_LOG2 : FP8_P_SCALE_LOG2;
    q8.flag = kstride > 1 ? flag8 : nullptr;
    AttnPv8Args v8{};
    v8.P8 = q8.P8; v8.p_bs = q8.p_bs; v8.vt8 = sc.vt8 + (long long)b0 * C * r.ld8; v8.ldv = r.ld8; v8.vt_bs = (long long)C * r.ld8; v8.kext = r.kext8;
    v8.o = sc.o + (long long)b0 * S * C; v8.ldo = C; v8.o_bs = (long long)S * C;
    v8.out_scale = 1.0f / FP8_QK_SCALE;                // (P8's own scale cancels against the row sums, which are sums of P8)
    v8.S = S; v8.C = C; v8.batch = nb; v8.zeros = c->zeros;
    VTCK(profiled(c, s, VT_PROF_ATTN_QK8, 2.0 * nb * (double)S * S * C, "attn exp scores fp8", [&] { return vt_launch_attn_qk_fp8(q8, s); }));
    if (kstride > 1) {                                 // both launches are no-ops unless the numerator sweep met a value beyond 448; not timed
        redo.kstride = 0; redo.gate = flag8; redo.gate_expect = 1;
        HIPCK(c, vt_launch_attn_qk_fp8(redo, s), "attn row max fp8 (exact)");
        redo.mode = 3; redo.rowout = nullptr; redo.nsplit = nsplit8; redo.pscale_log2 = FP8_P_SCALE_LOG2; redo.flag = nullptr;
        HIPCK(c, vt_launch_attn_qk_fp8(redo, s), "attn exp scores fp8 (exact)");
    }
    return profiled(c, s, VT_PROF_ATTN_PV8, 2.0 * nb * (double)S * S * C, "attn pv fp8", [&] { return vt_launch_attn_pv_fp8(v8, s); });
}

// o = P v -> bf16 [nb][S][C] on the generic GEMM, from the group's score GEMM `a` (rows of P~ scaled by 1 / row sum in the epilogue)
int attn_pv_gemm(const AttnRun& r, ConvGemmArgs a, int b0, const float* rinv) {
    const AttnScratch& sc = r.sc;
    const int S = r.S, C = r.C, lp = r.lp;
    a.X = sc.probs; a.W = sc.vt + (long long)b0 * C * lp; a.out_f16 = nullptr; a.out_bf16 = sc.o + (long long)b0 * S * C;
    a.Cin = r.ld; a.Cout = C; a.Wrows = C; a.ldx = lp; a.ldw = lp; a.ldo = C; a.alpha = 1.f;
    a.x_bs = (long long)S * lp; a.w_bs = (long long)C * lp; a.o_bs = (long long)S * C;
    a.row_part = nullptr; a.gate = nullptr;
    if (r.mode == 2) { a.row_mode = 0; a.row_in = nullptr; } else { a.row_mode = 3; a.row_in = rinv; }
    a.x_stream = r.c->pv_stream;
    return launch_gemm(r.c, a, r.s, "attn pv");
}

// Stage 2 for images [b0, b0 + nb): scores, softmax numerators P~ and their row sums, o = P v
int attn_group_scores_pv(const AttnRun& r, int b0, int nb) {
    vt_context* c = r.c; const AttnScratch& sc = r.sc; hipStream_t s = r.s;
    const int S = r.S, C = r.C, lp = r.lp, mode = r.mode;
    const bf16_t* q = sc.qk + (long long)b0 * S * 2 * C;
    float* shift = sc.shift + (long long)b0 * S;
    float* rinv = sc.rinv + (long long)b0 * S;
    const int* gate = mode == 0 ? sc.flags + b0 / sc.group : nullptr;
    // s = q k^T / sqrt(C), [nb][S][ld]
    ConvGemmArgs a = r.gemm();
    a.X = q; a.W = q + C;
    a.Win = a.Wout = S; a.Cin = C; a.Cout = r.ld; a.Wrows = S; a.ldx = 2 * C; a.ldw = 2 * C; a.ldo = lp;
    a.x_bs = a.w_bs = (long long)S * 2 * C; a.o_bs = (long long)S * lp; a.batch = nb; a.alpha = r.scale;
    a.row_bs = S;
    if (mode == 2) {
        // fp16 scores (|s| is O(1): fp16's 2^-11 is far below the bf16 rounding of P), one softmax pass over them
        a.out_f16 = sc.scores;
        VTCK(launch_gemm(c, a, s, "attn scores"));
        HIPCK(c, vt_launch_softmax_rows(sc.scores, 1, sc.probs, (long long)nb * S, S, lp, lp, s), "attn softmax");
        return attn_pv_gemm(r, a, b0, rinv);
    }
    if (!r.qk_kernel()) {
        a.short_tiles = c->gemm_short;
        const int slots = vt_conv_gemm_col_slots(a);
        if ((size_t)slots > attn_slots_bound(S)) return c->fail(VT_ERR_WORKSPACE, "attention: %d column slots exceed the scratch", slots);
        // exact row maxima (always in mode 1; in mode 0 only when the operand-norm bound was too loose for this group)
        a.row_mode = 1; a.row_part = sc.part; a.gate = gate; a.gate_expect = 1;
        VTCK(launch_gemm(c, a, s, "attn row max"));
        HIPCK(c, vt_launch_attn_row_reduce(sc.part, slots, S, S, nb, 0, shift, gate, 1, s), "attn row max reduce");
        // P~ = exp(s - shift) as bf16 + the row sums of what was stored
        a.row_mode = 2; a.row_in = shift; a.out_bf16 = sc.probs; a.gate = nullptr;
        VTCK(launch_gemm(c, a, s, "attn exp scores"));
        HIPCK(c, vt_launch_attn_row_reduce(sc.part, slots, S, S, nb, 1, rinv, nullptr, 0, s), "attn row sums");
        return attn_pv_gemm(r, a, b0, rinv);
    }
    if (r.f8) return attn_group_fp8(r, b0, nb);
    // the dedicated kernel (attn_qk.hip): Q rows resident in registers, keys streamed, a wave owns whole rows ->
    // row maxima / sums accumulate in registers, no partial buffers
    AttnQkArgs k{};
    k.q = q; k.k = q + C; k.S = S; k.C = C; k.ldq = 2 * C; k.qk_bs = (long long)S * 2 * C;
    k.row_bs = S; k.alpha = r.scale; k.batch = nb; k.zeros = c->zeros;
    k.mode = 1; k.rowout = shift; k.gate = gate; k.gate_expect = 1;
    HIPCK(c, vt_launch_attn_qk(k, s), "attn row max");
    k.mode = 2; k.P = sc.probs; k.ldp = lp; k.p_bs = (long long)S * lp; k.rowin = shift; k.rowout = rinv; k.gate = nullptr;
    const bool frag_pv = c->attn_pv_kernel && vt_attn_pv_supported(S, C);      // P written in fragment order and consumed by attn_pv.hip
    if (frag_pv) {
        // row sums leave as four segment sums in the partials scratch (attn_qk.hip)
        if ((size_t)4 * nb * S > sc.group * attn_slots_bound(S) * (size_t)S) return c->fail(VT_ERR_WORKSPACE, "attention: segment sums exceed the scratch");
        k.p_frag = 1; k.p_bs = vt_attn_pt_elems(S);
        k.rowout = sc.part; k.split_stride = (long long)nb * S;
        k.nsplit = sweep_nsplit(nb * ((S + 255) / 256), (S + 63) / 64, 8);
    }
    VTCK(profiled(c, s, VT_PROF_ATTN_QK, 2.0 * nb * (double)S * S * C, "attn exp scores", [&] { return vt_launch_attn_qk(k, s); }));
    if (!frag_pv) return attn_pv_gemm(r, a, b0, rinv);
    if (sc.save_sums)      // the training forward keeps the segment sums of every image: [4][B][S], this group's columns
        HIPCK(c, hipMemcpy2DAsync(sc.save_sums + (long long)b0 * S, (size_t)r.B * S * 4, sc.part, (size_t)nb * S * 4, (size_t)nb * S * 4, 4, hipMemcpyDeviceToDevice, s),
              "attn segment sums");
    AttnPvArgs v{};
    v.Pt = sc.probs; v.pt_bs = vt_attn_pt_elems(S); v.vt = sc.vt + (long long)b0 * C * lp; v.ldv = lp; v.vt_bs = (long long)C * lp;
    v.rsum = sc.part; v.split_stride = (long long)nb * S; v.row_bs = S; v.o = sc.o + (long long)b0 * S * C; v.ldo = C; v.o_bs = (long long)S * C;
    v.S = S; v.C = C; v.batch = nb; v.zeros = c->zeros;
    return profiled(c, s, VT_PROF_ATTN_PV, 2.0 * nb * (double)S * S * C, "attn pv", [&] { return vt_launch_attn_pv(v, s); });
}

// Stage 3: out = o Wo^T + bo + residual, with the GroupNorm partials of the result when the next norm can take them
int attn_out_proj(const AttnRun& r, const void* res, void* out, GnState* gn, int groups, int rdt) {
    vt_context* c = r.c; const AttnW& w = r.w; const AttnScratch& sc = r.sc; hipStream_t s = r.s;
    const int B = r.B, S = r.S, C = r.C;
    if (gn) gn->parts = 0;
    if (c->attn_proj_kernel && r.qk_kernel() && (C % 16) == 0) {
        // on attn_qk.hip's skeleton (mode 5): rows = tokens o, keys = Wo (shared by the batch), the residual stream added and
        // stored as fp16 / fp32 in the epilogue, GroupNorm partials of the result per (32-token slab, 16-channel group) for the norm that follows
        AttnQkArgs po{};
        po.mode = 5; po.q = sc.o; po.ldq = C; po.qk_bs = (long long)S * C; po.S = S; po.C = C;
        po.k = w.wo; po.ldk = C; po.k_bs = 0; po.nk = C; po.kbias = w.bo;
        po.ldp = C; po.p_bs = (long long)S * C; po.alpha = 1.f; po.batch = B; po.zeros = c->zeros; po.row_bs = S;
        if (rdt == 1) { po.res_f32 = (const float*)res; po.out_f32 = (float*)out; } else { po.res_f16 = (const f16_t*)res; po.out_f16 = (f16_t*)out; }
        if (gn && c->fuse_gn_stats && C / groups == 16) { po.gn_partial = gn->partial; po.gn_parts = vt_attn_linear_parts(S); gn->parts = po.gn_parts; }
        po.nsplit = split_for((long long)B * ((S + 255) / 256), (C + 63) / 64);
        return profiled(c, s, VT_PROF_PROJ_BF16, 2.0 * B * (double)S * C * C, "attn out proj", [&] { return vt_launch_attn_qk(po, s); });
    }
    // -> fp32 [B][S][C] on the generic GEMM
    ConvGemmArgs a = r.gemm();
    a.X = sc.o; a.W = w.wo; a.bias = w.bo; a.bias_mode = 1;
    if (rdt == 1) { a.res = (const float*)res; a.out_f32 = (float*)out; } else { a.res_f16 = (const f16_t*)res; a.out_f16 = (f16_t*)out; }
    a.Win = a.Wout = S; a.Cin = C; a.Cout = C; a.Wrows = C; a.ldx = C; a.ldw = C; a.ldo = C; a.ldr = C;
    a.x_bs = (long long)S * C; a.w_bs = 0; a.o_bs = a.x_bs; a.r_bs = a.x_bs; a.batch = B;
    const int cpg = C / groups;
    if (gn && c->fuse_gn_stats && (cpg == 4 || cpg == 8 || cpg == 16) && C > 32 && (C % (C <= 128 ? 128 : 256)) == 0) {
        a.short_tiles = c->gemm_short;
        a.gn_partial = gn->partial; a.gn_cpg = cpg; gn->parts = vt_conv_gemm_ptiles_of(a);
    }
    return launch_gemm(c, a, s, "attn out proj");
}

}  // namespace

int attn_sweep_nsplit(int qblocks, int ktiles, int min_tiles) { return sweep_nsplit(qblocks, ktiles, min_tiles); }

// diffusers Attention for the VAE mid block: 1 head, dim_head = C, scale 1/sqrt(C).
// x16: group-normed tokens [B][S][C] bf16.  out = to_out(softmax(q k^T / sqrt(C)) v) + residual.
// `x_e4m3`: x16 holds the tokens as e4m3(8 x) bytes ([B][S][C], one byte each) -- what the encoder's GroupNorm pass writes when
// attn_proj_is_fp8(); with bf16 tokens on that path (the op-level entry) they are converted here first.
int run_attention(vt_context* c, const AttnW& w, const bf16_t* x16, const void* res, void* out, int B, int S,
                  const AttnScratch& sc, hipStream_t s, GnState* gn, int groups, int rdt, bool x_e4m3) {
    const int C = w.c;
    const AttnRun r{c, w, sc, B, S, C, s, (S + 7) / 8 * 8, (int)attn_pitch(S), (int)attn_pitch8(S), (S + 15) / 16 * 16,
                    attn_is_fp8(c, S, C), attn_proj_is_fp8(c, w, S, C), 1.0f / sqrtf((float)C), c->attn_mode};
    if (x_e4m3 && !r.p8) return c->fail(VT_ERR_STATE, "internal: e4m3 tokens for a bf16 projection");
    VTCK(attn_project(r, x16, x_e4m3));
    if (r.f8) {
        HIPCK(c, hipMemsetAsync(sc.flags, 0, (size_t)((B + sc.group - 1) / sc.group) * 4, s), "attn flags");
        // (bf16 projections: q8 | k8 come out of the row-norms pass; the norms themselves are not used: the fp8 path takes a sampled / the exact row maximum)
        if (!r.p8) HIPCK(c, vt_launch_attn_row_norms_fp8(sc.qk, (long long)B * S, C, FP8_QK_SCALE, sc.qk8, sc.qn, sc.kn, sc.sd, c->status, s), "attn q|k -> e4m3");
    } else if (r.mode == 0) {
        HIPCK(c, hipMemsetAsync(sc.flags, 0, (size_t)((B + sc.group - 1) / sc.group) * 4, s), "attn flags");
        HIPCK(c, vt_launch_attn_row_norms(sc.qk, (long long)B * S, C, sc.qn, sc.kn, sc.sd, s), "attn row norms");
        HIPCK(c, vt_launch_attn_shift(sc.qn, sc.kn, sc.sd, B, S, r.scale, 120.f, sc.shift, sc.flags, sc.group, s), "attn shift");
    }
    if (r.f8 && !r.p8) HIPCK(c, vt_launch_attn_vt_to_fp8(sc.vt, (long long)C * r.lp, r.lp, sc.vt8, (long long)C * r.ld8, r.ld8, S, r.kext8, C, B, FP8_QK_SCALE, c->status, s), "attn v^T fp8");
    for (int b0 = 0; b0 < B; b0 += sc.group) VTCK(attn_group_scores_pv(r, b0, B - b0 < sc.group ? B - b0 : sc.group));
    return attn_out_proj(r, res, out, gn, groups, rdt);
}

}  // namespace vt

using namespace vt;

extern "C" {

size_t vt_op_attention_workspace_bytes(int B, int S, int C) {
    if (B <= 0 || S <= 0 || C <= 0) return 0;
    return attn_scratch_bytes(B, S, C) + ALIGN;
}

int vt_op_attention(vt_context* c, const void* x16, const float* res, float* out, int B, int S, int C, void* ws, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (!c->enc.finalized) return c->fail(VT_ERR_STATE, "encoder weights not finalized");
    if (C != c->enc.attn.c) return c->fail(VT_ERR_INVALID, "vt_op_attention: C = %d but the mid-block attention has %d channels", C, c->enc.attn.c);
    if (!x16 || !out || !ws || ((uintptr_t)ws % ALIGN)) return c->fail(VT_ERR_INVALID, "vt_op_attention: bad buffer");
    return run_attention(c, c->enc.attn, (const bf16_t*)x16, res, out, B, S, carve_attn((char*)ws, B, S, C), (hipStream_t)stream);
}

}  // extern "C"
