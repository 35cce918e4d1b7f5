// Weight packing (host code): number conversions, the operand layouts of every conv / attention kernel, vt_encoder_finalize and
// vt_image_decoder_finalize over the same per-layer packers (pack_conv, get_resnet, get_mid_block).
#include <math.h>

#include <algorithm>
#include <string.h>

#include "vt_context.h"

namespace vt {

static uint16_t f2bf(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // keep NaN a NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
float bf2f(uint16_t h) { uint32_t u = (uint32_t)h << 16; float f; memcpy(&f, &u, 4); return f; }
// float -> IEEE fp16 bits, round to nearest even (the compiler's own conversion: _Float16 is a host type too)
static uint16_t f2h(float f) { const _Float16 h = (_Float16)f; uint16_t u; memcpy(&u, &h, 2); return u; }
float h2f(uint16_t h) {
    const uint32_t s = (h >> 15) & 1, e = (h >> 10) & 31, m = h & 1023;
    uint32_t u;
    if (e == 0) {
        if (m == 0) u = s << 31;
        else { int sh = 0; uint32_t mm = m; while (!(mm & 1024)) { mm <<= 1; ++sh; } u = (s << 31) | ((uint32_t)(113 - sh) << 23) | ((mm & 1023) << 13); }
    } else if (e == 31) u = (s << 31) | 0x7f800000u | (m << 13);
    else u = (s << 31) | ((e + 112) << 23) | (m << 13);
    float f; memcpy(&f, &u, 4); return f;
}

// float -> OCP e4m3fn (1-4-3, bias 7, max 448, no infinities), round to nearest even, saturating
static uint8_t f2e4m3(float f) {
    if (f != f) return 0x7f;
    const uint8_t sgn = signbit(f) ? 0x80 : 0x00;
    const float a = fabsf(f);
    if (a >= 448.f) return sgn | 0x7e;
    if (a < 0.015625f) return sgn | (uint8_t)nearbyintf(a * 512.f);       // subnormals: multiples of 2^-9 (8 -> the smallest normal)
    int e;
    const float m = frexpf(a, &e);                                          // a = m 2^e, m in [0.5, 1)
    int M = (int)nearbyintf((2.f * m - 1.f) * 8.f), E = e - 1;
    if (M == 8) { M = 0; ++E; }
    const int biased = E + 7;
    if (biased > 15 || (biased == 15 && M > 6)) return sgn | 0x7e;
    return sgn | (uint8_t)((biased << 3) | M);
}
// the e4m3 scale of n values: the largest magnitude lands on 448
static float e4m3_scale(const float* v, size_t n) {
    float amax = 0.f;
    for (size_t i = 0; i < n; ++i) amax = fmaxf(amax, fabsf(v[i]));
    return amax > 0.f ? amax / 448.f : 1.f;
}

// The operand layouts.  Every halo-type kernel reads its weights as one contiguous [cout rows][chunk] tile per K-step:
//   dst[((cin / chunk) * taps + step(tap)) * cout + row(o)) * chunk + cin % chunk] = cvt(w_oihw[o][cin][tap], o)
// with chunk 32 (16-bit operands) or 64 (e4m3), `step` the kernel's K-step order and `row` its cout interleave.
template <class T, class Step, class Row, class Cvt>
static std::vector<T> permute_weights(const float* w_oihw, int cout, int cin, int taps, int chunk, Step step, Row row, Cvt cvt) {
    std::vector<T> dst((size_t)cout * taps * cin, 0);
    for (int o = 0; o < cout; ++o) {
        const int r = row(o);
        for (int i = 0; i < cin; ++i)
            for (int t = 0; t < taps; ++t)
                dst[(((size_t)(i / chunk) * taps + step(t)) * cout + r) * chunk + i % chunk] = cvt(w_oihw[((size_t)o * cin + i) * taps + t], o);
    }
    return dst;
}
// ... and the generic GEMM's: [cout][ky*k+kx][cin] (k-contiguous MFMA operand rows)
template <class T, class Cvt>
static std::vector<T> pack_ohwi(const float* w_oihw, int cout, int cin, int taps, Cvt cvt) {
    std::vector<T> dst((size_t)cout * taps * cin);
    for (int o = 0; o < cout; ++o)
        for (int i = 0; i < cin; ++i)
            for (int t = 0; t < taps; ++t)
                dst[((size_t)o * taps + t) * cin + i] = cvt(w_oihw[((size_t)o * cin + i) * taps + t], o);
    return dst;
}
static int same(int v) { return v; }
static int row64(int o) { return (o & ~63) + vt_halo_row_of_cout(o & 63); }         // the 16-bit halo kernels' cout interleave
static int row32(int o) { return (o & ~31) + vt_halo_fp8_row_of_cout(o & 31); }     // the e4m3 halo kernels'
static int step_halo(int t) { return vt_halo_step_of_tap(t); }                      // step = kx*3 + ky
static int step_s2(int t) { return vt_s2_step_of_tap(t); }                          // steps in plane order
static uint16_t to_bf16(float f, int) { return f2bf(f); }
static uint16_t to_f16(float f, int) { return f2h(f); }

ConvE4m3 pack_conv_e4m3(const float* w_oihw, int cout, int cin, bool s2_layout) {
    ConvE4m3 p;
    std::vector<float> scale(cout), scale_g(cout);
    p.mult8.resize(cout); p.mult8g.resize(cout);
    for (int o = 0; o < cout; ++o) {
        scale[o] = e4m3_scale(w_oihw + (size_t)o * cin * 9, (size_t)cin * 9);
        p.mult8[o] = scale[o] / FP8_ACT_SCALE;
        scale_g[o] = p.mult8[o] * FP8_ACT_SCALE;        // (the GEMM and stride-2 forms have always divided by this product, not by scale[o] itself)
        p.mult8g[o] = scale_g[o] / FP8_RES_SCALE;       // their input carries FP8_RES_SCALE
    }
    // conv3x3_halo_fp8.hip: Wp8[cin/64][step (kx-major)][cout row][64]
    p.wp8 = permute_weights<uint8_t>(w_oihw, cout, cin, 9, 64, step_halo, row32, [&](float f, int o) { return f2e4m3(f / scale[o]); });
    const auto cvt_g = [&](float f, int o) { return f2e4m3(f / scale_g[o]); };
    p.w8g = pack_ohwi<uint8_t>(w_oihw, cout, cin, 9, cvt_g);
    // conv3x3_s2_halo_fp8.hip: Wp[cin/64][step (vt_s2_step_of_tap)][cout row][64]
    if (s2_layout) p.wp8s2 = permute_weights<uint8_t>(w_oihw, cout, cin, 9, 64, step_s2, row32, cvt_g);
    return p;
}

template <class T, class V>
static bool up(vt_context* c, const T** dst, const std::vector<V>& v) { return (*dst = (const T*)c->upload(v.data(), v.size() * sizeof(V))) != nullptr; }

// Every packing of one conv from its fp32 OIHW weight `wv` and bias `bv` (cout floats); `name` is for messages only.
// `mult8_host`: receives the fp8 halo kernel's per-cout multipliers (empty when the conv has no fp8 form)
int pack_conv(vt_context* c, const std::string& name, const float* wv, const float* bv, int cout, int cin, int k, ConvW* out, bool stride2,
              std::vector<float>* mult8_host) {
    const auto failed = [&] { return c->fail(VT_ERR_HIP, "upload failed for %s", name.c_str()); };
    out->cin = cin; out->cout = cout; out->k = k;
    if (!up(c, &out->w, pack_ohwi<uint16_t>(wv, cout, cin, k * k, to_bf16)) || !(out->b = (const float*)c->upload(bv, (size_t)cout * 4))) return failed();
    // halo kernel: Wp[cin/32][step][cout][32] (step = kx*3 + ky) so each K-step's weight tile is one contiguous block
    if (k == 3 && vt_conv3x3_halo_supported(cin, cout) && !up(c, &out->wp, permute_weights<uint16_t>(wv, cout, cin, 9, 32, step_halo, row64, to_bf16))) return failed();
    // stride-2 kernel: Wp2[cin/32][step][cout row][32], steps in plane order (vt_s2_step_of_tap)
    if (k == 3 && stride2 && vt_conv3x3_s2_supported(cin, cout) && !up(c, &out->wp2, permute_weights<uint16_t>(wv, cout, cin, 9, 32, step_s2, row64, to_bf16))) return failed();
    // fp16-operand mode (vt_set_flag 18): the same layouts with fp16 bits -- 11 significand bits of every weight instead of 8
    if (k == 3 && cout <= 32 && !up(c, &out->w16, pack_ohwi<uint16_t>(wv, cout, cin, 9, to_f16))) return failed();
    if (k == 3 && vt_conv_out_halo_supported(cin, cout)) {
        // conv_out's own halo tile: [cin/32][tap = ky * 3 + kx][cout][32], both operand types
        if (!up(c, &out->wpo, permute_weights<uint16_t>(wv, cout, cin, 9, 32, same, same, to_bf16)) ||
            !up(c, &out->wpo16, permute_weights<uint16_t>(wv, cout, cin, 9, 32, same, same, to_f16))) return failed();
    }
    if (out->wp && !up(c, &out->wp16, permute_weights<uint16_t>(wv, cout, cin, 9, 32, step_halo, row64, to_f16))) return failed();
    if (out->wp2 && !up(c, &out->wp2_16, permute_weights<uint16_t>(wv, cout, cin, 9, 32, step_s2, row64, to_f16))) return failed();
    if (k == 3 && c->pack_fp8 && vt_conv3x3_halo_fp8_supported(cin, cout)) {
        const ConvE4m3 p = pack_conv_e4m3(wv, cout, cin, stride2 && vt_conv3x3_s2_fp8_supported(cin, cout));
        if (!up(c, &out->wp8, p.wp8) || !up(c, &out->mult8, p.mult8) || !up(c, &out->w8g, p.w8g) || !up(c, &out->mult8g, p.mult8g)) return failed();
        if (!p.wp8s2.empty() && !up(c, &out->wp8s2, p.wp8s2)) return failed();
        if (mult8_host) *mult8_host = p.mult8;
    }
    return VT_OK;
}
// conv_shortcut for conv2's launch (declared in vt_context.h): the packing both the finalizers and vt_op_conv3x3_block read
int pack_fused_shortcut(vt_context* c, const std::string& name, const float* w_oi, const float* bias_sum, int cout, int cin, const bf16_t** wp,
                        const float** bias, const bf16_t** wp16) {
    if (!up(c, wp, permute_weights<uint16_t>(w_oi, cout, cin, 1, 32, same, row64, to_bf16)) || !(*bias = (const float*)c->upload(bias_sum, (size_t)cout * 4)) ||
        !up(c, wp16, permute_weights<uint16_t>(w_oi, cout, cin, 1, 32, same, row64, to_f16)))
        return c->fail(VT_ERR_HIP, "upload failed for %s", name.c_str());
    return VT_OK;
}
// ... of the conv whose tensors the caller set as `name`.weight / .bias
static int get_conv(vt_context* c, const std::string& name, int cout, int cin, int k, ConvW* out, bool stride2 = false, std::vector<float>* mult8_host = nullptr) {
    const HostTensor* w = c->find(name + ".weight");
    const HostTensor* b = c->find(name + ".bias");
    if (!w || !b) return c->fail(VT_ERR_MISSING_WEIGHT, "missing weight %s.{weight,bias}", name.c_str());
    if (w->shape.size() != 4 || w->shape[0] != cout || w->shape[1] != cin || w->shape[2] != k || w->shape[3] != k || b->numel() != cout)
        return c->fail(VT_ERR_INVALID, "shape mismatch for %s", name.c_str());
    return pack_conv(c, name, w->v.data(), b->v.data(), cout, cin, k, out, stride2, mult8_host);
}
static int get_norm(vt_context* c, const std::string& name, int ch, NormW* out) {
    const HostTensor* g = c->find(name + ".weight");
    const HostTensor* b = c->find(name + ".bias");
    if (!g || !b) return c->fail(VT_ERR_MISSING_WEIGHT, "missing weight %s.{weight,bias}", name.c_str());
    if (g->numel() != ch || b->numel() != ch) return c->fail(VT_ERR_INVALID, "shape mismatch for %s", name.c_str());
    out->g = (const float*)c->upload(g->v.data(), ch * 4);
    out->b = (const float*)c->upload(b->v.data(), ch * 4);
    out->c = ch;
    if (!out->g || !out->b) return c->fail(VT_ERR_HIP, "upload failed for %s", name.c_str());
    return VT_OK;
}
static int get_resnet(vt_context* c, const std::string& p, int cin, int cout, ResnetW* r) {
    r->cin = cin; r->cout = cout;
    std::vector<float> mult2;                       // conv2's fp8 multipliers
    VTCK(get_norm(c, p + ".norm1", cin, &r->n1));
    VTCK(get_conv(c, p + ".conv1", cout, cin, 3, &r->c1));
    VTCK(get_norm(c, p + ".norm2", cout, &r->n2));
    VTCK(get_conv(c, p + ".conv2", cout, cout, 3, &r->c2, false, &mult2));
    r->has_sc = cin != cout;
    if (r->has_sc) VTCK(get_conv(c, p + ".conv_shortcut", cout, cin, 1, &r->sc));
    if (r->has_sc && r->c2.wp && (cin % 32) == 0) {
        const float* w = c->find(p + ".conv_shortcut.weight")->v.data();
        const HostTensor* bs = c->find(p + ".conv_shortcut.bias");
        const HostTensor* b2 = c->find(p + ".conv2.bias");
        std::vector<float> bb(cout);
        for (int o = 0; o < cout; ++o) bb[o] = b2->v[o] + bs->v[o];
        VTCK(pack_fused_shortcut(c, p + ".conv_shortcut", w, bb.data(), cout, cin, &r->sc_wp, &r->b_c2sc, &r->sc_wp16));
        // fp8 conv2: its epilogue multiplies the accumulator by mult[cout] = scale / 8, so the shortcut rows carry 1 / mult
        if (r->c2.wp8 && !up(c, &r->sc_wp8, permute_weights<uint16_t>(w, cout, cin, 1, 32, same, row32, [&](float f, int o) { return f2bf(f / mult2[o]); })))
            return c->fail(VT_ERR_HIP, "upload failed for %s.conv_shortcut", p.c_str());
    }
    return VT_OK;
}
static int get_linear_bf16(vt_context* c, const std::string& name, int out, int in, std::vector<uint16_t>* w, std::vector<float>* b) {
    const HostTensor* wt = c->find(name + ".weight");
    const HostTensor* bt = c->find(name + ".bias");
    if (!wt || !bt) return c->fail(VT_ERR_MISSING_WEIGHT, "missing weight %s.{weight,bias}", name.c_str());
    if (wt->numel() != (int64_t)out * in || bt->numel() != out) return c->fail(VT_ERR_INVALID, "shape mismatch for %s", name.c_str());
    for (float f : wt->v) w->push_back(f2bf(f));
    for (float f : bt->v) b->push_back(f);
    return VT_OK;
}

std::vector<float> pack_conv_in(const float* w_o27, int cout) {
    std::vector<float> p((size_t)27 * cout);
    for (int o = 0; o < cout; ++o) for (int k = 0; k < 27; ++k) p[(size_t)k * cout + o] = w_o27[(size_t)o * 27 + k];
    return p;
}

// conv_in_mfma_kernel's weights: [2 (hi, lo)][128 rows][32 k] bf16, rows in the interleaved cout order; w = hi + lo to ~2^-17;
// the bias rides in k = 27..29 of the hi rows as three bf16 pieces (the kernel's operand is 1.0 there).
std::vector<uint16_t> pack_conv_in_mfma(const float* w_o27, const float* bias) {
    std::vector<uint16_t> pk((size_t)2 * 128 * 32, 0);
    for (int o = 0; o < 128; ++o) {
        const int row = row64(o);
        for (int k = 0; k < 27; ++k) {
            const float f = w_o27[(size_t)o * 27 + k];
            const uint16_t hi = f2bf(f);
            pk[(size_t)row * 32 + k] = hi;
            pk[(size_t)(128 + row) * 32 + k] = f2bf(f - bf2f(hi));
        }
        float rest = bias[o];
        for (int k = 27; k < 30; ++k) {
            const uint16_t piece = f2bf(rest);
            pk[(size_t)row * 32 + k] = piece;
            rest -= bf2f(piece);
        }
    }
    return pk;
}

static int get_conv_in(vt_context* c, EncoderW& e) {
    const int c0 = e.block_out[0];
    const HostTensor* w = c->find("encoder.conv_in.weight");
    const HostTensor* b = c->find("encoder.conv_in.bias");
    if (!w || !b) return c->fail(VT_ERR_MISSING_WEIGHT, "missing weight encoder.conv_in.{weight,bias}");
    if (w->numel() != (int64_t)c0 * 27 || b->numel() != c0) return c->fail(VT_ERR_INVALID, "shape mismatch for encoder.conv_in");
    if (!up(c, &e.conv_in_w, pack_conv_in(w->v.data(), c0)) || !up(c, &e.conv_in_b, b->v)) return c->fail(VT_ERR_HIP, "upload failed for conv_in");
    if (c0 == 128 && e.groups == 32 && !up(c, &e.conv_in_wpk, pack_conv_in_mfma(w->v.data(), b->v.data()))) return c->fail(VT_ERR_HIP, "upload failed for conv_in");
    return VT_OK;
}

static int get_attention(vt_context* c, const std::string& a, int C, AttnW* at) {
    VTCK(get_norm(c, a + ".group_norm", C, &at->gn));
    std::vector<uint16_t> wqk, wv, wo; std::vector<float> bqk, bv, bo;
    VTCK(get_linear_bf16(c, a + ".to_q", C, C, &wqk, &bqk));
    VTCK(get_linear_bf16(c, a + ".to_k", C, C, &wqk, &bqk));
    VTCK(get_linear_bf16(c, a + ".to_v", C, C, &wv, &bv));
    VTCK(get_linear_bf16(c, a + ".to_out.0", C, C, &wo, &bo));
    at->c = C;
    // fp8 mode's projections: e4m3 of the bf16-rounded matrix over one scale
    auto pack8 = [&](const std::vector<uint16_t>& w, float* scale) {
        std::vector<float> f(w.size());
        for (size_t i = 0; i < w.size(); ++i) f[i] = bf2f(w[i]);
        *scale = e4m3_scale(f.data(), f.size());
        std::vector<uint8_t> o(w.size());
        for (size_t i = 0; i < w.size(); ++i) o[i] = f2e4m3(f[i] / *scale);
        return o;
    };
    const bool ok = up(c, &at->wqk, wqk) && up(c, &at->wv, wv) && up(c, &at->wo, wo) && up(c, &at->bqk, bqk) && up(c, &at->bv, bv) && up(c, &at->bo, bo) &&
                    up(c, &at->wqk8, pack8(wqk, &at->sqk)) && up(c, &at->wv8, pack8(wv, &at->sv));
    return ok ? VT_OK : c->fail(VT_ERR_HIP, "upload failed for attention");
}

// `prefix`.mid_block: resnet, attention, resnet.  The packing order decides only the order of the model's allocation list, and each model
// keeps the one it had: the encoder packs the attention after both resnets, the image decoder between them.
static int get_mid_block(vt_context* c, const std::string& prefix, int C, bool attn_last, ResnetW* mid0, AttnW* attn, ResnetW* mid1) {
    VTCK(get_resnet(c, prefix + ".mid_block.resnets.0", C, C, mid0));
    if (!attn_last) VTCK(get_attention(c, prefix + ".mid_block.attentions.0", C, attn));
    VTCK(get_resnet(c, prefix + ".mid_block.resnets.1", C, C, mid1));
    if (attn_last) VTCK(get_attention(c, prefix + ".mid_block.attentions.0", C, attn));
    return VT_OK;
}

// the host copies of a finalized model's tensors are no longer needed: erase every key that starts with `prefix`
static void erase_host_tensors(vt_context* c, const std::string& prefix) {
    for (auto it = c->weights.begin(); it != c->weights.end();)
        it = (it->first.compare(0, prefix.size(), prefix) == 0) ? c->weights.erase(it) : ++it;
}

}  // namespace vt

using namespace vt;

extern "C" int vt_encoder_finalize(vt_context* c) {
    if (!c) return VT_ERR_INVALID;
    EncoderW& e = c->enc;
    if (!e.configured) return c->fail(VT_ERR_STATE, "vt_encoder_configure was not called");
    DeviceGuard guard(c);
    // a second finalize frees the packed weights of the first: until THIS one succeeds the context is "not finalized" and no
    // weight pointer of the previous packing survives (a failed re-finalize must not leave vt_encode reading freed memory)
    e.finalized = false;
    e.conv_in_wpk = nullptr; e.conv_in_w = nullptr; e.conv_in_b = nullptr;
    e.stages.clear(); e.mid0 = ResnetW(); e.mid1 = ResnetW(); e.attn = AttnW(); e.norm_out = NormW(); e.conv_out = ConvW();
    c->free_allocs(c->enc_allocs);
    c->cur_allocs = &c->enc_allocs;
    VTCK(get_conv_in(c, e));
    int ci = e.block_out[0];
    for (size_t i = 0; i < e.block_out.size(); ++i) {
        StageW st;
        const int co = e.block_out[i];
        for (int j = 0; j < e.layers; ++j) {
            ResnetW rw;
            char nm[128]; snprintf(nm, sizeof nm, "encoder.down_blocks.%zu.resnets.%d", i, j);
            VTCK(get_resnet(c, nm, ci, co, &rw));
            st.res.push_back(rw);
            ci = co;
        }
        if (i + 1 < e.block_out.size()) {
            char nm[128]; snprintf(nm, sizeof nm, "encoder.down_blocks.%zu.downsamplers.0.conv", i);
            VTCK(get_conv(c, nm, co, co, 3, &st.down, true));
            st.has_down = true;
        }
        e.stages.push_back(st);
    }
    const int C = e.block_out.back();
    VTCK(get_mid_block(c, "encoder", C, true, &e.mid0, &e.attn, &e.mid1));
    VTCK(get_norm(c, "encoder.conv_norm_out", C, &e.norm_out));
    VTCK(get_conv(c, "encoder.conv_out", 2 * e.latent, C, 3, &e.conv_out));
    erase_host_tensors(c, "encoder.");
    e.finalized = true;
    return VT_OK;
}

// ---- the VAE's image decoder ----------------------------------------------------------------------
// upsamplers.0.conv: the ordinary packings (the literal route) and, where conv3x3_up2.hip takes the shape, the folded one -- packed on the
// device from the fp32 OIHW tensor into a bf16 and an fp16 copy
static int get_upsample_conv(vt_context* c, const std::string& name, int ch, UpBlockW* u) {
    VTCK(get_conv(c, name, ch, ch, 3, &u->up));
    if (!vt_conv3x3_up2_supported(ch, ch)) return VT_OK;
    const HostTensor* w = c->find(name + ".weight");
    const size_t n = (size_t)ch * ch * 9, nf = (size_t)ch * ch * 16;
    float* tmp = nullptr;
    void *p16 = nullptr, *ph = nullptr;
    if (hipMalloc(&p16, nf * 2) != hipSuccess) return c->fail(VT_ERR_HIP, "upload failed for %s", name.c_str());
    c->cur_allocs->push_back(p16);
    if (hipMalloc(&ph, nf * 2) != hipSuccess) return c->fail(VT_ERR_HIP, "upload failed for %s", name.c_str());
    c->cur_allocs->push_back(ph);
    if (hipMalloc((void**)&tmp, n * 4) != hipSuccess) return c->fail(VT_ERR_HIP, "upload failed for %s", name.c_str());
    hipError_t e = hipMemcpy(tmp, w->v.data(), n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = vt_launch_pack_up2(tmp, (bf16_t*)p16, (f16_t*)ph, ch, ch, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    (void)hipFree(tmp);
    if (e != hipSuccess) return c->hipfail(e, "pack_up2");
    u->up_wp = (const bf16_t*)p16; u->up_wp16 = (const bf16_t*)ph;
    return VT_OK;
}

static int finalize_image_decoder(vt_context* c, ImageDecoderW& d) {
    const int nb = (int)d.block_out.size(), C = d.block_out.back();
    {   // conv_in: the latent channels zero-padded to a 32-channel chunk, so that it runs on the halo conv (and on fp16 operands with flag 18)
        const int Lp = (d.latent + 31) / 32 * 32;
        const HostTensor* w = c->find("decoder.conv_in.weight");
        const HostTensor* b = c->find("decoder.conv_in.bias");
        if (!w || !b) return c->fail(VT_ERR_MISSING_WEIGHT, "missing weight decoder.conv_in.{weight,bias}");
        if (w->numel() != (int64_t)C * d.latent * 9 || b->numel() != C) return c->fail(VT_ERR_INVALID, "shape mismatch for decoder.conv_in");
        std::vector<float> wpad((size_t)C * Lp * 9, 0.f);
        for (int o = 0; o < C; ++o) std::copy(w->v.begin() + (size_t)o * d.latent * 9, w->v.begin() + (size_t)(o + 1) * d.latent * 9, wpad.begin() + (size_t)o * Lp * 9);
        VTCK(pack_conv(c, "decoder.conv_in", wpad.data(), b->v.data(), C, Lp, 3, &d.conv_in));
    }
    VTCK(get_mid_block(c, "decoder", C, false, &d.mid0, &d.attn, &d.mid1));
    int ci = C;
    for (int i = 0; i < nb; ++i) {
        UpBlockW u;
        const int co = d.block_out[nb - 1 - i];
        for (int j = 0; j < d.layers + 1; ++j) {
            ResnetW rw;
            char nm[128]; snprintf(nm, sizeof nm, "decoder.up_blocks.%d.resnets.%d", i, j);
            VTCK(get_resnet(c, nm, ci, co, &rw));
            u.res.push_back(rw);
            ci = co;
        }
        if (i + 1 < nb) {
            char nm[128]; snprintf(nm, sizeof nm, "decoder.up_blocks.%d.upsamplers.0.conv", i);
            VTCK(get_upsample_conv(c, nm, co, &u));
            u.has_up = true;
        }
        d.ups.push_back(u);
    }
    VTCK(get_norm(c, "decoder.conv_norm_out", ci, &d.norm_out));
    // conv_out (ci -> out_ch <= 32) rides the encoder's 32-cout conv_out tiles: rows [out_ch, 32) of the weight and the bias are zero
    const HostTensor* w = c->find("decoder.conv_out.weight");
    const HostTensor* b = c->find("decoder.conv_out.bias");
    if (!w || !b) return c->fail(VT_ERR_MISSING_WEIGHT, "missing weight decoder.conv_out.{weight,bias}");
    if (w->numel() != (int64_t)d.out_ch * ci * 9 || b->numel() != d.out_ch) return c->fail(VT_ERR_INVALID, "shape mismatch for decoder.conv_out");
    std::vector<float> wpad((size_t)32 * ci * 9, 0.f), bpad(32, 0.f);
    std::copy(w->v.begin(), w->v.end(), wpad.begin());
    std::copy(b->v.begin(), b->v.end(), bpad.begin());
    return pack_conv(c, "decoder.conv_out", wpad.data(), bpad.data(), 32, ci, 3, &d.conv_out);
}

extern "C" int vt_image_decoder_finalize(vt_context* c) {
    if (!c) return VT_ERR_INVALID;
    ImageDecoderW& d = c->imgdec;
    if (!d.configured) return c->fail(VT_ERR_STATE, "vt_image_decoder_configure was not called");
    DeviceGuard guard(c);
    // as vt_encoder_finalize: until THIS call succeeds the decoder is "not finalized" and no pointer of an earlier packing survives
    d.finalized = false;
    d.conv_in = ConvW(); d.mid0 = ResnetW(); d.mid1 = ResnetW(); d.attn = AttnW(); d.ups.clear(); d.norm_out = NormW(); d.conv_out = ConvW();
    c->free_allocs(c->imgdec_allocs);
    std::vector<void*>* const saved = c->cur_allocs;
    c->cur_allocs = &c->imgdec_allocs;
    c->pack_fp8 = false;                                  // decode has no fp8 mode
    const int r = finalize_image_decoder(c, d);
    c->pack_fp8 = true;
    c->cur_allocs = saved;
    erase_host_tensors(c, "decoder.");
    if (r) return r;
    d.finalized = true;
    return VT_OK;
}
