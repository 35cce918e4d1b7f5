// The VAE image decoder's launch schedule (host code) and its ABI: latents [B][latent][h][w] -> image [B][out_ch][8h][8w] for the FLUX
// configuration.  Layer order of the diffusers Decoder: conv_in, mid block (resnet, attention, resnet), the up blocks (layers_per_block + 1
// resnets each, an Upsample2D after all but the last), conv_norm_out + SiLU, conv_out.  Every layer but the Upsample2D conv runs on the
// kernels the encoder uses, and the mid block, every resnet and conv_out through the run layer both schedules share (VaeRun, vt_vae_run.h);
// what is the decoder's own: the latent staging + conv_in and the up blocks.  Upsample2D runs folded (conv3x3_up2.hip) or, with
// vt_set_flag 22 or for a shape that kernel refuses, as a nearest-2x pass + the stride-1 conv.  No fp8 mode: vt_decode_image switches the
// context's fp8 flag off for its own launches (the shared steps have fp8 branches).  No host synchronisation, caller-owned buffers.
#include <algorithm>

#include "vt_vae_run.h"

namespace vt {
namespace {

// z [B][L][h][w] fp32 -> NHWC 16-bit rows of Lp >= L channels (zeros above L: conv_in's operand, padded to a 32-channel chunk), bf16 or
// fp16 bits, optionally un-scaled first: (z - shift) / scaling, DiffusersVAEWrapper.decode's arithmetic in IEEE fp32
__global__ __launch_bounds__(256)
void latent_to_nhwc_kernel(const float* __restrict__ z, bf16_t* __restrict__ y, int L, int Lp, int HW, long long n, float shift, float scaling,
                           int unscale, int f16) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int ch = (int)(idx % Lp);
    const long long p = idx / Lp;
    const long long b = p / HW, px = p - b * HW;
    float v = 0.f;
    if (ch < L) {
        v = z[(b * L + ch) * HW + px];
        if (unscale) v = __fdiv_rn(__fsub_rn(v, shift), scaling);
    }
    if (f16) ((f16_t*)y)[idx] = (f16_t)v; else y[idx] = (bf16_t)v;
}

// the staged latents (conv_in's operand), carved between the (scale, shift) table and the attention scratch
size_t z16_bytes(const ImageDecoderW& d, int B, int h, int w) { return align_up((size_t)B * h * w * d.conv_in_cin() * 2 + SLACK); }

VaePlan plan_decoder(const ImageDecoderW& d, int B, int h, int w) {
    VaePlan p;
    // the producer of GroupNorm partials that only the decoder has: the folded Upsample2D conv, over the low-resolution tile grid
    auto note = [&](int hh, int ww, int ch) { p.note(hh, ww, ch, vt_conv3x3_up2_tiles((hh + 1) / 2, (ww + 1) / 2)); };
    const int nb = (int)d.block_out.size();
    int hh = h, ww = w;
    note(hh, ww, d.block_out.back());
    for (int i = 0; i < nb; ++i) {
        const int co = d.block_out[nb - 1 - i];
        note(hh, ww, co);
        if (i + 1 < nb) { hh *= 2; ww *= 2; note(hh, ww, co); }
    }
    p.finish(B, d.groups, h * w, d.block_out.back(), z16_bytes(d, B, h, w));
    return p;
}

bool shape_ok(const ImageDecoderW& d, int B, int h, int w) {
    if (B <= 0 || h < 1 || w < 1) return false;
    const int up = 1 << ((int)d.block_out.size() - 1);
    // 32-bit per-image offsets inside the kernels: the largest tensor is the last Upsample2D's output
    const long long H = (long long)h * up, W = (long long)w * up;
    int cmax = 0;
    for (int ch : d.block_out) cmax = std::max(cmax, ch);
    return H * W * cmax < (1LL << 31) && H < (1 << 20) && W < (1 << 20);
}

// The shared resnet / attention / conv_out steps take their fp8 branches from c->fp8: off for the lifetime of one vt_decode_image call,
// and back to what the caller (the encoder's mode) had set on every return path.
struct NoFp8 {
    vt_context* c; int saved;
    explicit NoFp8(vt_context* c_) : c(c_), saved(c_->fp8) { c->fp8 = 0; }
    ~NoFp8() { c->fp8 = saved; }
};

// One vt_decode_image call: the shared run plus what only the decoder has, the staged latents, conv_in and the up blocks.
struct DecRun : VaeRun {
    const ImageDecoderW& d;
    bf16_t* z16;                                   // the latents as conv_in's operand

    DecRun(vt_context* c_, const VaePlan& p, int B_, int h_, int w_, void* ws, hipStream_t s_) : VaeRun(c_, c_->imgdec.groups, B_, h_, w_, s_), d(c_->imgdec) {
        z16 = (bf16_t*)carve(p, ws, z16_bytes(d, B, h, w));
    }

    int conv_in(const float* z, int unscale) {
        const int Lp = d.conv_in_cin();
        const long long n = (long long)B * h * w * Lp;
        const bool xf16 = conv_f16(c, d.conv_in, 1, false);
        hipLaunchKernelGGL(latent_to_nhwc_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, z, z16, d.latent, Lp, h * w, n,
                           d.has_shift ? d.shift : 0.f, d.has_scaling ? d.scaling : 1.f, unscale, (int)xf16);
        HIPCK(c, hipGetLastError(), "latent_to_nhwc");
        ConvOpts o; o.gn = &gn; o.groups = groups; o.rdt = rdt; o.x_f16 = xf16;
        return run_conv(c, d.conv_in, z16, B, h, w, 1, 1, h, w, nullptr, f32[cur], nullptr, s, o);       // the halo conv where it takes the shape, else the generic GEMM
    }

    bool up_folded(const UpBlockW& u) const { return !c->up2_literal && u.up_wp != nullptr; }
    // does the block's Upsample2D conv multiply fp16 operands (so its input copy carries fp16 bits)?  The producer of that copy must be a halo conv.
    bool up_x_f16(const UpBlockW& u) const {
        const ResnetW& last = u.res.back();
        if (!c->f16_ops || c->fuse_gn_apply || !(c->use_halo_conv && last.c2.wp)) return false;
        return up_folded(u) ? u.up_wp16 != nullptr : conv_f16(c, u.up, 1, false);
    }

    // the resnets of up block i and, unless it is the last, its Upsample2D
    int up_block(size_t i) {
        const UpBlockW& u = d.ups[i];
        const bool xf16 = u.has_up && up_x_f16(u);
        for (size_t j = 0; j < u.res.size(); ++j) {
            BlockOut out;
            out.only16 = u.has_up && j + 1 == u.res.size();
            out.f16 = out.only16 && xf16;
            VTCK(resnet(u.res[j], out));
        }
        if (!u.has_up) return VT_OK;
        const int ch = u.up.cout, nxt = (cur + 1) % 3;
        const ResnetW* next = d.ups[i + 1].res[0].has_sc ? &d.ups[i + 1].res[0] : nullptr;
        // the 16-bit copy of the new h for the next block's conv_shortcut: in tmid when a separate shortcut conv consumes it before conv1
        // overwrites tmid; fused into conv2 it must outlive conv1, so it goes to the third rotating buffer (that block's `scb`)
        bf16_t* copy = !next ? nullptr : (fuse_sc(*next) ? (bf16_t*)f32[(nxt + 2) % 3] : tmid);
        const bool folded = up_folded(u);
        const bool copy16 = copy && fuse_sc(*next) && conv_f16(c, next->c2, 1, true) && (folded || (c->use_halo_conv && u.up.wp));
        const int cpg = ch / groups;
        const bool fuse = c->fuse_gn_stats && (cpg == 4 || cpg == 8 || cpg == 16);
        if (folded) {
            ConvUp2Args a{};
            a.X = hb; a.Wp = xf16 ? u.up_wp16 : u.up_wp; a.f16 = xf16; a.bias = u.up.b; a.zeros = c->zeros;
            a.out_f32 = rdt == 1 ? (float*)f32[nxt] : nullptr; a.out_f16 = rdt == 2 ? (f16_t*)f32[nxt] : nullptr;
            a.out_16 = copy; a.out16_f16 = copy16;
            a.batch = B; a.H = h; a.W = w; a.Cin = ch; a.Cout = ch;
            gn.parts = 0;
            if (fuse) { a.gn_partial = gn.partial; a.gn_cpg = cpg; gn.parts = vt_conv3x3_up2_tiles(h, w); }
            VTCK(profiled(c, s, VT_PROF_UP2, 2.0 * B * (double)(4 * h * w) * ch * 4.0 * ch, "conv3x3_up2", [&] { return vt_launch_conv3x3_up2(a, s); }));
        } else {
            HIPCK(c, vt_launch_upsample2x_nhwc16(hb, act, B, h, w, ch, s), "upsample2x");
            ConvOpts o;
            o.gn = &gn; o.groups = groups; o.rdt = rdt; o.x_f16 = xf16; o.o16_f16 = copy16;
            VTCK(run_conv(c, u.up, act, B, 2 * h, 2 * w, 1, 1, 2 * h, 2 * w, nullptr, f32[nxt], copy, s, o));
        }
        h16 = copy; h16_is_f16 = copy16;
        cur = nxt; h *= 2; w *= 2;
        return VT_OK;
    }
};

}  // namespace
}  // namespace vt

using namespace vt;

extern "C" {

int vt_image_decoder_configure(vt_context* c, int out_ch, int latent, const int* block_out, int n_blocks, int layers, int groups,
                               float scaling, int has_scaling, float shift, int has_shift) {
    if (!c) return VT_ERR_INVALID;
    if (out_ch < 1 || out_ch > 32) return c->fail(VT_ERR_INVALID, "out_channels must be 1..32 (got %d)", out_ch);
    if (!block_out || n_blocks < 1 || n_blocks > 8 || layers < 1 || layers > 8 || latent < 1 || latent > 256 || groups < 1)
        return c->fail(VT_ERR_INVALID, "bad image decoder configuration");
    ImageDecoderW& d = c->imgdec;
    { DeviceGuard guard(c); c->free_allocs(c->imgdec_allocs); }       // a re-upload replaces the packed weights; the encoder's are untouched
    d = ImageDecoderW();
    d.out_ch = out_ch; d.latent = latent; d.layers = layers; d.groups = groups;
    d.block_out.assign(block_out, block_out + n_blocks);
    VTCK(check_block_out(c, block_out, n_blocks, groups));
    if (has_scaling && scaling == 0.f) return c->fail(VT_ERR_INVALID, "scaling_factor must not be 0");
    d.scaling = scaling; d.has_scaling = has_scaling != 0; d.shift = shift; d.has_shift = has_shift != 0;
    d.configured = true;
    return VT_OK;
}

size_t vt_decode_image_workspace_bytes(const vt_context* c, int B, int h, int w) {
    if (!c || !c->imgdec.configured || !shape_ok(c->imgdec, B, h, w)) return 0;
    return plan_decoder(c->imgdec, B, h, w).total;
}

int vt_decode_image(vt_context* c, const float* z, int B, int h, int w, int unscale, float* image, size_t image_bytes, void* ws, size_t ws_bytes,
                    void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    const ImageDecoderW& d = c->imgdec;
    if (!d.finalized) return c->fail(VT_ERR_STATE, "image decoder weights not finalized");
    if (!z || !image || !ws) return c->fail(VT_ERR_INVALID, "vt_decode_image: null buffer");
    if (!shape_ok(d, B, h, w)) return c->fail(VT_ERR_INVALID, "vt_decode_image: unsupported shape %d x %d x %d", B, h, w);
    const int up = 1 << ((int)d.block_out.size() - 1);
    const size_t need_img = (size_t)B * d.out_ch * ((size_t)h * up) * ((size_t)w * up) * 4;
    if (image_bytes < need_img) return c->fail(VT_ERR_INVALID, "vt_decode_image: image buffer %zu < required %zu", image_bytes, need_img);
    const VaePlan p = plan_decoder(d, B, h, w);
    if (ws_bytes < p.total) return c->fail(VT_ERR_WORKSPACE, "vt_decode_image: workspace %zu < required %zu", ws_bytes, p.total);
    if (((uintptr_t)ws) % ALIGN) return c->fail(VT_ERR_INVALID, "vt_decode_image: workspace must be 256-B aligned");
    const NoFp8 no_fp8(c);                                               // decode has no fp8 form: 16-bit operands everywhere
    DecRun run(c, p, B, h, w, ws, (hipStream_t)stream);
    VTCK(run.conv_in(z, unscale));
    VTCK(run.resnet(d.mid0));
    VTCK(run.mid_attention(d.attn));
    VTCK(run.resnet(d.mid1));
    for (size_t i = 0; i < d.ups.size(); ++i) VTCK(run.up_block(i));
    // conv_norm_out + SiLU + conv_out -> fp32 NCHW image (the first out_ch of the zero-padded 32 couts)
    return run.conv_out(d.conv_out, d.norm_out, d.out_ch, 1.f, 0.f, image);
}

}  // extern "C"
