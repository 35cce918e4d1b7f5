// The run layer that the VAE encoder's and the image decoder's launch schedules share (bodies in vae_run.hip): the workspace plan and its
// carve, the rotating residual-stream buffers, and the steps both models are made of -- ResnetBlock2D, the mid block's attention,
// conv_norm_out + conv_out.  encoder.hip adds conv_in and the down stages, image_decoder.hip conv_in and the up blocks.
#pragma once
#include "vt_context.h"

namespace vt {

constexpr size_t SLACK = 4096;

// What one call needs of its workspace.  A schedule notes every activation tensor it holds, then finishes the plan.
struct VaePlan {
    size_t max_elems = 0;      // per image, largest activation tensor (elements)
    int max_c = 0, max_chunks = 0;
    int S = 0, C = 0;          // the mid block's attention: tokens, channels
    size_t total = 0;
    // a [h][w][ch] tensor; own_parts: the most GroupNorm-partial triples per (image, group) that a producer only this schedule has writes
    // of it (the standalone pass, the generic GEMM and the stride-1 halo conv are counted here)
    void note(int h, int w, int ch, int own_parts);
    // extra: bytes the schedule carves for itself between the (scale, shift) table and the attention scratch
    void finish(int B, int groups, int S_, int C_, size_t extra = 0);
};

// what the kernels ask of a block_out_channels list and norm_num_groups (both vt_*_configure entries); sets the error message
int check_block_out(vt_context* c, const int* block_out, int n, int groups);

// what the conv that follows a block wants of the block's output (the 16-bit copy `hb`)
struct BlockOut {
    bool only16 = false;      // the only consumer is that conv (16-bit operand, no norm): skip the residual-stream copy of h and the stats
    bool e4m3 = false;        // that conv runs on fp8 operands, so the copy is written as e4m3 instead of bf16
    bool f16 = false, planar = false;
};

// One vt_encode / vt_decode_image call: the carved workspace and the position in the rotating buffers.
struct VaeRun {
    vt_context* c; int B; hipStream_t s;
    int rdt;                                       // residual-stream buffers: fp16 by default (res_fp16), fp32 otherwise; sized for fp32 either way
    int groups;
    void* f32[3]; bf16_t* b16[3];
    GnState gn; AttnScratch as;
    int cur = 0;                                   // f32[cur] holds the residual stream h
    bf16_t *act, *tmid, *hb;                       // GN(+SiLU) output = conv operand / conv1 output / 16-bit copy of h feeding a stride-2 or Upsample2D conv
    int h, w;
    const bf16_t* h16 = nullptr;                   // 16-bit copy of the current h, when one exists (a stride-2 / Upsample2D conv wrote it for the next conv_shortcut) ...
    bool h16_is_f16 = false;                       // ... holding fp16 bits (fp16-operand mode, for a fused shortcut) instead of bf16

    VaeRun(vt_context* c_, int groups_, int B_, int h_, int w_, hipStream_t s_)
        : c(c_), B(B_), s(s_), rdt(c_->res_fp16 ? 2 : 1), groups(groups_), h(h_), w(w_) {}

    // lays the plan out in ws: 3 residual + 3 16-bit buffers, partials, (scale, shift) table, `extra` bytes, attention scratch.
    // Returns the `extra` bytes, i.e. the pointer just past the table.
    char* carve(const VaePlan& p, void* ws, size_t extra = 0);

    bool fuse_sc(const ResnetW& rw) const;
    // one ResnetBlock2D: h <- conv2(silu(gn(conv1(silu(gn(h)))))) + shortcut(h16); consumes h16
    int resnet(const ResnetW& rw, const BlockOut& out = BlockOut());
    int mid_attention(const AttnW& attn);
    // norm + SiLU + conv_out -> the first `keep` couts * post_scale + post_shift as fp32 NCHW
    int conv_out(const ConvW& cw, const NormW& norm, int keep, float post_scale, float post_shift, float* out);
};

}  // namespace vt
