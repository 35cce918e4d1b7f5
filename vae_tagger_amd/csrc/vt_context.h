// Internal to the host side of the library: the context behind the C ABI, the packed-weight tables, and the few functions that
// cross the host units (weights.hip, encoder.hip, vae_run.hip, image_decoder.hip, attention.hip, attention_backward.hip, ops.hip,
// ops_backward.hip, capi.hip): the conv / GroupNorm launch helpers of encoder.hip and attention.hip's entry.  What the operator entries share
// on top of it (their argument checks) is vt_ops.h.  The run layer both VAE schedules are built on (VaeRun: workspace plan and
// carve, resnet / mid-attention / conv_out steps) has a header of its own, vt_vae_run.h.  Nothing here is part of the public header.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include <array>
#include <map>
#include <string>
#include <vector>

#include "../../include/vae_tagger_hip.h"
#include "vt_decoder.h"
#include "vt_kernels.h"

namespace vt {

struct HostTensor {
    std::vector<float> v;
    std::vector<int64_t> shape;
    int64_t numel() const { int64_t n = 1; for (auto d : shape) n *= d; return n; }
};

struct ConvW {
    const bf16_t* w = nullptr; const bf16_t* wp = nullptr; const float* b = nullptr; int cin = 0, cout = 0, k = 0;   // w: [cout][tap][cin]; wp: halo-kernel packing
    const bf16_t* wp2 = nullptr;        // stride-2 phase-plane kernel's packing (conv3x3_s2_halo.hip)
    const bf16_t* wpo = nullptr; const bf16_t* wpo16 = nullptr;   // conv_out_halo.hip's packing [cin/32][tap][32 couts][32] (bf16 / fp16 bits), Cout == 32 only
    // the same three layouts holding fp16 bits (vt_set_flag 18: fp16 operands for the convs); w16 only for Cout <= 32 (conv_out)
    const bf16_t* w16 = nullptr; const bf16_t* wp16 = nullptr; const bf16_t* wp2_16 = nullptr;
    const unsigned char* wp8 = nullptr; const float* mult8 = nullptr;   // fp8 halo kernel: e4m3 weights / per-cout (scale / act_scale)
    const unsigned char* w8g = nullptr; const float* mult8g = nullptr;  // fp8 generic GEMM (stride-2 convs): [cout][tap][cin] e4m3 / per-cout scale (input scale 1)
    const unsigned char* wp8s2 = nullptr;                                // fp8 stride-2 phase-plane kernel's packing (same scales: mult8g)
};
struct NormW { const float* g = nullptr; const float* b = nullptr; int c = 0; };
struct ResnetW {
    NormW n1, n2; ConvW c1, c2, sc; bool has_sc = false; int cin = 0, cout = 0;
    // conv_shortcut fused into conv2's launch (Conv3x3Args::scW): [cin/32][cout][32] bf16, interleaved cout rows; bias c2 + sc
    const bf16_t* sc_wp = nullptr; const float* b_c2sc = nullptr;
    const bf16_t* sc_wp16 = nullptr;     // sc_wp holding fp16 bits (vt_set_flag 18)
    const bf16_t* sc_wp8 = nullptr;      // the same for the fp8 conv2: rows in its cout order, values divided by conv2's mult[cout]
};
struct AttnW { NormW gn; const bf16_t *wqk = nullptr, *wv = nullptr, *wo = nullptr; const float *bqk = nullptr, *bv = nullptr, *bo = nullptr; int c = 0;
               // fp8 mode's projections (proj_fp8_kernel): [Wq; Wk] and Wv as e4m3(W / s), one scale per matrix
               const unsigned char *wqk8 = nullptr, *wv8 = nullptr; float sqk = 1.f, sv = 1.f; };
struct StageW { std::vector<ResnetW> res; bool has_down = false; ConvW down; };

struct EncoderW {
    bool configured = false, finalized = false;
    int in_ch = 3, latent = 16, layers = 2, groups = 32;
    std::vector<int> block_out;
    float scaling = 1.f, shift = 0.f;
    bool has_scaling = false, has_shift = false;
    const bf16_t* conv_in_wpk = nullptr; // MFMA variant (C0 == 128, 32 groups): [128 rows][32 k] bf16, interleaved cout rows
    const float* conv_in_w = nullptr;   // [27][C0] fp32
    const float* conv_in_b = nullptr;
    std::vector<StageW> stages;
    ResnetW mid0, mid1;
    AttnW attn;
    NormW norm_out;
    ConvW conv_out;
};

// The VAE's image decoder (diffusers Decoder: conv_in, mid block, up blocks with Upsample2D, conv_norm_out, conv_out).
struct UpBlockW {
    std::vector<ResnetW> res; bool has_up = false;
    ConvW up;                                                    // upsamplers.0.conv as an ordinary 3x3 conv: the literal route (vt_set_flag 22)
    const bf16_t* up_wp = nullptr; const bf16_t* up_wp16 = nullptr;   // the folded packing (conv3x3_up2.hip), bf16 / fp16 bits; null where the kernel refuses the shape
};
struct ImageDecoderW {
    bool configured = false, finalized = false;
    int out_ch = 3, latent = 16, layers = 2, groups = 32;
    std::vector<int> block_out;
    float scaling = 1.f, shift = 0.f;
    bool has_scaling = false, has_shift = false;
    ConvW conv_in;                                               // over the latent channels zero-padded to a 32-channel chunk
    int conv_in_cin() const { return (latent + 31) / 32 * 32; }
    ResnetW mid0, mid1;
    AttnW attn;
    std::vector<UpBlockW> ups;
    NormW norm_out;
    ConvW conv_out;                                              // zero-padded to 32 couts (the 32-cout tiles write the first out_ch as fp32 NCHW)
};

constexpr float FP8_ACT_SCALE = 8.0f;      // activations are stored as e4m3(8 x): |silu(GroupNorm)| up to 56 before saturation
constexpr float FP8_RES_SCALE = 1.0f;      // the un-normalised residual stream feeding a stride-2 conv is stored as e4m3(x): |x| up to 448

constexpr size_t ALIGN = 256;
inline size_t align_up(size_t x) { return (x + ALIGN - 1) / ALIGN * ALIGN; }

}  // namespace vt

struct vt_context {
    int device = 0;
    std::string err;
    std::map<std::string, vt::HostTensor> weights;
    std::vector<void*> enc_allocs, dec_allocs, imgdec_allocs;     // packed weights (encoder, tag decoder, image decoder), each freed when ITS model is configured again
    vt::ImageDecoderW imgdec;
    std::vector<void*>* cur_allocs = &enc_allocs;
    bool pack_fp8 = true;           // weights.hip: pack the e4m3 forms of the 3x3 convs too (off while the image decoder, which has no fp8 mode, is finalized)
    void* zeros = nullptr;
    int* status = nullptr;          // device word: sticky VT_STATUS_* bits raised by kernels (vt_status reads / clears it)
    vt::EncoderW enc;
    DecoderWeights dec;
    bool dec_configured = false, dec_finalized = false;
    int use_halo_conv = 1;          // vt_set_flag(ctx, 0, v)
    int fuse_gn_stats = 1;          // vt_set_flag(ctx, 1, v)
    int fuse_gn_apply = 0;          // vt_set_flag(ctx, 2, v): break-even on MI355X today, off by default
    int res_fp16 = 1;               // vt_set_flag(ctx, 4, v): residual stream stored as fp16 (math stays fp32)
    int attn_mode = 0;              // vt_set_flag(ctx, 7, v): see run_attention
    int fuse_shortcut = 1;          // vt_set_flag(ctx, 8, v): resnet conv_shortcut inside conv2's launch
    int pv_stream = 1;              // vt_set_flag(ctx, 10, v): P.V reads P (4+ GB, read once) with the streaming cache policy
    int attn_qk_kernel = 1;         // vt_set_flag(ctx, 9, v): dedicated Q.K^T kernel (attn_qk.hip) instead of the generic GEMM
    int attn_pv_kernel = 1;         // vt_set_flag(ctx, 12, v): P.V on its own kernel, P in MFMA fragment order (attn_pv.hip)
    int fp8 = 0;                    // vt_set_flag(ctx, 11, v): stride-1 3x3 resnet convs on fp8 (e4m3) operands (BASELINE configs[4])
    int halo_occ2 = 3;              // vt_set_flag(ctx, 3, v): two-workgroups-per-CU tile mode of the halo conv
    int gemm_short = 1;             // vt_set_flag(ctx, 6, v): short-K GEMM launches on the two-workgroups-per-CU tile
    int proj_fp8 = 1;               // vt_set_flag(ctx, 15, v): with the fp8 attention, the q | k and v projections on e4m3 operands too, writing q8 | k8 and v8^T directly
    int attn_fp8 = 1;               // vt_set_flag(ctx, 14, v): in fp8 mode (flag 11) Q.K^T and P.V run on e4m3 operands too (attn_fp8.hip)
    // diagnostics (vt_debug_trace): order-independent checksums of every GroupNorm's (scale, shift) table, in launch order
    unsigned long long* dbg = nullptr; int dbg_n = 0; bool dbg_on = false;
    int conv_out_halo = 1;          // vt_set_flag(ctx, 20, v): conv_out on its 32-cout halo tile (conv_out_halo.hip) instead of the generic GEMM
    int s2_planar = 1;              // vt_set_flag(ctx, 19, v): the 16-bit / e4m3 copy of a stage's output that feeds its stride-2 conv is written chunk-planar
    int eval_merge_vec = 1;         // vt_set_flag(ctx, 21, v): vt_eval_export / vt_eval_merge move keys 16 B per lane on the aligned part (0: 8 B)
                                    // ([C/32 or C/64][H][W][chunk]) so that both halves of every 128-B line are staged three K-steps apart, not nine
    int f16_ops = 0;                // vt_set_flag(ctx, 18, v): fp16 instead of bf16 operands for the convs (same 2 B, 11 significand bits instead of 8)
    int attn_proj_kernel = 1;       // vt_set_flag(ctx, 17, v): the bf16 q | k and v^T projections on attn_qk.hip's skeleton (mode 4) instead of the generic GEMM
    int fp8_tile = 0;               // vt_set_flag(ctx, 16, v): fp8 halo conv tile shape = v & 3 (0: 8 x 32 px, 4 waves, two workgroups per CU; 1: 16 x 32 px;
                                    // 2: 8 x 64 px, 8 waves, one per CU) on the layers with Cin <= 128, or on every layer with v & 4
    int up2_literal = 0;            // vt_set_flag(ctx, 22, v): Upsample2D as a nearest-2x pass + the stride-1 3x3 conv instead of the folded kernel (conv3x3_up2.hip)
    int s2_dgrad_literal = 0;       // vt_set_flag(ctx, 23, v): vt_op_conv_s2_backward_data as a scatter pass + the stride-1 data gradient instead of conv3x3_s2_dgrad.hip
    int s2_halo = 1;                // vt_set_flag(ctx, 13, v): stride-2 convs on the phase-plane halo kernel instead of the generic GEMM
    // vt_resize_u8: pinned staging of the coefficient tables + the event of the last H2D copy that read it
    int* rs_host = nullptr; size_t rs_host_ints = 0; hipEvent_t rs_event = nullptr;
    // vt_resize_normalize_batch: a ring of pinned blocks (descriptors + coefficient tables of one call each), the event of the H2D copy that
    // last read each, and the host tables already built, keyed (in size, out size, filter, transposed)
    struct RsRingSlot { void* host = nullptr; size_t bytes = 0; hipEvent_t ev = nullptr; bool used = false; };
    static constexpr int RS_RING = 4;
    RsRingSlot rs_ring[RS_RING];
    unsigned rs_ring_next = 0;
    std::map<std::array<int, 4>, std::vector<int>> rs_tables;
    int conv_in_mfma = 1;           // vt_set_flag(ctx, 5, v): conv_in on the matrix cores (bf16 im2col), else exact fp32 VALU
    void* op_scratch = nullptr; size_t op_scratch_bytes = 0;

    // optional per-launch timing of the MFMA kernel (HIP events on the launch stream)
    struct ProfRec { hipEvent_t e0, e1; double flops; int cfg; };
    bool profiling = false;
    std::vector<ProfRec> prof;
    std::vector<hipEvent_t> event_pool;
    size_t events_used = 0;
    hipEvent_t next_event() {
        if (events_used == event_pool.size()) {
            hipEvent_t e = nullptr;
            if (hipEventCreate(&e) != hipSuccess) return nullptr;
            event_pool.push_back(e);
        }
        return event_pool[events_used++];
    }

    int fail(int code, const char* fmt, ...) {
        char buf[512];
        va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
        err = buf;
        return code;
    }
    int hipfail(hipError_t e, const char* what) { return fail(VT_ERR_HIP, "%s: %s", what, hipGetErrorString(e)); }

    void* upload(const void* host, size_t bytes) {
        void* d = nullptr;
        if (hipMalloc(&d, bytes ? bytes : 16) != hipSuccess) return nullptr;
        cur_allocs->push_back(d);
        if (bytes && hipMemcpy(d, host, bytes, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
        return d;
    }
    void free_allocs(std::vector<void*>& v) {
        for (void* p : v) (void)hipFree(p);
        v.clear();
    }
    // the operators' halo-type kernels read repacked weights: op_scratch, one buffer for them, grown on demand (its contents are not kept)
    int ensure_op_scratch(size_t bytes) {
        if (op_scratch_bytes >= bytes) return VT_OK;
        if (op_scratch) (void)hipFree(op_scratch);
        op_scratch = nullptr; op_scratch_bytes = 0;
        const hipError_t e = hipMalloc(&op_scratch, bytes);
        if (e != hipSuccess) return hipfail(e, "hipMalloc(op scratch)");
        op_scratch_bytes = bytes;
        return VT_OK;
    }
    const vt::HostTensor* find(const std::string& k) const {
        auto it = weights.find(k);
        return it == weights.end() ? nullptr : &it->second;
    }
};

namespace vt {

// Every entry point that touches the GPU runs on the context's device and leaves the caller's current device as it found it.
struct DeviceGuard {
    int prev = -1, dev;
    explicit DeviceGuard(const vt_context* c) : dev(c->device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() { if (prev >= 0 && prev != dev) (void)hipSetDevice(prev); }
};

#define HIPCK(ctx, e, what) do { hipError_t _e = (e); if (_e != hipSuccess) return (ctx)->hipfail(_e, what); } while (0)
#define VTCK(e) do { const int _r = (e); if (_r) return _r; } while (0)       // pass a VT_ERR_* of a callee on (its message is already set)

// The one profiler bracket: `launch()` (returning hipError_t) between two events of the pool, recorded under `slot` with `count`
// (FLOPs; bytes for VT_PROF_GN_APPLY) -- or, with profiling off, just the launch.
template <class Launch>
int profiled(vt_context* c, hipStream_t s, int slot, double count, const char* what, Launch&& launch) {
    if (!c->profiling) { HIPCK(c, launch(), what); return VT_OK; }
    vt_context::ProfRec r;
    r.e0 = c->next_event(); r.e1 = c->next_event();
    if (!r.e0 || !r.e1) return c->fail(VT_ERR_HIP, "event pool exhausted");
    r.flops = count; r.cfg = slot;
    HIPCK(c, hipEventRecord(r.e0, s), "hipEventRecord");
    HIPCK(c, launch(), what);
    HIPCK(c, hipEventRecord(r.e1, s), "hipEventRecord");
    c->prof.push_back(r);
    return VT_OK;
}

// ---- weights.hip ----------------------------------------------------------------------------------
float bf2f(uint16_t h);
float h2f(uint16_t h);
std::vector<float> pack_conv_in(const float* w_o27, int cout);                      // [cout][27] -> [k = ci*9+ky*3+kx][cout] fp32
std::vector<uint16_t> pack_conv_in_mfma(const float* w_o27, const float* bias);
// every e4m3 form of one 3x3 conv, from one set of per-cout scales
struct ConvE4m3 {
    std::vector<uint8_t> wp8;  std::vector<float> mult8;      // conv3x3_halo_fp8.hip's packing, scale / FP8_ACT_SCALE
    std::vector<uint8_t> w8g;  std::vector<float> mult8g;     // the generic GEMM's [cout][tap][cin], scale / FP8_RES_SCALE
    std::vector<uint8_t> wp8s2;                               // conv3x3_s2_halo_fp8.hip's packing (scales: mult8g); only when asked for
};
ConvE4m3 pack_conv_e4m3(const float* w_oihw, int cout, int cin, bool s2_layout);
// The per-layer packers vt_encoder_finalize / vt_image_decoder_finalize and vt_op_conv3x3_block share; every upload goes to c->cur_allocs.
// pack_conv: every packing of one conv from its fp32 OIHW weight `wv` and bias `bv` (cout floats, host); `name` is for messages only;
// `mult8_host` receives the fp8 halo kernel's per-cout multipliers (empty when the conv has no fp8 form).
int pack_conv(vt_context* c, const std::string& name, const float* wv, const float* bv, int cout, int cin, int k, ConvW* out, bool stride2 = false,
              std::vector<float>* mult8_host = nullptr);
// pack_fused_shortcut: a 1x1 conv_shortcut for conv2's launch (Conv3x3Args::scW): [cin/32][cout rows, interleaved][32] as bf16 (*wp) and
// fp16 bits (*wp16), and the launch's bias `bias_sum` = conv2's + the shortcut's (cout floats, host) as *bias.  cin % 32 == 0.
int pack_fused_shortcut(vt_context* c, const std::string& name, const float* w_oi, const float* bias_sum, int cout, int cin, const bf16_t** wp,
                        const float** bias, const bf16_t** wp16);

// ---- capi.hip (Pillow's resample tables, shared with resize_batch.hip) ----------------------------
int rs_ksize(int in_size, int out_size, int kind);
void rs_table(int in_size, int out_size, int kind, int* tab);     // tab[out_size][2 + ksize] = (first, count, coefficients...)

// ---- capi.hip (diagnostics) -----------------------------------------------------------------------
void dbg_sum(vt_context* c, const void* p, size_t bytes, hipStream_t s);

// ---- encoder.hip ----------------------------------------------------------------------------------
// GroupNorm bookkeeping: `partial` holds (n, mean, M2) triples for the tensor that will be normalised next,
// written either by the producing conv's epilogue (stats_parts > 0) or by the standalone stats pass.
struct GnState {
    float* partial = nullptr; float* ss = nullptr;
    int parts = 0;            // triples per (image, group) currently in `partial`; 0 = none
};
struct ScFuse { const bf16_t* x; const bf16_t* wp; const float* bias; int cin; const bf16_t* wp8; const bf16_t* wp16;
                bool x_f16;      // x carries fp16 bits (its producer wrote them for an fp16-operand conv2); else bf16
};
// What a run_conv call may ask for beyond the plain conv; a call site names only what it means.
struct ConvOpts {
    GnState* gn = nullptr;              // if non-null, the epilogue also writes GroupNorm partials of the output (cpg = cout / groups)
    int groups = 32;
    // when ss is given the conv input is silu(x*scale + shift) with x = xnorm_f32 (fp32) or x (bf16),
    // fused into the halo staging (only valid when norm_conv_fusable()).
    const float* xnorm_f32 = nullptr; const float* ss = nullptr;
    int rdt = 1;                        // `res` / `oh` are the residual-stream tensors (input to add, output to write): fp32 when rdt == 1, fp16 when rdt == 2
    const ScFuse* sc = nullptr;         // a 1x1 conv of sc->x fused into the halo launch (resnet conv_shortcut); then `res` must be null
    bool x_fp8 = false, o16_e4m3 = false;
    bool x_f16 = false;                 // x (and sc->x) hold fp16 bits: conv_f16() of this conv
    bool o16_f16 = false;               // o16 is written as fp16 bits: conv_f16() of ITS consumer
    bool planar = false;                // stride 1: o16 is written chunk-planar; stride 2: x is chunk-planar (both: s2_input_planar() of the stride-2 conv)
};
int launch_gemm(vt_context* c, const ConvGemmArgs& a, hipStream_t s, const char* what);
int launch_halo(vt_context* c, const Conv3x3Args& a, hipStream_t s, const char* what);
int launch_halo_fp8(vt_context* c, const Conv3x3Fp8Args& a, hipStream_t s, const char* what);
int run_conv(vt_context* c, const ConvW& w, const bf16_t* x, int B, int Hin, int Win, int stride, int pad, int Hout, int Wout,
             const void* res, void* oh, bf16_t* o16, hipStream_t s, const ConvOpts& o = ConvOpts());
// y = act(GroupNorm(x)) as 16-bit rows (xdt 0 bf16, 1 fp32, 2 fp16); uses epilogue-produced partials when g.parts > 0
int run_gn(vt_context* c, const void* x, int xdt, int B, int HW, const NormW& n, int groups, int silu, bf16_t* y, GnState& g, hipStream_t s,
           bool out_fp8 = false, bool out_f16 = false);
// fp16-operand mode (vt_set_flag 18): does THIS conv multiply fp16 operands?
bool conv_f16(const vt_context* c, const ConvW& w, int stride, bool has_sc);
// what run_norm_conv's caller may ask of the conv's 16-bit output, and the shortcut to fuse
struct NormConvOpts { const ScFuse* sc = nullptr; bool o16_e4m3 = false, o16_f16 = false, o16_planar = false; };
// conv3x3(silu(GroupNorm(x))): x is the tensor to normalise (xdt), res / oh the residual in / out (rdt), o16 an optional 16-bit copy
int run_norm_conv(vt_context* c, const NormW& n, const ConvW& w, const void* x, int xdt, int B, int H, int W, int groups, bf16_t* act,
                  const void* res, void* oh, bf16_t* o16, GnState& gn, bool want_stats, hipStream_t s, int rdt, const NormConvOpts& nc = NormConvOpts());

// ---- attention.hip --------------------------------------------------------------------------------
struct AttnScratch {
    bf16_t* qk; bf16_t* vt; f16_t* scores; bf16_t* probs; bf16_t* o;
    unsigned char* qk8; unsigned char* vt8;     // fp8 attention operands: e4m3(8 q | 8 k) [B][S][2C], e4m3(8 v^T) [B][C][attn_pitch8(S)]
    unsigned char* x8; float* ident;            // op-level entry only: e4m3(8 x) tokens made from the caller's bf16 ones, and the identity (scale, shift) that pass takes
    float* qn; float* kn; float* sd; float* shift; float* rinv; float* part; int* flags;
    int group;
    float* save_sums = nullptr;                 // training forward: [4][B][S] copy of every image's segment sums (the partials scratch holds one group's)
};
size_t attn_pitch_of(int S);                    // row pitch (elements) of v^T and of the row-major S x S matrices
int attn_group_of(int B, int S);                // images whose probabilities are materialised at a time
int attn_sweep_nsplit(int qblocks, int ktiles, int min_tiles);      // workgroups per query block of a segment-sum sweep
size_t attn_scratch_bytes(int B, int S, int C);
AttnScratch carve_attn(char* p, int B, int S, int C);
bool attn_proj_is_fp8(const vt_context* c, const AttnW& w, int S, int C);
int run_attention(vt_context* c, const AttnW& w, const bf16_t* x16, const void* res, void* out, int B, int S, const AttnScratch& sc,
                  hipStream_t s, GnState* gn = nullptr, int groups = 32, int rdt = 1, bool x_e4m3 = false);

}  // namespace vt
