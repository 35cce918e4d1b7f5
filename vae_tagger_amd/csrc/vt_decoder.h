// Decoder weight table (device fp32 pointers) + launch entry points, shared by decoder.hip and the host side (vt_context.h, capi.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

struct DecSelfAttnW {
    const float *ln_w, *ln_b, *q_w, *q_b, *k_w, *k_b, *v_w, *v_b, *o_w, *o_b;
};

struct DecoderWeights {
    int num_classes = 0;
    int latent_channels = 16;
    int heads = 8;
    int plain = 0;            // ClassificationDecoder (--no_attention)
    int use_spatial = 0, use_self = 0, use_cross = 0;
    int ca_hidden = 2;
    const float *ca_w0 = nullptr, *ca_w2 = nullptr, *sa_w = nullptr;
    const float *fc_w = nullptr, *fc_b = nullptr, *bn_scale = nullptr, *bn_shift = nullptr;
    // the BatchNorm tensors bn_scale / bn_shift were folded from (the front trainer reads and writes them: train_front.hip)
    const float *bn_w = nullptr, *bn_b = nullptr, *bn_mean = nullptr, *bn_var = nullptr;
    DecSelfAttnW sa{};
    const float *qg_w = nullptr, *qg_b = nullptr;
    const float *cx_q_w = nullptr, *cx_q_b = nullptr, *cx_k_w = nullptr, *cx_k_b = nullptr;
    const float *cx_v_w = nullptr, *cx_v_b = nullptr, *cx_o_w = nullptr, *cx_o_b = nullptr;
    const float* cls_w[4] = {nullptr, nullptr, nullptr, nullptr};
    const float* cls_b[4] = {nullptr, nullptr, nullptr, nullptr};
    const float* cls_ln_w[3] = {nullptr, nullptr, nullptr};
    const float* cls_ln_b[3] = {nullptr, nullptr, nullptr};
};

// the classifier head: `hidden` Linear -> LayerNorm -> activation layers of widths dims[1..hidden] over a feature row of dims[0]
// floats, then Linear(dims[hidden], dims[hidden + 1] = num_classes); act 0 = ReLU, 1 = LeakyReLU(0.2)
struct DecHeadShape { int hidden = 0; int dims[5] = {0, 0, 0, 0, 0}; int act = 0; };
struct DecHeadParams { const float* w[4]; const float* b[4]; const float* ln_w[3]; const float* ln_b[3]; };
DecHeadShape vt_decoder_head_shape(const DecoderWeights& w);
// the head's two kernels, as vt_decoder_forward launches them (train_head.hip's forward runs the same launches: same bits)
hipError_t vt_dec_linear(const float* x, const float* w, const float* bias, float* y, int B, int IN, int OUT, hipStream_t s);
hipError_t vt_dec_ln_act(float* y, const float* g, const float* b, int rows, int N, int act, hipStream_t s);
// SpatialAttention's pool [B][C][2], channel gate [B][C] and spatial gate [B][HW], as vt_decoder_front launches them (train_front.hip's
// training-mode forward runs the same launches: same bits)
hipError_t vt_dec_pool(const float* x, int B, int C, int HW, float* pool, hipStream_t s);
hipError_t vt_dec_gate(const float* pool, const float* w0, const float* w2, int B, int C, int R, float* gate, hipStream_t s);
hipError_t vt_dec_sgate(const float* sp, const float* w, int B, int H, int W, float* sg, hipStream_t s);
// the cross-attention piece over the front's rows x [B][512], as vt_decoder_front launches it (train_cross.hip's forward runs the same
// launches: same bits); feat holds x on entry (or is x) and ends as the feature rows; cq / cqp / co keep q, q_proj(q) and the attention output
hipError_t vt_dec_cross(const DecoderWeights& w, const float* x, int B, float* cq, float* cqp, float* co, float* cat, float* feat, hipStream_t s);
// vt_decoder_forward = front (latent -> feature rows [B][dims[0]]) + head (feature rows -> logits)
hipError_t vt_decoder_front(const DecoderWeights& w, const float* latent_nchw, int B, int H, int W, float* ws, float* feat, hipStream_t s);
hipError_t vt_decoder_head(const DecHeadShape& h, const DecHeadParams& p, const float* feat, int B, float* hbuf, float* logits, hipStream_t s);
hipError_t vt_decoder_forward(const DecoderWeights& w, const float* latent_nchw, int B, int H, int W, float* ws,
                              float* logits, hipStream_t s);
size_t vt_decoder_workspace_floats(int B, int C, int H, int W);
hipError_t vt_decoder_sort(const float* logits, int B, int N, float* conf, long long* idx, hipStream_t s);
hipError_t vt_decoder_summary(const float* conf, const long long* idx, int B, int N, float threshold, int K, float* top_conf,
                              int* top_idx, float* stats, hipStream_t s);
// the summary under one threshold per class (device class_thresholds [N]): the passing pairs are compacted in sorted order
hipError_t vt_decoder_summary_per_class(const float* conf, const long long* idx, int B, int N, const float* class_thresholds, int K,
                                        float* top_conf, int* top_idx, float* stats, hipStream_t s);
