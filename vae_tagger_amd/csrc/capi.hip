// C ABI (include/vae_tagger_hip.h): context life cycle, weight upload, flags, status word, the decoder / evaluator / preprocess /
// resize entry points, diagnostics and the profiler read-out.  The encoder lives in weights.hip (packing), encoder.hip and
// attention.hip (launch schedule); the single-layer entry points in ops.hip and ops_backward.hip.
// No torch types, no host synchronisation inside hot-path calls, caller-owned buffers.
#include <math.h>
#include <string.h>

#include "vt_context.h"
#include "vt_eval.h"

using namespace vt;

namespace {
// diagnostics: sum of the 32-bit words of a buffer (integer adds commute: the same bytes give the same sum whatever the thread order)
__global__ void dbg_checksum_kernel(const unsigned int* __restrict__ p, long long n, unsigned long long* __restrict__ out) {
    unsigned long long acc = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) acc += (unsigned long long)p[i] * (unsigned long long)(i % 1021 + 1);
    atomicAdd(out, acc);
}
constexpr int DBG_SLOTS = 256;
}  // namespace

void vt::dbg_sum(vt_context* c, const void* p, size_t bytes, hipStream_t s) {
    if (!c->dbg_on || !c->dbg || c->dbg_n >= DBG_SLOTS) return;
    hipLaunchKernelGGL(dbg_checksum_kernel, dim3(64), dim3(256), 0, s, (const unsigned int*)p, (long long)(bytes / 4), c->dbg + c->dbg_n);
    ++c->dbg_n;
}

// ===================================================================================================
extern "C" {

const char* vt_version(void) { return "vae_tagger_hip 0.1.0 (gfx950)"; }

int vt_create(int device, vt_context** out) {
    if (!out) return VT_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return VT_ERR_HIP;
    vt_context* c = new vt_context();
    c->device = device;
    DeviceGuard guard(c);
    // one zeroed page: DMA source of padded / out-of-image lanes; its last word is the sticky status word
    if (hipMalloc(&c->zeros, 4096 + 256) != hipSuccess || hipMemset(c->zeros, 0, 4096 + 256) != hipSuccess) { delete c; return VT_ERR_HIP; }
    c->status = (int*)((char*)c->zeros + 4096);
    *out = c;
    return VT_OK;
}

void vt_destroy(vt_context* c) {
    if (c && c->dbg) { DeviceGuard guard(c); (void)hipFree(c->dbg); c->dbg = nullptr; }
    if (!c) return;
    {
        DeviceGuard guard(c);
        for (hipEvent_t e : c->event_pool) (void)hipEventDestroy(e);
        if (c->op_scratch) (void)hipFree(c->op_scratch);
        if (c->rs_host) (void)hipHostFree(c->rs_host);
        if (c->rs_event) (void)hipEventDestroy(c->rs_event);
        for (auto& sl : c->rs_ring) { if (sl.host) (void)hipHostFree(sl.host); if (sl.ev) (void)hipEventDestroy(sl.ev); }
        c->free_allocs(c->enc_allocs);
        c->free_allocs(c->dec_allocs);
        c->free_allocs(c->imgdec_allocs);
        if (c->zeros) (void)hipFree(c->zeros);
    }
    delete c;
}

const char* vt_last_error(const vt_context* c) { return c ? c->err.c_str() : "null context"; }

int vt_set_weight(vt_context* c, const char* name, const void* data, int dtype, const int64_t* shape, int ndim) {
    if (!c || !name || !data || ndim < 0 || ndim > 8 || (ndim && !shape)) return c ? c->fail(VT_ERR_INVALID, "vt_set_weight: bad argument") : VT_ERR_INVALID;
    HostTensor t;
    t.shape.assign(shape, shape + ndim);
    const int64_t n = t.numel();
    if (n < 0 || n > (1LL << 31)) return c->fail(VT_ERR_INVALID, "vt_set_weight: bad shape for %s", name);
    t.v.resize((size_t)n);
    if (dtype == VT_F32) memcpy(t.v.data(), data, (size_t)n * 4);
    else if (dtype == VT_BF16) for (int64_t i = 0; i < n; ++i) t.v[i] = bf2f(((const uint16_t*)data)[i]);
    else if (dtype == VT_F16) for (int64_t i = 0; i < n; ++i) t.v[i] = h2f(((const uint16_t*)data)[i]);
    else return c->fail(VT_ERR_INVALID, "vt_set_weight: unknown dtype %d", dtype);
    c->weights[name] = std::move(t);
    return VT_OK;
}

// ---- decoder --------------------------------------------------------------------------------------
int vt_decoder_configure(vt_context* c, int num_classes, int latent_channels, int plain, int use_spatial,
                         int use_self, int use_cross, int heads) {
    if (!c) return VT_ERR_INVALID;
    if (num_classes < 1 || latent_channels != 16 || heads < 1) return c->fail(VT_ERR_INVALID, "bad decoder configuration (latent_channels must be 16)");
    if (!plain && use_self && (8 % heads)) return c->fail(VT_ERR_INVALID, "attention_heads must divide 8");
    if (!plain && use_cross && (256 % heads)) return c->fail(VT_ERR_INVALID, "attention_heads must divide 256");
    { DeviceGuard guard(c); c->free_allocs(c->dec_allocs); }
    c->dec = DecoderWeights();
    c->dec.num_classes = num_classes; c->dec.latent_channels = latent_channels; c->dec.plain = plain;
    c->dec.use_spatial = use_spatial; c->dec.use_self = use_self; c->dec.use_cross = use_cross; c->dec.heads = heads;
    c->dec_configured = true; c->dec_finalized = false;
    return VT_OK;
}

static int dec_get(vt_context* c, const char* name, int64_t numel, const float** out) {
    const HostTensor* t = c->find(name);
    if (!t) return c->fail(VT_ERR_MISSING_WEIGHT, "missing weight %s", name);
    if (t->numel() != numel) return c->fail(VT_ERR_INVALID, "shape mismatch for %s (%lld elements, expected %lld)", name, (long long)t->numel(), (long long)numel);
    *out = (const float*)c->upload(t->v.data(), (size_t)numel * 4);
    if (!*out) return c->fail(VT_ERR_HIP, "upload failed for %s", name);
    return VT_OK;
}

int vt_decoder_finalize(vt_context* c) {
    if (!c) return VT_ERR_INVALID;
    if (!c->dec_configured) return c->fail(VT_ERR_STATE, "vt_decoder_configure was not called");
    DeviceGuard guard(c);
    c->dec_finalized = false;                      // (see vt_encoder_finalize: a failed re-finalize leaves "not finalized", no dangling pointers)
    {
        DecoderWeights fresh;
        const DecoderWeights& o = c->dec;
        fresh.num_classes = o.num_classes; fresh.latent_channels = o.latent_channels; fresh.heads = o.heads; fresh.plain = o.plain;
        fresh.use_spatial = o.use_spatial; fresh.use_self = o.use_self; fresh.use_cross = o.use_cross;
        c->dec = fresh;
    }
    c->free_allocs(c->dec_allocs);
    c->cur_allocs = &c->dec_allocs;
    DecoderWeights& d = c->dec;
    const int C = d.latent_channels, N = d.num_classes;
    int r;
#define G(name, n, ptr) if ((r = dec_get(c, name, n, ptr))) return r
    if (d.plain) {
        const int dims[3] = {C * 16, 512, 256};
        for (int i = 0; i < 2; ++i) {
            char k[64];
            snprintf(k, sizeof k, "classifier.%d.weight", 4 * i); G(k, (int64_t)dims[i + 1] * dims[i], &d.cls_w[i]);
            snprintf(k, sizeof k, "classifier.%d.bias", 4 * i); G(k, dims[i + 1], &d.cls_b[i]);
            snprintf(k, sizeof k, "classifier.%d.weight", 4 * i + 1); G(k, dims[i + 1], &d.cls_ln_w[i]);
            snprintf(k, sizeof k, "classifier.%d.bias", 4 * i + 1); G(k, dims[i + 1], &d.cls_ln_b[i]);
        }
        G("classifier.8.weight", (int64_t)N * 256, &d.cls_w[2]);
        G("classifier.8.bias", N, &d.cls_b[2]);
    } else {
        const int H = C / 2;
        if (d.use_spatial) {
            d.ca_hidden = C / 8;
            G("spatial_attention.channel_att.0.weight", (int64_t)d.ca_hidden * C, &d.ca_w0);
            G("spatial_attention.channel_att.2.weight", (int64_t)C * d.ca_hidden, &d.ca_w2);
            G("spatial_attention.spatial_att.0.weight", 98, &d.sa_w);
        }
        G("feature_compress.0.weight", (int64_t)H * C * 9, &d.fc_w);
        G("feature_compress.0.bias", H, &d.fc_b);
        {   // fold eval-mode BatchNorm2d (running stats, eps 1e-5): y = x*scale + shift
            const HostTensor *g = c->find("feature_compress.1.weight"), *b = c->find("feature_compress.1.bias");
            const HostTensor *m = c->find("feature_compress.1.running_mean"), *v = c->find("feature_compress.1.running_var");
            if (!g || !b || !m || !v) return c->fail(VT_ERR_MISSING_WEIGHT, "missing weight feature_compress.1.*");
            if (g->numel() != H || b->numel() != H || m->numel() != H || v->numel() != H) return c->fail(VT_ERR_INVALID, "shape mismatch for feature_compress.1");
            std::vector<float> sc(H), sh(H);
            for (int i = 0; i < H; ++i) {
                const float inv = 1.0f / sqrtf(v->v[i] + 1e-5f);
                sc[i] = g->v[i] * inv;
                sh[i] = b->v[i] - m->v[i] * sc[i];
            }
            d.bn_scale = (const float*)c->upload(sc.data(), H * 4);
            d.bn_shift = (const float*)c->upload(sh.data(), H * 4);
            d.bn_w = (const float*)c->upload(g->v.data(), H * 4);
            d.bn_b = (const float*)c->upload(b->v.data(), H * 4);
            d.bn_mean = (const float*)c->upload(m->v.data(), H * 4);
            d.bn_var = (const float*)c->upload(v->v.data(), H * 4);
            if (!d.bn_scale || !d.bn_shift || !d.bn_w || !d.bn_b || !d.bn_mean || !d.bn_var) return c->fail(VT_ERR_HIP, "upload failed for batch norm");
        }
        if (d.use_self) {
            const char* p = "self_attention_post.";
            std::string s(p);
            G((s + "norm.weight").c_str(), H, &d.sa.ln_w); G((s + "norm.bias").c_str(), H, &d.sa.ln_b);
            G((s + "q_proj.weight").c_str(), H * H, &d.sa.q_w); G((s + "q_proj.bias").c_str(), H, &d.sa.q_b);
            G((s + "k_proj.weight").c_str(), H * H, &d.sa.k_w); G((s + "k_proj.bias").c_str(), H, &d.sa.k_b);
            G((s + "v_proj.weight").c_str(), H * H, &d.sa.v_w); G((s + "v_proj.bias").c_str(), H, &d.sa.v_b);
            G((s + "out_proj.weight").c_str(), H * H, &d.sa.o_w); G((s + "out_proj.bias").c_str(), H, &d.sa.o_b);
        }
        if (d.use_cross) {
            G("query_generator.weight", (int64_t)512 * H * 64, &d.qg_w); G("query_generator.bias", 512, &d.qg_b);
            G("cross_attention.q_proj.weight", 256 * 512, &d.cx_q_w); G("cross_attention.q_proj.bias", 256, &d.cx_q_b);
            G("cross_attention.k_proj.weight", 256 * H, &d.cx_k_w); G("cross_attention.k_proj.bias", 256, &d.cx_k_b);
            G("cross_attention.v_proj.weight", 256 * H, &d.cx_v_w); G("cross_attention.v_proj.bias", 256, &d.cx_v_b);
            G("cross_attention.out_proj.weight", 512 * 256, &d.cx_o_w); G("cross_attention.out_proj.bias", 512, &d.cx_o_b);
        }
        const int dims[4] = {H * 64, 1024, 512, 256};
        for (int i = 0; i < 3; ++i) {
            char k[64];
            snprintf(k, sizeof k, "classifier.%d.weight", 4 * i); G(k, (int64_t)dims[i + 1] * dims[i], &d.cls_w[i]);
            snprintf(k, sizeof k, "classifier.%d.bias", 4 * i); G(k, dims[i + 1], &d.cls_b[i]);
            snprintf(k, sizeof k, "classifier.%d.weight", 4 * i + 1); G(k, dims[i + 1], &d.cls_ln_w[i]);
            snprintf(k, sizeof k, "classifier.%d.bias", 4 * i + 1); G(k, dims[i + 1], &d.cls_ln_b[i]);
        }
        G("classifier.12.weight", (int64_t)N * 256, &d.cls_w[3]);
        G("classifier.12.bias", N, &d.cls_b[3]);
    }
#undef G
    for (auto it = c->weights.begin(); it != c->weights.end();)
        it = (it->first.compare(0, 8, "encoder.") != 0 && it->first.compare(0, 8, "decoder.") != 0) ? c->weights.erase(it) : ++it;   // (decoder.*: the VAE's image decoder)
    c->dec_finalized = true;
    return VT_OK;
}

size_t vt_decode_workspace_bytes(const vt_context* c, int B, int h, int w) {
    if (!c || !c->dec_configured || B <= 0 || h <= 0 || w <= 0) return 0;
    return align_up(vt_decoder_workspace_floats(B, c->dec.latent_channels, h, w) * 4);
}

int vt_decode_logits(vt_context* c, const float* latent, int B, int h, int w, float* logits, void* ws, size_t ws_bytes,
                     void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (!c->dec_finalized) return c->fail(VT_ERR_STATE, "decoder weights not finalized");
    if (!latent || !logits || !ws || B <= 0 || h <= 0 || w <= 0) return c->fail(VT_ERR_INVALID, "vt_decode_logits: bad argument");
    if (ws_bytes < vt_decode_workspace_bytes(c, B, h, w)) return c->fail(VT_ERR_WORKSPACE, "vt_decode_logits: workspace too small");
    HIPCK(c, vt_decoder_forward(c->dec, latent, B, h, w, (float*)ws, logits, (hipStream_t)stream), "decoder_forward");
    return VT_OK;
}

int vt_get_confidence(vt_context* c, const float* logits, int B, int N, float* conf, int64_t* idx, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (!logits || !conf || !idx || B <= 0 || N <= 0) return c->fail(VT_ERR_INVALID, "vt_get_confidence: bad argument");
    HIPCK(c, vt_decoder_sort(logits, B, N, conf, (long long*)idx, (hipStream_t)stream), "decoder_sort");
    return VT_OK;
}

int vt_summarize_confidence(vt_context* c, const float* conf, const int64_t* idx, int B, int N, float threshold, int K,
                            float* top_conf, int32_t* top_idx, float* stats, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (!conf || !idx || !top_conf || !top_idx || !stats || B <= 0 || N <= 0 || K <= 0) return c->fail(VT_ERR_INVALID, "vt_summarize_confidence: bad argument");
    HIPCK(c, vt_decoder_summary(conf, (const long long*)idx, B, N, threshold, K, top_conf, (int*)top_idx, stats, (hipStream_t)stream), "decoder_summary");
    return VT_OK;
}

int vt_summarize_confidence_per_class(vt_context* c, const float* conf, const int64_t* idx, int B, int N, const float* class_thresholds,
                                      int K, float* top_conf, int32_t* top_idx, float* stats, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (!conf || !idx || !class_thresholds || !top_conf || !top_idx || !stats || B <= 0 || N <= 0 || K <= 0)
        return c->fail(VT_ERR_INVALID, "vt_summarize_confidence_per_class: bad argument");
    HIPCK(c, vt_decoder_summary_per_class(conf, (const long long*)idx, B, N, class_thresholds, K, top_conf, (int*)top_idx, stats,
                                          (hipStream_t)stream), "decoder_summary_per_class");
    return VT_OK;
}

int vt_status(vt_context* c, int clear, int* status_out, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (!status_out) return c->fail(VT_ERR_INVALID, "vt_status: null output");
    hipStream_t s = (hipStream_t)stream;
    int v = 0;
    // the copy targets a stack slot: nothing may return while it is in flight, so synchronise before looking at any later error
    HIPCK(c, hipMemcpyAsync(&v, c->status, sizeof(int), hipMemcpyDeviceToHost, s), "vt_status copy");
    const hipError_t ec = clear ? hipMemsetAsync(c->status, 0, sizeof(int), s) : hipSuccess;
    HIPCK(c, hipStreamSynchronize(s), "vt_status sync");
    HIPCK(c, ec, "vt_status clear");
    *status_out = v;
    return VT_OK;
}

int vt_status_async(vt_context* c, int clear, int* status_out, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (!status_out) return c->fail(VT_ERR_INVALID, "vt_status_async: null output");
    hipStream_t s = (hipStream_t)stream;
    HIPCK(c, hipMemcpyAsync(status_out, c->status, sizeof(int), hipMemcpyDefault, s), "vt_status_async copy");
    if (clear) HIPCK(c, hipMemsetAsync(c->status, 0, sizeof(int), s), "vt_status_async clear");
    return VT_OK;
}

// ---- streaming evaluator (eval_metrics.hip).  Every argument is checked on the host before anything is launched or written. ----
// reset / update / grow feed the state; average_precision, read_counts and recount (per-class thresholds, from the keys) read it out;
// export / merge move it between ranks.
namespace {
bool eval_dims_ok(int N, int T, long long capacity) {
    return N > 0 && T > 0 && T <= VT_EVAL_MAX_T && capacity >= 0 && capacity <= VT_EVAL_MAX_N_SEEN &&
           (capacity == 0 || (unsigned long long)N * (unsigned long long)capacity < (1ull << 40));
}
bool misaligned(const void* p) { return ((uintptr_t)p & (ALIGN - 1)) != 0; }
int eval_check_state(vt_context* c, const char* who, const void* state, size_t state_bytes, int N, int T, long long capacity) {
    if (!eval_dims_ok(N, T, capacity)) return c->fail(VT_ERR_INVALID, "%s: bad dimensions (N = %d, T = %d of at most %d, capacity = %lld)", who, N, T, VT_EVAL_MAX_T, capacity);
    if (!state || misaligned(state)) return c->fail(VT_ERR_INVALID, "%s: state is null or not 256-B aligned", who);
    const size_t need = vt_eval_layout(N, T, capacity).total;
    if (state_bytes < need) return c->fail(VT_ERR_WORKSPACE, "%s: state holds %zu bytes, %zu needed", who, state_bytes, need);
    return VT_OK;
}
}  // namespace

size_t vt_eval_state_bytes(int N, int T, long long capacity) {
    return eval_dims_ok(N, T, capacity) ? vt_eval_layout(N, T, capacity).total : 0;
}

int vt_eval_reset(vt_context* c, void* state, size_t state_bytes, int N, int T, const double* thresholds, int t_main, long long capacity,
                  void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (int r = eval_check_state(c, "vt_eval_reset", state, state_bytes, N, T, capacity)) return r;
    if (!thresholds || t_main < 0 || t_main >= T) return c->fail(VT_ERR_INVALID, "vt_eval_reset: null thresholds or t_main = %d outside [0, %d)", t_main, T);
    EvalThresholds th;
    for (int i = 0; i < VT_EVAL_MAX_T; ++i) th.v[i] = i < T ? thresholds[i] : INFINITY;
    HIPCK(c, vt_eval_launch_reset(state, vt_eval_layout(N, T, capacity), th, (hipStream_t)stream), "eval_reset");
    return VT_OK;
}

int vt_eval_update(vt_context* c, void* state, size_t state_bytes, int N, int T, int t_main, long long capacity, const float* probs,
                   const void* labels, int labels_dtype, int B, long long n_seen, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (int r = eval_check_state(c, "vt_eval_update", state, state_bytes, N, T, capacity)) return r;
    if (t_main < 0 || t_main >= T) return c->fail(VT_ERR_INVALID, "vt_eval_update: t_main = %d outside [0, %d)", t_main, T);
    if (!probs || !labels || (labels_dtype != VT_F32 && labels_dtype != VT_U8)) return c->fail(VT_ERR_INVALID, "vt_eval_update: null input or labels neither VT_F32 nor VT_U8");
    if (B <= 0 || B > VT_EVAL_MAX_B || n_seen < 0 || n_seen + B > VT_EVAL_MAX_N_SEEN)
        return c->fail(VT_ERR_INVALID, "vt_eval_update: B = %d outside [1, %d] or n_seen = %lld out of range", B, VT_EVAL_MAX_B, n_seen);
    if (capacity > 0 && n_seen + B > capacity) return c->fail(VT_ERR_INVALID, "vt_eval_update: n_seen + B = %lld exceeds the capacity %lld", n_seen + B, capacity);
    HIPCK(c, vt_eval_launch_update(state, vt_eval_layout(N, T, capacity), probs, labels, labels_dtype == VT_U8, B, N, T, t_main, capacity, n_seen,
                                   (hipStream_t)stream), "eval_update");
    return VT_OK;
}

int vt_eval_grow(vt_context* c, const void* old_state, size_t old_bytes, long long old_capacity, void* new_state, size_t new_bytes,
                 long long new_capacity, int N, int T, long long n_seen, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (int r = eval_check_state(c, "vt_eval_grow (old)", old_state, old_bytes, N, T, old_capacity)) return r;
    if (int r = eval_check_state(c, "vt_eval_grow (new)", new_state, new_bytes, N, T, new_capacity)) return r;
    if (old_capacity <= 0 || new_capacity < old_capacity || n_seen < 0 || n_seen > old_capacity || old_state == new_state)
        return c->fail(VT_ERR_INVALID, "vt_eval_grow: capacities %lld -> %lld with n_seen = %lld", old_capacity, new_capacity, n_seen);
    const EvalLayout lo = vt_eval_layout(N, T, old_capacity), ln = vt_eval_layout(N, T, new_capacity);
    hipStream_t s = (hipStream_t)stream;
    HIPCK(c, hipMemcpyAsync(new_state, old_state, lo.head_bytes, hipMemcpyDeviceToDevice, s), "eval_grow head");
    if (n_seen > 0)
        HIPCK(c, hipMemcpy2DAsync((char*)new_state + ln.keys, (size_t)new_capacity * 8, (const char*)old_state + lo.keys, (size_t)old_capacity * 8,
                                  (size_t)n_seen * 8, (size_t)N, hipMemcpyDeviceToDevice, s), "eval_grow keys");
    return VT_OK;
}

size_t vt_eval_ap_workspace_bytes(int N, long long n_seen) {
    if (N <= 0 || n_seen <= 0 || (unsigned long long)N * (unsigned long long)n_seen > (unsigned long long)VT_EVAL_MICRO_LIMIT) return 0;
    return vt_eval_align((size_t)N * (size_t)n_seen * 8);
}

int vt_eval_average_precision(vt_context* c, void* state, size_t state_bytes, int N, int T, long long capacity, long long n_seen,
                              double* ap_out, size_t ap_bytes, double* micro_ap_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (int r = eval_check_state(c, "vt_eval_average_precision", state, state_bytes, N, T, capacity)) return r;
    if (capacity <= 0) return c->fail(VT_ERR_STATE, "vt_eval_average_precision: the state keeps no keys (capacity 0)");
    if (n_seen <= 0 || n_seen > capacity) return c->fail(VT_ERR_INVALID, "vt_eval_average_precision: n_seen = %lld outside [1, capacity = %lld]", n_seen, capacity);
    if (!ap_out || ((uintptr_t)ap_out & 7)) return c->fail(VT_ERR_INVALID, "vt_eval_average_precision: ap_out is null or misaligned");
    if (ap_bytes < (size_t)N * 8) return c->fail(VT_ERR_WORKSPACE, "vt_eval_average_precision: ap_out holds %zu bytes, %zu needed", ap_bytes, (size_t)N * 8);
    if (micro_ap_out) {
        const size_t need = vt_eval_ap_workspace_bytes(N, n_seen);
        if (need == 0) return c->fail(VT_ERR_INVALID, "vt_eval_average_precision: micro AP runs on the device while n_seen * N < 2^31");
        if ((uintptr_t)micro_ap_out & 7) return c->fail(VT_ERR_INVALID, "vt_eval_average_precision: micro_ap_out is misaligned");
        if (!workspace || misaligned(workspace)) return c->fail(VT_ERR_INVALID, "vt_eval_average_precision: workspace is null or not 256-B aligned");
        if (workspace_bytes < need) return c->fail(VT_ERR_WORKSPACE, "vt_eval_average_precision: workspace holds %zu bytes, %zu needed", workspace_bytes, need);
    }
    HIPCK(c, vt_eval_launch_ap(state, vt_eval_layout(N, T, capacity), N, capacity, n_seen, ap_out, micro_ap_out, (unsigned long long*)workspace,
                               (hipStream_t)stream), "eval_average_precision");
    return VT_OK;
}

int vt_eval_read_counts(vt_context* c, const void* state, size_t state_bytes, int N, int T, long long capacity, uint32_t* counts_out,
                        size_t counts_bytes, uint32_t* support_out, size_t support_bytes, uint64_t* row_stats_out, size_t row_stats_bytes,
                        void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (int r = eval_check_state(c, "vt_eval_read_counts", state, state_bytes, N, T, capacity)) return r;
    if (!counts_out || !support_out || !row_stats_out) return c->fail(VT_ERR_INVALID, "vt_eval_read_counts: null output");
    const size_t nc = (size_t)N * T * 2 * 4, ns = (size_t)N * 4, nr = 3 * 8;
    if (counts_bytes < nc || support_bytes < ns || row_stats_bytes < nr)
        return c->fail(VT_ERR_WORKSPACE, "vt_eval_read_counts: outputs hold %zu / %zu / %zu bytes, %zu / %zu / %zu needed", counts_bytes, support_bytes,
                       row_stats_bytes, nc, ns, nr);
    const EvalLayout l = vt_eval_layout(N, T, capacity);
    hipStream_t s = (hipStream_t)stream;
    const char* st = (const char*)state;
    HIPCK(c, hipMemcpyAsync(counts_out, st + l.counts, nc, hipMemcpyDefault, s), "eval_read counts");
    HIPCK(c, hipMemcpyAsync(support_out, st + l.support, ns, hipMemcpyDefault, s), "eval_read support");
    HIPCK(c, hipMemcpyAsync(row_stats_out, st + l.row_stats, nr, hipMemcpyDefault, s), "eval_read row_stats");
    return VT_OK;
}

size_t vt_eval_recount_workspace_bytes(int N, long long n_seen) {
    if (N <= 0 || n_seen < 0 || n_seen > VT_EVAL_MAX_N_SEEN) return 0;
    return vt_eval_recount_ws_bytes(N, n_seen);
}

int vt_eval_recount(vt_context* c, const void* state, size_t state_bytes, int N, int T, long long capacity, long long n_seen,
                    const double* class_thresholds, uint32_t* counts_out, size_t counts_bytes, uint64_t* row_stats_out,
                    size_t row_stats_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (int r = eval_check_state(c, "vt_eval_recount", state, state_bytes, N, T, capacity)) return r;
    if (n_seen < 0 || n_seen > VT_EVAL_MAX_N_SEEN || n_seen > capacity)
        return c->fail(VT_ERR_INVALID, "vt_eval_recount: n_seen = %lld outside [0, capacity = %lld]%s", n_seen, capacity,
                       capacity == 0 ? " (the state keeps no keys)" : "");
    if (!class_thresholds || ((uintptr_t)class_thresholds & 7)) return c->fail(VT_ERR_INVALID, "vt_eval_recount: class_thresholds is null or misaligned");
    if (!counts_out || ((uintptr_t)counts_out & 3) || !row_stats_out || ((uintptr_t)row_stats_out & 7))
        return c->fail(VT_ERR_INVALID, "vt_eval_recount: an output is null or misaligned");
    if (!workspace || misaligned(workspace)) return c->fail(VT_ERR_INVALID, "vt_eval_recount: workspace is null or not 256-B aligned");
    const size_t nc = (size_t)N * 2 * 4, nr = 3 * 8, need = vt_eval_recount_ws_bytes(N, n_seen);
    if (counts_bytes < nc || row_stats_bytes < nr)
        return c->fail(VT_ERR_WORKSPACE, "vt_eval_recount: outputs hold %zu / %zu bytes, %zu / %zu needed", counts_bytes, row_stats_bytes, nc, nr);
    if (workspace_bytes < need) return c->fail(VT_ERR_WORKSPACE, "vt_eval_recount: workspace holds %zu bytes, %zu needed", workspace_bytes, need);
    HIPCK(c, vt_eval_launch_recount(state, vt_eval_layout(N, T, capacity), N, capacity, n_seen, class_thresholds, counts_out,
                                    (unsigned long long*)row_stats_out, workspace, (hipStream_t)stream), "eval_recount");
    return VT_OK;
}

// ---- state blocks as a wire format: export at a common capacity, merge on one device -----------------------------------------------
namespace {
bool blocks_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}
}  // namespace

int vt_eval_export(vt_context* c, const void* state, size_t state_bytes, int N, int T, long long capacity, long long n_seen, void* out_state,
                   size_t out_bytes, long long out_capacity, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (int r = eval_check_state(c, "vt_eval_export (state)", state, state_bytes, N, T, capacity)) return r;
    if (int r = eval_check_state(c, "vt_eval_export (out)", out_state, out_bytes, N, T, out_capacity)) return r;
    if (n_seen < 0 || n_seen > VT_EVAL_MAX_N_SEEN || (capacity > 0 && n_seen > capacity))
        return c->fail(VT_ERR_INVALID, "vt_eval_export: n_seen = %lld outside [0, capacity = %lld]", n_seen, capacity);
    if (out_capacity != 0 && out_capacity < n_seen)
        return c->fail(VT_ERR_INVALID, "vt_eval_export: out_capacity = %lld is neither 0 nor >= n_seen = %lld", out_capacity, n_seen);
    if (out_capacity > 0 && capacity == 0 && n_seen > 0)
        return c->fail(VT_ERR_INVALID, "vt_eval_export: the state keeps no keys (capacity 0) but out_capacity = %lld", out_capacity);
    const EvalLayout l = vt_eval_layout(N, T, capacity), lo = vt_eval_layout(N, T, out_capacity);
    if (blocks_overlap(state, l.total, out_state, lo.total)) return c->fail(VT_ERR_INVALID, "vt_eval_export: out_state overlaps the state");
    HIPCK(c, vt_eval_launch_export(state, l, out_state, lo, N, capacity, n_seen, out_capacity, c->eval_merge_vec, (hipStream_t)stream), "eval_export");
    return VT_OK;
}

int vt_eval_merge(vt_context* c, void* dst, size_t dst_bytes, int N, int T, long long dst_capacity, long long dst_n_seen,
                  const vt_eval_source* sources, int W, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (int r = eval_check_state(c, "vt_eval_merge (dst)", dst, dst_bytes, N, T, dst_capacity)) return r;
    if (!sources || W < 1 || W > VT_EVAL_MAX_MERGE) return c->fail(VT_ERR_INVALID, "vt_eval_merge: null sources or W = %d outside [1, %d]", W, VT_EVAL_MAX_MERGE);
    if (dst_n_seen < 0 || dst_n_seen > VT_EVAL_MAX_N_SEEN || (dst_capacity > 0 && dst_n_seen > dst_capacity))
        return c->fail(VT_ERR_INVALID, "vt_eval_merge: dst_n_seen = %lld outside [0, capacity = %lld]", dst_n_seen, dst_capacity);
    const EvalLayout l = vt_eval_layout(N, T, dst_capacity);
    EvalMergeArg a;
    a.W = W;
    long long total = dst_n_seen;
    for (int w = 0; w < W; ++w) {
        const vt_eval_source& s = sources[w];
        if (int r = eval_check_state(c, "vt_eval_merge (source)", s.state, s.state_bytes, N, T, s.capacity)) return r;
        if (s.n_seen < 0 || s.n_seen > VT_EVAL_MAX_N_SEEN || (s.capacity > 0 && s.n_seen > s.capacity))
            return c->fail(VT_ERR_INVALID, "vt_eval_merge: source %d has n_seen = %lld outside [0, capacity = %lld]", w, s.n_seen, s.capacity);
        if (blocks_overlap(dst, l.total, s.state, vt_eval_layout(N, T, s.capacity).total))
            return c->fail(VT_ERR_INVALID, "vt_eval_merge: source %d is dst or overlaps it", w);
        if (dst_capacity > 0 && s.capacity == 0 && s.n_seen > 0)
            return c->fail(VT_ERR_INVALID, "vt_eval_merge: source %d keeps no keys (capacity 0) for its %lld samples, dst does", w, s.n_seen);
        a.src[w] = EvalMergeSrc{(const char*)s.state, s.capacity, s.n_seen, s.n_seen, total};
        total += s.n_seen;
        if (total > VT_EVAL_MAX_N_SEEN) return c->fail(VT_ERR_INVALID, "vt_eval_merge: %lld samples in all, 2^31 or more", total);
    }
    if (dst_capacity > 0 && total > dst_capacity)
        return c->fail(VT_ERR_INVALID, "vt_eval_merge: dst_n_seen + the sources' samples = %lld exceeds the capacity %lld", total, dst_capacity);
    HIPCK(c, vt_eval_launch_merge(dst, l, N, dst_capacity, a, c->eval_merge_vec, (hipStream_t)stream), "eval_merge");
    return VT_OK;
}

int vt_set_flag(vt_context* c, int flag, int value) {
    if (!c) return VT_ERR_INVALID;
    if (flag == 0) { c->use_halo_conv = value != 0; return VT_OK; }
    if (flag == 1) { c->fuse_gn_stats = value != 0; return VT_OK; }
    if (flag == 2) { c->fuse_gn_apply = value != 0; return VT_OK; }
    if (flag == 3) { c->halo_occ2 = value < 0 ? 0 : (value > 4 ? 4 : value); return VT_OK; }
    if (flag == 4) { c->res_fp16 = value != 0; return VT_OK; }
    if (flag == 5) { c->conv_in_mfma = value != 0; return VT_OK; }
    if (flag == 6) { c->gemm_short = value != 0; return VT_OK; }
    if (flag == 8) { c->fuse_shortcut = value != 0; return VT_OK; }
    if (flag == 9) { c->attn_qk_kernel = value != 0; return VT_OK; }
    if (flag == 10) { c->pv_stream = value != 0; return VT_OK; }
    if (flag == 11) { c->fp8 = value != 0; return VT_OK; }
    if (flag == 16) { if ((value & 3) == 3 || value < 0 || value > 7) return c->fail(VT_ERR_INVALID, "vt_set_flag(16): tile shape 0..2 (+4: every layer)"); c->fp8_tile = value; return VT_OK; }
    if (flag == 12) { c->attn_pv_kernel = value != 0; return VT_OK; }
    if (flag == 17) { c->attn_proj_kernel = value != 0; return VT_OK; }
    if (flag == 18) { c->f16_ops = value != 0; return VT_OK; }
    if (flag == 19) { c->s2_planar = value != 0; return VT_OK; }
    if (flag == 21) { c->eval_merge_vec = value != 0; return VT_OK; }
    if (flag == 20) { c->conv_out_halo = value != 0; return VT_OK; }
    if (flag == 22) { c->up2_literal = value != 0; return VT_OK; }
    if (flag == 23) { c->s2_dgrad_literal = value != 0; return VT_OK; }
    if (flag == 13) { c->s2_halo = value != 0; return VT_OK; }
    if (flag == 14) { c->attn_fp8 = value != 0; return VT_OK; }
    if (flag == 15) { c->proj_fp8 = value != 0; return VT_OK; }
    if (flag == 7) {
        if (value < 0 || value > 2) return c->fail(VT_ERR_INVALID, "vt_set_flag(7): value %d not in 0..2", value);
        c->attn_mode = value;
        return VT_OK;
    }
    return c->fail(VT_ERR_INVALID, "vt_set_flag: unknown flag %d", flag);
}

int vt_profile_num_configs(void) { return VT_NUM_PROF_SLOTS; }

int vt_preprocess_u8(vt_context* c, const uint8_t* in_hwc, int B, int H, int W, float* out_nchw, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    HIPCK(c, vt_launch_preprocess_u8(in_hwc, out_nchw, B, H, W, (hipStream_t)stream), "vt_preprocess_u8");
    return VT_OK;
}

// ---- device-side resize (Pillow's ImagingResample, 8 bits per channel) ---------------------------
namespace {
constexpr int RS_BITS = 32 - 8 - 2;
double rs_filter(int kind, double x) {
    if (kind == 0) {                                   // bilinear_filter, support 1
        if (x < 0.0) x = -x;
        return x < 1.0 ? 1.0 - x : 0.0;
    }
    if (-3.0 <= x && x < 3.0) {                        // lanczos_filter, support 3 (truncated sinc)
        auto sinc = [](double v) { if (v == 0.0) return 1.0; v *= M_PI; return sin(v) / v; };
        return sinc(x) * sinc(x / 3);
    }
    return 0.0;
}
}  // namespace
extern "C++" {
namespace vt {
int rs_ksize(int in_size, int out_size, int kind) {
    double fs = (double)in_size / out_size;
    if (fs < 1.0) fs = 1.0;
    return (int)ceil((kind == 0 ? 1.0 : 3.0) * fs) * 2 + 1;
}
// Pillow's precompute_coeffs + normalize_coeffs_8bpc for box (0, in_size): tab[xx] = (first, count, coefficients[ksize])
void rs_table(int in_size, int out_size, int kind, int* tab) {
    const double scale = (double)in_size / out_size;
    double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = (kind == 0 ? 1.0 : 3.0) * filterscale, ss = 1.0 / filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    std::vector<double> w(ksize);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) { w[x] = rs_filter(kind, (x + xmin - center + 0.5) * ss); ww += w[x]; }
        int* t = tab + (size_t)xx * (2 + ksize);
        t[0] = xmin; t[1] = xmax;
        for (int x = 0; x < ksize; ++x) {
            double v = x < xmax ? w[x] : 0.0;
            if (x < xmax && ww != 0.0) v /= ww;
            t[2 + x] = v < 0 ? (int)(-0.5 + v * (1 << RS_BITS)) : (int)(0.5 + v * (1 << RS_BITS));
        }
    }
}
}  // namespace vt
}  // extern "C++"
namespace {
struct RsPlan { int kh, kv; size_t tab_h, tab_v, tmp, total; };   // table sizes in ints, tmp / total in bytes
RsPlan rs_plan(int crop_h, int crop_w, int dst_h, int dst_w, int kind) {
    RsPlan p{};
    const bool nh = dst_w != crop_w, nv = dst_h != crop_h;
    p.kh = nh ? rs_ksize(crop_w, dst_w, kind) : 0;
    p.kv = nv ? rs_ksize(crop_h, dst_h, kind) : 0;
    p.tab_h = nh ? (size_t)dst_w * (2 + p.kh) : 0;
    p.tab_v = nv ? (size_t)dst_h * (2 + p.kv) : 0;
    p.tmp = (nh && nv) ? (size_t)crop_h * dst_w * 3 : ((nv && !nh) ? (size_t)crop_h * crop_w * 3 : 0);
    p.total = align_up((p.tab_h + p.tab_v) * 4) + align_up(p.tmp);
    return p;
}
}  // namespace

int vt_resize_table(int in_size, int out_size, int filter, int* table_out, int table_ints) {
    if (in_size <= 0 || out_size <= 0 || (filter != 0 && filter != 1)) return -1;
    const int ks = rs_ksize(in_size, out_size, filter);
    if (!table_out) return ks;
    if ((long long)table_ints < (long long)out_size * (2 + ks)) return -1;
    rs_table(in_size, out_size, filter, table_out);
    return ks;
}

size_t vt_resize_workspace_bytes(int crop_h, int crop_w, int dst_h, int dst_w, int filter) {
    if (crop_h <= 0 || crop_w <= 0 || dst_h <= 0 || dst_w <= 0 || (filter != 0 && filter != 1)) return 0;
    return rs_plan(crop_h, crop_w, dst_h, dst_w, filter).total + 256;
}

int vt_resize_u8(vt_context* c, const uint8_t* src_hwc, int src_h, int src_w, int crop_left, int crop_top, int crop_w, int crop_h,
                 uint8_t* dst_hwc, int dst_h, int dst_w, int filter, void* workspace, size_t workspace_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    if (!src_hwc || !dst_hwc || (filter != 0 && filter != 1) || crop_w <= 0 || crop_h <= 0 || dst_w <= 0 || dst_h <= 0 ||
        crop_left < 0 || crop_top < 0 || crop_left + crop_w > src_w || crop_top + crop_h > src_h)
        return c->fail(VT_ERR_INVALID, "vt_resize_u8: bad argument");
    DeviceGuard guard(c);
    const RsPlan p = rs_plan(crop_h, crop_w, dst_h, dst_w, filter);
    char* ws = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    if (p.total && (!workspace || workspace_bytes < p.total + (size_t)(ws - (char*)workspace)))
        return c->fail(VT_ERR_WORKSPACE, "vt_resize_u8: workspace %zu < required %zu", workspace_bytes, p.total + 256);
    hipStream_t s = (hipStream_t)stream;
    int* tab = (int*)ws;
    const size_t ints = p.tab_h + p.tab_v;
    if (ints) {
        if (!c->rs_event) HIPCK(c, hipEventCreateWithFlags(&c->rs_event, hipEventDisableTiming), "hipEventCreate");
        else HIPCK(c, hipEventSynchronize(c->rs_event), "hipEventSynchronize");     // the previous copy has read the staging buffer
        if (c->rs_host_ints < ints) {
            if (c->rs_host) (void)hipHostFree(c->rs_host);
            c->rs_host = nullptr; c->rs_host_ints = 0;
            HIPCK(c, hipHostMalloc((void**)&c->rs_host, ints * 4, hipHostMallocDefault), "hipHostMalloc");
            c->rs_host_ints = ints;
        }
        if (p.tab_h) rs_table(crop_w, dst_w, filter, c->rs_host);
        if (p.tab_v) rs_table(crop_h, dst_h, filter, c->rs_host + p.tab_h);
        HIPCK(c, hipMemcpyAsync(tab, c->rs_host, ints * 4, hipMemcpyHostToDevice, s), "hipMemcpyAsync(tables)");
        HIPCK(c, hipEventRecord(c->rs_event, s), "hipEventRecord");
    }
    unsigned char* tmp = p.tmp ? (unsigned char*)(ws + align_up(ints * 4)) : nullptr;
    HIPCK(c, vt_launch_resize_u8(src_hwc, src_h, src_w, crop_left, crop_top, crop_w, crop_h, dst_hwc, dst_h, dst_w,
                                 p.tab_h ? tab : nullptr, p.kh, p.tab_v ? tab + p.tab_h : nullptr, p.kv, tmp, s), "vt_resize_u8");
    return VT_OK;
}

// ---- diagnostics --------------------------------------------------------------------------------
int vt_debug_trace(vt_context* c, int enable, unsigned long long* sums_out, int max_sums, int* n_out) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (enable) {
        if (!c->dbg) HIPCK(c, hipMalloc((void**)&c->dbg, DBG_SLOTS * 8), "hipMalloc(debug trace)");
        HIPCK(c, hipMemset(c->dbg, 0, DBG_SLOTS * 8), "hipMemset(debug trace)");
        c->dbg_n = 0; c->dbg_on = true;
        return VT_OK;
    }
    c->dbg_on = false;
    HIPCK(c, hipDeviceSynchronize(), "hipDeviceSynchronize");
    const int n = c->dbg_n < max_sums ? c->dbg_n : max_sums;
    if (sums_out && n > 0) HIPCK(c, hipMemcpy(sums_out, c->dbg, (size_t)n * 8, hipMemcpyDeviceToHost), "hipMemcpy(debug trace)");
    if (n_out) *n_out = n;
    return VT_OK;
}

// ---- profiling ----------------------------------------------------------------------------------
int vt_profile_begin(vt_context* c) {
    if (!c) return VT_ERR_INVALID;
    c->prof.clear(); c->events_used = 0; c->profiling = true;
    return VT_OK;
}

int vt_profile_end(vt_context* c, int max_cfg, long long* launches, double* total_ms, double* total_flops,
                   const char** names) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    c->profiling = false;
    if (max_cfg < VT_NUM_PROF_SLOTS || !launches || !total_ms || !total_flops) return c->fail(VT_ERR_INVALID, "vt_profile_end: need room for %d slots", VT_NUM_PROF_SLOTS);
    for (int i = 0; i < VT_NUM_PROF_SLOTS; ++i) { launches[i] = 0; total_ms[i] = 0; total_flops[i] = 0; if (names) names[i] = vt_conv_gemm_config_name(i); }
    for (auto& r : c->prof) {
        HIPCK(c, hipEventSynchronize(r.e1), "hipEventSynchronize");
        float ms = 0.f;
        HIPCK(c, hipEventElapsedTime(&ms, r.e0, r.e1), "hipEventElapsedTime");
        launches[r.cfg] += 1; total_ms[r.cfg] += ms; total_flops[r.cfg] += r.flops;
    }
    c->prof.clear(); c->events_used = 0;
    return VT_OK;
}

}  // extern "C"
