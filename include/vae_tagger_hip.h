/*
 * vae_tagger_hip.h -- C ABI of libvae_tagger_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the inference hot path of spawner1145/vae-tagger.  The reference has no
 * FFI of its own: the boundary is a Python object protocol.  Each entry
 * point below names the reference call it stands in for; INTEGRATION.md shows the ctypes stub.
 *
 * Conventions
 *   - plain C types only; every buffer is caller-owned DEVICE memory unless marked "host";
 *   - `stream` is a hipStream_t passed as void* (0 = default stream); no call synchronises the host;
 *   - every call returns VT_OK or an error code; vt_last_error(ctx) gives the message; nothing aborts;
 *   - one context per device / thread; no global state: every option of vt_set_flag lives in the context, every call runs on
 *     the context's device and restores the caller's current device before it returns;
 *   - workspace is caller-provided (query the *_workspace_bytes function first), 256-B aligned.
 */
#ifndef VAE_TAGGER_HIP_H
#define VAE_TAGGER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vt_context vt_context;

enum { VT_OK = 0, VT_ERR_INVALID = 1, VT_ERR_HIP = 2, VT_ERR_STATE = 3, VT_ERR_MISSING_WEIGHT = 4,
       VT_ERR_WORKSPACE = 5 };
enum { VT_F32 = 0, VT_BF16 = 1, VT_F16 = 2, VT_U8 = 3 /* evaluator labels only */ };

const char* vt_version(void);
int vt_create(int device, vt_context** out);
void vt_destroy(vt_context* ctx);
const char* vt_last_error(const vt_context* ctx);

/* ---- model construction --------------------------------------------------------------------
 * vt_encoder_configure   <- AutoencoderKL(...) hyper-parameters, diffusers_vae_loader.py:8-35
 * vt_set_weight          <- vae.load_state_dict(state_dict, strict=False), diffusers_vae_loader.py:44
 *                           and decoder.load_state_dict(...), infer_full.py:63.  `name` is the
 *                           state-dict key (diffusers / reference naming); `data` is a HOST pointer.
 * vt_encoder_finalize    packs weights for the MFMA kernels ([Cout][tap][Cin] bf16) and uploads them.
 * vt_decoder_configure   <- create_attention_decoder / ClassificationDecoder, infer_full.py:42-58
 */
int vt_encoder_configure(vt_context* ctx, int in_channels, int latent_channels, const int* block_out_channels,
                         int n_blocks, int layers_per_block, int norm_num_groups, float scaling_factor,
                         int has_scaling_factor, float shift_factor, int has_shift_factor);
int vt_set_weight(vt_context* ctx, const char* name, const void* host_data, int dtype, const int64_t* shape,
                  int ndim);
int vt_encoder_finalize(vt_context* ctx);
int vt_decoder_configure(vt_context* ctx, int num_classes, int latent_channels, int plain_decoder,
                         int use_spatial_attention, int use_self_attention, int use_cross_attention,
                         int attention_heads);
int vt_decoder_finalize(vt_context* ctx);

/* ---- hot path ------------------------------------------------------------------------------
 * vt_encode          <- DiffusersVAEWrapper.encode(x), diffusers_vae_loader.py:78-86:
 *                       vae.encode(x).latent_dist.mode() * scaling_factor + shift_factor.
 *                       x: fp32 NCHW [B,3,H,W] in [-1,1].  mode selects what is written (fp32 NCHW):
 *                         0: moments [B,2*latent,H/8,W/8] (mean | logvar) -- AutoencoderKL.encode surface
 *                         1: latent_dist.mode() = mean [B,latent,H/8,W/8]
 *                         2: mode() * scaling_factor + shift_factor -- DiffusersVAEWrapper.encode
 *                       (H/8, W/8 for the four-block FLUX configuration; in general H >> (num_blocks - 1), W >> (num_blocks - 1):
 *                       one Downsample2D per block but the last.  The library cannot see the size of latent_out: the caller's
 *                       buffer must hold B x channels x that many fp32 values.)
 * vt_decode_logits   <- decoder.forward(latent), modules.py:424-468 / :333-349 -> fp32 [B,N]
 * vt_get_confidence  <- sigmoid + descending sort, modules.py:470-475 (ties: ascending tag index; NaN logits sort last;
 *                       any N: up to 16384 tags in one LDS pass, more through global-memory merge passes)
 * vt_summarize_confidence <- the per-image summary loop of infer_full.py:106-125 on the sorted outputs: per image the
 *                       first K (confidence fp32, tag index int32; -1 / 0 beyond N) pairs and stats[4] = {number of tags with
 *                       confidence >= threshold, max confidence, (sum of the first five) / 5, number of non-finite confidences}
 * vt_summarize_confidence_per_class  the same summary with one threshold PER TAG (device fp32 class_thresholds [N], e.g. the
 *                       per_class_thresholds a threshold search wrote): tag idx passes when confidence >= class_thresholds[idx] -- the
 *                       CLI's >= convention (the evaluator's vt_eval_* decide with a strict >, as the reference does in both places); a
 *                       NaN confidence never passes.  The passing tags are no longer a prefix of the sorted list: per image the first K
 *                       PASSING (confidence, tag index) pairs are written in sorted order (0 / -1 behind the last passing one) and
 *                       stats[4] = {number of passing tags, max confidence, (sum of the first five of the sorted list) / 5, number of
 *                       non-finite confidences}.  Any N the sort supports.  With all thresholds equal to t: the same stats and the same
 *                       first min(count, K) pairs as vt_summarize_confidence at t.
 * vt_status          sticky device-side health word of the context (SYNCHRONISES `stream`): bit 0 (VT_STATUS_NONFINITE) =
 *                       some GroupNorm saw non-finite statistics since the last clear -- an activation left the fp16 range
 *                       of the residual-stream storage (rerun with vt_set_flag(ctx, 4, 0)) or the weights hold inf / NaN;
 *                       bit 1 (VT_STATUS_FP8_SATURATED, fp8 mode only) = some activation exceeded the e4m3 range (+-448 after its
 *                       scale) and was clamped -- the checkpoint's activations are too large for flag 11; rerun without it
 * vt_encode_tag      <- the loop body of infer_full.py:101-105 for a whole batch
 */
size_t vt_encode_workspace_bytes(const vt_context* ctx, int B, int H, int W);
int vt_encode(vt_context* ctx, const float* x_nchw, int B, int H, int W, int mode, float* latent_out,
              void* workspace, size_t workspace_bytes, void* stream);
size_t vt_decode_workspace_bytes(const vt_context* ctx, int B, int h, int w);
int vt_decode_logits(vt_context* ctx, const float* latent_nchw, int B, int h, int w, float* logits_out,
                     void* workspace, size_t workspace_bytes, void* stream);
int vt_get_confidence(vt_context* ctx, const float* logits, int B, int N, float* conf_sorted_out,
                      int64_t* indices_out, void* stream);
int vt_summarize_confidence(vt_context* ctx, const float* conf_sorted, const int64_t* indices, int B, int N, float threshold,
                            int K, float* top_conf_out /* [B][K] */, int32_t* top_idx_out /* [B][K] */,
                            float* stats_out /* [B][4] */, void* stream);
int vt_summarize_confidence_per_class(vt_context* ctx, const float* conf_sorted, const int64_t* indices, int B, int N,
                                      const float* class_thresholds /* device [N] */, int K, float* top_conf_out /* [B][K] */,
                                      int32_t* top_idx_out /* [B][K] */, float* stats_out /* [B][4] */, void* stream);
enum { VT_STATUS_NONFINITE = 1, VT_STATUS_FP8_SATURATED = 2 };
int vt_status(vt_context* ctx, int clear, int* status_out /* host */, void* stream);
/* the same word WITHOUT a host synchronisation: copied (and optionally cleared) in stream order into `status_out`, which is pinned host
 * memory or device memory and is valid once work recorded on `stream` behind this call has completed (an event / a later sync).  The
 * pipelined CLIs read batch n's word this way while batch n + 1 runs (infer_full.py:95-128 is the serial loop they replace). */
int vt_status_async(vt_context* ctx, int clear, int* status_out /* pinned host or device */, void* stream);
size_t vt_encode_tag_workspace_bytes(const vt_context* ctx, int B, int H, int W);
int vt_encode_tag(vt_context* ctx, const float* x_nchw, int B, int H, int W, float* latent_out /* may be NULL */,
                  float* logits_out, void* workspace, size_t workspace_bytes, void* stream);

/* vt_preprocess_u8 <- transforms.ToTensor() + Normalize([0.5]*3, [0.5]*3), modules.py:136-140, on the device:
 * uint8 HWC RGB [B,H,W,3] -> fp32 NCHW [B,3,H,W] in [-1,1] (the resize stays with PIL on the host). */
int vt_preprocess_u8(vt_context* ctx, const uint8_t* in_hwc, int B, int H, int W, float* out_nchw, void* stream);

/* vt_resize_u8 <- transforms.Resize((r, r)) (filter 0, bilinear) and SmartResize's crop + Image.resize(LANCZOS) (filter 1),
 * modules.py:126-178: Pillow's two-pass 8-bit resample (libImaging/Resample.c) reproduced bit for bit on the device.
 * src: uint8 HWC RGB [src_h][src_w][3]; the crop box (left, top, crop_w, crop_h) inside it is resized to dst uint8 HWC
 * [dst_h][dst_w][3].  The coefficient tables are built on the host exactly as Pillow builds them and copied with the
 * stream; the call does not wait for the GPU (it may wait for the PREVIOUS call's table copy). */
size_t vt_resize_workspace_bytes(int crop_h, int crop_w, int dst_h, int dst_w, int filter);
/* Host-only: one axis' table as vt_resize_u8 builds it, table_out[out_size][2 + ksize] = (first sample, count,
 * 22-bit coefficients...); returns ksize (call with table_out = NULL to size the buffer), -1 on a bad argument. */
int vt_resize_table(int in_size, int out_size, int filter, int* table_out, int table_ints);
int vt_resize_u8(vt_context* ctx, const uint8_t* src_hwc, int src_h, int src_w, int crop_left, int crop_top, int crop_w, int crop_h,
                 uint8_t* dst_hwc, int dst_h, int dst_w, int filter, void* workspace, size_t workspace_bytes, void* stream);

/* vt_resize_normalize_batch: vt_resize_u8 + vt_preprocess_u8 for a whole batch in one call.  B source images (device, uint8 HWC
 * RGB) of DIFFERENT sizes, each with its own crop box, are resized to one common dst_h x dst_w and written as the encoder's input:
 *   out_u8_hwc[k] == vt_resize_u8 of item k, byte for byte (a pass is skipped when that axis keeps its size, as in Pillow);
 *   out_nchw      == vt_preprocess_u8(out_u8_hwc), bit for bit.
 * Either output may be NULL (not both); the uint8 batch image is not written unless asked for.  Two launches per call whatever B
 * is: descriptors and per-image coefficient tables live in the workspace and the grid's z index selects the image.  The tables are
 * built on the host (and remembered per (size, size, filter)) and staged through a small ring of pinned blocks owned by the context:
 * the call does not wait for the GPU unless the ring has wrapped onto a block whose copy is still in flight.
 * `items` is a HOST array.  Every size is checked before anything is launched: an undersized output or workspace gives
 * VT_ERR_WORKSPACE, a NULL pointer, a crop box outside its source or an unsupported size VT_ERR_INVALID, and nothing is written.
 * vt_resize_batch_workspace_bytes returns 0 for arguments the call would reject as invalid (source pointers are not looked at). */
typedef struct { const uint8_t* src_hwc; int src_h, src_w, crop_left, crop_top, crop_w, crop_h; } vt_resize_item;
size_t vt_resize_batch_workspace_bytes(const vt_resize_item* items /* host [B] */, int B, int dst_h, int dst_w, int filter);
int vt_resize_normalize_batch(vt_context* ctx, const vt_resize_item* items /* host [B] */, int B, int dst_h, int dst_w, int filter,
                              float* out_nchw /* [B,3,dst_h,dst_w], may be NULL */, size_t out_nchw_bytes,
                              uint8_t* out_u8_hwc /* [B,dst_h,dst_w,3], may be NULL */, size_t out_u8_bytes,
                              void* workspace, size_t workspace_bytes, void* stream);

/* ---- streaming multi-label evaluator <- MultiLabelEvaluator.compute_metrics / find_optimal_threshold, evaluation.py:13-275, without the
 * n x c host matrix: the state lives in ONE caller-owned device block and is fed batch by batch in stream order; no call below
 * synchronises the host.  The state remembers nothing about its own shape: every call takes (N classes, T thresholds, capacity)
 * as the reset call did, and checks every buffer's byte size before anything is launched -- an undersized buffer is
 * VT_ERR_WORKSPACE, a null / misaligned pointer or an out-of-range argument VT_ERR_INVALID, and nothing is written.
 * Block layout (every section 256-B aligned): thresholds fp64 [32] | row_stats uint64 [3] | per-row scratch uint32 [4096] |
 * support uint32 [N] | counts uint32 [N][T][2] = (tp, fp) | keys uint64 [N][capacity].
 *   - a prediction is (double)p > thresholds[t], strict and in fp64 (numpy's float32_array > float64_scalar; for the fp32 comparison
 *     of a Python float pass the threshold rounded to fp32); a label is positive when > 0 (VT_F32 or VT_U8 labels);
 *   - row_stats = { rows whose prediction at t_main equals the label row, mismatching elements at t_main, non-finite probabilities };
 *   - capacity = samples the key store can hold; 0 = counts only (no average precision).  Key of (class j, sample i): high word = the
 *     monotone unsigned map of the probability's fp32 bits that the confidence sort uses, low word = (~i << 1) | label; stored class-major;
 *   - limits: T <= 32, B <= 4096 per update, n_seen + B < 2^31; micro AP on the device while n_seen * N < 2^31 (beyond that the
 *     workspace query returns 0: pass micro_ap_out = NULL and average on the host).
 * The grow call copies a state into a larger block (new_capacity >= old_capacity) in stream order.  The average-precision call sorts
 * the first n_seen keys of every class row IN PLACE (the state stays valid for further updates) and writes AP per class as fp64
 * (NaN for a class without a positive; scikit-learn's step-wise definition, ties grouped); with micro_ap_out != NULL it also ranks the
 * flattened store in `workspace`.  The read call copies counts [N][T][2], support [N] and row_stats [3] in stream order into device or
 * pinned host memory: they are valid once `stream` has passed the call.
 * The recount call re-decides every stored prediction under ONE THRESHOLD PER CLASS (device fp64 class_thresholds [N]) from the first
 * n_seen keys of every class row, without touching the state: the probability comes back from the key's high word (the sort-key map is
 * a bijection on the fp32 bits; -0 reads as +0), label and sample index from the low word, and a prediction is
 * (double)p > class_thresholds[j], the rule of vt_eval_update.  counts_out [N][2] = (tp, fp) per class; row_stats_out [3] = { rows whose
 * prediction row equals the label row, mismatching elements, non-finite probabilities } -- the state's own row_stats when every class
 * gets thresholds[t_main], its counts[:, t, :] when every class gets thresholds[t].  The per-sample mismatch tally is indexed by the
 * sample index in the key, so the result is the same before and after vt_eval_average_precision has sorted the rows, and on a state
 * vt_eval_merge produced.  Needs a key store: capacity == 0 with n_seen > 0, or n_seen > capacity, is VT_ERR_INVALID.  The workspace
 * (vt_eval_recount_workspace_bytes; device memory, 256-B aligned) holds the integer accumulators and the tally and is zeroed by the
 * call; sums are integers (vector atomics), so the outputs are bit-reproducible.  Outputs: device or pinned host memory. */
size_t vt_eval_state_bytes(int N, int T, long long capacity);
int vt_eval_reset(vt_context* ctx, void* state, size_t state_bytes, int N, int T, const double* thresholds /* host [T] */, int t_main,
                  long long capacity, void* stream);
int vt_eval_update(vt_context* ctx, void* state, size_t state_bytes, int N, int T, int t_main, long long capacity,
                   const float* probs /* [B][N] */, const void* labels /* [B][N] */, int labels_dtype /* VT_F32 | VT_U8 */, int B,
                   long long n_seen /* samples of the earlier updates */, void* stream);
int vt_eval_grow(vt_context* ctx, const void* old_state, size_t old_state_bytes, long long old_capacity, void* new_state,
                 size_t new_state_bytes, long long new_capacity, int N, int T, long long n_seen, void* stream);
size_t vt_eval_ap_workspace_bytes(int N, long long n_seen);
int vt_eval_average_precision(vt_context* ctx, void* state, size_t state_bytes, int N, int T, long long capacity, long long n_seen,
                              double* ap_out /* [N] */, size_t ap_bytes, double* micro_ap_out /* [1], may be NULL */, void* workspace,
                              size_t workspace_bytes, void* stream);
int vt_eval_read_counts(vt_context* ctx, const void* state, size_t state_bytes, int N, int T, long long capacity, uint32_t* counts_out,
                        size_t counts_bytes, uint32_t* support_out, size_t support_bytes, uint64_t* row_stats_out, size_t row_stats_bytes,
                        void* stream);
size_t vt_eval_recount_workspace_bytes(int N, long long n_seen);
int vt_eval_recount(vt_context* ctx, const void* state, size_t state_bytes, int N, int T, long long capacity, long long n_seen,
                    const double* class_thresholds /* DEVICE [N] */, uint32_t* counts_out /* [N][2] = (tp, fp) */, size_t counts_bytes,
                    uint64_t* row_stats_out /* [3] */, size_t row_stats_bytes, void* workspace, size_t workspace_bytes, void* stream);

/* ---- sharded evaluation: a state block as a wire format, and the merge of several blocks on one device.  Same contract as above:
 * every size is checked on the host before anything is launched (undersized buffer: VT_ERR_WORKSPACE; null / misaligned pointer or
 * out-of-range argument: VT_ERR_INVALID; nothing is written), no host synchronisation, work is queued on `stream`.
 * vt_eval_export writes into out_state an ordinary state of capacity out_capacity (vt_eval_state_bytes(N, T, out_capacity) bytes) that
 * holds the same statistics: thresholds, row_stats, support and counts copied, the row scratch zeroed, the first n_seen key columns of
 * every class row copied and the padding columns zero-filled -- the block's bytes are a function of the data only.  out_capacity is
 * >= n_seen (it may be SMALLER than capacity: unlike vt_eval_grow the export compacts) or 0 (head only, no keys).  Ranks with different
 * n_seen and capacities that export at the maximum n_seen all get blocks of one size: what an all-gather moves.
 * vt_eval_merge adds the W sources' support, counts and row_stats into dst (integers: bit-reproducible) and appends the first n_w keys
 * of every class row of source w at column dst_n_seen + sum_{v<w} n_v, sources in the order given.  The sample index in a key's low
 * word, (~i << 1) | label, is rebased by that column offset o -- the key minus (o << 1), which never borrows into the high word while
 * i + o < 2^31 -- so the merged block is the state one evaluator fed every sample in that order would hold: it takes further
 * vt_eval_update calls with n_seen = the total, and vt_eval_average_precision.  dst keeps its thresholds; equal threshold tables and
 * t_main in the sources are the caller's contract.  Two launches whatever W is (the descriptors travel as a kernel argument).
 * Refused with VT_ERR_INVALID: W < 1 or W > 64; a source that is dst or overlaps it; dst_capacity > 0 with a source of capacity 0 and
 * n_seen > 0; dst_n_seen + sum n_w > dst_capacity when dst_capacity > 0; a total of 2^31 or more.  dst_capacity == 0 merges the head only.
 * `sources` is a HOST array; a source's n_seen is the number of samples its block holds (its counts cover all of them). */
typedef struct { const void* state; size_t state_bytes; long long capacity; long long n_seen; } vt_eval_source;
int vt_eval_export(vt_context* ctx, const void* state, size_t state_bytes, int N, int T, long long capacity, long long n_seen,
                   void* out_state, size_t out_bytes, long long out_capacity, void* stream);
int vt_eval_merge(vt_context* ctx, void* dst, size_t dst_bytes, int N, int T, long long dst_capacity, long long dst_n_seen,
                  const vt_eval_source* sources /* host [W] */, int W, void* stream);

/* ---- streaming validation loss <- the validation loop of train_decoder.py:218-241 and the three losses it chooses from:
 * nn.BCEWithLogitsLoss, FocalLoss and ClassBalancedLoss (improved_losses.py:39-72).  Forward only.  Same contract as vt_eval_*: ONE
 * caller-owned device block (vt_loss_state_bytes(N) bytes, 256-B aligned) fed batch by batch in stream order; every byte size is
 * checked on the host before anything is launched -- an undersized buffer is VT_ERR_WORKSPACE, a null / misaligned pointer or an
 * out-of-range argument VT_ERR_INVALID, and nothing is written; no call synchronises the host.
 * vt_loss_update takes the decoder's LOGITS fp32 [B][N] (not the sigmoid outputs, which saturate) and the labels: a VT_F32 label is
 * used as its value (the `tag:weight` floats of the training JSON need not be 0 or 1), a VT_U8 label is 0 or 1.  Per element, in
 * fp64 from the fp32 inputs:
 *     bce   = max(x, 0) - x y + log1p(exp(-|x|))            (the stable form of binary_cross_entropy_with_logits)
 *     focal = alpha (1 - exp(-bce))^gamma bce               (alpha, gamma stored at reset; gamma >= 0)
 * Block layout (every section 256-B aligned):
 *     params  { fp64 alpha, fp64 gamma, uint64 has_weights, uint64 N }
 *   | totals  { fp64 [3] = sum over the updates of the PER-BATCH MEAN of bce, of focal and of weighted bce -- each
 *               sum_j w_j (sum of class j over the batch) / (B N), w_j = 1 for the first two --, uint64 [3] = updates, elements,
 *               non-finite logits }
 *   | class weights fp64 [N] (1.0 when reset was given none)  | class sums fp64 [N][2] = (bce, focal) over every row seen
 *   | the last update's partials, one { fp64 [3], uint64 } per 64 classes.
 * totals[k] / updates is train_decoder.py's val_loss / val_steps for this batching; sum_j sums[j][k] / elements is the mean over all
 * elements, independent of the batching.  A non-finite logit propagates into the sums as it would into the reference's loss; the
 * counter says why.  An infinite class weight (a class without a sample, ClassBalancedLoss) makes the weighted sums infinite.
 * Determinism: no floating-point atomic (no atomic at all); per update one thread owns a class, rows and classes are combined in an
 * order fixed by (B, N) alone, so the state after a given call sequence is bit-identical from run to run.  B <= 4096 per update.
 * vt_loss_reset clears the block; class_weights is a HOST fp64 [N] or NULL and is free again when the call returns.
 * vt_loss_read copies the whole block as it stands, in stream order, into device or pinned host memory of vt_loss_state_bytes(N) bytes.
 * vt_loss_merge adds the W sources into dst IN THE ORDER GIVEN (dst = ((dst + s_0) + s_1) + ...: reproducible for a given sharding);
 * dst keeps its parameters.  The parameters every block was reset with are the caller's to state (HOST values, as (N, T, capacity)
 * are for vt_eval_*): a source whose alpha, gamma or class weights differ bit-wise from dst's is VT_ERR_INVALID, as are W < 1, W > 64
 * and a source that is dst or overlaps it. */
typedef struct { const void* state; size_t state_bytes; double alpha; double gamma; const double* class_weights /* host [N] or NULL */; } vt_loss_source;
size_t vt_loss_state_bytes(int N);
int vt_loss_reset(vt_context* ctx, void* state, size_t state_bytes, int N, double alpha, double gamma,
                  const double* class_weights /* host [N] or NULL */, void* stream);
int vt_loss_update(vt_context* ctx, void* state, size_t state_bytes, int N, const float* logits /* [B][N] */,
                   const void* labels /* [B][N] */, int labels_dtype /* VT_F32 | VT_U8 */, int B, void* stream);
int vt_loss_read(vt_context* ctx, const void* state, size_t state_bytes, int N, void* out, size_t out_bytes, void* stream);
int vt_loss_merge(vt_context* ctx, void* dst, size_t dst_bytes, int N, double alpha, double gamma,
                  const double* class_weights /* host [N] or NULL */, const vt_loss_source* sources /* host [W] */, int W, void* stream);

/* ---- per-image (example-based) metrics <- calculate_metrics, batch_inference_test.py:63-137: for every image precision_i =
 * |true & pred| / |pred|, recall_i = |true & pred| / |true|, F1_i and the exact match, averaged over the images -- the reduction of
 * the [B][N] matrix along the CLASSES, where vt_eval_* reduces it along the samples.  Same contract as vt_eval_* / vt_loss_*: ONE
 * caller-owned device block (vt_sample_state_bytes(T, capacity) bytes, 256-B aligned) fed batch by batch in stream order; every size
 * is checked on the host before anything is launched -- an undersized buffer is VT_ERR_WORKSPACE, a null / misaligned pointer or an
 * out-of-range argument VT_ERR_INVALID, and nothing is written; no call synchronises the host.
 * Block layout (every section 256-B aligned):
 *     thresholds fp64 [32]
 *   | totals { uint64 [32] = (rule, T, 0 ...), uint32 [4096]: non-finite probabilities seen in row b of every update }
 *   | true uint32 [capacity]                       (an image's true tags: positive labels + true_extra)
 *   | rows uint32 [capacity][T][2] = (tp, predicted)
 * so a merge of shards is a concatenation of `true` and `rows` (and a sum of the 4096 slots).  T <= 32, B <= 4096 per update,
 * n_seen + B <= capacity < 2^31.
 *   - a prediction is (double)p > thresholds[t] (VT_SAMPLE_GT, the rule of vt_eval_update) or (double)p >= thresholds[t] (VT_SAMPLE_GE,
 *     infer_full.py's conf_value >= confidence_threshold), decided in fp64; a NaN probability never predicts; a non-finite one is
 *     counted; a label is positive when > 0 (VT_F32 or VT_U8 labels);
 *   - vt_sample_update writes, for row b, true[n_seen + b] = (positive labels of the row) + true_extra[b] (device uint32 [B] or NULL:
 *     the image's ground-truth tags that are not in the tag list -- the reference counts them in |true|, so they lower recall) and
 *     (tp, predicted) for every threshold.  One launch, one workgroup per row, all T thresholds from one pass over the row, no atomics;
 *   - vt_sample_from_keys fills a T = 1 state from the first n_seen keys of every class row of a vt_eval_* state (capacity > 0) under
 *     ONE THRESHOLD PER CLASS (device fp64 class_thresholds [N]): the probability comes back from the key's high word as
 *     vt_eval_recount recovers it, label and sample index from the low word, so the result is the same before and after
 *     vt_eval_average_precision has sorted the rows and on a state vt_eval_merge produced.  true_extra: device uint32 [n_seen] or NULL.
 *     The tallies go through integer vector atomics into rows the call zeroes itself: bit-reproducible.  The evaluator state is only read;
 *   - vt_sample_finish writes vt_sample_finish_bytes(T) bytes into `out` (device or pinned host memory):
 *         fp64 [T][3] = { sum precision_i, sum recall_i, sum F1_i } | uint64 [T][2] = { exact matches, images with no prediction }
 *       | uint64 [2] = { images with no true tag, non-finite probabilities }
 *     with the reference's conventions: precision 0 when nothing is predicted, recall 1 when the image has no true tag,
 *     F1 = 2 P R / (P + R) from the fp64 P and R or 0 when P + R = 0, exact match when tp == predicted == true.  The sums run in
 *     image order (the order of the reference's loop), without floating-point atomics: two runs give the same bits, and a host
 *     loop over the same images gives them too.  (scikit-learn's
 *     average="samples" recall is (sum recall_i - images with no true tag) / n.)
 *   - vt_sample_read_rows copies true [n_seen] and rows [n_seen][T][2] in stream order into device or pinned host memory. */
enum { VT_SAMPLE_GT = 0, VT_SAMPLE_GE = 1 };
size_t vt_sample_state_bytes(int T, long long capacity);
int vt_sample_reset(vt_context* ctx, void* state, size_t state_bytes, int T, const double* thresholds /* host [T] */, int rule,
                    long long capacity, void* stream);
int vt_sample_update(vt_context* ctx, void* state, size_t state_bytes, int T, long long capacity, const float* probs /* [B][N] */,
                     const void* labels /* [B][N] */, int labels_dtype /* VT_F32 | VT_U8 */, const uint32_t* true_extra /* [B] or NULL */,
                     int B, int N, long long n_seen /* samples of the earlier updates */, void* stream);
int vt_sample_from_keys(vt_context* ctx, const void* eval_state, size_t eval_state_bytes, int N, int T_eval, long long capacity,
                        long long n_seen, const double* class_thresholds /* DEVICE [N] */, int rule,
                        const uint32_t* true_extra /* DEVICE [n_seen] or NULL */, void* sample_state /* T = 1 */, size_t sample_state_bytes,
                        long long sample_capacity, void* stream);
size_t vt_sample_finish_bytes(int T);
int vt_sample_finish(vt_context* ctx, const void* state, size_t state_bytes, int T, long long capacity, long long n_seen, void* out,
                     size_t out_bytes, void* stream);
int vt_sample_read_rows(vt_context* ctx, const void* state, size_t state_bytes, int T, long long capacity, long long n_seen,
                        uint32_t* true_out /* [n_seen] */, size_t true_bytes, uint32_t* rows_out /* [n_seen][T][2] */, size_t rows_bytes,
                        void* stream);

/* algorithmic FLOPs of one encoder forward at HxW -- for roofline reporting */
double vt_encoder_flops(const vt_context* ctx, int H, int W);

/* ---- training the decoder's classifier head (train_decoder.py:173-263) --------------------------------------------------------
 * vt_decode_logits = front + head.  The FRONT (ClassificationDecoder: the 4x4 adaptive pool; AttentionClassificationDecoder: spatial
 * attention, feature_compress, self- / cross-attention) ends in one feature row per image, [B][F] fp32 with F = vt_decoder_feature_dim
 * (256 plain, 512 attention) whatever the latent's size; the HEAD is `classifier.*`: Linear -> LayerNorm -> (Leaky)ReLU -> Dropout
 * layers and Linear(256, N).  vt_decode_features runs the front alone (workspace: vt_decode_workspace_bytes); vt_head_forward on its
 * rows gives vt_decode_logits' bits.  With these calls alone the front is frozen (BatchNorm on its running statistics, no dropout), so
 * an image's feature row never changes and can be cached across epochs; the attention decoder's front is trained by vt_front_* and its
 * cross-attention by vt_cross_* below.
 *
 * The trainer keeps everything in one caller-owned, 256-B aligned device block of vt_head_state_bytes(ctx) bytes (layout:
 * csrc/vt_train.h): fp32 parameters, gradients, Adam m and v, the gradient norm / clip coefficient, and a ring of VT_HEAD_RING fp64
 * loss values.  Every linear layer's INPUT width must be a multiple of 256 (the backward kernel's column block): true of both reference
 * heads at latent_channels = 16 (F = 256 / 512, hidden 1024 / 512 / 256); otherwise vt_head_state_bytes returns 0.  fp32 storage, fp64 loss elements and scalar reductions, no atomics: every sum runs in an order fixed by the shapes, so
 * the same call sequence leaves the same bits.  No call synchronises the host.  The decoder must be finalized; its shapes size the block.
 *   vt_head_init      parameters <- the context's classifier tables; gradients, m, v, ring <- 0
 *   vt_head_forward   eval-mode logits [B][N] of the state's parameters
 *   vt_head_forward_backward   forward (train != 0: dropout at dropout_p[layer], HOST array of the hidden layers' rates, NULL = none;
 *                     mask of element i of layer l at (seed, step): a counter-based hash, regenerated in backward; survivors scaled
 *                     by 1 / (1 - p)), the loss, its gradient, backward through every layer, ADDED into the gradients.
 *                     loss_kind 0: BCE-with-logits, mean over B N; 1: focal alpha (1 - e^-bce)^gamma bce; 2: class_weights[c] bce
 *                     (device fp32 [N]: losses.class_balanced_weights).  labels [B][N]: VT_F32 used as its value, or VT_U8 (0 / 1).
 *                     ring[step % VT_HEAD_RING] = loss_scale x loss; the gradients are those of loss_scale x loss.
 *                     logits_out (may be NULL): the forward's logits.  masks_out (may be NULL): one byte per element and hidden layer,
 *                     layer after layer, [B][d_l] each (1 = kept).  Workspace: vt_head_workspace_bytes(ctx, B).
 *   vt_head_clip      clip_grad_norm_(max_norm): total L2 norm of the gradients forward_backward left (partials written by the
 *                     kernels that wrote them, added in a fixed order), coef = min(1, max_norm / (norm + 1e-6)); the gradients are
 *                     scaled in place when coef < 1 and keep their bits otherwise.  VT_HEAD_NORM reads { fp64 norm^2, fp32 norm, fp32 coef }.
 *                     (Gradients set with vt_head_write are not in the norm until a forward_backward has added to them.)
 *   vt_head_step      torch.optim.AdamW's update number t (1-based) with decoupled weight decay; zeroes the gradients in the same pass
 *   vt_head_commit    the context's classifier tables <- parameters: vt_decode_logits and everything on it sees the trained head
 *   vt_head_read / vt_head_write   one named tensor ("classifier.8.weight") of the parameters, gradients, m or v, the loss ring
 *                     (fp64 [VT_HEAD_RING]) or the norm scalars, copied in stream order to / from device or pinned host memory
 */
enum { VT_HEAD_PARAM = 0, VT_HEAD_GRAD = 1, VT_HEAD_ADAM_M = 2, VT_HEAD_ADAM_V = 3, VT_HEAD_LOSS_RING = 4, VT_HEAD_NORM = 5 };
enum { VT_HEAD_LOSS_BCE = 0, VT_HEAD_LOSS_FOCAL = 1, VT_HEAD_LOSS_CLASS_BALANCED = 2 };
int vt_decoder_feature_dim(const vt_context* ctx);
int vt_decode_features(vt_context* ctx, const float* latent_nchw, int B, int h, int w, float* features_out /* [B][F] */, void* workspace,
                       size_t workspace_bytes, void* stream);
size_t vt_head_state_bytes(const vt_context* ctx);
size_t vt_head_workspace_bytes(const vt_context* ctx, int B);
int vt_head_init(vt_context* ctx, void* state, size_t state_bytes, void* stream);
int vt_head_forward(vt_context* ctx, const void* state, size_t state_bytes, const float* features, int B, float* logits_out, void* workspace,
                    size_t workspace_bytes, void* stream);
int vt_head_forward_backward(vt_context* ctx, void* state, size_t state_bytes, const float* features, const void* labels, int labels_dtype,
                             int B, int loss_kind, double focal_alpha, double focal_gamma, const float* class_weights, double loss_scale,
                             int train, const float* dropout_p /* host */, unsigned long long seed, unsigned long long step,
                             float* logits_out, unsigned char* masks_out, void* workspace, size_t workspace_bytes, void* stream);
int vt_head_clip(vt_context* ctx, void* state, size_t state_bytes, float max_norm, void* stream);
int vt_head_step(vt_context* ctx, void* state, size_t state_bytes, double lr, double beta1, double beta2, double eps, double weight_decay,
                 long long t, void* stream);
int vt_head_commit(vt_context* ctx, const void* state, size_t state_bytes, void* stream);
int vt_head_read(vt_context* ctx, const void* state, size_t state_bytes, int kind, const char* name, void* out, size_t out_bytes, void* stream);
int vt_head_write(vt_context* ctx, void* state, size_t state_bytes, int kind, const char* name, const void* src, size_t src_bytes,
                  void* stream);

/* ---- training the attention decoder's front (csrc/train_front.hip) ------------------------------------------------------------
 * spatial_attention.*, feature_compress.* and self_attention_post.* of AttentionClassificationDecoder at latent_channels = 16, heads in
 * {1, 2, 4, 8}, each of spatial and self attention on or off (vt_front_state_bytes returns 0 otherwise, and for the plain decoder).  On a
 * decoder with cross-attention these calls train the same 17 tensors and vt_front_forward yields, in both modes, the rows cross-attention
 * reads (modules.py:448), not the head's feature rows: vt_cross_* below is the piece between the two.  Same conventions as the head
 * trainer: a caller-owned, 256-B aligned state block (layout: csrc/vt_train.h), fp32 storage, fp64 statistics and norm partials, no
 * atomics, every sum in an order fixed by the shapes, no host synchronisation.  The gradient with respect to the latent is not
 * computed (the encoder is frozen).
 *   vt_front_init      parameters and BatchNorm running statistics <- the context's tables; gradients, m, v, num_batches_tracked <- 0
 *   vt_front_forward   train = 0: the inference front on the state's parameters and running statistics (right after init or commit:
 *                      vt_decode_features' bits).  train != 0: BatchNorm on the batch's statistics (biased variance over B h w, fp64
 *                      partials per 256 pixels finished in order), running_mean / running_var updated with momentum 0.1 and the unbiased
 *                      variance, num_batches_tracked + 1; dropout at attention_dropout on the softmax weights [B][heads][64][64], mask =
 *                      the head trainer's hash of (seed, step, layer 8, element), survivors scaled by 1 / (1 - p); mask_out (may be
 *                      NULL) receives it as bytes.  The workspace (vt_front_workspace_bytes) keeps what the backward of the SAME batch
 *                      reads: pass the same latent, dropout arguments and workspace to vt_front_backward before the next forward.
 *   vt_front_backward  d_features [B][F] -> gradients of every front tensor, ADDED into the state.  Channel max: the gradient goes to
 *                      the arg-max channel, the lowest index on a tie; ReLU: derivative 0 at exactly 0.
 *   vt_front_step      AdamW as vt_head_step.   vt_front_commit   the context's tables <- the state, the BatchNorm fold included
 *   vt_front_read / vt_front_write   by state-dict key; kinds VT_HEAD_PARAM / GRAD / ADAM_M / ADAM_V / NORM, and the BatchNorm buffers
 *                      VT_FRONT_BN_MEAN / VT_FRONT_BN_VAR (fp32 [8]) / VT_FRONT_BN_TRACKED (int64), for which `name` is ignored
 *   vt_head_forward_backward_dx   vt_head_forward_backward (same bits in the state) + d_features [B][F] = d loss / d features
 *   vt_train_clip      one clip_grad_norm_ over both blocks: norm^2 = the head's partials in order, then the front's; both blocks get
 *                      the same { norm^2, norm, coef } and are scaled in place when coef < 1, untouched otherwise
 */
enum { VT_FRONT_BN_MEAN = 6, VT_FRONT_BN_VAR = 7, VT_FRONT_BN_TRACKED = 8 };
size_t vt_front_state_bytes(const vt_context* ctx);
size_t vt_front_workspace_bytes(const vt_context* ctx, int B, int h, int w);
int vt_front_init(vt_context* ctx, void* state, size_t state_bytes, void* stream);
int vt_front_forward(vt_context* ctx, void* state, size_t state_bytes, const float* latent_nchw, int B, int h, int w, int train,
                     float attention_dropout, unsigned long long seed, unsigned long long step, float* features_out /* [B][F] */,
                     unsigned char* mask_out, void* workspace, size_t workspace_bytes, void* stream);
int vt_front_backward(vt_context* ctx, void* state, size_t state_bytes, const float* latent_nchw, const float* d_features /* [B][F] */, int B,
                      int h, int w, float attention_dropout, unsigned long long seed, unsigned long long step, void* workspace,
                      size_t workspace_bytes, void* stream);
int vt_front_step(vt_context* ctx, void* state, size_t state_bytes, double lr, double beta1, double beta2, double eps, double weight_decay,
                  long long t, void* stream);
int vt_front_commit(vt_context* ctx, const void* state, size_t state_bytes, void* stream);
int vt_front_read(vt_context* ctx, const void* state, size_t state_bytes, int kind, const char* name, void* out, size_t out_bytes, void* stream);
int vt_front_write(vt_context* ctx, void* state, size_t state_bytes, int kind, const char* name, const void* src, size_t src_bytes,
                   void* stream);
int vt_head_forward_backward_dx(vt_context* ctx, void* state, size_t state_bytes, const float* features, const void* labels, int labels_dtype,
                                int B, int loss_kind, double focal_alpha, double focal_gamma, const float* class_weights, double loss_scale,
                                int train, const float* dropout_p /* host */, unsigned long long seed, unsigned long long step,
                                float* logits_out, unsigned char* masks_out, float* d_features /* [B][F] */, void* workspace,
                                size_t workspace_bytes, void* stream);
int vt_train_clip(vt_context* ctx, void* head_state, size_t head_state_bytes, void* front_state, size_t front_state_bytes, float max_norm,
                  void* stream);

/* ---- training the attention decoder's cross-attention (csrc/train_cross.hip) ---------------------------------------------------
 * query_generator.* and cross_attention.* (ten tensors, 530 176 parameters; modules.py:105-124, :451-459): the piece between the rows
 * x [B][512] vt_front_forward yields on a decoder with cross-attention and the feature rows the head reads.  A third caller-owned,
 * 256-B aligned state block with the conventions above (layout: csrc/vt_train.h).  vt_cross_state_bytes is non-zero exactly for an
 * attention decoder with cross-attention, latent_channels = 16 and heads in {1, 2, 4, 8}; B <= 1024.  The piece has no dropout and no
 * normalisation layer: training and eval forward are the same function.
 *   vt_cross_init      parameters <- the context's tables; gradients, m, v <- 0
 *   vt_cross_forward   features_out = x + mean(out_proj(attention(q_proj(q), k / v of x's 64 tokens)) + q), q = query_generator(x): the
 *                      inference launches on the state's tensors (after the front's eval forward: vt_decode_features' bits).
 *                      features_out may not alias x_in.  The workspace (vt_cross_workspace_bytes) keeps what the backward of the SAME
 *                      batch reads: pass the same x_in and workspace to vt_cross_backward before the next forward.
 *   vt_cross_backward  d_features [B][512] -> gradients of all ten tensors, ADDED into the state, and d_x_out [B][512] = d loss / d x
 *                      (d_features + the piece's own part), which vt_front_backward takes as its d_features.  d_x_out may be d_features.
 *   vt_cross_step      AdamW as vt_head_step.   vt_cross_commit   the context's tables <- the state
 *   vt_cross_read / vt_cross_write   by state-dict key; kinds VT_HEAD_PARAM / GRAD / ADAM_M / ADAM_V, and VT_HEAD_NORM (read only)
 *   vt_train_clip3     vt_train_clip over three blocks: norm^2 = the head's partials in order, then the front's, then the cross
 *                      block's; the same { norm^2, norm, coef } is written to all three
 */
size_t vt_cross_state_bytes(const vt_context* ctx);
size_t vt_cross_workspace_bytes(const vt_context* ctx, int B);
int vt_cross_init(vt_context* ctx, void* state, size_t state_bytes, void* stream);
int vt_cross_forward(vt_context* ctx, void* state, size_t state_bytes, const float* x_in /* [B][512] */, int B, float* features_out /* [B][512] */,
                     void* workspace, size_t workspace_bytes, void* stream);
int vt_cross_backward(vt_context* ctx, void* state, size_t state_bytes, const float* x_in, const float* d_features /* [B][512] */, int B,
                      float* d_x_out /* [B][512] */, void* workspace, size_t workspace_bytes, void* stream);
int vt_cross_step(vt_context* ctx, void* state, size_t state_bytes, double lr, double beta1, double beta2, double eps, double weight_decay,
                  long long t, void* stream);
int vt_cross_commit(vt_context* ctx, const void* state, size_t state_bytes, void* stream);
int vt_cross_read(vt_context* ctx, const void* state, size_t state_bytes, int kind, const char* name, void* out, size_t out_bytes, void* stream);
int vt_cross_write(vt_context* ctx, void* state, size_t state_bytes, int kind, const char* name, const void* src, size_t src_bytes,
                   void* stream);
int vt_train_clip3(vt_context* ctx, void* head_state, size_t head_state_bytes, void* front_state, size_t front_state_bytes, void* cross_state,
                   size_t cross_state_bytes, float max_norm, void* stream);

/* ---- sharded training: the gradient exchange (csrc/train_common.hip) ------------------------------------------------------------
 * Data-parallel ranks all-gather their gradients and every rank merges them itself, in rank order, on the device: no atomics, the
 * same bits on every rank and run to run, so the ranks' parameters and Adam moments never drift apart and nothing is broadcast.
 * The same three calls exist for each trainer block (vt_head_ / vt_front_ / vt_cross_):
 *   grads_floats   P: the floats of the block's gradient section, padding included (0 where state_bytes is 0)
 *   grads_export   dst (device, 16-B aligned, dst_bytes >= 4 P) <- the gradient section, in stream order
 *   grads_merge    gradient[e] = (float) sum over r = 0 .. K-1, in that order, of weights[r] * (double)src[r * stride_floats + e]: fp64,
 *                  the multiply and the add rounded separately, one final cast.  src: device, 16-B aligned, not inside the state;
 *                  stride_floats a multiple of 4 and >= P (several blocks may sit side by side in one gathered buffer); 1 <= K <= 64;
 *                  weights: HOST array of K finite, non-negative values (n_r / sum n: the merged gradient is then the concatenated
 *                  batch's); a rank whose weight is 0 is still read.  The same launch rewrites every squared-norm partial of the block
 *                  from the merged values, so clip and step follow as after a backward.
 */
size_t vt_head_grads_floats(const vt_context* ctx);
int vt_head_grads_export(vt_context* ctx, const void* state, size_t state_bytes, void* dst, size_t dst_bytes, void* stream);
int vt_head_grads_merge(vt_context* ctx, void* state, size_t state_bytes, const float* src, size_t stride_floats, int K, const double* weights,
                        void* stream);
size_t vt_front_grads_floats(const vt_context* ctx);
int vt_front_grads_export(vt_context* ctx, const void* state, size_t state_bytes, void* dst, size_t dst_bytes, void* stream);
int vt_front_grads_merge(vt_context* ctx, void* state, size_t state_bytes, const float* src, size_t stride_floats, int K, const double* weights,
                         void* stream);
size_t vt_cross_grads_floats(const vt_context* ctx);
int vt_cross_grads_export(vt_context* ctx, const void* state, size_t state_bytes, void* dst, size_t dst_bytes, void* stream);
int vt_cross_grads_merge(vt_context* ctx, void* state, size_t state_bytes, const float* src, size_t stride_floats, int K, const double* weights,
                         void* stream);

/* ---- options ---------------------------------------------------------------------------------
 * flag 0: 1 (default) = 3x3 stride-1 convs use the halo-tile kernel (conv3x3_halo.hip),
 *         0 = every contraction uses the generic implicit-GEMM kernel (conv_gemm.hip).
 * flag 1: 1 (default) = conv epilogues emit GroupNorm partial statistics for the next norm,
 *         0 = every GroupNorm runs its own statistics pass.
 * flag 2: 1 = GroupNorm-apply + SiLU in front of a 3x3 stride-1 conv runs inside that conv's halo staging,
 *         0 (default) = as a standalone HBM-bound pass (one read + one bf16 write of the tensor).
 * flag 3: two-workgroups-per-CU tiles of the halo conv: 3 (default) = every plain-input layer on the
 *         4-wave x 256-VGPR tile (16x16 px x 128 couts), 2 = only the 128-cout layers on it, 1 = the 128-cout layers on
 *         the 8-wave x 128-VGPR tile, 0 = one workgroup per CU (16x16 px x 256 couts / 32x16 px x 128 couts);
 *         4 = the round-4 experiment tile: ONE wave per SIMD (4 waves x 512 registers, accumulators in AGPRs, 32x16 px x 128 couts) --
 *         bit-identical outputs, 16-21 % slower on bare layer loops; kept for the microbenchmark, never the default.
 * flag 4: 1 (default) = the residual stream between resnet blocks is STORED as fp16 (all arithmetic stays fp32;
 *         halves the HBM traffic of the conv2 epilogues and of norm1) and each block's conv1 output as fp16 instead of
 *         bf16 (read only by norm2), 0 = stored as fp32 / bf16.
 * flag 5: 1 (default) = conv_in (3 -> 128 channels) runs on the matrix cores with split (hi + lo) bf16 operands
 *         (products to ~2^-16 relative), 0 = exact fp32 VALU conv.  vt_op_conv_in follows it when Cout == 128.
 * flag 6: 1 (default) = 1x1 / GEMM launches with K <= 512 (resnet shortcuts, attention
 *         projections, Q.K^T) and the 128-cout stride-2 conv use a 192x128 tile at two workgroups per CU,
 *         0 = the 256x256 / 256x128 tiles.
 * flag 7: mid-block attention softmax. 0 (default) = no softmax pass: Q.K^T stores exp(s - c_i) (c_i from operand norms),
 *         P.V divides by the row sums; a launch group whose norm bound is too loose is flagged on the device and takes c_i
 *         = the exact row maximum from an extra, otherwise gated-off Q.K^T pass.  1 = always the exact row maximum.
 *         2 = fp16 scores, a row-softmax pass, bf16 P.
 * flag 8: 1 (default) = a resnet block's 1x1 conv_shortcut runs inside its conv2 launch (extra K-steps on a bf16 copy of the
 *         block input): no shortcut tensor is written or read back.  0 = separate GEMM launch + residual add.
 * flag 9: 1 (default) = Q.K^T of the mid-block attention (modes 0 / 1 of flag 7, 512 channels) on its own kernel (Q rows in
 *         registers, keys streamed through LDS, row sums in registers); 0 = the generic GEMM with the exp epilogue.
 * flag 10: 1 (default) = P.V reads the probabilities (4+ GB per launch, read once) with the streaming (nt) cache policy so they
 *         do not displace the rest of the working set from L2 / Infinity Cache; 0 = default policy.
 * flag 12: 1 (default) = with flag 9, Q.K^T stores the probabilities in the MFMA fragment order it holds them in and P.V runs on its
 *         own kernel that loads them straight into registers (only v^T passes through LDS); 0 = row-major P + the generic GEMM.
 * flag 11: 1 = BASELINE.json configs[4]: all 23 3x3 convolutions of the resnet / downsample stack run on fp8 (OCP e4m3) operands on
 *         the fp8 MFMA (2x the bf16 rate): the 20 stride-1 convs on v_mfma_scale_f32_32x32x64_f8f6f4 (conv3x3_halo_fp8.hip), the
 *         three stride-2 convs on the same instruction over the input's phase planes (conv3x3_s2_halo_fp8.hip; flag 13).  Weights e4m3
 *         with per-output-channel scales; activations e4m3(8 x) written by the GroupNorm-apply pass, the block output feeding a
 *         stride-2 conv e4m3(x); fp32 accumulate.  The mid-block attention follows (flags 14, 15); conv_in, conv_out, the 1x1
 *         shortcuts and to_out stay bf16 / fp32.  OPT-IN, for tagging only: latents move by ~1e-1 (max; rms 2e-2), logits stay
 *         within 1e-2 of the CPU reference (measured 4-5e-3; tests/diagnostics/fp8_study.py).  0 (default) = bf16.
 * flag 13: 1 (default) = the three stride-2 convs (Downsample2D) run on the phase-plane halo kernels (conv3x3_s2_halo.hip, and
 *         conv3x3_s2_halo_fp8.hip in fp8 mode); 0 = on the generic implicit GEMM (bf16, or its e4m3 variant).
 * flag 14: 1 (default) = in fp8 mode Q.K^T and P.V multiply e4m3 operands on v_mfma_scale_f32_16x16x128_f8f6f4 (attn_fp8.hip: q8 | k8 =
 *         e4m3(8 q | 8 k), v8^T, numerators e4m3(32 exp(s - sampled row maximum)) with a device-side overflow flag and a gated exact
 *         redo; flag 7 = 1: always the exact maximum); 0 = the bf16 attention kernels in fp8 mode too.
 * flag 15: 1 (default) = with flag 14, the q | k and v projections multiply e4m3 operands too (tokens e4m3(8 x) from the GroupNorm pass,
 *         [Wq; Wk] and Wv as e4m3(W / s), one scale per matrix) and write q8 | k8 and v8^T directly (proj_fp8_kernel); 0 = bf16
 *         projections followed by conversion passes.
 * flag 16: tile shape of the fp8 halo conv (flag 11) = value & 3: 0 (default) = 8 rows x 32 px x 128 couts on 4 waves, two workgroups
 *         per CU; 1 = 16 x 32 px, 2 = 8 x 64 px, both on 8 waves, one workgroup per CU (a staged weight tile serves twice the pixels);
 *         applied to the layers with Cin <= 128, or to every layer with value & 4.  The conv outputs are bit-identical for every value (the
 *         GroupNorm partials are per tile, so their merge order -- the last bits of the statistics -- follows the shape).
 * flag 17: 1 (default) = the attention's bf16 linear layers run on attn_qk.hip's skeleton: q | k and v^T (mode 4: one operand's rows in
 *         registers, the other's streamed through LDS, bias + bf16 store in the epilogue) and to_out (mode 5: + residual stream, fp16 / fp32
 *         stores, GroupNorm partials of the result); 0 = the generic GEMM (conv_gemm.hip).
 * flag 18: 1 = fp16 instead of bf16 MFMA operands for the convolutions (GroupNorm outputs, the 16-bit operand copies and the packed
 *         weights carry fp16 bits: the same 2 B per element, 11 significand bits instead of 8; v_mfma_f32_16x16x32_f16).  Latents move
 *         ~6x closer to the fp32 reference (max |dlatent| 1.5e-3 instead of 1e-2 .. 2e-2 on smooth pictures, where bf16's rounding
 *         errors add coherently); the matrix pipe draws more power on fp16 data, about 4 % of the images/s.  Values must fit fp16
 *         (|x| <= 65504: GroupNorm + SiLU outputs and weights do; an overflow shows as status bit 0).  Ignored in fp8 mode (flag 11);
 *         needs the default kernel selection (flags 0, 2, 3, 13 at their defaults), other settings keep bf16 for the convs they affect.
 *         The attention keeps bf16 (its softmax numerators need bf16's range).  0 (default) = bf16 operands, BASELINE.json's dtype.
 * flag 19: 1 (default) = the 16-bit (fp8 mode: e4m3) copy of a stage's output that feeds its stride-2 conv is written chunk-planar --
 *         [C/32][H][W][32] (e4m3: [C/64][H][W][64]) per image instead of NHWC -- when a phase-plane kernel (flag 13) reads it: a 128-B line
 *         then holds one channel chunk of two neighbouring pixels, the halves of a row's two planes staged three K-steps apart, instead of
 *         two chunks of one pixel staged nine K-steps apart, by when the line has left the L2 (every line was fetched twice);
 *         0 = NHWC.  Same arithmetic, same bits.
 * flag 20: 1 (default) = conv_out (512 -> 32 channels, the moments / mode() epilogue) on its own 32-cout halo tile (conv_out_halo.hip: the
 *         18 x 18 halo of a 16 x 16-pixel tile and the chunk's nine weight tiles staged once per 32-channel chunk); 0 = the generic GEMM.

 * flag 21: 1 (default) = vt_eval_export / vt_eval_merge move the keys 16 B per lane on the 16-B aligned part of every destination run;
 *         0 = 8 B per lane throughout.  Same bytes out (tools/bench_eval.py --merge times both).
 * flag 22: 0 (default) = Upsample2D (nearest 2x + 3x3 conv) runs folded, as four 2x2 phase convs of the low-resolution input
 *         (conv3x3_up2.hip: 4 taps per output pixel instead of 9, no 4x-sized intermediate tensor); 1 = the literal route, a nearest-2x
 *         pass into a 16-bit buffer followed by the stride-1 3x3 conv -- the A/B partner and on-device cross-check, and what a channel
 *         count the folded kernel refuses takes either way.  The two differ by accumulation order and by the folded weights' one rounding.
 *         The data gradient vt_op_upsample2x_conv3x3_backward_data follows the same flag: the route of the backward is the route of the forward.
 * flag 23: 0 (default) = vt_op_conv_s2_backward_data runs the scatter kernel (conv3x3_s2_dgrad.hip: 9 products per 2x2 quad of dx); 1 = the
 *         literal route, dy scattered to the odd positions of a zeroed tensor + the stride-1 data gradient (36 products) -- the A/B partner.
 */
int vt_set_flag(vt_context* ctx, int flag, int value);

/* ---- measurement ----------------------------------------------------------------------------
 * Between vt_profile_begin and vt_profile_end every launch of the implicit-GEMM MFMA kernel is
 * bracketed by hipEvents recorded on the launch stream.  vt_profile_end synchronises on them and
 * returns, per kernel/tile configuration (vt_profile_num_configs() of them), the launch count, summed duration (ms) and summed
 * ALGORITHMIC FLOPs (2*B*Hout*Wout*Cout*taps*Cin).  The LAST slot is the HBM-bound GroupNorm(+SiLU) apply
 * pass: its 'flops' entry carries algorithmic BYTES (one read + one bf16 write).  bench.py derives
 * roofline.achieved from these.
 */
/* diagnostics: between vt_debug_trace(ctx, 1, ...) and vt_debug_trace(ctx, 0, sums, max, &n) every GroupNorm of the encoder records two
 * order-independent checksums on the launch stream -- of the (n, mean, M2) partials it consumed and of its (scale, shift) table -- in launch order;
 * the second call synchronises the device and copies them out.  Two runs of the same input give the same list unless some producer's statistics
 * are not deterministic; the first differing index names the layer (tests/diagnostics/gn_trace_diff.py). */
int vt_debug_trace(vt_context* ctx, int enable, unsigned long long* sums_out, int max_sums, int* n_out);
int vt_profile_num_configs(void);
int vt_profile_begin(vt_context* ctx);
int vt_profile_end(vt_context* ctx, int max_cfg, long long* launches, double* total_ms, double* total_flops,
                   const char** kernel_names);

/* ---- the VAE's image decoder: latents -> images ------------------------------------------------
 * diffusers' Decoder for AutoencoderKL: conv_in (latent -> block_out[-1]), mid block (resnet, single-head attention, resnet), one up
 * block per entry of block_out_channels taken in reverse (layers_per_block + 1 resnets each, an Upsample2D -- nearest 2x + 3x3 conv --
 * after all but the last), conv_norm_out + SiLU, conv_out.  Weights are diffusers' `decoder.*` keys (49 545 475 parameters for the FLUX
 * configuration), handed over with vt_set_weight between vt_image_decoder_configure and vt_image_decoder_finalize; the packed weights
 * live in an allocation list of their own, so configuring / finalizing the encoder or the tag decoder leaves them alone and vice versa.
 * GroupNorm eps is 1e-6.  out_channels <= 32 (conv_out rides the 32-cout tiles, zero-padded); conv_in runs over the latent channels
 * zero-padded to a 32-channel chunk; block_out_channels as for the encoder.
 * scaling / shift (with their has_ flags) are the configuration's scaling_factor / shift_factor, used by `unscale` below.
 * Decode runs 16-bit operands everywhere -- bf16, or fp16 with flag 18 where a kernel has that form -- and ignores the fp8 flags
 * (11, 14, 15, 16).  Flags 0-4, 6-10, 12, 13, 17, 18, 20 act as in the encoder; flag 22 selects the Upsample2D route. */
int vt_image_decoder_configure(vt_context* ctx, int out_channels, int latent_channels, const int* block_out_channels, int n_blocks,
                               int layers_per_block, int groups, float scaling, int has_scaling, float shift, int has_shift);
int vt_image_decoder_finalize(vt_context* ctx);
/* bytes of 256-B aligned scratch vt_decode_image needs for B latents of h x w; 0 for an unsupported shape (or before configure) */
size_t vt_decode_image_workspace_bytes(const vt_context* ctx, int B, int h, int w);
/* z: fp32 NCHW [B][latent][h][w] (device).  unscale = 1 applies (z - shift) / scaling first (IEEE fp32: DiffusersVAEWrapper.decode's
 * arithmetic); 0 decodes z as it is (AutoencoderKL.decode).  image_out: fp32 NCHW [B][out_channels][h * 2^(n_blocks-1)][w * 2^(n_blocks-1)],
 * image_bytes its size: VT_ERR_INVALID if that is too small for the result, VT_ERR_WORKSPACE if workspace_bytes is below
 * vt_decode_image_workspace_bytes.  Asynchronous on `stream`; an overflow of the fp16 residual-stream storage raises bit 0 of the sticky
 * status word (vt_status), as in vt_encode.  Bit-identical from run to run. */
int vt_decode_image(vt_context* ctx, const float* z_nchw, int B, int h, int w, int unscale, float* image_out, size_t image_bytes,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- VAE validation loss <- the validation loops of train_vae.py:216-268 and train_full.py:290-338 with the losses of
 * improved_losses.py (ImprovedTripletLoss :81-105, ContrastiveLoss :13-37, CombinedLoss' reconstruction and KL :277-287).  Forward only.
 * Same contract as vt_loss_*: one caller-owned device block (256-B aligned), every size checked on the host before anything is
 * launched -- an undersized buffer is VT_ERR_WORKSPACE, a null / misaligned pointer or an out-of-range argument VT_ERR_INVALID, and
 * nothing is written --, no host synchronisation, no atomics, every sum in fp64 from the fp32 inputs in an order fixed by the shapes
 * alone (partials per 4096 elements, added in index order by a second launch): bit-identical from run to run.
 *
 * vt_posterior_sample: moments fp32 NCHW [B][2C][hw] (mean | logvar, vt_encode mode 0); logvar is clamped to [-30, 20].
 *   z_out (fp32 [B][C][hw], may be NULL) = mean + std eps with std = fp32(exp(0.5 logvar)), as ONE fused fp32 multiply-add fma(std, eps, mean): a single rounding;
 *   kl_out (fp64 [B], may be NULL) = 0.5 sum(mean^2 + var - 1 - logvar).  eps is a counter-based standard normal keyed on
 *   (seed, draw) and (first_image + b, element index within the image): two 64-bit words of vt_head_mix64, u1 = ((x1 >> 11) + 1) 2^-53
 *   in (0, 1], u2 = (x2 >> 11) 2^-53, eps = fp32(sqrt(-2 ln u1) cos(2 pi u2)) evaluated in fp64.  An image's noise depends on its
 *   global index, not on the batching.
 * vt_vae_loss_update: anchor / positive / negative (negative may be NULL: contrastive only) each give `z` fp32 [B][C][hw], or
 *   `moments` to sample z in flight with (seed of reset, draw, first_image) -- the same bits vt_posterior_sample writes, never stored --,
 *   or both (z is used, moments give the KL).  moments == NULL: that stream contributes no KL (kl_mean divides by the streams that do).
 *   recon and target fp32 [B][3][H][W], both or neither; labels_a and labels_p [B][N] VT_F32 or VT_U8, both or neither (then N = 0).
 *   Per image i (row of rows_out, fp64 [B][VT_VAE_LOSS_ROW], may be NULL):
 *     0 mse | 1 kl_a | 2 kl_p | 3 kl_n | 4 kl_mean | 5 log1p(kl_mean / 10000) | 6 pos cosine distance | 7 neg cosine distance |
 *     8 pos euclidean distance | 9 neg euclidean distance | 10 triplet (cosine) | 11 triplet (euclidean) | 12 contrastive (cosine) |
 *     13 contrastive (euclidean) | 14 sum labels_a | 15 overlap | 16 union | 17 triplet weight | 18 label similarity
 *   cosine distance = 1 - a.p / (max(|a|, 1e-12) max(|p|, 1e-12)); euclidean = sqrt(sum (a - p + 1e-6)^2);
 *   triplet = max(pos - neg + margin_triplet, 0) (1 + 0.5 overlap / (sum labels_a + 1e-8)) (weight 1 without labels);
 *   contrastive, with s = overlap / (union + 1e-8): s > jaccard_threshold ? s pos^2 : (1 - s) max(margin_contrastive - pos, 0)^2.
 *   Block: params { fp64 margin_triplet, margin_contrastive, jaccard_threshold, uint64 seed } at 0 | totals at 256 { fp64 [7] sums over
 *   the updates of the per-batch components (mse, kl_mean, log1p(kl_mean / 10000) of the BATCH's kl_mean, triplet cos, triplet euclid,
 *   contrastive cos, contrastive euclid: each the mean over the batch), fp64 [7] sums over the images of the per-image values, added
 *   one image after the other -- independent of the batching --, uint64 [7] updates, images, non-finite inputs, updates with recon,
 *   images with recon, updates with a negative, images with a negative } | scratch of the last update from 512.
 * vt_vae_loss_state_bytes: the block for updates of up to B images of C x hw latents and H x W images; 0 if out of range.
 * vt_vae_loss_read copies the first VT_VAE_LOSS_HEAD_BYTES bytes (params and totals) in stream order into device or pinned host memory. */
#define VT_VAE_LOSS_ROW 19
#define VT_VAE_LOSS_HEAD_BYTES 512
typedef struct { const float* moments; const float* z; int draw; } vt_vae_loss_input;
int vt_posterior_sample(vt_context* ctx, const float* moments, int B, int C, int hw, unsigned long long seed, int draw,
                        long long first_image, float* z_out, double* kl_out, void* stream);
/* vt_posterior_mode_latent: the tag decoder's input in train_full, DiffusersVAEWrapper.encode's latent from moments that are already there.
 *   moments fp32 NCHW [B'][2C][hw] with B' >= B (only the first B images are read: the anchors of an [a; p; n] encoder pass);
 *   latent_out fp32 [B][C][hw] = mean * scaling + shift, the multiply only with has_scaling and the add only with has_shift (the
 *   configuration's flags), each rounded on its own in fp32 -- the bits of torch's two eager ops.  One pass, float4 loads and stores when
 *   C * hw % 4 == 0 and both pointers are 16-B aligned, else one guarded float at a time.  A null or misaligned pointer, a shape out of
 *   range or a non-finite factor whose flag is set is VT_ERR_INVALID, and nothing is written. */
int vt_posterior_mode_latent(vt_context* ctx, const float* moments, int B, int C, int hw, float scaling, int has_scaling, float shift,
                             int has_shift, float* latent_out, void* stream);
size_t vt_vae_loss_state_bytes(int B, int C, int hw, int H, int W);
int vt_vae_loss_reset(vt_context* ctx, void* state, size_t state_bytes, double margin_triplet, double margin_contrastive,
                      double jaccard_threshold, unsigned long long seed, void* stream);
int vt_vae_loss_update(vt_context* ctx, void* state, size_t state_bytes, const vt_vae_loss_input* anchor, const vt_vae_loss_input* positive,
                       const vt_vae_loss_input* negative /* or NULL */, const float* recon, const float* target, int H, int W,
                       const void* labels_a, const void* labels_p, int labels_dtype /* VT_F32 | VT_U8 */, int N, int B, int C, int hw,
                       long long first_image, double* rows_out /* [B][VT_VAE_LOSS_ROW] or NULL */, void* stream);
int vt_vae_loss_read(vt_context* ctx, const void* state, size_t state_bytes, void* out, size_t out_bytes, void* stream);

/* ---- gradient of the VAE's training loss <- one step of train_vae.py:131-179:
 *   total = w_rec mse_loss(recon, target) + w_kl log(1 + kl_mean / 10000) + w_tri ImprovedTripletLoss(z_a, z_p, z_n, labels_a, labels_p)
 * with kl_mean the batch mean of (kl_a + kl_p + kl_n) / 3 and the triplet term the batch mean of the weighted hinge, cosine or euclidean
 * (`similarity`).  --use_simplified_vae_loss is w_kl = 0.  The contrastive term has no gradient here: a call without a negative stream is
 * refused.  Self-contained: it reads and writes no vt_vae_loss_* state block, recomputes the per-image sums with the forward's own device
 * functions, and regenerates every eps from the counter (seed, draw, first_image + b, element): anchor / positive / negative give
 * `moments` (fp32 NCHW [B][2C][hw]) and `draw`, and `z` must be NULL.  Same discipline as the forward: sizes checked on the host before
 * anything is launched (VT_ERR_WORKSPACE for a small workspace, VT_ERR_INVALID for a null / misaligned pointer, an out-of-range shape, a
 * missing negative, a non-finite weight or margin; nothing is written), one stream, no host synchronisation, no atomics, fp64 arithmetic
 * from the fp32 inputs with one rounding at the store, bit-identical from run to run.
 *   dz_dec (fp32 [B][C][hw] or NULL): the gradient of the latent the image was decoded from, sampled from the ANCHOR's moments with draw
 *     `dz_draw`; it is added to the anchor's d mean and, under that draw's eps, to its d logvar.
 *   recon, target fp32 [B][3][H][W], both or neither (then the reconstruction term is 0); labels as vt_vae_loss_update takes them.
 * Outputs, each may be NULL:
 *   d_recon fp32 [B][3][H][W] = w_rec 2 (recon - target) / (B 3HW);
 *   d_moments_a / _p / _n fp32 [B][2C][hw]: d mean = g + c_kl mean, d logvar = in_clamp (0.5 sum_draws g std eps + c_kl 0.5 (var - 1)) with
 *     g the element's d total / d z (the triplet term; for the anchor's decode draw, dz_dec), c_kl = w_kl / (3 B 10000 (1 + kl_mean / 10000)),
 *     std = fp32(exp(0.5 logvar)) as the forward rounds it, var = exp(0.5 logvar)^2 in fp64, and in_clamp = 1 for -30 <= logvar <= 20
 *     (inclusive, as torch.clamp's backward), else 0.  The hinge has derivative 0 at 0;
 *   rows_out fp64 [B][VT_VAE_LOSS_ROW]: vt_vae_loss_update's columns with margin_triplet = margin, the same bits; the contrastive
 *     columns 12 and 13 are 0;
 *   loss_out fp64 [4]: reconstruction, kl (log1p of the batch's kl_mean / 10000), triplet (of `similarity`) and total, each batch sum
 *     taken one image after the other.
 * workspace: 256-B aligned, vt_vae_loss_backward_workspace_bytes(B, C, hw, H, W) bytes (0: shape out of range; H = W = 0: no image). */
#define VT_VAE_COSINE 0
#define VT_VAE_EUCLIDEAN 1
size_t vt_vae_loss_backward_workspace_bytes(int B, int C, int hw, int H, int W);
int vt_vae_loss_backward(vt_context* ctx, const vt_vae_loss_input* anchor, const vt_vae_loss_input* positive, const vt_vae_loss_input* negative,
                         const float* dz_dec /* or NULL */, int dz_draw, const float* recon, const float* target, int H, int W,
                         const void* labels_a, const void* labels_p, int labels_dtype /* VT_F32 | VT_U8 */, int N, int B, int C, int hw,
                         unsigned long long seed, long long first_image, double w_rec, double w_kl, double w_tri, double margin,
                         int similarity /* VT_VAE_COSINE | VT_VAE_EUCLIDEAN */, float* d_recon, float* d_moments_a, float* d_moments_p,
                         float* d_moments_n, double* rows_out, double* loss_out /* [4] */, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the optimiser of the VAE train step (csrc/vae_optim.hip): clip_grad_norm_ and AdamW over n gradient tensors where they lie ----
 * The parameters live in one fp32 arena, the Adam moments m and v in two more of the same layout: tensor i owns a slot of
 * ceil(numel[i] / VT_VAE_OPTIM_TILE) tiles of VT_VAE_OPTIM_TILE floats, slots follow each other in the order given, so a tile never
 * straddles two tensors and every slot is 16-B aligned; the padding is zero and stays zero (it is never read from a gradient and
 * never stored).  vt_vae_optim_layout is that rule as a pure host function: offsets_out[i] (floats; may be NULL) and *total_out (may
 * be NULL); VT_ERR_INVALID for n < 1, a null numel or a numel <= 0.
 * `grads` is a HOST array of n device pointers (fp32, contiguous, 4-B aligned; a 16-B aligned one takes the float4 path), `numel` a HOST
 * array; both are read during the call only.  They travel in kernel arguments, `chunk` tensors per launch (0: VT_VAE_OPTIM_CHUNK, else 1
 * .. VT_VAE_OPTIM_CHUNK): no host-to-device copy, no staging, no allocation, no host synchronisation; the results do not depend on `chunk`.
 * Everything is checked on the host before anything is launched: null / misaligned pointer, n < 1, numel <= 0, max_norm <= 0, an arena
 * smaller than the layout's total or an out-of-range optimiser argument is VT_ERR_INVALID, a small workspace VT_ERR_WORKSPACE, and a
 * refused call writes nothing.
 *   vt_vae_optim_norm   one workgroup per tile squares in fp64 and writes one fp64 partial at the tile's global index (workspace: 256-B
 *                       aligned, vt_vae_optim_workspace_bytes(numel, n) bytes, 0 for arguments the call would refuse); a last
 *                       single-workgroup launch adds the partials in an order fixed by their count and writes scalars_out (device, 16-B aligned) =
 *                       { fp64 norm^2, fp32 norm = (float)sqrt(norm^2), fp32 coef = min(1, max_norm / (norm + 1e-6f)) }, vt_head_clip's
 *                       formula.  No atomics; bit-identical from run to run; the gradients are not written.
 *   vt_vae_optim_step   AdamW's update number t (1-based) as vt_head_step, per element the same source; with `scalars` (device, what
 *                       vt_vae_optim_norm wrote; may be NULL) and coef < 1 the gradient is first multiplied by coef, one fp32 multiply
 *                       with one rounding.  Reads g, p, m, v and writes p, m, v: the gradients are neither zeroed nor written.
 *                       arena_floats: the floats each of params / m / v (256-B aligned) holds. */
#define VT_VAE_OPTIM_TILE 4096
#define VT_VAE_OPTIM_CHUNK 64
int vt_vae_optim_layout(const long long* numel /* host [n] */, int n, long long* offsets_out /* host [n] or NULL */, long long* total_out);
size_t vt_vae_optim_workspace_bytes(const long long* numel /* host [n] */, int n);
int vt_vae_optim_norm(vt_context* ctx, const float* const* grads /* host [n] */, const long long* numel /* host [n] */, int n, float max_norm,
                      void* scalars_out, void* workspace, size_t workspace_bytes, int chunk, void* stream);
int vt_vae_optim_step(vt_context* ctx, float* params, float* m, float* v, size_t arena_floats, const float* const* grads /* host [n] */,
                      const long long* numel /* host [n] */, int n, const void* scalars /* or NULL */, double lr, double beta1, double beta2,
                      double eps, double weight_decay, long long t, int chunk, void* stream);
/* vt_full_optim_norm: train_full's ONE clip_grad_norm_ over the VAE's gradient tensors and the tag decoder's state blocks together.
 * The first ten arguments are vt_vae_optim_norm's and mean the same; n may be any prefix of a trainer's tensors (the encoder's come first in
 * its arenas, so the encoder-only step of the simplified loss is a smaller n on the same arenas).  head_state is the head's block
 * (vt_head_state_bytes), front_state and cross_state the front's and the cross-attention's, each NULL with size 0 when absent (the plain
 * decoder has only the head; the cross-attention's comes with the front's); they are checked as vt_head_clip / vt_train_clip /
 * vt_train_clip3 check them.  The VAE's per-tile partials are written exactly as vt_vae_optim_norm writes them; one single-workgroup
 * launch then forms S_vae in vt_vae_optim_norm's order, S_blocks in vt_train_clip's (the head's partials in index order, then the
 * front's, then the cross-attention's), total = S_vae + S_blocks (one fp64 add), norm = (float)sqrt(total), coef = min(1, max_norm /
 * (norm + 1e-6f)), and writes the same 16 bytes to scalars_out and to every present block's scalars.  The blocks' gradients are then
 * scaled in place as vt_train_clip scales them; the VAE's gradients are NOT written -- vt_vae_optim_step folds the coefficient in.
 * No atomics, no host synchronisation; bit-identical from run to run and under any `chunk`; a refused call writes nothing. */
int vt_full_optim_norm(vt_context* ctx, const float* const* grads /* host [n] */, const long long* numel /* host [n] */, int n, float max_norm,
                       void* scalars_out, void* workspace, size_t workspace_bytes, int chunk, void* head_state, size_t head_state_bytes,
                       void* front_state /* or NULL */, size_t front_state_bytes, void* cross_state /* or NULL */, size_t cross_state_bytes,
                       void* stream);
/* The gradient exchange of a sharded train_vae: the gradient as ONE row of the arenas' layout, so that rank r of K
 * can own the tiles [r S, (r + 1) S), S = ceil(tiles / K), merge only those and gather the rest.  `grads`, `numel`, n and `chunk` as above.
 *   vt_vae_grads_export  writes EVERY float of row[0, row_floats) (device, 256-B aligned; row_floats a multiple of VT_VAE_OPTIM_TILE, at
 *                        least the layout's total): tensor i at its slot offset, zero in the rest of its last tile and from the total on.
 *                        No memset is needed before it; elements past numel[i] are never loaded; the bits do not depend on `chunk` or on
 *                        a gradient's alignment.
 *   vt_vae_grads_merge   for e in [0, floats): out[e] = (float)acc with acc = weights[0] * (double)x_0, then for r = 1 .. K-1 in that order
 *                        acc = acc + weights[r] * (double)x_r, x_r = rows[r * row_stride_floats + first_float + e]; every product and
 *                        every sum is rounded to fp64 on its own.  The first product is NOT added to 0.0: K = 1 with weight 1 is the
 *                        identity, -0.0 included.  `weights`: K HOST doubles, finite and non-negative, read during the call; 1 <= K <= 64;
 *                        first_float and floats multiples of VT_VAE_OPTIM_TILE, floats > 0, first_float + floats <= row_stride_floats (a
 *                        multiple of 4); rows and out 16-B aligned device memory that do not overlap.  One workgroup per tile, no atomics:
 *                        merging a range in one call or in pieces gives the same bytes.
 * vt_vae_optim_norm and vt_vae_optim_step then run unchanged on pointers INTO the merged row (slot offsets are multiples of the tile).
 * A refused call (VT_ERR_INVALID) launches nothing; nothing synchronises the host. */
int vt_vae_grads_export(vt_context* ctx, const float* const* grads /* host [n] */, const long long* numel /* host [n] */, int n, float* row,
                        size_t row_floats, int chunk, void* stream);
int vt_vae_grads_merge(vt_context* ctx, const float* rows, size_t row_stride_floats, int K, const double* weights /* host [K] */,
                       size_t first_float, size_t floats, float* out, void* stream);
/* vt_vae_grads_accumulate: gradient accumulation of train_full -- the n fresh gradient tensors of one micro-step
 * into ONE fp32 row of the arenas' layout that holds the sum across micro-steps.  `grads`, `numel`, n, `chunk`, `row` and `row_floats` as
 * for vt_vae_grads_export.  Per element g of tensor i, at its slot:
 *   t = scale * g                one fp32 multiply; scale == 1 leaves the bits, -0.0 included
 *   first != 0:  row = t         and +0.0 in the rest of the tensor's last tile and from the layout's total to row_floats: every float of
 *                                the row is written, no memset is needed, and with scale == 1 the row is vt_vae_grads_export's byte for byte
 *   first == 0:  a = row; if `scalars` (device TrainScalars, 16-B aligned, or NULL) holds a coef (fp32 at byte 12) < 1, a = coef * a, one
 *                fp32 multiply rounded on its own; row = a + t, one fp32 add.  Two products and one add, three separately rounded
 *                operations, never a fused multiply-add.  A NaN or >= 1 coef multiplies nothing (vt_vae_optim_step's rule).  Padding is
 *                neither read nor written.
 * So the coefficient that the clip of the PREVIOUS micro-step wrote is applied to the accumulated row here, as the row is read anyway, and
 * not by a pass of its own.  One 256-thread workgroup per tile, no atomics; elements past numel[i] are never loaded; the bits do not depend
 * on `chunk` or on a gradient's alignment.  VT_ERR_INVALID, with nothing launched: n < 1, a null grads / numel / row, a numel <= 0, a
 * misaligned or short row, a non-finite scale, misaligned scalars, a chunk outside 0 .. VT_VAE_OPTIM_CHUNK.  No host synchronisation. */
int vt_vae_grads_accumulate(vt_context* ctx, const float* const* grads /* host [n] */, const long long* numel /* host [n] */, int n,
                            float* row, size_t row_floats, float scale, const void* scalars /* device TrainScalars, or NULL */, int first,
                            int chunk, void* stream);

/* ---- single operators (parity tests drive each kernel through the same ABI) ------------------
 * NHWC bf16 activations, weights in the reference's own layouts (fp32 host order is converted by
 * the caller to bf16 [Cout][kh][kw][Cin]); fp32 accumulate.
 */
int vt_op_conv2d(vt_context* ctx, const void* x_bf16_nhwc, const void* w_bf16_ohwi, const float* bias,
                 const float* residual_f32, float* out_f32, void* out_bf16, int B, int Hin, int Win, int Cin,
                 int Cout, int ksize, int stride, int pad_lo, int pad_hi, void* stream);
/* 3x3 stride-1 pad-1 conv of silu(x*scale + shift): x is fp32 or bf16 NHWC, scale_shift [B][Cin][2]; the
 * normalise + SiLU runs inside the conv's LDS staging (no separate pass).  Cin % 32 == 0, Cout % 128 == 0. */
int vt_op_norm_silu_conv3x3(vt_context* ctx, const void* x_nhwc, int x_dtype, const float* scale_shift,
                            const void* w_bf16_ohwi, const float* bias, const float* residual_f32, float* out_f32,
                            void* out_bf16, int B, int H, int W, int Cin, int Cout, void* stream);
/* conv2d whose epilogue also produces the GroupNorm statistics of its output: returns per (image, channel)
 * (scale, shift) with GroupNorm(out) = out*scale + shift.  The encoder uses this fusion between layers. */
size_t vt_op_conv2d_gn_workspace_bytes(int B, int Hout, int Wout, int Cout);
int vt_op_conv2d_gn(vt_context* ctx, const void* x_bf16_nhwc, const void* w_bf16_ohwi, const float* bias,
                    const float* residual_f32, float* out_f32, void* out_bf16, int B, int Hin, int Win, int Cin,
                    int Cout, int ksize, int stride, int pad_lo, int pad_hi, int groups, float eps, const float* gamma,
                    const float* beta, float* scale_shift_out, void* workspace, void* stream);
/* Upsample2D of the VAE decoder as a single operator: out = conv3x3(nearest_2x(x)) + bias, stride 1, pad 1, Cin == Cout == C.
 * x is the LOW-resolution tensor, NHWC 16-bit [B][h][w][C] (bf16; fp16 bits with flag 18); w fp32 OIHW [C][C][3][3] ON THE DEVICE, packed
 * inside the call on the stream; out fp32 NHWC [B][2h][2w][C].  By default the folded kernel runs (conv3x3_up2.hip: four 2x2 phase convs
 * of the low-resolution input with pre-summed weights -- each folded weight is the fp32 sum, ky-major then kx, of 1, 2 or 4 original taps,
 * rounded to the operand type once; C % 64 == 0); with flag 22, or for a C the folded kernel refuses, the literal route: a nearest-2x pass
 * into a 16-bit buffer, then the stride-1 3x3 conv (C % 8 == 0; fp16 operands only where the halo conv has that form).  Scratch comes
 * from the context (grown on demand: the first call of a size may synchronise).  No atomics: bit-identical from run to run.
 * _gn additionally returns the GroupNorm (scale, shift) [B][C][2] of the OUTPUT from the epilogue's (n, mean, M2) partials, finalised
 * as vt_op_conv2d_gn does (C / groups in {4, 8, 16}; bias required). */
int vt_op_upsample2x_conv3x3(vt_context* ctx, const void* x_bf16_nhwc, const float* w_f32_oihw, const float* bias, float* out_f32,
                             int B, int h, int w, int C, void* stream);
int vt_op_upsample2x_conv3x3_gn(vt_context* ctx, const void* x_bf16_nhwc, const float* w_f32_oihw, const float* bias, float* out_f32,
                                int B, int h, int w, int C, int groups, float eps, const float* gamma, const float* beta,
                                float* scale_shift_out, void* stream);
/* the fp8 conv of flag 11 as a single operator: x fp32 NHWC and w fp32 OIHW (both on the device) are quantised exactly as the
 * encoder quantises them (x -> e4m3(8 x), w -> e4m3 with per-cout absmax scales); out fp32 NHWC.  Cin % 64 == 0, Cout % 128 == 0. */
size_t vt_op_conv3x3_fp8_workspace_bytes(int B, int H, int W, int Cin, int Cout);
int vt_op_conv3x3_fp8(vt_context* ctx, const float* x_f32_nhwc, const float* w_f32_oihw, const float* bias, const float* residual_f32,
                      float* out_f32, int B, int H, int W, int Cin, int Cout, int stride /* 1: pad 1; 2: pad (0,1,0,1), x -> e4m3(x) */,
                      void* workspace, void* stream);
/* One 3x3 conv of a ResnetBlock2D / Downsample2D in the forms the VAE schedules launch by default, through their own dispatcher
 * (run_conv: flags 0, 3, 13 and 18 pick the kernel exactly as in vt_encode) and their own weight packers.  stride 1 (pad 1) or 2 (pad
 * (0,1,0,1), out H / 2 x W / 2).  Cin % 32 == 0, Cout % 128 == 0 (what both halo kernels take).
 *   x16       16-bit NHWC [B][H][W][Cin]; with x_planar (stride 2 only) chunk-planar, [Cin/32][H][W][32] per image.  bf16, or fp16 bits
 *             when flag 18 is on -- then the conv must have an fp16-operand kernel under the current flags, else VT_ERR_INVALID.
 *   w, bias   fp32 OIHW [Cout][Cin][3][3] and [Cout] ON THE DEVICE; bias is the launch's final bias (conv2's + the shortcut's).  Copied to
 *             the host, packed by the finalizers' routines, uploaded and freed inside the call: synchronises.
 *   sc_x16, sc_w   optional fused conv_shortcut (stride 1, no residual): 16-bit NHWC [B][H][W][sc_cin] of x16's type and fp32 [Cout][sc_cin]
 *             (device), sc_cin % 32 == 0; runs as sc_cin / 32 extra K-steps at the centre tap.
 *   residual, out   the residual stream in and out, [B][Ho][Wo][Cout], each optional, VT_F32 or VT_F16 (res_dtype, out_dtype: one type
 *             for both when both are given -- the stream has one).
 *   out16     optional 16-bit operand copy of the output: bf16, or fp16 bits with out16_f16; NHWC, or with out16_planar (stride 1)
 *             chunk-planar [Cout/32][H][W][32] per image, element (b, y, x, c) at (((b * (Cout/32) + c/32) * H + y) * W + x) * 32 + c % 32.
 *   scale_shift_out   optional [B][Cout][2]: GroupNorm (scale, shift) of the output from the epilogue's (n, mean, M2) partials, finalised
 *             as vt_op_conv2d_gn does (Cout / groups in {4, 8, 16}; gamma, beta [Cout]); workspace (256-B aligned, >=
 *             vt_op_conv3x3_block_workspace_bytes) holds the partials and is needed only then.
 * Every combination is checked on the host first: what the dispatcher or a launcher refuses (a shortcut or a planar copy off the halo
 * kernel, planar input at stride 1, an fp16 residual with an fp32 output, fp16 operands where no kernel has them, ...) returns an error
 * code with a message and writes nothing. */
size_t vt_op_conv3x3_block_workspace_bytes(int B, int H, int W, int Cout, int stride);
int vt_op_conv3x3_block(vt_context* ctx, const void* x16, int x_planar, const float* w_f32_oihw, const float* bias, const void* sc_x16,
                        const float* sc_w_f32, int sc_cin, const void* residual, int res_dtype, void* out, int out_dtype, void* out16,
                        int out16_f16, int out16_planar, int B, int H, int W, int Cin, int Cout, int stride, int groups, float eps,
                        const float* gamma, const float* beta, float* scale_shift_out, void* workspace, size_t workspace_bytes, void* stream);
int vt_op_gemm_nt(vt_context* ctx, const void* a_bf16, const void* b_bf16, const float* bias, float* out_f32,
                  void* out_bf16, int batch, int M, int N, int K, int lda, int ldb, int ldo, long long a_bs,
                  long long b_bs, long long o_bs, float alpha, int bias_per_row, void* stream);
int vt_op_conv_in(vt_context* ctx, const float* x_nchw, const float* w_oihw, const float* bias, float* out_f32,
                  void* out_bf16, int B, int H, int W, int Cout, void* workspace, void* stream);
size_t vt_op_groupnorm_workspace_bytes(int B, int HW, int C);
int vt_op_groupnorm(vt_context* ctx, const void* x, int x_dtype, int B, int HW, int C, int groups, float eps,
                    const float* gamma, const float* beta, int silu, void* y_bf16, void* workspace, void* stream);
int vt_op_softmax_rows(vt_context* ctx, const float* scores, void* probs_bf16, int rows, int n, int lds, int ldp,
                       void* stream);
/* ---- backward of one ResnetBlock2D's layers (the block both VAE models consist of).  All gradients fp32, all MFMA operands bf16 with fp32
 * accumulation whatever flag 18 says; no atomics, every result bit-identical from run to run; one stream, no host synchronisation (the data
 * gradient takes its scratch from the context: the first call of a size may synchronise).  vae_tagger_amd/vae_backward.py composes them.
 *
 * vt_op_cast_bias_grad: one pass over dy (fp32 [rows][C], rows = B*H*W): dy16 = bf16(dy), round to nearest even, and dbias[c] = sum over rows
 * (either output may be NULL).  Sums: fp64 per lane, per row chunk, then a fixed-order fp64 finish.  C % 4 == 0, C <= 1024; workspace only
 * with dbias. */
size_t vt_op_cast_bias_grad_workspace_bytes(long long rows, int C);
int vt_op_cast_bias_grad(vt_context* ctx, const float* dy_f32, void* dy16_out, float* dbias_out, long long rows, int C, void* workspace,
                         size_t workspace_bytes, void* stream);
/* Data gradient of a stride-1 conv, 3x3 pad 1 or 1x1: dx[b][y][x][ci] = sum dy16[b][y+1-ky][x+1-kx][co] * bf16(W[co][ci][ky][kx]) (+ dx_add),
 * fp32 NHWC.  W is the conv's fp32 OIHW parameter ON THE DEVICE; it is packed (rotated by 180 degrees, transposed in (co, ci), rounded to bf16)
 * on the stream and the forward stride-1 conv vt_op_conv2d runs is launched on it.  dy16 bf16 NHWC [B][H][W][Cout]; dx_add optional fp32
 * [B][H][W][Cin] (the conv's residual input).  Cin % 8 == 0, Cout % 8 == 0. */
int vt_op_conv_backward_data(vt_context* ctx, const void* dy16_nhwc, const float* w_f32_oihw, const float* dx_add, float* dx_f32, int B, int H,
                             int W, int Cin, int Cout, int ksize, void* stream);
/* Weight gradient of the same convs: dw[co][ci][ky][kx] = sum_{b,y,x} dy16[b][y][x][co] * a16[b][y+ky-1][x+kx-1][ci] (taps outside the image
 * count as 0), fp32 OIHW.  a16 is the conv's forward operand, bf16 NHWC [B][H][W][Cin].  The pixels are cut into `splits` slices (0: chosen from
 * the shape so that workgroups ~ twice the CU count, two being resident per CU; more than the number of pixel steps: clamped); each slice writes a partial dw to the
 * workspace, a second launch adds them in slice order.  Cin % 64 == 0, Cout % 64 == 0, ksize 1 or 3, any B, H, W >= 1.  The workspace must
 * be sized with the same `splits`. */
size_t vt_op_conv_backward_weight_workspace_bytes(int B, int H, int W, int Cin, int Cout, int ksize, int splits);
int vt_op_conv_backward_weight(vt_context* ctx, const void* dy16_nhwc, const void* a16_nhwc, float* dw_f32_oihw, int B, int H, int W, int Cin,
                               int Cout, int ksize, int splits, void* workspace, size_t workspace_bytes, void* stream);
/* ---- backward of the two resampling layers.  Precision and discipline as above: bf16 MFMA operands with fp32 accumulation
 * whatever flag 18 says, fp32 gradients, one stream, no atomics, bit-identical from run to run and across any `splits`.
 *
 * Downsample2D, y = conv3x3(pad(x, (0,1,0,1)), W), stride 2, Ho = H / 2, Wo = W / 2 (odd H, W are legal; H, W >= 2).
 * Data gradient: dx[b][2i+a][2j+a'][ci] by the parity of the output pixel -- row phase a = 0 takes ky 0 from dy row i and ky 2 from dy row i - 1,
 * phase a = 1 takes ky 1 from dy row i, columns alike, dy outside [0, Ho) x [0, Wo) = 0 -- on bf16(W), 9 (phase, tap) products per 2x2 quad
 * (conv3x3_s2_dgrad.hip; Cin % 64 == 0, Cout % 64 == 0).  With vt_set_flag(ctx, 23, 1), or channel counts that kernel refuses (multiples of 8), the
 * literal route: dy16 scattered to the odd positions of a zeroed H x W tensor, then vt_op_conv_backward_data's launch.  dy16 bf16 NHWC
 * [B][Ho][Wo][Cout], W fp32 OIHW on the device, dx_add optional fp32 [B][H][W][Cin], dx fp32 [B][H][W][Cin]; scratch from the context. */
int vt_op_conv_s2_backward_data(vt_context* ctx, const void* dy16_nhwc, const float* w_f32_oihw, const float* dx_add, float* dx_f32, int B, int H, int W,
                                int Cin, int Cout, void* stream);
/* Weight gradient: dw[co][ci][ky][kx] = sum_{b,i,j} dy16[b][i][j][co] * a16[b][2i+ky][2j+kx][ci], a16 (bf16 NHWC [B][H][W][Cin], the layer's input)
 * outside the image = 0.  `splits`, the workspace and the channel rule as vt_op_conv_backward_weight. */
size_t vt_op_conv_s2_backward_weight_workspace_bytes(int B, int H, int W, int Cin, int Cout, int splits);
int vt_op_conv_s2_backward_weight(vt_context* ctx, const void* dy16_nhwc, const void* a16_nhwc, float* dw_f32_oihw, int B, int H, int W, int Cin, int Cout,
                                  int splits, void* workspace, size_t workspace_bytes, void* stream);
/* Upsample2D, y = conv3x3(nearest2x(x), W) as vt_op_upsample2x_conv3x3 computes it; h, w >= 1 are the LOW resolution.
 * Data gradient: the route follows the forward's.  Default: the exact adjoint of the folded forward -- dx[i][j] = sum over the 16 (phase, tap)
 * pairs of Wf^T[phase][tap] . dy16[2 (i + 1 - ry - a) + a][2 (j + 1 - rx - a') + a'], Wf the forward's folded matrices (fp32 sum ky-major then kx,
 * rounded to bf16 once), a 4x4 stride-2 gather (conv3x3_up2_dgrad.hip; C % 64 == 0).  With flag 22 (literal forward), or a C that kernel
 * refuses (multiples of 8): vt_op_conv_backward_data's launch on bf16(W) at 2h x 2w, then the 2x2 sum ((00 + 01) + 10) + 11.  dy16 bf16
 * [B][2h][2w][C], dx_add optional and dx fp32 [B][h][w][C]; scratch from the context. */
int vt_op_upsample2x_conv3x3_backward_data(vt_context* ctx, const void* dy16_nhwc, const float* w_f32_oihw, const float* dx_add, float* dx_f32, int B, int h,
                                           int w, int C, void* stream);
/* Weight gradient: dw[co][ci][ky][kx] = sum_P dy16[P][co] * x16[(P + (ky-1, kx-1)) >> 1][ci] over the high-resolution pixels P, the bounds tested
 * before the shift; x16 bf16 NHWC [B][h][w][C] (no upsampled tensor is written).  `splits` and the workspace as vt_op_conv_backward_weight. */
size_t vt_op_upsample2x_conv3x3_backward_weight_workspace_bytes(int B, int h, int w, int C, int splits);
int vt_op_upsample2x_conv3x3_backward_weight(vt_context* ctx, const void* dy16_nhwc, const void* x16_nhwc, float* dw_f32_oihw, int B, int h, int w, int C,
                                             int splits, void* workspace, size_t workspace_bytes, void* stream);
/* ---- the two full-resolution end convs of the VAE, 3 channels on one side: encoder.conv_in 3 -> C, decoder.conv_out C -> 3.
 *
 * vt_op_conv_thin_backward_weight: their weight gradient, a [27 -> 32 rows] x Cw matrix with the pixel index as K.  `thin` is the 3-channel side,
 * fp32 NCHW [B][3][H][W] (conv_in's image; conv_out's loss gradient); it enters the MFMA split, hi = bf16(v), lo = bf16(v - hi), two MFMAs per
 * K-step into the same fp32 accumulators, so its side of every product is fp32-grade.  `wide` is bf16 NHWC [B][H][W][Cw].
 *   thin_is_input = 1 (conv_in; wide = dy16):  dw[c][t][ky][kx] = sum_{b,y,x} wide[b][y][x][c] * thin[b][t][y+ky-1][x+kx-1], fp32 OIHW [Cw][3][3][3]
 *   thin_is_input = 0 (conv_out; wide = a16, the conv's forward operand; thin = dy):
 *                                               dw[t][c][ky][kx] = sum_{b,y,x} thin[b][t][y][x] * wide[b][y+ky-1][x+kx-1][c], fp32 OIHW [3][Cw][3][3]
 * Taps outside the image count as 0.  thin_sums_out (optional) [3] = sum_{b,y,x} thin[b][t][y][x] (conv_out's bias gradient): fp64 partials per
 * workgroup, finished in a fixed order.  The pixels are cut into `splits` slices (0: chosen from the shape so that the workgroups fill three slots on
 * each of the 256 CUs; more than the number of pixel tiles: clamped); each slice writes an fp32 partial to the workspace, a second launch adds them
 * in slice order.  No atomics, bit-identical from run to run; on exact data independent of `splits`.  Cw % 64 == 0, Cw <= 512, any B, H, W >= 1.  The
 * workspace (16-byte aligned) must be sized with the same `splits`.  One stream, no host synchronisation; refused while flag 18 is on; a refused
 * call writes nothing. */
size_t vt_op_conv_thin_backward_weight_workspace_bytes(int B, int H, int W, int Cw, int splits);
int vt_op_conv_thin_backward_weight(vt_context* ctx, const float* thin_nchw, const void* wide16_nhwc, int thin_is_input, float* dw_out,
                                    float* thin_sums_out, int B, int H, int W, int Cw, int splits, void* workspace, size_t workspace_bytes, void* stream);
/* vt_op_conv_thin_forward: vt_op_conv_in with the weights packed ON THE STREAM (no host copy, no synchronisation), then the same kernels: the
 * matrix-core one when C == 128 and flag 5 is on, else the fp32 VALU one (C % 8 == 0, C <= 256).  x fp32 NCHW [B][3][H][W]; out_f32 and / or out_bf16 NHWC
 * [B][H][W][C]; bias [C] or NULL (= 0).
 *   transpose_rotate = 0: w is fp32 [C][3][3][3] -- conv_in's forward, bit-identical to vt_op_conv_in on the same weights.
 *   transpose_rotate = 1: w is conv_out's own parameter [3][C][3][3]; the conv runs on W'[c][t][ky][kx] = w[t][c][2-ky][2-kx] with a zero bias
 *     (`bias` is ignored) -- the DATA GRADIENT of conv_out: d image in, dx fp32 NHWC out, at conv_in's fp32-grade products.
 * The workspace (16-byte aligned, vt_op_conv_thin_forward_workspace_bytes(C)) holds the packed weights and the zero bias.  Refused while flag 18 is on. */
size_t vt_op_conv_thin_forward_workspace_bytes(int C);
int vt_op_conv_thin_forward(vt_context* ctx, const float* x_nchw, const float* w, const float* bias, int transpose_rotate, float* out_f32,
                            void* out_bf16, int B, int H, int W, int C, void* workspace, size_t workspace_bytes, void* stream);
/* error while flag 18 (fp16 operands) is on: functions that mix these operators with the forward ones ask here first */
int vt_op_backward_operands_check(vt_context* ctx);
/* (mean, rstd) fp32 [B][groups][2] of an fp32 tensor [B][HW][C], from fp64 sums of x and x^2 taken in a fixed order (the forward's (scale, shift)
 * table cannot stand in: it loses xh wherever gamma = 0).  Same shapes as vt_op_groupnorm_silu_backward. */
size_t vt_op_groupnorm_stats_workspace_bytes(int B, int HW, int C);
int vt_op_groupnorm_stats(vt_context* ctx, const float* x_f32, int B, int HW, int C, int groups, float eps, float* stats_out, void* workspace,
                          size_t workspace_bytes, void* stream);
/* Backward of a = silu(GroupNorm(x)): with xh = (x - mean) rstd, u = gamma xh + beta, s = sigmoid(u), du = da s (1 + u (1 - s)):
 * dbeta[c] = sum du, dgamma[c] = sum du xh, dx = rstd (gamma du - mean_g(gamma du) - xh mean_g(gamma du xh)) (+ dx_add), means over the (C/groups) HW
 * elements of one image's group.  x, da, dx_add, dx fp32 [B][HW][C]; stats from vt_op_groupnorm_stats; dx16 (optional) = bf16(dx); dgamma, dbeta
 * optional.  Two passes over x and da; the sums are fp64 throughout, in a fixed order.  C / groups in {2, 4, 8, 16}, C a power of two <= 1024. */
size_t vt_op_groupnorm_silu_backward_workspace_bytes(int B, int HW, int C);
int vt_op_groupnorm_silu_backward(vt_context* ctx, const float* x_f32, const float* stats, const float* gamma, const float* beta, const float* da_f32,
                                  const float* dx_add, float* dx_f32, void* dx16_out, float* dgamma_out, float* dbeta_out, int B, int HW, int C,
                                  int groups, void* workspace, size_t workspace_bytes, void* stream);
/* The same passes for a GroupNorm WITHOUT activation (the attention block's): du = dh.  Everything else as vt_op_groupnorm_silu_backward. */
size_t vt_op_groupnorm_backward_workspace_bytes(int B, int HW, int C);
int vt_op_groupnorm_backward(vt_context* ctx, const float* x_f32, const float* stats, const float* gamma, const float* beta, const float* dh_f32,
                             const float* dx_add, float* dx_f32, void* dx16_out, float* dgamma_out, float* dbeta_out, int B, int HW, int C, int groups,
                             void* workspace, size_t workspace_bytes, void* stream);

/* ---- Mid-block attention for training.  C = 512 only; any S >= 1.  One stream, no host synchronisation, no atomics.
 *
 * vt_op_attention_forward_train: y = to_out(softmax(q k^T / sqrt(C)) v) + x with h = GroupNorm32(x) (eps 1e-6, no SiLU), on CALLER-OWNED fp32
 * parameters on the device in diffusers' layouts (group_norm.{weight,bias} [C]; to_q / to_k / to_v / to_out.0 .weight [C][C], .bias [C]).  The
 * weights are packed to bf16 on the stream and the launches are those of vt_op_groupnorm + vt_op_attention at default flags (y is bit-identical
 * to them on a context whose encoder holds the same weights); refused unless flags 7, 9, 11, 12, 17 and 18 are at their defaults.  What the
 * backward needs is left in caller buffers: h16 bf16 [B][S][C]; qk16 bf16 [B][S][2C] (q | k per token); vT16 bf16 [B][C][pitch],
 * pitch = vt_op_attention_vt_pitch(S), keys contiguous; o16 bf16 and o fp32 [B][S][C] (o = the bf16 values to_out consumed); shift fp32 [B][S]
 * (the softmax exponent shift c_i of every row); sums fp32 [4][B][S] (the four key-segment sums of exp(s - c_i) per row, added as
 * ((s0 + s1) + s2) + s3); stats fp32 [B][32][2] = (mean, rstd) as vt_op_groupnorm_stats writes them.  x is fp32 [B][S][C]; tokens are the
 * NHWC pixels. */
int vt_op_attention_vt_pitch(int S);
size_t vt_op_attention_forward_train_workspace_bytes(int B, int S, int C);
int vt_op_attention_forward_train(vt_context* ctx, const float* x_f32, const float* gn_weight, const float* gn_bias, const float* wq, const float* bq,
                                  const float* wk, const float* bk, const float* wv, const float* bv, const float* wo, const float* bo, float* y_f32,
                                  void* h16_out, void* qk16_out, void* vT16_out, void* o16_out, float* o_f32_out, float* shift_out, float* sums_out,
                                  float* stats_out, int B, int S, int C, void* workspace, size_t workspace_bytes, void* stream);
/* vt_op_attention_core_backward: given do (the gradient of o, fp32 [B][S][C]) and what the forward left, with p = softmax(alpha q k^T),
 * alpha = 1 / sqrt(C), D_i = sum_c do[i][c] o[i][c]:  ds = p * (do v^T - D),  dq = alpha ds k,  dk = alpha ds^T q,  dv = p^T do  -- fp32 [B][S][C],
 * plus their bf16 copies where dq16 / dk16 / dv16 are not NULL.  All MFMA operands are bf16 with fp32 accumulation whatever flags 11, 14, 15
 * and 18 say.  Seven S x S x C products on the forward's two kernel skeletons (the minimum is five; the two extra recompute p once per
 * direction so that no S x S matrix is ever read transposed).  Images are processed `group` at a time (0: as many as the forward; larger values
 * are clamped to that) with two fragment-ordered S x S bf16 buffers per group image in the workspace; `nsplit` workgroups share a row
 * block's sweep (0: chosen from the shape; clamped to the number of 64-row tiles).  Neither changes a bit of the result, nor does the batch an
 * image runs in; results are bit-identical from run to run.  The workspace size is a function of the shape alone; 256-byte aligned. */
size_t vt_op_attention_core_backward_workspace_bytes(int B, int S, int C);
int vt_op_attention_core_backward(vt_context* ctx, const void* qk16, const void* vT16, const float* o_f32, const float* do_f32, const float* shift,
                                  const float* sums, float* dq_f32, float* dk_f32, float* dv_f32, void* dq16_out, void* dk16_out, void* dv16_out, int B,
                                  int S, int C, int group, int nsplit, void* workspace, size_t workspace_bytes, void* stream);
/* Measurement aid (tools/bench_attention_backward.py): the same call running only the launches whose bit is set in `stages`, on whatever the
 * workspace holds from an earlier full run -- bit 0 the layout passes, 1 the softmax numerators, 2 ds, 3 dq, 4 p^T, 5 dv, 6 ds^T, 7 dk; bit 8, not
 * part of the backward, launches the forward's P.V on the first fragment buffer.  stages = 0xff is vt_op_attention_core_backward. */
int vt_op_attention_core_backward_stages(vt_context* ctx, const void* qk16, const void* vT16, const float* o_f32, const float* do_f32, const float* shift,
                                         const float* sums, float* dq_f32, float* dk_f32, float* dv_f32, void* dq16_out, void* dk16_out, void* dv16_out,
                                         int B, int S, int C, int group, int nsplit, void* workspace, size_t workspace_bytes, void* stream, unsigned stages);

size_t vt_op_attention_workspace_bytes(int B, int S, int C);
int vt_op_attention(vt_context* ctx, const void* x_bf16 /* [B][S][C] normed tokens */, const float* residual_f32,
                    float* out_f32, int B, int S, int C, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VAE_TAGGER_HIP_H */
