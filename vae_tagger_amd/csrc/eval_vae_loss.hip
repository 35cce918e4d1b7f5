// VAE validation loss on the device: posterior.sample() / .kl() and the per-batch loss of the reference's VAE validation loops
// (train_vae.py:216-268, train_full.py:290-338; improved_losses.py:13-37, :81-105, :277-287), accumulated in one caller-owned block.
// Forward only.  Every sum is fp64 from the fp32 inputs.  No atomics: a workgroup owns 4096 consecutive elements of one image (thread t
// takes the four float4 at 4t, 4t + 1024, ...), its 256 threads are combined by a wave tree and the four waves in wave order; a second
// launch adds an image's partials in index order (lane l takes l, l + 64, ...; wave tree) and forms the per-image row; a third, one-wave
// launch adds the rows one image after the other.  The order of every sum is a function of the shapes alone.
// The latent pass reads the three moments tensors once and writes partials only: z = mean + std eps is formed in registers by the same
// device function vt_posterior_sample stores it with, so the in-flight state is the given-z state bit for bit.
#include <math.h>

#include "vt_context.h"
#include "vt_vae_loss.h"

using namespace vt;

namespace {

constexpr int VL_KL_T = 1024;               // vt_posterior_sample's kl_out: one workgroup per image

// grid (chunks of D, B).  partial: aa pp nn ap an dap dan kl_a kl_p kl_n | non-finite
template <bool VEC>
__global__ __launch_bounds__(VL_T) void vae_latent_kernel(VaeLatentArg a, const double* __restrict__ params, long long D, long long first_image,
                                                          long long chunks, double* __restrict__ partials) {
    vl_latent_partials<VEC>(a, ((const unsigned long long*)params)[3], D, first_image, chunks, partials);
}

// grid (chunks of E, B).  partial: sum (recon - target)^2 | non-finite
template <bool VEC>
__global__ __launch_bounds__(VL_T) void vae_image_kernel(const float* __restrict__ recon, const float* __restrict__ target, long long E, long long chunks,
                                                         double* __restrict__ partials) {
#pragma clang fp contract(off)
    const long long b = blockIdx.y, chunk = blockIdx.x;
    double acc[1] = {0.0};
    unsigned bad = 0;
    for (int j = 0; j < VL_SWEEPS; ++j) {
        const long long e0 = chunk * VT_VAE_CHUNK + (long long)j * VL_STEP + 4 * (long long)threadIdx.x;
        if (e0 >= E) break;
        float r[4], t[4];
        vl_load4<VEC>(recon + b * E, e0, E, r);
        vl_load4<VEC>(target + b * E, e0, E, t);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (e0 + k >= E) continue;
            const double d = (double)r[k] - (double)t[k];
            acc[0] += d * d;
            bad += (vl_bad(r[k]) ? 1u : 0u) + (vl_bad(t[k]) ? 1u : 0u);
        }
    }
    vl_block_fold<1>(acc, bad, partials + VT_VAE_IMG_PART * (b * chunks + chunk));
}

// grid B, one wave: an image's partials in index order and its labels -> the image's row
template <typename L>
__global__ __launch_bounds__(64) void vae_row_kernel(VaeRowArg f, const double* __restrict__ params, const double* __restrict__ lat, long long lat_chunks,
                                                     const double* __restrict__ img, long long img_chunks, long long E, const L* __restrict__ labels_a,
                                                     const L* __restrict__ labels_p, int N, double* __restrict__ rows, double* __restrict__ rows_out,
                                                     unsigned long long* __restrict__ bad_out) {
#pragma clang fp contract(off)
    const long long b = blockIdx.x;
    double v[10], w[4], r[VT_VAE_LOSS_ROW];
    unsigned long long bad;
    vl_row_sums(f, (int)threadIdx.x, b, lat, lat_chunks, img, img_chunks, labels_a, labels_p, N, v, w, bad);
    if (threadIdx.x != 0) return;
    vl_row_values(f, params[0], params[1], params[2], E, v, w, r);
#pragma unroll
    for (int k = 0; k < VT_VAE_LOSS_ROW; ++k) {
        rows[VT_VAE_LOSS_ROW * b + k] = r[k];
        if (rows_out) rows_out[VT_VAE_LOSS_ROW * b + k] = r[k];
    }
    bad_out[b] = bad;
}

// one wave: lane k < 7 owns component k and walks the rows one image after the other; lane 7 the counters
__global__ __launch_bounds__(64) void vae_batch_kernel(VaeRowArg f, const double* __restrict__ rows, const unsigned long long* __restrict__ bad, int B,
                                                       double* __restrict__ totals) {
#pragma clang fp contract(off)
    const int k = threadIdx.x;
    unsigned long long* counters = (unsigned long long*)(totals + 2 * VT_VAE_LOSS_K);
    if (k < VT_VAE_LOSS_K) {
        const int column = k == 0 ? 0 : k < 3 ? 3 + k : 7 + k;                    // row entries 0, 4, 5, 10, 11, 12, 13
        const bool on = k == 0 ? f.has_recon != 0 : (k == 3 || k == 4) ? f.has_n != 0 : true;
        if (!on) return;
        double batch = 0.0, kl = 0.0, images = totals[VT_VAE_LOSS_K + k];
        for (int b = 0; b < B; ++b) {
            const double x = rows[VT_VAE_LOSS_ROW * b + column];
            batch += x; images += x;
            if (k == 2) kl += rows[VT_VAE_LOSS_ROW * b + 4];
        }
        totals[k] += k == 2 ? log1p(kl / (double)B / 10000.0) : batch / (double)B;
        totals[VT_VAE_LOSS_K + k] = images;
    } else if (k == VT_VAE_LOSS_K) {
        unsigned long long nb = 0;
        for (int b = 0; b < B; ++b) nb += bad[b];
        counters[0] += 1ull; counters[1] += (unsigned long long)B; counters[2] += nb;
        if (f.has_recon) { counters[3] += 1ull; counters[4] += (unsigned long long)B; }
        if (f.has_n) { counters[5] += 1ull; counters[6] += (unsigned long long)B; }
    }
}

__global__ __launch_bounds__(64) void vae_init_kernel(double* __restrict__ params, double mt, double mc, double thr, unsigned long long seed) {
    if (threadIdx.x == 0) { params[0] = mt; params[1] = mc; params[2] = thr; ((unsigned long long*)params)[3] = seed; }
}

// grid (chunks of D, B): z_out = mean + std eps, the element-to-thread mapping of the latent pass
template <bool VEC>
__global__ __launch_bounds__(VL_T) void vae_sample_kernel(const float* __restrict__ moments, long long D, unsigned long long seed, int draw,
                                                          long long first_image, float* __restrict__ z_out) {
#pragma clang fp contract(off)
    const long long b = blockIdx.y;
    const uint64_t key = vt_vae_image_key(vt_vae_stream_key(seed, (uint64_t)(int64_t)draw), (uint64_t)(first_image + b));
    const float* m = moments + 2 * b * D;
    for (int j = 0; j < VL_SWEEPS; ++j) {
        const long long e0 = (long long)blockIdx.x * VT_VAE_CHUNK + (long long)j * VL_STEP + 4 * (long long)threadIdx.x;
        if (e0 >= D) break;
        float mean[4], lv[4], z[4];
        vl_load4<VEC>(m, e0, D, mean);
        vl_load4<VEC>(m + D, e0, D, lv);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            double unused;
            z[k] = e0 + k < D ? vae_z(mean[k], lv[k], vae_eps(key, (uint64_t)(e0 + k)), unused) : 0.0f;
        }
        if (VEC) {
            *(float4*)(z_out + b * D + e0) = make_float4(z[0], z[1], z[2], z[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (e0 + k < D) z_out[b * D + e0 + k] = z[k];
        }
    }
}

// grid B, 1024 threads: kl_out[b] = 0.5 sum of the image's KL terms (thread t takes t, t + 1024, ...; wave tree; waves in order)
__global__ __launch_bounds__(VL_KL_T) void vae_kl_kernel(const float* __restrict__ moments, long long D, double* __restrict__ kl_out) {
#pragma clang fp contract(off)
    __shared__ double s_red[VL_KL_T / 64];
    const long long b = blockIdx.x;
    const float* m = moments + 2 * b * D;
    double acc = 0.0;
    for (long long e = threadIdx.x; e < D; e += VL_KL_T) {
        double t;
        (void)vae_z(m[e], m[D + e], 0.0f, t);
        acc += t;
    }
    acc = vl_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double v = s_red[0];
        for (int w = 1; w < VL_KL_T / 64; ++w) v += s_red[w];
        kl_out[b] = 0.5 * v;
    }
}

// grid (chunks of D, B): out[b] = mean[b] * scaling + shift, each op only when its flag is set, the multiply and the add rounded separately
// (torch's two eager ops); the element-to-thread mapping of the sample pass, all loads of a thread issued before its first store
template <bool VEC>
__global__ __launch_bounds__(VL_T) void vae_mode_latent_kernel(const float* __restrict__ moments, long long D, float scaling, int has_scaling, float shift,
                                                               int has_shift, float* __restrict__ out) {
#pragma clang fp contract(off)
    const long long b = blockIdx.y;
    const float* m = moments + 2 * b * D;
    float v[VL_SWEEPS][4];
#pragma unroll
    for (int j = 0; j < VL_SWEEPS; ++j) {
        const long long e0 = (long long)blockIdx.x * VT_VAE_CHUNK + (long long)j * VL_STEP + 4 * (long long)threadIdx.x;
        if (e0 < D) vl_load4<VEC>(m, e0, D, v[j]);
    }
#pragma unroll
    for (int j = 0; j < VL_SWEEPS; ++j) {
        const long long e0 = (long long)blockIdx.x * VT_VAE_CHUNK + (long long)j * VL_STEP + 4 * (long long)threadIdx.x;
        if (e0 >= D) break;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float x = v[j][k];
            if (has_scaling) {
                x = x * scaling;
                asm volatile("" : "+v"(x));         // (-ffp-contract=fast on the command line would fuse the product into the add below)
            }
            if (has_shift) x = x + shift;
            v[j][k] = x;
        }
        vl_store4<VEC>(out + b * D, e0, D, v[j]);
    }
}

int vl_check_state(vt_context* c, const char* who, const void* state, size_t state_bytes, size_t need) {
    if (!state || vl_misaligned(state, ALIGN)) return c->fail(VT_ERR_INVALID, "%s: state is null or not 256-B aligned", who);
    if (state_bytes < need) return c->fail(VT_ERR_WORKSPACE, "%s: state holds %zu bytes, %zu needed", who, state_bytes, need);
    return VT_OK;
}

#define VLCK(c, what) HIPCK(c, hipGetLastError(), what)

}  // namespace

extern "C" {

int vt_posterior_sample(vt_context* c, const float* moments, int B, int C, int hw, unsigned long long seed, int draw, long long first_image,
                        float* z_out, double* kl_out, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (!vl_shape_ok(B, C, hw)) return c->fail(VT_ERR_INVALID, "vt_posterior_sample: B = %d (1..%d), C = %d or hw = %d out of range", B, VT_EVAL_MAX_B, C, hw);
    if (!moments || vl_misaligned(moments, 4) || vl_misaligned(z_out, 4) || vl_misaligned(kl_out, 8))
        return c->fail(VT_ERR_INVALID, "vt_posterior_sample: moments is null, or a pointer is misaligned");
    if (draw < 0 || first_image < 0) return c->fail(VT_ERR_INVALID, "vt_posterior_sample: draw and first_image are >= 0");
    const long long D = (long long)C * hw;
    hipStream_t s = (hipStream_t)stream;
    if (z_out) {
        const dim3 grid((unsigned)vt_vae_chunks(D), (unsigned)B);
        if (D % 4 == 0 && !vl_misaligned(moments, 16) && !vl_misaligned(z_out, 16))
            hipLaunchKernelGGL(vae_sample_kernel<true>, grid, dim3(VL_T), 0, s, moments, D, seed, draw, first_image, z_out);
        else
            hipLaunchKernelGGL(vae_sample_kernel<false>, grid, dim3(VL_T), 0, s, moments, D, seed, draw, first_image, z_out);
        VLCK(c, "posterior_sample");
    }
    if (kl_out) {
        hipLaunchKernelGGL(vae_kl_kernel, dim3((unsigned)B), dim3(VL_KL_T), 0, s, moments, D, kl_out); VLCK(c, "posterior_sample kl");
    }
    return VT_OK;
}

int vt_posterior_mode_latent(vt_context* c, const float* moments, int B, int C, int hw, float scaling, int has_scaling, float shift, int has_shift,
                             float* latent_out, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    const char* who = "vt_posterior_mode_latent";
    if (!vl_shape_ok(B, C, hw)) return c->fail(VT_ERR_INVALID, "%s: B = %d (1..%d), C = %d or hw = %d out of range", who, B, VT_EVAL_MAX_B, C, hw);
    if (!moments || !latent_out || vl_misaligned(moments, 4) || vl_misaligned(latent_out, 4))
        return c->fail(VT_ERR_INVALID, "%s: moments or latent_out is null or misaligned", who);
    if ((has_scaling && !isfinite(scaling)) || (has_shift && !isfinite(shift)))
        return c->fail(VT_ERR_INVALID, "%s: scaling = %g and shift = %g must be finite where their flags are set", who, scaling, shift);
    const long long D = (long long)C * hw;
    const dim3 grid((unsigned)vt_vae_chunks(D), (unsigned)B);
    hipStream_t s = (hipStream_t)stream;
    if (D % 4 == 0 && !vl_misaligned(moments, 16) && !vl_misaligned(latent_out, 16))
        hipLaunchKernelGGL(vae_mode_latent_kernel<true>, grid, dim3(VL_T), 0, s, moments, D, scaling, has_scaling != 0, shift, has_shift != 0, latent_out);
    else
        hipLaunchKernelGGL(vae_mode_latent_kernel<false>, grid, dim3(VL_T), 0, s, moments, D, scaling, has_scaling != 0, shift, has_shift != 0, latent_out);
    VLCK(c, "posterior_mode_latent");
    return VT_OK;
}

size_t vt_vae_loss_state_bytes(int B, int C, int hw, int H, int W) {
    if (!vl_shape_ok(B, C, hw) || H < 0 || W < 0 || ((H == 0) != (W == 0)) || (H > 0 && !vl_image_ok(H, W))) return 0;
    return vt_vae_loss_layout(B, (long long)C * hw, 3ll * H * W).total;
}

int vt_vae_loss_reset(vt_context* c, void* state, size_t state_bytes, double margin_triplet, double margin_contrastive, double jaccard_threshold,
                      unsigned long long seed, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (int r = vl_check_state(c, "vt_vae_loss_reset", state, state_bytes, VT_VAE_LOSS_HEAD)) return r;
    if (!isfinite(margin_triplet) || !isfinite(margin_contrastive) || !isfinite(jaccard_threshold))
        return c->fail(VT_ERR_INVALID, "vt_vae_loss_reset: the margins and the threshold must be finite");
    hipStream_t s = (hipStream_t)stream;
    HIPCK(c, hipMemsetAsync(state, 0, VT_VAE_LOSS_HEAD, s), "vae_loss_reset clear");
    hipLaunchKernelGGL(vae_init_kernel, dim3(1), dim3(64), 0, s, (double*)state, margin_triplet, margin_contrastive, jaccard_threshold, seed);
    VLCK(c, "vae_loss_reset init");
    return VT_OK;
}

int vt_vae_loss_update(vt_context* c, void* state, size_t state_bytes, const vt_vae_loss_input* anchor, const vt_vae_loss_input* positive,
                       const vt_vae_loss_input* negative, const float* recon, const float* target, int H, int W, const void* labels_a,
                       const void* labels_p, int labels_dtype, int N, int B, int C, int hw, long long first_image, double* rows_out, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (!vl_shape_ok(B, C, hw)) return c->fail(VT_ERR_INVALID, "vt_vae_loss_update: B = %d (1..%d), C = %d or hw = %d out of range", B, VT_EVAL_MAX_B, C, hw);
    if (!anchor || !positive) return c->fail(VT_ERR_INVALID, "vt_vae_loss_update: anchor and positive are required");
    if (first_image < 0) return c->fail(VT_ERR_INVALID, "vt_vae_loss_update: first_image < 0");
    const long long D = (long long)C * hw;
    const vt_vae_loss_input* in[3] = {anchor, positive, negative};
    VaeLatentArg la;
    VaeRowArg f;
    bool vec = D % 4 == 0;
    for (int s = 0; s < 3; ++s) {
        VaeStream& v = la.s[s];
        v.moments = nullptr; v.z = nullptr; v.draw = 0; v.present = in[s] != nullptr;
        f.has_kl[s] = 0;
        if (!in[s]) continue;
        if (!in[s]->moments && !in[s]->z) return c->fail(VT_ERR_INVALID, "vt_vae_loss_update: input %d has neither moments nor z", s);
        if (vl_misaligned(in[s]->moments, 4) || vl_misaligned(in[s]->z, 4)) return c->fail(VT_ERR_INVALID, "vt_vae_loss_update: input %d is misaligned", s);
        if (in[s]->draw < 0) return c->fail(VT_ERR_INVALID, "vt_vae_loss_update: input %d has a negative draw", s);
        v.moments = in[s]->moments; v.z = in[s]->z; v.draw = in[s]->draw;
        f.has_kl[s] = v.moments != nullptr;
        vec = vec && !vl_misaligned(v.moments, 16) && !vl_misaligned(v.z, 16);
    }
    if ((recon == nullptr) != (target == nullptr)) return c->fail(VT_ERR_INVALID, "vt_vae_loss_update: recon and target come together or not at all");
    if (recon && (!vl_image_ok(H, W) || vl_misaligned(recon, 4) || vl_misaligned(target, 4)))
        return c->fail(VT_ERR_INVALID, "vt_vae_loss_update: H = %d, W = %d out of range, or recon / target misaligned", H, W);
    if ((labels_a == nullptr) != (labels_p == nullptr)) return c->fail(VT_ERR_INVALID, "vt_vae_loss_update: labels_a and labels_p come together or not at all");
    if (labels_a && ((labels_dtype != VT_F32 && labels_dtype != VT_U8) || N < 1 || N > (1 << 24) ||
                     (labels_dtype == VT_F32 && (vl_misaligned(labels_a, 4) || vl_misaligned(labels_p, 4)))))
        return c->fail(VT_ERR_INVALID, "vt_vae_loss_update: labels neither VT_F32 nor VT_U8, misaligned, or N = %d outside [1, 2^24]", N);
    if (vl_misaligned(rows_out, 8)) return c->fail(VT_ERR_INVALID, "vt_vae_loss_update: rows_out is misaligned");
    const long long E = recon ? 3ll * H * W : 0;
    const VaeLossLayout l = vt_vae_loss_layout(B, D, E);
    if (int r = vl_check_state(c, "vt_vae_loss_update", state, state_bytes, l.total)) return r;
    f.has_n = negative != nullptr; f.has_recon = recon != nullptr; f.has_labels = labels_a != nullptr;

    hipStream_t s = (hipStream_t)stream;
    char* st = (char*)state;
    const double* params = (const double*)(st + l.params);
    double* totals = (double*)(st + l.totals);
    double* rows = (double*)(st + l.rows);
    double* lat = (double*)(st + l.lat);
    double* img = (double*)(st + l.img);
    unsigned long long* bad = (unsigned long long*)(rows + (size_t)VT_VAE_LOSS_ROW * B);      // the images' non-finite counts follow the rows
    const dim3 lgrid((unsigned)l.lat_chunks, (unsigned)B);
    if (vec) hipLaunchKernelGGL(vae_latent_kernel<true>, lgrid, dim3(VL_T), 0, s, la, params, D, first_image, l.lat_chunks, lat);
    else hipLaunchKernelGGL(vae_latent_kernel<false>, lgrid, dim3(VL_T), 0, s, la, params, D, first_image, l.lat_chunks, lat);
    VLCK(c, "vae_loss_update latent");
    if (recon) {
        const dim3 igrid((unsigned)l.img_chunks, (unsigned)B);
        if (E % 4 == 0 && !vl_misaligned(recon, 16) && !vl_misaligned(target, 16))
            hipLaunchKernelGGL(vae_image_kernel<true>, igrid, dim3(VL_T), 0, s, recon, target, E, l.img_chunks, img);
        else
            hipLaunchKernelGGL(vae_image_kernel<false>, igrid, dim3(VL_T), 0, s, recon, target, E, l.img_chunks, img);
        VLCK(c, "vae_loss_update image");
    }
    if (labels_a && labels_dtype == VT_U8)
        hipLaunchKernelGGL(vae_row_kernel<unsigned char>, dim3((unsigned)B), dim3(64), 0, s, f, params, lat, l.lat_chunks, img, l.img_chunks, E,
                           (const unsigned char*)labels_a, (const unsigned char*)labels_p, N, rows, rows_out, bad);
    else
        hipLaunchKernelGGL(vae_row_kernel<float>, dim3((unsigned)B), dim3(64), 0, s, f, params, lat, l.lat_chunks, img, l.img_chunks, E,
                           (const float*)labels_a, (const float*)labels_p, N, rows, rows_out, bad);
    VLCK(c, "vae_loss_update rows");
    hipLaunchKernelGGL(vae_batch_kernel, dim3(1), dim3(64), 0, s, f, rows, bad, B, totals); VLCK(c, "vae_loss_update batch");
    return VT_OK;
}

int vt_vae_loss_read(vt_context* c, const void* state, size_t state_bytes, void* out, size_t out_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    if (int r = vl_check_state(c, "vt_vae_loss_read", state, state_bytes, VT_VAE_LOSS_HEAD)) return r;
    if (!out || vl_misaligned(out, 8)) return c->fail(VT_ERR_INVALID, "vt_vae_loss_read: out is null or misaligned");
    if (out_bytes < (size_t)VT_VAE_LOSS_HEAD) return c->fail(VT_ERR_WORKSPACE, "vt_vae_loss_read: out holds %zu bytes, %d needed", out_bytes, VT_VAE_LOSS_HEAD);
    const uintptr_t a = (uintptr_t)state, b = (uintptr_t)out;
    if (a < b + VT_VAE_LOSS_HEAD && b < a + VT_VAE_LOSS_HEAD) return c->fail(VT_ERR_INVALID, "vt_vae_loss_read: out overlaps the state");
    HIPCK(c, hipMemcpyAsync(out, state, VT_VAE_LOSS_HEAD, hipMemcpyDefault, (hipStream_t)stream), "vae_loss_read");
    return VT_OK;
}

}  // extern "C"
