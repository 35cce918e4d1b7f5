// VAE validation loss on the device: layout of the caller-owned state block and the counter-based normal draw (eval_vae_loss.hip; mirrored
// by vae_tagger_amd/vae_losses.py and vae_tagger_amd/improved_losses.py), and the device functions the forward (eval_vae_loss.hip) and the
// loss's gradient (vae_loss_backward.hip) share: the draw, z, the partial sums, the block fold and the per-image row.  Shared, so that a
// value both compute has the same bits.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/vae_tagger_hip.h"
#include "vt_eval.h"
#include "vt_train.h"

constexpr int VT_VAE_CHUNK = 4096;          // elements of one workgroup's partial: a constant, so the order of every sum follows from D alone
constexpr int VT_VAE_LAT_PART = 12;         // fp64 per latent partial: aa pp nn ap an dap dan kl_a kl_p kl_n | uint64 non-finite | pad
constexpr int VT_VAE_IMG_PART = 2;          // fp64 per image partial: sum (recon - target)^2 | uint64 non-finite
constexpr int VT_VAE_LOSS_K = 7;            // components: mse, kl_mean, kl_log, triplet cos, triplet euclid, contrastive cos, contrastive euclid
constexpr int VT_VAE_LOSS_COUNTERS = 7;     // updates, images, non-finite inputs, updates / images with recon, updates / images with a negative
constexpr int VT_VAE_LOSS_HEAD = 512;       // params (256 B) + totals (256 B): what vt_vae_loss_read copies
constexpr long long VT_VAE_MAX_D = 1ll << 34;      // elements of one image: its chunks stay inside one grid dimension

// One block, every section 256-B aligned:
//   params { fp64 margin_triplet, margin_contrastive, jaccard_threshold, uint64 seed }
// | totals { fp64 [7] sums over the updates of the per-batch components, fp64 [7] sums over the images of the per-image components,
//            uint64 [7] counters }
// | scratch of the last update: rows fp64 [B][VT_VAE_LOSS_ROW] then uint64 [B] non-finite counts | latent partials fp64 [B][chunks(D)][12] | image partials fp64 [B][chunks(E)][2]
struct VaeLossLayout {
    size_t params, totals, rows, lat, img, total;
    long long lat_chunks, img_chunks;        // ceil(D / 4096), ceil(E / 4096)
};
inline long long vt_vae_chunks(long long n) { return (n + VT_VAE_CHUNK - 1) / VT_VAE_CHUNK; }
inline VaeLossLayout vt_vae_loss_layout(int B, long long D, long long E) {
    VaeLossLayout l;
    l.lat_chunks = vt_vae_chunks(D);
    l.img_chunks = vt_vae_chunks(E);
    l.params = 0;
    l.totals = 256;
    l.rows = VT_VAE_LOSS_HEAD;
    l.lat = l.rows + vt_eval_align(sizeof(double) * (VT_VAE_LOSS_ROW + 1) * (size_t)B);
    l.img = l.lat + vt_eval_align(sizeof(double) * VT_VAE_LAT_PART * (size_t)B * (size_t)l.lat_chunks);
    l.total = l.img + vt_eval_align(sizeof(double) * VT_VAE_IMG_PART * (size_t)B * (size_t)l.img_chunks);
    return l;
}

// The workspace of vt_vae_loss_backward, every section 256-B aligned: the forward's scratch (rows and non-finite counts, latent partials,
// image partials), then one coefficient record per image and one for the batch.
constexpr int VT_VAE_BWD_COEF = 8;          // fp64 per image: cosine ka kp kn ipn inn | euclidean tp tn (vae_loss_backward.hip)
constexpr int VT_VAE_BWD_BATCH = 8;         // fp64 for the batch: c_kl | pad
struct VaeLossBackwardLayout {
    size_t rows, lat, img, coef, batch, total;
    long long lat_chunks, img_chunks;
};
inline VaeLossBackwardLayout vt_vae_loss_backward_layout(int B, long long D, long long E) {
    VaeLossBackwardLayout l;
    l.lat_chunks = vt_vae_chunks(D);
    l.img_chunks = vt_vae_chunks(E);
    l.rows = 0;
    l.lat = l.rows + vt_eval_align(sizeof(double) * (VT_VAE_LOSS_ROW + 1) * (size_t)B);
    l.img = l.lat + vt_eval_align(sizeof(double) * VT_VAE_LAT_PART * (size_t)B * (size_t)l.lat_chunks);
    l.coef = l.img + vt_eval_align(sizeof(double) * VT_VAE_IMG_PART * (size_t)B * (size_t)l.img_chunks);
    l.batch = l.coef + vt_eval_align(sizeof(double) * VT_VAE_BWD_COEF * (size_t)B);
    l.total = l.batch + vt_eval_align(sizeof(double) * VT_VAE_BWD_BATCH);
    return l;
}

// ---- the draw: a standard normal per (seed, draw, image, element), no stored state ----
// stream key = mix64(seed + golden (draw + 1)); image key = mix64(stream key + odd (image + 1)); the element's two words are
// mix64(image key ^ 2e) and mix64(image key ^ (2e + 1)).  u1 = ((x1 >> 11) + 1) 2^-53 lies in (0, 1] -- never 0, it goes into the
// logarithm --, u2 = (x2 >> 11) 2^-53 in [0, 1).  Box-Muller in fp64, rounded to fp32 once.
VT_TRAIN_HD inline uint64_t vt_vae_stream_key(uint64_t seed, uint64_t draw) { return vt_head_mix64(seed + 0x9E3779B97F4A7C15ull * (draw + 1)); }
VT_TRAIN_HD inline uint64_t vt_vae_image_key(uint64_t stream_key, uint64_t image) {
    return vt_head_mix64(stream_key + 0xD1B54A32D192ED03ull * (image + 1));
}

inline bool vl_misaligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }
inline bool vl_shape_ok(int B, int C, int hw) {
    return B >= 1 && B <= VT_EVAL_MAX_B && C >= 1 && hw >= 1 && (long long)C * hw <= VT_VAE_MAX_D;
}
inline bool vl_image_ok(int H, int W) { return H >= 1 && W >= 1 && 3ll * H * W <= VT_VAE_MAX_D; }

#if defined(__HIPCC__)
// ---- device functions of the forward and of the loss's gradient.  The kernels themselves stay in their units. ----
constexpr int VL_T = 256;                   // threads of a partial's workgroup
constexpr int VL_STEP = 4 * VL_T;           // elements one sweep of the workgroup covers
constexpr int VL_SWEEPS = VT_VAE_CHUNK / VL_STEP;

struct VaeStream { const float* moments; const float* z; int draw; int present; };
struct VaeLatentArg { VaeStream s[3]; };

__device__ __forceinline__ bool vl_bad(float x) { return !(fabsf(x) <= 3.0e38f); }

// the element's standard normal: Box-Muller in fp64 on two words of the image key, rounded to fp32 once
__device__ __forceinline__ float vae_eps(uint64_t image_key, uint64_t e) {
#pragma clang fp contract(off)
    const uint64_t x1 = vt_head_mix64(image_key ^ (2 * e)), x2 = vt_head_mix64(image_key ^ (2 * e + 1));
    const double u1 = (double)((x1 >> 11) + 1) * 0x1p-53, u2 = (double)(x2 >> 11) * 0x1p-53;
    return (float)(sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2));
}

// std = fp32(exp(0.5 logvar)) with the logvar clamped to [-30, 20]; lc the clamped logvar, sd the fp64 exponential.
// A NaN logvar stays NaN through the clamp, as torch.clamp keeps it.
__device__ __forceinline__ float vae_std(float logvar, double& lc, double& sd) {
#pragma clang fp contract(off)
    const float c = logvar < -30.0f ? -30.0f : (logvar > 20.0f ? 20.0f : logvar);
    lc = (double)c;
    sd = exp(0.5 * lc);
    return (float)sd;
}

// z = fma(std, eps, mean) in fp32, one rounding: the one expression every kernel that forms z goes through.  Written as the fma it has always
// been on gfx950 -- the earlier __fadd_rn(mean, __fmul_rn(std, eps)) was contracted to one v_fma_f32 by the build's -ffp-contract=fast, which
// reaches the intrinsics' inline bodies -- so that the value no longer depends on the contraction setting.
__device__ __forceinline__ float vae_z_of(float mean, float std32, float eps) { return __fmaf_rn(std32, eps, mean); }

// z = fma(fp32(exp(0.5 logvar)), eps, mean), and the element's KL term mean^2 + var - 1 - logvar (var = std^2, fp64).
__device__ __forceinline__ float vae_z(float mean, float logvar, float eps, double& kl_term) {
#pragma clang fp contract(off)
    double lc, sd;
    const float std32 = vae_std(logvar, lc, sd);
    kl_term = (double)mean * (double)mean + sd * sd - 1.0 - lc;
    return vae_z_of(mean, std32, eps);
}

// four consecutive floats from e0 (a multiple of 4): one 16-byte load, or guarded scalar loads with the same element-to-thread mapping
template <bool VEC>
__device__ __forceinline__ void vl_load4(const float* __restrict__ p, long long e0, long long n, float out[4]) {
    if (VEC) {
        const float4 v = *(const float4*)(p + e0);
        out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k] = e0 + k < n ? p[e0 + k] : 0.0f;
    }
}

// the store of the same four elements
template <bool VEC>
__device__ __forceinline__ void vl_store4(float* __restrict__ p, long long e0, long long n, const float v[4]) {
    if (VEC) {
        *(float4*)(p + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (e0 + k < n) p[e0 + k] = v[k];
    }
}

// the workgroup's NV running sums -> partial[0 .. NV-1] and the non-finite count -> partial[NV] (as uint64): wave tree, then waves in order
template <int NV>
__device__ __forceinline__ void vl_block_fold(double (&acc)[NV], unsigned bad, double* __restrict__ partial) {
#pragma clang fp contract(off)
    __shared__ double s_red[VL_T / 64][NV];
    __shared__ unsigned s_bad[VL_T / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i)
        for (int d = 32; d > 0; d >>= 1) acc[i] += __shfl_down(acc[i], d);
    for (int d = 32; d > 0; d >>= 1) bad += __shfl_down(bad, d);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) s_red[wave][i] = acc[i];
        s_bad[wave] = bad;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        double v = s_red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < VL_T / 64; ++w) v += s_red[w][threadIdx.x];
        partial[threadIdx.x] = v;
    } else if (threadIdx.x == NV) {
        unsigned long long b = 0;
#pragma unroll
        for (int w = 0; w < VL_T / 64; ++w) b += s_bad[w];
        ((unsigned long long*)partial)[NV] = b;
    }
}

// the body of the latent pass, grid (chunks of D, B).  partial: aa pp nn ap an dap dan kl_a kl_p kl_n | non-finite
template <bool VEC>
__device__ __forceinline__ void vl_latent_partials(const VaeLatentArg& a, unsigned long long seed, long long D, long long first_image, long long chunks,
                                                   double* __restrict__ partials) {
#pragma clang fp contract(off)
    const long long b = blockIdx.y, chunk = blockIdx.x;
    uint64_t key[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) key[s] = vt_vae_image_key(vt_vae_stream_key(seed, (uint64_t)(int64_t)a.s[s].draw), (uint64_t)(first_image + b));
    const bool has_n = a.s[2].present != 0;
    double acc[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) acc[i] = 0.0;
    unsigned bad = 0;
    for (int j = 0; j < VL_SWEEPS; ++j) {
        const long long e0 = chunk * VT_VAE_CHUNK + (long long)j * VL_STEP + 4 * (long long)threadIdx.x;
        if (e0 >= D) break;
        float z[3][4];
        double kt[3][4];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
#pragma unroll
            for (int k = 0; k < 4; ++k) { z[s][k] = 0.0f; kt[s][k] = 0.0; }
            if (!a.s[s].present) continue;
            float mean[4], lv[4];
            if (a.s[s].moments) {
                const float* m = a.s[s].moments + 2 * b * D;
                vl_load4<VEC>(m, e0, D, mean);
                vl_load4<VEC>(m + D, e0, D, lv);
            }
            if (a.s[s].z) vl_load4<VEC>(a.s[s].z + b * D, e0, D, z[s]);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (e0 + k >= D) continue;
                if (a.s[s].moments) {
                    const float eps = a.s[s].z ? 0.0f : vae_eps(key[s], (uint64_t)(e0 + k));
                    const float zs = vae_z(mean[k], lv[k], eps, kt[s][k]);
                    if (!a.s[s].z) z[s][k] = zs;
                    bad += (vl_bad(mean[k]) ? 1u : 0u) + (vl_bad(lv[k]) ? 1u : 0u);
                }
                bad += vl_bad(z[s][k]) ? 1u : 0u;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (e0 + k >= D) continue;
            const double va = (double)z[0][k], vp = (double)z[1][k], vn = (double)z[2][k];
            const double dp = va - vp + 1e-6;
            acc[0] += va * va; acc[1] += vp * vp; acc[3] += va * vp; acc[5] += dp * dp;
            if (has_n) {
                const double dn = va - vn + 1e-6;
                acc[2] += vn * vn; acc[4] += va * vn; acc[6] += dn * dn;
            }
            acc[7] += kt[0][k]; acc[8] += kt[1][k]; acc[9] += kt[2][k];
        }
    }
    vl_block_fold<10>(acc, bad, partials + VT_VAE_LAT_PART * (b * chunks + chunk));
}

__device__ __forceinline__ double vl_label(const float* p, long long i) { return (double)p[i]; }
__device__ __forceinline__ double vl_label(const unsigned char* p, long long i) { return p[i] ? 1.0 : 0.0; }
// F.relu / torch.clamp(min=0): a NaN stays a NaN
__device__ __forceinline__ double vl_relu(double x) { return x <= 0.0 ? 0.0 : x; }
__device__ __forceinline__ double vl_wave_sum(double v) {
#pragma clang fp contract(off)
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
    return v;
}
__device__ __forceinline__ double vl_contrastive(double dist, double sim, double thr, double margin) {
#pragma clang fp contract(off)
    const double similar = sim > thr ? 1.0 : 0.0;
    const double gap = vl_relu(margin - dist);
    return (similar * (dist * dist) + (1.0 - similar) * (gap * gap)) * (sim > thr ? sim : 1.0 - sim);
}

struct VaeRowArg { int has_kl[3]; int has_n, has_recon, has_labels; };

// one wave (lane l of 64) on image b: the image's partials in index order and its labels -> the sums, valid on lane 0.
// v: aa pp nn ap an dap dan kl_a kl_p kl_n;  w: squared error, sum labels_a, overlap, union
template <typename L>
__device__ __forceinline__ void vl_row_sums(const VaeRowArg& f, int l, long long b, const double* __restrict__ lat, long long lat_chunks,
                                            const double* __restrict__ img, long long img_chunks, const L* __restrict__ labels_a,
                                            const L* __restrict__ labels_p, int N, double (&v)[10], double (&w)[4], unsigned long long& bad) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 10; ++i) v[i] = 0.0;
    bad = 0;
    for (long long i = l; i < lat_chunks; i += 64) {
        const double* p = lat + VT_VAE_LAT_PART * (b * lat_chunks + i);
#pragma unroll
        for (int k = 0; k < 10; ++k) v[k] += p[k];
        bad += ((const unsigned long long*)p)[10];
    }
    double se = 0.0;
    if (f.has_recon)
        for (long long i = l; i < img_chunks; i += 64) {
            const double* p = img + VT_VAE_IMG_PART * (b * img_chunks + i);
            se += p[0];
            bad += ((const unsigned long long*)p)[1];
        }
    double sa = 0.0, ov = 0.0, un = 0.0;
    if (f.has_labels)
        for (int j = l; j < N; j += 64) {
            const double ya = vl_label(labels_a, b * N + j), yp = vl_label(labels_p, b * N + j);
            sa += ya; ov += ya * yp; un += ya + yp - ya * yp;
        }
#pragma unroll
    for (int k = 0; k < 10; ++k) v[k] = vl_wave_sum(v[k]);
    w[0] = vl_wave_sum(se); w[1] = vl_wave_sum(sa); w[2] = vl_wave_sum(ov); w[3] = vl_wave_sum(un);
    for (int d = 32; d > 0; d >>= 1) bad += __shfl_down(bad, d);
}

// the image's row from its sums (mt, mc: the triplet's and the contrastive margin; thr: the label-similarity threshold)
__device__ __forceinline__ void vl_row_values(const VaeRowArg& f, double mt, double mc, double thr, long long E, const double (&v)[10],
                                              const double (&w)[4], double (&r)[VT_VAE_LOSS_ROW]) {
#pragma clang fp contract(off)
    const double se = w[0], sa = w[1], ov = w[2], un = w[3];
    r[0] = f.has_recon ? se / (double)E : 0.0;
    r[1] = f.has_kl[0] ? 0.5 * v[7] : 0.0;
    r[2] = f.has_kl[1] ? 0.5 * v[8] : 0.0;
    r[3] = f.has_kl[2] ? 0.5 * v[9] : 0.0;
    const int nk = f.has_kl[0] + f.has_kl[1] + f.has_kl[2];
    r[4] = nk ? (r[1] + r[2] + r[3]) / (double)nk : 0.0;
    r[5] = log1p(r[4] / 10000.0);
    const double na = fmax(sqrt(v[0]), 1e-12), np = fmax(sqrt(v[1]), 1e-12), nn = fmax(sqrt(v[2]), 1e-12);
    r[6] = 1.0 - v[3] / (na * np);
    r[7] = f.has_n ? 1.0 - v[4] / (na * nn) : 0.0;
    r[8] = sqrt(v[5]);
    r[9] = f.has_n ? sqrt(v[6]) : 0.0;
    const double wt = f.has_labels ? 1.0 + 0.5 * (ov / (sa + 1e-8)) : 1.0;
    const double sim = ov / (un + 1e-8);
    r[10] = f.has_n ? vl_relu(r[6] - r[7] + mt) * wt : 0.0;
    r[11] = f.has_n ? vl_relu(r[8] - r[9] + mt) * wt : 0.0;
    r[12] = vl_contrastive(r[6], sim, thr, mc);
    r[13] = vl_contrastive(r[8], sim, thr, mc);
    r[14] = sa; r[15] = ov; r[16] = un; r[17] = wt; r[18] = sim;
}
#endif  // __HIPCC__
