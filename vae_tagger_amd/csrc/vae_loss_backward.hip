// Gradient of the VAE's training loss on the device (train_vae.py:131-179 with the losses of improved_losses.py):
//   total = w_rec mse(recon, target) + w_kl log(1 + kl_mean / 10000) + w_tri ImprovedTripletLoss(z_a, z_p, z_n, labels_a, labels_p)
// -> d recon and d moments of the three streams, the per-image rows and the batch's losses.  z = mean + std eps is never stored: every eps
// is regenerated from the counter, as the forward's latent pass does.  The discipline is the forward's (eval_vae_loss.hip): fp64 arithmetic
// from the fp32 inputs and one rounding at the store, no contraction, no atomics, sums in an order fixed by the shapes, a float4 path and a
// guarded scalar path with one element-to-thread mapping.  The partial sums, the block fold and the row arithmetic ARE the forward's
// device functions (vt_vae_loss.h), so a rows_out column both calls fill has the same bits.
//
// Launches, all on one stream: latent partials (chunks of D, B) | image pass (chunks of E, B): d recon and / or the squared-error
// partials | coefficients (B, one wave): the image's row and its triplet coefficients | batch (one wave): the losses and c_kl |
// latent gradient (chunks of D, B): three d moments.
//
// Per image, with t = w_tri weight [pos - neg + margin > 0] / B, N. = max(|.|, 1e-12) and c. = [|.| >= 1e-12] (F.normalize's clamp):
//   cosine     g_a = ka a - ipn p + inn n,  g_p = kp p - ipn a,  g_n = inn a - kn n
//              ipn = t / (Na Np), inn = t / (Na Nn), ka = ca t (a.p / Np - a.n / Nn) / (Na^2 |a|), kp = cp t a.p / (Na Np^2 |p|), kn likewise
//   euclidean  g_a = tp (a - p + 1e-6) - tn (a - n + 1e-6),  g_p = -tp (a - p + 1e-6),  g_n = tn (a - n + 1e-6);  tp = t / dist_p, 0 at dist_p = 0
// and per element  d mean = g [+ dz_dec] + c_kl mean,  d logvar = in_clamp (0.5 (g std eps [+ dz_dec std eps_dec]) + c_kl 0.5 (var - 1)).
#include <math.h>

#include "vt_context.h"
#include "vt_vae_loss.h"

using namespace vt;

namespace {

struct VlbGradArg {
    const float* moments[3];
    float* d_moments[3];
    int draw[3];
    const float* dz_dec;
    int dz_draw, euclidean;
};
struct VlbWeights { double w_rec, w_kl, w_tri, margin; };

template <bool VEC>
__global__ __launch_bounds__(VL_T) void vlb_latent_kernel(VaeLatentArg a, unsigned long long seed, long long D, long long first_image, long long chunks,
                                                          double* __restrict__ partials) {
    vl_latent_partials<VEC>(a, seed, D, first_image, chunks, partials);
}

// grid (chunks of E, B): d_recon = scale (recon - target) (if d_recon) and the forward's image partial (if partials)
template <bool VEC>
__global__ __launch_bounds__(VL_T) void vlb_image_kernel(const float* __restrict__ recon, const float* __restrict__ target, long long E, long long chunks,
                                                         double scale, float* __restrict__ d_recon, double* __restrict__ partials) {
#pragma clang fp contract(off)
    const long long b = blockIdx.y, chunk = blockIdx.x;
    double acc[1] = {0.0};
    unsigned bad = 0;
    for (int j = 0; j < VL_SWEEPS; ++j) {
        const long long e0 = chunk * VT_VAE_CHUNK + (long long)j * VL_STEP + 4 * (long long)threadIdx.x;
        if (e0 >= E) break;
        float r[4], t[4], g[4];
        vl_load4<VEC>(recon + b * E, e0, E, r);
        vl_load4<VEC>(target + b * E, e0, E, t);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            g[k] = 0.0f;
            if (e0 + k >= E) continue;
            const double d = (double)r[k] - (double)t[k];
            acc[0] += d * d;
            bad += (vl_bad(r[k]) ? 1u : 0u) + (vl_bad(t[k]) ? 1u : 0u);
            g[k] = (float)(scale * d);
        }
        if (d_recon) vl_store4<VEC>(d_recon + b * E, e0, E, g);
    }
    if (partials) vl_block_fold<1>(acc, bad, partials + VT_VAE_IMG_PART * (b * chunks + chunk));
}

// grid B, one wave: the image's row (the forward's; the contrastive columns 12 and 13 are not computed here and are 0) and its coefficients
template <typename L>
__global__ __launch_bounds__(64) void vlb_coef_kernel(VaeRowArg f, VlbWeights wt, int euclidean, int B, const double* __restrict__ lat, long long lat_chunks,
                                                      const double* __restrict__ img, long long img_chunks, long long E, const L* __restrict__ labels_a,
                                                      const L* __restrict__ labels_p, int N, double* __restrict__ rows, double* __restrict__ rows_out,
                                                      unsigned long long* __restrict__ bad_out, double* __restrict__ coef) {
#pragma clang fp contract(off)
    const long long b = blockIdx.x;
    double v[10], w[4], r[VT_VAE_LOSS_ROW];
    unsigned long long bad;
    vl_row_sums(f, (int)threadIdx.x, b, lat, lat_chunks, img, img_chunks, labels_a, labels_p, N, v, w, bad);
    if (threadIdx.x != 0) return;
    vl_row_values(f, wt.margin, 0.0, 0.0, E, v, w, r);
    r[12] = 0.0; r[13] = 0.0;
#pragma unroll
    for (int k = 0; k < VT_VAE_LOSS_ROW; ++k) {
        rows[VT_VAE_LOSS_ROW * b + k] = r[k];
        if (rows_out) rows_out[VT_VAE_LOSS_ROW * b + k] = r[k];
    }
    bad_out[b] = bad;
    // the hinge's derivative is 0 at 0 (a NaN stays active and spreads, as in the forward)
    const double x = euclidean ? r[8] - r[9] + wt.margin : r[6] - r[7] + wt.margin;
    const double t = wt.w_tri * r[17] / (double)B * (x <= 0.0 ? 0.0 : 1.0);
    double c[VT_VAE_BWD_COEF];
#pragma unroll
    for (int k = 0; k < VT_VAE_BWD_COEF; ++k) c[k] = 0.0;
    if (euclidean) {
        c[0] = r[8] > 0.0 ? t / r[8] : 0.0;
        c[1] = r[9] > 0.0 ? t / r[9] : 0.0;
    } else {
        const double ra = sqrt(v[0]), rp = sqrt(v[1]), rn = sqrt(v[2]);
        const double na = fmax(ra, 1e-12), np = fmax(rp, 1e-12), nn = fmax(rn, 1e-12);
        c[0] = ra >= 1e-12 ? t * (v[3] / np - v[4] / nn) / (na * na * ra) : 0.0;
        c[1] = rp >= 1e-12 ? t * v[3] / (na * np * np * rp) : 0.0;
        c[2] = rn >= 1e-12 ? t * v[4] / (na * nn * nn * rn) : 0.0;
        c[3] = t / (na * np);
        c[4] = t / (na * nn);
    }
#pragma unroll
    for (int k = 0; k < VT_VAE_BWD_COEF; ++k) coef[VT_VAE_BWD_COEF * b + k] = c[k];
}

// one wave: lanes 0, 1, 2 walk the rows' mse, kl_mean and triplet columns one image after the other -> loss_out { recon, kl, triplet, total }
// and batch[0] = c_kl = w_kl / (3 B 10000 (1 + kl_mean / 10000))
__global__ __launch_bounds__(64) void vlb_batch_kernel(VlbWeights wt, int euclidean, int B, const double* __restrict__ rows, double* __restrict__ batch,
                                                       double* __restrict__ loss_out) {
#pragma clang fp contract(off)
    const int k = threadIdx.x;
    const int column = k == 0 ? 0 : k == 1 ? 4 : euclidean ? 11 : 10;
    double sum = 0.0;
    if (k < 3)
        for (int b = 0; b < B; ++b) sum += rows[VT_VAE_LOSS_ROW * b + column];
    const double value = k == 1 ? log1p(sum / (double)B / 10000.0) : sum / (double)B;
    const double recon = __shfl(value, 0), kl = __shfl(value, 1), tri = __shfl(value, 2);
    if (k == 1) batch[0] = wt.w_kl / (3.0 * (double)B * 10000.0 * (1.0 + sum / (double)B / 10000.0));
    if (k == 0 && loss_out) {
        loss_out[0] = recon; loss_out[1] = kl; loss_out[2] = tri;
        loss_out[3] = wt.w_rec * recon + wt.w_kl * kl + wt.w_tri * tri;
    }
}

// grid (chunks of D, B): the three d moments, the element-to-thread mapping of the latent pass
template <bool VEC>
__global__ __launch_bounds__(VL_T) void vlb_grad_kernel(VlbGradArg a, unsigned long long seed, long long D, long long first_image,
                                                        const double* __restrict__ coef, const double* __restrict__ batch) {
#pragma clang fp contract(off)
    const long long b = blockIdx.y;
    uint64_t key[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) key[s] = vt_vae_image_key(vt_vae_stream_key(seed, (uint64_t)(int64_t)a.draw[s]), (uint64_t)(first_image + b));
    const uint64_t key_dec = vt_vae_image_key(vt_vae_stream_key(seed, (uint64_t)(int64_t)a.dz_draw), (uint64_t)(first_image + b));
    double c[VT_VAE_BWD_COEF];
#pragma unroll
    for (int k = 0; k < VT_VAE_BWD_COEF; ++k) c[k] = coef[VT_VAE_BWD_COEF * b + k];
    const double c_kl = batch[0];
    for (int j = 0; j < VL_SWEEPS; ++j) {
        const long long e0 = (long long)blockIdx.x * VT_VAE_CHUNK + (long long)j * VL_STEP + 4 * (long long)threadIdx.x;
        if (e0 >= D) break;
        float mean[3][4], lv[3][4], dz[4] = {0.0f, 0.0f, 0.0f, 0.0f}, dm[3][4], dl[3][4];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const float* m = a.moments[s] + 2 * b * D;
            vl_load4<VEC>(m, e0, D, mean[s]);
            vl_load4<VEC>(m + D, e0, D, lv[s]);
        }
        if (a.dz_dec) vl_load4<VEC>(a.dz_dec + b * D, e0, D, dz);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int s = 0; s < 3; ++s) { dm[s][k] = 0.0f; dl[s][k] = 0.0f; }
            if (e0 + k >= D) continue;
            double sd[3], sf[3], ep[3], z[3], g[3];
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                double lc;
                const float std32 = vae_std(lv[s][k], lc, sd[s]);
                const float eps = vae_eps(key[s], (uint64_t)(e0 + k));
                sf[s] = (double)std32; ep[s] = (double)eps;
                z[s] = (double)vae_z_of(mean[s][k], std32, eps);                  // the forward's z, bit for bit
            }
            if (a.euclidean) {
                const double dp = z[0] - z[1] + 1e-6, dn = z[0] - z[2] + 1e-6;
                g[0] = dp * c[0] - dn * c[1];
                g[1] = -(dp * c[0]);
                g[2] = dn * c[1];
            } else {
                g[0] = z[0] * c[0] - z[1] * c[3] + z[2] * c[4];
                g[1] = z[1] * c[1] - z[0] * c[3];
                g[2] = z[0] * c[4] - z[2] * c[2];
            }
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                double d_mean = g[s], sampled = g[s] * sf[s] * ep[s];
                if (s == 0 && a.dz_dec) {
                    const double dzv = (double)dz[k];
                    d_mean += dzv;
                    sampled += dzv * sf[0] * (double)vae_eps(key_dec, (uint64_t)(e0 + k));
                }
                const bool in_clamp = lv[s][k] >= -30.0f && lv[s][k] <= 20.0f;
                dm[s][k] = (float)(d_mean + c_kl * (double)mean[s][k]);
                dl[s][k] = in_clamp ? (float)(0.5 * sampled + c_kl * (0.5 * (sd[s] * sd[s] - 1.0))) : 0.0f;
            }
        }
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            if (!a.d_moments[s]) continue;
            float* o = a.d_moments[s] + 2 * b * D;
            vl_store4<VEC>(o, e0, D, dm[s]);
            vl_store4<VEC>(o + D, e0, D, dl[s]);
        }
    }
}

#define VLCK(c, what) HIPCK(c, hipGetLastError(), what)

}  // namespace

extern "C" {

size_t vt_vae_loss_backward_workspace_bytes(int B, int C, int hw, int H, int W) {
    if (!vl_shape_ok(B, C, hw) || H < 0 || W < 0 || ((H == 0) != (W == 0)) || (H > 0 && !vl_image_ok(H, W))) return 0;
    return vt_vae_loss_backward_layout(B, (long long)C * hw, 3ll * H * W).total;
}

int vt_vae_loss_backward(vt_context* c, const vt_vae_loss_input* anchor, const vt_vae_loss_input* positive, const vt_vae_loss_input* negative,
                         const float* dz_dec, int dz_draw, const float* recon, const float* target, int H, int W, const void* labels_a,
                         const void* labels_p, int labels_dtype, int N, int B, int C, int hw, unsigned long long seed, long long first_image,
                         double w_rec, double w_kl, double w_tri, double margin, int similarity, float* d_recon, float* d_moments_a,
                         float* d_moments_p, float* d_moments_n, double* rows_out, double* loss_out, void* workspace, size_t workspace_bytes,
                         void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    const char* who = "vt_vae_loss_backward";
    if (!vl_shape_ok(B, C, hw)) return c->fail(VT_ERR_INVALID, "%s: B = %d (1..%d), C = %d or hw = %d out of range", who, B, VT_EVAL_MAX_B, C, hw);
    if (!anchor || !positive) return c->fail(VT_ERR_INVALID, "%s: anchor and positive are required", who);
    if (!negative) return c->fail(VT_ERR_INVALID, "%s: a negative stream is required (the contrastive term has no gradient here)", who);
    if (first_image < 0 || dz_draw < 0) return c->fail(VT_ERR_INVALID, "%s: first_image and dz_draw are >= 0", who);
    if (similarity != VT_VAE_COSINE && similarity != VT_VAE_EUCLIDEAN) return c->fail(VT_ERR_INVALID, "%s: similarity is VT_VAE_COSINE or VT_VAE_EUCLIDEAN", who);
    if (!isfinite(w_rec) || !isfinite(w_kl) || !isfinite(w_tri) || !isfinite(margin))
        return c->fail(VT_ERR_INVALID, "%s: the weights and the margin must be finite", who);
    const long long D = (long long)C * hw;
    const vt_vae_loss_input* in[3] = {anchor, positive, negative};
    float* d_moments[3] = {d_moments_a, d_moments_p, d_moments_n};
    VaeLatentArg la;
    VlbGradArg ga;
    bool vec = D % 4 == 0, vec_grad = D % 4 == 0 && !vl_misaligned(dz_dec, 16);
    for (int s = 0; s < 3; ++s) {
        if (!in[s]->moments || in[s]->z) return c->fail(VT_ERR_INVALID, "%s: input %d needs its moments and takes no stored z", who, s);
        if (vl_misaligned(in[s]->moments, 4) || vl_misaligned(d_moments[s], 4)) return c->fail(VT_ERR_INVALID, "%s: moments or d_moments %d misaligned", who, s);
        if (in[s]->draw < 0) return c->fail(VT_ERR_INVALID, "%s: input %d has a negative draw", who, s);
        la.s[s].moments = in[s]->moments; la.s[s].z = nullptr; la.s[s].draw = in[s]->draw; la.s[s].present = 1;
        ga.moments[s] = in[s]->moments; ga.d_moments[s] = d_moments[s]; ga.draw[s] = in[s]->draw;
        vec = vec && !vl_misaligned(in[s]->moments, 16);
        vec_grad = vec_grad && !vl_misaligned(in[s]->moments, 16) && !vl_misaligned(d_moments[s], 16);
    }
    if (vl_misaligned(dz_dec, 4)) return c->fail(VT_ERR_INVALID, "%s: dz_dec is misaligned", who);
    if ((recon == nullptr) != (target == nullptr)) return c->fail(VT_ERR_INVALID, "%s: recon and target come together or not at all", who);
    if (d_recon && !recon) return c->fail(VT_ERR_INVALID, "%s: d_recon needs recon and target", who);
    if (recon && (!vl_image_ok(H, W) || vl_misaligned(recon, 4) || vl_misaligned(target, 4) || vl_misaligned(d_recon, 4)))
        return c->fail(VT_ERR_INVALID, "%s: H = %d, W = %d out of range, or recon / target / d_recon misaligned", who, H, W);
    if ((labels_a == nullptr) != (labels_p == nullptr)) return c->fail(VT_ERR_INVALID, "%s: labels_a and labels_p come together or not at all", who);
    if (labels_a && ((labels_dtype != VT_F32 && labels_dtype != VT_U8) || N < 1 || N > (1 << 24) ||
                     (labels_dtype == VT_F32 && (vl_misaligned(labels_a, 4) || vl_misaligned(labels_p, 4)))))
        return c->fail(VT_ERR_INVALID, "%s: labels neither VT_F32 nor VT_U8, misaligned, or N = %d outside [1, 2^24]", who, N);
    if (vl_misaligned(rows_out, 8) || vl_misaligned(loss_out, 8)) return c->fail(VT_ERR_INVALID, "%s: rows_out or loss_out is misaligned", who);
    const long long E = recon ? 3ll * H * W : 0;
    const VaeLossBackwardLayout l = vt_vae_loss_backward_layout(B, D, E);
    if (!workspace || vl_misaligned(workspace, ALIGN)) return c->fail(VT_ERR_INVALID, "%s: workspace is null or not 256-B aligned", who);
    if (workspace_bytes < l.total) return c->fail(VT_ERR_WORKSPACE, "%s: workspace holds %zu bytes, %zu needed", who, workspace_bytes, l.total);
    ga.dz_dec = dz_dec; ga.dz_draw = dz_draw; ga.euclidean = similarity == VT_VAE_EUCLIDEAN;
    VaeRowArg f;
    f.has_kl[0] = f.has_kl[1] = f.has_kl[2] = 1;
    f.has_n = 1; f.has_recon = recon != nullptr; f.has_labels = labels_a != nullptr;
    const VlbWeights wt = {w_rec, w_kl, w_tri, margin};

    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    double* rows = (double*)(ws + l.rows);
    double* lat = (double*)(ws + l.lat);
    double* img = (double*)(ws + l.img);
    double* coef = (double*)(ws + l.coef);
    double* batch = (double*)(ws + l.batch);
    unsigned long long* bad = (unsigned long long*)(rows + (size_t)VT_VAE_LOSS_ROW * B);
    const bool latent = d_moments_a || d_moments_p || d_moments_n || rows_out || loss_out;      // (d_recon alone needs no sum)
    if (recon && (d_recon || latent)) {
        const dim3 igrid((unsigned)l.img_chunks, (unsigned)B);
        const double scale = w_rec * 2.0 / ((double)B * (double)E);
        if (E % 4 == 0 && !vl_misaligned(recon, 16) && !vl_misaligned(target, 16) && !vl_misaligned(d_recon, 16))
            hipLaunchKernelGGL(vlb_image_kernel<true>, igrid, dim3(VL_T), 0, s, recon, target, E, l.img_chunks, scale, d_recon, latent ? img : nullptr);
        else
            hipLaunchKernelGGL(vlb_image_kernel<false>, igrid, dim3(VL_T), 0, s, recon, target, E, l.img_chunks, scale, d_recon, latent ? img : nullptr);
        VLCK(c, "vae_loss_backward image");
    }
    if (!latent) return VT_OK;
    const dim3 lgrid((unsigned)l.lat_chunks, (unsigned)B);
    if (vec) hipLaunchKernelGGL(vlb_latent_kernel<true>, lgrid, dim3(VL_T), 0, s, la, seed, D, first_image, l.lat_chunks, lat);
    else hipLaunchKernelGGL(vlb_latent_kernel<false>, lgrid, dim3(VL_T), 0, s, la, seed, D, first_image, l.lat_chunks, lat);
    VLCK(c, "vae_loss_backward latent");
    if (labels_a && labels_dtype == VT_U8)
        hipLaunchKernelGGL(vlb_coef_kernel<unsigned char>, dim3((unsigned)B), dim3(64), 0, s, f, wt, ga.euclidean, B, lat, l.lat_chunks, img, l.img_chunks, E,
                           (const unsigned char*)labels_a, (const unsigned char*)labels_p, N, rows, rows_out, bad, coef);
    else
        hipLaunchKernelGGL(vlb_coef_kernel<float>, dim3((unsigned)B), dim3(64), 0, s, f, wt, ga.euclidean, B, lat, l.lat_chunks, img, l.img_chunks, E,
                           (const float*)labels_a, (const float*)labels_p, N, rows, rows_out, bad, coef);
    VLCK(c, "vae_loss_backward coefficients");
    hipLaunchKernelGGL(vlb_batch_kernel, dim3(1), dim3(64), 0, s, wt, ga.euclidean, B, rows, batch, loss_out); VLCK(c, "vae_loss_backward batch");
    if (d_moments_a || d_moments_p || d_moments_n) {
        if (vec_grad) hipLaunchKernelGGL(vlb_grad_kernel<true>, lgrid, dim3(VL_T), 0, s, ga, seed, D, first_image, coef, batch);
        else hipLaunchKernelGGL(vlb_grad_kernel<false>, lgrid, dim3(VL_T), 0, s, ga, seed, D, first_image, coef, batch);
        VLCK(c, "vae_loss_backward gradient");
    }
    return VT_OK;
}

}  // extern "C"
