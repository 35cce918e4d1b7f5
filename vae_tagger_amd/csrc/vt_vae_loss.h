// VAE validation loss on the device: layout of the caller-owned state block and the counter-based normal draw (eval_vae_loss.hip; mirrored
// by vae_tagger_amd/vae_losses.py and vae_tagger_amd/improved_losses.py).
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

// ---- the draw: a standard normal per (seed, draw, image, element), no stored state ----
// stream key = mix64(seed + golden (draw + 1)); image key = mix64(stream key + odd (image + 1)); the element's two words are
// mix64(image key ^ 2e) and mix64(image key ^ (2e + 1)).  u1 = ((x1 >> 11) + 1) 2^-53 lies in (0, 1] -- never 0, it goes into the
// logarithm --, u2 = (x2 >> 11) 2^-53 in [0, 1).  Box-Muller in fp64, rounded to fp32 once.
VT_TRAIN_HD inline uint64_t vt_vae_stream_key(uint64_t seed, uint64_t draw) { return vt_head_mix64(seed + 0x9E3779B97F4A7C15ull * (draw + 1)); }
VT_TRAIN_HD inline uint64_t vt_vae_image_key(uint64_t stream_key, uint64_t image) {
    return vt_head_mix64(stream_key + 0xD1B54A32D192ED03ull * (image + 1));
}
