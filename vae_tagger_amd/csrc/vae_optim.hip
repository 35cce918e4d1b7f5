// The optimiser of the VAE train step: clip_grad_norm_ and AdamW over n freshly allocated fp32 gradient tensors, read where they lie.
// The block trainers (train_common.hip) own one state block whose kernels write the gradients into it; here the backward hands over 244
// tensors that change address every step, so their pointers travel in kernel arguments: a by-value table of { gradient, slot offset,
// numel } for up to VT_VAE_OPTIM_CHUNK tensors per launch (24 B each, 1.5 KB a table), a handful of launches per pass, no copy, no staging.
// Parameters, m and v live in three arenas of one layout (vt_vae_optim_layout): tensor i owns ceil(numel / VT_VAE_OPTIM_TILE) tiles, so a
// workgroup's tile lies inside one tensor and its global index -- which is where its squared-norm partial goes -- is fixed by the shapes.
// The trainers' conventions hold: fp32 storage, fp64 reductions in an order fixed by the shapes, no atomics, nothing synchronises the host.
#include <math.h>

#include "vt_common.h"
#include "vt_context.h"
#include "vt_train.h"

using namespace vt;

namespace {

constexpr long long TILE = VT_VAE_OPTIM_TILE;
constexpr int QUADS = VT_VAE_OPTIM_TILE / 4 / 256;          // float4s of a tile per thread
static_assert(VT_VAE_OPTIM_TILE % 1024 == 0, "a tile is a whole number of float4s per thread of a 256-thread workgroup");

struct OptimEntry { const float* g; long long off; long long numel; };     // off: the slot's first float in the arenas, a multiple of TILE
struct OptimTable { OptimEntry e[VT_VAE_OPTIM_CHUNK]; int count; };
static_assert(sizeof(OptimTable) <= 2048, "the table and the scalars beside it stay well under the 4 KB of kernel arguments");

// workgroup b of a launch -> its tensor (the last entry whose first tile is <= b; the entries' tiles follow each other) and the tile
// inside it.  b is uniform, so these are scalar loads from the argument block.
__device__ __forceinline__ int optim_find(const OptimTable& t, long long b, long long* tile) {
    const long long base = t.e[0].off / TILE;
    int lo = 0, hi = t.count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (t.e[mid].off / TILE - base <= b) lo = mid; else hi = mid - 1;
    }
    *tile = b - (t.e[lo].off / TILE - base);
    return lo;
}

// Thread j's float4s j, j + 256, ... of tile `tile` of a gradient: a gradient that is not 16-B aligned, and the float4 that the tensor's end
// cuts, are loaded one float at a time into the same places; what lies past numel is 0 and is never loaded.
__device__ __forceinline__ void optim_load_tile(const OptimEntry& e, long long tile, float4 (&x)[QUADS]) {
    const float* __restrict__ g = e.g;
    const bool vec = ((uintptr_t)g & 15) == 0;
    if (vec && (tile + 1) * TILE <= e.numel) {                  // a whole tile of an aligned tensor: every load is issued before the first use
#pragma unroll
        for (int r = 0; r < QUADS; ++r) x[r] = *(const float4*)(g + tile * TILE + 4 * ((long long)threadIdx.x + 256 * r));
    } else {
#pragma unroll
        for (int r = 0; r < QUADS; ++r) {
            const long long i = tile * TILE + 4 * ((long long)threadIdx.x + 256 * r);
            x[r] = float4{0.f, 0.f, 0.f, 0.f};
            if (i + 4 <= e.numel) {
                if (vec) x[r] = *(const float4*)(g + i);
                else { x[r].x = g[i]; x[r].y = g[i + 1]; x[r].z = g[i + 2]; x[r].w = g[i + 3]; }
            } else if (i < e.numel) {
                x[r].x = g[i];
                if (i + 1 < e.numel) x[r].y = g[i + 1];
                if (i + 2 < e.numel) x[r].z = g[i + 2];
            }
        }
    }
}

// One workgroup per tile.  Thread j owns the float4s j, j + 256, ... of the tile and adds their squares x, y, z, w in that order, in
// fp64 (optim_load_tile: the partial has the same bits whether the gradient is 16-B aligned or not).
__global__ __launch_bounds__(256) void vae_optim_sq_kernel(OptimTable t, double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double red[4];
    long long tile;
    const OptimEntry e = t.e[optim_find(t, blockIdx.x, &tile)];
    double sq = 0.0;
    float4 x[QUADS];
    optim_load_tile(e, tile, x);
#pragma unroll
    for (int r = 0; r < QUADS; ++r) {
        sq = sq + (double)x[r].x * (double)x[r].x;
        sq = sq + (double)x[r].y * (double)x[r].y;
        sq = sq + (double)x[r].z * (double)x[r].z;
        sq = sq + (double)x[r].w * (double)x[r].w;
    }
    const double total = block_sum_256d(sq, red);
    if (threadIdx.x == 0) part[e.off / TILE + tile] = total;
}

// one workgroup: the partials in an order fixed by their count -> { norm^2, norm, coef }, train_clip_kernel's formula
__global__ __launch_bounds__(256) void vae_optim_clip_kernel(const double* __restrict__ part, long long n, float max_norm, TrainScalars* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double red[4];
    // thread j adds partials j, j + 256, ... in that order, as four chains (index / 256 mod 4) whose loads do not wait for each other
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (long long i = threadIdx.x; i < n; i += 1024) {
        a0 += part[i];
        if (i + 256 < n) a1 += part[i + 256];
        if (i + 512 < n) a2 += part[i + 512];
        if (i + 768 < n) a3 += part[i + 768];
    }
    const double total = block_sum_256d(((a0 + a1) + a2) + a3, red);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(total);
        const float coef = max_norm / (norm + 1e-6f);
        TrainScalars v;
        v.sq = total; v.norm = norm; v.coef = coef < 1.0f ? coef : 1.0f;
        *out = v;
    }
}

// the joint clip of train_full, one workgroup: S_vae over the VAE's tile partials exactly as vae_optim_clip_kernel adds them, then S_blocks
// over the decoder-side blocks' partials exactly as train_clip_kernel adds them (head, front, cross; an absent block has n = 0), then ONE
// fp64 add, the VAE first -> { norm^2, norm, coef } by the same formula, the same 16 bytes to the VAE's scalars and to every present block's
struct JointBlocks { const double* part[VT_CLIP_MAX_BLOCKS]; int n[VT_CLIP_MAX_BLOCKS]; TrainScalars* sc[VT_CLIP_MAX_BLOCKS]; int count; };
__global__ __launch_bounds__(256) void full_optim_clip_kernel(const double* __restrict__ part, long long n, JointBlocks blocks, float max_norm,
                                                              TrainScalars* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double red[4];
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (long long i = threadIdx.x; i < n; i += 1024) {
        a0 += part[i];
        if (i + 256 < n) a1 += part[i + 256];
        if (i + 512 < n) a2 += part[i + 512];
        if (i + 768 < n) a3 += part[i + 768];
    }
    const double s_vae = block_sum_256d(((a0 + a1) + a2) + a3, red);
    double s_blocks = 0.0;
#pragma unroll
    for (int k = 0; k < VT_CLIP_MAX_BLOCKS; ++k) {
        const double* __restrict__ p = blocks.part[k];
        double a = 0.0;
        for (int i = threadIdx.x; i < blocks.n[k]; i += 256) a += p[i];
        const double t = block_sum_256d(a, red);
        s_blocks = k ? s_blocks + t : t;
    }
    if (threadIdx.x == 0) {
        const double total = s_vae + s_blocks;
        const float norm = (float)sqrt(total);
        const float coef = max_norm / (norm + 1e-6f);
        TrainScalars v;
        v.sq = total; v.norm = norm; v.coef = coef < 1.0f ? coef : 1.0f;
        *out = v;
#pragma unroll
        for (int k = 0; k < VT_CLIP_MAX_BLOCKS; ++k)
            if (k < blocks.count) *blocks.sc[k] = v;
    }
}

// the clip's scale folded in: g * coef as one fp32 multiply.  The product is pinned in a register: with -ffp-contract=fast on the
// command line the backend would fuse it into adamw_one's g - m whatever the pragma says, and the fused difference has other bits.
__device__ __forceinline__ float optim_scaled(float g, float coef, bool scale) {
#pragma clang fp contract(off)
    if (scale) {
        g = g * coef;
        asm volatile("" : "+v"(g));
    }
    return g;
}

struct AdamArgs { float decay, w1, beta2, w2, step_size, rbc2, eps; };

// One workgroup per tile, thread j on the float4s j, j + 256, ...  A float4 that lies inside the tensor: p, m, v are loaded and stored as
// float4 (the slot is 16-B aligned), g as a float4 when its pointer is 16-B aligned, else as four floats.  The float4 that the tensor's
// end cuts: one guarded float at a time, so a padding lane is never loaded from the gradient and never stored.  The gradient is only read.
// (VT_NO_PACKED_F32: the compiler would pair these float4 lanes into packed fp32 ops with a source op_sel -- vt_common.h)
__global__ __launch_bounds__(256) VT_NO_PACKED_F32 void vae_optim_adamw_kernel(OptimTable t, float* __restrict__ P, float* __restrict__ M, float* __restrict__ V,
                                                                              const TrainScalars* __restrict__ sc, AdamArgs a) {
    long long tile;
    const OptimEntry e = t.e[optim_find(t, blockIdx.x, &tile)];
    const float* __restrict__ g = e.g;
    const bool vec = ((uintptr_t)g & 15) == 0;
    const float coef = sc ? sc->coef : 1.0f;
    const bool scale = coef < 1.0f;
#pragma unroll
    for (int r = 0; r < QUADS; ++r) {
        const long long i = tile * TILE + 4 * ((long long)threadIdx.x + 256 * r);
        const long long o = e.off + i;
        if (i + 4 <= e.numel) {
            float4 x;
            if (vec) x = *(const float4*)(g + i);
            else { x.x = g[i]; x.y = g[i + 1]; x.z = g[i + 2]; x.w = g[i + 3]; }
            float4 p = *(float4*)(P + o), m = *(float4*)(M + o), v = *(float4*)(V + o);
            x.x = optim_scaled(x.x, coef, scale); x.y = optim_scaled(x.y, coef, scale);
            x.z = optim_scaled(x.z, coef, scale); x.w = optim_scaled(x.w, coef, scale);
            adamw_one(p.x, x.x, m.x, v.x, a.decay, a.w1, a.beta2, a.w2, a.step_size, a.rbc2, a.eps);
            adamw_one(p.y, x.y, m.y, v.y, a.decay, a.w1, a.beta2, a.w2, a.step_size, a.rbc2, a.eps);
            adamw_one(p.z, x.z, m.z, v.z, a.decay, a.w1, a.beta2, a.w2, a.step_size, a.rbc2, a.eps);
            adamw_one(p.w, x.w, m.w, v.w, a.decay, a.w1, a.beta2, a.w2, a.step_size, a.rbc2, a.eps);
            *(float4*)(P + o) = p; *(float4*)(M + o) = m; *(float4*)(V + o) = v;
        } else {
            for (int k = 0; k < 3; ++k) {
                if (i + k >= e.numel) break;
                float x = optim_scaled(g[i + k], coef, scale);
                float p = P[o + k], m = M[o + k], v = V[o + k];
                adamw_one(p, x, m, v, a.decay, a.w1, a.beta2, a.w2, a.step_size, a.rbc2, a.eps);
                P[o + k] = p; M[o + k] = m; V[o + k] = v;
            }
        }
    }
}

// The gradient exchange of a sharded train_vae: the n gradient tensors packed into ONE fp32 row of the arenas' layout, so that ranks can
// exchange and merge ranges of tiles.  One workgroup per tile, the loads of optim_load_tile, four float4 stores per thread: the rest of a
// tensor's last tile is written as zero, so a row needs no memset.
__global__ __launch_bounds__(256) void vae_grads_export_kernel(OptimTable t, float* __restrict__ row) {
    long long tile;
    const OptimEntry e = t.e[optim_find(t, blockIdx.x, &tile)];
    float4 x[QUADS];
    optim_load_tile(e, tile, x);
    float* __restrict__ dst = row + e.off + tile * TILE;
#pragma unroll
    for (int r = 0; r < QUADS; ++r) *(float4*)(dst + 4 * ((long long)threadIdx.x + 256 * r)) = x[r];
}

// the tiles of a row behind the layout's total (the padding that makes the owners' ranges equal): zero
__global__ __launch_bounds__(256) void vae_grads_zero_kernel(float* __restrict__ dst) {
    float* __restrict__ d = dst + (long long)blockIdx.x * TILE;
#pragma unroll
    for (int r = 0; r < QUADS; ++r) *(float4*)(d + 4 * ((long long)threadIdx.x + 256 * r)) = float4{0.f, 0.f, 0.f, 0.f};
}

// Gradient accumulation of train_full: the n fresh gradient tensors of one micro-step into ONE fp32 row of the arenas' layout that holds the
// sum across micro-steps.  t = scale * g, one fp32 multiply (skipped at scale == 1: the same bits).  FIRST: row = t over the whole tile,
// +0.0 past the tensor's end -- the export's stores, so every float of the tensor's tiles is written.  Otherwise a = row, a = coef * a when
// the scalars hold a coef < 1 (the clip of the micro-step before, applied here and nowhere else), row = a + t: two products and one add,
// each rounded on its own -- the products are pinned in registers because -ffp-contract=fast would fuse one into the add, pragma or not.
// The float4 that the tensor's end cuts goes one guarded float at a time: padding is neither read nor written.
__device__ __forceinline__ float accum_one(float a, float g, float scale, bool scaled, float coef, bool clipped) {
#pragma clang fp contract(off)
    if (scaled) g = g * scale;
    if (clipped) a = a * coef;
    asm volatile("" : "+v"(g), "+v"(a));
    return a + g;
}
template <bool FIRST>
__global__ __launch_bounds__(256) VT_NO_PACKED_F32 void vae_grads_accumulate_kernel(OptimTable t, float* __restrict__ row, float scale,
                                                                                    const TrainScalars* __restrict__ sc) {
#pragma clang fp contract(off)
    long long tile;
    const OptimEntry e = t.e[optim_find(t, blockIdx.x, &tile)];
    const bool scaled = scale != 1.0f;
    float4 x[QUADS];
    optim_load_tile(e, tile, x);
    float* __restrict__ dst = row + e.off + tile * TILE;
    if (FIRST) {
#pragma unroll
        for (int r = 0; r < QUADS; ++r) {
            const long long i = tile * TILE + 4 * ((long long)threadIdx.x + 256 * r);
            if (scaled) {                                       // (a lane past the end stays +0.0 under a negative scale too)
                if (i < e.numel) x[r].x = x[r].x * scale;
                if (i + 1 < e.numel) x[r].y = x[r].y * scale;
                if (i + 2 < e.numel) x[r].z = x[r].z * scale;
                if (i + 3 < e.numel) x[r].w = x[r].w * scale;
            }
            *(float4*)(dst + 4 * ((long long)threadIdx.x + 256 * r)) = x[r];
        }
    } else {
        const float coef = sc ? sc->coef : 1.0f;
        const bool clipped = coef < 1.0f;                       // a NaN or >= 1 coefficient multiplies nothing (vae_optim_adamw_kernel's rule)
#pragma unroll
        for (int r = 0; r < QUADS; ++r) {
            const long long q = 4 * ((long long)threadIdx.x + 256 * r), i = tile * TILE + q;
            if (i + 4 <= e.numel) {
                float4 a = *(float4*)(dst + q);
                a.x = accum_one(a.x, x[r].x, scale, scaled, coef, clipped); a.y = accum_one(a.y, x[r].y, scale, scaled, coef, clipped);
                a.z = accum_one(a.z, x[r].z, scale, scaled, coef, clipped); a.w = accum_one(a.w, x[r].w, scale, scaled, coef, clipped);
                *(float4*)(dst + q) = a;
            } else if (i < e.numel) {
                dst[q] = accum_one(dst[q], x[r].x, scale, scaled, coef, clipped);
                if (i + 1 < e.numel) dst[q + 1] = accum_one(dst[q + 1], x[r].y, scale, scaled, coef, clipped);
                if (i + 2 < e.numel) dst[q + 2] = accum_one(dst[q + 2], x[r].z, scale, scaled, coef, clipped);
            }
        }
    }
}

// out[e] = (float)(w[0] x_0 + w[1] x_1 + ... + w[K-1] x_{K-1}), x_r = rows[r * stride + first + e], in fp64, added in that order, every
// product and every sum rounded on its own (train_merge_kernel's arithmetic, except that the first product is not added to 0.0: with
// K = 1 and w = 1 the merge is the identity on every bit pattern of a number, -0.0 included).  One workgroup per tile of the range, thread
// j on float4s j, j + 256, ...; the ranks are taken MERGE_GROUP at a time and a group's loads of a float4 position are all issued before
// its first add, so at K = 8 a wave has eight independent loads in flight per position.  A rank whose weight is 0 is still read.
constexpr int MERGE_GROUP = 8;
struct MergeWeights { double w[VT_MERGE_MAX_RANKS]; };
__global__ __launch_bounds__(256) VT_NO_PACKED_F32 void vae_grads_merge_kernel(const float* __restrict__ rows, long long stride, int K, MergeWeights w,
                                                                               float* __restrict__ out) {
#pragma clang fp contract(off)
    const long long base = (long long)blockIdx.x * TILE + 4 * (long long)threadIdx.x;      // (rows already points at first_float)
#pragma unroll
    for (int q = 0; q < QUADS; ++q) {
        const long long i = base + 1024 * q;
        double ax = 0.0, ay = 0.0, az = 0.0, aw = 0.0;
        for (int r0 = 0; r0 < K; r0 += MERGE_GROUP) {
            float4 v[MERGE_GROUP];
#pragma unroll
            for (int k = 0; k < MERGE_GROUP; ++k)
                if (r0 + k < K) v[k] = *(const float4*)(rows + (long long)(r0 + k) * stride + i);
#pragma unroll
            for (int k = 0; k < MERGE_GROUP; ++k) {
                if (r0 + k < K) {
                    const double wr = w.w[r0 + k];
                    double px = wr * (double)v[k].x, py = wr * (double)v[k].y, pz = wr * (double)v[k].z, pw = wr * (double)v[k].w;
                    // (pinned: -ffp-contract=fast on the command line would fuse a product into the add that follows, pragma or not)
                    asm volatile("" : "+v"(px), "+v"(py), "+v"(pz), "+v"(pw));
                    if (r0 + k == 0) { ax = px; ay = py; az = pz; aw = pw; }
                    else { ax = ax + px; ay = ay + py; az = az + pz; aw = aw + pw; }
                }
            }
        }
        float4 o;
        o.x = (float)ax; o.y = (float)ay; o.z = (float)az; o.w = (float)aw;
        *(float4*)(out + i) = o;
    }
}

// the arguments both entry points share: n, the tensors, the chunk; `total` = floats of an arena, `tiles` = total / TILE
int optim_check(vt_context* c, const char* who, const float* const* grads, const long long* numel, int n, int chunk, long long* total) {
    if (n < 1 || !grads || !numel) return c->fail(VT_ERR_INVALID, "%s: n = %d tensors (>= 1) with host arrays of gradients and numels expected", who, n);
    if (chunk < 0 || chunk > VT_VAE_OPTIM_CHUNK) return c->fail(VT_ERR_INVALID, "%s: chunk = %d, 0 or 1 to %d expected", who, chunk, VT_VAE_OPTIM_CHUNK);
    long long off = 0;
    for (int i = 0; i < n; ++i) {
        if (numel[i] <= 0 || numel[i] > (1ll << 40)) return c->fail(VT_ERR_INVALID, "%s: tensor %d has numel = %lld, 1 to 2^40 expected", who, i, numel[i]);
        if (!grads[i] || ((uintptr_t)grads[i] & 3)) return c->fail(VT_ERR_INVALID, "%s: gradient %d is null or not 4-B aligned", who, i);
        off += (numel[i] + TILE - 1) / TILE * TILE;
    }
    *total = off;
    return VT_OK;
}

// what the two norm entries check beyond optim_check: the bound, the scalars and the partials' workspace
int norm_check(vt_context* c, const char* who, const float* const* grads, const long long* numel, int n, float max_norm, const void* scalars_out,
               const void* workspace, size_t workspace_bytes, int chunk, long long* total) {
    VTCK(optim_check(c, who, grads, numel, n, chunk, total));
    if (!(max_norm > 0.f)) return c->fail(VT_ERR_INVALID, "%s: max_norm = %g must be positive", who, max_norm);
    if (!scalars_out || ((uintptr_t)scalars_out & 15)) return c->fail(VT_ERR_INVALID, "%s: scalars_out is null or not 16-B aligned", who);
    if (!workspace || ((uintptr_t)workspace & (ALIGN - 1))) return c->fail(VT_ERR_INVALID, "%s: workspace is null or not 256-B aligned", who);
    const size_t need = align_up(sizeof(double) * (size_t)(*total / TILE));
    if (workspace_bytes < need) return c->fail(VT_ERR_WORKSPACE, "%s: workspace holds %zu bytes, %zu needed", who, workspace_bytes, need);
    return VT_OK;
}

// the tensors `chunk` at a time: launch(table, tiles of the table)
template <class Launch>
int optim_chunks(vt_context* c, const char* who, const float* const* grads, const long long* numel, int n, int chunk, Launch&& launch) {
    if (chunk == 0) chunk = VT_VAE_OPTIM_CHUNK;
    long long off = 0;
    for (int first = 0; first < n; first += chunk) {
        OptimTable t;
        t.count = n - first < chunk ? n - first : chunk;
        long long tiles = 0;
        for (int k = 0; k < VT_VAE_OPTIM_CHUNK; ++k) {
            if (k < t.count) {
                const long long nt = (numel[first + k] + TILE - 1) / TILE;
                t.e[k].g = grads[first + k]; t.e[k].off = off; t.e[k].numel = numel[first + k];
                off += nt * TILE; tiles += nt;
            } else {
                t.e[k].g = nullptr; t.e[k].off = 0; t.e[k].numel = 0;
            }
        }
        if (tiles > 0x7fffffffll) return c->fail(VT_ERR_INVALID, "%s: %lld tiles in one launch", who, tiles);
        launch(t, (unsigned)tiles);
        HIPCK(c, hipGetLastError(), who);
    }
    return VT_OK;
}

}  // namespace

extern "C" {

int vt_vae_optim_layout(const long long* numel, int n, long long* offsets_out, long long* total_out) {
    if (n < 1 || !numel) return VT_ERR_INVALID;
    for (int i = 0; i < n; ++i)
        if (numel[i] <= 0 || numel[i] > (1ll << 40)) return VT_ERR_INVALID;
    long long off = 0;
    for (int i = 0; i < n; ++i) {
        if (offsets_out) offsets_out[i] = off;
        off += (numel[i] + TILE - 1) / TILE * TILE;
    }
    if (total_out) *total_out = off;
    return VT_OK;
}

size_t vt_vae_optim_workspace_bytes(const long long* numel, int n) {
    long long total = 0;
    if (vt_vae_optim_layout(numel, n, nullptr, &total) != VT_OK) return 0;
    return align_up(sizeof(double) * (size_t)(total / TILE));
}

int vt_vae_optim_norm(vt_context* c, const float* const* grads, const long long* numel, int n, float max_norm, void* scalars_out, void* workspace,
                      size_t workspace_bytes, int chunk, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    const char* who = "vt_vae_optim_norm";
    long long total = 0;
    VTCK(norm_check(c, who, grads, numel, n, max_norm, scalars_out, workspace, workspace_bytes, chunk, &total));
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)workspace;
    VTCK(optim_chunks(c, who, grads, numel, n, chunk, [&](const OptimTable& t, unsigned tiles) {
        hipLaunchKernelGGL(vae_optim_sq_kernel, dim3(tiles), dim3(256), 0, s, t, part);
    }));
    hipLaunchKernelGGL(vae_optim_clip_kernel, dim3(1), dim3(256), 0, s, (const double*)part, total / TILE, max_norm, (TrainScalars*)scalars_out);
    HIPCK(c, hipGetLastError(), who);
    return VT_OK;
}

int vt_full_optim_norm(vt_context* c, const float* const* grads, const long long* numel, int n, float max_norm, void* scalars_out, void* workspace,
                       size_t workspace_bytes, int chunk, void* head_state, size_t head_state_bytes, void* front_state, size_t front_state_bytes,
                       void* cross_state, size_t cross_state_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    const char* who = "vt_full_optim_norm";
    long long total = 0;
    VTCK(norm_check(c, who, grads, numel, n, max_norm, scalars_out, workspace, workspace_bytes, chunk, &total));
    DecoderBlocks d;
    VTCK(vt_train_decoder_blocks(c, who, head_state, head_state_bytes, front_state, front_state_bytes, cross_state, cross_state_bytes, &d));
    JointBlocks k;
    for (int i = 0; i < VT_CLIP_MAX_BLOCKS; ++i) {
        const TrainBlockRef& b = d.ref[i < d.n ? i : 0];
        k.part[i] = (const double*)((char*)b.state + b.layout->normpart);
        k.n[i] = i < d.n ? b.layout->norm_parts : 0;
        k.sc[i] = (TrainScalars*)((char*)b.state + b.layout->scalars);
    }
    k.count = d.n;
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)workspace;
    VTCK(optim_chunks(c, who, grads, numel, n, chunk, [&](const OptimTable& t, unsigned tiles) {
        hipLaunchKernelGGL(vae_optim_sq_kernel, dim3(tiles), dim3(256), 0, s, t, part);
    }));
    hipLaunchKernelGGL(full_optim_clip_kernel, dim3(1), dim3(256), 0, s, (const double*)part, total / TILE, k, max_norm, (TrainScalars*)scalars_out);
    HIPCK(c, hipGetLastError(), who);
    return vt_train_scale_blocks(c, who, d.ref, d.n, s);
}

int vt_vae_optim_step(vt_context* c, float* params, float* m, float* v, size_t arena_floats, const float* const* grads, const long long* numel, int n,
                      const void* scalars, double lr, double beta1, double beta2, double eps, double weight_decay, long long t, int chunk,
                      void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    const char* who = "vt_vae_optim_step";
    long long total = 0;
    VTCK(optim_check(c, who, grads, numel, n, chunk, &total));
    if (!params || !m || !v || (((uintptr_t)params | (uintptr_t)m | (uintptr_t)v) & (ALIGN - 1)))
        return c->fail(VT_ERR_INVALID, "%s: params, m or v is null or not 256-B aligned", who);
    if (arena_floats < (size_t)total) return c->fail(VT_ERR_INVALID, "%s: the arenas hold %zu floats, %lld needed", who, arena_floats, total);
    if ((uintptr_t)scalars & 15) return c->fail(VT_ERR_INVALID, "%s: scalars is not 16-B aligned", who);
    if (t < 1 || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !isfinite(lr) || !isfinite(weight_decay))
        return c->fail(VT_ERR_INVALID, "%s: t >= 1, betas in [0, 1), eps >= 0 and finite lr / weight_decay expected", who);
    const double bc1 = 1.0 - pow(beta1, (double)t), bc2 = 1.0 - pow(beta2, (double)t);
    const AdamArgs a = {(float)(1.0 - lr * weight_decay), (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)(lr / bc1), (float)sqrt(bc2),
                        (float)eps};
    hipStream_t s = (hipStream_t)stream;
    return optim_chunks(c, who, grads, numel, n, chunk, [&](const OptimTable& tb, unsigned tiles) {
        hipLaunchKernelGGL(vae_optim_adamw_kernel, dim3(tiles), dim3(256), 0, s, tb, params, m, v, (const TrainScalars*)scalars, a);
    });
}

int vt_vae_grads_export(vt_context* c, const float* const* grads, const long long* numel, int n, float* row, size_t row_floats, int chunk,
                        void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    const char* who = "vt_vae_grads_export";
    long long total = 0;
    VTCK(optim_check(c, who, grads, numel, n, chunk, &total));
    if (!row || ((uintptr_t)row & (ALIGN - 1))) return c->fail(VT_ERR_INVALID, "%s: row is null or not 256-B aligned", who);
    if (row_floats % TILE || row_floats < (size_t)total)
        return c->fail(VT_ERR_INVALID, "%s: a row of %zu floats, a multiple of %lld that is at least %lld expected", who, row_floats, TILE, total);
    const long long pad_tiles = ((long long)row_floats - total) / TILE;
    if (pad_tiles > 0x7fffffffll) return c->fail(VT_ERR_INVALID, "%s: %lld tiles of padding in one launch", who, pad_tiles);
    hipStream_t s = (hipStream_t)stream;
    VTCK(optim_chunks(c, who, grads, numel, n, chunk, [&](const OptimTable& t, unsigned tiles) {
        hipLaunchKernelGGL(vae_grads_export_kernel, dim3(tiles), dim3(256), 0, s, t, row);
    }));
    if (pad_tiles) {
        hipLaunchKernelGGL(vae_grads_zero_kernel, dim3((unsigned)pad_tiles), dim3(256), 0, s, row + total);
        HIPCK(c, hipGetLastError(), who);
    }
    return VT_OK;
}

int vt_vae_grads_accumulate(vt_context* c, const float* const* grads, const long long* numel, int n, float* row, size_t row_floats, float scale,
                            const void* scalars, int first, int chunk, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    const char* who = "vt_vae_grads_accumulate";
    long long total = 0;
    VTCK(optim_check(c, who, grads, numel, n, chunk, &total));
    if (!row || ((uintptr_t)row & (ALIGN - 1))) return c->fail(VT_ERR_INVALID, "%s: row is null or not 256-B aligned", who);
    if (row_floats % TILE || row_floats < (size_t)total)
        return c->fail(VT_ERR_INVALID, "%s: a row of %zu floats, a multiple of %lld that is at least %lld expected", who, row_floats, TILE, total);
    if (!isfinite(scale)) return c->fail(VT_ERR_INVALID, "%s: scale = %g must be finite", who, (double)scale);
    if ((uintptr_t)scalars & 15) return c->fail(VT_ERR_INVALID, "%s: scalars is not 16-B aligned", who);
    const long long pad_tiles = ((long long)row_floats - total) / TILE;
    if (pad_tiles > 0x7fffffffll) return c->fail(VT_ERR_INVALID, "%s: %lld tiles of padding in one launch", who, pad_tiles);
    hipStream_t s = (hipStream_t)stream;
    const TrainScalars* sc = (const TrainScalars*)scalars;
    VTCK(optim_chunks(c, who, grads, numel, n, chunk, [&](const OptimTable& t, unsigned tiles) {
        if (first) hipLaunchKernelGGL(vae_grads_accumulate_kernel<true>, dim3(tiles), dim3(256), 0, s, t, row, scale, sc);
        else hipLaunchKernelGGL(vae_grads_accumulate_kernel<false>, dim3(tiles), dim3(256), 0, s, t, row, scale, sc);
    }));
    if (first && pad_tiles) {                                    // (an accumulating call leaves the zeros the first one wrote)
        hipLaunchKernelGGL(vae_grads_zero_kernel, dim3((unsigned)pad_tiles), dim3(256), 0, s, row + total);
        HIPCK(c, hipGetLastError(), who);
    }
    return VT_OK;
}

int vt_vae_grads_merge(vt_context* c, const float* rows, size_t row_stride_floats, int K, const double* weights, size_t first_float, size_t floats,
                       float* out, void* stream) {
    if (!c) return VT_ERR_INVALID;
    DeviceGuard guard(c);
    const char* who = "vt_vae_grads_merge";
    if (K < 1 || K > VT_MERGE_MAX_RANKS) return c->fail(VT_ERR_INVALID, "%s: K = %d ranks, 1 to %d expected", who, K, VT_MERGE_MAX_RANKS);
    if (!rows || ((uintptr_t)rows & 15) || !out || ((uintptr_t)out & 15)) return c->fail(VT_ERR_INVALID, "%s: rows or out is null or not 16-B aligned", who);
    if (floats == 0 || floats % TILE || first_float % TILE || floats / TILE > 0x7fffffffull)
        return c->fail(VT_ERR_INVALID, "%s: first_float = %zu and floats = %zu, multiples of %lld with floats > 0 expected", who, first_float, floats, TILE);
    if (row_stride_floats % 4 || first_float + floats > row_stride_floats)
        return c->fail(VT_ERR_INVALID, "%s: a row stride of %zu floats, a multiple of 4 that holds first_float + floats = %zu expected", who,
                       row_stride_floats, first_float + floats);
    if (!weights) return c->fail(VT_ERR_INVALID, "%s: weights is null", who);
    MergeWeights w;
    for (int r = 0; r < VT_MERGE_MAX_RANKS; ++r) {
        w.w[r] = r < K ? weights[r] : 0.0;
        if (!isfinite(w.w[r]) || w.w[r] < 0.0) return c->fail(VT_ERR_INVALID, "%s: weight %d = %g must be finite and non-negative", who, r, w.w[r]);
    }
    hipLaunchKernelGGL(vae_grads_merge_kernel, dim3((unsigned)(floats / TILE)), dim3(256), 0, (hipStream_t)stream, rows + first_float,
                       (long long)row_stride_floats, K, w, out);
    HIPCK(c, hipGetLastError(), who);
    return VT_OK;
}

}  // extern "C"
