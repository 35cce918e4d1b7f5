// What the mid-block attention kernels share: the pieces of the two hand-tuned skeletons -- "rows resident in
// registers, the other operand streamed through LDS" (attn_qk.hip, attn_bwd.hip's attn_bwd_qk_kernel; in e4m3 attn_fp8.hip's
// attn_qk_fp8_kernel and proj_fp8_kernel) and "P in MFMA fragment order, v^T through LDS" (attn_pv.hip, attn_bwd.hip's
// attn_bwd_pv_kernel, attn_fp8.hip's attn_pv_fp8_kernel) -- their tile decodes, the fragment-order piece addressing and the launchers'
// grid rule.  Everything here is a device inline, a host inline or a template: every kernel is still a __global__ of its own unit.
// Epilogues, every wait and its count, and the order of stage, MFMAs, epilogue and store around the barrier are NOT here: they are
// what the kernels differ in.
// Inlining is not neutral in a 250-VGPR kernel, and a helper is optimised on its own before it is inlined.  So the scalar operands of
// the decode come by const reference, and the staging pieces are OBJECTS that hold references to the kernel's operands, as the lambdas
// they replace did in their closures: with plain values no kernel compiles to the code it had.  What could not be shared in any form
// that leaves every kernel's code alone is listed in section 4.28 and stays spelled out in the kernels.  (Such an object lives in the
// kernel's scope beside the variables it refers to, as a closure would; it is not meant to be copied out of it.)
#pragma once
#include "vt_halo.h"
#include "vt_kernels.h"

namespace vt_attn {
constexpr int QB = 256;        // resident (query) rows per workgroup (8 waves x 32)
constexpr int D = 512;         // head dim (= channels of the mid block)
namespace b16 {                // bf16 operands
constexpr int KT = 64;         // streamed rows (keys) per LDS tile
constexpr int KROWB = D * 2;   // bytes per streamed row in LDS
constexpr int KBUF = KT * KROWB;
constexpr int ROWB = KT * 2;   // P.V: bytes per LDS row (one channel, 64 keys)
constexpr int PT_TILE = 2048;  // elements of a (32-row slab, key tile) of the fragment-ordered P: 4 pieces x 64 lanes x 8
}  // namespace b16
namespace e4m3 {               // e4m3 operands: byte rows
constexpr int KT = 128;        // keys per LDS tile = one k-step of P.V
constexpr int KROWB = D;       // bytes per key row in LDS
constexpr int KBUF = KT * KROWB;    // 64 KB
constexpr int ROWB = KT;       // P.V: bytes per LDS row of the v^T tile (one channel, 128 keys)
}  // namespace e4m3
}  // namespace vt_attn

// ---- tile decodes ---------------------------------------------------------------------------------------------------------------------
// Q.K^T type: one workgroup per (image, block of 256 resident rows, split of the streamed sweep).  An XCD gets a contiguous range of
// workgroups = the query tiles of one image (or a few): its L2 keeps that image's keys.  The splits of a query block are neighbours:
// they share its Q rows in L2.  (rows and nsplit by reference, row0 formed where the kernel asks for it: see above.)
struct VtAttnQkTile {
    int b, qt, ksp, nsplit;    // image, block of resident rows, this workgroup's split of the sweep, number of splits (>= 1)
    __device__ __forceinline__ int row0(int wave) const { return qt * vt_attn::QB + wave * 32; }      // first row of a wave's 32-row slab
};
__device__ __forceinline__ VtAttnQkTile vt_attn_qk_tile(const int& rows, const int& nsplit_arg) {
    const int qtiles = (rows + vt_attn::QB - 1) / vt_attn::QB;
    const int nsplit = nsplit_arg > 1 ? nsplit_arg : 1;
    const int logical = vt_xcd_remap(blockIdx.x, gridDim.x);
    const int per_img = qtiles * nsplit;
    const int b = logical / per_img, qs = logical - b * per_img;
    const int qt = qs / nsplit, ksp = qs - qt * nsplit;
    return {b, qt, ksp, nsplit};
}
// P.V type: one workgroup per (image, query block, part of CB channels); the parts of a query block are neighbours in launch order, so
// the later reads of its P stream hit L2.  slab = this wave's 32-query slab of the image; slab_real: it holds at least one query.
struct VtAttnPvTile {
    int cb, b, qb, slab;
    bool slab_real;
};
template <int CB>
__device__ __forceinline__ VtAttnPvTile vt_attn_pv_tile(int S, int wave) {
    constexpr int NCP = vt_attn::D / CB;               // channel parts per query block
    const int qblocks = (S + vt_attn::QB - 1) / vt_attn::QB;
    const int logical = vt_xcd_remap(blockIdx.x, gridDim.x);
    const int cb = logical % NCP;                      // channel part: neighbours share the P stream
    const int rest = logical / NCP;
    const int b = rest / qblocks, qb = rest - b * qblocks;
    const int nslab = (S + 31) / 32;
    const int slab = qb * 8 + wave;
    return {cb, b, qb, slab, slab < nslab};
}

// ---- fragment-order pieces ------------------------------------------------------------------------------------------------------------
// The bf16 pieces of a (32-row slab, 64-key tile), as attn_qk's epilogue holds them: piece (j, h) of lane (fq, fr) = row 16 j + fr, keys
// 32 h + 8 fq .. + 7 -- the B operand of v_mfma_f32_16x16x32_bf16 for out^T[c][q] = sum_k v^T[c][k] P[q][k].  Stored as they stand: 1 KB
// contiguous per instruction, a wave's stream over the key tiles sequential in memory, tile kt at kt * PT_TILE elements.  Nontemporal both
// ways: a piece is written once and read by the two or four workgroups of its query block.
// Lane `lane`'s first piece of slab `slab`, tile 0, of the image whose P begins at `img`:
template <typename T>
__device__ __forceinline__ T* vt_attn_frag_base(T* img, int S, int slab, int lane) { return img + (long long)slab * vt_attn_pt_slab_stride(S) + lane * 8; }
// the four pieces of a lane at `s` = its first piece of the (slab, tile)
__device__ __forceinline__ void vt_attn_frag_load(bf16x8 (&d)[2][2], const bf16_t* s) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int h = 0; h < 2; ++h) d[j][h] = __builtin_nontemporal_load((const bf16x8*)(s + (j * 2 + h) * 512));
}
__device__ __forceinline__ void vt_attn_frag_store(bf16_t* dst, const bf16x8 (&v)[2][2]) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int h = 0; h < 2; ++h) __builtin_nontemporal_store(v[j][h], (bf16x8*)(dst + (j * 2 + h) * 512));
}

// ---- Q.K^T type, e4m3 (v_mfma_scale_f32_16x16x128_f8f6f4: a lane holds 32 consecutive k-bytes of its row) ---------------------------------
// Key tile staging: one wave-instruction = 2 key rows (1 KB); lane l -> row (l >> 5), physical 16-B chunk (l & 31), which holds
// logical chunk (l & 31) ^ (R & 15) (R = LDS row): the 16 rows a fragment read touches hit 16 different chunk slots.
// With R = 2 (8 jj + wave) + (lane >> 5): row tile m = jj and r = 2 wave + (lane >> 5) for every jj, so a lane's eight source
// addresses of a tile differ by wave-uniform offsets only (kept that way on purpose: eight hoisted 64-bit per-lane addresses spill).
struct VtAttn8QkStage {
    const unsigned char* const& kb;    // the image's streamed operand, nkeys rows of pitch ldk
    const int &ldk, &nkeys;
    const void* const& zeros;
    const int& wave;
    const int sr_, skey, schunk;       // r of this lane's rows; their key inside the block, before the row tile's 16 (m >> 2) + 4 (m & 3); the chunk's byte offset
    __device__ __forceinline__ VtAttn8QkStage(const unsigned char* const& kb_, const int& ldk_, const int& nkeys_, const void* const& zeros_, const int& wave_, int lane)
        : kb(kb_), ldk(ldk_), nkeys(nkeys_), zeros(zeros_), wave(wave_), sr_(2 * wave_ + (lane >> 5)), skey(32 * (sr_ >> 2) + (sr_ & 3)), schunk(((lane & 31) ^ sr_) << 4) {}
    __device__ __forceinline__ void operator()(char* smem, int kt, int buf) const {
        using namespace vt_attn::e4m3;
        const int key_l = kt * KT + vt_opaque(skey);
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            const int key = key_l + 16 * (jj >> 2) + 4 * (jj & 3);
            const void* src = key < nkeys ? (const void*)(kb + (long long)key * ldk + schunk) : zeros;
            __builtin_amdgcn_global_load_lds(VT_GLOBAL_PTR(src), VT_LDS_PTR(smem + buf * KBUF + (jj * 8 + wave) * 1024), 16, 0, 0);
        }
    }
};
// The 32 MFMAs of HALF H (four row tiles, 64 keys) of a 128-key tile; kbase[ks & 1][half] = the kernel's per-lane fragment offsets.
// Key fragments (32 B per lane = two ds_read_b128) through a ring of register sets, read AHEAD positions before their MFMAs.
template <int H>
__device__ __forceinline__ void vt_attn8_qk_mfma_half(f32x4 (&acc)[4][2], const i32x8 (&qf)[2][4], const char* ks_base, const int (&kbase)[2][2]) {
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    constexpr int AHEAD = 3, RING = 4;
    i32x8 kf[RING];
    auto frag = [&](int idx) __attribute__((always_inline)) -> i32x8 {
        const int ks = idx >> 2, m = 4 * H + (idx & 3);
        const char* p = ks_base + (ks >> 1) * 256 + m * 16 * vt_attn::e4m3::KROWB;
        return vt_cat8(*(const i32x4*)(p + kbase[ks & 1][0]), *(const i32x4*)(p + kbase[ks & 1][1]));
    };
#pragma unroll
    for (int p = 0; p < AHEAD; ++p) kf[p] = frag(p);
#pragma unroll
    for (int idx = 0; idx < 16; ++idx) {
        if (idx + AHEAD < 16) kf[(idx + AHEAD) % RING] = frag(idx + AHEAD);
        const int ks = idx >> 2, mm = idx & 3;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            acc[mm][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(kf[idx % RING], qf[j][ks], ks == 0 ? zero4 : acc[mm][j], 0, 0, 0, 127, 0, 127);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// ---- P.V type -------------------------------------------------------------------------------------------------------------------------
// v^T tile staging (T = bf16_t: 64 keys per tile; unsigned char: 128): one wave-instruction = 8 LDS rows x 128 B; lane l -> row (l >> 3),
// physical chunk (l & 7), logical chunk = physical ^ (row & 7); LDS row R holds channel (R & ~63) + (R & 3) + 4 ((R >> 4) & 3) +
// 16 ((R >> 2) & 3) (interleaved cout map of conv_gemm.hip: a lane ends up with 16 consecutive channels).  Keys >= kext (the written
// extent of v^T) come from the zero page.
template <int CB, typename T>
struct VtAttnPvStage {
    const T* const& vb;        // the workgroup's CB rows (channels) of v^T, pitch ldv
    const int &ldv, &kext;
    const void* const& zeros;
    const int& wave;
    const int lrow, lchunk;
    __device__ __forceinline__ VtAttnPvStage(const T* const& vb_, const int& ldv_, const int& kext_, const void* const& zeros_, const int& wave_, int lane)
        : vb(vb_), ldv(ldv_), kext(kext_), zeros(zeros_), wave(wave_), lrow(lane >> 3), lchunk((lane & 7) ^ (lane >> 3)) {}
    __device__ __forceinline__ void operator()(char* smem, int kt, int buf) const {     // tile kt into buffer buf (CB rows x 128 B each)
        constexpr int CHUNK = 16 / (int)sizeof(T);     // elements per 16-B chunk; a tile is 8 chunks of keys
#pragma unroll
        for (int jj = 0; jj < CB / 64; ++jj) {
            const int R = (jj * 8 + wave) * 8 + lrow;
            const int ch = (R & ~63) + (R & 3) + 4 * ((R >> 4) & 3) + 16 * ((R >> 2) & 3);
            const int key = kt * (8 * CHUNK) + lchunk * CHUNK;
            const void* src = key < kext ? (const void*)(vb + (long long)ch * ldv + key) : zeros;
            __builtin_amdgcn_global_load_lds(VT_GLOBAL_PTR(src), VT_LDS_PTR(smem + buf * (CB * 128) + (jj * 8 + wave) * 1024), 16, 0, 0);
        }
    }
};
// A fragment (channel tile ct, key half h) of a bf16 v^T tile: LDS row ct*16 + fr, logical chunk 4 h + fq -> physical ^ (row & 7) = ^ (fr & 7)
__device__ __forceinline__ void vt_attn_pv_foff(int (&foff)[2], int fr, int fq) {
    foff[0] = fr * vt_attn::b16::ROWB + (((0 + fq) ^ (fr & 7)) << 4);
    foff[1] = fr * vt_attn::b16::ROWB + (((4 + fq) ^ (fr & 7)) << 4);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
// Grid of a P.V-type launch: two 256-channel workgroups per query block, or four 128-channel ones (`narrow`) when the wide form would
// give fewer than 192 workgroups: it would leave a quarter or more of the 256 CUs without one (batch 1 at 1024^2 has 64 query blocks,
// 128 wide workgroups; the narrow form fills the chip).  The caller answers nblk > 2^31 - 1 with hipErrorInvalidValue.
struct VtAttnPvGrid {
    long long nblk;
    bool narrow;
};
inline VtAttnPvGrid vt_attn_pv_grid(int S, int batch) {
    const long long qblk = (long long)((S + vt_attn::QB - 1) / vt_attn::QB) * batch;
    const bool narrow = qblk * 2 < 192;
    return {qblk * (narrow ? 4 : 2), narrow};
}
// What the two linear forms of vt_launch_attn_qk (modes 4 and 5) ask of their arguments alike; `min_ldp`: the smallest pitch of the output
inline bool vt_attn_linear_args_ok(const AttnQkArgs& a, int min_ldp) {
    if (!a.q || !a.k || !a.zeros || a.batch <= 0 || a.C != vt_attn::D || a.S <= 0 || a.nk <= 0 || a.gate) return false;
    if ((a.ldq % 8) || (a.ldk % 8) || (a.qk_bs % 8) || (a.k_bs % 8) || (a.ldp % 8) || (a.p_bs % 8) || a.ldp < min_ldp) return false;
    if ((long long)a.S * a.ldq >= (1LL << 31) || (long long)a.nk * a.ldk >= (1LL << 31)) return false;
    const int nsp = a.nsplit > 1 ? a.nsplit : 1;
    if (nsp > (a.nk + vt_attn::b16::KT - 1) / vt_attn::b16::KT) return false;
    return (long long)((a.S + vt_attn::QB - 1) / vt_attn::QB) * a.batch * nsp <= 0x7fffffffLL;
}
