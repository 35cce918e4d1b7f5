// 3x3 / stride 1 / pad 1 convolution on fp8 (OCP e4m3) operands -- BASELINE.json configs[4], opt-in (vt_set_flag(ctx, 11, 1)).
//
// Same halo-tile implicit GEMM as conv3x3_halo.hip (X halo staged once per channel chunk and read at shifted rows by all nine
// taps, weights through an LDS ring filled by LDS-DMA under counted vmcnt waits, one raw s_barrier per K-step, fragments of
// step t+1 read during step t, halo rows reused across ky from registers), re-shaped for
// v_mfma_scale_f32_32x32x64_f8f6f4 (both scales 2^0): twice the bf16 FLOPs per matrix-pipe cycle.
//   * an LDS row is still 64 B, now 64 fp8 channels: a K-step = (64-channel chunk, tap) carries twice the K of the bf16
//     kernel at the same LDS / DMA bytes, so every data rate per unit time stays where the bf16 kernel has it;
//   * workgroup = 4 waves (2 pixel-row groups x 2 cout groups) x <= 256 VGPRs, 80 KB LDS: two workgroups per CU;
//     tile = 8 rows x 32 pixels x 128 couts, wave tile = 4 rows x 32 pixels x 64 couts = 4 x 2 MFMAs of 32x32x64;
//   * operand fragment = 32 B per lane: lane (g = lane >> 5, i = lane & 31) holds channels 32 g .. 32 g + 31 of row i (weights:
//     cout row, activations: pixel), read as two ds_read_b128; rows 64 B apart are conflict-free with the 16-B chunk
//     swizzle  physical = logical ^ ((row ^ (row >> 2)) & 3), applied to the DMA's per-lane source address and to the reads;
//   * cout rows are packed so that accumulator register r of lane (g, x) is cout base + 16 g + r: 16 consecutive couts of one
//     pixel per lane (32-B fp16 / 64-B fp32 runs per store pair, GroupNorm groups stay inside a lane).
// Operands: X = e4m3(act_scale * silu(GroupNorm(.))) written by the GroupNorm-apply pass (groupnorm.hip, fp8 output);
// W = e4m3(w / wscale[cout]) packed by the host; the epilogue computes acc * (wscale[cout] / act_scale) + bias.
#include <type_traits>

#include "vt_halo.h"
#include "vt_kernels.h"

#ifdef HALO_STAMP
// Diagnostic build only (tools/stamp_halo_fp8.py): wall-clock stamps (s_memrealtime, 100 MHz) of the phases of one workgroup and
// one s_memtime (shader clock) pair around the main loop; written only for launches that match the filter, into a buffer nothing
// else reads.  In the product build no stamp executes.
__device__ unsigned long long* g_halo8_stamps = nullptr;
__device__ int g_halo8_filter[3] = {0, 0, 0};         // H, Cin, 1 + (fp16 residual present); 0 = any
extern "C" int vt_debug_halo_fp8_stamps(unsigned long long* buf, int H, int Cin, int res) {
    const int f[3] = {H, Cin, res};
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(g_halo8_filter), f, sizeof(f));
    if (e != hipSuccess) return (int)e;
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_halo8_stamps), &buf, sizeof(buf));
}
#define STAMP_ON (g_halo8_stamps && threadIdx.x == 0 && (!g_halo8_filter[0] || g_halo8_filter[0] == a.H) && \
                  (!g_halo8_filter[1] || g_halo8_filter[1] == a.Cin) && (!g_halo8_filter[2] || g_halo8_filter[2] == 1 + (a.res_f16 != nullptr)))
#define STAMP(slot)                                                                                            \
    do {                                                                                                       \
        unsigned long long t_;                                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                                     \
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                         \
        __builtin_amdgcn_sched_barrier(0);                                                                     \
        if (STAMP_ON) g_halo8_stamps[(long long)blockIdx.x * 16 + (slot)] = t_;                                \
    } while (0)
#define STAMP_CLK(slot)                                                                                        \
    do {                                                                                                       \
        unsigned long long t_;                                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                                     \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                             \
        __builtin_amdgcn_sched_barrier(0);                                                                     \
        if (STAMP_ON) g_halo8_stamps[(long long)blockIdx.x * 16 + (slot)] = t_;                                \
    } while (0)
#else
#define STAMP(slot) do {} while (0)
#define STAMP_CLK(slot) do {} while (0)
#endif

namespace {

constexpr int HB = 64;                       // bytes per LDS row
constexpr int WC = 2, TP = 4;                // cout wave groups (x 64 couts); tile rows per wave
constexpr int BC = WC * 64;                  // 128 couts per workgroup
constexpr int WPCS = BC / 16;                // W pieces per K-step: 8
constexpr int WBUF = BC * HB;                // 8 KB per stage
constexpr int NW = 4;                        // weight ring depth
constexpr int LEAD = NW - 1;                 // W(t + LEAD) is issued during step t (two barriers after the stage's last read)
constexpr int WOUT = LEAD - 2;               // W tiles issued after the one a barrier needs (fragments of t+1 are read during t)

// Tile shape = (WP x TP) rows x (WX x 32) pixels x 128 couts on WP x WX x 2 waves; a wave's tile is always 4 rows x 32 px x 64 couts.
//   <2, 1>: 8 x 32 px, 4 waves, 80 KB LDS, two workgroups per CU (the default);
//   <4, 1>: 16 x 32 px, 8 waves, one workgroup per CU: one staged weight tile serves twice the pixels, halo over-read 1.19x instead of 1.33x;
//   <2, 2>: 8 x 64 px, 8 waves, one workgroup per CU (over-read 1.29x).  vt_set_flag(ctx, 16, shape); round-4 A/B: profiles/r04/halo_fp8_tile_shapes_ab.log
template <int WP_, int WX_>
struct Shape {
    static constexpr int WP = WP_, WX = WX_;
    static constexpr int TWX = 32 * WX;                  // tile width in pixels (the MFMA's N = 32 per wave)
    static constexpr int HWID = TWX + 2;                 // halo width
    static constexpr int ROWS = WP * TP;                 // tile rows
    static constexpr int NWV = WP * WX * WC, NT = 64 * NWV;
    static constexpr int HROWS = (ROWS + 2) * HWID;      // halo pixels
    static constexpr int NXW = ((HROWS + 15) / 16 + NWV - 1) / NWV;      // X pieces (16 rows each) per wave
    static constexpr int XBUF = NXW * NWV * 16 * HB;     // bytes per halo buffer
    static constexpr int WPW = WPCS / NWV;               // W pieces per wave and K-step
    static constexpr int SMEM_LOOP = 2 * XBUF + NW * WBUF;
    static constexpr int SMEM_RES = NWV * 16384 + WBUF;  // epilogue: a 16-KB fp16 residual tile per wave + the GroupNorm scratch behind them
    static constexpr int SMEM = SMEM_LOOP > SMEM_RES ? SMEM_LOOP : SMEM_RES;
    static constexpr int WG_PER_CU = SMEM <= 80 * 1024 ? 2 : 1;
    static_assert(WPCS % NWV == 0 && SMEM <= 160 * 1024, "tile shape");
};

template <int WP, int WX>
__global__ __launch_bounds__(64 * WP * WX * WC, 2) void conv3x3_halo_fp8_kernel(const Conv3x3Fp8Args a) {
    typedef Shape<WP, WX> SH;
    constexpr int TWX = SH::TWX, HWID = SH::HWID, ROWS = SH::ROWS, NWV = SH::NWV, HROWS = SH::HROWS, NXW = SH::NXW, XBUF = SH::XBUF,
                  WPW = SH::WPW, SMEM = SH::SMEM;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const xbase = smem;                    // 2 halo buffers
    char* const wbase = smem + 2 * XBUF;         // NW weight stages
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wc = wave % WC, wx = (wave / WC) % WX, wp = wave / (WC * WX);
    const int g = lane >> 5, li = lane & 31;
    STAMP(0);

    // ---- tile coordinates
    const VtHaloTile tl = vt_halo_tile_of(a);
    const int b = tl.b, tile = tl.tile;
    const int ty0 = tl.tyi * ROWS, tx0 = tl.txi() * TWX;
    const int c0 = tl.ct * BC;
    const unsigned char* Xb = a.X + (long long)b * a.H * a.W * a.Cin;
    const int nchunk = a.Cin >> 6;
    const int nk = nchunk * 9;

    // ---- DMA bookkeeping: one wave-instruction = 16 LDS rows x 64 B; lane l -> row (l >> 2), physical chunk (l & 3),
    // logical chunk = physical ^ vt_swz8(row) (swz of a piece's row depends on the row inside the piece only: pieces start at multiples of 16)
    const int drow = lane >> 2;
    const int dchunk = (lane & 3) ^ vt_swz8(drow);
    const int hr0 = wave * 16 + drow;
    const int hy0 = hr0 / HWID, hx0 = hr0 - (hr0 / HWID) * HWID;
    const int wsrc0 = (c0 + wave * 16 + drow) * HB + dchunk * 16;       // byte offset inside a K-step's [Cout][64] tile
    const int wstep = a.Cout * HB;                                     // bytes between consecutive K-steps

    auto issue_x_dma = [&](int chunk) {
#ifdef EXP_NO_DMA                    // timing experiment only (wrong results): the first two halos and the first NW weight tiles serve every K-step
        if (chunk >= 2) return;
#endif
        char* dst = xbase + (chunk & 1) * XBUF;
        int hy = vt_opaque(hy0), hx = hx0, hr = hr0;
#pragma nounroll
        for (int j = 0; j < NXW; ++j) {
            const int iy = ty0 - 1 + hy, ix = tx0 - 1 + hx;
            const bool v = hr < HROWS && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            const void* src = v ? (const void*)(Xb + ((iy * a.W + ix) * a.Cin + chunk * 64 + dchunk * 16)) : a.zeros;
            __builtin_amdgcn_global_load_lds(VT_GLOBAL_PTR(src), VT_LDS_PTR(dst + (j * NWV + wave) * 1024), 16, 0, 0);
            hr += NWV * 16;
            hx += (NWV * 16) % HWID; hy += (NWV * 16) / HWID;
            if (hx >= HWID) { hx -= HWID; ++hy; }
        }
    };
    auto issue_w = [&](int t) {
#ifdef EXP_NO_DMA
        if (t >= NW) return;
#endif
        char* dst = wbase + (t % NW) * WBUF;
#ifdef W_WINDOW_EXPERIMENT       // timing experiment only (wrong results): every K-step's weights from a window of W_WINDOW_EXPERIMENT tiles
        const unsigned char* wt = a.Wp + (long long)(t % W_WINDOW_EXPERIMENT) * wstep + vt_opaque(wsrc0);
#else
        const unsigned char* wt = a.Wp + (long long)t * wstep + vt_opaque(wsrc0);
#endif
#pragma unroll
        for (int j = 0; j < WPW; ++j)
            __builtin_amdgcn_global_load_lds(VT_GLOBAL_PTR(wt + j * NWV * 16 * HB), VT_LDS_PTR(dst + (j * NWV + wave) * 1024), 16, 0, 0);
    };

    // ---- prologue: DMA first; the epilogue constants load under its latency
    issue_x_dma(0);
#pragma unroll
    for (int t = 0; t < LEAD; ++t)
        if (t < nk) issue_w(t);
    asm volatile("" ::: "memory");
    STAMP(1);

    f32x16 acc[2][TP];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < TP; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[h][j][r] = 0.f;

    // fragment rows: W stage row wc*64 + 32 h + li; X halo row (wp*TP + r) * HWID + dx + li
    const int wrow0 = wc * 64 + li;
    const int xrow0 = wp * TP * HWID + wx * 32 + li;
    i32x8 wfc[2], xr[TP + 2];
    {
        int ahead0 = nk - 1;
        if (ahead0 > LEAD - 1) ahead0 = LEAD - 1;
        vt_wait_vmcnt<16>(ahead0 * WPW);         // W(0) and X(0) landed (this wave's pieces) ...
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_barrier();            // ... and everybody else's
        asm volatile("" ::: "memory");
#pragma unroll
        for (int h = 0; h < 2; ++h) wfc[h] = vt_read_frag8(wbase, vt_opaque(wrow0) + 32 * h, g);
#pragma unroll
        for (int r = 0; r < TP + 2; ++r) xr[r] = vt_read_frag8(xbase, vt_opaque(xrow0) + r * HWID, g);
    }
    STAMP(2);
    STAMP_CLK(11);

    // One chunk = 9 K-steps (taps, kx-major: step p -> dx = p / 3, dy = p % 3).  VM-op issue order per wave and step:
    // [wait][barrier] ... W(t+LEAD) [+ the next chunk's halo at tap 0], both in the middle of the MFMA sequence.
    auto do_chunk = [&](int chunk, auto last_tag) {
        constexpr bool LAST = decltype(last_tag)::value;
        const char* xs = xbase + (chunk & 1) * XBUF;
        const int tbase = chunk * 9;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int t = tbase + tap;
            if constexpr (!LAST) {
                int n = WOUT * WPW;
                if (tap >= 1 && tap <= LEAD - 1) n += NXW;               // the next halo, DMA'd at tap 0
                vt_wait_vmcnt<16>(n);
            } else {
                // the last chunk ends the kernel's K-steps (nk = 9 * nchunk): t + 1 = nk - (8 - tap), all compile-time
                int ahead = 7 - tap;
                if (ahead > WOUT) ahead = WOUT;
                if (ahead < 0) ahead = 0;
                vt_wait_vmcnt<16>(ahead * WPW);
            }
            asm volatile("" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            const int dx = tap / 3, dy = tap % 3;
            const bool has_next = !LAST || tap < 8;
            const bool next_group = !LAST || dx < 2;
            const int dx_n = (dx + 1) % 3;
            const char* xs_n = (dx == 2) ? xbase + ((chunk + 1) & 1) * XBUF : xs;
            const char* ws_n = wbase + ((t + 1) % NW) * WBUF;
#ifndef EXP_NO_FRAG_READS            // timing experiment only (wrong results): the step-0 fragments serve every K-step
            auto refill = [&](int r) { xr[r] = vt_read_frag8(xs_n, vt_opaque(xrow0) + r * HWID + dx_n, g); };
#else
            auto refill = [&](int) {};
#endif
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int j = 0; j < TP; ++j) {
#pragma unroll
                for (int h = 0; h < 2; ++h)
                    acc[h][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wfc[h], xr[j + dy], acc[h][j], 0, 0, 0, 127, 0, 127);
                if (next_group) {                                        // rows whose last reader has just issued
                    if (dy == 0 && j == 0) refill(0);
                    if (dy == 1 && j == 0) refill(1);
                    if (dy == 2) refill(j + 2);
                }
                if (j == TP / 2 - 1) {
                    if (!LAST || tap + LEAD < 9) issue_w(t + LEAD);
                    if constexpr (!LAST) { if (tap == 0) issue_x_dma(chunk + 1); }
                }
            }
            __builtin_amdgcn_s_setprio(0);
#ifndef EXP_NO_FRAG_READS
            if (has_next) {
#pragma unroll
                for (int h = 0; h < 2; ++h) wfc[h] = vt_read_frag8(ws_n, vt_opaque(wrow0) + 32 * h, g);
            }
#endif
            __builtin_amdgcn_sched_barrier(0);           // a K-step's MFMAs stay inside it (sunk past later barriers they cost spills)
        }
    };
    for (int chunk = 0; chunk + 1 < nchunk; ++chunk) do_chunk(chunk, std::false_type{});
    do_chunk(nchunk - 1, std::true_type{});
    STAMP_CLK(12);
    STAMP(3);
    if (a.scX) {
        // ---- fused 1x1 shortcut (a resnet block's conv_shortcut): acc += scW . scX at the tile's own pixels, as scCin / 32 plain
        // K-steps of bf16 32x32x16 MFMAs on the SAME accumulators (the fp8 and bf16 32x32 forms share the accumulator layout).
        // scW is pre-divided by mult[cout] on the host, so the epilogue's acc * mult + bias scales it back.
        const bf16_t* Xs = a.scX + (long long)b * a.H * a.W * a.scCin;
        const int scn = a.scCin >> 5;
#pragma nounroll
        for (int c = 0; c < scn; ++c) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                        // the staging buffers are free
            asm volatile("" ::: "memory");
            static_assert(ROWS * TWX / 16 == 4 * NWV, "shortcut staging: 4 pieces per wave");
#pragma unroll
            for (int j = 0; j < 4; ++j) {                        // the tile's ROWS x TWX pixels, 16 per piece, 4 pieces per wave
                const int pp = (j * NWV + wave) * 16 + drow;
                const int iy = ty0 + pp / TWX, ix = tx0 + pp % TWX;
                const void* src = (iy < a.H && ix < a.W) ? (const void*)(Xs + ((long long)(iy * a.W + ix) * a.scCin + c * 32 + dchunk * 8)) : a.zeros;
                __builtin_amdgcn_global_load_lds(VT_GLOBAL_PTR(src), VT_LDS_PTR(xbase + (j * NWV + wave) * 1024), 16, 0, 0);
            }
            const bf16_t* wt = a.scW + ((long long)c * a.Cout + c0 + wave * 16 + drow) * 32 + dchunk * 8;
#pragma unroll
            for (int j = 0; j < WPW; ++j)
                __builtin_amdgcn_global_load_lds(VT_GLOBAL_PTR(wt + j * NWV * 16 * 32), VT_LDS_PTR(wbase + (j * NWV + wave) * 1024), 16, 0, 0);
            vt_wait_vmcnt<16>(0);
            asm volatile("" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {                     // k = 16 ks + 8 g .. + 7: logical 16-B chunk 2 ks + g
                bf16x8 wf[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int row = wrow0 + 32 * h;
                    wf[h] = *(const bf16x8*)(wbase + row * HB + (((2 * ks + g) ^ vt_swz8(row)) << 4));
                }
#pragma unroll
                for (int j = 0; j < TP; ++j) {
                    const int row = (wp * TP + j) * TWX + wx * 32 + li;
                    const bf16x8 xf = *(const bf16x8*)(xbase + row * HB + (((2 * ks + g) ^ vt_swz8(row)) << 4));
#pragma unroll
                    for (int h = 0; h < 2; ++h)
                        acc[h][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[h], xf, acc[h][j], 0, 0, 0);
                }
            }
        }
    }
    // pin the accumulators here: left alone, the compiler sinks each chain's last MFMAs into the epilogue's conditional
    // blocks (behind the first stores), keeps the operand fragments alive for them and spills ~100 registers
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < TP; ++j) asm volatile("" : "+v"(acc[h][j]));
    asm volatile("" ::: "memory");

    // ---- epilogue: register r of lane (g, x = li) in acc[h][j] is cout cw(h) + r of pixel (ty0 + wp*TP + j, tx0 + li)
    const int HWp = a.H * a.W;
    const long long ob = (long long)b * HWp * a.Cout;
    const int x = tx0 + wx * 32 + li;
    // fp16 residual: fetched with ONE LDS-DMA burst per wave (its own 4 rows x 32 px x 64 couts = 16 KB, into the staging
    // buffers the main loop no longer needs) instead of eight dependent global-load round trips inside the store loop.
    // Piece p of a wave = pixels 8 p .. 8 p + 7 of its region x 128 B; lane l -> pixel (l >> 3), physical 16-B chunk (l & 7),
    // logical chunk = physical ^ (pixel & 7) (rows 128 B apart: 2-way instead of 8-way bank conflicts on the reads).
    char* const rbuf = smem + wave * 16384;
    if (a.res_f16) {
        __syncthreads();                                 // every wave has read its last fragments: the buffers are free
#pragma unroll 4
        for (int pc = 0; pc < 16; ++pc) {
            const int pp = pc * 8 + (lane >> 3);
            const int yy = ty0 + wp * TP + (pp >> 5), xx = tx0 + wx * 32 + (pp & 31);
            const int lc = (lane & 7) ^ (pp & 7);
            const void* src = (yy < a.H && xx < a.W)
                ? (const void*)(a.res_f16 + ob + ((long long)yy * a.W + xx) * a.Cout + c0 + wc * 64 + lc * 8) : a.zeros;
            __builtin_amdgcn_global_load_lds(VT_GLOBAL_PTR(src), VT_LDS_PTR(rbuf + pc * 1024), 16, 0, 0);
        }
    }
    unsigned valid = 0;
    float amax8 = 0.f;                                  // largest |value| handed to the e4m3 conversion
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int cw = c0 + wc * 64 + 32 * h + 16 * g;
        f32x4 mul[4], bia[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            mul[i] = *(const f32x4*)(a.mult + cw + 4 * i);
            bia[i] = a.bias ? *(const f32x4*)(a.bias + cw + 4 * i) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if (h == 0 && a.res_f16) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's residual tile is in LDS
#ifdef HALO_STAMP
        if (h == 0) STAMP(9);
#endif
#pragma unroll
        for (int j = 0; j < TP; ++j) {
            const int y = ty0 + wp * TP + j;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[h][j][r] = fmaf(acc[h][j][r], mul[r >> 2][r & 3], bia[r >> 2][r & 3]);
            if (y >= a.H || x >= a.W) continue;
            valid |= 1u << j;
            const long long o = ob + ((long long)y * a.W + x) * a.Cout + cw;
            if (a.res) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f32x4 rv = *(const f32x4*)(a.res + o + 4 * i);
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[h][j][4 * i + q] += rv[q];
                }
            }
            if (a.res_f16) {
                const int pp = j * 32 + li;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const f16x8 rh = *(const f16x8*)(rbuf + pp * 128 + (((4 * h + 2 * g + i) ^ (pp & 7)) << 4));
#pragma unroll
                    for (int q = 0; q < 8; ++q) acc[h][j][8 * i + q] += (float)rh[q];
                }
            }
            if (a.out_f32) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    *(f32x4*)(a.out_f32 + o + 4 * i) = f32x4{acc[h][j][4 * i], acc[h][j][4 * i + 1], acc[h][j][4 * i + 2], acc[h][j][4 * i + 3]};
            }
            if (a.out_f16) vt_halo_store16_f8(a.out_f16 + o, acc[h][j]);
            if (a.out_e4m3) {
                i32x4 o8 = {0, 0, 0, 0};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float t[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) t[q] = acc[h][j][4 * i + q] * a.out_e4m3_scale;
                    amax8 = fmaxf(fmaxf(fabsf(t[0]), fabsf(t[1])), fmaxf(fmaxf(fabsf(t[2]), fabsf(t[3])), amax8));
#pragma unroll
                    for (int q = 0; q < 4; ++q) t[q] = __builtin_amdgcn_fmed3f(t[q], -448.f, 448.f);
                    o8[i] = __builtin_amdgcn_cvt_pk_fp8_f32(t[0], t[1], o8[i], false);
                    o8[i] = __builtin_amdgcn_cvt_pk_fp8_f32(t[2], t[3], o8[i], true);
                }
                // a.out8_planar: [Cout/64][H][W][64] (chunk-planar) for the fp8 stride-2 phase-plane kernel (see conv3x3_s2_halo.hip)
                const long long o8a = a.out8_planar ? (((long long)(b * (a.Cout >> 6) + (cw >> 6)) * a.H + y) * a.W + x) * 64 + (cw & 63) : o;
                *(i32x4*)(a.out_e4m3 + o8a) = o8;
            }
            if (a.out_bf16) vt_halo_store16_f8(a.out_bf16 + o, acc[h][j]);
        }
    }
    if (a.out_e4m3 && a.status && amax8 > 448.f) atomicOr(a.status, 2);      // e4m3 saturates silently: sticky bit 1 of vt_status
    STAMP(4);
    if (a.gn_partial) {
        // GroupNorm (n, mean, M2) of this tile's outputs for the next norm
        float* lds = (float*)(smem + SMEM - WBUF);         // the last weight stage: clear of the residual staging (waves x 16 KB from 0)
        if (!a.res_f16 && !a.scX) {                        // those paths have passed a barrier since the last K-step's fragment reads
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        }
        vt_gn_epilogue_partials_f8<TP, WP, WX>(acc, valid, a, b, tile, c0, wp, wx, wc, lane, lds);
    }
#ifdef HALO_STAMP
    STAMP(5);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    STAMP(6);
    if (STAMP_ON) {
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        g_halo8_stamps[(long long)blockIdx.x * 16 + 7] = ((unsigned long long)xcc << 32) | hw;
    }
#endif
}

}  // namespace

bool vt_conv3x3_halo_fp8_supported(int Cin, int Cout) { return Cin >= 64 && (Cin % 64) == 0 && (Cout % 128) == 0; }
int vt_conv3x3_halo_fp8_tiles_shape(int H, int W, int shape) {
    const int rows = shape == 1 ? Shape<4, 1>::ROWS : Shape<2, 1>::ROWS, twx = shape == 2 ? Shape<2, 2>::TWX : Shape<2, 1>::TWX;
    return ((W + twx - 1) / twx) * ((H + rows - 1) / rows);
}
int vt_conv3x3_halo_fp8_tiles(int H, int W) { return vt_conv3x3_halo_fp8_tiles_shape(H, W, 0); }      // (the default shape has the most tiles)

// LDS row (inside a 32-cout MFMA block) that must hold cout_local, so that accumulator register r of lane group g is cout 16 g + r
int vt_halo_fp8_row_of_cout(int cout_local /*0..31*/) {
    const int gg = cout_local >> 4, q = (cout_local >> 2) & 3, t = cout_local & 3;
    return 8 * q + 4 * gg + t;
}

namespace {
template <int WP, int WX>
hipError_t launch_shape(const Conv3x3Fp8Args& a, hipStream_t s) {
    typedef Shape<WP, WX> SH;
    static std::atomic<unsigned long long> attr_done{0};
    hipError_t ea = vt_dynamic_smem_once(attr_done, SH::SMEM, conv3x3_halo_fp8_kernel<WP, WX>);
    if (ea != hipSuccess) return ea;
    Conv3x3Fp8Args k = a;
    const long long nblk = vt_halo_tile_grid(k, (a.W + SH::TWX - 1) / SH::TWX, (a.H + SH::ROWS - 1) / SH::ROWS, a.Cout / BC, a.batch);
    if (!nblk) return hipErrorInvalidValue;
    hipLaunchKernelGGL((conv3x3_halo_fp8_kernel<WP, WX>), dim3((unsigned)nblk), dim3(SH::NT), SH::SMEM, s, k);
    return hipGetLastError();
}
}  // namespace

hipError_t vt_launch_conv3x3_halo_fp8(const Conv3x3Fp8Args& a, hipStream_t s) {
    if (!a.X || !a.Wp || !a.mult || !a.zeros || (!a.out_f32 && !a.out_bf16 && !a.out_f16 && !a.out_e4m3)) return hipErrorInvalidValue;
    if ((a.res && a.res_f16) || (a.res_f16 && a.out_f32)) return hipErrorInvalidValue;
    if (!vt_conv3x3_halo_fp8_supported(a.Cin, a.Cout) || a.batch <= 0 || a.H <= 0 || a.W <= 0) return hipErrorInvalidValue;
    if (!vt_gn_cpg_ok(a.gn_partial, a.gn_cpg)) return hipErrorInvalidValue;
    if (!vt_fits_i32((long long)a.H * a.W * a.Cin) || !vt_fits_i32((long long)(a.Cin / 64) * 9 * a.Cout * 64)) return hipErrorInvalidValue;
    if ((a.scX != nullptr) != (a.scW != nullptr)) return hipErrorInvalidValue;
    if (a.scX && (a.scCin <= 0 || (a.scCin % 32) || a.res || a.res_f16 || !vt_fits_i32((long long)a.H * a.W * a.scCin))) return hipErrorInvalidValue;
    if (a.shape == 1) return launch_shape<4, 1>(a, s);
    if (a.shape == 2) return launch_shape<2, 2>(a, s);
    if (a.shape != 0) return hipErrorInvalidValue;
    return launch_shape<2, 1>(a, s);
}
