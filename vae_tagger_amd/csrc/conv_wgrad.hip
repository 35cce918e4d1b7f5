// Weight gradient of the VAE's stride-1 convs (3x3 pad 1, and the 1x1 conv_shortcut) on bf16 MFMA operands:
//   dw[co][ci][ky][kx] = sum over pixels p = (b, y, x) of dy16[p][co] * a16[b][y + ky - 1][x + kx - 1][ci]        (taps outside the image: 0)
// The reduction (K) dimension is the PIXEL index, which in NHWC is the strided one of both operands.  A workgroup (4 waves) owns a 64-cout x 64-cin x
// all-taps block of dw and one contiguous slice of the pixel tiles.  Per tile it stages, row-major as they lie in HBM,
//   the [WG_TH x WG_TW pixels][64 cout] piece of dy16 and the [(WG_TH + 2) x (WG_TW + 2) pixels][64 cin] piece of a16 (halo included, zero filled
//   outside the image and past ragged ends),
// and feeds v_mfma_f32_16x16x32_bf16 from ds_read_b64_tr_b16 reads of both images, so that K is the pixel index with no shuffle.  The one staged
// activation piece serves all nine taps: a tap is a row offset ((ky * AW + kx) staged pixels) of the same image.
//
// LDS image: one staged pixel is 64 channels = 128 B, padded to WG_ROWB = 160 B (40 dwords).  A transposed read takes, per 32-lane half, two 4-row x
// 16-column blocks; the K order is chosen (pixel of a K-step = 16 h + 4 g + q for read h, lane group g, element q) so that a half's two blocks are 8
// CONSECUTIVE staged pixels in the same 16 columns.  Pixel r starts at dword 40 r + c: 40 r mod 64 runs through 0, 40, 16, 56, 32, 8, 48, 24 for 8
// consecutive r whatever the first one -- eight disjoint 8-dword windows = all 64 banks once: conflict-free for dy and for every tap shift of a16.
// All lane addresses are multiples of 8 B (160 r + 2 (c0 + 4 p)), the dynamic-LDS base is 16-B aligned (no static LDS in this unit), and every
// transposed read runs with all 64 lanes active (ragged tiles are zero-filled, never skipped).
//
// Split over pixels: grid = splits x (Cout / 64) x (Cin / 64); slice s covers tiles [s * steps / splits, (s + 1) * steps / splits) in tile order and
// writes its fp32 partial block to ws[s]; wgrad_reduce_kernel then adds the slices in slice order.  No atomics: bit-identical from run to run.
#include <atomic>

#include "vt_common.h"
#include "vt_kernels.h"

namespace {

constexpr int WG_TW = 32;          // pixels of one K-step: one row segment of the tile
constexpr int WG_TH = 6;           // K-steps (rows) per staged tile
constexpr int WG_BC = 64;          // channel tile, both operands
constexpr int WG_ROWB = 160;       // bytes per staged pixel
constexpr int WG_THREADS = 256;
constexpr int WG_CUS = 256;        // MI355X
constexpr int WG_PER_CU = 2;       // workgroups resident per CU (74 KB of LDS, < 256 VGPRs each): the split rule fills both slots, so that one
                                   // workgroup's staging (no double buffer) hides under the other's MFMAs

template <int KS> struct WgGeom {
    static constexpr int HALO = KS / 2;
    static constexpr int AW = WG_TW + 2 * HALO, AH = WG_TH + 2 * HALO;
    static constexpr int DY_BYTES = WG_TH * WG_TW * WG_ROWB;
    static constexpr int A_BYTES = AH * AW * WG_ROWB;
    static constexpr int LDS = DY_BYTES + A_BYTES;      // 3x3: 30720 + 43520 = 74240 B (two workgroups per CU); 1x1: 61440 B
};

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

// one K-step's operand of a lane: the two transposed reads (pixels 16 h + 4 g + q, h = 0, 1) joined into the MFMA's 8 k-values
__device__ __forceinline__ bf16x8 tr_operand(const char* p) {
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)p);
    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(p + 16 * WG_ROWB));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// (amdgpu_waves_per_eu(2): at most 256 registers, so that two workgroups share a CU; left alone the compiler takes 272)
template <int KS>
__global__ __launch_bounds__(WG_THREADS) __attribute__((amdgpu_waves_per_eu(2))) void conv_wgrad_kernel(ConvWgradArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using G = WgGeom<KS>;
    constexpr int TAPS = KS * KS;
    char* sdy = smem;
    char* sa = smem + G::DY_BYTES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nci = g.Cin / WG_BC, nblk = nci * (g.Cout / WG_BC);
    const int blk = blockIdx.x % nblk, slice = blockIdx.x / nblk;
    const int co0 = (blk / nci) * WG_BC, ci0 = (blk % nci) * WG_BC;
    const int wm = wave >> 1, wn = wave & 1;           // the wave's 32-cout x 32-cin quarter of the block
    const int t0 = (int)((long long)slice * g.steps / g.splits), t1 = (int)((long long)(slice + 1) * g.steps / g.splits);

    f32x4 acc[TAPS][2][2];
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n) acc[t][m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    // transposed-read address of this lane: lane 4 q + p of group grp supplies pixel (4 grp + q), columns 4 p .. 4 p + 3 of the 16-column block
    const int grp = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const int dy_off = (4 * grp + q) * WG_ROWB + (wm * 32 + 4 * p) * 2;
    const int a_off = (4 * grp + q) * WG_ROWB + (wn * 32 + 4 * p) * 2;
    const int per_img = g.tiles_x * g.tiles_y;

    for (int t = t0; t < t1; ++t) {
        const int b = t / per_img, r = t - b * per_img;
        const int y0 = (r / g.tiles_x) * WG_TH, x0 = (r % g.tiles_x) * WG_TW;
        __syncthreads();                               // the previous tile's reads are over
        for (int idx = tid; idx < WG_TH * WG_TW * 8; idx += WG_THREADS) {
            const int px = idx >> 3, ch = idx & 7;
            const int y = y0 + px / WG_TW, x = x0 + px % WG_TW;
            uint4 v = uint4{0u, 0u, 0u, 0u};
            if (y < g.H && x < g.W) v = *(const uint4*)(g.dy + (((long long)b * g.H + y) * g.W + x) * g.Cout + co0 + ch * 8);
            *(uint4*)(sdy + px * WG_ROWB + ch * 16) = v;
        }
        for (int idx = tid; idx < G::AH * G::AW * 8; idx += WG_THREADS) {
            const int px = idx >> 3, ch = idx & 7;
            const int y = y0 + px / G::AW - G::HALO, x = x0 + px % G::AW - G::HALO;
            uint4 v = uint4{0u, 0u, 0u, 0u};
            if (y >= 0 && y < g.H && x >= 0 && x < g.W) v = *(const uint4*)(g.a + (((long long)b * g.H + y) * g.W + x) * g.Cin + ci0 + ch * 8);
            *(uint4*)(sa + px * WG_ROWB + ch * 16) = v;
        }
        __syncthreads();
        // A K-step is the 32 pixels of one tile row.  Walk the STAGED ACTIVATION rows instead of the dy rows: the fragments of activation row ar
        // (one per column shift kx and cin tile) meet dy row ar - ky for each ky, so they are read once for three taps, and the dy fragments of
        // the last three rows stay in registers -- 16 transposed reads per 36 MFMAs instead of 40.  Fully unrolled: every index is static.
        bf16x8 af[3][2];
#pragma unroll
        for (int ar = 0; ar < G::AH; ++ar) {
            if (ar < WG_TH) {
#pragma unroll
                for (int m = 0; m < 2; ++m) af[ar % 3][m] = tr_operand(sdy + dy_off + m * 32 + ar * WG_TW * WG_ROWB);
            }
            bf16x8 bfr[KS][2];
#pragma unroll
            for (int kx = 0; kx < KS; ++kx)
#pragma unroll
                for (int n = 0; n < 2; ++n) bfr[kx][n] = tr_operand(sa + a_off + n * 32 + (ar * G::AW + kx) * WG_ROWB);
#pragma unroll
            for (int ky = 0; ky < KS; ++ky) {
                const int ty = ar - ky;                 // the dy row this activation row serves at tap row ky
                if (ty < 0 || ty >= WG_TH) continue;
#pragma unroll
                for (int kx = 0; kx < KS; ++kx)
#pragma unroll
                    for (int n = 0; n < 2; ++n)
#pragma unroll
                        for (int m = 0; m < 2; ++m)
                            acc[ky * KS + kx][m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ty % 3][m], bfr[kx][n], acc[ky * KS + kx][m][n], 0, 0, 0);
            }
        }
    }
    // D layout of 16x16x32: column (cin) = lane & 15, row (cout) = 4 (lane >> 4) + register
    float* out = g.ws + (long long)slice * g.Cout * g.Cin * TAPS;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int ci = ci0 + wn * 32 + n * 16 + (lane & 15);
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int co = co0 + wm * 32 + m * 16 + 4 * grp + rr;
                float* o = out + ((long long)co * g.Cin + ci) * TAPS;
#pragma unroll
                for (int tap = 0; tap < TAPS; ++tap) o[tap] = acc[tap][m][n][rr];
            }
        }
}

// ---- the two resampling layers: the same MFMA loop, transposed reads, split and reduce; only the activation piece differs ----
//   MODE 1, Downsample2D (3x3 stride 2, pad (0,1)): dw[co][ci][ky][kx] = sum dy[b][i][j][co] * a[b][2i + ky][2j + kx][ci], a outside the image = 0.
//     A K-step is a dy row segment of 32 pixels, so the 32 activation pixels of a tap are 2 columns apart.  The piece (rows 2 y0 .. 2 y0 + 2 TH,
//     columns 2 x0 .. 2 x0 + 64) is therefore staged DE-INTERLEAVED by column parity: a staged row holds the 33 even columns, then the 32 odd ones
//     (65 staged pixels), and tap kx reads 32 CONSECUTIVE staged pixels from offset 0 (kx 0), 33 (kx 1) or 1 (kx 2).  The bank argument at the top of
//     this file needs exactly that -- 8 consecutive staged pixels per half, from any first pixel -- so every read stays conflict-free.  TH = 2:
//     10 240 B of dy + 5 x 65 x 160 = 52 000 B of activations = 62 240 B, two workgroups per CU (TH = 3 is 88 160 B: one).
//   MODE 2, Upsample2D (nearest 2x, then 3x3 pad 1): dw = sum_P dy[P][co] * x[(P + (ky - 1, kx - 1)) >> 1][ci], bounds tested on the high-resolution
//     coordinates before the shift.  The piece is staged from the low-resolution x16; everything after the staging is the 3x3 kernel (TH = 6).
template <int MODE> struct RsGeom {
    static constexpr int TH = MODE == 1 ? 2 : WG_TH;
    static constexpr int AH = MODE == 1 ? 2 * TH + 1 : TH + 2;
    static constexpr int AW = MODE == 1 ? 2 * WG_TW + 1 : WG_TW + 2;       // staged pixels per activation row
    static constexpr int ODD0 = WG_TW + 1;                                  // MODE 1: first staged pixel of the odd columns
    static constexpr int DY_BYTES = TH * WG_TW * WG_ROWB;
    static constexpr int A_BYTES = AH * AW * WG_ROWB;
    static constexpr int LDS = DY_BYTES + A_BYTES;                          // stride 2: 62 240 B; upsample: 74 240 B
    static constexpr int kx_off(int kx) { return MODE == 1 ? (kx == 0 ? 0 : kx == 1 ? ODD0 : 1) : kx; }
};

template <int MODE>
__global__ __launch_bounds__(WG_THREADS) __attribute__((amdgpu_waves_per_eu(2))) void conv_wgrad_rs_kernel(ConvWgradArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using G = RsGeom<MODE>;
    constexpr int TAPS = 9;
    char* sdy = smem;
    char* sa = smem + G::DY_BYTES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nci = g.Cin / WG_BC, nblk = nci * (g.Cout / WG_BC);
    const int blk = blockIdx.x % nblk, slice = blockIdx.x / nblk;
    const int co0 = (blk / nci) * WG_BC, ci0 = (blk % nci) * WG_BC;
    const int wm = wave >> 1, wn = wave & 1;
    const int t0 = (int)((long long)slice * g.steps / g.splits), t1 = (int)((long long)(slice + 1) * g.steps / g.splits);

    f32x4 acc[TAPS][2][2];
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n) acc[t][m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int grp = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const int dy_off = (4 * grp + q) * WG_ROWB + (wm * 32 + 4 * p) * 2;
    const int a_off = (4 * grp + q) * WG_ROWB + (wn * 32 + 4 * p) * 2;
    const int per_img = g.tiles_x * g.tiles_y;

    for (int t = t0; t < t1; ++t) {
        const int b = t / per_img, r = t - b * per_img;
        const int y0 = (r / g.tiles_x) * G::TH, x0 = (r % g.tiles_x) * WG_TW;       // in dy's coordinates (g.H x g.W)
        __syncthreads();
        for (int idx = tid; idx < G::TH * WG_TW * 8; idx += WG_THREADS) {
            const int px = idx >> 3, ch = idx & 7;
            const int y = y0 + px / WG_TW, x = x0 + px % WG_TW;
            uint4 v = uint4{0u, 0u, 0u, 0u};
            if (y < g.H && x < g.W) v = *(const uint4*)(g.dy + (((long long)b * g.H + y) * g.W + x) * g.Cout + co0 + ch * 8);
            *(uint4*)(sdy + px * WG_ROWB + ch * 16) = v;
        }
        for (int idx = tid; idx < G::AH * G::AW * 8; idx += WG_THREADS) {
            const int px = idx >> 3, ch = idx & 7;
            const int ry = px / G::AW, rx = px - ry * G::AW;
            int y, x;                                   // the activation pixel in a's coordinates (g.aH x g.aW)
            bool ok;
            if constexpr (MODE == 1) {
                y = 2 * y0 + ry;
                x = 2 * x0 + (rx < G::ODD0 ? 2 * rx : 2 * (rx - G::ODD0) + 1);
                ok = y < g.aH && x < g.aW;
            } else {
                const int Y = y0 + ry - 1, X = x0 + rx - 1;        // high resolution: tested before the shift
                ok = Y >= 0 && Y < g.H && X >= 0 && X < g.W;
                y = Y >> 1; x = X >> 1;
            }
            uint4 v = uint4{0u, 0u, 0u, 0u};
            if (ok) v = *(const uint4*)(g.a + (((long long)b * g.aH + y) * g.aW + x) * g.Cin + ci0 + ch * 8);
            *(uint4*)(sa + px * WG_ROWB + ch * 16) = v;
        }
        __syncthreads();
        // walk the staged activation rows as the 3x3 kernel does; row ar meets dy row ar - ky (upsample) or (ar - ky) / 2 where that is whole (stride 2)
        bf16x8 af[3][2];
#pragma unroll
        for (int ar = 0; ar < G::AH; ++ar) {
            const int nr = MODE == 1 ? ar / 2 : ar;     // the dy row first needed at this activation row
            if ((MODE != 1 || (ar & 1) == 0) && nr < G::TH) {
#pragma unroll
                for (int m = 0; m < 2; ++m) af[nr % 3][m] = tr_operand(sdy + dy_off + m * 32 + nr * WG_TW * WG_ROWB);
            }
            bf16x8 bfr[3][2];
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                for (int n = 0; n < 2; ++n) bfr[kx][n] = tr_operand(sa + a_off + n * 32 + (ar * G::AW + G::kx_off(kx)) * WG_ROWB);
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int d = ar - ky;
                if (d < 0 || (MODE == 1 && (d & 1))) continue;
                const int ty = MODE == 1 ? d / 2 : d;
                if (ty >= G::TH) continue;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                    for (int n = 0; n < 2; ++n)
#pragma unroll
                        for (int m = 0; m < 2; ++m)
                            acc[ky * 3 + kx][m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ty % 3][m], bfr[kx][n], acc[ky * 3 + kx][m][n], 0, 0, 0);
            }
        }
    }
    float* out = g.ws + (long long)slice * g.Cout * g.Cin * TAPS;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int ci = ci0 + wn * 32 + n * 16 + (lane & 15);
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int co = co0 + wm * 32 + m * 16 + 4 * grp + rr;
                float* o = out + ((long long)co * g.Cin + ci) * TAPS;
#pragma unroll
                for (int tap = 0; tap < TAPS; ++tap) o[tap] = acc[tap][m][n][rr];
            }
        }
}

// dw[i] = ws[0][i] + ws[1][i] + ... in slice order, four elements per thread
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const f32x4* __restrict__ ws, f32x4* __restrict__ dw, long long n4, int splits) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    f32x4 s = ws[i];
    for (int k = 1; k < splits; ++k) s += ws[(long long)k * n4 + i];
    dw[i] = s;
}

template <int KS>
hipError_t launch_wgrad(const ConvWgradArgs& a, hipStream_t s) {
    static std::atomic<unsigned long long> done{0};
    hipError_t e = vt_dynamic_smem_once(done, WgGeom<KS>::LDS, conv_wgrad_kernel<KS>);
    if (e != hipSuccess) return e;
    const long long wgs = (long long)a.splits * (a.Cin / WG_BC) * (a.Cout / WG_BC);
    if (wgs > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(conv_wgrad_kernel<KS>, dim3((unsigned)wgs), dim3(WG_THREADS), WgGeom<KS>::LDS, s, a);
    return hipGetLastError();
}

template <int MODE>
hipError_t launch_wgrad_rs(const ConvWgradArgs& a, hipStream_t s) {
    static std::atomic<unsigned long long> done{0};
    hipError_t e = vt_dynamic_smem_once(done, RsGeom<MODE>::LDS, conv_wgrad_rs_kernel<MODE>);
    if (e != hipSuccess) return e;
    const long long wgs = (long long)a.splits * (a.Cin / WG_BC) * (a.Cout / WG_BC);
    if (wgs > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(conv_wgrad_rs_kernel<MODE>, dim3((unsigned)wgs), dim3(WG_THREADS), RsGeom<MODE>::LDS, s, a);
    return hipGetLastError();
}

int rs_th(int mode) { return mode == 1 ? RsGeom<1>::TH : RsGeom<2>::TH; }

}  // namespace

int vt_conv_wgrad_rs_steps(int mode, int B, int Hdy, int Wdy) {
    if ((mode != 1 && mode != 2) || B <= 0 || Hdy <= 0 || Wdy <= 0) return 0;
    const int th = rs_th(mode);
    const long long n = (long long)B * ((Hdy + th - 1) / th) * ((Wdy + WG_TW - 1) / WG_TW);
    return n > 0x7fffffffLL ? 0 : (int)n;
}

int vt_conv_wgrad_rs_auto_splits(int mode, int B, int Hdy, int Wdy, int Cin, int Cout) {
    const int steps = vt_conv_wgrad_rs_steps(mode, B, Hdy, Wdy);
    const int nblk = (Cin / WG_BC) * (Cout / WG_BC);
    if (steps <= 0 || nblk <= 0) return 0;
    int sp = WG_PER_CU * WG_CUS / nblk;
    if (sp < 1) sp = 1;
    return sp > steps ? steps : sp;
}

// a.H, a.W: dy's size; a.aH, a.aW: the activation's (mode 1: Downsample2D's input, aH / 2 == H; mode 2: Upsample2D's input, 2 aH == H)
hipError_t vt_launch_conv_wgrad_rs(const ConvWgradArgs& a_in, int mode, hipStream_t s) {
    ConvWgradArgs a = a_in;
    if (!a.dy || !a.a || !a.dw || !a.ws || !vt_conv_wgrad_supported(a.Cin, a.Cout, 3)) return hipErrorInvalidValue;
    if (mode == 1 ? (a.aH / 2 != a.H || a.aW / 2 != a.W) : (mode != 2 || 2 * a.aH != a.H || 2 * a.aW != a.W)) return hipErrorInvalidValue;
    a.ksize = 3;
    a.steps = vt_conv_wgrad_rs_steps(mode, a.batch, a.H, a.W);
    if (a.steps <= 0 || a.splits < 1 || a.splits > a.steps) return hipErrorInvalidValue;
    const int th = rs_th(mode);
    a.tiles_x = (a.W + WG_TW - 1) / WG_TW;
    a.tiles_y = (a.H + th - 1) / th;
    hipError_t e = mode == 1 ? launch_wgrad_rs<1>(a, s) : launch_wgrad_rs<2>(a, s);
    if (e != hipSuccess) return e;
    const long long n4 = (long long)a.Cout * a.Cin * 9 / 4;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, (const f32x4*)a.ws, (f32x4*)a.dw, n4, a.splits);
    return hipGetLastError();
}

int vt_conv_wgrad_steps(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    const long long n = (long long)B * ((H + WG_TH - 1) / WG_TH) * ((W + WG_TW - 1) / WG_TW);
    return n > 0x7fffffffLL ? 0 : (int)n;
}

bool vt_conv_wgrad_supported(int Cin, int Cout, int ksize) {
    return Cin >= WG_BC && Cout >= WG_BC && (Cin % WG_BC) == 0 && (Cout % WG_BC) == 0 && (ksize == 1 || ksize == 3);
}

int vt_conv_wgrad_auto_splits(int B, int H, int W, int Cin, int Cout) {
    const int steps = vt_conv_wgrad_steps(B, H, W);
    const int nblk = (Cin / WG_BC) * (Cout / WG_BC);
    if (steps <= 0 || nblk <= 0) return 0;
    int sp = WG_PER_CU * WG_CUS / nblk;
    if (sp < 1) sp = 1;
    return sp > steps ? steps : sp;
}

hipError_t vt_launch_conv_wgrad(const ConvWgradArgs& a_in, hipStream_t s) {
    ConvWgradArgs a = a_in;
    if (!a.dy || !a.a || !a.dw || !a.ws || !vt_conv_wgrad_supported(a.Cin, a.Cout, a.ksize)) return hipErrorInvalidValue;
    a.steps = vt_conv_wgrad_steps(a.batch, a.H, a.W);
    if (a.steps <= 0 || a.splits < 1 || a.splits > a.steps) return hipErrorInvalidValue;
    a.tiles_x = (a.W + WG_TW - 1) / WG_TW;
    a.tiles_y = (a.H + WG_TH - 1) / WG_TH;
    hipError_t e = a.ksize == 3 ? launch_wgrad<3>(a, s) : launch_wgrad<1>(a, s);
    if (e != hipSuccess) return e;
    const long long n4 = (long long)a.Cout * a.Cin * a.ksize * a.ksize / 4;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, (const f32x4*)a.ws, (f32x4*)a.dw, n4, a.splits);
    return hipGetLastError();
}
