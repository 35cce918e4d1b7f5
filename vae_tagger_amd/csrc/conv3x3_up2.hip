// Upsample2D of the VAE decoder -- nearest-neighbour 2x followed by a 3x3 / stride 1 / pad 1 convolution -- as ONE kernel on the
// low-resolution input.  Output pixel (2i+a, 2j+b) of phase (a, b) is a 2x2 convolution of the low-resolution image with weights that are
// sums of the original taps:
//
//   phase a = 0:  folded row tap 0 reads low-res row i-1 with {ky 0};      tap 1 reads row i   with {ky 1, ky 2}
//   phase a = 1:  folded row tap 0 reads low-res row i   with {ky 0, ky 1}; tap 1 reads row i+1 with {ky 2}
//
// and the same table for columns (b, kx).  Zero padding of the upsampled tensor coincides with zero padding of the low-resolution one, so
// the identity is exact at the borders.  16 folded [Cout][Cin] matrices (4 phases x 2x2 taps) replace the 9 original ones, each output
// pixel costs 4 taps instead of 9, and the 4x-sized upsampled tensor is never written.
//
// Skeleton of conv3x3_halo.hip: NHWC 16-bit input, the (ROWS+2) x 18 low-resolution halo of a ROWS x 16 pixel tile staged in LDS once per
// 32-channel chunk by LDS-DMA, v_mfma_f32_16x16x32_bf16 (or _f16: the fp16-operand mode) with fp32 accumulation, weights = A operand with
// the interleaved cout rows (a lane owns 16 consecutive couts of its pixel).  A K-step is (chunk, phase, folded tap); the 16 K-steps of a
// chunk read only 9 distinct (row, column) shifts of the one staged halo, and a wave holds those fragments -- 4 halo rows x 3 column shifts
// for its 2 low-resolution rows -- in registers for the whole chunk.
//
// Tile: 4 waves, 8 x 16 low-resolution pixels (16 x 32 outputs) x 64 couts per workgroup; a wave owns 2 low-resolution rows x 16 px x 64
// couts x 4 phases = 32 accumulator tiles (128 VGPRs).  Per chunk the workgroup stages the halo (12 KB) and the chunk's 16 weight tiles
// (64 KB) in one burst, single-buffered: 76 KB, so TWO workgroups share a CU and one runs its MFMAs while the other stages.
#include "vt_halo.h"
#include "vt_kernels.h"

namespace {

constexpr int HB = 64;                     // bytes per LDS row (32 16-bit channels)
constexpr int TW = 16;                     // low-resolution tile width (one MFMA column block)
constexpr int HWID = TW + 2;               // halo width
constexpr int ROWS = 8;                    // low-resolution tile rows: 2 per wave
constexpr int NWV = 4;                     // waves per workgroup
constexpr int TPW = 2;                     // low-resolution rows per wave
constexpr int BC = 64;                     // couts per workgroup
constexpr int TC = 4;                      // 16-cout MFMA tiles per wave
constexpr int HROWS = (ROWS + 2) * HWID;   // 180 halo pixels
constexpr int XPCS = (HROWS + 15) / 16;    // 12 DMA pieces (16 LDS rows each) per halo
constexpr int XBUF = XPCS * 16 * HB;       // 12 KB
constexpr int WBLK = BC * HB;              // one folded matrix's 64-cout tile: 4 KB
constexpr int WPCS = 16 * BC / 16;         // 64 DMA pieces per chunk (16 K-steps x 4)
constexpr int SMEM = XBUF + 16 * WBLK;     // 77 824 B

template <bool F16>
__device__ __forceinline__ f32x4 up2_mfma(bf16x8 a, bf16x8 b, f32x4 c) {
    if constexpr (F16) {
        typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    } else {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
}

template <bool F16>
__global__ __launch_bounds__(64 * NWV, 2)
void conv3x3_up2_kernel(const ConvUp2Args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const xbase = smem;
    char* const wbase = smem + XBUF;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // = the wave's row pair inside the tile
    const int fr = lane & 15, fq = lane >> 4;

    // ---- tile coordinates: blocks run (image, pixel tile, cout tile) with the cout tile fastest
    int logical = vt_xcd_remap(blockIdx.x, gridDim.x);
    const int per_img = a.ptiles * a.ctiles;
    const int b = logical / per_img;
    logical -= b * per_img;
    const int tile = logical / a.ctiles;
    const int ct = logical - tile * a.ctiles;
    const int tyi = tile / a.tiles_x;
    const int ty0 = tyi * ROWS, tx0 = (tile - tyi * a.tiles_x) * TW;
    const int c0 = ct * BC;

    const bf16_t* Xb = a.X + (long long)b * a.H * a.W * a.Cin;
    const int nchunk = a.Cin >> 5;

    // ---- staging.  One DMA piece = 16 LDS rows x 64 B; lane l -> row (l >> 2), physical 16-B chunk (l & 3); the logical chunk is
    // physical ^ (((row >> 2) & 1) << 1) (conv3x3_halo.hip's swizzle: ds_read_b128 of 16 consecutive rows is then conflict-free at every shift)
    const int drow = lane >> 2;
    const int dchunk = (lane & 3) ^ (((lane >> 4) & 1) << 1);
    auto stage = [&](int chunk) {
#pragma nounroll
        for (int pc = wave; pc < XPCS; pc += NWV) {
            const int hr = pc * 16 + drow;
            const int hy = hr / HWID, hx = hr - hy * HWID;
            const int iy = ty0 - 1 + hy, ix = tx0 - 1 + hx;
            const bool v = hr < HROWS && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            const void* src = v ? (const void*)(Xb + ((iy * a.W + ix) * a.Cin + dchunk * 8 + chunk * 32)) : a.zeros;
            __builtin_amdgcn_global_load_lds(VT_GLOBAL_PTR(src), VT_LDS_PTR(xbase + pc * 1024), 16, 0, 0);
        }
        // Wp[chunk][phase * 4 + tap][Cout rows][32]: K-step q's tile of this workgroup's 64 couts is 4 pieces
        const bf16_t* wsrc = a.Wp + ((long long)chunk * 16 * a.Cout + c0 + drow) * 32 + dchunk * 8;
#pragma nounroll
        for (int pc = wave; pc < WPCS; pc += NWV) {
            const int q = pc >> 2, part = pc & 3;
            __builtin_amdgcn_global_load_lds(VT_GLOBAL_PTR(wsrc + ((long long)q * a.Cout + part * 16) * 32), VT_LDS_PTR(wbase + pc * 1024), 16, 0, 0);
        }
    };

    // accumulators start at the bias; tile i / register r of lane (fq, fr) = cout c0 + 16 fq + 4 i + r.
    // acc[i][p * 2 + j]: phase p = a * 2 + b, low-resolution row j of the wave
    f32x4 acc[TC][8];
#pragma unroll
    for (int i = 0; i < TC; ++i) {
        const f32x4 bv = a.bias ? *(const f32x4*)(a.bias + c0 + 16 * fq + 4 * i) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = bv;
    }

    // fragment addresses.  W tile row i * 16 + fr: its swizzle bit is bit 2 of fr (tile bases are multiples of 16 rows)
    const int wfoff = fr * HB + ((fq ^ (((fr >> 2) & 1) << 1)) << 4);

#pragma nounroll
    for (int chunk = 0; chunk < nchunk; ++chunk) {
        __syncthreads();                                   // every wave's fragment reads of the previous chunk have returned
        stage(chunk);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces have landed ...
        __syncthreads();                                   // ... and everybody else's
        // the 9 shifts x this wave's rows: halo row (2 wave + r), r = 0..3, column shift s = 0..2
        bf16x8 xf[4][3];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const int row = (wave * TPW + r) * HWID + s + fr;
                xf[r][s] = *(const bf16x8*)(xbase + row * HB + ((fq ^ (((row >> 2) & 1) << 1)) << 4));
            }
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int pa = p >> 1, pb = p & 1;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int ry = t >> 1, rx = t & 1;           // folded tap: low-resolution offset (ry - 1 + pa, rx - 1 + pb)
                const char* ws = wbase + (p * 4 + t) * WBLK + wfoff;
                bf16x8 wf[TC];
#pragma unroll
                for (int i = 0; i < TC; ++i) wf[i] = *(const bf16x8*)(ws + i * 16 * HB);
#pragma unroll
                for (int j = 0; j < TPW; ++j) {
#pragma unroll
                    for (int i = 0; i < TC; ++i)
                        acc[i][p * 2 + j] = up2_mfma<F16>(wf[i], xf[j + ry + pa][rx + pb], acc[i][p * 2 + j]);
                }
            }
        }
    }

    // ---- epilogue: a lane owns 16 consecutive couts of output pixel (2 (ty0 + 2 wave + j) + pa, 2 (tx0 + fr) + pb)
    const int Ho = 2 * a.H, Wo = 2 * a.W;
    const long long ob = (long long)b * Ho * Wo * a.Cout;
    const int lx = tx0 + fr;
    const int cw = c0 + 16 * fq;
    unsigned valid = 0;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
            const int ly = ty0 + wave * TPW + j;
            if (ly >= a.H || lx >= a.W) continue;
            const int jj = p * 2 + j;
            valid |= 1u << jj;
            const long long o = ob + ((long long)(2 * ly + (p >> 1)) * Wo + (2 * lx + (p & 1))) * a.Cout + cw;
            if (a.out_f32) {
#pragma unroll
                for (int i = 0; i < TC; ++i) *(f32x4*)(a.out_f32 + o + 4 * i) = acc[i][jj];
            }
            if (a.out_f16) {
#pragma unroll
                for (int i = 0; i < TC; i += 2) vt_halo_store16(a.out_f16 + o + 4 * i, acc[i][jj], acc[i + 1][jj]);
            }
            if (a.out_16) {
#pragma unroll
                for (int i = 0; i < TC; i += 2) {
                    if (a.out16_f16) vt_halo_store16((f16_t*)a.out_16 + o + 4 * i, acc[i][jj], acc[i + 1][jj]);
                    else vt_halo_store16(a.out_16 + o + 4 * i, acc[i][jj], acc[i + 1][jj]);
                }
            }
        }
    }
    if (a.gn_partial) {
        // GroupNorm (n, mean, M2) of this tile's outputs for the next norm1: one triple per (tile, group), merged in a fixed order
        __syncthreads();                                   // every wave is done with the staging LDS
        const int G = a.Cout / a.gn_cpg;
        float* out = a.gn_partial + (((long long)b * a.ptiles + tile) * G + c0 / a.gn_cpg) * 3;
        vt_gn_epilogue_partials_il<TC, 8>(acc, valid, a.gn_cpg, wave, NWV, 0, BC, (float*)smem, out);
    }
}

template <bool F16>
hipError_t launch_up2(const ConvUp2Args& a, hipStream_t s) {
    static std::atomic<unsigned long long> attr_done{0};
    auto kern = conv3x3_up2_kernel<F16>;
    hipError_t ea = vt_dynamic_smem_once(attr_done, SMEM, kern);
    if (ea != hipSuccess) return ea;
    ConvUp2Args k = a;
    k.tiles_x = (a.W + TW - 1) / TW;
    k.ptiles = k.tiles_x * ((a.H + ROWS - 1) / ROWS);
    k.ctiles = a.Cout / BC;
    const long long nblk = (long long)k.ptiles * k.ctiles * a.batch;
    if (nblk <= 0 || nblk > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(64 * NWV), SMEM, s, k);
    return hipGetLastError();
}

// fp32 OIHW -> the folded packing Wp[Cin/32][phase * 4 + tap][Cout rows][32], a bf16 and an fp16 copy.  The fp32 sum runs ky-major, kx
// inside, left to right, and is rounded to the operand type once.
__global__ void pack_up2_kernel(const float* __restrict__ w, bf16_t* __restrict__ wp_bf16, f16_t* __restrict__ wp_f16, int Cin, int Cout) {
    const long long n = (long long)Cout * Cin * 16;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int q = (int)(idx & 15);
    const int ci = (int)((idx >> 4) % Cin);
    const int co = (int)((idx >> 4) / Cin);
    const int pa = q >> 3, pb = (q >> 2) & 1, ry = (q >> 1) & 1, rx = q & 1;
    // taps of the 3x3 kernel that land on folded tap ry of phase pa: (pa, ry) = (0,0) {0}, (0,1) {1,2}, (1,0) {0,1}, (1,1) {2}
    const int ky0 = pa == 0 ? (ry == 0 ? 0 : 1) : (ry == 0 ? 0 : 2), ky1 = pa == 0 ? (ry == 0 ? 0 : 2) : (ry == 0 ? 1 : 2);
    const int kx0 = pb == 0 ? (rx == 0 ? 0 : 1) : (rx == 0 ? 0 : 2), kx1 = pb == 0 ? (rx == 0 ? 0 : 2) : (rx == 0 ? 1 : 2);
    const float* wt = w + ((long long)co * Cin + ci) * 9;
    float sum = 0.f;
    bool first = true;
    for (int ky = ky0; ky <= ky1; ++ky)
        for (int kx = kx0; kx <= kx1; ++kx) {
            const float v = wt[ky * 3 + kx];
            sum = first ? v : __fadd_rn(sum, v);
            first = false;
        }
    const int row = (co & ~63) + vt_halo_row_of_cout(co & 63);
    const long long d = (((long long)(ci >> 5) * 16 + q) * Cout + row) * 32 + (ci & 31);
    if (wp_bf16) wp_bf16[d] = (bf16_t)sum;
    if (wp_f16) wp_f16[d] = (f16_t)sum;
}

// fp32 OIHW 3x3 -> the stride-1 kernels' 16-bit operands (the literal route): layout 0 = [Cout][tap][Cin] (generic GEMM),
// 1 = conv3x3_halo.hip's Wp[Cin/32][step][Cout rows][32]; f16 selects fp16 instead of bf16 bits
__global__ void pack_f32_oihw_kernel(const float* __restrict__ w, bf16_t* __restrict__ dst, int Cin, int Cout, int layout, int f16) {
    const long long n = (long long)Cout * Cin * 9;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int tap = (int)(idx % 9);
    const int ci = (int)((idx / 9) % Cin);
    const int co = (int)(idx / ((long long)Cin * 9));
    const int row = (co & ~63) + vt_halo_row_of_cout(co & 63);
    const long long d = layout == 0 ? ((long long)co * 9 + tap) * Cin + ci
                                    : (((long long)(ci >> 5) * 9 + vt_halo_step_of_tap(tap)) * Cout + row) * 32 + (ci & 31);
    if (f16) ((f16_t*)dst)[d] = (f16_t)w[idx]; else dst[d] = (bf16_t)w[idx];
}

// nearest-neighbour 2x of NHWC 16-bit rows, 16 B per thread (the literal route's intermediate tensor)
__global__ __launch_bounds__(256)
void upsample2x_nhwc16_kernel(const uint4* __restrict__ x, uint4* __restrict__ y, int H, int W, int C8, long long n) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int c = (int)(idx % C8);
    long long p = idx / C8;
    const int X = (int)(p % (2 * W)); p /= 2 * W;
    const int Y = (int)(p % (2 * H));
    const long long b = p / (2 * H);
    y[idx] = x[((b * H + (Y >> 1)) * W + (X >> 1)) * C8 + c];
}

}  // namespace

bool vt_conv3x3_up2_supported(int Cin, int Cout) { return Cin >= 32 && (Cin % 32) == 0 && Cout >= BC && (Cout % BC) == 0; }
int vt_conv3x3_up2_tiles(int H, int W) { return ((W + TW - 1) / TW) * ((H + ROWS - 1) / ROWS); }

hipError_t vt_launch_conv3x3_up2(const ConvUp2Args& a, hipStream_t s) {
    if (!a.X || !a.Wp || !a.zeros || (!a.out_f32 && !a.out_f16 && !a.out_16)) return hipErrorInvalidValue;
    if (!vt_conv3x3_up2_supported(a.Cin, a.Cout) || a.batch <= 0 || a.H <= 0 || a.W <= 0) return hipErrorInvalidValue;
    if (!vt_gn_cpg_ok(a.gn_partial, a.gn_cpg) || !vt_fits_i32((long long)a.H * a.W * a.Cin)) return hipErrorInvalidValue;
    if ((long long)a.H * 2 + 1 >= (1LL << 30) || (long long)a.W * 2 + 1 >= (1LL << 30)) return hipErrorInvalidValue;
    return a.f16 ? launch_up2<true>(a, s) : launch_up2<false>(a, s);
}

hipError_t vt_launch_pack_up2(const float* w_oihw, bf16_t* wp_bf16, f16_t* wp_f16, int Cin, int Cout, hipStream_t s) {
    const long long n = (long long)Cout * Cin * 16;
    if (!w_oihw || (!wp_bf16 && !wp_f16) || n <= 0 || (n + 255) / 256 > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pack_up2_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w_oihw, wp_bf16, wp_f16, Cin, Cout);
    return hipGetLastError();
}

hipError_t vt_launch_pack_f32_oihw(const float* w_oihw, bf16_t* dst, int Cin, int Cout, int layout, int f16, hipStream_t s) {
    const long long n = (long long)Cout * Cin * 9;
    if (!w_oihw || !dst || n <= 0 || (n + 255) / 256 > 0x7fffffffLL || (layout == 1 && (Cin % 32 || Cout % 64))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pack_f32_oihw_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w_oihw, dst, Cin, Cout, layout, f16);
    return hipGetLastError();
}

hipError_t vt_launch_upsample2x_nhwc16(const void* x, void* y, int B, int H, int W, int C, hipStream_t s) {
    if (!x || !y || B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C % 8)) return hipErrorInvalidValue;
    const long long n = (long long)B * 2 * H * 2 * W * (C / 8);
    if ((n + 255) / 256 > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(upsample2x_nhwc16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const uint4*)x, (uint4*)y, H, W, C / 8, n);
    return hipGetLastError();
}
