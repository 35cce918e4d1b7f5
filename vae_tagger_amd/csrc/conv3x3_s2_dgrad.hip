// Data gradient of Downsample2D's conv (3x3, stride 2, padding (0,1,0,1)) in SCATTER form, as ONE kernel on the low-resolution gradient.
// The forward is y[i][j] = sum W[ky][kx] x[2i + ky][2j + kx], so by the parity of the dx pixel:
//
//   dx row 2i     (phase a = 0):  ky 0 from dy row i,  ky 2 from dy row i - 1
//   dx row 2i + 1 (phase a = 1):  ky 1 from dy row i
//
// and the same table for columns; dy rows / columns outside [0, Ho) x [0, Wo) count as 0.  The four phases of a 2x2 output quad have 4, 2, 2
// and 1 taps: 9 (phase, tap) products -- each of the nine weight matrices is used exactly once per quad -- where the literal route (dy scattered
// to the odd positions of a zeroed H x W tensor, then the stride-1 data gradient) spends 36.
//
// Skeleton of conv3x3_up2.hip: one low-resolution 16-bit halo staged in LDS once per 32-channel chunk by LDS-DMA feeds four output phases per wave;
// v_mfma_f32_16x16x32_bf16 with fp32 accumulation, weights = A operand with the interleaved output-channel rows (a lane owns 16 consecutive cins of
// its pixel).  The K dimension is Cout; the output channels are Cin.  Tile: 4 waves, 8 x 16 low-resolution quads (16 x 32 pixels of dx) x 64 cins
// per workgroup, a wave owns 2 quad rows = 32 accumulator tiles.  The halo reaches one row up and one column left only: (ROWS + 1) x 17 = 153
// pixels = 10 KB, the chunk's nine weight tiles 36 KB: 46 KB, two workgroups per CU (__launch_bounds__(256, 2): 128 accumulator registers of 256).
//
// For odd H (W) the last row (column) of dx exists in phase 0 only: the quad grid covers (H + 1) / 2 x (W + 1) / 2 quads, the staging tests dy's
// own bounds Ho = H / 2, Wo = W / 2, and a missing phase is masked AT THE STORE; the K-loop never skips.
#include "vt_common.h"
#include "vt_kernels.h"

namespace {

constexpr int HB = 64;                     // bytes per LDS row (32 bf16 channels)
constexpr int TW = 16;                     // quad tile width (one MFMA column block)
constexpr int HWID = TW + 1;               // halo width: one column to the left
constexpr int ROWS = 8;                    // quad rows per tile: 2 per wave
constexpr int NWV = 4;
constexpr int TPW = 2;
constexpr int BC = 64;                     // cins per workgroup
constexpr int TC = 4;                      // 16-cin MFMA tiles per wave
constexpr int HROWS = (ROWS + 1) * HWID;   // 153 halo pixels
constexpr int XPCS = (HROWS + 15) / 16;    // 10 DMA pieces
constexpr int XBUF = XPCS * 16 * HB;       // 10 KB
constexpr int WBLK = BC * HB;              // one tap's 64-cin tile: 4 KB
constexpr int WPCS = 9 * BC / 16;          // 36 DMA pieces per chunk
constexpr int SMEM = XBUF + 9 * WBLK;      // 47 104 B

__global__ __launch_bounds__(64 * NWV, 2)
void conv3x3_s2_dgrad_kernel(const ConvS2DgradArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[SMEM];      // static (< 64 KB): the code object reports it
    char* const xbase = smem;
    char* const wbase = smem + XBUF;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fr = lane & 15, fq = lane >> 4;

    int logical = vt_xcd_remap(blockIdx.x, gridDim.x);
    const int per_img = a.ptiles * a.ctiles;
    const int b = logical / per_img;
    logical -= b * per_img;
    const int tile = logical / a.ctiles;
    const int ct = logical - tile * a.ctiles;
    const int tyi = tile / a.tiles_x;
    const int ty0 = tyi * ROWS, tx0 = (tile - tyi * a.tiles_x) * TW;
    const int c0 = ct * BC;

    const bf16_t* Xb = a.dy + (long long)b * a.Ho * a.Wo * a.Cout;
    const int nchunk = a.Cout >> 5;

    // staging as conv3x3_up2.hip: one DMA piece = 16 LDS rows x 64 B, lane l -> row (l >> 2), physical 16-B chunk (l & 3), logical chunk =
    // physical ^ (((row >> 2) & 1) << 1)
    const int drow = lane >> 2;
    const int dchunk = (lane & 3) ^ (((lane >> 4) & 1) << 1);
    auto stage = [&](int chunk) {
#pragma nounroll
        for (int pc = wave; pc < XPCS; pc += NWV) {
            const int hr = pc * 16 + drow;
            const int hy = hr / HWID, hx = hr - hy * HWID;
            const int iy = ty0 - 1 + hy, ix = tx0 - 1 + hx;
            const bool v = hr < HROWS && iy >= 0 && iy < a.Ho && ix >= 0 && ix < a.Wo;
            const void* src = v ? (const void*)(Xb + ((iy * a.Wo + ix) * a.Cout + dchunk * 8 + chunk * 32)) : a.zeros;
            __builtin_amdgcn_global_load_lds(VT_GLOBAL_PTR(src), VT_LDS_PTR(xbase + pc * 1024), 16, 0, 0);
        }
        // Wp[chunk][tap][Cin rows][32]: tap q's tile of this workgroup's 64 cins is 4 pieces
        const bf16_t* wsrc = a.Wp + ((long long)chunk * 9 * a.Cin + c0 + drow) * 32 + dchunk * 8;
#pragma nounroll
        for (int pc = wave; pc < WPCS; pc += NWV) {
            const int q = pc >> 2, part = pc & 3;
            __builtin_amdgcn_global_load_lds(VT_GLOBAL_PTR(wsrc + ((long long)q * a.Cin + part * 16) * 32), VT_LDS_PTR(wbase + pc * 1024), 16, 0, 0);
        }
    };

    // acc[i][p * 2 + j]: phase p = a * 2 + b, quad row j of the wave; tile i / register r of lane (fq, fr) = cin c0 + 16 fq + 4 i + r
    f32x4 acc[TC][8];
#pragma unroll
    for (int i = 0; i < TC; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int wfoff = fr * HB + ((fq ^ (((fr >> 2) & 1) << 1)) << 4);

#pragma nounroll
    for (int chunk = 0; chunk < nchunk; ++chunk) {
        __syncthreads();
        stage(chunk);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        // halo row (2 wave + r), r = 0..2, = dy row ty0 + 2 wave + r - 1; column shift s = 0..1 = dy column tx0 + fr + s - 1
        bf16x8 xf[3][2];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int row = (wave * TPW + r) * HWID + s + fr;
                xf[r][s] = *(const bf16x8*)(xbase + row * HB + ((fq ^ (((row >> 2) & 1) << 1)) << 4));
            }
        }
        // the 9-entry K-step table: tap (ky, kx) belongs to phase (ky == 1, kx == 1) and reads dy row i - (ky == 2), column j - (kx == 2)
#pragma unroll
        for (int q = 0; q < 9; ++q) {
            const int ky = q / 3, kx = q - 3 * ky;
            const int p = (ky == 1 ? 2 : 0) + (kx == 1 ? 1 : 0);
            const int dr = ky == 2 ? 0 : 1, dc = kx == 2 ? 0 : 1;
            const char* ws = wbase + q * WBLK + wfoff;
            bf16x8 wf[TC];
#pragma unroll
            for (int i = 0; i < TC; ++i) wf[i] = *(const bf16x8*)(ws + i * 16 * HB);
#pragma unroll
            for (int j = 0; j < TPW; ++j) {
#pragma unroll
                for (int i = 0; i < TC; ++i)
                    acc[i][p * 2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[i], xf[j + dr][dc], acc[i][p * 2 + j], 0, 0, 0);
            }
        }
    }

    // epilogue: a lane owns 16 consecutive cins of dx pixel (2 (ty0 + 2 wave + j) + pa, 2 (tx0 + fr) + pb); ragged phases are masked here
    const long long ob = (long long)b * a.H * a.W * a.Cin;
    const int cw = c0 + 16 * fq;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
            const int Y = 2 * (ty0 + wave * TPW + j) + (p >> 1), X = 2 * (tx0 + fr) + (p & 1);
            if (Y >= a.H || X >= a.W) continue;
            const long long o = ob + ((long long)Y * a.W + X) * a.Cin + cw;
#pragma unroll
            for (int i = 0; i < TC; ++i) {
                f32x4 v = acc[i][p * 2 + j];
                if (a.dx_add) v += *(const f32x4*)(a.dx_add + o + 4 * i);
                *(f32x4*)(a.dx + o + 4 * i) = v;
            }
        }
    }
}

// fp32 OIHW -> Wp[Cout/32][ky * 3 + kx][Cin rows][32] bf16: the transposes of the nine tap matrices, rounded once
__global__ void pack_s2_dgrad_kernel(const float* __restrict__ w, bf16_t* __restrict__ wp, int Cin, int Cout) {
    const long long n = (long long)Cout * Cin * 9;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;       // over w [Cout][Cin][9]
    if (idx >= n) return;
    const int q = (int)(idx % 9);
    const int ci = (int)((idx / 9) % Cin);
    const int co = (int)(idx / ((long long)Cin * 9));
    const int row = (ci & ~63) + vt_halo_row_of_cout(ci & 63);
    wp[(((long long)(co >> 5) * 9 + q) * Cin + row) * 32 + (co & 31)] = (bf16_t)w[idx];
}

}  // namespace

bool vt_conv3x3_s2_dgrad_supported(int Cin, int Cout) { return Cin >= BC && (Cin % BC) == 0 && Cout >= 32 && (Cout % 32) == 0; }

hipError_t vt_launch_pack_s2_dgrad(const float* w_oihw, bf16_t* wp, int Cin, int Cout, hipStream_t s) {
    const long long n = (long long)Cout * Cin * 9;
    if (!w_oihw || !wp || !vt_conv3x3_s2_dgrad_supported(Cin, Cout) || (n + 255) / 256 > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pack_s2_dgrad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w_oihw, wp, Cin, Cout);
    return hipGetLastError();
}

hipError_t vt_launch_conv3x3_s2_dgrad(const ConvS2DgradArgs& a, hipStream_t s) {
    if (!a.dy || !a.Wp || !a.dx || !a.zeros) return hipErrorInvalidValue;
    if (!vt_conv3x3_s2_dgrad_supported(a.Cin, a.Cout) || a.batch <= 0 || a.H < 2 || a.W < 2) return hipErrorInvalidValue;
    if ((long long)(a.H / 2) * (a.W / 2) * a.Cout >= (1LL << 31) || a.H >= (1 << 29) || a.W >= (1 << 29)) return hipErrorInvalidValue;     // 32-bit per-image dy offsets
    ConvS2DgradArgs k = a;
    k.Ho = a.H / 2; k.Wo = a.W / 2;
    k.tiles_x = ((a.W + 1) / 2 + TW - 1) / TW;
    k.ptiles = k.tiles_x * (((a.H + 1) / 2 + ROWS - 1) / ROWS);
    k.ctiles = a.Cin / BC;
    const long long nblk = (long long)k.ptiles * k.ctiles * a.batch;
    if (nblk <= 0 || nblk > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(conv3x3_s2_dgrad_kernel, dim3((unsigned)nblk), dim3(64 * NWV), 0, s, k);
    return hipGetLastError();
}
