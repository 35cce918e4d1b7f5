// Data gradient of Upsample2D (nearest 2x, then 3x3 / stride 1 / pad 1) in GATHER form, as ONE kernel on the high-resolution gradient: the exact
// adjoint of conv3x3_up2.hip.  With that file's fold table (phase a, folded row tap ry reads low-resolution row i + ry - 1 + a),
//
//   dx[i'][j'][ci] = sum over the 16 (phase (a, b), tap (ry, rx)) pairs of  Wf[a, b, ry, rx][co][ci] * dy[2 (i' + 1 - ry - a) + a][2 (j' + 1 - rx - b) + b][co]
//
// i.e. a 4 x 4, stride-2 gather over dy rows 2i' - 1 .. 2i' + 2: 16 products per low-resolution pixel where the literal route (the stride-1 data
// gradient at 2h x 2w, then a 2x2 sum) spends 36 and writes and re-reads a 4x-sized fp32 tensor.  The weights are the transposes of the
// forward's own folded matrices: the same fp32 sums (ky-major, kx inside), rounded to bf16 once.
//
// Parity planes: dy[2u + a][2v + b] for fixed (a, b) is a low-resolution image P_ab[u][v], and phase (a, b) reads P_ab at row offsets
// 1 - ry - a and column offsets 1 - rx - b, all within {-1, 0, 1}.  The staging DMA picks every pixel's address itself, so each plane's
// (ROWS + 2) x 18 halo is staged DE-INTERLEAVED, as a dense low-resolution halo, and the fragment reads are those of conv3x3_up2.hip:
// 16 consecutive LDS rows per read, conflict-free under its swizzle.  No strided LDS read exists.
//
// K-loop: (32-cout chunk, row parity a); an iteration stages the two planes (a, 0), (a, 1) (2 x 12 KB) and the 8 folded matrices of phases
// (a, 0), (a, 1) (32 KB) -- 56 KB, so two workgroups share a CU and one stages while the other multiplies -- and runs 8 of the chunk's 16
// K-steps.  Tile as the forward: 4 waves, 8 x 16 low-resolution pixels x 64 cins, a wave owns 2 rows = 8 accumulator tiles.
#include <type_traits>

#include "vt_common.h"
#include "vt_kernels.h"

namespace {

constexpr int HB = 64;
constexpr int TW = 16;
constexpr int HWID = TW + 2;
constexpr int ROWS = 8;
constexpr int NWV = 4;
constexpr int TPW = 2;
constexpr int BC = 64;                     // cins per workgroup
constexpr int TC = 4;
constexpr int HROWS = (ROWS + 2) * HWID;   // 180 halo pixels per plane
constexpr int XPCS = (HROWS + 15) / 16;    // 12 DMA pieces per plane
constexpr int XBUF = XPCS * 16 * HB;       // 12 KB per plane
constexpr int WBLK = BC * HB;              // 4 KB
constexpr int WPCS = 8 * BC / 16;          // 32 DMA pieces per iteration
constexpr int SMEM = 2 * XBUF + 8 * WBLK;  // 57 344 B

__global__ __launch_bounds__(64 * NWV, 2)
void conv3x3_up2_dgrad_kernel(const ConvUp2DgradArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[SMEM];      // static (< 64 KB): the code object reports it
    char* const xbase = smem;
    char* const wbase = smem + 2 * XBUF;

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

    const int Wo = 2 * a.W;
    const bf16_t* Xb = a.dy + (long long)b * 4 * a.H * a.W * a.C;
    const int niter = (a.C >> 5) * 2;

    const int drow = lane >> 2;
    const int dchunk = (lane & 3) ^ (((lane >> 4) & 1) << 1);
    auto stage = [&](int chunk, int pa) {
#pragma nounroll
        for (int pc = wave; pc < 2 * XPCS; pc += NWV) {
            const int pb = pc >= XPCS ? 1 : 0;
            const int hr = (pc - pb * XPCS) * 16 + drow;
            const int hy = hr / HWID, hx = hr - hy * HWID;
            const int u = ty0 - 1 + hy, v = tx0 - 1 + hx;                   // the plane's (low-resolution) coordinates
            const bool ok = hr < HROWS && u >= 0 && u < a.H && v >= 0 && v < a.W;
            const void* src = ok ? (const void*)(Xb + (((2 * u + pa) * Wo + 2 * v + pb) * a.C + dchunk * 8 + chunk * 32)) : a.zeros;
            __builtin_amdgcn_global_load_lds(VT_GLOBAL_PTR(src), VT_LDS_PTR(xbase + pc * 1024), 16, 0, 0);
        }
        // Wp[chunk][pa * 8 + pb * 4 + tap][C rows][32]
        const bf16_t* wsrc = a.Wp + (((long long)chunk * 16 + pa * 8) * a.C + c0 + drow) * 32 + dchunk * 8;
#pragma nounroll
        for (int pc = wave; pc < WPCS; pc += NWV) {
            const int q = pc >> 2, part = pc & 3;
            __builtin_amdgcn_global_load_lds(VT_GLOBAL_PTR(wsrc + ((long long)q * a.C + part * 16) * 32), VT_LDS_PTR(wbase + pc * 1024), 16, 0, 0);
        }
    };

    f32x4 acc[TC][TPW];
#pragma unroll
    for (int i = 0; i < TC; ++i)
#pragma unroll
        for (int j = 0; j < TPW; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int wfoff = fr * HB + ((fq ^ (((fr >> 2) & 1) << 1)) << 4);

    // one iteration's 8 K-steps for row parity PA (a template so that every fragment index is static)
    auto steps = [&](auto pa_c) {
        constexpr int PA = decltype(pa_c)::value;
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) {
            bf16x8 xf[4][3];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    const int row = (wave * TPW + r) * HWID + s + fr;
                    xf[r][s] = *(const bf16x8*)(xbase + pb * XBUF + row * HB + ((fq ^ (((row >> 2) & 1) << 1)) << 4));
                }
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int ry = t >> 1, rx = t & 1;
                const char* ws = wbase + (pb * 4 + t) * WBLK + wfoff;
                bf16x8 wf[TC];
#pragma unroll
                for (int i = 0; i < TC; ++i) wf[i] = *(const bf16x8*)(ws + i * 16 * HB);
#pragma unroll
                for (int j = 0; j < TPW; ++j) {
#pragma unroll
                    for (int i = 0; i < TC; ++i)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[i], xf[j + 2 - ry - PA][2 - rx - pb], acc[i][j], 0, 0, 0);
                }
            }
        }
    };

#pragma nounroll
    for (int it = 0; it < niter; ++it) {
        const int chunk = it >> 1, pa = it & 1;
        __syncthreads();
        stage(chunk, pa);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (pa == 0) steps(std::integral_constant<int, 0>{}); else steps(std::integral_constant<int, 1>{});
    }

    const long long ob = (long long)b * a.H * a.W * a.C;
    const int lx = tx0 + fr;
    const int cw = c0 + 16 * fq;
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        const int ly = ty0 + wave * TPW + j;
        if (ly >= a.H || lx >= a.W) continue;
        const long long o = ob + ((long long)ly * a.W + lx) * a.C + cw;
#pragma unroll
        for (int i = 0; i < TC; ++i) {
            f32x4 v = acc[i][j];
            if (a.dx_add) v += *(const f32x4*)(a.dx_add + o + 4 * i);
            *(f32x4*)(a.dx + o + 4 * i) = v;
        }
    }
}

// fp32 OIHW -> Wp[C/32 (cout chunks)][phase * 4 + tap][C rows (cin)][32 couts]: conv3x3_up2.hip's folding arithmetic -- the fp32 sum runs ky-major,
// kx inside, left to right, and is rounded to bf16 once -- written transposed
__global__ void pack_up2_dgrad_kernel(const float* __restrict__ w, bf16_t* __restrict__ wp, int C) {
    const long long n = (long long)C * C * 16;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int q = (int)(idx & 15);
    const int ci = (int)((idx >> 4) % C);
    const int co = (int)((idx >> 4) / C);
    const int pa = q >> 3, pb = (q >> 2) & 1, ry = (q >> 1) & 1, rx = q & 1;
    const int ky0 = pa == 0 ? (ry == 0 ? 0 : 1) : (ry == 0 ? 0 : 2), ky1 = pa == 0 ? (ry == 0 ? 0 : 2) : (ry == 0 ? 1 : 2);
    const int kx0 = pb == 0 ? (rx == 0 ? 0 : 1) : (rx == 0 ? 0 : 2), kx1 = pb == 0 ? (rx == 0 ? 0 : 2) : (rx == 0 ? 1 : 2);
    const float* wt = w + ((long long)co * C + ci) * 9;
    float sum = 0.f;
    bool first = true;
    for (int ky = ky0; ky <= ky1; ++ky)
        for (int kx = kx0; kx <= kx1; ++kx) {
            const float v = wt[ky * 3 + kx];
            sum = first ? v : __fadd_rn(sum, v);
            first = false;
        }
    const int row = (ci & ~63) + vt_halo_row_of_cout(ci & 63);
    wp[(((long long)(co >> 5) * 16 + q) * C + row) * 32 + (co & 31)] = (bf16_t)sum;
}

}  // namespace

bool vt_conv3x3_up2_dgrad_supported(int C) { return C >= BC && (C % BC) == 0; }

hipError_t vt_launch_pack_up2_dgrad(const float* w_oihw, bf16_t* wp, int C, hipStream_t s) {
    const long long n = (long long)C * C * 16;
    if (!w_oihw || !wp || !vt_conv3x3_up2_dgrad_supported(C) || (n + 255) / 256 > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pack_up2_dgrad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w_oihw, wp, C);
    return hipGetLastError();
}

hipError_t vt_launch_conv3x3_up2_dgrad(const ConvUp2DgradArgs& a, hipStream_t s) {
    if (!a.dy || !a.Wp || !a.dx || !a.zeros) return hipErrorInvalidValue;
    if (!vt_conv3x3_up2_dgrad_supported(a.C) || a.batch <= 0 || a.H <= 0 || a.W <= 0) return hipErrorInvalidValue;
    if ((long long)4 * a.H * a.W * a.C >= (1LL << 31) || a.H >= (1 << 29) || a.W >= (1 << 29)) return hipErrorInvalidValue;     // 32-bit per-image dy offsets
    ConvUp2DgradArgs k = a;
    k.tiles_x = (a.W + TW - 1) / TW;
    k.ptiles = k.tiles_x * ((a.H + ROWS - 1) / ROWS);
    k.ctiles = a.C / BC;
    const long long nblk = (long long)k.ptiles * k.ctiles * a.batch;
    if (nblk <= 0 || nblk > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(conv3x3_up2_dgrad_kernel, dim3((unsigned)nblk), dim3(64 * NWV), 0, s, k);
    return hipGetLastError();
}
