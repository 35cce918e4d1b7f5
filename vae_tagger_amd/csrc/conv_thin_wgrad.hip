// Weight gradient of the VAE's two full-resolution end convs, 3x3 pad 1 with 3 channels on one side (encoder.conv_in 3 -> C, decoder.conv_out C -> 3;
// DESIGN.md section 4.23), and the device-side packer of conv_in's weight layouts.
//
// Operands: thin = the 3-channel side, fp32 NCHW [B][3][H][W]; wide = the 16-bit side, bf16 NHWC [B][H][W][Cw].  Both forms are ONE matrix product
//   D[r][c] = sum over pixels p = (b, y, x) of T_r[p] * wide[p][c],     r = t * 9 + ky * 3 + kx  (27 rows, padded to 32),
//   T_r[p] = thin[b][t][y + s (ky - 1)][x + s (kx - 1)]  (0 outside the image),  s = +1 for conv_in (thin is the conv's input), -1 for conv_out (thin is dy),
// with the PIXEL index as K.  They differ in the sign of the tap offset and in where D[r][c] lands in dw ([Cw][27] or [3][Cw][9]).
//
// A workgroup (4 waves) owns 64 columns (channels) of D and one contiguous slice of the pixel tiles (TW_TH rows x 32 pixels).  Per tile it stages
//   the [TW_TH x 32 pixels][64 channels] piece of wide, row-major as it lies in HBM, in conv_wgrad.hip's LDS image: a staged pixel is 128 B padded to
//   160 B, so that the 8 consecutive pixels a 32-lane half reads with ds_read_b64_tr_b16 fall into eight disjoint 8-dword bank windows (the argument at
//   the top of conv_wgrad.hip; here only the un-shifted reads occur), and
//   the fp32 halo [3][TW_TH + 2][34] of thin, as conv_in_mfma_kernel stages its image.
// The thin operand needs no transpose: a row's pixels are contiguous in NCHW, which is the K direction.  A lane of the A operand holds row r = lane & 15
// (+ 16 for the second row tile) and the 8 pixels 16 (j >> 2) + 4 (lane >> 4) + (j & 3), j = 0..7 -- the K order of the transposed reads -- which it
// reads as 8 floats from the halo at its own tap offset and SPLITS: hi = bf16(v), lo = bf16(v - hi), two MFMAs into the same accumulators (the
// products are fp32-grade on the thin side, as in the forward conv_in).  Rows 27..31 are zeros.  The waves share the K dimension: wave w takes tile
// rows w and w + 4, all 64 columns (4 column tiles x 2 row tiles = 8 accumulators); at the end the four waves' accumulators are added through LDS in
// wave order.  All 64 lanes are active at every transposed read; ragged tiles are zero-filled, never skipped.
//
// The next tile's pieces are loaded into registers before the current tile's MFMAs and written to LDS after them: the kernel is bound by the bytes of
// wide (one pass over it), not by its 16 MFMAs per 4 KB.
//
// Split over pixels: grid = splits x (Cw / 64); slice s covers tiles [s * steps / splits, (s + 1) * steps / splits) and writes its fp32 partial
// [32][Cw] to ws[s]; conv_thin_reduce_kernel adds the slices in slice order and scatters into dw's index order.  thin_sums: the workgroups of column
// block 0 add the INTERIOR of their thin pieces (never the halo) in fp64, one partial per slice, finished in slice order.  No atomics.
#include <atomic>

#include "vt_common.h"
#include "vt_kernels.h"

namespace {

constexpr int TW_TW = 32;          // pixels of one K-step: one row segment of the tile
constexpr int TW_TH = 8;           // rows per staged tile: two per wave
constexpr int TW_BC = 64;          // channels per workgroup
constexpr int TW_ROWB = 160;       // bytes per staged pixel
constexpr int TW_THREADS = 256;
constexpr int TW_CUS = 256;        // MI355X
constexpr int TW_PER_CU = 3;       // workgroups resident per CU: 45 040 B of LDS each
constexpr int TW_RW = TW_TW + 2, TW_RH = TW_TH + 2;
constexpr int TW_WIDE_BYTES = TW_TH * TW_TW * TW_ROWB;                  // 40 960
constexpr int TW_THIN_FLOATS = 3 * TW_RH * TW_RW;                       // 1020
constexpr int TW_LDS = TW_WIDE_BYTES + TW_THIN_FLOATS * 4;              // 45 040
constexpr int TW_WIDE_LOADS = TW_TH * TW_TW * 8 / TW_THREADS;           // 16-byte loads per thread and tile: 8
constexpr int TW_THIN_LOADS = (TW_THIN_FLOATS + TW_THREADS - 1) / TW_THREADS;   // 4
static_assert(TW_WIDE_BYTES >= 4 * 8 * 64 * 16, "the end reduction reuses the wide piece");

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

__device__ __forceinline__ bf16x8 tw_tr_operand(const char* p) {
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)p);
    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(p + 16 * TW_ROWB));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

struct TwTile { int b, y0, x0; };

__device__ __forceinline__ TwTile tw_tile(const ConvThinWgradArgs& g, int t) {
    const int per_img = g.tiles_x * g.tiles_y;
    const int b = t / per_img, r = t - b * per_img;
    return TwTile{b, (r / g.tiles_x) * TW_TH, (r % g.tiles_x) * TW_TW};
}

__global__ __launch_bounds__(TW_THREADS, 3) void conv_thin_wgrad_kernel(ConvThinWgradArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* swide = smem;
    float* sthin = (float*)(smem + TW_WIDE_BYTES);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nblk = g.Cw / TW_BC;
    const int blk = blockIdx.x % nblk, slice = blockIdx.x / nblk;
    const int c0 = blk * TW_BC;
    const int t0 = (int)((long long)slice * g.steps / g.splits), t1 = (int)((long long)(slice + 1) * g.steps / g.splits);
    const bool want_sums = g.thin_sums != nullptr && blk == 0;

    f32x4 acc[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    // the wide operand's transposed-read address (conv_wgrad.hip): lane 4 q + p of group grp supplies pixel 4 grp + q, columns 4 p .. 4 p + 3
    const int grp = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const int w_off = (4 * grp + q) * TW_ROWB + 4 * p * 2;
    // the thin operand's halo offset of this lane's two rows r = (lane & 15) + 16 m: float index of (plane t, halo row oy, halo column ox + 4 grp)
    int t_off[2];
    bool t_ok[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int r = (lane & 15) + 16 * m;
        t_ok[m] = r < 27;
        const int rr = t_ok[m] ? r : 0;
        const int t = rr / 9, ky = (rr - t * 9) / 3, kx = rr - t * 9 - ky * 3;
        const int oy = g.thin_is_input ? ky : 2 - ky, ox = g.thin_is_input ? kx : 2 - kx;
        t_off[m] = (t * TW_RH + oy) * TW_RW + ox + 4 * grp;
    }

    uint4 wreg[TW_WIDE_LOADS];
    float treg[TW_THIN_LOADS];
    auto fetch = [&](int t) {
        const TwTile tl = tw_tile(g, t);
#pragma unroll
        for (int i = 0; i < TW_WIDE_LOADS; ++i) {
            const int idx = tid + i * TW_THREADS, px = idx >> 3, ch = idx & 7;
            const int y = tl.y0 + px / TW_TW, x = tl.x0 + px % TW_TW;
            uint4 v = uint4{0u, 0u, 0u, 0u};
            if (y < g.H && x < g.W) v = *(const uint4*)(g.wide + (((long long)tl.b * g.H + y) * g.W + x) * g.Cw + c0 + ch * 8);
            wreg[i] = v;
        }
#pragma unroll
        for (int i = 0; i < TW_THIN_LOADS; ++i) {
            const int idx = tid + i * TW_THREADS;
            const int c = idx / (TW_RH * TW_RW), r = (idx / TW_RW) % TW_RH, xx = idx % TW_RW;
            const int iy = tl.y0 - 1 + r, ix = tl.x0 - 1 + xx;
            float v = 0.f;
            if (idx < TW_THIN_FLOATS && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W) v = g.thin[(((long long)tl.b * 3 + c) * g.H + iy) * g.W + ix];
            treg[i] = v;
        }
    };

    double tsum = 0.0;                                  // threads 0..191: plane tid >> 6, interior pixels lane, lane + 64, ... of every tile
    fetch(t0);
    for (int t = t0; t < t1; ++t) {
        __syncthreads();                               // the previous tile's reads are over
#pragma unroll
        for (int i = 0; i < TW_WIDE_LOADS; ++i) {
            const int idx = tid + i * TW_THREADS, px = idx >> 3, ch = idx & 7;
            *(uint4*)(swide + px * TW_ROWB + ch * 16) = wreg[i];
        }
#pragma unroll
        for (int i = 0; i < TW_THIN_LOADS; ++i) {
            const int idx = tid + i * TW_THREADS;
            if (idx < TW_THIN_FLOATS) sthin[idx] = treg[i];
        }
        __syncthreads();
        if (t + 1 < t1) fetch(t + 1);                  // in flight under this tile's MFMAs
        if (want_sums && wave < 3) {
#pragma unroll
            for (int i = 0; i < TW_TH * TW_TW / 64; ++i) {
                const int px = lane + 64 * i;
                tsum += (double)sthin[(wave * TW_RH + 1 + px / TW_TW) * TW_RW + 1 + px % TW_TW];
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int ty = wave + 4 * h;               // this wave's tile row: one K-step of 32 pixels
            bf16x8 th[2], tlo[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const float* src = sthin + t_off[m] + ty * TW_RW;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float v = t_ok[m] ? src[16 * (j >> 2) + (j & 3)] : 0.f;
                    th[m][j] = (bf16_t)v;
                    tlo[m][j] = (bf16_t)(v - (float)th[m][j]);
                }
            }
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const bf16x8 wf = tw_tr_operand(swide + w_off + n * 32 + ty * TW_TW * TW_ROWB);
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(th[m], wf, acc[m][n], 0, 0, 0);
                    acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tlo[m], wf, acc[m][n], 0, 0, 0);
                }
            }
        }
    }
    // the four waves' accumulators, added in wave order through the (now free) wide piece
    __syncthreads();
    f32x4* red = (f32x4*)swide;                        // [wave][m * 4 + n][lane]
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) red[(wave * 8 + m * 4 + n) * 64 + lane] = acc[m][n];
    double* dred = (double*)(smem + 4 * 8 * 64 * 16);   // [3][64], behind the accumulators (32 768 + 1536 <= 40 960)
    if (want_sums && wave < 3) dred[wave * 64 + lane] = tsum;
    __syncthreads();
    float* out = (float*)g.ws + (long long)slice * 32 * g.Cw;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int tile = (tid >> 6) + 4 * e, ln = tid & 63;            // D layout of 16x16x32: column = lane & 15, row = 4 (lane >> 4) + register
        f32x4 s = red[tile * 64 + ln];
#pragma unroll
        for (int w = 1; w < 4; ++w) s += red[(w * 8 + tile) * 64 + ln];
        const int m = tile >> 2, n = tile & 3;
        const int col = c0 + n * 16 + (ln & 15);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) out[(long long)(m * 16 + 4 * (ln >> 4) + rr) * g.Cw + col] = s[rr];
    }
    if (want_sums && tid < 3) {
        double s = 0.0;
        for (int i = 0; i < 64; ++i) s += dred[tid * 64 + i];
        ((double*)((char*)g.ws + (size_t)g.splits * 32 * g.Cw * sizeof(float)))[slice * 3 + tid] = s;
    }
}

constexpr int RED_UNROLL = 32;

// dw[index of (r, c)] = ws[0][r][c] + ws[1][r][c] + ... in slice order; thin_sums[t] = the fp64 partials in slice order
__global__ __launch_bounds__(256) void conv_thin_reduce_kernel(ConvThinWgradArgs g) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const float* ws = (const float*)g.ws;
    if (i < 27 * g.Cw) {
        const int r = i / g.Cw, c = i - r * g.Cw;
        // with hundreds of slices this loop is a chain of load latencies: RED_UNROLL independent loads are in flight before their (ordered) adds
        const long long stride = 32LL * g.Cw;
        float s = ws[i];
        int k = 1;
        for (; k + RED_UNROLL <= g.splits; k += RED_UNROLL) {
            float v[RED_UNROLL];
#pragma unroll
            for (int j = 0; j < RED_UNROLL; ++j) v[j] = ws[(k + j) * stride + i];
#pragma unroll
            for (int j = 0; j < RED_UNROLL; ++j) s += v[j];
        }
        for (; k < g.splits; ++k) s += ws[k * stride + i];
        const int t = r / 9, tap = r - t * 9;
        g.dw[g.thin_is_input ? c * 27 + r : (t * g.Cw + c) * 9 + tap] = s;
    }
    if (g.thin_sums && i < 3) {
        const double* part = (const double*)((const char*)g.ws + (size_t)g.splits * 32 * g.Cw * sizeof(float));
        double s = 0.0;
        int k = 0;
        for (; k + RED_UNROLL <= g.splits; k += RED_UNROLL) {
            double v[RED_UNROLL];
#pragma unroll
            for (int j = 0; j < RED_UNROLL; ++j) v[j] = part[(k + j) * 3 + i];
#pragma unroll
            for (int j = 0; j < RED_UNROLL; ++j) s += v[j];
        }
        for (; k < g.splits; ++k) s += part[k * 3 + i];
        g.thin_sums[i] = (float)s;
    }
}

// conv_in's weight layouts (weights.hip's pack_conv_in / pack_conv_in_mfma), one thread per (cout, k)
__device__ __forceinline__ float thin_w(const float* w, int rotate, int C, int o, int k) {
    if (!rotate) return w[o * 27 + k];
    const int t = k / 9, tap = k - t * 9;
    return w[(t * C + o) * 9 + 8 - tap];                // W'[o][t][ky][kx] = w[t][o][2 - ky][2 - kx]
}

__global__ __launch_bounds__(256) void pack_conv_thin_kernel(const float* __restrict__ w, const float* __restrict__ bias, int rotate, int mfma,
                                                             void* __restrict__ dst, float* __restrict__ zero_bias, int C) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= C * 32) return;
    const int o = i >> 5, k = i & 31;
    if (zero_bias && k == 0) zero_bias[o] = 0.f;
    if (!mfma) {
        if (k < 27) ((float*)dst)[k * C + o] = thin_w(w, rotate, C, o, k);
        return;
    }
    bf16_t* pk = (bf16_t*)dst;
    const int row = (o & ~63) + vt_halo_row_of_cout(o & 63);
    bf16_t hi = (bf16_t)0.f, lo = (bf16_t)0.f;
    if (k < 27) {
        const float f = thin_w(w, rotate, C, o, k);
        hi = (bf16_t)f;
        lo = (bf16_t)(f - (float)hi);
    } else if (k < 30) {                                // the bias as three bf16 pieces
        float rest = bias ? bias[o] : 0.f;
        for (int kk = 27; kk <= k; ++kk) {
            hi = (bf16_t)rest;
            rest -= (float)hi;
        }
    }
    pk[row * 32 + k] = hi;
    pk[(128 + row) * 32 + k] = lo;
}

}  // namespace

int vt_conv_thin_wgrad_steps(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    const long long n = (long long)B * ((H + TW_TH - 1) / TW_TH) * ((W + TW_TW - 1) / TW_TW);
    return n > 0x7fffffffLL ? 0 : (int)n;
}

bool vt_conv_thin_wgrad_supported(int Cw) { return Cw >= TW_BC && (Cw % TW_BC) == 0 && Cw <= 512; }

int vt_conv_thin_wgrad_auto_splits(int B, int H, int W, int Cw) {
    const int steps = vt_conv_thin_wgrad_steps(B, H, W);
    if (steps <= 0 || !vt_conv_thin_wgrad_supported(Cw)) return 0;
    int sp = TW_PER_CU * TW_CUS / (Cw / TW_BC);
    if (sp < 1) sp = 1;
    return sp > steps ? steps : sp;
}

size_t vt_conv_thin_wgrad_ws_bytes(int Cw, int splits) {
    return (size_t)splits * 32 * Cw * sizeof(float) + (size_t)splits * 3 * sizeof(double);
}

hipError_t vt_launch_conv_thin_wgrad(const ConvThinWgradArgs& a_in, hipStream_t s) {
    ConvThinWgradArgs a = a_in;
    if (!a.thin || !a.wide || !a.dw || !a.ws || !vt_conv_thin_wgrad_supported(a.Cw)) return hipErrorInvalidValue;
    a.steps = vt_conv_thin_wgrad_steps(a.batch, a.H, a.W);
    if (a.steps <= 0 || a.splits < 1 || a.splits > a.steps) return hipErrorInvalidValue;
    a.tiles_x = (a.W + TW_TW - 1) / TW_TW;
    a.tiles_y = (a.H + TW_TH - 1) / TW_TH;
    a.thin_is_input = a.thin_is_input != 0;
    static std::atomic<unsigned long long> done{0};
    hipError_t e = vt_dynamic_smem_once(done, TW_LDS, conv_thin_wgrad_kernel);
    if (e != hipSuccess) return e;
    const long long wgs = (long long)a.splits * (a.Cw / TW_BC);
    if (wgs > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(conv_thin_wgrad_kernel, dim3((unsigned)wgs), dim3(TW_THREADS), TW_LDS, s, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(conv_thin_reduce_kernel, dim3((unsigned)((27 * a.Cw + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t vt_launch_pack_conv_thin(const float* w, const float* bias, int rotate, int mfma, void* dst, float* zero_bias, int C, hipStream_t s) {
    if (!w || !dst || C <= 0 || (mfma && C != 128)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pack_conv_thin_kernel, dim3((unsigned)((C * 32 + 255) / 256)), dim3(256), 0, s, w, bias, rotate, mfma, dst, zero_bias, C);
    return hipGetLastError();
}
