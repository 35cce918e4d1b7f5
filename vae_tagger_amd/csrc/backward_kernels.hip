// The HBM-bound passes of the resnet block's backward: the cast + bias-gradient pass, the weight pack of the data gradient,
// the (mean, rstd) form of the GroupNorm statistics and the GroupNorm + SiLU backward.  fp32 rows [rows][C], a lane owns 4 consecutive channels of a
// pixel (16-B accesses).  Every sum over pixels is taken in fp64 -- per lane, then over the lanes of a workgroup, the chunks and the images in a FIXED
// order -- because an fp64 add per element is free in a pass that waits on HBM, and it makes the result independent of how the pixels are chunked
// to ~2^-53 instead of 2^-24.  No atomics.
#include "vt_common.h"
#include "vt_kernels.h"

namespace {

constexpr int BK_THREADS = 256;
constexpr int BK_PASSES = 32;            // pixel passes per workgroup of a summing kernel
constexpr int BK_FIN_ROWS = 16;          // finish kernels: 16 channels x 16 strided partial rows per workgroup

struct Lanes { int tpp, ppp, threads; };   // lanes per pixel, pixels per pass, workgroup size
__host__ __device__ inline Lanes lanes_of(int C) {
    Lanes l;
    l.tpp = C / 4;
    l.ppp = l.tpp >= BK_THREADS ? 1 : BK_THREADS / l.tpp;
    l.threads = l.tpp * l.ppp;
    return l;
}

__device__ __forceinline__ float sigmoid_acc(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---- cast + column sums -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BK_THREADS) void cast_bias_kernel(const float* __restrict__ dy, bf16_t* __restrict__ dy16, double* __restrict__ part,
                                                               long long rows, int C, int chunk_rows) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* red = (double*)smem;                               // [threads][4]
    const Lanes L = lanes_of(C);
    const int tc = threadIdx.x % L.tpp, tp = threadIdx.x / L.tpp;
    const long long r0 = (long long)blockIdx.x * chunk_rows;
    const long long r1 = r0 + chunk_rows < rows ? r0 + chunk_rows : rows;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long r = r0 + tp; r < r1; r += L.ppp) {
        const f32x4 v = __builtin_nontemporal_load((const f32x4*)(dy + r * C + tc * 4));
        if (dy16) {
            bf16x4 o;
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = (bf16_t)v[i];
            *(bf16x4*)(dy16 + r * C + tc * 4) = o;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] += (double)v[i];
    }
    if (!part) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) red[threadIdx.x * 4 + i] = s[i];
    __syncthreads();
    if (tp == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double a = 0.0;
            for (int k = 0; k < L.ppp; ++k) a += red[(k * L.tpp + tc) * 4 + i];
            part[(long long)blockIdx.x * C + tc * 4 + i] = a;
        }
    }
}

// out[c] = sum over the nparts rows of part[nparts][ncols] (fp64): 16 strided row sums per column, added in row order
__global__ __launch_bounds__(BK_THREADS) void colsum_finish_kernel(const double* __restrict__ part, int nparts, int ncols, float* __restrict__ out) {
    __shared__ double red[BK_FIN_ROWS][BK_FIN_ROWS];
    const int r = threadIdx.x >> 4, cl = threadIdx.x & 15, c = blockIdx.x * BK_FIN_ROWS + cl;
    double a = 0.0;
    if (c < ncols)
        for (int k = r; k < nparts; k += BK_FIN_ROWS) a += part[(long long)k * ncols + c];
    red[r][cl] = a;
    __syncthreads();
    if (r == 0 && c < ncols) {
        double t = 0.0;
        for (int k = 0; k < BK_FIN_ROWS; ++k) t += red[k][cl];
        out[c] = (float)t;
    }
}

// ---- weights of the data gradient -------------------------------------------------------------------------------------------------------------
__global__ void pack_dgrad_kernel(const float* __restrict__ w, bf16_t* __restrict__ dst, int Cin, int Cout, int taps) {
    const long long n = (long long)Cout * Cin * taps;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;       // over dst [Cin][taps][Cout]
    if (idx >= n) return;
    const int co = (int)(idx % Cout);
    const int tap = (int)((idx / Cout) % taps);
    const int ci = (int)(idx / ((long long)Cout * taps));
    dst[idx] = (bf16_t)w[((long long)co * Cin + ci) * taps + (taps - 1 - tap)];
}

// ---- GroupNorm statistics as (mean, rstd) -----------------------------------------------------------------------------------------------------
// pass: part[b][chunk][c][2] = (sum x, sum x^2) over the chunk's pixels, in fp64 (x is fp32: the squares are exact, and E[x^2] - mean^2 in fp64 keeps
// 53 - 2 log2(|mean| / std) bits -- 33 at |mean| = 1000 std, where the fp32 input itself has lost 10 of its 24)
__global__ __launch_bounds__(BK_THREADS) void gn_stats64_kernel(const float* __restrict__ x, double* __restrict__ part, int HW, int C, int chunk_pix, int nchunks) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* red = (double*)smem;                               // [threads][8]
    const Lanes L = lanes_of(C);
    const int b = blockIdx.y, chunk = blockIdx.x;
    const int tc = threadIdx.x % L.tpp, tp = threadIdx.x / L.tpp;
    const int p0 = chunk * chunk_pix, p1 = min(HW, p0 + chunk_pix);
    const long long base = (long long)b * HW * C + tc * 4;
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    for (int p = p0 + tp; p < p1; p += L.ppp) {
        const f32x4 xv = *(const f32x4*)(x + base + (long long)p * C);
#pragma unroll
        for (int i = 0; i < 4; ++i) { const double v = (double)xv[i]; s1[i] += v; s2[i] += v * v; }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) { red[threadIdx.x * 8 + 2 * i] = s1[i]; red[threadIdx.x * 8 + 2 * i + 1] = s2[i]; }
    __syncthreads();
    if (tp == 0) {
        double* o = part + (((long long)b * nchunks + chunk) * C + tc * 4) * 2;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            double a = 0.0;
            for (int k = 0; k < L.ppp; ++k) a += red[(k * L.tpp + tc) * 8 + i];
            o[i] = a;
        }
    }
}

// one wave per (image, group): lane l adds the (chunk, channel of the group) partials l, l + 64, ...; xor trees give every lane the same sums
__global__ __launch_bounds__(64) void gn_stats64_finish_kernel(const double* __restrict__ part, int nchunks, int HW, int C, int groups, float eps,
                                                               float* __restrict__ stats) {
    const int g = blockIdx.x, b = blockIdx.y, lane = threadIdx.x, cpg = C / groups;
    double s = 0.0, q = 0.0;
    for (int i = lane; i < nchunks * cpg; i += 64) {
        const double* t = part + (((long long)b * nchunks + i / cpg) * C + g * cpg + i % cpg) * 2;
        s += t[0]; q += t[1];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); q += __shfl_xor(q, o, 64); }
    if (lane == 0) {
        const double n = (double)cpg * (double)HW, mean = s / n, var = fmax(q / n - mean * mean, 0.0);
        float* o = stats + ((long long)b * groups + g) * 2;
        o[0] = (float)mean;
        o[1] = (float)(1.0 / sqrt(var + (double)eps));
    }
}

// ---- GroupNorm + SiLU backward ----------------------------------------------------------------------------------------------------------------
// xh = (x - mean) * rstd, u = gamma * xh + beta, s = sigmoid(u), du = da * s * (1 + u * (1 - s))
struct GnLane { float g[4], bt[4], mean[4], rstd[4]; };
__device__ __forceinline__ GnLane gn_lane(const float* stats, const float* gamma, const float* beta, int b, int c, int groups, int cpg) {
    GnLane l;
    const f32x4 gg = *(const f32x4*)(gamma + c), bb = *(const f32x4*)(beta + c);
#pragma unroll
    for (int i = 0; i < 4; ++i) { l.g[i] = gg[i]; l.bt[i] = bb[i]; }
    // 4 aligned channels lie in one group (cpg 4, 8 or 16) or in two, two channels each (cpg 2)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float* st = stats + ((long long)b * groups + (c + 2 * h) / cpg) * 2;
        l.mean[2 * h] = l.mean[2 * h + 1] = st[0]; l.rstd[2 * h] = l.rstd[2 * h + 1] = st[1];
    }
    return l;
}
// (SILU = false: the plain GroupNorm of the attention block, du = da)
template <bool SILU>
__device__ __forceinline__ void gn_du(const GnLane& l, const f32x4& x, const f32x4& da, float (&xh)[4], float (&du)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        xh[i] = (x[i] - l.mean[i]) * l.rstd[i];
        if constexpr (!SILU) { du[i] = da[i]; continue; }
        const float u = fmaf(l.g[i], xh[i], l.bt[i]);
        const float s = sigmoid_acc(u);
        du[i] = da[i] * s * (1.0f + u * (1.0f - s));
    }
}

// pass 1: part[b][chunk][c][2] = (sum du, sum du * xh) over the chunk's pixels
template <bool SILU>
__global__ __launch_bounds__(BK_THREADS) void gn_bwd_partials_kernel(const float* __restrict__ x, const float* __restrict__ stats, const float* __restrict__ gamma,
                                                                     const float* __restrict__ beta, const float* __restrict__ da, double* __restrict__ part,
                                                                     int HW, int C, int groups, int chunk_pix, int nchunks) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* red = (double*)smem;                               // [threads][8]
    const Lanes L = lanes_of(C);
    const int b = blockIdx.y, chunk = blockIdx.x;
    const int tc = threadIdx.x % L.tpp, tp = threadIdx.x / L.tpp;
    const GnLane l = gn_lane(stats, gamma, beta, b, tc * 4, groups, C / groups);
    const int p0 = chunk * chunk_pix, p1 = min(HW, p0 + chunk_pix);
    const long long base = (long long)b * HW * C + tc * 4;
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    for (int p = p0 + tp; p < p1; p += L.ppp) {
        const f32x4 xv = *(const f32x4*)(x + base + (long long)p * C), dv = *(const f32x4*)(da + base + (long long)p * C);
        float xh[4], du[4];
        gn_du<SILU>(l, xv, dv, xh, du);
#pragma unroll
        for (int i = 0; i < 4; ++i) { s1[i] += (double)du[i]; s2[i] += (double)du[i] * (double)xh[i]; }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) { red[threadIdx.x * 8 + 2 * i] = s1[i]; red[threadIdx.x * 8 + 2 * i + 1] = s2[i]; }
    __syncthreads();
    if (tp == 0) {
        double* o = part + (((long long)b * nchunks + chunk) * C + tc * 4) * 2;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            double a = 0.0;
            for (int k = 0; k < L.ppp; ++k) a += red[(k * L.tpp + tc) * 8 + i];
            o[i] = a;
        }
    }
}

// finish 1, one workgroup per (16 channels, image): S[b][c][2] = the chunk sums, 16 strided sums added in order; then the two group means
// gm[b][g] = (sum_c gamma_c S1, sum_c gamma_c S2) / (cpg * HW) of the groups these 16 channels hold
__global__ __launch_bounds__(BK_THREADS) void gn_bwd_finish_kernel(const double* __restrict__ part, const float* __restrict__ gamma, double* __restrict__ S,
                                                                   float* __restrict__ gm, int HW, int C, int groups, int nchunks) {
    __shared__ double red[BK_FIN_ROWS][BK_FIN_ROWS][2];
    __shared__ double tot[BK_FIN_ROWS][2];
    const int b = blockIdx.y, r = threadIdx.x >> 4, cl = threadIdx.x & 15, c = blockIdx.x * BK_FIN_ROWS + cl;
    double a1 = 0.0, a2 = 0.0;
    for (int k = r; k < nchunks; k += BK_FIN_ROWS) {
        const double* t = part + (((long long)b * nchunks + k) * C + c) * 2;
        a1 += t[0]; a2 += t[1];
    }
    red[r][cl][0] = a1; red[r][cl][1] = a2;
    __syncthreads();
    if (r == 0) {
        double t1 = 0.0, t2 = 0.0;
        for (int k = 0; k < BK_FIN_ROWS; ++k) { t1 += red[k][cl][0]; t2 += red[k][cl][1]; }
        tot[cl][0] = t1; tot[cl][1] = t2;
        double* o = S + ((long long)b * C + c) * 2;
        o[0] = t1; o[1] = t2;
    }
    __syncthreads();
    const int cpg = C / groups;
    if ((int)threadIdx.x < BK_FIN_ROWS / cpg) {
        const int gl = threadIdx.x;
        double m1 = 0.0, m2 = 0.0;
        for (int k = 0; k < cpg; ++k) {
            const double gk = (double)gamma[blockIdx.x * BK_FIN_ROWS + gl * cpg + k];
            m1 += gk * tot[gl * cpg + k][0]; m2 += gk * tot[gl * cpg + k][1];
        }
        const double inv = 1.0 / ((double)cpg * (double)HW);
        float* o = gm + ((long long)b * groups + (blockIdx.x * BK_FIN_ROWS) / cpg + gl) * 2;
        o[0] = (float)(m1 * inv); o[1] = (float)(m2 * inv);
    }
}

// finish 2: dbeta[c] = sum_b S[b][c][0], dgamma[c] = sum_b S[b][c][1], images in order
__global__ void gn_bwd_params_kernel(const double* __restrict__ S, float* __restrict__ dgamma, float* __restrict__ dbeta, int B, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double a1 = 0.0, a2 = 0.0;
    for (int b = 0; b < B; ++b) { a1 += S[((long long)b * C + c) * 2]; a2 += S[((long long)b * C + c) * 2 + 1]; }
    if (dbeta) dbeta[c] = (float)a1;
    if (dgamma) dgamma[c] = (float)a2;
}

// pass 2: dx = rstd * (gamma du - m1 - xh m2) (+ dx_add), and its bf16 copy
template <bool SILU>
__global__ __launch_bounds__(BK_THREADS) void gn_bwd_dx_kernel(const float* __restrict__ x, const float* __restrict__ stats, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, const float* __restrict__ da, const float* __restrict__ gm,
                                                               const float* __restrict__ dx_add, float* __restrict__ dx, bf16_t* __restrict__ dx16, int HW, int C,
                                                               int groups, int pix_per_block) {
    const Lanes L = lanes_of(C);
    const int b = blockIdx.y;
    const int tc = threadIdx.x % L.tpp, tp = threadIdx.x / L.tpp;
    const int cpg = C / groups;
    const GnLane l = gn_lane(stats, gamma, beta, b, tc * 4, groups, cpg);
    float m1[4], m2[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float* m = gm + ((long long)b * groups + (tc * 4 + 2 * h) / cpg) * 2;
        m1[2 * h] = m1[2 * h + 1] = m[0]; m2[2 * h] = m2[2 * h + 1] = m[1];
    }
    const int p0 = blockIdx.x * pix_per_block, p1 = min(HW, p0 + pix_per_block);
    const long long base = (long long)b * HW * C + tc * 4;
    for (int p = p0 + tp; p < p1; p += L.ppp) {
        const long long o = base + (long long)p * C;
        const f32x4 xv = *(const f32x4*)(x + o), dv = *(const f32x4*)(da + o);
        float xh[4], du[4];
        gn_du<SILU>(l, xv, dv, xh, du);
        f32x4 r;
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = l.rstd[i] * (l.g[i] * du[i] - m1[i] - xh[i] * m2[i]);
        if (dx_add) r += *(const f32x4*)(dx_add + o);
        *(f32x4*)(dx + o) = r;
        if (dx16) {
            bf16x4 h;
#pragma unroll
            for (int i = 0; i < 4; ++i) h[i] = (bf16_t)r[i];
            *(bf16x4*)(dx16 + o) = h;
        }
    }
}

// ---- the resampling layers' literal routes ---------------------------------------------------------------------------------
// Downsample2D: y[i][j] is the stride-1 pad-1 conv's output at (2i + 1, 2j + 1), so its data gradient is the stride-1 one of dy scattered there
__global__ __launch_bounds__(256) void scatter_odd_kernel(const uint4* __restrict__ dy, uint4* __restrict__ out, int H, int W, int C8, long long n) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;       // over out [B][H][W][C8]
    if (idx >= n) return;
    const int c = (int)(idx % C8);
    long long p = idx / C8;
    const int X = (int)(p % W); p /= W;
    const int Y = (int)(p % H);
    const long long b = p / H;
    const int Ho = H / 2, Wo = W / 2;
    uint4 v = uint4{0u, 0u, 0u, 0u};
    if ((Y & 1) && (X & 1)) v = dy[((b * Ho + (Y >> 1)) * Wo + (X >> 1)) * C8 + c];     // (Y odd and < H: Y >> 1 < Ho)
    out[idx] = v;
}

// Upsample2D: the four high-resolution gradients of a low-resolution pixel, added in a fixed order
__global__ __launch_bounds__(256) void sum2x2_kernel(const f32x4* __restrict__ t, const f32x4* __restrict__ dx_add, f32x4* __restrict__ dx, int h, int w, int C4,
                                                     long long n) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;       // over dx [B][h][w][C4]
    if (idx >= n) return;
    const int c = (int)(idx % C4);
    long long p = idx / C4;
    const int j = (int)(p % w); p /= w;
    const int i = (int)(p % h);
    const long long b = p / h;
    const long long r0 = ((b * 2 * h + 2 * i) * 2 * w + 2 * j) * C4 + c, r1 = r0 + (long long)2 * w * C4;
    f32x4 s = t[r0];
    s += t[r0 + C4];
    s += t[r1];
    s += t[r1 + C4];
    if (dx_add) s += dx_add[idx];
    dx[idx] = s;
}

int gn_bwd_chunks(int HW, int C) { const int cp = lanes_of(C).ppp * BK_PASSES; return (HW + cp - 1) / cp; }
size_t up16(size_t v) { return (v + 15) / 16 * 16; }

}  // namespace

bool vt_cast_bias_supported(int C) {
    return C >= 4 && (C % 4) == 0 && C <= 4 * BK_THREADS;       // (a workgroup is C / 4 lanes x as many pixels as fit in 256 threads)
}

int vt_cast_bias_chunks(long long rows, int C) {
    if (rows <= 0 || !vt_cast_bias_supported(C)) return 0;
    const long long cr = (long long)lanes_of(C).ppp * BK_PASSES;
    const long long n = (rows + cr - 1) / cr;
    return n > 0x7fffffffLL ? 0 : (int)n;
}

hipError_t vt_launch_cast_bias_grad(const float* dy, bf16_t* dy16, float* dbias, long long rows, int C, double* part, hipStream_t s) {
    const int chunks = vt_cast_bias_chunks(rows, C);
    if (!dy || (!dy16 && !dbias) || chunks <= 0 || (dbias && !part)) return hipErrorInvalidValue;
    const Lanes L = lanes_of(C);
    hipLaunchKernelGGL(cast_bias_kernel, dim3(chunks), dim3(L.threads), (size_t)L.threads * 4 * sizeof(double), s, dy, dy16, dbias ? part : nullptr, rows, C,
                       L.ppp * BK_PASSES);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !dbias) return e;
    hipLaunchKernelGGL(colsum_finish_kernel, dim3((C + BK_FIN_ROWS - 1) / BK_FIN_ROWS), dim3(BK_THREADS), 0, s, part, chunks, C, dbias);
    return hipGetLastError();
}

hipError_t vt_launch_pack_dgrad_weights(const float* w_oihw, bf16_t* dst, int Cin, int Cout, int ksize, hipStream_t s) {
    const long long n = (long long)Cout * Cin * ksize * ksize;
    if (!w_oihw || !dst || n <= 0 || (ksize != 1 && ksize != 3) || (n + 255) / 256 > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pack_dgrad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w_oihw, dst, Cin, Cout, ksize * ksize);
    return hipGetLastError();
}

hipError_t vt_launch_scatter_odd_nhwc16(const void* dy16, void* out16, int B, int H, int W, int C, hipStream_t s) {
    if (!dy16 || !out16 || B <= 0 || H < 2 || W < 2 || C <= 0 || (C % 8)) return hipErrorInvalidValue;
    const long long n = (long long)B * H * W * (C / 8);
    if ((n + 255) / 256 > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scatter_odd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const uint4*)dy16, (uint4*)out16, H, W, C / 8, n);
    return hipGetLastError();
}

hipError_t vt_launch_sum2x2_f32(const float* t, const float* dx_add, float* dx, int B, int h, int w, int C, hipStream_t s) {
    if (!t || !dx || B <= 0 || h <= 0 || w <= 0 || C <= 0 || (C % 4)) return hipErrorInvalidValue;
    const long long n = (long long)B * h * w * (C / 4);
    if ((n + 255) / 256 > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sum2x2_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const f32x4*)t, (const f32x4*)dx_add, (f32x4*)dx, h, w, C / 4, n);
    return hipGetLastError();
}

bool vt_gn_silu_bwd_supported(int C, int groups) {
    if (C <= 0 || groups <= 0 || C % groups || C > 1024) return false;
    const int cpg = C / groups;
    if (cpg != 2 && cpg != 4 && cpg != 8 && cpg != 16) return false;
    return (C % BK_FIN_ROWS) == 0 && (BK_THREADS % (C / 4)) == 0;
}

size_t vt_gn_stats64_ws_bytes(int B, int HW, int C) {
    if (B <= 0 || HW <= 0 || C < 16 || (C % 16) || C > 1024) return 0;
    return up16((size_t)B * gn_bwd_chunks(HW, C) * C * 2 * sizeof(double));
}

hipError_t vt_launch_gn_stats64(const float* x, int B, int HW, int C, int groups, float eps, float* stats, void* ws, hipStream_t s) {
    if (!x || !stats || !ws || B <= 0 || HW <= 0 || groups > 64 || !vt_gn_silu_bwd_supported(C, groups)) return hipErrorInvalidValue;
    const Lanes L = lanes_of(C);
    const int nchunks = gn_bwd_chunks(HW, C);
    hipLaunchKernelGGL(gn_stats64_kernel, dim3(nchunks, B), dim3(L.threads), (size_t)L.threads * 8 * sizeof(double), s, x, (double*)ws, HW, C, L.ppp * BK_PASSES, nchunks);
    hipLaunchKernelGGL(gn_stats64_finish_kernel, dim3(groups, B), dim3(64), 0, s, (const double*)ws, nchunks, HW, C, groups, eps, stats);
    return hipGetLastError();
}

size_t vt_gn_silu_bwd_ws_bytes(int B, int HW, int C) {
    if (B <= 0 || HW <= 0 || C < 16 || (C % 16) || C > 1024) return 0;
    return up16((size_t)B * gn_bwd_chunks(HW, C) * C * 2 * sizeof(double)) + up16((size_t)B * C * 2 * sizeof(double)) + up16((size_t)B * 64 * 2 * sizeof(float));
}

template <bool SILU>
static hipError_t launch_gn_backward(const float* x, const float* stats, const float* gamma, const float* beta, const float* da, const float* dx_add,
                                     float* dx, bf16_t* dx16, float* dgamma, float* dbeta, int B, int HW, int C, int groups, void* ws, hipStream_t s) {
    if (!x || !stats || !gamma || !beta || !da || !dx || !ws || B <= 0 || HW <= 0 || groups > 64 || !vt_gn_silu_bwd_supported(C, groups)) return hipErrorInvalidValue;
    const Lanes L = lanes_of(C);
    const int nchunks = gn_bwd_chunks(HW, C);
    char* p = (char*)ws;
    double* part = (double*)p; p += up16((size_t)B * nchunks * C * 2 * sizeof(double));
    double* S = (double*)p; p += up16((size_t)B * C * 2 * sizeof(double));
    float* gm = (float*)p;
    hipLaunchKernelGGL(gn_bwd_partials_kernel<SILU>, dim3(nchunks, B), dim3(L.threads), (size_t)L.threads * 8 * sizeof(double), s, x, stats, gamma, beta, da, part, HW, C,
                       groups, L.ppp * BK_PASSES, nchunks);
    hipLaunchKernelGGL(gn_bwd_finish_kernel, dim3(C / BK_FIN_ROWS, B), dim3(BK_THREADS), 0, s, part, gamma, S, gm, HW, C, groups, nchunks);
    if (dgamma || dbeta) hipLaunchKernelGGL(gn_bwd_params_kernel, dim3((C + 255) / 256), dim3(256), 0, s, S, dgamma, dbeta, B, C);
    const int ppb = L.ppp * 4;
    hipLaunchKernelGGL(gn_bwd_dx_kernel<SILU>, dim3((HW + ppb - 1) / ppb, B), dim3(L.threads), 0, s, x, stats, gamma, beta, da, gm, dx_add, dx, dx16, HW, C, groups, ppb);
    return hipGetLastError();
}

hipError_t vt_launch_gn_silu_backward(const float* x, const float* stats, const float* gamma, const float* beta, const float* da, const float* dx_add,
                                      float* dx, bf16_t* dx16, float* dgamma, float* dbeta, int B, int HW, int C, int groups, void* ws, hipStream_t s) {
    return launch_gn_backward<true>(x, stats, gamma, beta, da, dx_add, dx, dx16, dgamma, dbeta, B, HW, C, groups, ws, s);
}

hipError_t vt_launch_gn_backward(const float* x, const float* stats, const float* gamma, const float* beta, const float* da, const float* dx_add,
                                 float* dx, bf16_t* dx16, float* dgamma, float* dbeta, int B, int HW, int C, int groups, void* ws, hipStream_t s) {
    return launch_gn_backward<false>(x, stats, gamma, beta, da, dx_add, dx, dx16, dgamma, dbeta, B, HW, C, groups, ws, s);
}
