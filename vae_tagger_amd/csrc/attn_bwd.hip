// Backward of the VAE mid-block attention core (1 head, d = 512): dq, dk, dv on the two skeletons of the forward.
//
// attn_bwd_qk_kernel is attn_qk.hip's skeleton -- a wave keeps 32 rows x 512 of one operand in registers, the other operand's rows stream through
// LDS in tiles of 64 -- with three new epilogues, all of which leave bf16 pieces in the MFMA fragment order attn_pv.hip consumes:
//   mode 0  rows = do16, streamed = v16: the accumulators are dp; the epilogue loads the softmax numerators of the same (32-row slab, 64-key tile)
//           -- in fragment order they have exactly the lane layout the epilogue holds -- and stores ds = alpha * num * invsum_i * (dp - D_i);
//   mode 1  rows = k16, streamed = q16: p^T = exp(alpha k.q - c_col) / sum_col, the shift and the sum now per STREAMED row (one fused exponent
//           offset per column, loaded per tile);
//   mode 2  rows = v16, streamed = do16: the epilogue loads p^T and stores ds^T = alpha * p^T * (dp^T - D_col).
// attn_bwd_pv_kernel is attn_pv.hip's skeleton with a gradient epilogue: fp32 stores (plus an optional bf16 copy), no row normalisation.
// What the two skeletons share with the forward in a form that leaves every kernel's code alone is in vt_attn.h (the tile decodes, the x^T
// staging, the fragment-order pieces, the grid rule); the resident-slab load, the bf16 tile staging and both MFMA rings are still written
// out here as in attn_qk.hip / attn_pv.hip, and have to be kept in step by hand (DESIGN.md section 4.28 says which forms were tried).
// The kernels are separate instantiations in a separate unit.  No atomics; every output element is written by
// exactly one lane from a fixed-order accumulation, so results are bit-identical from run to run and independent of the batch, of the image
// group and of how a sweep is split over workgroups (the split only decides which workgroup runs a tile's epilogue).
#include <hip/hip_runtime.h>

#include "vt_attn.h"

using namespace vt_attn;          // QB = 256 resident rows per workgroup, D = 512
using namespace vt_attn::b16;     // KT = 64 streamed rows per LDS tile, KROWB / KBUF, ROWB, PT_TILE

namespace {

template <int BM>
__global__ __launch_bounds__(512, 2) void attn_bwd_qk_kernel(const AttnBwdQkArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];     // 2 tiles of the streamed operand
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fr = lane & 15, fq = lane >> 4;
    const VtAttnQkTile t = vt_attn_qk_tile(a.S, a.nsplit);
    const int b = t.b, ksp = t.ksp, nsplit = t.nsplit;
    const bf16_t* qb = a.rows + (long long)b * a.r_bs;
    const bf16_t* kb = a.str + (long long)b * a.s_bs;
    const int nkeys = a.S;
    const int row0 = t.row0(wave);
    const bool slab_on = row0 < a.S;                               // (wave-uniform) this wave's slab holds at least one real row

    // ---- this wave's resident slab: B operand of k-step ks for row tile j = rows[row0 + 16 j + fr][32 ks + 8 fq .. +8]
    bf16x8 qf[2][16];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int row = row0 + j * 16 + fr;
        const bf16_t* src = row < a.S ? qb + (long long)row * a.ldr + fq * 8 : (const bf16_t*)a.zeros;
        const int step = row < a.S ? 32 : 0;
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) qf[j][ks] = *(const bf16x8*)(src + ks * step);
    }
    float rs[2], rd[2];                                 // per resident row: the factor of the stored value (0 on padding rows), and D_i (mode 0)
    bool rok[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int row = row0 + j * 16 + fr;
        rok[j] = row < a.S;
        const long long vi = (long long)b * a.vec_bs + row;
        if (BM == 0) { rs[j] = rok[j] ? a.rowscale[vi] * a.alpha : 0.f; rd[j] = rok[j] ? a.rowd[vi] : 0.f; }
        else { rs[j] = rok[j] ? (BM == 2 ? a.alpha : 1.f) : 0.f; rd[j] = 0.f; }
    }
    const float alpha2 = a.alpha * 1.44269504f;

    // ---- tile staging and fragment addressing: attn_qk.hip's (one wave-instruction = one streamed row, chunks swizzled by the LDS row)
    auto stage = [&](int kt, int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            const int R = wave * 8 + jj;
            const int key = kt * KT + 32 * ((R >> 5) & 1) + 8 * ((R >> 2) & 3) + 4 * ((R >> 4) & 1) + (R & 3);
            const void* src = key < nkeys ? (const void*)(kb + (long long)key * a.lds + ((lane ^ (R & 15)) << 3)) : a.zeros;
            __builtin_amdgcn_global_load_lds(VT_GLOBAL_PTR(src), VT_LDS_PTR(smem + buf * KBUF + R * KROWB), 16, 0, 0);
        }
    };
    int kbase[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) kbase[m] = fr * KROWB + (((((m ^ (fr >> 2)) & 3) << 2) | ((fq ^ fr) & 3)) << 4);

    f32x4 acc[4][2];
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

    // the pieces of this wave's (slab, tile): piece (j, h) of lane (fq, fr) = resident row 16 j + fr, streamed rows 32 h + 8 fq .. + 7
    bf16x8 pin[2][2] = {};
    const long long pbase = (long long)b * a.p_bs + (long long)(row0 >> 5) * vt_attn_pt_slab_stride(a.S) + lane * 8;
    auto load_pin = [&](int kt) __attribute__((always_inline)) {
        if constexpr (BM == 1) return;
        if (!slab_on) return;
        vt_attn_frag_load(pin, a.Pin + pbase + (long long)kt * PT_TILE);
    };
    auto epilogue = [&](int kt) __attribute__((always_inline)) {
        const int key0 = kt * KT + 8 * fq;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float cv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if constexpr (BM != 0) {                   // per streamed row: the fused exponent offset (mode 1) or D (mode 2); vec_bs covers the last tile
                const float* cp = a.colv + (long long)b * a.vec_bs + key0 + 32 * h;
                const f32x4 c0 = *(const f32x4*)cp, c1 = *(const f32x4*)(cp + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) { cv[e] = c0[e]; cv[4 + e] = c1[e]; }
            }
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float av = acc[2 * h + (e >> 2)][j][e & 3];
                    float val;
                    if constexpr (BM == 1) {
                        const bool real = key0 + 32 * h + e < nkeys;
                        const float ex = __builtin_amdgcn_exp2f(fmaf(av, alpha2, -cv[e]));
                        val = (real && rok[j]) ? ex : 0.f;
                    } else if constexpr (BM == 0) {
                        val = (float)pin[j][h][e] * rs[j] * (av - rd[j]);
                    } else {
                        val = (float)pin[j][h][e] * rs[j] * (av - cv[e]);
                    }
                    pin[j][h][e] = (bf16_t)val;
                }
        }
        if (slab_on) vt_attn_frag_store(a.Pout + pbase + (long long)kt * PT_TILE, pin);
    };

    // waves w and w + 4 share a SIMD: one half runs its epilogue behind its MFMAs, the other in front of them (attn_qk.hip)
    const bool late = (wave & 4) != 0;
    const int nkt_all = (nkeys + KT - 1) / KT;
    const int kt0 = (int)((long long)ksp * nkt_all / nsplit), nkt = (int)((long long)(ksp + 1) * nkt_all / nsplit);
    if (nkt <= kt0) return;                                        // (workgroup-uniform)
    stage(kt0, kt0 & 1);
    for (int kt = kt0; kt < nkt; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // this wave's rows of tile kt (and its pieces, and its stores) have landed ...
        __builtin_amdgcn_s_barrier();                              // ... everyone's; and everyone has READ tile kt - 1
        asm volatile("" ::: "memory");
        if (late) {
            if (kt + 1 < nkt) stage(kt + 1, (kt + 1) & 1);
            if (kt > kt0) epilogue(kt - 1);
        }
        load_pin(kt);                                              // in flight during the MFMAs
        const char* ks_base = smem + (kt & 1) * KBUF;
        constexpr int AHEAD = 6;
        bf16x8 kf[8];
        auto frag = [&](int idx) __attribute__((always_inline)) {
            const int ks = idx >> 2, i = idx & 3;
            return *(const bf16x8*)(ks_base + kbase[ks & 3] + (ks >> 2) * 256 + i * 16 * KROWB);
        };
#pragma unroll
        for (int p = 0; p < AHEAD; ++p) kf[p] = frag(p);
#pragma unroll
        for (int idx = 0; idx < 64; ++idx) {
            if (idx + AHEAD < 64) kf[(idx + AHEAD) & 7] = frag(idx + AHEAD);
            const int ks = idx >> 2, i = idx & 3;
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[idx & 7], qf[j][ks], ks == 0 ? zero4 : acc[i][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (!late) {
            if (kt + 1 < nkt) stage(kt + 1, (kt + 1) & 1);
            epilogue(kt);
        }
    }
    if (late) epilogue(nkt - 1);
}

// ---- the gradient P.V: out[q][c] = sum_k P[q][k] x^T[c][k], fp32 (+ bf16 copy) ---------------------------------------------------------------
template <int CB>
__global__ __launch_bounds__(512, 2) void attn_bwd_pv_kernel(const AttnBwdPvArgs a) {
    constexpr int VBUF = CB * ROWB;
    constexpr int NCT = CB / 16;
    extern __shared__ __attribute__((aligned(16))) char smem[];     // 2 x^T tiles
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fr = lane & 15, fq = lane >> 4;
    const VtAttnPvTile t = vt_attn_pv_tile<CB>(a.S, wave);
    const int cb = t.cb, b = t.b, slab = t.slab;
    const int nkt = (a.S + KT - 1) / KT;
    const bf16_t* pt = vt_attn_frag_base(a.Pt + (long long)b * a.pt_bs, a.S, t.slab_real ? slab : 0, lane);
    const bf16_t* vb = a.xt + (long long)b * a.xt_bs + (long long)cb * CB * a.ldx;
    const int ld8 = (a.S + 7) / 8 * 8;                 // keys [S, ld8) of x^T are written as zero; beyond: the zero page

    const VtAttnPvStage<CB, bf16_t> stage(vb, a.ldx, ld8, a.zeros, wave, lane);
    int foff[2];
    vt_attn_pv_foff(foff, fr, fq);

    f32x4 acc[NCT][2];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[ct][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    bf16x8 pf[2][2], pn[2][2];
    stage(smem, 0, 0);
    vt_attn_frag_load(pf, pt);
    for (int kt = 0; kt < nkt; ++kt) {
        __syncthreads();
        if (kt + 1 < nkt) {
            stage(smem, kt + 1, (kt + 1) & 1);
            vt_attn_frag_load(pn, pt + (long long)(kt + 1) * PT_TILE);
        }
        const char* vs = smem + (kt & 1) * VBUF;
        constexpr int AHEAD = 6;
        bf16x8 af[8];
        auto frag = [&](int idx) __attribute__((always_inline)) { return *(const bf16x8*)(vs + (idx % NCT) * 16 * ROWB + foff[idx / NCT]); };
#pragma unroll
        for (int p = 0; p < AHEAD; ++p) af[p] = frag(p);
#pragma unroll
        for (int idx = 0; idx < 2 * NCT; ++idx) {
            if (idx + AHEAD < 2 * NCT) af[(idx + AHEAD) & 7] = frag(idx + AHEAD);
            const int h = idx / NCT, ct = idx % NCT;
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[ct][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[idx & 7], pf[j][h], acc[ct][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (kt + 1 < nkt) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int h = 0; h < 2; ++h) pf[j][h] = pn[j][h];
        }
    }
    // ---- epilogue: lane (fq, fr) holds, for row 16 j + fr of its slab and every 64-channel group G, the 16 consecutive channels
    // 64 G + 16 fq + 4 i + r (tile ct = 4 G + i, register r): four 16-B fp32 stores per group, and two 16-B bf16 stores of the copy
    if (!t.slab_real) return;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int row = slab * 32 + j * 16 + fr;
        if (row >= a.S) continue;
        const long long off = (long long)b * a.o_bs + (long long)row * a.ldo + cb * CB + 16 * fq;
#pragma unroll
        for (int G = 0; G < CB / 64; ++G) {
#pragma unroll
            for (int i = 0; i < 4; ++i) *(f32x4*)(a.out + off + 64 * G + 4 * i) = acc[4 * G + i][j];
            if (a.out16) {
#pragma unroll
                for (int i = 0; i < 4; i += 2) {
                    bf16x8 hv;
#pragma unroll
                    for (int r = 0; r < 4; ++r) { hv[r] = (bf16_t)acc[4 * G + i][j][r]; hv[4 + r] = (bf16_t)acc[4 * G + i + 1][j][r]; }
                    *(bf16x8*)(a.out16 + off + 64 * G + 4 * i) = hv;
                }
            }
        }
    }
}

// ---- layout passes (HBM-bound, S x 512 tensors) -------------------------------------------------------------------------------------------------
// One wave per token: D = sum_c do * o (fp32, a fixed xor tree), do16 = bf16(do), 1 / row sum from the forward's four segment sums (added in
// attn_pv's order), and the fused exponent offset of the key direction c * log2(e) + log2(sum).  Rows [S, vec_bs) of the three vectors: 0.
__global__ __launch_bounds__(256) void attn_bwd_rows_kernel(const float* __restrict__ dout, const float* __restrict__ o, const float* __restrict__ shift,
                                                            const float* __restrict__ sums, long long split_stride, bf16_t* __restrict__ do16,
                                                            float* __restrict__ dvec, float* __restrict__ rinv, float* __restrict__ coff, int S, int vec_bs) {
    const int lane = threadIdx.x & 63, b = blockIdx.y;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= vec_bs) return;
    const long long vi = (long long)b * vec_bs + row;
    if (row >= S) {
        if (lane == 0) { dvec[vi] = 0.f; rinv[vi] = 0.f; coff[vi] = 0.f; }
        return;
    }
    const long long base = ((long long)b * S + row) * D + lane * 8;
    const f32x4 g0 = *(const f32x4*)(dout + base), g1 = *(const f32x4*)(dout + base + 4);
    const f32x4 o0 = *(const f32x4*)(o + base), o1 = *(const f32x4*)(o + base + 4);
    bf16x8 h;
    float acc = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) { h[e] = (bf16_t)g0[e]; h[4 + e] = (bf16_t)g1[e]; acc = fmaf(g0[e], o0[e], acc); }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = fmaf(g1[e], o1[e], acc);
    *(bf16x8*)(do16 + base) = h;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) {
        const float* ps = sums + (long long)b * S + row;
        const float sum = ((ps[0] + ps[split_stride]) + ps[2 * split_stride]) + ps[3 * split_stride];
        dvec[vi] = acc;
        rinv[vi] = 1.f / sum;
        coff[vi] = fmaf(shift[(long long)b * S + row], 1.44269504f, log2f(sum));
    }
}

// dst[c][r] = src[r][c] for a bf16 matrix of R rows x Cc columns (pitches lds, ldd; batch strides s_bs, d_bs); dst columns [R, Rpad) are written as 0
__global__ __launch_bounds__(256) void transpose16_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst, int R, int Cc, int Rpad, int lds, int ldd,
                                                          long long s_bs, long long d_bs) {
    __shared__ bf16_t tile[64][66];
    const int b = blockIdx.z, r0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const bf16_t* s = src + (long long)b * s_bs;
    bf16_t* d = dst + (long long)b * d_bs;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int r = r0 + ty * 16 + k, c = c0 + tx;
        tile[ty * 16 + k][tx] = (r < R && c < Cc) ? s[(long long)r * lds + c] : (bf16_t)0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int c = c0 + ty * 16 + k, r = r0 + tx;
        if (c < Cc && r < Rpad) d[(long long)c * ldd + r] = tile[tx][ty * 16 + k];
    }
}

__global__ void bf16_to_f32_kernel(const bf16_t* __restrict__ src, float* __restrict__ dst, long long n8) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n8) return;
    const bf16x8 v = *(const bf16x8*)(src + i * 8);
    f32x4 lo, hi;
#pragma unroll
    for (int e = 0; e < 4; ++e) { lo[e] = (float)v[e]; hi[e] = (float)v[4 + e]; }
    *(f32x4*)(dst + i * 8) = lo;
    *(f32x4*)(dst + i * 8 + 4) = hi;
}

}  // namespace

hipError_t vt_launch_bf16_to_f32(const bf16_t* src, float* dst, long long n, hipStream_t s) {
    if (!src || !dst || n <= 0 || (n % 8) || (n / 8 + 255) / 256 > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bf16_to_f32_kernel, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, s, src, dst, n / 8);
    return hipGetLastError();
}

bool vt_attn_bwd_supported(int S, int C) { return C == D && S > 0; }

hipError_t vt_launch_attn_bwd_qk(const AttnBwdQkArgs& a, hipStream_t s) {
    if (!a.rows || !a.str || !a.Pout || !a.zeros || a.batch <= 0 || !vt_attn_bwd_supported(a.S, a.C) || a.mode < 0 || a.mode > 2) return hipErrorInvalidValue;
    if ((a.ldr % 8) || (a.lds % 8) || (a.r_bs % 8) || (a.s_bs % 8) || (a.p_bs % 8) || a.ldr < D || a.lds < D) return hipErrorInvalidValue;
    if ((long long)a.S * a.ldr >= (1LL << 31) || (long long)a.S * a.lds >= (1LL << 31) || a.p_bs < vt_attn_pt_elems(a.S)) return hipErrorInvalidValue;
    const int nkt = (a.S + KT - 1) / KT;
    if ((a.vec_bs % 8) || a.vec_bs < (long long)nkt * KT) return hipErrorInvalidValue;     // the epilogue loads whole 64-row tiles of the per-row vectors
    if (a.mode == 0 ? (!a.Pin || !a.rowscale || !a.rowd) : !a.colv) return hipErrorInvalidValue;
    if (a.mode == 2 && !a.Pin) return hipErrorInvalidValue;
    const int nsp = a.nsplit > 1 ? a.nsplit : 1;
    if (nsp > nkt) return hipErrorInvalidValue;
    const long long nblk = (long long)((a.S + QB - 1) / QB) * a.batch * nsp;
    if (nblk > 0x7fffffffLL) return hipErrorInvalidValue;
    static std::atomic<unsigned long long> attr_done{0};
    hipError_t ea = vt_dynamic_smem_once(attr_done, 2 * KBUF, attn_bwd_qk_kernel<0>, attn_bwd_qk_kernel<1>, attn_bwd_qk_kernel<2>);
    if (ea != hipSuccess) return ea;
    if (a.mode == 0) hipLaunchKernelGGL(attn_bwd_qk_kernel<0>, dim3((unsigned)nblk), dim3(512), 2 * KBUF, s, a);
    else if (a.mode == 1) hipLaunchKernelGGL(attn_bwd_qk_kernel<1>, dim3((unsigned)nblk), dim3(512), 2 * KBUF, s, a);
    else hipLaunchKernelGGL(attn_bwd_qk_kernel<2>, dim3((unsigned)nblk), dim3(512), 2 * KBUF, s, a);
    return hipGetLastError();
}

hipError_t vt_launch_attn_bwd_pv(const AttnBwdPvArgs& a, hipStream_t s) {
    if (!a.Pt || !a.xt || !a.out || !a.zeros || a.batch <= 0 || !vt_attn_bwd_supported(a.S, a.C)) return hipErrorInvalidValue;
    if ((a.ldx % 8) || (a.xt_bs % 8) || (a.ldo % 8) || (a.o_bs % 8) || (a.pt_bs % 8) || a.ldo < D) return hipErrorInvalidValue;
    if (a.ldx < (a.S + 7) / 8 * 8 || (long long)a.C * a.ldx >= (1LL << 31) || a.pt_bs < vt_attn_pt_elems(a.S)) return hipErrorInvalidValue;
    const VtAttnPvGrid g = vt_attn_pv_grid(a.S, a.batch);
    if (g.nblk > 0x7fffffffLL) return hipErrorInvalidValue;
    static std::atomic<unsigned long long> attr_256{0}, attr_128{0};
    hipError_t ea = vt_dynamic_smem_once(attr_256, 2 * 256 * ROWB, attn_bwd_pv_kernel<256>);
    if (ea == hipSuccess) ea = vt_dynamic_smem_once(attr_128, 2 * 128 * ROWB, attn_bwd_pv_kernel<128>);
    if (ea != hipSuccess) return ea;
    if (g.narrow) hipLaunchKernelGGL(attn_bwd_pv_kernel<128>, dim3((unsigned)g.nblk), dim3(512), 2 * 128 * ROWB, s, a);
    else hipLaunchKernelGGL(attn_bwd_pv_kernel<256>, dim3((unsigned)g.nblk), dim3(512), 2 * 256 * ROWB, s, a);
    return hipGetLastError();
}

hipError_t vt_launch_attn_bwd_rows(const float* dout, const float* o, const float* shift, const float* sums, long long split_stride, bf16_t* do16, float* dvec,
                                   float* rinv, float* coff, int batch, int S, int vec_bs, hipStream_t s) {
    if (!dout || !o || !shift || !sums || !do16 || !dvec || !rinv || !coff || batch <= 0 || S <= 0 || vec_bs < S || batch > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(attn_bwd_rows_kernel, dim3((unsigned)((vec_bs + 3) / 4), (unsigned)batch), dim3(256), 0, s, dout, o, shift, sums, split_stride, do16, dvec, rinv,
                       coff, S, vec_bs);
    return hipGetLastError();
}

hipError_t vt_launch_transpose16(const bf16_t* src, bf16_t* dst, int R, int Cc, int Rpad, int lds, int ldd, long long s_bs, long long d_bs, int batch, hipStream_t s) {
    if (!src || !dst || R <= 0 || Cc <= 0 || Rpad < R || ldd < Rpad || lds < Cc || batch <= 0 || batch > 65535 || (Cc + 63) / 64 > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(transpose16_kernel, dim3((unsigned)((Rpad + 63) / 64), (unsigned)((Cc + 63) / 64), (unsigned)batch), dim3(256), 0, s, src, dst, R, Cc, Rpad, lds, ldd,
                       s_bs, d_bs);
    return hipGetLastError();
}
