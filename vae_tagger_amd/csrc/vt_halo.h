// What the 3x3 halo convolution kernels share: the tile-grid decode and its host half, the counted
// waits and the optimiser barriers, the fp8 fragment reads and the 16-bit stores of a lane's 16 consecutive couts.  (The
// GroupNorm-partials epilogues are in vt_common.h, which conv_gemm.hip shares.)  Everything here is a device inline, a host
// inline or a template: every kernel is still compiled in its own translation unit with its own constants.  Schedules, wait
// counts, ring depths, tile shapes and the barrier in front of an epilogue are NOT here: they are what the kernels differ in.
#pragma once
#include <utility>

#include "vt_common.h"

// ---- counted waits -----------------------------------------------------------------------------------------------------------
// s_waitcnt vmcnt(n) for a count that is a compile-time constant after unrolling at almost every call site (the count is an
// immediate of the instruction: a run-time n selects among MAXN + 1 instructions; n outside 0 .. MAXN waits for everything).
template <int K>
__device__ __forceinline__ void vt_wait_vmcnt_imm() {
    asm volatile("s_waitcnt vmcnt(%[k])" ::[k] "n"(K) : "memory");
}
// ... that also names the registers an inline-asm load wrote (one or two of them, `r`): nothing that consumes them
// can be scheduled above the wait (hipcc neither counts asm loads nor knows when their data lands).
template <int K, typename V, int N>
__device__ __forceinline__ void vt_wait_vmcnt_imm(V (&r)[N]) {
    static_assert(N == 1 || N == 2, "one or two tied registers");
    if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(%[k])" : "+v"(r[0]), "+v"(r[1]) : [k] "n"(K) : "memory");
    else asm volatile("s_waitcnt vmcnt(%[k])" : "+v"(r[0]) : [k] "n"(K) : "memory");
}
template <int... Ks, typename... R>
__device__ __forceinline__ void vt_wait_vmcnt_seq(int n, std::integer_sequence<int, Ks...>, R&... r) {
    if (!((n == Ks ? (vt_wait_vmcnt_imm<Ks>(r...), true) : false) || ...)) vt_wait_vmcnt_imm<0>(r...);
}
template <int MAXN>
__device__ __forceinline__ void vt_wait_vmcnt(int n) {
    vt_wait_vmcnt_seq(n, std::make_integer_sequence<int, MAXN + 1>{});
}
template <int MAXN, typename V, int N>
__device__ __forceinline__ void vt_wait_vmcnt_tied(int n, V (&r)[N]) {
    vt_wait_vmcnt_seq(n, std::make_integer_sequence<int, MAXN + 1>{}, r);
}

// Identity the optimiser cannot see through: stops loop-invariant address arithmetic built on `v` from being
// hoisted into (and spilled from) long-lived registers -- it is recomputed where it is used instead.
__device__ __forceinline__ int vt_opaque(int v) {
    asm volatile("" : "+v"(v));
    return v;
}
// the same for a wave-uniform value: the plane-buffer bases must not be combined with the per-lane fragment offsets into
// loop-invariant address tables (3 slots x 8 bases x 2 pitches live across the whole K loop spill)
__device__ __forceinline__ int vt_opaque_s(int v) {
    asm volatile("" : "+s"(v));
    return v;
}

// ---- fp8 operand fragments ---------------------------------------------------------------------------------------------------
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ i32x8 vt_cat8(i32x4 lo, i32x4 hi) { return i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]}; }
// 16-B chunk swizzle of the fp8 halo kernels' 64-B LDS rows: physical = logical ^ vt_swz8(row), conflict-free for rows 64 B apart
__device__ __forceinline__ int vt_swz8(int row) { return (row ^ (row >> 2)) & 3; }
// 32-byte fragment of 64-B LDS row `row`: logical chunks 2 g, 2 g + 1
__device__ __forceinline__ i32x8 vt_read_frag8(const char* base, int row, int g) {
    const int a = row * 64 + (((2 * g) ^ vt_swz8(row)) << 4);
    return vt_cat8(*(const i32x4*)(base + a), *(const i32x4*)(base + (a ^ 16)));
}

// ---- tile grid ---------------------------------------------------------------------------------------------------------------
// One workgroup per (image, pixel tile, cout tile), cout tile fastest.  The divisors are launch constants: the host passes
// 2^40 / d + 1 multipliers, so the runtime integer divisions (~50 instructions each) in front of the first DMA become multiplies.
// Host half: fills tiles_x / ctiles / per_img / ptiles and the multipliers of the launch-args copy `k`; returns the number of
// workgroups, or 0 when it is outside 1 .. 2^31 - 1 (the launcher answers hipErrorInvalidValue).
template <typename Args>
inline long long vt_halo_tile_grid(Args& k, int tiles_x, int tiles_y, int ctiles, int batch) {
    const long long tiles = (long long)tiles_x * tiles_y;
    const long long nblk = tiles * ctiles * batch;
    if (nblk <= 0 || nblk > 0x7fffffffLL) return 0;
    k.tiles_x = tiles_x; k.ctiles = ctiles; k.per_img = (int)(tiles * ctiles); k.ptiles = (int)tiles;
    // n / d = (n * m) >> 40 with m = 2^40 / d + 1 for every n < nblk: exact when n * d < 2^40; n * m must also fit 64 bits
    // (m <= 2^40 + 1, so n < 2^23).  Otherwise m = 0 and the kernel divides.
    auto magic = [&](long long d) -> unsigned long long {
        return (nblk * d < (1LL << 40) && nblk < (1LL << 23)) ? ((1ULL << 40) / (unsigned long long)d + 1ULL) : 0ULL;
    };
    k.m_per_img = magic(k.per_img); k.m_ctiles = magic(k.ctiles); k.m_tiles_x = magic(k.tiles_x);
    return nblk;
}
// Device half: this workgroup's image, pixel tile (index, row, column) and cout tile.  The column is formed where the kernel
// asks for it, after its `tyi * ROWS`: the order the kernels always had, which keeps their code what it was to the instruction.
struct VtHaloTile {
    int b, tile, ct, tyi, tiles_x;
    __device__ __forceinline__ int txi() const { return tile - tyi * tiles_x; }
};
template <typename Args>
__device__ __forceinline__ VtHaloTile vt_halo_tile_of(const Args& a) {
    auto fdiv = [](int n, unsigned long long m, int d) -> int {
        return m ? (int)(((unsigned long long)(unsigned)n * m) >> 40) : n / d;
    };
    int logical = vt_xcd_remap(blockIdx.x, gridDim.x);
    VtHaloTile t;
    t.b = fdiv(logical, a.m_per_img, a.per_img);
    logical -= t.b * a.per_img;
    t.tile = fdiv(logical, a.m_ctiles, a.ctiles);
    t.ct = logical - t.tile * a.ctiles;
    t.tyi = fdiv(t.tile, a.m_tiles_x, a.tiles_x);
    t.tiles_x = a.tiles_x;
    return t;
}

// ---- 16-bit stores of a lane's 16 consecutive couts ----------------------------------------------------------------------------
// Interleaved cout map (conv3x3_halo, conv3x3_s2_halo, conv3x3_up2): tile i / register r of acc[i][j] is cout 4 i + r of the
// lane's run, so tiles i (`lo`) and i + 1 (`hi`) make one 16-byte store at dst = run + 4 i.  T = f16_t for the fp16 activation
// stream and for an operand copy whose consumer runs on fp16 operands, bf16_t otherwise.  STORE = false is the EPI_NOSTORE timing
// experiment: the values are formed and dropped.  (The loop over i and the fp16 / bf16 choice stay in the kernels: with them in
// here, behind a reference to the accumulator array, none of the three compiles to the code it had.)
template <bool STORE = true, typename T>
__device__ __forceinline__ void vt_halo_store16(T* dst, const f32x4& lo, const f32x4& hi) {
    typedef T Tx8 __attribute__((ext_vector_type(8)));
    Tx8 h;
#pragma unroll
    for (int r = 0; r < 4; ++r) { h[r] = (T)lo[r]; h[4 + r] = (T)hi[r]; }
    if constexpr (STORE) *(Tx8*)dst = h;
    else asm volatile("" :: "v"(h));
}
// The fp8 kernels' form: the 16 registers of one 32x32 accumulator are the 16 consecutive couts.  T = f16_t or bf16_t.
template <typename T>
__device__ __forceinline__ void vt_halo_store16_f8(T* dst, const f32x16& v) {
    typedef T Tx8 __attribute__((ext_vector_type(8)));
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        Tx8 hh;
#pragma unroll
        for (int q = 0; q < 8; ++q) hh[q] = (T)v[8 * i + q];
        *(Tx8*)(dst + 8 * i) = hh;
    }
}
