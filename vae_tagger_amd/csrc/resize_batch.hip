// vt_resize_normalize_batch: Pillow's 8-bit two-pass resample (misc_kernels.hip: resize_h_kernel / resize_v_kernel) + ToTensor +
// Normalize (preprocess_u8_kernel) for a whole batch of images of different sizes in two launches.  The grid's z index selects the
// image; its descriptor (source pointer, crop box, where its tables and its intermediate image live) is read from the workspace.
//   pass 1 (rsb_h_kernel): crop + horizontal resample -> uint8 [crop_h][dst_w][3] per image in the workspace; the source row segment a
//           block needs is loaded once, as aligned dwords, into LDS (a crop copy when the width does not change);
//   pass 2 (rsb_v_kernel): vertical resample of that image (or a copy when the height does not change), rounded to uint8 as
//           ImagingResampleVertical_8bpc rounds it, normalised with preprocess_u8_kernel's expression and stored as fp32 NCHW
//           (and as uint8 HWC when the caller asks for it).
// Horizontal tables are stored transposed ([2 + ksize][dst_w]: the lanes of a wave read neighbouring ints); vertical ones as rs_table
// builds them (a block reads one row of the table: uniform addresses).
#include <string.h>

#include "vt_context.h"

using namespace vt;

namespace {

constexpr int RSB_PRECISION_BITS = 32 - 8 - 2;
constexpr int RSB_LDS_BYTES = 16384;           // source row segment of one block: 256 outputs x scale + 2 x support pixels, 3 B each

struct RsbDesc {
    const unsigned char* src;
    int src_h, src_w, left, top, crop_w, crop_h;
    int kh, kv;                 // coefficients per output of the horizontal / vertical pass; 0 = the pass is skipped
    int tab_h, tab_v;           // offsets (ints) of this image's tables in the table block
    long long tmp;              // offset (bytes) of this image's [crop_h][dst_w][3] intermediate in the tmp block
};

__device__ __forceinline__ int rsb_clip8(int v) {
    v >>= RSB_PRECISION_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__global__ __launch_bounds__(256) void rsb_h_kernel(const RsbDesc* __restrict__ descs, const int* __restrict__ tabs,
                                                    unsigned char* __restrict__ tmp_base, int dst_w) {
    __shared__ unsigned int seg[RSB_LDS_BYTES / 4];
    const RsbDesc d = descs[blockIdx.z];
    const int y = blockIdx.y;
    if (y >= d.crop_h) return;                                        // (block-uniform: the grid is sized by the tallest crop)
    const int x_lo = blockIdx.x * 256;
    if (x_lo >= dst_w) return;
    unsigned char* out = tmp_base + d.tmp + (long long)y * dst_w * 3;
    const unsigned char* row = d.src + ((long long)(d.top + y) * d.src_w + d.left) * 3;
    if (d.kh == 0) {                                                  // width unchanged (dst_w == crop_w): crop copy
        const int nbytes = dst_w * 3;
        for (int i = threadIdx.x; i < 768; i += 256) {
            const int b = x_lo * 3 + i;
            if (b < nbytes) out[b] = row[b];
        }
        return;
    }
    const int* T = tabs + d.tab_h;                                    // [2 + kh][dst_w]
    const int x_hi = min(x_lo + 255, dst_w - 1);
    const int s0 = T[x_lo], s1 = T[x_hi] + T[dst_w + x_hi];           // source pixels [s0, s1) cover this block's outputs (first / last are monotonic)
    const uintptr_t img0 = (uintptr_t)d.src, img1 = img0 + (size_t)d.src_h * d.src_w * 3;
    const uintptr_t a0 = (uintptr_t)row + (size_t)s0 * 3, a1 = (uintptr_t)row + (size_t)s1 * 3;
    const uintptr_t base = a0 & ~(uintptr_t)3;
    const int head = (int)(a0 - base);
    const bool staged = s1 > s0 && (a1 - base) <= (uintptr_t)RSB_LDS_BYTES;
    if (staged) {
        const int nd = (int)((a1 - base + 3) >> 2);
        for (int i = threadIdx.x; i < nd; i += 256) {
            const uintptr_t A = base + 4 * (uintptr_t)i;
            unsigned int v = 0;
            if (A >= img0 && A + 4 <= img1) v = *(const unsigned int*)A;
            else {                                                    // the dword straddles the image's first / last byte
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const uintptr_t q = A + b;
                    if (q >= img0 && q < img1) v |= (unsigned int)(*(const unsigned char*)q) << (8 * b);
                }
            }
            seg[i] = v;
        }
        __syncthreads();
    }
    const int xx = x_lo + threadIdx.x;
    if (xx >= dst_w) return;
    const int x0 = T[xx], n = T[dst_w + xx];
    int c0 = 1 << (RSB_PRECISION_BITS - 1), c1 = c0, c2 = c0;
    if (staged && x0 >= s0 && x0 + n <= s1) {
        const unsigned char* p = (const unsigned char*)seg + head + (x0 - s0) * 3;
        for (int k = 0; k < n; ++k) {
            const int w = T[(long long)(2 + k) * dst_w + xx];
            c0 += p[3 * k] * w; c1 += p[3 * k + 1] * w; c2 += p[3 * k + 2] * w;
        }
    } else {
        const unsigned char* p = row + (long long)x0 * 3;
        for (int k = 0; k < n; ++k) {
            const int w = T[(long long)(2 + k) * dst_w + xx];
            c0 += p[3 * k] * w; c1 += p[3 * k + 1] * w; c2 += p[3 * k + 2] * w;
        }
    }
    unsigned char* o = out + (long long)xx * 3;
    o[0] = (unsigned char)rsb_clip8(c0); o[1] = (unsigned char)rsb_clip8(c1); o[2] = (unsigned char)rsb_clip8(c2);
}

__global__ __launch_bounds__(256) void rsb_v_kernel(const RsbDesc* __restrict__ descs, const int* __restrict__ tabs,
                                                    const unsigned char* __restrict__ tmp_base, float* __restrict__ out_f,
                                                    unsigned char* __restrict__ out_u8, int dst_h, int dst_w) {
    const RsbDesc d = descs[blockIdx.z];
    const int xx = blockIdx.x * 256 + threadIdx.x, yy = blockIdx.y;
    if (xx >= dst_w) return;
    const unsigned char* in = tmp_base + d.tmp;                       // [crop_h][dst_w][3]
    int r[3];
    if (d.kv == 0) {                                                  // height unchanged (dst_h == crop_h)
        const unsigned char* p = in + ((long long)yy * dst_w + xx) * 3;
        r[0] = p[0]; r[1] = p[1]; r[2] = p[2];
    } else {
        const int* t = tabs + d.tab_v + (long long)yy * (2 + d.kv);
        const int y0 = t[0], n = t[1];
        const unsigned char* p = in + ((long long)y0 * dst_w + xx) * 3;
        int c0 = 1 << (RSB_PRECISION_BITS - 1), c1 = c0, c2 = c0;
        for (int k = 0; k < n; ++k) {
            const int w = t[2 + k];
            const unsigned char* q = p + (long long)k * dst_w * 3;
            c0 += q[0] * w; c1 += q[1] * w; c2 += q[2] * w;
        }
        r[0] = rsb_clip8(c0); r[1] = rsb_clip8(c1); r[2] = rsb_clip8(c2);
    }
    const long long HW = (long long)dst_h * dst_w, pix = (long long)yy * dst_w + xx, b = blockIdx.z;
    if (out_f) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = __fdiv_rn((float)r[c], 255.0f);           // preprocess_u8_kernel's expression
            out_f[(b * 3 + c) * HW + pix] = (v - 0.5f) / 0.5f;
        }
    }
    if (out_u8) {
        unsigned char* o = out_u8 + (b * HW + pix) * 3;
        o[0] = (unsigned char)r[0]; o[1] = (unsigned char)r[1]; o[2] = (unsigned char)r[2];
    }
}

// ---- host: the plan of one call (shared by the sizing function and the call) ---------------------------------------------------
struct RsbTable { int in, out, transposed, offset, ksize; };
struct RsbPlan {
    std::vector<RsbDesc> desc;
    std::vector<RsbTable> tables;              // the distinct tables of the call (images of one size share theirs)
    size_t desc_bytes = 0, tab_ints = 0, tmp_bytes = 0, total = 0;
    int max_crop_h = 0;
};

int rsb_table_offset(RsbPlan& p, int in, int out, int filter, int transposed, int* ksize) {
    *ksize = rs_ksize(in, out, filter);
    for (const RsbTable& t : p.tables)
        if (t.in == in && t.out == out && t.transposed == transposed) return t.offset;
    const RsbTable t{in, out, transposed, (int)p.tab_ints, *ksize};
    p.tables.push_back(t);
    p.tab_ints += (size_t)out * (2 + *ksize);
    return t.offset;
}

// false: an argument the call rejects as VT_ERR_INVALID (source pointers aside)
bool rsb_plan(const vt_resize_item* items, int B, int dst_h, int dst_w, int filter, RsbPlan& p) {
    if (!items || B <= 0 || B > 65535 || dst_h <= 0 || dst_w <= 0 || dst_h > 65535 || dst_w > (1 << 24) || (filter != 0 && filter != 1)) return false;
    p.desc.resize((size_t)B);
    for (int k = 0; k < B; ++k) {
        const vt_resize_item& it = items[k];
        if (it.src_h <= 0 || it.src_w <= 0 || it.crop_w <= 0 || it.crop_h <= 0 || it.crop_left < 0 || it.crop_top < 0 ||
            (long long)it.crop_left + it.crop_w > it.src_w || (long long)it.crop_top + it.crop_h > it.src_h || it.crop_h > 65535 ||
            it.src_w > (1 << 24))
            return false;
        RsbDesc& d = p.desc[(size_t)k];
        d.src = it.src_hwc; d.src_h = it.src_h; d.src_w = it.src_w; d.left = it.crop_left; d.top = it.crop_top; d.crop_w = it.crop_w; d.crop_h = it.crop_h;
        d.kh = d.kv = 0; d.tab_h = d.tab_v = 0;
        if (it.crop_w != dst_w) d.tab_h = rsb_table_offset(p, it.crop_w, dst_w, filter, 1, &d.kh);
        if (it.crop_h != dst_h) d.tab_v = rsb_table_offset(p, it.crop_h, dst_h, filter, 0, &d.kv);
        if (p.tab_ints > (size_t)1 << 30) return false;
        d.tmp = (long long)p.tmp_bytes;
        p.tmp_bytes += align_up((size_t)it.crop_h * dst_w * 3);
        if (it.crop_h > p.max_crop_h) p.max_crop_h = it.crop_h;
    }
    p.desc_bytes = align_up((size_t)B * sizeof(RsbDesc));
    p.total = p.desc_bytes + align_up(p.tab_ints * 4) + p.tmp_bytes;
    return true;
}

// the host table of one axis, built once per (in, out, filter, transposed) and kept by the context
const std::vector<int>& rsb_host_table(vt_context* c, const RsbTable& t, int filter) {
    const std::array<int, 4> key{t.in, t.out, filter, t.transposed};
    auto it = c->rs_tables.find(key);
    if (it != c->rs_tables.end()) return it->second;
    if (c->rs_tables.size() >= 256) c->rs_tables.clear();            // (bounded: a data set of arbitrary sizes must not grow it for ever)
    const int stride = 2 + t.ksize;
    std::vector<int> tab((size_t)t.out * stride);
    rs_table(t.in, t.out, filter, tab.data());
    if (t.transposed) {
        std::vector<int> tr(tab.size());
        for (int x = 0; x < t.out; ++x)
            for (int j = 0; j < stride; ++j) tr[(size_t)j * t.out + x] = tab[(size_t)x * stride + j];
        tab.swap(tr);
    }
    return c->rs_tables.emplace(key, std::move(tab)).first->second;
}

}  // namespace

extern "C" {

size_t vt_resize_batch_workspace_bytes(const vt_resize_item* items, int B, int dst_h, int dst_w, int filter) {
    RsbPlan p;
    if (!rsb_plan(items, B, dst_h, dst_w, filter, p)) return 0;
    return p.total + 256;
}

int vt_resize_normalize_batch(vt_context* c, const vt_resize_item* items, int B, int dst_h, int dst_w, int filter,
                              float* out_nchw, size_t out_nchw_bytes, uint8_t* out_u8_hwc, size_t out_u8_bytes,
                              void* workspace, size_t workspace_bytes, void* stream) {
    if (!c) return VT_ERR_INVALID;
    RsbPlan p;
    if (!rsb_plan(items, B, dst_h, dst_w, filter, p)) return c->fail(VT_ERR_INVALID, "vt_resize_normalize_batch: bad argument (NULL items, B, size, filter or a crop box outside its source)");
    for (int k = 0; k < B; ++k)
        if (!items[k].src_hwc) return c->fail(VT_ERR_INVALID, "vt_resize_normalize_batch: item %d has a NULL source", k);
    if (!out_nchw && !out_u8_hwc) return c->fail(VT_ERR_INVALID, "vt_resize_normalize_batch: no output buffer");
    if (!workspace) return c->fail(VT_ERR_INVALID, "vt_resize_normalize_batch: NULL workspace");
    const size_t px = (size_t)B * dst_h * dst_w * 3;
    if (out_nchw && out_nchw_bytes < px * 4)
        return c->fail(VT_ERR_WORKSPACE, "vt_resize_normalize_batch: fp32 output of %zu bytes < required %zu", out_nchw_bytes, px * 4);
    if (out_u8_hwc && out_u8_bytes < px)
        return c->fail(VT_ERR_WORKSPACE, "vt_resize_normalize_batch: uint8 output of %zu bytes < required %zu", out_u8_bytes, px);
    char* ws = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    if (workspace_bytes < p.total + (size_t)(ws - (char*)workspace))
        return c->fail(VT_ERR_WORKSPACE, "vt_resize_normalize_batch: workspace %zu < required %zu", workspace_bytes, p.total + 256);
    DeviceGuard guard(c);
    hipStream_t s = (hipStream_t)stream;
    // descriptors + tables of this call -> one pinned block of the ring -> one H2D copy in stream order
    const size_t staged = p.desc_bytes + p.tab_ints * 4;
    vt_context::RsRingSlot& sl = c->rs_ring[c->rs_ring_next++ % vt_context::RS_RING];
    if (!sl.ev) HIPCK(c, hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming), "hipEventCreate");
    else if (sl.used) HIPCK(c, hipEventSynchronize(sl.ev), "hipEventSynchronize");      // only when the ring wrapped onto a copy still in flight
    if (sl.bytes < staged) {
        if (sl.host) (void)hipHostFree(sl.host);
        sl.host = nullptr; sl.bytes = 0; sl.used = false;
        const size_t want = staged * 5 / 4 + 65536;
        HIPCK(c, hipHostMalloc(&sl.host, want, hipHostMallocDefault), "hipHostMalloc");
        sl.bytes = want;
    }
    memcpy(sl.host, p.desc.data(), (size_t)B * sizeof(RsbDesc));
    int* host_tabs = (int*)((char*)sl.host + p.desc_bytes);
    for (const RsbTable& t : p.tables) {
        const std::vector<int>& tab = rsb_host_table(c, t, filter);
        memcpy(host_tabs + t.offset, tab.data(), tab.size() * 4);
    }
    HIPCK(c, hipMemcpyAsync(ws, sl.host, staged, hipMemcpyHostToDevice, s), "hipMemcpyAsync(descriptors, tables)");
    HIPCK(c, hipEventRecord(sl.ev, s), "hipEventRecord");
    sl.used = true;
    const RsbDesc* descs = (const RsbDesc*)ws;
    const int* tabs = (const int*)(ws + p.desc_bytes);
    unsigned char* tmp = (unsigned char*)(ws + p.desc_bytes + align_up(p.tab_ints * 4));
    const unsigned gx = (unsigned)((dst_w + 255) / 256);
    hipLaunchKernelGGL(rsb_h_kernel, dim3(gx, (unsigned)p.max_crop_h, (unsigned)B), dim3(256), 0, s, descs, tabs, tmp, dst_w);
    HIPCK(c, hipGetLastError(), "vt_resize_normalize_batch (horizontal pass)");
    hipLaunchKernelGGL(rsb_v_kernel, dim3(gx, (unsigned)dst_h, (unsigned)B), dim3(256), 0, s, descs, tabs, (const unsigned char*)tmp, out_nchw,
                       (unsigned char*)out_u8_hwc, dst_h, dst_w);
    HIPCK(c, hipGetLastError(), "vt_resize_normalize_batch (vertical pass)");
    return VT_OK;
}

}  // extern "C"
