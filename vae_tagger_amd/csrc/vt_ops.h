// What the vt_op_* entries (ops.hip, ops_backward.hip, attention_backward.hip) share: the checks an entry makes before its first launch and the
// launch sequences more than one of them issues.  A new operator is written against these.
#pragma once
#include <algorithm>

#include "vt_context.h"

namespace vt {

// The caller's workspace against what `<op>_workspace_bytes` asks for; `align` is 16 or ALIGN.
inline int check_workspace(vt_context* c, const char* op, const void* ws, size_t ws_bytes, size_t need, size_t align, int code = VT_ERR_INVALID) {
    if (ws && ((uintptr_t)ws % align) == 0 && ws_bytes >= need) return VT_OK;
    return c->fail(code, "%s: workspace must be %zu-byte aligned and hold %s_workspace_bytes = %zu bytes (got %zu)", op, align, op, need, ws_bytes);
}

// Slices of a weight gradient's pixel loop: the caller's count, clamped so that every slice holds at least one step, or with 0 the shape's own.
inline int slice_count(int splits, int steps, int auto_value) { return splits <= 0 ? auto_value : std::min(splits, steps); }

// What a conv's GroupNorm epilogue takes: gamma, beta and the (scale, shift) table, 1 .. 64 groups of 4, 8 or 16 of the C output channels.
inline int check_gn_epilogue(vt_context* c, const char* op, const float* gamma, const float* beta, const float* scale_shift, int C, int groups) {
    if (!gamma || !beta || !scale_shift || groups < 1 || groups > 64 || C % groups) return c->fail(VT_ERR_INVALID, "%s: bad GroupNorm argument", op);
    const int cpg = C / groups;
    if (cpg != 4 && cpg != 8 && cpg != 16) return c->fail(VT_ERR_INVALID, "%s: channels per group must be 4, 8 or 16", op);
    return VT_OK;
}

// run_conv writes GroupNorm partials only with flag 1 on: an operator that was asked for them holds it at 1 while this lives.
struct FuseGnStats {
    vt_context* c; int saved;
    explicit FuseGnStats(vt_context* c_) : c(c_), saved(c_->fuse_gn_stats) { c->fuse_gn_stats = 1; }
    ~FuseGnStats() { c->fuse_gn_stats = saved; }
    FuseGnStats(const FuseGnStats&) = delete;
    FuseGnStats& operator=(const FuseGnStats&) = delete;
};

// The epilogue's partials -> (scale, shift); a conv that ran on a kernel without the epilogue left none.
inline int finish_gn_stats(vt_context* c, const char* op, const GnState& gn, int B, int C, int groups, float eps, const float* gamma, const float* beta,
                           float* scale_shift, hipStream_t s) {
    if (gn.parts == 0) return c->fail(VT_ERR_INVALID, "%s: this shape has no stats epilogue", op);
    HIPCK(c, vt_launch_gn_finalize(gn.partial, gn.parts, B, C, groups, eps, gamma, beta, scale_shift, s), "gn_finalize");
    return VT_OK;
}

// bf16 OHWI 3x3 weights -> the halo kernels' packing, at the start of the operator scratch (*wp)
inline int repack_halo(vt_context* c, const void* w_ohwi, int Cin, int Cout, hipStream_t s, const bf16_t** wp) {
    VTCK(c->ensure_op_scratch((size_t)Cout * 9 * Cin * 2));
    HIPCK(c, vt_launch_repack_ohwi_to_halo((const bf16_t*)w_ohwi, (bf16_t*)c->op_scratch, Cin, Cout, s), "repack");
    *wp = (const bf16_t*)c->op_scratch;
    return VT_OK;
}

}  // namespace vt
