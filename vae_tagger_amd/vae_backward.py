"""Backward of the VAE's blocks -- ResnetBlock2D (the block both VAE models consist of), the mid attention block, the two resampling layers
(Downsample2D's stride-2 conv and Upsample2D), and their compositions: the mid block, a down block and an up block -- on the device: thin wrappers
over the vt_op_* backward operators (include/vae_tagger_hip.h, DESIGN.md sections 4.19, 4.20 and 4.22).  Tensors are torch tensors of one HIP device,
activations NHWC ([B, H, W, C]), parameters in diffusers' own layouts (conv weights fp32 OIHW).  All gradients are fp32; every MFMA operand is bf16.
Every launch goes to torch's current stream of the tensors' device and nothing here synchronises with the host.  There is no eager fallback: a shape
an operator refuses raises VTError.

This is NOT train_vae: there is no optimiser, no loss, no CLI, no backward of conv_in and conv_out and no whole-model backward here.
"""
import ctypes

import torch

from . import _lib

GROUPS, EPS = 32, 1e-6          # ResnetBlock2D's GroupNorm in the FLUX VAE

_contexts = {}


def context(device=None):
    """The vt_context this module's functions use on `device` (default: the current one); flags set on it (vt_set_flag) apply to them."""
    idx = torch.device(device).index if device is not None else None
    if idx is None:
        idx = torch.cuda.current_device()
    if idx not in _contexts:
        _contexts[idx] = _lib.Context(idx)
    return _contexts[idx]


def _vp(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _f32(t, what):
    if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous fp32 tensor on the device")
    return t


def _bf16(t, what):
    if t.dtype != torch.bfloat16 or not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous bf16 tensor on the device")
    return t


def _workspace(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)      # (torch's allocations are 512-byte aligned)


def cast_bias_grad(dy, *, want_dy16=True, want_bias=True):
    """dy fp32 [..., C] -> (bf16 copy or None, column sums over all leading dimensions or None), one pass."""
    dy = _f32(dy, "dy")
    ctx = context(dy.device)
    C = dy.shape[-1]
    rows = dy.numel() // C
    dy16 = torch.empty(dy.shape, dtype=torch.bfloat16, device=dy.device) if want_dy16 else None
    db = torch.empty(C, dtype=torch.float32, device=dy.device) if want_bias else None
    n = ctx.lib.vt_op_cast_bias_grad_workspace_bytes(rows, C) if want_bias else 0
    ws = _workspace(n, dy.device)
    ctx.call("vt_op_cast_bias_grad", _vp(dy), _vp(dy16), _vp(db), rows, C, _vp(ws), ws.numel(), _stream(dy))
    return dy16, db


def conv_backward_data(dy16, weight, *, dx_add=None):
    """dy16 bf16 [B, H, W, Cout], weight fp32 OIHW (3x3 pad 1 or 1x1, stride 1) -> dx fp32 [B, H, W, Cin] (+ dx_add)."""
    dy16 = _bf16(dy16, "dy16")
    weight = _f32(weight, "weight")
    B, H, W, Cout = dy16.shape
    Cin, k = weight.shape[1], weight.shape[2]
    if weight.shape[0] != Cout or weight.shape[3] != k:
        raise ValueError("weight does not match dy16")
    if dx_add is not None and tuple(_f32(dx_add, "dx_add").shape) != (B, H, W, Cin):
        raise ValueError("dx_add must have dx's shape")
    dx = torch.empty(B, H, W, Cin, dtype=torch.float32, device=dy16.device)
    context(dy16.device).call("vt_op_conv_backward_data", _vp(dy16), _vp(weight), _vp(dx_add), _vp(dx), B, H, W, Cin, Cout, k, _stream(dy16))
    return dx


def conv_backward_weight(dy16, a16, ksize, *, splits=0):
    """dy16 bf16 [B, H, W, Cout], a16 bf16 [B, H, W, Cin] (the conv's forward operand) -> dW fp32 [Cout, Cin, k, k]."""
    dy16, a16 = _bf16(dy16, "dy16"), _bf16(a16, "a16")
    B, H, W, Cout = dy16.shape
    Cin = a16.shape[-1]
    if tuple(a16.shape[:3]) != (B, H, W):
        raise ValueError("a16 does not match dy16")
    ctx = context(dy16.device)
    dw = torch.empty(Cout, Cin, ksize, ksize, dtype=torch.float32, device=dy16.device)
    ws = _workspace(ctx.lib.vt_op_conv_backward_weight_workspace_bytes(B, H, W, Cin, Cout, ksize, int(splits)), dy16.device)
    ctx.call("vt_op_conv_backward_weight", _vp(dy16), _vp(a16), _vp(dw), B, H, W, Cin, Cout, ksize, int(splits), _vp(ws), ws.numel(), _stream(dy16))
    return dw


def conv_backward(dy, a16, weight, *, need_input=True, need_weight=True, need_bias=True, dx_add=None, splits=0):
    """Backward of y = conv(a16, bf16(weight)) + bias, stride 1, 3x3 pad 1 or 1x1.  dy: the fp32 gradient [B, H, W, Cout], or its bf16 copy when
    no bias gradient is asked for (a producer that already wrote the copy saves the cast pass).  -> (dx or None, dW or None, dbias or None)."""
    if dy.dtype == torch.bfloat16:
        if need_bias:
            raise ValueError("the bias gradient needs the fp32 dy")
        dy16, db = dy, None
    else:
        dy16, db = cast_bias_grad(dy, want_bias=need_bias)
    dw = conv_backward_weight(dy16, a16, weight.shape[2], splits=splits) if need_weight else None
    dx = conv_backward_data(dy16, weight, dx_add=dx_add) if need_input else None
    return dx, dw, db


def groupnorm_stats(x, groups=GROUPS, eps=EPS):
    """x fp32 [B, ..., C] -> (mean, rstd) fp32 [B, groups, 2]"""
    x = _f32(x, "x")
    ctx = context(x.device)
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    stats = torch.empty(B, groups, 2, dtype=torch.float32, device=x.device)
    ws = _workspace(ctx.lib.vt_op_groupnorm_stats_workspace_bytes(B, HW, C), x.device)
    ctx.call("vt_op_groupnorm_stats", _vp(x), B, HW, C, groups, float(eps), _vp(stats), _vp(ws), ws.numel(), _stream(x))
    return stats


def groupnorm_silu_backward(x, stats, gamma, beta, da, *, dx_add=None, want_dx16=False):
    """Backward of a = silu(GroupNorm(x)).  -> (dx fp32, dx16 bf16 or None, dgamma, dbeta); dx_add (fp32, x's shape) is added into dx."""
    x, da = _f32(x, "x"), _f32(da, "da")
    if da.shape != x.shape or (dx_add is not None and _f32(dx_add, "dx_add").shape != x.shape):
        raise ValueError("da and dx_add must have x's shape")
    ctx = context(x.device)
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    groups = stats.shape[1]
    dx = torch.empty_like(x)
    dx16 = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device) if want_dx16 else None
    dg = torch.empty(C, dtype=torch.float32, device=x.device)
    db = torch.empty(C, dtype=torch.float32, device=x.device)
    ws = _workspace(ctx.lib.vt_op_groupnorm_silu_backward_workspace_bytes(B, HW, C), x.device)
    ctx.call("vt_op_groupnorm_silu_backward", _vp(x), _vp(_f32(stats, "stats")), _vp(_f32(gamma, "gamma")), _vp(_f32(beta, "beta")), _vp(da), _vp(dx_add),
             _vp(dx), _vp(dx16), _vp(dg), _vp(db), B, HW, C, groups, _vp(ws), ws.numel(), _stream(x))
    return dx, dx16, dg, db


# ---- the block ------------------------------------------------------------------------------------------------------------------------------------

def _norm_silu(ctx, x, gamma, beta):
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    ws = _workspace(ctx.lib.vt_op_groupnorm_workspace_bytes(B, HW, C), x.device)
    ctx.call("vt_op_groupnorm", _vp(x), _lib.VT_F32, B, HW, C, GROUPS, EPS, _vp(gamma), _vp(beta), 1, _vp(y), _vp(ws), _stream(x))
    return y


def _conv(ctx, a16, weight, bias, residual=None):
    B, H, W, Cin = a16.shape
    Cout, k = weight.shape[0], weight.shape[2]
    w16 = weight.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)             # the forward operator's weight operand: bf16 OHWI
    y = torch.empty(B, H, W, Cout, dtype=torch.float32, device=a16.device)
    ctx.call("vt_op_conv2d", _vp(a16), _vp(w16), _vp(bias), _vp(residual), _vp(y), None, B, H, W, Cin, Cout, k, 1, k // 2, k // 2, _stream(a16))
    return y


def _check_params(params, x):
    names = ["norm1.weight", "norm1.bias", "conv1.weight", "conv1.bias", "norm2.weight", "norm2.bias", "conv2.weight", "conv2.bias"]
    cin, cout = params["conv1.weight"].shape[1], params["conv1.weight"].shape[0]
    if cin != cout:
        names += ["conv_shortcut.weight", "conv_shortcut.bias"]
    missing = [n for n in names if n not in params]
    if missing or set(params) - set(names):
        raise ValueError(f"params must hold exactly {names}")
    for n in names:
        _f32(params[n], n)
    if x.shape[-1] != cin:
        raise ValueError(f"x has {x.shape[-1]} channels, the block takes {cin}")
    return cin != cout


def resnet_block_forward_train(params, x):
    """ResnetBlock2D forward on the existing operators, keeping what the backward needs.  x fp32 NHWC.  -> (y fp32 NHWC, saved)"""
    x = _f32(x, "x")
    ctx = context(x.device)
    ctx.call("vt_op_backward_operands_check")
    has_sc = _check_params(params, x)
    stats1 = groupnorm_stats(x)
    a1 = _norm_silu(ctx, x, params["norm1.weight"], params["norm1.bias"])
    h1 = _conv(ctx, a1, params["conv1.weight"], params["conv1.bias"])
    stats2 = groupnorm_stats(h1)
    a2 = _norm_silu(ctx, h1, params["norm2.weight"], params["norm2.bias"])
    saved = {"x": x, "h1": h1, "a1": a1, "a2": a2, "stats1": stats1, "stats2": stats2}
    if has_sc:
        saved["x16"] = x.to(torch.bfloat16)
        res = _conv(ctx, saved["x16"], params["conv_shortcut.weight"], params["conv_shortcut.bias"])
    else:
        res = x
    y = _conv(ctx, a2, params["conv2.weight"], params["conv2.bias"], residual=res)
    return y, saved


def resnet_block_backward(params, saved, dy, *, splits=0):
    """dy fp32 NHWC, the gradient of resnet_block_forward_train's y.  -> (dx fp32 NHWC, grads keyed like params)"""
    dy = _f32(dy, "dy")
    ctx = context(dy.device)
    ctx.call("vt_op_backward_operands_check")
    has_sc = "x16" in saved
    g = {}
    # 1. cast + db2 (the shortcut conv sees the same dy: dbsc = db2)
    dy16, db2 = cast_bias_grad(dy)
    g["conv2.bias"] = db2
    # 2. conv2
    g["conv2.weight"] = conv_backward_weight(dy16, saved["a2"], 3, splits=splits)
    da2 = conv_backward_data(dy16, params["conv2.weight"])
    # 3. norm2 + SiLU: dh1 and its bf16 copy
    dh1, dh1_16, g["norm2.weight"], g["norm2.bias"] = groupnorm_silu_backward(saved["h1"], saved["stats2"], params["norm2.weight"], params["norm2.bias"], da2,
                                                                              want_dx16=True)
    # 4. conv1
    g["conv1.weight"] = conv_backward_weight(dh1_16, saved["a1"], 3, splits=splits)
    _, g["conv1.bias"] = cast_bias_grad(dh1, want_dy16=False)
    da1 = conv_backward_data(dh1_16, params["conv1.weight"])
    # 5. shortcut
    if has_sc:
        dxs = conv_backward_data(dy16, params["conv_shortcut.weight"])
        g["conv_shortcut.weight"] = conv_backward_weight(dy16, saved["x16"], 1, splits=splits)
        g["conv_shortcut.bias"] = db2.clone()
    else:
        dxs = dy
    # 6. norm1 + SiLU, the shortcut's gradient added in the same pass
    dx, _, g["norm1.weight"], g["norm1.bias"] = groupnorm_silu_backward(saved["x"], saved["stats1"], params["norm1.weight"], params["norm1.bias"], da1, dx_add=dxs)
    return dx, {k: g[k] for k in params}


# ---- the resampling layers: Downsample2D's stride-2 conv and Upsample2D -----------------------------------------------------

def downsample_backward_data(dy16, weight, H, W, *, dx_add=None):
    """dy16 bf16 [B, H // 2, W // 2, Cout], weight fp32 [Cout, Cin, 3, 3] of y = conv(pad(x, (0,1,0,1)), W), stride 2 -> dx fp32 [B, H, W, Cin] (+ dx_add)."""
    dy16, weight = _bf16(dy16, "dy16"), _f32(weight, "weight")
    B, Ho, Wo, Cout = dy16.shape
    Cin = weight.shape[1]
    if tuple(weight.shape) != (Cout, Cin, 3, 3) or (Ho, Wo) != (H // 2, W // 2):
        raise ValueError("weight or (H, W) does not match dy16")
    if dx_add is not None and tuple(_f32(dx_add, "dx_add").shape) != (B, H, W, Cin):
        raise ValueError("dx_add must have dx's shape")
    dx = torch.empty(B, H, W, Cin, dtype=torch.float32, device=dy16.device)
    context(dy16.device).call("vt_op_conv_s2_backward_data", _vp(dy16), _vp(weight), _vp(dx_add), _vp(dx), B, H, W, Cin, Cout, _stream(dy16))
    return dx


def downsample_backward_weight(dy16, a16, *, splits=0):
    """dy16 bf16 [B, H // 2, W // 2, Cout], a16 bf16 [B, H, W, Cin] (the layer's input) -> dW fp32 [Cout, Cin, 3, 3]."""
    dy16, a16 = _bf16(dy16, "dy16"), _bf16(a16, "a16")
    B, H, W, Cin = a16.shape
    Cout = dy16.shape[-1]
    if tuple(dy16.shape[:3]) != (B, H // 2, W // 2):
        raise ValueError("a16 does not match dy16")
    ctx = context(dy16.device)
    dw = torch.empty(Cout, Cin, 3, 3, dtype=torch.float32, device=dy16.device)
    ws = _workspace(ctx.lib.vt_op_conv_s2_backward_weight_workspace_bytes(B, H, W, Cin, Cout, int(splits)), dy16.device)
    ctx.call("vt_op_conv_s2_backward_weight", _vp(dy16), _vp(a16), _vp(dw), B, H, W, Cin, Cout, int(splits), _vp(ws), ws.numel(), _stream(dy16))
    return dw


def upsample_backward_data(dy16, weight, *, dx_add=None):
    """dy16 bf16 [B, 2h, 2w, C], weight fp32 [C, C, 3, 3] of y = conv3x3(nearest2x(x), W) -> dx fp32 [B, h, w, C] (+ dx_add); the route (folded or
    literal, flag 22) is the forward operator's."""
    dy16, weight = _bf16(dy16, "dy16"), _f32(weight, "weight")
    B, H2, W2, C = dy16.shape
    if tuple(weight.shape) != (C, C, 3, 3) or H2 % 2 or W2 % 2:
        raise ValueError("weight does not match dy16, or dy16 has an odd size")
    h, w = H2 // 2, W2 // 2
    if dx_add is not None and tuple(_f32(dx_add, "dx_add").shape) != (B, h, w, C):
        raise ValueError("dx_add must have dx's shape")
    dx = torch.empty(B, h, w, C, dtype=torch.float32, device=dy16.device)
    context(dy16.device).call("vt_op_upsample2x_conv3x3_backward_data", _vp(dy16), _vp(weight), _vp(dx_add), _vp(dx), B, h, w, C, _stream(dy16))
    return dx


def upsample_backward_weight(dy16, x16, *, splits=0):
    """dy16 bf16 [B, 2h, 2w, C], x16 bf16 [B, h, w, C] (the layer's low-resolution input) -> dW fp32 [C, C, 3, 3]."""
    dy16, x16 = _bf16(dy16, "dy16"), _bf16(x16, "x16")
    B, h, w, C = x16.shape
    if tuple(dy16.shape) != (B, 2 * h, 2 * w, C):
        raise ValueError("x16 does not match dy16")
    ctx = context(dy16.device)
    dw = torch.empty(C, C, 3, 3, dtype=torch.float32, device=dy16.device)
    ws = _workspace(ctx.lib.vt_op_upsample2x_conv3x3_backward_weight_workspace_bytes(B, h, w, C, int(splits)), dy16.device)
    ctx.call("vt_op_upsample2x_conv3x3_backward_weight", _vp(dy16), _vp(x16), _vp(dw), B, h, w, C, int(splits), _vp(ws), ws.numel(), _stream(dy16))
    return dw


def _resample_backward(data_fn, weight_fn, dy, need_input, need_weight, need_bias, splits):
    if dy.dtype == torch.bfloat16:
        if need_bias:
            raise ValueError("the bias gradient needs the fp32 dy")
        dy16, db = dy, None
    else:
        dy16, db = cast_bias_grad(dy, want_bias=need_bias)
    dw = weight_fn(dy16, splits) if need_weight else None
    dx = data_fn(dy16) if need_input else None
    return dx, dw, db


def downsample_backward(dy, a16, weight, *, need_input=True, need_weight=True, need_bias=True, dx_add=None, splits=0):
    """Backward of Downsample2D: y = conv(pad(a16, (0,1,0,1)), bf16(weight)) + bias, 3x3 stride 2.  dy: the fp32 gradient [B, H // 2, W // 2, Cout] (or
    its bf16 copy when no bias gradient is asked for); a16 bf16 [B, H, W, Cin].  -> (dx or None, dW or None, dbias or None)"""
    H, W = a16.shape[1], a16.shape[2]
    return _resample_backward(lambda d: downsample_backward_data(d, weight, H, W, dx_add=dx_add), lambda d, sp: downsample_backward_weight(d, a16, splits=sp),
                              dy, need_input, need_weight, need_bias, splits)


def upsample_backward(dy, x16, weight, *, need_input=True, need_weight=True, need_bias=True, dx_add=None, splits=0):
    """Backward of Upsample2D: y = conv3x3(nearest2x(x16), weight) + bias as vt_op_upsample2x_conv3x3 computes it.  dy: the fp32 gradient
    [B, 2h, 2w, C] (or its bf16 copy when no bias gradient is asked for); x16 bf16 [B, h, w, C].  -> (dx or None, dW or None, dbias or None)"""
    return _resample_backward(lambda d: upsample_backward_data(d, weight, dx_add=dx_add), lambda d, sp: upsample_backward_weight(d, x16, splits=sp),
                              dy, need_input, need_weight, need_bias, splits)


def downsample_forward(weight, bias, a16):
    """Downsample2D on the forward operator: a16 bf16 [B, H, W, Cin] -> y fp32 [B, H // 2, W // 2, Cout]"""
    a16, weight = _bf16(a16, "a16"), _f32(weight, "weight")
    B, H, W, Cin = a16.shape
    Cout = weight.shape[0]
    if tuple(weight.shape) != (Cout, Cin, 3, 3) or H < 2 or W < 2:
        raise ValueError("weight does not match a16, or a16 is smaller than 2 x 2")
    w16 = weight.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
    y = torch.empty(B, H // 2, W // 2, Cout, dtype=torch.float32, device=a16.device)
    context(a16.device).call("vt_op_conv2d", _vp(a16), _vp(w16), _vp(bias), None, _vp(y), None, B, H, W, Cin, Cout, 3, 2, 0, 1, _stream(a16))
    return y


def upsample_forward(weight, bias, x16):
    """Upsample2D on the forward operator: x16 bf16 [B, h, w, C] -> y fp32 [B, 2h, 2w, C]"""
    x16, weight = _bf16(x16, "x16"), _f32(weight, "weight")
    B, h, w, C = x16.shape
    if tuple(weight.shape) != (C, C, 3, 3):
        raise ValueError("weight does not match x16")
    y = torch.empty(B, 2 * h, 2 * w, C, dtype=torch.float32, device=x16.device)
    context(x16.device).call("vt_op_upsample2x_conv3x3", _vp(x16), _vp(weight), _vp(bias), _vp(y), B, h, w, C, _stream(x16))
    return y


# ---- a down block / an up block: resnets.0 .. resnets.N-1, then the optional resampling layer ---------------------------------------------------------

DOWN_RESAMPLE, UP_RESAMPLE = "downsamplers.0.conv.", "upsamplers.0.conv."


def _split_block(params, resample):
    """-> ({"resnets.i.": its parameters} in order, the resampling layer's parameters or None)"""
    parts, rs = {}, {}
    for k, v in params.items():
        if k.startswith(resample):
            rs[k[len(resample):]] = v
            continue
        bits = k.split(".")
        if len(bits) < 3 or bits[0] != "resnets" or not bits[1].isdigit():
            raise ValueError(f"{k}: not a parameter of resnets.<i> or {resample[:-1]}")
        parts.setdefault(f"resnets.{int(bits[1])}.", {})[".".join(bits[2:])] = v
    n = len(parts)
    if n == 0 or sorted(parts) != sorted(f"resnets.{i}." for i in range(n)):
        raise ValueError("params must hold resnets.0 .. resnets.N-1")
    if rs and sorted(rs) != ["bias", "weight"]:
        raise ValueError(f"{resample}: expected weight and bias")
    return {f"resnets.{i}.": parts[f"resnets.{i}."] for i in range(n)}, (rs or None)


def _block_forward_train(params, x, resample, forward):
    ctx = context(x.device)
    ctx.call("vt_op_backward_operands_check")
    parts, rs = _split_block(params, resample)
    saved = {}
    for p, q in parts.items():
        x, saved[p] = resnet_block_forward_train(q, x)
    if rs is not None:
        x16 = x.to(torch.bfloat16)
        saved[resample] = {"x16": x16}
        x = forward(_f32(rs["weight"], "weight"), _f32(rs["bias"], "bias"), x16)
    return x, saved


def _block_backward(params, saved, dy, resample, backward, splits):
    context(dy.device).call("vt_op_backward_operands_check")
    parts, rs = _split_block(params, resample)
    g = {}
    if rs is not None:
        dy, g[resample + "weight"], g[resample + "bias"] = backward(_f32(dy, "dy"), saved[resample]["x16"], rs["weight"], splits=splits)
    for p in reversed(list(parts)):
        dy, gp = resnet_block_backward(parts[p], saved[p], dy, splits=splits)
        g.update({p + k: v for k, v in gp.items()})
    return dy, {k: g[k] for k in params}


def down_block_forward_train(params, x):
    """DownEncoderBlock2D of the VAE: resnets.0 .. resnets.N-1, then downsamplers.0.conv where params holds it.  x fp32 NHWC.  -> (y fp32 NHWC, saved)"""
    return _block_forward_train(params, _f32(x, "x"), DOWN_RESAMPLE, downsample_forward)


def down_block_backward(params, saved, dy, *, splits=0):
    """dy fp32 NHWC, the gradient of down_block_forward_train's y.  -> (dx fp32 NHWC, grads keyed like params)"""
    return _block_backward(params, saved, dy, DOWN_RESAMPLE, downsample_backward, splits)


def up_block_forward_train(params, x):
    """UpDecoderBlock2D of the VAE: resnets.0 .. resnets.N-1, then upsamplers.0.conv where params holds it.  x fp32 NHWC.  -> (y fp32 NHWC, saved)"""
    return _block_forward_train(params, _f32(x, "x"), UP_RESAMPLE, upsample_forward)


def up_block_backward(params, saved, dy, *, splits=0):
    """dy fp32 NHWC, the gradient of up_block_forward_train's y.  -> (dx fp32 NHWC, grads keyed like params)"""
    return _block_backward(params, saved, dy, UP_RESAMPLE, upsample_backward, splits)


# ---- the attention block -------------------------------------------------------------------------------------------------------------------------

ATTN_C = 512                      # the attention kernels' only channel count (the FLUX VAE's mid block)
ATTN_PARAMS = ["group_norm.weight", "group_norm.bias", "to_q.weight", "to_q.bias", "to_k.weight", "to_k.bias", "to_v.weight", "to_v.bias",
               "to_out.0.weight", "to_out.0.bias"]
ATTN_SAVED = ["x", "h16", "qk16", "vT16", "o16", "o", "shift", "sums", "stats"]


def groupnorm_backward(x, stats, gamma, beta, dh, *, dx_add=None, want_dx16=False):
    """Backward of h = GroupNorm(x) (no activation).  -> (dx fp32, dx16 bf16 or None, dgamma, dbeta); dx_add (fp32, x's shape) is added into dx."""
    x, dh = _f32(x, "x"), _f32(dh, "dh")
    if dh.shape != x.shape or (dx_add is not None and _f32(dx_add, "dx_add").shape != x.shape):
        raise ValueError("dh and dx_add must have x's shape")
    ctx = context(x.device)
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    groups = stats.shape[1]
    dx = torch.empty_like(x)
    dx16 = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device) if want_dx16 else None
    dg = torch.empty(C, dtype=torch.float32, device=x.device)
    db = torch.empty(C, dtype=torch.float32, device=x.device)
    ws = _workspace(ctx.lib.vt_op_groupnorm_backward_workspace_bytes(B, HW, C), x.device)
    ctx.call("vt_op_groupnorm_backward", _vp(x), _vp(_f32(stats, "stats")), _vp(_f32(gamma, "gamma")), _vp(_f32(beta, "beta")), _vp(dh), _vp(dx_add),
             _vp(dx), _vp(dx16), _vp(dg), _vp(db), B, HW, C, groups, _vp(ws), ws.numel(), _stream(x))
    return dx, dx16, dg, db


def attention_core_backward(qk16, vT16, o, do, shift, sums, *, want_bf16=True, group=0, nsplit=0):
    """dq, dk, dv of o = softmax(q k^T / sqrt(C)) v from what attention_block_forward_train saved.  qk16 bf16 [B, S, 2C], vT16 bf16 [B, C, pitch],
    o and do fp32 [B, S, C], shift fp32 [B, S], sums fp32 [4, B, S].  -> (dq, dk, dv fp32 [B, S, C], (dq16, dk16, dv16) or None).  `group` (images per
    launch) and `nsplit` (workgroups per row block of a sweep) are scheduling knobs: 0 = chosen from the shape; no value changes a bit."""
    qk16, vT16, o, do = _bf16(qk16, "qk16"), _bf16(vT16, "vT16"), _f32(o, "o"), _f32(do, "do")
    B, S, C = o.shape
    ctx = context(o.device)
    if C == ATTN_C:
        if tuple(qk16.shape) != (B, S, 2 * C) or tuple(vT16.shape) != (B, C, ctx.lib.vt_op_attention_vt_pitch(S)) or do.shape != o.shape:
            raise ValueError("qk16 / vT16 / do do not match o")
        if tuple(_f32(shift, "shift").shape) != (B, S) or tuple(_f32(sums, "sums").shape) != (4, B, S):
            raise ValueError("shift must be [B, S] and sums [4, B, S]")
    outs = [torch.empty(B, S, C, dtype=torch.float32, device=o.device) for _ in range(3)]
    outs16 = [torch.empty(B, S, C, dtype=torch.bfloat16, device=o.device) for _ in range(3)] if want_bf16 else [None] * 3
    ws = _workspace(ctx.lib.vt_op_attention_core_backward_workspace_bytes(B, S, C), o.device)
    ctx.call("vt_op_attention_core_backward", _vp(qk16), _vp(vT16), _vp(o), _vp(do), _vp(shift), _vp(sums), *[_vp(t) for t in outs], *[_vp(t) for t in outs16],
             B, S, C, int(group), int(nsplit), _vp(ws), ws.numel(), _stream(o))
    return outs[0], outs[1], outs[2], (tuple(outs16) if want_bf16 else None)


def _check_attn_params(params, x):
    if sorted(params) != sorted(ATTN_PARAMS):
        raise ValueError(f"params must hold exactly {ATTN_PARAMS}")
    C = x.shape[-1]
    for n in ATTN_PARAMS:
        want = (C, C) if n.endswith("weight") and not n.startswith("group_norm") else (C,)
        if tuple(_f32(params[n], n).shape) != want:
            raise ValueError(f"{n}: expected shape {want}")


def attention_block_forward_train(params, x):
    """The mid-block attention (GroupNorm, to_q / to_k / to_v, softmax(q k^T / sqrt(C)) v, to_out, + x) on caller-owned fp32 parameters, keeping what
    the backward needs.  x fp32 NHWC [B, H, W, 512].  -> (y fp32 NHWC, saved)"""
    x = _f32(x, "x")
    if x.dim() != 4:
        raise ValueError("x must be NHWC")
    ctx = context(x.device)
    ctx.call("vt_op_backward_operands_check")
    _check_attn_params(params, x)
    B, H, W, C = x.shape
    S, dev = H * W, x.device
    pitch = ctx.lib.vt_op_attention_vt_pitch(S) if C == ATTN_C else S
    bf, f32 = torch.bfloat16, torch.float32
    y = torch.empty_like(x)
    saved = {"x": x, "h16": torch.empty(B, H, W, C, dtype=bf, device=dev), "qk16": torch.empty(B, S, 2 * C, dtype=bf, device=dev),
             "vT16": torch.empty(B, C, pitch, dtype=bf, device=dev), "o16": torch.empty(B, H, W, C, dtype=bf, device=dev),
             "o": torch.empty(B, S, C, dtype=f32, device=dev), "shift": torch.empty(B, S, dtype=f32, device=dev),
             "sums": torch.empty(4, B, S, dtype=f32, device=dev), "stats": torch.empty(B, GROUPS, 2, dtype=f32, device=dev)}
    ws = _workspace(ctx.lib.vt_op_attention_forward_train_workspace_bytes(B, S, C), dev)
    ctx.call("vt_op_attention_forward_train", _vp(x), *[_vp(params[n]) for n in ATTN_PARAMS], _vp(y), *[_vp(saved[n]) for n in ATTN_SAVED[1:]], B, S, C,
             _vp(ws), ws.numel(), _stream(x))
    return y, saved


def attention_block_backward(params, saved, dy, *, splits=0, group=0, nsplit=0):
    """dy fp32 NHWC, the gradient of attention_block_forward_train's y.  -> (dx fp32 NHWC, grads keyed like params)"""
    dy = _f32(dy, "dy")
    ctx = context(dy.device)
    ctx.call("vt_op_backward_operands_check")
    B, H, W, C = dy.shape
    S = H * W
    w4 = lambda n: params[n].view(C, C, 1, 1)
    g = {}
    # 1. to_out: dbo, dWo = dy^T o, do = dy Wo (the residual passes dy on to dx in step 4)
    dy16, g["to_out.0.bias"] = cast_bias_grad(dy)
    g["to_out.0.weight"] = conv_backward_weight(dy16, saved["o16"], 1, splits=splits).view(C, C)
    do = conv_backward_data(dy16, w4("to_out.0.weight"))
    # 2. the core
    dq, dk, dv, (dq16, dk16, dv16) = attention_core_backward(saved["qk16"], saved["vT16"], saved["o"], do.view(B, S, C), saved["shift"], saved["sums"],
                                                              group=group, nsplit=nsplit)
    # 3. the three linears: weight gradients from the bf16 copies, bias sums from the fp32 gradients, dh chained through dx_add
    dh = None
    for name, d32, d16 in (("to_q", dq, dq16), ("to_k", dk, dk16), ("to_v", dv, dv16)):
        d16 = d16.view(B, H, W, C)
        g[name + ".weight"] = conv_backward_weight(d16, saved["h16"], 1, splits=splits).view(C, C)
        _, g[name + ".bias"] = cast_bias_grad(d32, want_dy16=False)
        dh = conv_backward_data(d16, w4(name + ".weight"), dx_add=dh)
    # 4. the norm, the residual's dy added in the same pass
    dx, _, g["group_norm.weight"], g["group_norm.bias"] = groupnorm_backward(saved["x"], saved["stats"], params["group_norm.weight"], params["group_norm.bias"], dh,
                                                                              dx_add=dy)
    return dx, {k: g[k] for k in params}


# ---- the mid block: resnets.0, attentions.0, resnets.1 ---------------------------------------------------------------------------------------------

MID_PARTS = (("resnets.0.", "resnet"), ("attentions.0.", "attention"), ("resnets.1.", "resnet"))


def _split_mid(params):
    parts = {p: {} for p, _ in MID_PARTS}
    for k, v in params.items():
        for p, _ in MID_PARTS:
            if k.startswith(p):
                parts[p][k[len(p):]] = v
                break
        else:
            raise ValueError(f"{k}: not a parameter of resnets.0, attentions.0 or resnets.1")
    return parts


def mid_block_forward_train(params, x):
    """UNetMidBlock2D of the VAE: resnets.0 -> attentions.0 -> resnets.1, parameters under diffusers' names.  -> (y fp32 NHWC, saved)"""
    parts = _split_mid(params)
    saved = {}
    for p, kind in MID_PARTS:
        fwd = resnet_block_forward_train if kind == "resnet" else attention_block_forward_train
        x, saved[p] = fwd(parts[p], x)
    return x, saved


def mid_block_backward(params, saved, dy, *, splits=0):
    """dy fp32 NHWC, the gradient of mid_block_forward_train's y.  -> (dx fp32 NHWC, grads keyed like params)"""
    parts = _split_mid(params)
    g = {}
    for p, kind in reversed(MID_PARTS):
        bwd = resnet_block_backward if kind == "resnet" else attention_block_backward
        dy, gp = bwd(parts[p], saved[p], dy, splits=splits)
        g.update({p + k: v for k, v in gp.items()})
    return dy, {k: g[k] for k in params}
