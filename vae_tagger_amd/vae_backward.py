"""Backward of the VAE's blocks -- ResnetBlock2D (the block both VAE models consist of), the mid attention block, the two resampling layers
(Downsample2D's stride-2 conv and Upsample2D), the four end convs, and their compositions: the mid block, a down block, an up block and the two whole
models (encoder_forward_train / encoder_backward: d moments -> the gradients of every encoder tensor; decoder_forward_train / decoder_backward: d image ->
the gradients of every decoder tensor and d z) -- on the device: thin wrappers over the vt_op_* backward operators (include/vae_tagger_hip.h, DESIGN.md
sections 4.19, 4.20, 4.22 and 4.23).  Tensors are torch tensors of one HIP device,
activations NHWC ([B, H, W, C]), parameters in diffusers' own layouts (conv weights fp32 OIHW).  All gradients are fp32; every MFMA operand is bf16.
Every launch goes to torch's current stream of the tensors' device and nothing here synchronises with the host.  There is no eager fallback: a shape
an operator refuses raises VTError.

The whole-model functions work in NCHW at their ends (the image, the moments, the latents) and in NHWC inside; encoder_saved_bytes / decoder_saved_bytes
say what a batch keeps between forward and backward before anything is allocated.

vae_loss_and_grads joins them into one step of train_vae.py: the three encodes, the anchor's decode, the loss (vt_vae_loss_backward: MSE, KL, triplet
and the backward of posterior.sample) and the gradients of all encoder and decoder tensors.

The optimiser, gradient clipping, checkpoints and the CLI are vae_tagger_amd/train_vae.py (VAETrainer reads these gradients where they lie; DESIGN.md
section 4.25), not here; the contrastive term and AdaptiveLossWeights have no gradient; the image's own gradient is not computed.
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


def _call_ws(ctx, op, size_args, t, *args):
    """ctx.call(op, *args, ws, ws_bytes, stream): the workspace is what `<op>_workspace_bytes(*size_args)` asks for (none with size_args None), on
    t's device, the stream torch's current one there."""
    n = getattr(ctx.lib, op + "_workspace_bytes")(*size_args) if size_args is not None else 0
    ws = _workspace(n, t.device)
    ctx.call(op, *args, _vp(ws), ws.numel(), _stream(t))


def _grads_like(params, *parts):
    """the gradients of parts ((prefix, grads keyed without it), ...) under their full names, keyed and ordered like params"""
    g = {p + k: v for p, gp in parts for k, v in gp.items()}
    return {k: g[k] for k in params}


def cast_bias_grad(dy, *, want_dy16=True, want_bias=True):
    """dy fp32 [..., C] -> (bf16 copy or None, column sums over all leading dimensions or None), one pass."""
    dy = _f32(dy, "dy")
    C = dy.shape[-1]
    rows = dy.numel() // C
    dy16 = torch.empty(dy.shape, dtype=torch.bfloat16, device=dy.device) if want_dy16 else None
    db = torch.empty(C, dtype=torch.float32, device=dy.device) if want_bias else None
    _call_ws(context(dy.device), "vt_op_cast_bias_grad", (rows, C) if want_bias else None, dy, _vp(dy), _vp(dy16), _vp(db), rows, C)
    return dy16, db


def _dy16_and_bias(dy, need_bias, need_dy16=True):
    """dy: the fp32 gradient, or its bf16 copy when no bias gradient is asked for (a producer that already wrote the copy saves the cast pass).
    -> (dy16, dbias or None); no pass at all where neither is needed."""
    if dy.dtype == torch.bfloat16:
        if need_bias:
            raise ValueError("the bias gradient needs the fp32 dy")
        return dy, None
    if not (need_dy16 or need_bias):
        return None, None
    return cast_bias_grad(dy, want_dy16=need_dy16, want_bias=need_bias)


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
    dw = torch.empty(Cout, Cin, ksize, ksize, dtype=torch.float32, device=dy16.device)
    shape = (B, H, W, Cin, Cout, ksize, int(splits))
    _call_ws(context(dy16.device), "vt_op_conv_backward_weight", shape, dy16, _vp(dy16), _vp(a16), _vp(dw), *shape)
    return dw


def conv_backward(dy, a16, weight, *, need_input=True, need_weight=True, need_bias=True, dx_add=None, splits=0):
    """Backward of y = conv(a16, bf16(weight)) + bias, stride 1, 3x3 pad 1 or 1x1.  dy: the fp32 gradient [B, H, W, Cout], or its bf16 copy when
    no bias gradient is asked for (a producer that already wrote the copy saves the cast pass).  -> (dx or None, dW or None, dbias or None)."""
    dy16, db = _dy16_and_bias(dy, need_bias)
    dw = conv_backward_weight(dy16, a16, weight.shape[2], splits=splits) if need_weight else None
    dx = conv_backward_data(dy16, weight, dx_add=dx_add) if need_input else None
    return dx, dw, db


def groupnorm_stats(x, groups=GROUPS, eps=EPS):
    """x fp32 [B, ..., C] -> (mean, rstd) fp32 [B, groups, 2]"""
    x = _f32(x, "x")
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    stats = torch.empty(B, groups, 2, dtype=torch.float32, device=x.device)
    _call_ws(context(x.device), "vt_op_groupnorm_stats", (B, HW, C), x, _vp(x), B, HW, C, groups, float(eps), _vp(stats))
    return stats


def _groupnorm_backward(op, x, stats, gamma, beta, d, d_name, dx_add, want_dx16):
    x, d = _f32(x, "x"), _f32(d, d_name)
    if d.shape != x.shape or (dx_add is not None and _f32(dx_add, "dx_add").shape != x.shape):
        raise ValueError(f"{d_name} and dx_add must have x's shape")
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    groups = stats.shape[1]
    dx = torch.empty_like(x)
    dx16 = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device) if want_dx16 else None
    dg = torch.empty(C, dtype=torch.float32, device=x.device)
    db = torch.empty(C, dtype=torch.float32, device=x.device)
    _call_ws(context(x.device), op, (B, HW, C), x, _vp(x), _vp(_f32(stats, "stats")), _vp(_f32(gamma, "gamma")), _vp(_f32(beta, "beta")), _vp(d), _vp(dx_add),
             _vp(dx), _vp(dx16), _vp(dg), _vp(db), B, HW, C, groups)
    return dx, dx16, dg, db


def groupnorm_silu_backward(x, stats, gamma, beta, da, *, dx_add=None, want_dx16=False):
    """Backward of a = silu(GroupNorm(x)).  -> (dx fp32, dx16 bf16 or None, dgamma, dbeta); dx_add (fp32, x's shape) is added into dx."""
    return _groupnorm_backward("vt_op_groupnorm_silu_backward", x, stats, gamma, beta, da, "da", dx_add, want_dx16)


def groupnorm_backward(x, stats, gamma, beta, dh, *, dx_add=None, want_dx16=False):
    """Backward of h = GroupNorm(x) (no activation).  -> (dx fp32, dx16 bf16 or None, dgamma, dbeta); dx_add (fp32, x's shape) is added into dx."""
    return _groupnorm_backward("vt_op_groupnorm_backward", x, stats, gamma, beta, dh, "dh", dx_add, want_dx16)


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


def resnet_block_backward(params, saved, dy, *, splits=0, want_dx16=False):
    """dy fp32 NHWC, the gradient of resnet_block_forward_train's y.  -> (dx fp32 NHWC, grads keyed like params); with want_dx16 norm1's pass also
    writes bf16(dx) and the result is (dx, grads, dx16)."""
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
    dx, dx16, g["norm1.weight"], g["norm1.bias"] = groupnorm_silu_backward(saved["x"], saved["stats1"], params["norm1.weight"], params["norm1.bias"], da1, dx_add=dxs,
                                                                              want_dx16=want_dx16)
    g = _grads_like(params, ("", g))
    return (dx, g, dx16) if want_dx16 else (dx, g)


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
    dw = torch.empty(Cout, Cin, 3, 3, dtype=torch.float32, device=dy16.device)
    shape = (B, H, W, Cin, Cout, int(splits))
    _call_ws(context(dy16.device), "vt_op_conv_s2_backward_weight", shape, dy16, _vp(dy16), _vp(a16), _vp(dw), *shape)
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
    dw = torch.empty(C, C, 3, 3, dtype=torch.float32, device=dy16.device)
    shape = (B, h, w, C, int(splits))
    _call_ws(context(dy16.device), "vt_op_upsample2x_conv3x3_backward_weight", shape, dy16, _vp(dy16), _vp(x16), _vp(dw), *shape)
    return dw


def _resample_backward(data_fn, weight_fn, dy, need_input, need_weight, need_bias, splits):
    dy16, db = _dy16_and_bias(dy, need_bias)
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


def _block_backward(params, saved, dy, resample, backward, splits, want_dx16=False):
    context(dy.device).call("vt_op_backward_operands_check")
    parts, rs = _split_block(params, resample)
    g = []
    if rs is not None:
        dy, dw, db = backward(_f32(dy, "dy"), saved[resample]["x16"], rs["weight"], splits=splits)
        g.append((resample, {"weight": dw, "bias": db}))
    dx16 = None
    for p in reversed(list(parts)):
        if want_dx16 and p == "resnets.0.":
            dy, gp, dx16 = resnet_block_backward(parts[p], saved[p], dy, splits=splits, want_dx16=True)
        else:
            dy, gp = resnet_block_backward(parts[p], saved[p], dy, splits=splits)
        g.append((p, gp))
    g = _grads_like(params, *g)
    return (dy, g, dx16) if want_dx16 else (dy, g)


def down_block_forward_train(params, x):
    """DownEncoderBlock2D of the VAE: resnets.0 .. resnets.N-1, then downsamplers.0.conv where params holds it.  x fp32 NHWC.  -> (y fp32 NHWC, saved)"""
    return _block_forward_train(params, _f32(x, "x"), DOWN_RESAMPLE, downsample_forward)


def down_block_backward(params, saved, dy, *, splits=0, want_dx16=False):
    """dy fp32 NHWC, the gradient of down_block_forward_train's y.  -> (dx fp32 NHWC, grads keyed like params); with want_dx16 also bf16(dx), as
    resnet_block_backward writes it."""
    return _block_backward(params, saved, dy, DOWN_RESAMPLE, downsample_backward, splits, want_dx16)


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
    _call_ws(ctx, "vt_op_attention_core_backward", (B, S, C), o, _vp(qk16), _vp(vT16), _vp(o), _vp(do), _vp(shift), _vp(sums), *[_vp(t) for t in outs],
             *[_vp(t) for t in outs16], B, S, C, int(group), int(nsplit))
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
    _call_ws(ctx, "vt_op_attention_forward_train", (B, S, C), x, _vp(x), *[_vp(params[n]) for n in ATTN_PARAMS], _vp(y), *[_vp(saved[n]) for n in ATTN_SAVED[1:]],
             B, S, C)
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
    return dx, _grads_like(params, ("", g))


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
    g = []
    for p, kind in reversed(MID_PARTS):
        bwd = resnet_block_backward if kind == "resnet" else attention_block_backward
        dy, gp = bwd(parts[p], saved[p], dy, splits=splits)
        g.append((p, gp))
    return dy, _grads_like(params, *g)


# ---- the end convs ---------------------------------------------------------------------------------------------------------
# Full resolution, 3 channels on one side (encoder.conv_in, decoder.conv_out): vt_op_conv_thin_backward_weight / vt_op_conv_thin_forward.
# Latent resolution (encoder.conv_out 512 -> 32, decoder.conv_in 16 -> 512): the existing operators, the short side zero-padded to 64 channels here.

WGRAD_C = 64                      # vt_op_conv_backward_weight's channel tile: the short side of a latent-resolution end is padded to it


def _nchw3(t, what):
    if _f32(t, what).dim() != 4 or t.shape[1] != 3:
        raise ValueError(f"{what}: expected fp32 NCHW [B, 3, H, W]")
    return t


def conv_thin_backward_weight(thin_nchw, wide16, thin_is_input, *, want_sums=False, splits=0):
    """The thin-side weight gradient.  thin fp32 NCHW [B, 3, H, W], wide16 bf16 NHWC [B, H, W, Cw].  -> (dW fp32 [Cw, 3, 3, 3] (thin_is_input) or
    [3, Cw, 3, 3], the thin side's channel sums [3] or None)"""
    thin, wide16 = _nchw3(thin_nchw, "thin"), _bf16(wide16, "wide16")
    B, _, H, W = thin.shape
    Cw = wide16.shape[-1]
    if tuple(wide16.shape[:3]) != (B, H, W):
        raise ValueError("wide16 does not match thin")
    dw = torch.empty((Cw, 3, 3, 3) if thin_is_input else (3, Cw, 3, 3), dtype=torch.float32, device=thin.device)
    sums = torch.empty(3, dtype=torch.float32, device=thin.device) if want_sums else None
    shape = (B, H, W, Cw, int(splits))
    _call_ws(context(thin.device), "vt_op_conv_thin_backward_weight", shape, thin, _vp(thin), _vp(wide16), int(bool(thin_is_input)), _vp(dw), _vp(sums), *shape)
    return dw, sums


def conv_thin_forward(x_nchw, weight, bias=None, *, transpose_rotate=False, want_f32=True, want_bf16=False):
    """The 3 -> C conv on conv_in's kernels, weights packed on the stream.  x fp32 NCHW [B, 3, H, W]; weight fp32 [C, 3, 3, 3], or with transpose_rotate
    conv_out's [3, C, 3, 3] (then this is conv_out's data gradient, and bias is ignored).  -> (fp32 NHWC [B, H, W, C] or None, its bf16 form or None)"""
    x, weight = _nchw3(x_nchw, "x"), _f32(weight, "weight")
    B, _, H, W = x.shape
    C = weight.shape[1] if transpose_rotate else weight.shape[0]
    if tuple(weight.shape) != ((3, C, 3, 3) if transpose_rotate else (C, 3, 3, 3)):
        raise ValueError("weight must be [C, 3, 3, 3], or [3, C, 3, 3] with transpose_rotate")
    if bias is not None and tuple(_f32(bias, "bias").shape) != (C,):
        raise ValueError("bias must be [C]")
    o32 = torch.empty(B, H, W, C, dtype=torch.float32, device=x.device) if want_f32 else None
    o16 = torch.empty(B, H, W, C, dtype=torch.bfloat16, device=x.device) if want_bf16 else None
    _call_ws(context(x.device), "vt_op_conv_thin_forward", (C,), x, _vp(x), _vp(weight), _vp(bias), int(bool(transpose_rotate)), _vp(o32), _vp(o16), B, H, W, C)
    return o32, o16


def conv_in_backward(dy, x_nchw, *, need_weight=True, need_bias=True, splits=0, dy16=None):
    """Backward of encoder.conv_in, y = conv(x, W) + b with x the fp32 NCHW image.  dy: the fp32 gradient NHWC [B, H, W, C], or its bf16 copy when no bias
    gradient is asked for; dy16 (optional): the bf16 copy a producer already wrote beside the fp32 dy.  -> (dW [C, 3, 3, 3], db); the image's own gradient
    is not offered."""
    c16, db = _dy16_and_bias(dy, need_bias, need_dy16=need_weight and dy16 is None)
    if dy16 is None or dy.dtype == torch.bfloat16:
        dy16 = c16
    dw = conv_thin_backward_weight(x_nchw, dy16, True, splits=splits)[0] if need_weight else None
    return dw, db


def conv_out_backward(d_image_nchw, a16, weight, *, need_input=True, need_weight=True, need_bias=True, splits=0):
    """Backward of decoder.conv_out, image = conv(a16, W) + b with W [3, C, 3, 3].  d_image fp32 NCHW [B, 3, H, W]; a16 bf16 NHWC [B, H, W, C], the conv's
    forward operand.  -> (dx fp32 NHWC [B, H, W, C] or None, dW or None, db [3] or None)"""
    dx = conv_thin_forward(d_image_nchw, weight, transpose_rotate=True)[0] if need_input else None
    dw, db = None, None
    if need_weight or need_bias:
        dw, db = conv_thin_backward_weight(d_image_nchw, a16, False, want_sums=need_bias, splits=splits)
    return dx, (dw if need_weight else None), db


def _pad_channels(t16, C):
    return t16 if t16.shape[-1] == C else torch.nn.functional.pad(t16, (0, C - t16.shape[-1]))


def latent_conv_out_backward(dy, a16, weight, *, splits=0):
    """Backward of encoder.conv_out (C -> 2L at latent resolution, 2L < 64): dy fp32 NHWC [B, h, w, 2L].  The weight gradient runs on dy16 zero-padded
    to 64 channels and is sliced.  -> (dx fp32 NHWC, dW, db)"""
    dy16, db = cast_bias_grad(dy)
    n = dy16.shape[-1]
    dw = conv_backward_weight(_pad_channels(dy16, -(-n // WGRAD_C) * WGRAD_C), a16, 3, splits=splits)[:n].contiguous()
    return conv_backward_data(dy16, weight), dw, db


def latent_conv_in_backward(dy, z16, weight, *, splits=0):
    """Backward of decoder.conv_in (L -> C at latent resolution, L < 64): dy fp32 NHWC [B, h, w, C]; z16 the staged latents, bf16 NHWC zero-padded to
    64 channels.  -> (dz fp32 NHWC [B, h, w, L], dW, db)"""
    dy16, db = cast_bias_grad(dy)
    L = weight.shape[1]
    dw = conv_backward_weight(dy16, z16, 3, splits=splits)[:, :L].contiguous()
    return conv_backward_data(dy16, weight), dw, db


# ---- the whole models ---------------------------------------------------------------------------------------------------------------------------------

ENDS = ("conv_in.", "conv_norm_out.", "conv_out.")


def _split_model(params, prefix, blocks):
    """params under `prefix` ("encoder." / "decoder.") -> ({"conv_in.": {weight, bias}, ...}, [block i's parameters], the mid block's)"""
    ends, blk, mid = {e: {} for e in ENDS}, {}, {}
    for k, v in params.items():
        r = k[len(prefix):] if k.startswith(prefix) else None
        bits = r.split(".", 2) if r else []
        if r and r.startswith("mid_block."):
            mid[r[len("mid_block."):]] = v
        elif len(bits) == 3 and bits[0] == blocks and bits[1].isdigit():
            blk.setdefault(int(bits[1]), {})[bits[2]] = v
        elif r and any(r in (e + "weight", e + "bias") for e in ENDS):
            ends[bits[0] + "."][bits[1]] = v
        else:
            raise ValueError(f"{k}: not a parameter of {prefix}conv_in, {blocks}.<i>, mid_block, conv_norm_out or conv_out")
    if not blk or sorted(blk) != list(range(len(blk))):
        raise ValueError(f"params must hold {prefix}{blocks}.0 .. {blocks}.N-1")
    for e in ENDS:
        if sorted(ends[e]) != ["bias", "weight"]:
            raise ValueError(f"{prefix}{e[:-1]}: expected weight and bias")
    return ends, [blk[i] for i in range(len(blk))], mid


def _shape(v):
    return tuple(v.shape) if hasattr(v, "shape") else tuple(v)


def model_structure(params, prefix):
    """The block structure read from the key names (values: tensors or shapes): {"blocks": [{"resnets": [(cin, cout), ...], "resample": bool}, ...],
    "mid": C, "conv_in": (cout, cin), "conv_out": (cout, cin)}"""
    blocks = "down_blocks" if prefix == "encoder." else "up_blocks"
    ends, blks, mid = _split_model(params, prefix, blocks)
    _split_mid(mid)
    out = []
    for q in blks:
        parts, rs = _split_block(q, DOWN_RESAMPLE if prefix == "encoder." else UP_RESAMPLE)
        out.append({"resnets": [(_shape(r["conv1.weight"])[1], _shape(r["conv1.weight"])[0]) for r in parts.values()], "resample": rs is not None})
    return {"blocks": out, "mid": _shape(mid["resnets.0.conv1.weight"])[0], "conv_in": _shape(ends["conv_in."]["weight"])[:2],
            "conv_out": _shape(ends["conv_out."]["weight"])[:2]}


def _norm_out_forward(ctx, ends, x):
    n = ends["conv_norm_out."]
    return {"x": x, "stats": groupnorm_stats(x), "a16": _norm_silu(ctx, x, _f32(n["weight"], "conv_norm_out.weight"), _f32(n["bias"], "conv_norm_out.bias"))}


def _norm_out_backward(ends, saved, da, g, prefix):
    n = ends["conv_norm_out."]
    dx, _, g[prefix + "conv_norm_out.weight"], g[prefix + "conv_norm_out.bias"] = groupnorm_silu_backward(saved["x"], saved["stats"], n["weight"], n["bias"], da)
    return dx


def encoder_forward_train(params, x_nchw):
    """The VAE encoder (conv_in, the down blocks, the mid block, conv_norm_out + SiLU, conv_out) on caller-owned fp32 parameters under diffusers' names
    (`encoder.*`, synth.encoder_manifest), keeping what the backward needs.  x fp32 NCHW [B, 3, H, W].  -> (moments fp32 NCHW [B, 2L, h, w], saved)"""
    x = _nchw3(x_nchw, "x")
    ctx = context(x.device)
    ctx.call("vt_op_backward_operands_check")
    ends, blks, mid = _split_model(params, "encoder.", "down_blocks")
    saved = {"x": x}
    h = conv_thin_forward(x, ends["conv_in."]["weight"], ends["conv_in."]["bias"])[0]
    for i, q in enumerate(blks):
        h, saved[f"down_blocks.{i}."] = down_block_forward_train(q, h)
    h, saved["mid_block."] = mid_block_forward_train(mid, h)
    saved["conv_norm_out."] = _norm_out_forward(ctx, ends, h)
    y = _conv(ctx, saved["conv_norm_out."]["a16"], _f32(ends["conv_out."]["weight"], "conv_out.weight"), _f32(ends["conv_out."]["bias"], "conv_out.bias"))
    return y.permute(0, 3, 1, 2).contiguous(), saved


def encoder_backward(params, saved, d_moments, *, splits=0, boundaries=None):
    """d_moments fp32 NCHW, the gradient of encoder_forward_train's moments.  -> grads: fp32, keyed and ordered like params.  boundaries (optional dict)
    receives the gradient (fp32 NHWC) of every stage's input: "conv_norm_out", "mid_block", "down_blocks.<i>" (tools/vae_backward_boundaries.py)."""
    at = boundaries if boundaries is not None else {}
    d = _f32(d_moments, "d_moments")
    context(d.device).call("vt_op_backward_operands_check")
    ends, blks, mid = _split_model(params, "encoder.", "down_blocks")
    g = {}
    dy = d.permute(0, 2, 3, 1).contiguous()
    dy, g["encoder.conv_out.weight"], g["encoder.conv_out.bias"] = latent_conv_out_backward(dy, saved["conv_norm_out."]["a16"], ends["conv_out."]["weight"], splits=splits)
    at["conv_norm_out"] = dy = _norm_out_backward(ends, saved["conv_norm_out."], dy, g, "encoder.")
    dy, gp = mid_block_backward(mid, saved["mid_block."], dy, splits=splits)
    at["mid_block"] = dy
    parts = [("encoder.mid_block.", gp)]
    dy16 = None
    for i in reversed(range(len(blks))):
        if i == 0:          # conv_in's weight gradient takes the bf16 copy norm1's pass writes: no cast pass at full resolution
            dy, gp, dy16 = down_block_backward(blks[i], saved[f"down_blocks.{i}."], dy, splits=splits, want_dx16=True)
        else:
            dy, gp = down_block_backward(blks[i], saved[f"down_blocks.{i}."], dy, splits=splits)
        parts.append((f"encoder.down_blocks.{i}.", gp))
        at[f"down_blocks.{i}"] = dy
    g["encoder.conv_in.weight"], g["encoder.conv_in.bias"] = conv_in_backward(dy, saved["x"], splits=splits, dy16=dy16)
    return _grads_like(params, ("", g), *parts)


def decoder_forward_train(params, z_nchw):
    """The VAE's image decoder (conv_in, the mid block, the up blocks, conv_norm_out + SiLU, conv_out) on caller-owned fp32 parameters under diffusers'
    names (`decoder.*`, synth.image_decoder_manifest).  z fp32 NCHW [B, L, h, w], L <= 64.  -> (image fp32 NCHW [B, 3, H, W], saved).  conv_in runs on
    the latents staged as bf16 NHWC, zero-padded to 64 channels (the inference decoder pads to 32: the same sums); conv_out on vt_op_conv2d with its 3
    couts zero-padded to 32, as the inference decoder's."""
    z = _f32(z_nchw, "z")
    ctx = context(z.device)
    ctx.call("vt_op_backward_operands_check")
    ends, blks, mid = _split_model(params, "decoder.", "up_blocks")
    w_in, w_out = _f32(ends["conv_in."]["weight"], "conv_in.weight"), _f32(ends["conv_out."]["weight"], "conv_out.weight")
    L, nout = w_in.shape[1], w_out.shape[0]
    if z.dim() != 4 or z.shape[1] != L or L > WGRAD_C or nout != 3:
        raise ValueError(f"z must be NCHW with conv_in's {L} <= {WGRAD_C} channels, and conv_out must have 3 output channels")
    z16 = _pad_channels(z.permute(0, 2, 3, 1).to(torch.bfloat16), WGRAD_C).contiguous()
    saved = {"z16": z16}
    h = _conv(ctx, z16, torch.nn.functional.pad(w_in, (0, 0, 0, 0, 0, WGRAD_C - L)), _f32(ends["conv_in."]["bias"], "conv_in.bias"))
    h, saved["mid_block."] = mid_block_forward_train(mid, h)
    for i, q in enumerate(blks):
        h, saved[f"up_blocks.{i}."] = up_block_forward_train(q, h)
    saved["conv_norm_out."] = _norm_out_forward(ctx, ends, h)
    y = _conv(ctx, saved["conv_norm_out."]["a16"], torch.nn.functional.pad(w_out, (0, 0, 0, 0, 0, 0, 0, 32 - nout)),
              torch.nn.functional.pad(_f32(ends["conv_out."]["bias"], "conv_out.bias"), (0, 32 - nout)))
    return y[..., :nout].permute(0, 3, 1, 2).contiguous(), saved


def decoder_backward(params, saved, d_image, *, splits=0, boundaries=None):
    """d_image fp32 NCHW [B, 3, H, W], the gradient of decoder_forward_train's image.  -> (dz fp32 NCHW [B, L, h, w], grads keyed and ordered like params).
    boundaries (optional dict) receives the gradient (fp32 NHWC) of every stage's input: "conv_norm_out", "up_blocks.<i>", "mid_block"."""
    at = boundaries if boundaries is not None else {}
    d = _nchw3(d_image, "d_image")
    context(d.device).call("vt_op_backward_operands_check")
    ends, blks, mid = _split_model(params, "decoder.", "up_blocks")
    g = {}
    dy, g["decoder.conv_out.weight"], g["decoder.conv_out.bias"] = conv_out_backward(d, saved["conv_norm_out."]["a16"], ends["conv_out."]["weight"], splits=splits)
    at["conv_norm_out"] = dy = _norm_out_backward(ends, saved["conv_norm_out."], dy, g, "decoder.")
    parts = []
    for i in reversed(range(len(blks))):
        dy, gp = up_block_backward(blks[i], saved[f"up_blocks.{i}."], dy, splits=splits)
        at[f"up_blocks.{i}"] = dy
        parts.append((f"decoder.up_blocks.{i}.", gp))
    dy, gp = mid_block_backward(mid, saved["mid_block."], dy, splits=splits)
    at["mid_block"] = dy
    parts.append(("decoder.mid_block.", gp))
    dz, g["decoder.conv_in.weight"], g["decoder.conv_in.bias"] = latent_conv_in_backward(dy, saved["z16"], ends["conv_in."]["weight"], splits=splits)
    return dz.permute(0, 3, 1, 2).contiguous(), _grads_like(params, ("", g), *parts)


# ---- what a batch keeps between forward and backward: pure-Python formulas, exactly the bytes of the `saved` structures ---------------------------------

def attention_vt_pitch(S):
    """vt_op_attention_vt_pitch in Python: S rounded up to 8, moved off the pitches that are multiples of 2 KB"""
    ld = (S + 7) // 8 * 8
    return ld + 2048 + 64 if (ld * 2) % 2048 == 0 else ld


def _resnet_saved_bytes(P, B, ci, co):
    return P * (ci * 4 + co * 4 + ci * 2 + co * 2) + 2 * B * GROUPS * 2 * 4 + (P * ci * 2 if ci != co else 0)


def _mid_saved_bytes(B, S, C):
    P = B * S
    attn = P * C * (4 + 2 + 4 + 2 + 4) + B * C * attention_vt_pitch(S) * 2 + P * 4 + 4 * P * 4 + B * GROUPS * 2 * 4     # x, h16, qk16, o16, o; vT16; shift; sums; stats
    return 2 * _resnet_saved_bytes(P, B, C, C) + attn


def _structure_of(params_or_config, prefix):
    if "block_out" in params_or_config or "layers_per_block" in params_or_config:
        from . import synth
        params_or_config = (synth.encoder_manifest if prefix == "encoder." else synth.image_decoder_manifest)(**params_or_config)
    return model_structure(params_or_config, prefix)


def _blocks_saved_bytes(st, B, h, w, up):
    n = 0
    for blk in st["blocks"]:
        for ci, co in blk["resnets"]:
            n += _resnet_saved_bytes(B * h * w, B, ci, co)
        if blk["resample"]:
            n += B * h * w * blk["resnets"][-1][1] * 2                    # the resampling layer's bf16 operand
            h, w = (2 * h, 2 * w) if up else (h // 2, w // 2)
    return n, h, w


def encoder_saved_bytes(params_or_config, B, H, W):
    """Bytes encoder_forward_train's `saved` holds for a [B, 3, H, W] batch (the image included).  params_or_config: the parameters (tensors or
    shapes under `encoder.*`) or the keywords of synth.encoder_manifest."""
    st = _structure_of(params_or_config, "encoder.")
    n, h, w = _blocks_saved_bytes(st, B, H, W, False)
    C = st["mid"]
    return B * 3 * H * W * 4 + n + _mid_saved_bytes(B, h * w, C) + B * h * w * C * (4 + 2) + B * GROUPS * 2 * 4


def decoder_saved_bytes(params_or_config, B, h, w):
    """Bytes decoder_forward_train's `saved` holds for [B, L, h, w] latents.  params_or_config as in encoder_saved_bytes (`decoder.*`,
    synth.image_decoder_manifest)."""
    st = _structure_of(params_or_config, "decoder.")
    C = st["mid"]
    n = B * h * w * WGRAD_C * 2 + _mid_saved_bytes(B, h * w, C)
    m, H, W = _blocks_saved_bytes(st, B, h, w, True)
    return n + m + B * H * W * st["blocks"][-1]["resnets"][-1][1] * (4 + 2) + B * GROUPS * 2 * 4


# ---- one step of train_vae: the three encodes, the anchor's decode, the loss and all 244 gradients --------------------------------------

DECODE_DRAW, TRIPLET_DRAWS = 0, (1, 2, 3)       # evaluate_vae's convention: the decoded latent is draw 0, the triplet's latents draws 1, 2, 3


def vae_loss_and_grads(params, anchor, positive, negative, labels_a=None, labels_p=None, *, weights, margin=1.0, similarity_type="cosine", seed=0,
                       first_image=0, splits=0, saved=None, boundaries=None, moments_out=None):
    """The training loss of train_vae.py (lines 131-179 of the reference; vae_losses.loss_backward_device) on one batch and its gradient in every
    parameter.  params: all `encoder.*` and `decoder.*` tensors (fp32, diffusers' names); anchor / positive / negative fp32 NCHW [B, 3, H, W]; labels
    [B, N] fp32 or uint8 / bool, or None; weights: {"reconstruction", "kl", "triplet"} (the simplified loss is kl = 0).
    -> (losses, grads): losses {"reconstruction", "kl", "triplet", "total"}, 0-d float64 device tensors (no synchronisation); grads fp32, keyed and
    ordered like params.  One encoder pass on the 3B images [a; p; n] (GroupNorm is per image: the reference's three calls), the anchor's latent
    (draw 0) decoded, nothing decoded from the positive or the negative, no scaling or shift factor -- as the reference's VAE wrapper.
    saved (optional dict) receives what the step keeps between its forward and its backward: "encoder", "decoder", "moments", "z", "recon"
    (vae_train_saved_bytes); boundaries (optional dict) the two models' own, under "decoder" and "encoder", and "dz" (fp32 NCHW); moments_out
    (optional list) is appended the encoder pass's moments [3B, 2L, h, w] (train_full's classifier reads the anchors' means from them)."""
    from . import vae_losses
    a = _nchw3(anchor, "anchor")
    ctx = context(a.device)
    ctx.call("vt_op_backward_operands_check")
    if negative is None:
        raise ValueError("a negative stream is required: the contrastive term has no gradient here")
    if positive.shape != a.shape or negative.shape != a.shape:
        raise ValueError("anchor, positive and negative are [B, 3, H, W] tensors of one shape")
    enc = {k: v for k, v in params.items() if k.startswith("encoder.")}
    dec = {k: v for k, v in params.items() if k.startswith("decoder.")}
    if len(enc) + len(dec) != len(params) or not enc or not dec:
        raise ValueError("params holds the encoder.* and the decoder.* tensors and nothing else")
    B = a.shape[0]
    moments, saved_e = encoder_forward_train(enc, torch.cat([a, _nchw3(positive, "positive"), _nchw3(negative, "negative")]))
    if moments_out is not None:
        moments_out.append(moments)
    L, h, w = moments.shape[1] // 2, moments.shape[2], moments.shape[3]
    z = torch.empty(B, L, h, w, dtype=torch.float32, device=a.device)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    ctx.call("vt_posterior_sample", _vp(moments), B, L, h * w, seed, DECODE_DRAW, int(first_image), _vp(z), None, _stream(z))
    recon, saved_d = decoder_forward_train(dec, z)
    if recon.shape != a.shape:
        raise ValueError(f"the decoder gives {tuple(recon.shape)} images for {tuple(a.shape)} inputs: the two models' resampling levels differ")
    if saved is not None:
        saved.update({"encoder": saved_e, "decoder": saved_d, "moments": moments, "z": z, "recon": recon})
    streams = [(moments[i * B:(i + 1) * B], d) for i, d in enumerate(TRIPLET_DRAWS)]
    common = dict(weights=weights, margin=margin, similarity_type=similarity_type, seed=seed, first_image=first_image, recon=recon, target=a, context=ctx)
    d_recon = torch.empty_like(recon)
    vae_losses.loss_backward_device(*streams, d_recon=d_recon, **common)
    at = boundaries if boundaries is not None else {}
    at["decoder"], at["encoder"] = {}, {}
    at["dz"], g = decoder_backward(dec, saved_d, d_recon, splits=splits, boundaries=at["decoder"])
    dz = at["dz"]
    d_moments = torch.empty_like(moments)
    loss_out = torch.empty(4, dtype=torch.float64, device=a.device)
    vae_losses.loss_backward_device(*streams, dz_dec=dz, dz_draw=DECODE_DRAW, labels_a=labels_a, labels_p=labels_p,
                                    d_moments=[d_moments[i * B:(i + 1) * B] for i in range(3)], loss_out=loss_out, **common)
    ge = encoder_backward(enc, saved_e, d_moments, splits=splits, boundaries=at["encoder"])
    return dict(zip(vae_losses.LOSS_NAMES, loss_out.unbind())), _grads_like(params, ("", g), ("", ge))


def vae_triplet_loss_and_grads(params, anchor, positive, negative, labels_a=None, labels_p=None, *, triplet_weight=1.0, margin=1.0,
                               similarity_type="cosine", seed=0, first_image=0, splits=0, saved=None, moments_out=None):
    """The VAE side of train_full's simplified loss (the reference's train_full.py:227-234 with SimplifiedCombinedLoss, improved_losses.py:160-193):
    triplet_weight x the triplet loss on the three sampled latents and nothing else.  The reconstruction never enters that loss, so every `decoder.*`
    tensor has no gradient there; here nothing is decoded: one encoder pass on [a; p; n], one vt_vae_loss_backward without recon, target, dz_dec or
    d_recon and with kl = 0, one encoder backward.  params: the `encoder.*` tensors (others are ignored and get no gradient).
    -> (losses, grads): losses as vae_loss_and_grads' (reconstruction is 0, kl the monitored value, total = triplet_weight x triplet); grads fp32 of
    the `encoder.*` tensors ONLY, keyed and ordered like them -- bit for bit vae_loss_and_grads' at weights {reconstruction 0, kl 0, triplet
    triplet_weight} with the same seed and first_image.  saved (optional dict) receives "encoder" and "moments" (vae_triplet_saved_bytes);
    moments_out (optional list) is appended the moments [3B, 2L, h, w]."""
    from . import vae_losses
    a = _nchw3(anchor, "anchor")
    ctx = context(a.device)
    ctx.call("vt_op_backward_operands_check")
    if negative is None:
        raise ValueError("a negative stream is required: the contrastive term has no gradient here")
    if positive.shape != a.shape or negative.shape != a.shape:
        raise ValueError("anchor, positive and negative are [B, 3, H, W] tensors of one shape")
    enc = {k: v for k, v in params.items() if k.startswith("encoder.")}
    if not enc:
        raise ValueError("params holds no encoder.* tensor")
    B = a.shape[0]
    moments, saved_e = encoder_forward_train(enc, torch.cat([a, _nchw3(positive, "positive"), _nchw3(negative, "negative")]))
    if moments_out is not None:
        moments_out.append(moments)
    if saved is not None:
        saved.update({"encoder": saved_e, "moments": moments})
    streams = [(moments[i * B:(i + 1) * B], d) for i, d in enumerate(TRIPLET_DRAWS)]
    d_moments = torch.empty_like(moments)
    loss_out = torch.empty(4, dtype=torch.float64, device=a.device)
    vae_losses.loss_backward_device(*streams, weights={"reconstruction": 0.0, "kl": 0.0, "triplet": float(triplet_weight)}, margin=margin,
                                    similarity_type=similarity_type, seed=int(seed) & 0xFFFFFFFFFFFFFFFF, first_image=first_image, labels_a=labels_a,
                                    labels_p=labels_p, d_moments=[d_moments[i * B:(i + 1) * B] for i in range(3)], loss_out=loss_out, context=ctx)
    ge = encoder_backward(enc, saved_e, d_moments, splits=splits)
    return dict(zip(vae_losses.LOSS_NAMES, loss_out.unbind())), ge


def vae_triplet_saved_bytes(params_or_config, B, H, W):
    """Bytes vae_triplet_loss_and_grads keeps between its forward and its backward for a [B, 3, H, W] batch: the encoder's `saved` at 3B images and
    the moments (3B) -- no decoded latent, no reconstruction, nothing of the image decoder.  params_or_config as in vae_train_saved_bytes."""
    if not params_or_config:
        from . import synth
        params_or_config = synth.encoder_manifest()
    st = _structure_of(_only(params_or_config, "encoder."), "encoder.")
    levels = sum(1 for blk in st["blocks"] if blk["resample"])
    h, w, L = H >> levels, W >> levels, st["conv_out"][0] // 2
    return encoder_saved_bytes(_only(params_or_config, "encoder."), 3 * B, H, W) + 3 * B * 2 * L * h * w * 4


def vae_train_saved_bytes(params_or_config, B, H, W):
    """Bytes vae_loss_and_grads keeps between its forward and its backward for a [B, 3, H, W] batch: the encoder's `saved` at 3B images, the decoder's at
    B latents, and its own moments (3B), decoded latent and reconstruction.  params_or_config: the parameters (tensors or shapes) or the keywords
    synth.encoder_manifest and synth.image_decoder_manifest share; an empty dict is those manifests' defaults, the FLUX configuration."""
    if not params_or_config:
        from . import synth
        params_or_config = {**synth.encoder_manifest(), **synth.image_decoder_manifest()}
    st = _structure_of(_only(params_or_config, "encoder."), "encoder.")
    levels = sum(1 for blk in st["blocks"] if blk["resample"])
    h, w, L = H >> levels, W >> levels, st["conv_out"][0] // 2
    own = (3 * B * 2 * L * h * w + B * L * h * w + B * 3 * H * W) * 4
    return encoder_saved_bytes(_only(params_or_config, "encoder."), 3 * B, H, W) + decoder_saved_bytes(_only(params_or_config, "decoder."), B, h, w) + own


def _only(params_or_config, prefix):
    if "block_out" in params_or_config or "layers_per_block" in params_or_config:
        return params_or_config
    return {k: v for k, v in params_or_config.items() if k.startswith(prefix)}
