"""Test helper: torch-CPU fp32 restatement of Upsample2D's fold (nearest 2x + conv3x3 == four 2x2 phase convs of the low-resolution
input with pre-summed weights), as conv3x3_up2.hip computes it.  The tests form their expected values with it."""
import torch
import torch.nn.functional as F

# taps ky of the 3x3 kernel that folded tap r of phase a collects (rows; the same table serves columns with b, kx)
FOLD_TAPS = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}


def fold_weights(w_oihw):
    """[O, I, 3, 3] fp32 -> [2, 2, O, I, 2, 2] indexed (a, b, o, i, ry, rx): fp32 sums taken ky-major, kx inside, left to right --
    the order of the device packer, so that the sum is the same fp32 number before its one rounding."""
    w = w_oihw.to(torch.float32)
    O, I = w.shape[:2]
    out = torch.zeros(2, 2, O, I, 2, 2, dtype=torch.float32)
    for a in range(2):
        for b in range(2):
            for ry in range(2):
                for rx in range(2):
                    s = None
                    for ky in FOLD_TAPS[(a, ry)]:
                        for kx in FOLD_TAPS[(b, rx)]:
                            s = w[:, :, ky, kx].clone() if s is None else s + w[:, :, ky, kx]
                    out[a, b, :, :, ry, rx] = s
    return out


def folded_upsample_conv(x_nchw, w_oihw, bias=None, round_fn=None):
    """conv3x3(nearest_2x(x)) evaluated through the fold; round_fn rounds the FOLDED weights (to the operand type) when given."""
    wf = fold_weights(w_oihw)
    if round_fn is not None:
        wf = round_fn(wf)
    B, _, h, w = x_nchw.shape
    out = torch.zeros(B, w_oihw.shape[0], 2 * h, 2 * w, dtype=torch.float32)
    for a in range(2):
        for b in range(2):
            # folded tap (ry, rx) of phase (a, b) reads low-resolution pixel (i + ry - 1 + a, j + rx - 1 + b)
            xp = F.pad(x_nchw, (1 - b, b, 1 - a, a))
            out[:, :, a::2, b::2] = F.conv2d(xp, wf[a, b])
    if bias is not None:
        out = out + bias.view(1, -1, 1, 1)
    return out


def literal_upsample_conv(x_nchw, w_oihw, bias=None):
    return F.conv2d(F.interpolate(x_nchw, scale_factor=2, mode="nearest"), w_oihw, bias, padding=1)


# ---- the whole image decoder ----------------------------------------------------------------------
# torch-CPU fp32 restatement of diffusers' Decoder over the `decoder.*` keys (conv_in, UNetMidBlock2D, UpDecoderBlock2D x N with
# Upsample2D, conv_norm_out / SiLU / conv_out).  PARITY UNPINNED against real diffusers, exactly as oracle/encoder_ref.py's encoder is:
# `diffusers` is not installed and the reference holds no decoder fixtures; the parameter count (49 545 475) and the key manifest pin the
# wiring.  `operands` = None (fp32), "bf16" or "fp16" rounds every conv / linear / attention matmul operand the way encoder_ref._Q does.
import math

GN_GROUPS, GN_EPS = 32, 1e-6


class _Q:
    def __init__(self, operands):
        self.dt = {None: None, "bf16": torch.bfloat16, "fp16": torch.float16}[operands]

    def __call__(self, t):
        return t if self.dt is None else t.to(self.dt).to(torch.float32)


def _gn(x, sd, name, q, silu):
    y = F.group_norm(x, GN_GROUPS, sd[name + ".weight"], sd[name + ".bias"], GN_EPS)
    return q(F.silu(y) if silu else y)


def _conv(x, sd, name, q, padding=1):
    return F.conv2d(x, q(sd[name + ".weight"]), sd[name + ".bias"], padding=padding)


def _resnet(h, sd, p, q):
    t = _gn(h, sd, p + ".norm1", q, True)
    t = q(_conv(t, sd, p + ".conv1", q))
    t = _gn(t, sd, p + ".norm2", q, True)
    t = _conv(t, sd, p + ".conv2", q)
    s = _conv(q(h), sd, p + ".conv_shortcut", q, padding=0) if (p + ".conv_shortcut.weight") in sd else h
    return t + s


def _attention(h, sd, p, q):
    b, c, hh, ww = h.shape
    x = q(F.group_norm(h, GN_GROUPS, sd[p + ".group_norm.weight"], sd[p + ".group_norm.bias"], GN_EPS)).reshape(b, c, hh * ww).transpose(1, 2)
    qq = q(F.linear(x, q(sd[p + ".to_q.weight"]), sd[p + ".to_q.bias"]))
    kk = q(F.linear(x, q(sd[p + ".to_k.weight"]), sd[p + ".to_k.bias"]))
    vv = q(F.linear(x, q(sd[p + ".to_v.weight"]), sd[p + ".to_v.bias"]))
    probs = torch.softmax(torch.matmul(qq, kk.transpose(1, 2)) * (1.0 / math.sqrt(c)), dim=-1)
    o = q(torch.matmul(q(probs), vv))
    o = F.linear(o, q(sd[p + ".to_out.0.weight"]), sd[p + ".to_out.0.bias"])
    return o.transpose(1, 2).reshape(b, c, hh, ww) + h


def decode_image(sd, z, n_blocks=4, layers_per_block=2, operands=None, taps=None):
    """z fp32 [B, latent, h, w] -> image fp32 [B, out, h * 2^(n_blocks-1), w * 2^(n_blocks-1)] (AutoencoderKL.decode(z).sample)"""
    q = _Q(operands)
    sd = {k: v.to(torch.float32) for k, v in sd.items() if k.startswith("decoder.")}
    h = _conv(q(z), sd, "decoder.conv_in", q)
    h = _resnet(h, sd, "decoder.mid_block.resnets.0", q)
    h = _attention(h, sd, "decoder.mid_block.attentions.0", q)
    h = _resnet(h, sd, "decoder.mid_block.resnets.1", q)
    if taps is not None:
        taps["mid"] = h
    for i in range(n_blocks):
        for j in range(layers_per_block + 1):
            h = _resnet(h, sd, f"decoder.up_blocks.{i}.resnets.{j}", q)
        u = f"decoder.up_blocks.{i}.upsamplers.0.conv"
        if (u + ".weight") in sd:
            h = _conv(F.interpolate(q(h), scale_factor=2.0, mode="nearest"), sd, u, q)
        if taps is not None:
            taps[f"up{i}"] = h
    h = _gn(h, sd, "decoder.conv_norm_out", q, True)
    return _conv(h, sd, "decoder.conv_out", q)
