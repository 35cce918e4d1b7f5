"""fp64 CPU reference of one conv of a ResnetBlock2D / Downsample2D as vt_op_conv3x3_block runs it: 3x3 conv (stride 1 pad 1, or stride 2 pad
(0,1,0,1)) + bias + optional 1x1 shortcut conv at the same pixel + optional residual, and what the kernels store of that sum.  Plain torch on
the CPU, nothing of the library.  Tensors are NHWC; the operands arrive already rounded to their 16-bit type, the residual to its storage type.
tests/test_conv_block_host.py checks this file against torch.nn.functional.conv2d."""
import torch


def planar_pack(t):
    """NHWC [B][H][W][C] -> chunk-planar [B][C/32][H][W][32] (Conv3x3Args::out16_planar, Conv3x3S2Args::x_planar)"""
    B, H, W, C = t.shape
    assert C % 32 == 0
    return t.reshape(B, H, W, C // 32, 32).permute(0, 3, 1, 2, 4).contiguous()


def planar_unpack(p):
    """chunk-planar [B][C/32][H][W][32] -> NHWC [B][H][W][C]"""
    B, n, H, W, k = p.shape
    assert k == 32
    return p.permute(0, 2, 3, 1, 4).reshape(B, H, W, n * 32).contiguous()


def conv_sum(x, w, bias, stride=1, sc_x=None, sc_w=None, residual=None):
    """x [B][H][W][Cin], w OIHW [Cout][Cin][3][3], bias [Cout], sc_x [B][H][W][scCin], sc_w [Cout][scCin], residual [B][Ho][Wo][Cout] -> the fp64
    sum [B][Ho][Wo][Cout], one tap at a time: out[y][x] += in[stride y + ky - pad][stride x + kx - pad] . w[:, :, ky, kx]."""
    assert stride in (1, 2)
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    Ho, Wo = (H, W) if stride == 1 else (H // 2, W // 2)
    lo = 1 if stride == 1 else 0                           # stride 2 pads (0, 1, 0, 1): nothing above / left, one row / column below / right
    xp = torch.zeros(B, H + 2, W + 2, Cin, dtype=torch.float64)
    xp[:, lo:lo + H, lo:lo + W] = x.double()
    wd = w.double()
    v = bias.double().view(1, 1, 1, Cout).expand(B, Ho, Wo, Cout).clone()
    for ky in range(3):
        for kx in range(3):
            win = xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            v += win @ wd[:, :, ky, kx].t()
    if sc_x is not None:
        assert stride == 1
        v += sc_x.double() @ sc_w.double().t()
    if residual is not None:
        v += residual.double()
    return v


def group_norm(v, groups, gamma, beta, eps=1e-6):
    """GroupNorm of NHWC v in fp64 (biased variance over H, W and the group's channels)"""
    B, H, W, C = v.shape
    g = v.double().reshape(B, H * W, groups, C // groups)
    mean = g.mean(dim=(1, 3), keepdim=True)
    var = ((g - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    n = ((g - mean) / torch.sqrt(var + eps)).reshape(B, H, W, C)
    return n * gamma.double().view(1, 1, 1, C) + beta.double().view(1, 1, 1, C)


def conv_block_ref(x, w, bias, stride=1, sc_x=None, sc_w=None, residual=None, copy_f16=False, groups=None, gamma=None, beta=None, eps=1e-6):
    """-> dict: v (fp64 sum), f16 = fp16(v), copy = bf16(v) or fp16(v) (copy_f16), copy_planar = the copy chunk-planar, gn = group_norm(v) when
    groups is given.  (The 16-bit roundings go through fp32, as the device's do: its stores round an fp32 accumulator.)"""
    v = conv_sum(x, w, bias, stride, sc_x, sc_w, residual)
    v32 = v.float()
    copy = v32.to(torch.float16 if copy_f16 else torch.bfloat16)
    r = {"v": v, "f16": v32.to(torch.float16), "copy": copy, "copy_planar": planar_pack(copy)}
    if groups is not None:
        r["gn"] = group_norm(v, groups, gamma, beta, eps)
    return r
