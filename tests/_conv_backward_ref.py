"""CPU restatements of the resnet block's backward (NCHW, any float dtype), written against torch.nn.functional.  tests/test_conv_backward_host.py
checks them against autograd in fp64; tests/test_conv_backward_device.py leans on them."""
import torch
import torch.nn.functional as F

GROUPS, EPS = 32, 1e-6


def ident(t):
    return t


def bf16_round_keep(t):
    """round to bf16, keep the dtype (fp64 stays fp64: the device's rounding points inside an fp64 evaluation)"""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def dgrad_ref(dy, w):
    """data gradient of a stride-1 conv (3x3 pad 1 or 1x1) as the FORWARD conv of dy with the weights rotated by 180 degrees and transposed"""
    k = w.shape[2]
    return F.conv2d(dy, w.flip(2, 3).transpose(0, 1).contiguous(), padding=k // 2)


def wgrad_ref(dy, a, ksize, slices=1):
    """dW[co][ci][ky][kx] = sum_p dy[p][co] a[p + (ky - 1, kx - 1)][ci]; the pixels p = (b, y, x) cut into `slices` contiguous runs, each run's
    partial summed in run order"""
    B, Cout, H, W = dy.shape
    Cin, h = a.shape[1], ksize // 2
    ap = F.pad(a, (h, h, h, h))
    n = B * H * W
    total = None
    for s in range(slices):
        lo, hi = s * n // slices, (s + 1) * n // slices
        mask = torch.zeros(n, dtype=dy.dtype)
        mask[lo:hi] = 1
        d = dy * mask.view(B, 1, H, W)
        part = torch.empty(Cout, Cin, ksize, ksize, dtype=dy.dtype)
        for ky in range(ksize):
            for kx in range(ksize):
                part[:, :, ky, kx] = torch.einsum("bohw,bihw->oi", d, ap[:, :, ky:ky + H, kx:kx + W])
        total = part if total is None else total + part
    return total


def gn_stats_ref(x, groups=GROUPS, eps=EPS):
    B, C = x.shape[:2]
    xg = x.reshape(B, groups, -1)
    mean = xg.mean(dim=2)
    var = xg.var(dim=2, unbiased=False)
    return mean, (var + eps).rsqrt()


def gn_silu_backward_ref(x, gamma, beta, da, groups=GROUPS, eps=EPS, dx_add=None):
    """backward of a = silu(group_norm(x)) by the formulas of the operator's contract -> (dx, dgamma, dbeta)"""
    B, C = x.shape[:2]
    mean, rstd = gn_stats_ref(x, groups, eps)
    cpg = C // groups
    mu = mean.repeat_interleave(cpg, dim=1).view(B, C, 1, 1)
    r = rstd.repeat_interleave(cpg, dim=1).view(B, C, 1, 1)
    g, bt = gamma.view(1, C, 1, 1), beta.view(1, C, 1, 1)
    xh = (x - mu) * r
    u = g * xh + bt
    s = torch.sigmoid(u)
    du = da * s * (1 + u * (1 - s))
    dbeta = du.sum(dim=(0, 2, 3))
    dgamma = (du * xh).sum(dim=(0, 2, 3))
    dxh = du * g
    shp = x.shape

    def gmean(t):
        return t.reshape(B, groups, -1).mean(dim=2).repeat_interleave(cpg, dim=1).view(B, C, 1, 1)

    dx = r * (dxh - gmean(dxh) - xh * gmean(dxh * xh))
    if dx_add is not None:
        dx = dx + dx_add
    return dx.view(shp), dgamma, dbeta


def block_forward_ref(p, x, rnd=ident):
    """functional ResnetBlock2D; rnd is applied where the device rounds a conv operand (activations and weights) -> (y, saved)"""
    a1 = rnd(F.silu(F.group_norm(x, GROUPS, p["norm1.weight"], p["norm1.bias"], EPS)))
    h1 = F.conv2d(a1, rnd(p["conv1.weight"]), p["conv1.bias"], padding=1)
    a2 = rnd(F.silu(F.group_norm(h1, GROUPS, p["norm2.weight"], p["norm2.bias"], EPS)))
    saved = {"x": x, "a1": a1, "h1": h1, "a2": a2}
    if "conv_shortcut.weight" in p:
        saved["x16"] = rnd(x)
        res = F.conv2d(saved["x16"], rnd(p["conv_shortcut.weight"]), p["conv_shortcut.bias"])
    else:
        res = x
    return F.conv2d(a2, rnd(p["conv2.weight"]), p["conv2.bias"], padding=1) + res, saved


def block_backward_ref(p, saved, dy, rnd=ident):
    """the block's backward in the operators' order, rnd at the device's rounding points (dy16, dh1's bf16 copy, the weights) -> (dx, grads)"""
    g = {}
    dy16 = rnd(dy)
    g["conv2.bias"] = dy.sum(dim=(0, 2, 3))
    g["conv2.weight"] = wgrad_ref(dy16, saved["a2"], 3)
    da2 = dgrad_ref(dy16, rnd(p["conv2.weight"]))
    dh1, g["norm2.weight"], g["norm2.bias"] = gn_silu_backward_ref(saved["h1"], p["norm2.weight"], p["norm2.bias"], da2)
    dh1_16 = rnd(dh1)
    g["conv1.weight"] = wgrad_ref(dh1_16, saved["a1"], 3)
    g["conv1.bias"] = dh1.sum(dim=(0, 2, 3))
    da1 = dgrad_ref(dh1_16, rnd(p["conv1.weight"]))
    if "x16" in saved:
        dxs = dgrad_ref(dy16, rnd(p["conv_shortcut.weight"]))
        g["conv_shortcut.weight"] = wgrad_ref(dy16, saved["x16"], 1)
        g["conv_shortcut.bias"] = g["conv2.bias"].clone()
    else:
        dxs = dy
    dx, g["norm1.weight"], g["norm1.bias"] = gn_silu_backward_ref(saved["x"], p["norm1.weight"], p["norm1.bias"], da1, dx_add=dxs)
    return dx, {k: g[k] for k in p}


def block_params(cin, cout, seed, dtype=torch.float64):
    gen = torch.Generator().manual_seed(seed)

    def rn(*shape, scale=1.0):
        return (scale * torch.randn(*shape, generator=gen, dtype=torch.float64)).to(dtype)

    p = {"norm1.weight": 1 + 0.2 * rn(cin), "norm1.bias": 0.2 * rn(cin), "conv1.weight": rn(cout, cin, 3, 3, scale=(9 * cin) ** -0.5),
         "conv1.bias": 0.1 * rn(cout), "norm2.weight": 1 + 0.2 * rn(cout), "norm2.bias": 0.2 * rn(cout),
         "conv2.weight": rn(cout, cout, 3, 3, scale=(9 * cout) ** -0.5), "conv2.bias": 0.1 * rn(cout)}
    if cin != cout:
        p["conv_shortcut.weight"] = rn(cout, cin, 1, 1, scale=cin ** -0.5)
        p["conv_shortcut.bias"] = 0.1 * rn(cout)
    return p


def block_autograd(p, x, dy):
    """autograd of the functional block in x's dtype, no rounding -> (y, dx, grads)"""
    q = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    xr = x.detach().clone().requires_grad_(True)
    y, _ = block_forward_ref(q, xr)
    grads = torch.autograd.grad(y, [xr] + [q[k] for k in p], dy)
    return y.detach(), grads[0], dict(zip(p.keys(), grads[1:]))
