"""CPU restatements of the two resampling layers' backward (NCHW, any float dtype): the phase formulations the device kernels run, the literal routes,
and the down / up blocks.  tests/test_resample_backward_host.py checks them against autograd in fp64; tests/test_resample_backward_device.py leans on
them.

Downsample2D: y = conv3x3(pad(x, (0,1,0,1)), W), stride 2.  Upsample2D: y = conv3x3(nearest2x(x), W), stride 1, pad 1."""
import torch
import torch.nn.functional as F

from _conv_backward_ref import block_backward_ref, block_forward_ref, block_params, dgrad_ref, ident

# ---- Downsample2D ---------------------------------------------------------------------------------------------------------------------------------
S2_TAPS = {0: ((0, 0), (2, -1)), 1: ((1, 0),)}        # output parity -> ((tap, dy offset), ...): row 2i takes ky 0 from dy row i and ky 2 from row i - 1


def down_forward_ref(x, w, bias=None):
    return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, bias, stride=2)


def s2_dgrad_phase_ref(dy, w, H, W):
    """the 9-product data gradient, by the parity of the dx pixel; dy outside [0, H // 2) x [0, W // 2) counts as 0"""
    B, Cout, Ho, Wo = dy.shape
    assert (Ho, Wo) == (H // 2, W // 2)
    Hq, Wq = (H + 1) // 2, (W + 1) // 2                    # quads, the last one ragged for odd sizes
    dyp = F.pad(dy, (1, Wq - Wo, 1, Hq - Ho))
    dx = torch.zeros(B, w.shape[1], H, W, dtype=dy.dtype)
    products = 0
    for a in (0, 1):
        for b in (0, 1):
            na, nb = (H - a + 1) // 2, (W - b + 1) // 2    # pixels of this phase
            for ky, d in S2_TAPS[a]:
                for kx, e in S2_TAPS[b]:
                    dx[:, :, a::2, b::2] += torch.einsum("bohw,oi->bihw", dyp[:, :, 1 + d:1 + d + na, 1 + e:1 + e + nb], w[:, :, ky, kx])
                    products += 1
    assert products == 9
    return dx


def s2_scatter_odd(dy, H, W):
    """dy at the odd positions (2i + 1, 2j + 1) of a zeroed H x W tensor: the gradient of the stride-1 pad-1 conv's output"""
    z = torch.zeros(dy.shape[0], dy.shape[1], H, W, dtype=dy.dtype)
    z[:, :, 1::2, 1::2] = dy
    return z


def s2_dgrad_literal_ref(dy, w, H, W):
    return dgrad_ref(s2_scatter_odd(dy, H, W), w)


def s2_wgrad_ref(dy, a):
    """dW[co][ci][ky][kx] = sum dy[b][i][j][co] a[b][2i + ky][2j + kx][ci], a outside the image = 0"""
    B, Cout, Ho, Wo = dy.shape
    ap = F.pad(a, (0, 2, 0, 2))
    dw = torch.empty(Cout, a.shape[1], 3, 3, dtype=dy.dtype)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = torch.einsum("bohw,bihw->oi", dy, ap[:, :, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2])
    return dw


# ---- Upsample2D -----------------------------------------------------------------------------------------------------------------------------------
UP_FOLD = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}        # (phase, folded tap) -> the 3x3 taps it sums


def up_forward_ref(x, w, bias=None):
    return F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, bias, padding=1)


def up2_fold(w, rnd=ident):
    """the forward's 16 folded matrices Wf[a][b][ry][rx] [Cout][Cin]: the sum in w's dtype, ky-major, kx inside, left to right, then rnd once"""
    wf = torch.empty(2, 2, 2, 2, w.shape[0], w.shape[1], dtype=w.dtype)
    for (a, ry), kys in UP_FOLD.items():
        for (b, rx), kxs in UP_FOLD.items():
            s = None
            for ky in kys:
                for kx in kxs:
                    s = w[:, :, ky, kx].clone() if s is None else s + w[:, :, ky, kx]
            wf[a, b, ry, rx] = rnd(s)
    return wf


def up2_forward_folded_ref(x, wf):
    """phase (a, b) of the output is a 2x2 conv of the low-resolution x: folded tap ry reads row i + ry - 1 + a"""
    B, C, h, w = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    y = torch.zeros(B, wf.shape[4], 2 * h, 2 * w, dtype=x.dtype)
    for a in (0, 1):
        for b in (0, 1):
            for ry in (0, 1):
                for rx in (0, 1):
                    y[:, :, a::2, b::2] += torch.einsum("bihw,oi->bohw", xp[:, :, ry + a:ry + a + h, rx + b:rx + b + w], wf[a, b, ry, rx])
    return y


def up2_dgrad_gather_ref(dy, wf):
    """the folded 16-product gather: dx[i][j] = sum Wf^T[a, b, ry, rx] . P_ab[i + 1 - ry - a][j + 1 - rx - b], P_ab[u][v] = dy[2u + a][2v + b]"""
    B, C, H2, W2 = dy.shape
    h, w = H2 // 2, W2 // 2
    dx = torch.zeros(B, wf.shape[5], h, w, dtype=dy.dtype)
    products = 0
    for a in (0, 1):
        for b in (0, 1):
            plane = F.pad(dy[:, :, a::2, b::2], (1, 1, 1, 1))
            for ry in (0, 1):
                for rx in (0, 1):
                    r0, c0 = 2 - ry - a, 2 - rx - b
                    dx += torch.einsum("bohw,oi->bihw", plane[:, :, r0:r0 + h, c0:c0 + w], wf[a, b, ry, rx])
                    products += 1
    assert products == 16
    return dx


def sum2x2(t):
    return ((t[:, :, 0::2, 0::2] + t[:, :, 0::2, 1::2]) + t[:, :, 1::2, 0::2]) + t[:, :, 1::2, 1::2]


def up2_dgrad_literal_ref(dy, w):
    """the stride-1 data gradient at 2h x 2w, then the 2x2 sum in the device's order"""
    return sum2x2(dgrad_ref(dy, w))


def up2_wgrad_ref(dy, x):
    """dW[co][ci][ky][kx] = sum_P dy[P][co] x[(P + (ky - 1, kx - 1)) >> 1][ci], the bounds tested in high-resolution coordinates"""
    B, C, H2, W2 = dy.shape
    up = F.pad(F.interpolate(x, scale_factor=2, mode="nearest"), (1, 1, 1, 1))
    dw = torch.empty(C, x.shape[1], 3, 3, dtype=dy.dtype)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = torch.einsum("bohw,bihw->oi", dy, up[:, :, ky:ky + H2, kx:kx + W2])
    return dw


# ---- a down block / an up block: two resnets (one with a channel change) and the resampling layer ---------------------------------------------------
def rs_block_params(kind, cin, cout, seed, dtype=torch.float64):
    """diffusers' names: resnets.0 (cin -> cout), resnets.1 (cout -> cout), downsamplers.0.conv / upsamplers.0.conv (cout -> cout)"""
    p = {}
    for i, (ci, co) in enumerate(((cin, cout), (cout, cout))):
        p.update({f"resnets.{i}.{k}": v for k, v in block_params(ci, co, seed=seed + i, dtype=dtype).items()})
    gen = torch.Generator().manual_seed(seed + 7)
    name = {"down": "downsamplers.0.conv.", "up": "upsamplers.0.conv."}[kind]
    p[name + "weight"] = ((9 * cout) ** -0.5 * torch.randn(cout, cout, 3, 3, generator=gen, dtype=torch.float64)).to(dtype)
    p[name + "bias"] = (0.1 * torch.randn(cout, generator=gen, dtype=torch.float64)).to(dtype)
    return p


def _parts(p):
    res = [{k[len(f"resnets.{i}."):]: v for k, v in p.items() if k.startswith(f"resnets.{i}.")} for i in range(2)]
    name = [k for k in p if "samplers" in k][0].rsplit(".", 1)[0] + "."
    return res, name


def rs_block_forward_ref(kind, p, x, rnd=ident, fold_rnd=None):
    """-> (y, saved).  rnd at the device's operand roundings; fold_rnd (up, folded route): the rounding of the folded matrices, summed in fp32 first"""
    res, name = _parts(p)
    saved = []
    for q in res:
        x, s = block_forward_ref(q, x, rnd=rnd)
        saved.append(s)
    x16 = rnd(x)
    w, bias = p[name + "weight"], p[name + "bias"]
    if kind == "down":
        y = down_forward_ref(x16, rnd(w), bias)
    elif fold_rnd is None:
        y = up_forward_ref(x16, rnd(w), bias)
    else:
        y = up2_forward_folded_ref(x16, up2_fold(w.float(), fold_rnd).to(x.dtype)) + bias.view(1, -1, 1, 1)
    saved.append(x16)
    return y, saved


def rs_block_backward_ref(kind, p, saved, dy, rnd=ident, fold_rnd=None):
    """the block's backward in the operators' order -> (dx, grads keyed like p)"""
    res, name = _parts(p)
    x16 = saved[2]
    dy16 = rnd(dy)
    g = {name + "bias": dy.sum(dim=(0, 2, 3))}
    w = p[name + "weight"]
    if kind == "down":
        g[name + "weight"] = s2_wgrad_ref(dy16, x16)
        d = s2_dgrad_phase_ref(dy16, rnd(w), x16.shape[2], x16.shape[3])
    else:
        g[name + "weight"] = up2_wgrad_ref(dy16, x16)
        d = up2_dgrad_literal_ref(dy16, rnd(w)) if fold_rnd is None else up2_dgrad_gather_ref(dy16, up2_fold(w.float(), fold_rnd).to(dy.dtype))
    for i in (1, 0):
        d, gi = block_backward_ref(res[i], saved[i], d, rnd=rnd)
        g.update({f"resnets.{i}.{k}": v for k, v in gi.items()})
    return d, {k: g[k] for k in p}


def rs_block_autograd(kind, p, x, dy):
    """autograd of the functional block in x's dtype, no rounding -> (y, dx, grads)"""
    q = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    xr = x.detach().clone().requires_grad_(True)
    y, _ = rs_block_forward_ref(kind, q, xr)
    grads = torch.autograd.grad(y, [xr] + [q[k] for k in p], dy)
    return y.detach(), grads[0], dict(zip(p.keys(), grads[1:]))
