"""CPU restatements of the mid-block attention and its backward (tokens [B, S, C] = the NHWC pixels, any float dtype).  `rnd` is applied where the
device rounds to bf16; with rnd = ident the restatement is the exact gradient (tests/test_attention_backward_host.py checks it against fp64
autograd), with rnd = bf16_round_keep it is the device's arithmetic up to summation order (tests/test_attention_backward_device.py leans on it)."""
import torch
import torch.nn.functional as F

from _conv_backward_ref import EPS, GROUPS, bf16_round_keep, ident  # noqa: F401

ATTN_PARAMS = ["group_norm.weight", "group_norm.bias", "to_q.weight", "to_q.bias", "to_k.weight", "to_k.bias", "to_v.weight", "to_v.bias",
               "to_out.0.weight", "to_out.0.bias"]


def attn_params(C, seed, dtype=torch.float64, gain=1.0):
    gen = torch.Generator().manual_seed(seed)

    def rn(*shape, scale=1.0):
        return (scale * torch.randn(*shape, generator=gen, dtype=torch.float64)).to(dtype)

    p = {"group_norm.weight": 1 + 0.2 * rn(C), "group_norm.bias": 0.2 * rn(C)}
    for name in ("to_q", "to_k", "to_v", "to_out.0"):
        g = gain if name in ("to_q", "to_k") else 1.0
        p[name + ".weight"] = g * rn(C, C, scale=C ** -0.5)
        p[name + ".bias"] = g * 0.1 * rn(C)
    return {k: p[k] for k in ATTN_PARAMS}


def group_norm_tokens(x, gamma, beta, groups=GROUPS, eps=EPS):
    """x [B, S, C] -> (h, xh, rstd [B, 1, C])"""
    B, S, C = x.shape
    xg = x.reshape(B, S, groups, C // groups)
    mean = xg.mean(dim=(1, 3), keepdim=True)
    var = xg.var(dim=(1, 3), unbiased=False, keepdim=True)
    rstd = (var + eps).rsqrt()
    xh = ((xg - mean) * rstd).reshape(B, S, C)
    return xh * gamma + beta, xh, rstd.expand(B, 1, groups, C // groups).reshape(B, 1, C)


def gn_backward_ref(x, gamma, beta, dh, groups=GROUPS, eps=EPS, dx_add=None):
    """backward of h = group_norm(x) (no activation), tokens [B, S, C] -> (dx, dgamma, dbeta)"""
    B, S, C = x.shape
    _, xh, rstd = group_norm_tokens(x, gamma, beta, groups, eps)
    dbeta, dgamma = dh.sum(dim=(0, 1)), (dh * xh).sum(dim=(0, 1))
    dxh = dh * gamma

    def gmean(t):
        return t.reshape(B, S, groups, C // groups).mean(dim=(1, 3), keepdim=True).expand(B, S, groups, C // groups).reshape(B, S, C)

    dx = rstd * (dxh - gmean(dxh) - xh * gmean(dxh * xh))
    return (dx if dx_add is None else dx + dx_add), dgamma, dbeta


def core_forward_ref(q, k, v, rnd=ident):
    """o = softmax(q k^T / sqrt(C)) v as the device evaluates it: numerators exp(s - c) rounded, their fp32 sum taken before the rounding, o rounded"""
    alpha = q.shape[-1] ** -0.5
    s = alpha * q @ k.transpose(1, 2)
    c = s.max(dim=-1, keepdim=True).values
    e = torch.exp(s - c)
    tot = e.sum(dim=-1, keepdim=True)
    o = rnd((rnd(e) @ v) / tot)
    return o, dict(e=e, tot=tot, c=c)


def core_backward_ref(q, k, v, o, do, sv, rnd=ident):
    """dq, dk, dv by the operator's formulas, rnd at do16, the numerators, ds, and p (then ds^T) of the key direction"""
    alpha = q.shape[-1] ** -0.5
    e, tot = sv["e"], sv["tot"]
    Dv = (do * o).sum(dim=-1, keepdim=True)
    do16 = rnd(do)
    dp = do16 @ v.transpose(1, 2)
    ds = rnd(alpha * (rnd(e) / tot) * (dp - Dv))                    # query direction
    dq = ds @ k
    pk = rnd(e / tot)                                               # key direction
    dv = pk.transpose(1, 2) @ do16
    dsk = rnd(alpha * pk * (dp - Dv))
    dk = dsk.transpose(1, 2) @ q
    return dq, dk, dv


def core_autograd(q, k, v, do):
    """autograd of the unrounded core in the inputs' dtype -> (o, dq, dk, dv)"""
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    o = torch.softmax(q @ k.transpose(1, 2) * q.shape[-1] ** -0.5, dim=-1) @ v
    return (o.detach(),) + tuple(torch.autograd.grad(o, [q, k, v], do))


def block_forward_ref(p, x, rnd=ident):
    """functional attention block on tokens x [B, S, C] -> (y, saved)"""
    h = rnd(group_norm_tokens(x, p["group_norm.weight"], p["group_norm.bias"])[0])
    q, k, v = (rnd(h @ rnd(p[n + ".weight"]).t() + p[n + ".bias"]) for n in ("to_q", "to_k", "to_v"))
    o, sv = core_forward_ref(q, k, v, rnd)
    y = o @ rnd(p["to_out.0.weight"]).t() + p["to_out.0.bias"] + x
    return y, dict(sv, x=x, h=h, q=q, k=k, v=v, o=o)


def block_backward_ref(p, saved, dy, rnd=ident):
    """the block's backward in the operators' order -> (dx, grads keyed like p)"""
    g = {}
    C = dy.shape[-1]
    dy16 = rnd(dy)
    g["to_out.0.bias"] = dy.sum(dim=(0, 1))
    g["to_out.0.weight"] = dy16.reshape(-1, C).t() @ saved["o"].reshape(-1, C)
    do = dy16 @ rnd(p["to_out.0.weight"])
    grads = core_backward_ref(saved["q"], saved["k"], saved["v"], saved["o"], do, saved, rnd)
    dh = 0
    for name, d in zip(("to_q", "to_k", "to_v"), grads):
        d16 = rnd(d)
        g[name + ".weight"] = d16.reshape(-1, C).t() @ saved["h"].reshape(-1, C)
        g[name + ".bias"] = d.sum(dim=(0, 1))
        dh = dh + d16 @ rnd(p[name + ".weight"])
    dx, g["group_norm.weight"], g["group_norm.bias"] = gn_backward_ref(saved["x"], p["group_norm.weight"], p["group_norm.bias"], dh, dx_add=dy)
    return dx, {k: g[k] for k in p}


def block_autograd(p, x, dy):
    """autograd of the unrounded block in x's dtype -> (y, dx, grads)"""
    q = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    xr = x.detach().clone().requires_grad_(True)
    B, S, C = x.shape
    h = F.group_norm(xr.transpose(1, 2), GROUPS, q["group_norm.weight"], q["group_norm.bias"], EPS).transpose(1, 2)
    qq, kk, vv = (h @ q[n + ".weight"].t() + q[n + ".bias"] for n in ("to_q", "to_k", "to_v"))
    o = torch.softmax(qq @ kk.transpose(1, 2) * C ** -0.5, dim=-1) @ vv
    y = o @ q["to_out.0.weight"].t() + q["to_out.0.bias"] + xr
    grads = torch.autograd.grad(y, [xr] + [q[k] for k in p], dy)
    return y.detach(), grads[0], dict(zip(p.keys(), grads[1:]))
