"""CPU restatements for the VAE's end convs and whole-model backward (NCHW, any float dtype): the thin-side weight gradient in both forms, the hi + lo
split, the transpose_rotate identity, and a functional encoder / decoder under diffusers' names.  One forward serves three uses: with rnd = ident it is
the exact model (autograd in fp64 gives the reference gradients, in fp32 the e32 yardstick; oracle/encoder_ref.py casts to fp32 and cannot serve here);
with rnd = bf16_round_keep, followed by model_backward_ref, it is the device's arithmetic up to summation order, composed from the per-block
restatements of _conv_backward_ref / _attention_backward_ref / _resample_backward_ref.  tests/test_vae_model_backward_host.py checks these against
fp64 autograd; tests/test_vae_model_backward_device.py leans on them."""
import torch
import torch.nn.functional as F

import _attention_backward_ref as attn_ref
from _conv_backward_ref import (EPS, GROUPS, bf16_round_keep, block_backward_ref, block_forward_ref, dgrad_ref, gn_silu_backward_ref, ident,  # noqa: F401
                                wgrad_ref)
from _resample_backward_ref import (down_forward_ref, s2_dgrad_phase_ref, s2_wgrad_ref, up2_dgrad_gather_ref, up2_fold, up2_forward_folded_ref,
                                    up2_wgrad_ref, up_forward_ref)

DOWN, UP = "downsamplers.0.conv.", "upsamplers.0.conv."


# ---- the thin side ------------------------------------------------------------------------------------------------------------------------------------
def split_hilo(v):
    """bf16(v) + bf16(v - bf16(v)), in v's dtype: what the thin operand is to the MFMA"""
    hi = bf16_round_keep(v)
    return hi + bf16_round_keep(v - hi)


def thin_wgrad_ref(thin, wide, thin_is_input):
    """thin [B, 3, H, W], wide [B, Cw, H, W].  thin_is_input: dw[c][t][ky][kx] = sum wide[p][c] thin[t][p + (ky - 1, kx - 1)]  -> [Cw, 3, 3, 3];
    else dw[t][c][ky][kx] = sum wide[q][c] thin[t][q - (ky - 1, kx - 1)] -> [3, Cw, 3, 3].  Taps outside the image are 0."""
    B, Cw, H, W = wide.shape
    tp = F.pad(thin, (1, 1, 1, 1))
    dw = torch.empty((Cw, 3, 3, 3) if thin_is_input else (3, Cw, 3, 3), dtype=wide.dtype)
    for ky in range(3):
        for kx in range(3):
            oy, ox = (ky, kx) if thin_is_input else (2 - ky, 2 - kx)
            m = torch.einsum("bchw,bthw->ct", wide, tp[:, :, oy:oy + H, ox:ox + W])
            if thin_is_input:
                dw[:, :, ky, kx] = m
            else:
                dw[:, :, ky, kx] = m.t()
    return dw


def rotate_transpose(w):
    """conv_out's parameter [3, C, 3, 3] -> W'[c][t][ky][kx] = w[t][c][2 - ky][2 - kx], the weights of the 3 -> C conv that is conv_out's data gradient"""
    return w.flip(2, 3).transpose(0, 1).contiguous()


# ---- structure from the key names ---------------------------------------------------------------------------------------------------------------------
def split_model(p, prefix):
    blocks = "down_blocks" if prefix == "encoder." else "up_blocks"
    ends, blk, mid = {}, {}, {}
    for k, v in p.items():
        assert k.startswith(prefix), k
        r = k[len(prefix):]
        bits = r.split(".", 2)
        if bits[0] == "mid_block":
            mid[r[len("mid_block."):]] = v
        elif bits[0] == blocks:
            blk.setdefault(int(bits[1]), {})[bits[2]] = v
        else:
            ends[r] = v
    out = []
    for i in range(len(blk)):
        n = 1 + max(int(k.split(".")[1]) for k in blk[i] if k.startswith("resnets."))
        res = [{k[len(f"resnets.{j}."):]: v for k, v in blk[i].items() if k.startswith(f"resnets.{j}.")} for j in range(n)]
        rs = {k.rsplit(".", 1)[1]: v for k, v in blk[i].items() if "samplers" in k}
        out.append((res, rs or None))
    return ends, out, mid


def _sub(d, prefix):
    return {k[len(prefix):]: v for k, v in d.items() if k.startswith(prefix)}


def _tokens(x):
    B, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(B, H * W, C)


def _image(t, H, W):
    B, S, C = t.shape
    return t.reshape(B, H, W, C).permute(0, 3, 1, 2)


# ---- the functional models ----------------------------------------------------------------------------------------------------------------------------
def _mid_forward(mid, x, rnd):
    saved = {}
    x, saved["r0"] = block_forward_ref(_sub(mid, "resnets.0."), x, rnd=rnd)
    H, W = x.shape[2:]
    t, saved["attn"] = attn_ref.block_forward_ref(_sub(mid, "attentions.0."), _tokens(x), rnd=rnd)
    x, saved["r1"] = block_forward_ref(_sub(mid, "resnets.1."), _image(t, H, W), rnd=rnd)
    return x, saved


def _mid_backward(mid, saved, dy, rnd, g, prefix):
    dy, gp = block_backward_ref(_sub(mid, "resnets.1."), saved["r1"], dy, rnd=rnd)
    g.update({prefix + "mid_block.resnets.1." + k: v for k, v in gp.items()})
    H, W = dy.shape[2:]
    dt, gp = attn_ref.block_backward_ref(_sub(mid, "attentions.0."), saved["attn"], _tokens(dy), rnd=rnd)
    g.update({prefix + "mid_block.attentions.0." + k: v for k, v in gp.items()})
    dy, gp = block_backward_ref(_sub(mid, "resnets.0."), saved["r0"], _image(dt, H, W), rnd=rnd)
    g.update({prefix + "mid_block.resnets.0." + k: v for k, v in gp.items()})
    return dy


def _norm_out(ends, x, rnd):
    return rnd(F.silu(F.group_norm(x, GROUPS, ends["conv_norm_out.weight"], ends["conv_norm_out.bias"], EPS)))


def encoder_forward_ref(p, x, rnd=ident):
    """-> (moments, saved).  rnd at the device's operand roundings; conv_in runs on split (fp32-grade) operands and is not rounded."""
    ends, blks, mid = split_model(p, "encoder.")
    saved = {"x": x, "blocks": [], "bounds": {}}
    h = F.conv2d(x, ends["conv_in.weight"], ends["conv_in.bias"], padding=1)
    for i, (res, rs) in enumerate(blks):
        sb = {"res": []}
        saved["bounds"][f"down_blocks.{i}"] = h
        for q in res:
            h, s = block_forward_ref(q, h, rnd=rnd)
            sb["res"].append(s)
        if rs is not None:
            sb["x16"] = rnd(h)
            h = down_forward_ref(sb["x16"], rnd(rs["weight"]), rs["bias"])
        saved["blocks"].append(sb)
    saved["bounds"]["mid_block"] = h
    h, saved["mid"] = _mid_forward(mid, h, rnd)
    saved["bounds"]["conv_norm_out"] = h
    saved["nx"], saved["a"] = h, _norm_out(ends, h, rnd)
    return F.conv2d(saved["a"], rnd(ends["conv_out.weight"]), ends["conv_out.bias"], padding=1), saved


def encoder_backward_ref(p, saved, d_moments, rnd=ident, split=ident):
    """the encoder's backward in the operators' order -> (grads keyed like p, dx at every block boundary)"""
    ends, blks, mid = split_model(p, "encoder.")
    g, at = {}, {}
    dy16 = rnd(d_moments)
    g["encoder.conv_out.bias"] = d_moments.sum(dim=(0, 2, 3))
    g["encoder.conv_out.weight"] = wgrad_ref(dy16, saved["a"], 3)
    dy = dgrad_ref(dy16, rnd(ends["conv_out.weight"]))
    dy, g["encoder.conv_norm_out.weight"], g["encoder.conv_norm_out.bias"] = gn_silu_backward_ref(saved["nx"], ends["conv_norm_out.weight"],
                                                                                                  ends["conv_norm_out.bias"], dy)
    at["conv_norm_out"] = dy
    dy = _mid_backward(mid, saved["mid"], dy, rnd, g, "encoder.")
    at["mid_block"] = dy
    for i in reversed(range(len(blks))):
        res, rs = blks[i]
        sb = saved["blocks"][i]
        name = f"encoder.down_blocks.{i}."
        if rs is not None:
            d16 = rnd(dy)
            g[name + DOWN + "bias"] = dy.sum(dim=(0, 2, 3))
            g[name + DOWN + "weight"] = s2_wgrad_ref(d16, sb["x16"])
            dy = s2_dgrad_phase_ref(d16, rnd(rs["weight"]), sb["x16"].shape[2], sb["x16"].shape[3])
        for j in reversed(range(len(res))):
            dy, gp = block_backward_ref(res[j], sb["res"][j], dy, rnd=rnd)
            g.update({f"{name}resnets.{j}.{k}": v for k, v in gp.items()})
        at[f"down_blocks.{i}"] = dy
    g["encoder.conv_in.bias"] = dy.sum(dim=(0, 2, 3))
    g["encoder.conv_in.weight"] = thin_wgrad_ref(split(saved["x"]), rnd(dy), True)
    return {k: g[k] for k in p}, at


def decoder_forward_ref(p, z, rnd=ident, fold_rnd=None):
    """-> (image, saved).  fold_rnd: the rounding of Upsample2D's folded matrices (the device's default route), None = the literal conv."""
    ends, blks, mid = split_model(p, "decoder.")
    saved = {"z16": rnd(z), "blocks": [], "bounds": {}}
    h = F.conv2d(saved["z16"], rnd(ends["conv_in.weight"]), ends["conv_in.bias"], padding=1)
    saved["bounds"]["mid_block"] = h
    h, saved["mid"] = _mid_forward(mid, h, rnd)
    for i, (res, rs) in enumerate(blks):
        sb = {"res": []}
        saved["bounds"][f"up_blocks.{i}"] = h
        for q in res:
            h, s = block_forward_ref(q, h, rnd=rnd)
            sb["res"].append(s)
        if rs is not None:
            sb["x16"] = rnd(h)
            if fold_rnd is None:
                h = up_forward_ref(sb["x16"], rnd(rs["weight"]), rs["bias"])
            else:
                h = up2_forward_folded_ref(sb["x16"], up2_fold(rs["weight"].float(), fold_rnd).to(h.dtype)) + rs["bias"].view(1, -1, 1, 1)
        saved["blocks"].append(sb)
    saved["bounds"]["conv_norm_out"] = h
    saved["nx"], saved["a"] = h, _norm_out(ends, h, rnd)
    return F.conv2d(saved["a"], rnd(ends["conv_out.weight"]), ends["conv_out.bias"], padding=1), saved


def decoder_backward_ref(p, saved, d_image, rnd=ident, fold_rnd=None, split=ident):
    """the decoder's backward in the operators' order -> (dz, grads keyed like p, dx at every block boundary)"""
    ends, blks, mid = split_model(p, "decoder.")
    g, at = {}, {}
    g["decoder.conv_out.bias"] = d_image.sum(dim=(0, 2, 3))
    g["decoder.conv_out.weight"] = thin_wgrad_ref(split(d_image), saved["a"], False)
    dy = F.conv2d(d_image, rotate_transpose(ends["conv_out.weight"]), padding=1)          # split operands on both sides: not rounded
    dy, g["decoder.conv_norm_out.weight"], g["decoder.conv_norm_out.bias"] = gn_silu_backward_ref(saved["nx"], ends["conv_norm_out.weight"],
                                                                                                  ends["conv_norm_out.bias"], dy)
    at["conv_norm_out"] = dy
    for i in reversed(range(len(blks))):
        res, rs = blks[i]
        sb = saved["blocks"][i]
        name = f"decoder.up_blocks.{i}."
        if rs is not None:
            d16 = rnd(dy)
            g[name + UP + "bias"] = dy.sum(dim=(0, 2, 3))
            g[name + UP + "weight"] = up2_wgrad_ref(d16, sb["x16"])
            if fold_rnd is None:
                dy = dgrad_ref(d16, rnd(rs["weight"]))
                dy = ((dy[:, :, 0::2, 0::2] + dy[:, :, 0::2, 1::2]) + dy[:, :, 1::2, 0::2]) + dy[:, :, 1::2, 1::2]
            else:
                dy = up2_dgrad_gather_ref(d16, up2_fold(rs["weight"].float(), fold_rnd).to(dy.dtype))
        for j in reversed(range(len(res))):
            dy, gp = block_backward_ref(res[j], sb["res"][j], dy, rnd=rnd)
            g.update({f"{name}resnets.{j}.{k}": v for k, v in gp.items()})
        at[f"up_blocks.{i}"] = dy
    dy = _mid_backward(mid, saved["mid"], dy, rnd, g, "decoder.")
    at["mid_block"] = dy
    d16 = rnd(dy)
    g["decoder.conv_in.bias"] = dy.sum(dim=(0, 2, 3))
    g["decoder.conv_in.weight"] = wgrad_ref(d16, saved["z16"], 3)
    return dgrad_ref(d16, rnd(ends["conv_in.weight"])), {k: g[k] for k in p}, at


def scale_of(exact, k):
    """the scale a gradient's error is measured against: its own largest exact value -- except to_k.bias, whose exact gradient is ZERO (a bias on k
    shifts every score of a row alike; softmax does not see it): it is measured against to_q.bias's, as tests/test_attention_backward_device.py does"""
    ref = exact[k[:-len("to_k.bias")] + "to_q.bias"] if k.endswith("attentions.0.to_k.bias") else exact[k]
    return ref.abs().max()


def rel(a, exact, k):
    return ((a.double() - exact[k]).abs().max() / scale_of(exact, k)).item()


def model_autograd(kind, p, x, dy):
    """autograd of the unrounded functional model in x's dtype -> (y, dx, grads keyed like p)"""
    q = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    xr = x.detach().clone().requires_grad_(True)
    y, _ = (encoder_forward_ref if kind == "encoder" else decoder_forward_ref)(q, xr)
    grads = torch.autograd.grad(y, [xr] + [q[k] for k in p], dy)
    return y.detach(), grads[0], dict(zip(p.keys(), grads[1:]))


def model_refs(kind, p, x, dy):
    """-> dict(exact, f32, emu): gradients keyed like p plus "dx" (the decoder's dz; the encoder's image gradient is not a device output and is left
    out), and emu_at: the emulation's dx at every block boundary"""
    p64 = {k: v.double() for k, v in p.items()}
    _, dx64, g64 = model_autograd(kind, p64, x.double(), dy.double())
    _, dx32, g32 = model_autograd(kind, p, x, dy)
    if kind == "encoder":
        _, saved = encoder_forward_ref(p64, x.double(), rnd=bf16_round_keep)
        ge, at = encoder_backward_ref(p64, saved, dy.double(), rnd=bf16_round_keep, split=split_hilo)
        return dict(exact=g64, f32=g32, emu=ge, emu_at=at)
    _, saved = decoder_forward_ref(p64, x.double(), rnd=bf16_round_keep, fold_rnd=bf16_round_keep)
    dze, ge, at = decoder_backward_ref(p64, saved, dy.double(), rnd=bf16_round_keep, fold_rnd=bf16_round_keep, split=split_hilo)
    return dict(exact=dict(g64, dx=dx64), f32=dict(g32, dx=dx32), emu=dict(ge, dx=dze), emu_at=at)
