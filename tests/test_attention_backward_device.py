"""The mid-block attention's backward on the device (vae_tagger_amd/vae_backward.py over vt_op_attention_core_backward, vt_op_groupnorm_backward and
vt_op_attention_forward_train).  Every gradient is held to the project's rule d_hip <= max(1.5 d_emu, 4 e32, 1e-7): max-abs errors relative to the
tensor's maximum against the exact fp64 gradient, d_emu = the fp64 restatement with the device's rounding points (tests/_attention_backward_ref.py),
e32 = torch's own fp32 autograd."""
import ctypes

import pytest
import torch

import _attention_backward_ref as R
import _conv_backward_ref as RC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 512

# B, H, W: S = 99 (one ragged query block, two key tiles: empty segments), 320 (two query blocks, five key tiles), 561 (ragged in every unit),
# 2112 (more than eight query blocks); S40x96: batch 96 x one query block = 96 blocks, where the gradient P.V takes its 256-channel form (every other
# shape here runs four 128-channel workgroups per block), on one partial key tile and a slab with 8 real rows in its second row tile
SHAPES = {"S99": (2, 9, 11), "S320": (2, 16, 20), "S561": (2, 17, 33), "S2112": (1, 64, 33), "S40x96": (96, 5, 8)}


@pytest.fixture(scope="module")
def vb():
    from vae_tagger_amd import vae_backward
    return vae_backward


def _rand(shape, seed, scale=1.0):
    return scale * torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _rel(a, ref, scale=None):
    return ((a.double() - ref).abs().max() / (ref.abs().max() if scale is None else scale)).item()


def _rule(tag, got, exact, emu, f32, scales=None):
    """the rule for a dict of tensors; prints one line per tensor; returns the names that miss it"""
    failed = []
    for k in got:
        sc = None if scales is None else scales.get(k)
        d_hip, d_emu, e32 = _rel(got[k], exact[k], sc), _rel(emu[k], exact[k], sc), _rel(f32[k], exact[k], sc)
        bound = max(1.5 * d_emu, 4.0 * e32, 1e-7)
        print(f"    {tag} {k}: d_hip {d_hip:.3e}  d_emu {d_emu:.3e}  e32 {e32:.3e}  d_hip / bound {d_hip / bound:.3f}")
        if not d_hip <= bound:
            failed.append(k)
    return failed


# ---- the core --------------------------------------------------------------------------------------------------------------------------------------
def _core_case(B, S, seed, zero_qk=False):
    """inputs (q, k, v representable in bf16), the three references, and the operator's device inputs built from the emulated forward"""
    q, k, v = (_bf(_rand((B, S, C), seed + i)) for i in range(3))
    if zero_qk:
        q, k = torch.zeros_like(q), torch.zeros_like(k)
    do = _rand((B, S, C), seed + 3)
    _, *exact = R.core_autograd(q.double(), k.double(), v.double(), do.double())
    _, *f32 = R.core_autograd(q, k, v, do)
    o_emu, sv = R.core_forward_ref(q.double(), k.double(), v.double(), rnd=R.bf16_round_keep)
    emu = R.core_backward_ref(q.double(), k.double(), v.double(), o_emu, do.double(), sv, rnd=R.bf16_round_keep)
    names = ("dq", "dk", "dv")
    sums = torch.zeros(4, B, S)
    sums[0] = sv["tot"].squeeze(-1).float()                          # ((s0 + 0) + 0) + 0: the row sum as one segment
    return dict(q=q, k=k, v=v, do=do, o=o_emu.float(), shift=sv["c"].squeeze(-1).float(), sums=sums, exact=dict(zip(names, exact)), f32=dict(zip(names, f32)),
                emu=dict(zip(names, emu)))


@pytest.fixture(scope="module")
def core_cases():
    return {name: _core_case(B, H * W, 100 + 10 * i) for i, (name, (B, H, W)) in enumerate(SHAPES.items())}


def _core_inputs(vb, r, sl=slice(None)):
    q, k, v = r["q"][sl], r["k"][sl], r["v"][sl]
    B, S, _ = q.shape
    pitch = vb.context(DEV).lib.vt_op_attention_vt_pitch(S)
    vT = torch.zeros(B, C, pitch, dtype=torch.bfloat16)
    vT[:, :, :S] = v.transpose(1, 2).to(torch.bfloat16)
    return (torch.cat([q, k], dim=2).to(DEV, torch.bfloat16).contiguous(), vT.to(DEV), r["o"][sl].contiguous().to(DEV), r["do"][sl].contiguous().to(DEV),
            r["shift"][sl].contiguous().to(DEV), r["sums"][:, sl].contiguous().to(DEV))


def _core(vb, r, sl=slice(None), **kw):
    out = vb.attention_core_backward(*_core_inputs(vb, r, sl), **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", list(SHAPES))
def test_core_parity_determinism_and_invariance(vb, core_cases, name):
    r = core_cases[name]
    dq, dk, dv, (dq16, dk16, dv16) = _core(vb, r)
    got = {"dq": dq.cpu(), "dk": dk.cpu(), "dv": dv.cpu()}
    assert all(torch.isfinite(t).all() for t in got.values())
    failed = _rule(name, got, r["exact"], r["emu"], r["f32"])
    assert not failed, failed
    for t32, t16 in ((dq, dq16), (dk, dk16), (dv, dv16)):
        assert torch.equal(t16, t32.to(torch.bfloat16))
    again = _core(vb, r)
    assert all(torch.equal(a, b) for a, b in zip((dq, dk, dv), again[:3])), "not bit-identical from run to run"
    # an image's result does not depend on the batch it ran in, on the image group or on the split of the sweeps
    B = r["q"].shape[0]
    if B > 1:
        one = _core(vb, r, slice(1, 2))
        assert all(torch.equal(a[1:2], b) for a, b in zip((dq, dk, dv), one[:3])), "depends on the batch"
        grouped = _core(vb, r, group=1)
        assert all(torch.equal(a, b) for a, b in zip((dq, dk, dv), grouped[:3])), "depends on the image group"
    for nsplit in (1, 2, 3, 4):
        split = _core(vb, r, nsplit=nsplit, want_bf16=False)
        assert split[3] is None
        assert all(torch.equal(a, b) for a, b in zip((dq, dk, dv), split[:3])), f"depends on nsplit = {nsplit}"


def test_core_uniform_probabilities(vb):
    """q = k = 0: p is uniform, so dq and dk are exactly 0 (ds multiplies k = 0, ds^T multiplies q = 0) and dv[j] = mean_i do[i]"""
    B, H, W = SHAPES["S320"]
    r = _core_case(B, H * W, 500, zero_qk=True)
    dq, dk, dv, _ = _core(vb, r)
    assert not dq.any() and not dk.any()
    mean = r["do"].double().mean(dim=1, keepdim=True).expand(-1, H * W, -1)
    assert _rel(r["exact"]["dv"], mean) <= 1e-12
    failed = _rule("uniform", {"dv": dv.cpu()}, {"dv": mean}, r["emu"], r["f32"])
    assert not failed, failed


# ---- the block -------------------------------------------------------------------------------------------------------------------------------------
def _block_case(B, H, W, seed, gain=1.0):
    p = R.attn_params(C, seed=seed, dtype=torch.float32, gain=gain)
    x, dy = _rand((B, H * W, C), seed + 1) + 0.5, _rand((B, H * W, C), seed + 2)
    p64 = {k: v.double() for k, v in p.items()}
    _, dx64, g64 = R.block_autograd(p64, x.double(), dy.double())
    _, dx32, g32 = R.block_autograd(p, x, dy)
    _, saved = R.block_forward_ref(p64, x.double(), rnd=R.bf16_round_keep)
    dxe, ge = R.block_backward_ref(p64, saved, dy.double(), rnd=R.bf16_round_keep)
    # the exact to_k.bias gradient is ZERO (a bias on k shifts every score of a row alike; softmax does not see it): its error has no scale of its own and
    # is measured against to_q.bias's gradient, the same kind of sum over the other index
    scales = {"to_k.bias": g64["to_q.bias"].abs().max()}
    return dict(p=p, x=x, dy=dy, shape=(B, H, W), exact=dict(g64, dx=dx64), f32=dict(g32, dx=dx32), emu=dict(ge, dx=dxe), scales=scales)


BLOCKS = {"S99": ("S99", 1.0), "S320": ("S320", 1.0), "S561": ("S561", 1.0), "S2112": ("S2112", 1.0), "S320-gain6": ("S320", 6.0)}


@pytest.fixture(scope="module")
def block_cases():
    return {}


def _block(block_cases, name):
    if name not in block_cases:
        shape, gain = BLOCKS[name]
        block_cases[name] = _block_case(*SHAPES[shape], seed=200 + 7 * list(BLOCKS).index(name), gain=gain)
    return block_cases[name]


def _dev_block(r):
    B, H, W = r["shape"]
    p = {k: v.to(DEV).contiguous() for k, v in r["p"].items()}
    return p, r["x"].reshape(B, H, W, C).to(DEV), r["dy"].reshape(B, H, W, C).to(DEV)


@pytest.mark.parametrize("name", list(BLOCKS))
def test_block_backward(vb, block_cases, name):
    r = _block(block_cases, name)
    B, H, W = r["shape"]
    p, x, dy = _dev_block(r)
    y, saved = vb.attention_block_forward_train(p, x)
    assert set(saved) == {"x", "h16", "qk16", "vT16", "o16", "o", "shift", "sums", "stats"}
    dx, grads = vb.attention_block_backward(p, saved, dy)
    dx2, grads2 = vb.attention_block_backward(p, saved, dy)
    torch.cuda.synchronize()
    assert list(grads) == list(p)
    assert all(grads[k].shape == p[k].shape and grads[k].dtype == torch.float32 for k in p)
    assert torch.equal(dx, dx2) and all(torch.equal(grads[k], grads2[k]) for k in p), "not bit-identical from run to run"
    if name.endswith("gain6"):
        # the operand-norm bound is too loose here: the group is flagged and the shift is the exact row maximum of the device's own scores
        qk = saved["qk16"].float()
        smax = (qk[:, :, :C] @ qk[:, :, C:].transpose(1, 2) * C ** -0.5).max(dim=-1).values
        assert (saved["shift"] - smax).abs().max().item() <= 1e-3 * smax.abs().max().item()
    got = {k: v.cpu() for k, v in grads.items()}
    got["dx"] = dx.cpu().reshape(B, H * W, C)
    failed = _rule(name, got, r["exact"], r["emu"], r["f32"], r["scales"])
    assert not failed, failed


def test_block_backward_is_independent_of_the_batch(vb, block_cases):
    r = _block(block_cases, "S320")
    p, x, dy = _dev_block(r)
    y, saved = vb.attention_block_forward_train(p, x)
    dx, _ = vb.attention_block_backward(p, saved, dy)
    y1, saved1 = vb.attention_block_forward_train(p, x[1:2].contiguous())
    dx1, _ = vb.attention_block_backward(p, saved1, dy[1:2].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(y[1:2], y1) and torch.equal(dx[1:2], dx1)


@pytest.mark.parametrize("gain", [1.0, 6.0])
def test_forward_train_matches_the_inference_operator_bit_for_bit(vb, gain):
    """vt_op_groupnorm + vt_op_attention on a context whose encoder holds the same (synthetic, seeded) weights: the same launches on the same roundings"""
    from vae_tagger_amd import _lib, synth
    from vae_tagger_amd.diffusers_vae_loader import get_diffusers_vae_config, load_diffusers_vae_from_config
    sd = synth.synth_state_dict(synth.encoder_manifest(), seed=0)
    A = "encoder.mid_block.attentions.0."
    for k in ("to_q", "to_k"):
        sd[A + k + ".weight"] = sd[A + k + ".weight"] * gain
        sd[A + k + ".bias"] = sd[A + k + ".bias"] * gain
    m = load_diffusers_vae_from_config(get_diffusers_vae_config())
    m.load_state_dict(sd, strict=False)
    ctx = m.to("cuda").eval()._context()
    B, H, W = SHAPES["S561"]
    S = H * W
    x = (_rand((B, H, W, C), 77) + 0.5).to(DEV)
    p = {n: sd[A + n].float().reshape(sd[A + n].shape[:2] if sd[A + n].dim() > 1 else (-1,)).contiguous().to(DEV) for n in R.ATTN_PARAMS}
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    h16 = torch.empty(B, S, C, dtype=torch.bfloat16, device=DEV)
    ws = torch.empty(max(ctx.lib.vt_op_groupnorm_workspace_bytes(B, S, C), 16), dtype=torch.uint8, device=DEV)
    ctx.call("vt_op_groupnorm", vp(x), _lib.VT_F32, B, S, C, 32, 1e-6, vp(p["group_norm.weight"]), vp(p["group_norm.bias"]), 0, vp(h16), vp(ws), None)
    want = torch.full((B, S, C), float("nan"), device=DEV)
    ws2 = torch.empty(ctx.lib.vt_op_attention_workspace_bytes(B, S, C), dtype=torch.uint8, device=DEV)
    ctx.call("vt_op_attention", vp(h16), vp(x), vp(want), B, S, C, vp(ws2), None)
    y, saved = vb.attention_block_forward_train(p, x)
    torch.cuda.synchronize()
    assert torch.equal(saved["h16"].reshape(B, S, C), h16)
    assert torch.equal(y.reshape(B, S, C), want)
    assert torch.equal(saved["o"], saved["o16"].reshape(B, S, C).float())


# ---- the mid block ---------------------------------------------------------------------------------------------------------------------------------
def _tok(t_nchw):
    B, Cc, H, W = t_nchw.shape
    return t_nchw.permute(0, 2, 3, 1).reshape(B, H * W, Cc)


def _img(t_tok, H, W):
    B, S, Cc = t_tok.shape
    return t_tok.reshape(B, H, W, Cc).permute(0, 3, 1, 2)


def _mid_forward(p, x_nchw, rnd):
    """resnets.0 -> attentions.0 -> resnets.1 from the two functional restatements (NCHW resnet blocks, token attention)"""
    H, W = x_nchw.shape[2:]
    sub = lambda pre: {k[len(pre):]: v for k, v in p.items() if k.startswith(pre)}
    y0, s0 = RC.block_forward_ref(sub("resnets.0."), x_nchw, rnd=rnd)
    y1, s1 = R.block_forward_ref(sub("attentions.0."), _tok(y0), rnd=rnd)
    y2, s2 = RC.block_forward_ref(sub("resnets.1."), _img(y1, H, W), rnd=rnd)
    return y2, (s0, s1, s2)


def _mid_backward(p, saved, dy_nchw, rnd):
    H, W = dy_nchw.shape[2:]
    sub = lambda pre: {k[len(pre):]: v for k, v in p.items() if k.startswith(pre)}
    g = {}
    d2, g2 = RC.block_backward_ref(sub("resnets.1."), saved[2], dy_nchw, rnd=rnd)
    d1, g1 = R.block_backward_ref(sub("attentions.0."), saved[1], _tok(d2), rnd=rnd)
    d0, g0 = RC.block_backward_ref(sub("resnets.0."), saved[0], _img(d1, H, W), rnd=rnd)
    for pre, gp in (("resnets.0.", g0), ("attentions.0.", g1), ("resnets.1.", g2)):
        g.update({pre + k: v for k, v in gp.items()})
    return d0, {k: g[k] for k in p}


def _mid_autograd(p, x, dy):
    q = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    xr = x.detach().clone().requires_grad_(True)
    y, _ = _mid_forward(q, xr, RC.ident)
    grads = torch.autograd.grad(y, [xr] + [q[k] for k in p], dy)
    return grads[0], dict(zip(p.keys(), grads[1:]))


def test_mid_block_backward(vb):
    B, H, W = SHAPES["S99"]
    p = {}
    for pre, sub in (("resnets.0.", RC.block_params(C, C, seed=301, dtype=torch.float32)), ("attentions.0.", R.attn_params(C, seed=302, dtype=torch.float32)),
                     ("resnets.1.", RC.block_params(C, C, seed=303, dtype=torch.float32))):
        p.update({pre + k: v for k, v in sub.items()})
    x, dy = _rand((B, C, H, W), 304) + 0.5, _rand((B, C, H, W), 305)
    p64 = {k: v.double() for k, v in p.items()}
    dx64, g64 = _mid_autograd(p64, x.double(), dy.double())
    dx32, g32 = _mid_autograd(p, x, dy)
    _, saved = _mid_forward(p64, x.double(), RC.bf16_round_keep)
    dxe, ge = _mid_backward(p64, saved, dy.double(), RC.bf16_round_keep)
    pd = {k: v.to(DEV).contiguous() for k, v in p.items()}
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)
    y, sv = vb.mid_block_forward_train(pd, nhwc(x))
    assert set(sv) == {"resnets.0.", "attentions.0.", "resnets.1."}
    dx, grads = vb.mid_block_backward(pd, sv, nhwc(dy))
    dx2, grads2 = vb.mid_block_backward(pd, sv, nhwc(dy))
    torch.cuda.synchronize()
    assert list(grads) == list(pd) and all(grads[k].shape == pd[k].shape for k in pd)
    assert torch.equal(dx, dx2) and all(torch.equal(grads[k], grads2[k]) for k in pd), "not bit-identical from run to run"
    got = {k: v.cpu() for k, v in grads.items()}
    got["dx"] = dx.cpu().permute(0, 3, 1, 2)
    scales = {"attentions.0.to_k.bias": g64["attentions.0.to_q.bias"].abs().max()}     # (an exactly-zero gradient: see _block_case)
    failed = _rule("mid", got, dict(g64, dx=dx64), dict(ge, dx=dxe), dict(g32, dx=dx32), scales)
    assert not failed, failed


# ---- GroupNorm backward ----------------------------------------------------------------------------------------------------------------------------
GN_CASES = [(1, 512, 5, 7, False), (3, 512, 17, 33, False), (3, 256, 17, 33, True), (1, 128, 16, 16, False)]


def _gn_case(B, Cc, H, W, zero_gamma):
    x = _rand((B, H * W, Cc), 31) + 3.0                            # a large common offset: mean >> std inside groups
    gamma, beta = 1 + 0.2 * _rand((Cc,), 32), 0.2 * _rand((Cc,), 33)
    if zero_gamma:
        gamma[[0, 5, 77, Cc - 1]] = 0.0
    return x, gamma, beta, _rand((B, H * W, Cc), 34)


def _autograd_gn(x, gamma, beta, dh, dtype):
    x, gamma, beta = (t.to(dtype).clone().requires_grad_(True) for t in (x, gamma, beta))
    h = torch.nn.functional.group_norm(x.transpose(1, 2), 32, gamma, beta, 1e-6).transpose(1, 2)
    return torch.autograd.grad(h, [x, gamma, beta], dh.to(dtype))


@pytest.mark.parametrize("B,Cc,H,W,zero_gamma", GN_CASES)
def test_groupnorm_backward(vb, B, Cc, H, W, zero_gamma):
    from test_train_device import FACTOR, FLOOR, check
    assert (FACTOR, FLOOR) == (4.0, 1e-7)
    x, gamma, beta, dh = _gn_case(B, Cc, H, W, zero_gamma)
    xd, dhd, gd, bd = x.reshape(B, H, W, Cc).to(DEV), dh.reshape(B, H, W, Cc).to(DEV), gamma.to(DEV), beta.to(DEV)
    stats = vb.groupnorm_stats(xd)
    dx, dx16, dg, db = vb.groupnorm_backward(xd, stats, gd, bd, dhd, want_dx16=True)
    again = vb.groupnorm_backward(xd, stats, gd, bd, dhd, want_dx16=True)
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip((dx, dx16, dg, db), again)), "not bit-identical from run to run"
    assert torch.equal(dx16, dx.to(torch.bfloat16))
    want64, want32 = _autograd_gn(x, gamma, beta, dh, torch.float64), _autograd_gn(x, gamma, beta, dh, torch.float32)
    check("dx", dx.cpu().reshape(B, H * W, Cc), want64[0], want32[0])
    check("dgamma", dg.cpu(), want64[1], want32[1])
    check("dbeta", db.cpu(), want64[2], want32[2])


def test_groupnorm_backward_adds_dx_add_exactly(vb):
    """dh = 0 makes the normalisation's own gradient exactly zero: dx is dx_add, bit for bit, and so is its bf16 copy"""
    x, gamma, beta, _ = _gn_case(2, 512, 5, 7, False)
    xd = x.reshape(2, 5, 7, 512).to(DEV)
    add = torch.randint(-100, 101, tuple(xd.shape), generator=torch.Generator().manual_seed(35)).float().to(DEV)
    stats = vb.groupnorm_stats(xd)
    dx, dx16, dg, db = vb.groupnorm_backward(xd, stats, gamma.to(DEV), beta.to(DEV), torch.zeros_like(xd), dx_add=add, want_dx16=True)
    torch.cuda.synchronize()
    assert torch.equal(dx, add) and torch.equal(dx16, add.to(torch.bfloat16))
    assert not dg.any() and not db.any()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(vb, core_cases):
    from vae_tagger_amd._lib import VTError
    ctx = vb.context(DEV)
    p256 = {k: v.to(DEV) for k, v in R.attn_params(256, seed=1, dtype=torch.float32).items()}
    with pytest.raises(VTError, match="C = 512"):
        vb.attention_block_forward_train(p256, torch.zeros(1, 4, 4, 256, device=DEV))
    z16 = lambda *s: torch.zeros(*s, device=DEV, dtype=torch.bfloat16)
    z32 = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(VTError, match="C = 512"):
        vb.attention_core_backward(z16(1, 16, 512), z16(1, 256, 16), z32(1, 16, 256), z32(1, 16, 256), z32(1, 16), z32(4, 1, 16))
    r = core_cases["S99"]
    qk, vT, o, do, shift, sums = _core_inputs(vb, r)
    B, S, _ = o.shape
    need = ctx.lib.vt_op_attention_core_backward_workspace_bytes(B, S, C)
    ws = torch.zeros(need, device=DEV, dtype=torch.uint8)
    outs = [torch.zeros(B, S, C, device=DEV) for _ in range(3)]
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    args = [vp(t) for t in (qk, vT, o, do, shift, sums)] + [vp(t) for t in outs] + [None, None, None, B, S, C, 0, 0, vp(ws)]
    with pytest.raises(VTError, match="workspace"):
        ctx.call("vt_op_attention_core_backward", *args, need - 1, None)
    ctx.call("vt_op_attention_core_backward", *args, need, None)
    p = {k: v.to(DEV) for k, v in R.attn_params(C, seed=2, dtype=torch.float32).items()}
    x = torch.zeros(1, 4, 4, C, device=DEV)
    y, saved = vb.attention_block_forward_train(p, x)
    ctx.call("vt_set_flag", 18, 1)
    try:
        with pytest.raises(VTError, match="fp16"):
            vb.attention_block_forward_train(p, x)
        with pytest.raises(VTError, match="fp16"):
            vb.attention_block_backward(p, saved, torch.zeros_like(y))
    finally:
        ctx.call("vt_set_flag", 18, 0)
    torch.cuda.synchronize()
