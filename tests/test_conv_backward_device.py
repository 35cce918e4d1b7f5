"""The resnet block's backward on the device (vae_tagger_amd/vae_backward.py over the vt_op_* backward operators): exact where the arithmetic is
exact (one-hot gradients, small integers), against the fp32 evaluation of the same operand-rounded numbers with the forward operators' accumulation-
order bound elsewhere, and -- for the sums and the whole block -- by tests/test_train_device.py's rule against fp64."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from _conv_backward_ref import (GROUPS, bf16_round_keep, block_autograd, block_backward_ref, block_forward_ref, block_params, gn_stats_ref)
from _util import bf16_round, nchw, nhwc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# B, Cin, Cout, H, W: tiny and ragged; ragged; exactly one tile, Cin != Cout; one row and one column past a tile edge; several channel tiles and images
SHAPES = [(1, 64, 64, 5, 7), (2, 128, 128, 9, 13), (1, 128, 256, 16, 16), (1, 256, 128, 17, 33), (3, 512, 512, 8, 24)]
K1_SHAPES = [SHAPES[0], SHAPES[3]]


@pytest.fixture(scope="module")
def vb():
    from vae_tagger_amd import vae_backward
    return vae_backward


@pytest.fixture(scope="module")
def rule():
    from test_train_device import FACTOR, FLOOR, check
    assert (FACTOR, FLOOR) == (4.0, 1e-7)
    return check


def _rand(shape, seed, scale=1.0):
    return scale * torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _randint(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def dev16(t_nchw):
    return nhwc(t_nchw).to(DEV, torch.bfloat16)


def dev32(t_nchw):
    return nhwc(t_nchw).to(DEV, torch.float32)


def wgrad(vb, dy, a, k, splits=0):
    """dy, a: NCHW values representable in bf16 -> dW fp32 OIHW (cpu)"""
    out = vb.conv_backward_weight(dev16(dy), dev16(a), k, splits=splits)
    torch.cuda.synchronize()
    return out.cpu()


def dgrad(vb, dy, w, dx_add=None):
    out = vb.conv_backward_data(dev16(dy), w.to(DEV).contiguous(), dx_add=None if dx_add is None else dev32(dx_add))
    torch.cuda.synchronize()
    return nchw(out.cpu())


# ---- weight gradient ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Cin,Cout,H,W", [SHAPES[1], SHAPES[3]])
def test_wgrad_one_hot_exact(vb, B, Cin, Cout, H, W):
    """dy = 1 at one (image, pixel, cout), a = an asymmetric integer ramp: dW[co] is the ramp shifted by the tap, zero where the tap leaves the image,
    and every other cout is exactly zero -- a swapped tap, shift, transposed-read lane or channel tile is a wrong number"""
    a = torch.arange(B * Cin * H * W, dtype=torch.float32).reshape(B, Cin, H, W) % 251 - 125.0
    ap = F.pad(a, (1, 1, 1, 1))
    pixels = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H // 2, W // 3)]       # four corners, an edge, an interior pixel
    for i, (y, x) in enumerate(pixels):
        b, co = i % B, (37 * i + 5) % Cout
        dy = torch.zeros(B, Cout, H, W)
        dy[b, co, y, x] = 1.0
        got = wgrad(vb, dy, a, 3)
        want = torch.zeros(Cout, Cin, 3, 3)
        want[co] = ap[b, :, y:y + 3, x:x + 3]
        assert torch.equal(got[co], want[co]), f"pixel {(y, x)}"
        if y == 0:
            assert torch.equal(got[co, :, 0], torch.zeros(Cin, 3))
        if x == W - 1:
            assert torch.equal(got[co, :, :, 2], torch.zeros(Cin, 3))
        assert torch.equal(got, want), f"pixel {(y, x)}: other couts are not zero"


@pytest.mark.parametrize("B,Cin,Cout,H,W,k", [s + (3,) for s in SHAPES] + [s + (1,) for s in K1_SHAPES])
def test_wgrad_and_dgrad_integer_data_exact(vb, B, Cin, Cout, H, W, k):
    """dy in {-1, 0, 1}, a in {-2..2}, W in {-1, 0, 1}: every partial sum is an integer below 2^24, so any split and any order give the fp64 result"""
    dy, a, w = _randint((B, Cout, H, W), -1, 1, 1), _randint((B, Cin, H, W), -2, 2, 2), _randint((Cout, Cin, k, k), -1, 1, 3)
    want_w = torch.nn.grad.conv2d_weight(a.double(), (Cout, Cin, k, k), dy.double(), padding=k // 2)
    want_x = torch.nn.grad.conv2d_input((B, Cin, H, W), w.double(), dy.double(), padding=k // 2)
    assert 2 * B * H * W < 2 ** 24 and k * k * Cout < 2 ** 24          # the largest possible sum of |products|: every partial sum is exact in fp32
    assert want_w.abs().max() < 2 ** 24 and want_x.abs().max() < 2 ** 24
    results = {sp: wgrad(vb, dy, a, k, splits=sp) for sp in (1, 2, 3, 0, B * H * W + 1)}
    for sp, got in results.items():
        assert torch.equal(got.double(), want_w), f"splits {sp}: max|d| {(got.double() - want_w).abs().max()}"
    got_x = dgrad(vb, dy, w)
    assert torch.equal(got_x.double(), want_x), (got_x.double() - want_x).abs().max()
    add = _randint((B, Cin, H, W), -3, 3, 4)
    assert torch.equal(dgrad(vb, dy, w, dx_add=add).double(), want_x + add.double())


@pytest.mark.parametrize("B,Cin,Cout,H,W,k", [s + (3,) for s in SHAPES] + [s + (1,) for s in K1_SHAPES])
def test_wgrad_and_dgrad_random_data(vb, B, Cin, Cout, H, W, k):
    """operands rounded to bf16 beforehand; against the fp32 evaluation of the same numbers, with the forward operators' accumulation-order bound"""
    dy_w = bf16_round(_rand((B, Cout, H, W), 11, (B * H * W) ** -0.5))
    dy_x = bf16_round(_rand((B, Cout, H, W), 12))
    a = bf16_round(_rand((B, Cin, H, W), 13))
    w = _rand((Cout, Cin, k, k), 14, (k * k * Cout) ** -0.5)
    want_w = torch.nn.grad.conv2d_weight(a, (Cout, Cin, k, k), dy_w, padding=k // 2)
    want_x = torch.nn.grad.conv2d_input((B, Cin, H, W), bf16_round(w), dy_x, padding=k // 2)
    got_w, got_x = wgrad(vb, dy_w, a, k), dgrad(vb, dy_x, w)
    print(f"wgrad k{k} {B}x{Cin}->{Cout}x{H}x{W}: max|d| = {(got_w - want_w).abs().max():.3e} (max|ref| {want_w.abs().max():.3f});  "
          f"dgrad: max|d| = {(got_x - want_x).abs().max():.3e} (max|ref| {want_x.abs().max():.3f})")
    assert torch.allclose(got_w, want_w, rtol=1e-4, atol=2e-4), (got_w - want_w).abs().max()
    assert torch.allclose(got_x, want_x, rtol=1e-4, atol=2e-4), (got_x - want_x).abs().max()
    assert torch.equal(wgrad(vb, dy_w, a, k), got_w) and torch.equal(dgrad(vb, dy_x, w), got_x), "not bit-identical from run to run"


# ---- cast + bias gradient ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Cin,Cout,H,W", SHAPES)
def test_cast_bias_grad(vb, rule, B, Cin, Cout, H, W):
    dy = _rand((B, H, W, Cout), 21) + 0.25
    d = dy.to(DEV)
    dy16, db = vb.cast_bias_grad(d)
    dy16b, dbb = vb.cast_bias_grad(d)
    torch.cuda.synchronize()
    assert torch.equal(dy16.cpu(), dy.to(torch.bfloat16))
    assert torch.equal(dy16, dy16b) and torch.equal(db, dbb), "not bit-identical from run to run"
    flat = dy.reshape(-1, Cout)
    rule("dbias", db.cpu(), flat.double().sum(0), flat.sum(0))
    only16, none = vb.cast_bias_grad(d, want_bias=False)
    assert none is None and torch.equal(only16, dy16)


# ---- GroupNorm statistics and GroupNorm + SiLU backward ----------------------------------------------------------------------------------------
GN_HW = {35: (5, 7), 256: (16, 16), 561: (17, 33)}
GN_CASES = [(B, C, hw, False) for C in (128, 256, 512) for hw in (35, 256, 561) for B in (1, 3)] + [(3, 256, 561, True)]


def _gn_case(B, C, hw, zero_gamma):
    H, W = GN_HW[hw]
    x = _rand((B, C, H, W), 31) + 3.0                              # a large common offset: mean >> std inside groups
    gamma, beta = 1 + 0.2 * _rand((C,), 32), 0.2 * _rand((C,), 33)
    if zero_gamma:
        gamma[[0, 5, 77, C - 1]] = 0.0
    return x, gamma, beta, _rand((B, C, H, W), 34)


def _autograd_gn(x, gamma, beta, da, dtype):
    x, gamma, beta = (t.to(dtype).clone().requires_grad_(True) for t in (x, gamma, beta))
    return torch.autograd.grad(F.silu(F.group_norm(x, GROUPS, gamma, beta, 1e-6)), [x, gamma, beta], da.to(dtype))


@pytest.mark.parametrize("B,C,hw,zero_gamma", GN_CASES)
def test_groupnorm_stats_and_silu_backward(vb, rule, B, C, hw, zero_gamma):
    x, gamma, beta, da = _gn_case(B, C, hw, zero_gamma)
    xd, dad, gd, bd = dev32(x), dev32(da), gamma.to(DEV), beta.to(DEV)
    stats = vb.groupnorm_stats(xd)
    m64, r64 = gn_stats_ref(x.double())
    m32, r32 = gn_stats_ref(x)
    print(f"B{B} C{C} HW{hw}{' gamma=0' if zero_gamma else ''}")
    rule("mean", stats[:, :, 0].cpu(), m64, m32)
    rule("rstd", stats[:, :, 1].cpu(), r64, r32)
    dx, dx16, dg, db = vb.groupnorm_silu_backward(xd, stats, gd, bd, dad, want_dx16=True)
    again = vb.groupnorm_silu_backward(xd, stats, gd, bd, dad, want_dx16=True)
    torch.cuda.synchronize()
    for u, v in zip((dx, dx16, dg, db), again):
        assert torch.equal(u, v), "not bit-identical from run to run"
    assert torch.equal(dx16, dx.to(torch.bfloat16))
    want64, want32 = _autograd_gn(x, gamma, beta, da, torch.float64), _autograd_gn(x, gamma, beta, da, torch.float32)
    rule("dx", nchw(dx.cpu()), want64[0], want32[0])
    rule("dgamma", dg.cpu(), want64[1], want32[1])
    rule("dbeta", db.cpu(), want64[2], want32[2])


def test_groupnorm_silu_backward_adds_dx_add_exactly(vb):
    """da = 0 makes the normalisation's own gradient exactly zero: dx is dx_add, bit for bit, and so is its bf16 copy"""
    x, gamma, beta, _ = _gn_case(2, 128, 35, False)
    xd = dev32(x)
    add = dev32(_randint(tuple(x.shape), -100, 100, 35))
    stats = vb.groupnorm_stats(xd)
    dx, dx16, dg, db = vb.groupnorm_silu_backward(xd, stats, gamma.to(DEV), beta.to(DEV), torch.zeros_like(xd), dx_add=add, want_dx16=True)
    torch.cuda.synchronize()
    assert torch.equal(dx, add) and torch.equal(dx16, add.to(torch.bfloat16))
    assert not dg.any() and not db.any()


# ---- the block ---------------------------------------------------------------------------------------------------------------------------------
BLOCKS = {"128-128": (1, 128, 128, 9, 13), "128-256": (2, 128, 256, 16, 16), "512-256": (1, 512, 256, 8, 24)}


@pytest.fixture(scope="module")
def block_refs():
    """per block: parameters, inputs, the exact fp64 gradients, the fp32 autograd ones and the fp64 restatement with the device's rounding points"""
    refs = {}
    for i, (name, (B, cin, cout, H, W)) in enumerate(BLOCKS.items()):
        p = block_params(cin, cout, seed=40 + i, dtype=torch.float32)
        x, dy = _rand((B, cin, H, W), 50 + i) + 0.5, _rand((B, cout, H, W), 60 + i)
        p64 = {k: v.double() for k, v in p.items()}
        _, dx64, g64 = block_autograd(p64, x.double(), dy.double())
        _, dx32, g32 = block_autograd(p, x, dy)
        _, saved = block_forward_ref(p64, x.double(), rnd=bf16_round_keep)
        dxe, ge = block_backward_ref(p64, saved, dy.double(), rnd=bf16_round_keep)
        refs[name] = dict(p=p, x=x, dy=dy, exact=dict(g64, dx=dx64), f32=dict(g32, dx=dx32), emu=dict(ge, dx=dxe))
    return refs


def _rel(a, ref):
    return ((a.double() - ref).abs().max() / ref.abs().max()).item()


@pytest.mark.parametrize("name", list(BLOCKS))
def test_block_backward(vb, block_refs, name):
    r = block_refs[name]
    p = {k: v.to(DEV).contiguous() for k, v in r["p"].items()}
    x, dy = dev32(r["x"]), dev32(r["dy"])
    y, saved = vb.resnet_block_forward_train(p, x)
    want_saved = {"x", "h1", "a1", "a2", "stats1", "stats2"} | ({"x16"} if "conv_shortcut.weight" in p else set())
    assert set(saved) == want_saved
    dx, grads = vb.resnet_block_backward(p, saved, dy)
    dx2, grads2 = vb.resnet_block_backward(p, saved, dy)
    torch.cuda.synchronize()
    assert list(grads) == list(p)
    assert all(grads[k].shape == p[k].shape and grads[k].dtype == torch.float32 for k in p)
    assert torch.equal(dx, dx2) and all(torch.equal(grads[k], grads2[k]) for k in p), "not bit-identical from run to run"
    got = {k: v.cpu() for k, v in grads.items()}
    got["dx"] = nchw(dx.cpu())
    failed = []
    for k, g in got.items():
        exact = r["exact"][k]
        d_hip, d_emu, e32 = _rel(g, exact), _rel(r["emu"][k], exact), _rel(r["f32"][k], exact)
        bound = max(1.5 * d_emu, 4.0 * e32, 1e-7)
        print(f"    {name} {k}: d_hip {d_hip:.3e}  d_emu {d_emu:.3e}  e32 {e32:.3e}  d_hip / bound {d_hip / bound:.3f}")
        if not d_hip <= bound:
            failed.append(k)
    assert not failed, failed


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals(vb):
    from vae_tagger_amd._lib import VTError
    dy16 = torch.zeros(1, 4, 4, 64, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(VTError, match="multiples of 64"):
        vb.conv_backward_weight(dy16, torch.zeros(1, 4, 4, 48, device=DEV, dtype=torch.bfloat16), 3)
    ctx = vb.context(DEV)
    a16 = torch.zeros(1, 4, 4, 64, device=DEV, dtype=torch.bfloat16)
    dw = torch.zeros(64, 64, 3, 3, device=DEV)
    need = ctx.lib.vt_op_conv_backward_weight_workspace_bytes(1, 4, 4, 64, 64, 3, 0)
    assert need > 0
    ws = torch.zeros(need, device=DEV, dtype=torch.uint8)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    with pytest.raises(VTError, match="workspace"):
        ctx.call("vt_op_conv_backward_weight", vp(dy16), vp(a16), vp(dw), 1, 4, 4, 64, 64, 3, 0, vp(ws), need - 1, None)
    ctx.call("vt_op_conv_backward_weight", vp(dy16), vp(a16), vp(dw), 1, 4, 4, 64, 64, 3, 0, vp(ws), need, None)
    p = {k: v.to(DEV) for k, v in block_params(128, 128, seed=1, dtype=torch.float32).items()}
    x = torch.zeros(1, 4, 4, 128, device=DEV)
    y, saved = vb.resnet_block_forward_train(p, x)
    ctx.call("vt_set_flag", 18, 1)
    try:
        with pytest.raises(VTError, match="fp16"):
            vb.resnet_block_forward_train(p, x)
        with pytest.raises(VTError, match="fp16"):
            vb.resnet_block_backward(p, saved, torch.zeros_like(y))
    finally:
        ctx.call("vt_set_flag", 18, 0)
    torch.cuda.synchronize()
