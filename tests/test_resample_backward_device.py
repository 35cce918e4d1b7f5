"""Backward of the two resampling layers on the device (vae_tagger_amd/vae_backward.py over vt_op_conv_s2_backward_* and
vt_op_upsample2x_conv3x3_backward_*): exact where the arithmetic is exact (one-hot gradients, small integers, the adjoint identity), against the
fp32 evaluation of the same operand-rounded numbers with the forward operators' accumulation-order bound elsewhere, and -- for a down block and an up
block -- by tests/test_conv_backward_device.py's rule against fp64 autograd.  Every data gradient runs on both of its routes (the new kernel and the
literal route: flag 23 for the stride-2 conv, flag 22 for Upsample2D)."""
import contextlib
import ctypes

import pytest
import torch
import torch.nn.functional as F

from _conv_backward_ref import bf16_round_keep
from _resample_backward_ref import (down_forward_ref, rs_block_autograd, rs_block_backward_ref, rs_block_forward_ref, rs_block_params, s2_dgrad_phase_ref,
                                    s2_wgrad_ref, sum2x2, up2_dgrad_gather_ref, up2_fold, up2_wgrad_ref, up_forward_ref)
from _util import bf16_round, nchw, nhwc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# B, Cin, Cout, H, W: tiny, both sides odd; ragged; exactly one tile of the up2 skeleton; one row and one column past the tile edges; several channel
# tiles and images; Cin != Cout
DOWN = [(1, 64, 64, 5, 7), (2, 128, 128, 10, 14), (1, 128, 128, 16, 32), (1, 256, 256, 34, 66), (3, 512, 512, 8, 24), (1, 64, 128, 9, 12)]
# B, C, h, w (low resolution)
UP = [(1, 64, 3, 5), (2, 128, 5, 7), (1, 128, 8, 16), (1, 256, 9, 17), (2, 512, 4, 12)]
ROUTES = ["kernel", "literal"]
cdiv = lambda a, b: -(-a // b)


@pytest.fixture(scope="module")
def vb():
    from vae_tagger_amd import vae_backward
    return vae_backward


@contextlib.contextmanager
def route(vb, flag, name):
    """flag 23 (stride-2 data gradient) / flag 22 (Upsample2D, forward and data gradient): 1 = the literal route"""
    ctx = vb.context(DEV)
    ctx.call("vt_set_flag", flag, 1 if name == "literal" else 0)
    try:
        yield
    finally:
        torch.cuda.synchronize()
        ctx.call("vt_set_flag", flag, 0)


def _rand(shape, seed, scale=1.0):
    return scale * torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _randint(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def _ramp(shape, mod, off):
    n = 1
    for s in shape:
        n *= s
    return (torch.arange(n, dtype=torch.float32) * 7 % mod - off).reshape(shape)       # asymmetric, every value exact in bf16


def dev16(t_nchw):
    return nhwc(t_nchw).to(DEV, torch.bfloat16)


def dev32(t_nchw):
    return nhwc(t_nchw).to(DEV, torch.float32)


def s2_dgrad(vb, dy, w, H, W, dx_add=None):
    out = vb.downsample_backward_data(dev16(dy), w.to(DEV).contiguous(), H, W, dx_add=None if dx_add is None else dev32(dx_add))
    torch.cuda.synchronize()
    return nchw(out.cpu())


def s2_wgrad(vb, dy, a, splits=0):
    out = vb.downsample_backward_weight(dev16(dy), dev16(a), splits=splits)
    torch.cuda.synchronize()
    return out.cpu()


def up_dgrad(vb, dy, w, dx_add=None):
    out = vb.upsample_backward_data(dev16(dy), w.to(DEV).contiguous(), dx_add=None if dx_add is None else dev32(dx_add))
    torch.cuda.synchronize()
    return nchw(out.cpu())


def up_wgrad(vb, dy, x, splits=0):
    out = vb.upsample_backward_weight(dev16(dy), dev16(x), splits=splits)
    torch.cuda.synchronize()
    return out.cpu()


def _pixels(H, W):
    """four corners, an edge, an interior pixel (of a gradient of size H x W)"""
    return sorted({(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H // 2, W // 3)})


# ---- one-hot, exact ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Cin,Cout,H,W", [DOWN[0], DOWN[3], DOWN[5]])
def test_stride2_one_hot_exact(vb, B, Cin, Cout, H, W):
    """dy = 1 at one (image, pixel, cout) against asymmetric integer ramps: dx is W[co] laid out at (2i + ky, 2j + kx), dW[co] is the activation patch
    at the same places, clipped by the image (for odd sizes the last row / column IS inside: phase 0 only), everything else exactly zero -- a swapped
    phase, tap, parity plane or shift is a wrong number"""
    Ho, Wo = H // 2, W // 2
    w, a = _ramp((Cout, Cin, 3, 3), 251, 125.0), _ramp((B, Cin, H, W), 241, 120.0)
    ap = F.pad(a, (0, 2, 0, 2))
    for n, (i, j) in enumerate(_pixels(Ho, Wo)):
        b, co = n % B, (37 * n + 5) % Cout
        dy = torch.zeros(B, Cout, Ho, Wo)
        dy[b, co, i, j] = 1.0
        want_x = torch.zeros(B, Cin, H + 2, W + 2)
        want_x[b, :, 2 * i:2 * i + 3, 2 * j:2 * j + 3] = w[co]
        want_x = want_x[:, :, :H, :W]
        want_w = torch.zeros(Cout, Cin, 3, 3)
        want_w[co] = ap[b, :, 2 * i:2 * i + 3, 2 * j:2 * j + 3]
        if H % 2 and i == Ho - 1:
            assert want_x[b, :, H - 1].any() and want_w[co, :, 2].any()          # the last row exists, through ky = 2 only
        if H % 2 == 0 and i == Ho - 1:
            assert not want_w[co, :, 2].any()
        for r in ROUTES:
            with route(vb, 23, r):
                got = s2_dgrad(vb, dy, w, H, W)
            assert torch.equal(got, want_x), f"dgrad ({r}) pixel {(i, j)}: max|d| {(got - want_x).abs().max()}"
        got = s2_wgrad(vb, dy, a)
        assert torch.equal(got[co], want_w[co]), f"wgrad pixel {(i, j)}"
        assert torch.equal(got, want_w), f"wgrad pixel {(i, j)}: other couts are not zero"


@pytest.mark.parametrize("B,C,h,w", [UP[0], UP[3]])
def test_upsample_one_hot_exact(vb, B, C, h, w):
    """dy = 1 at one high-resolution (image, pixel, cout): tap (ky, kx) sends W[co][:, ky, kx] to low-resolution pixel ((Y + ky - 1) >> 1, (X + kx - 1) >> 1)
    where the high-resolution tap lies inside the image, and dW[co][:, ky, kx] is x at that pixel.  |W| <= 31: folded sums of four taps are exact in bf16."""
    wt, x = _ramp((C, C, 3, 3), 63, 31.0), _ramp((B, C, h, w), 241, 120.0)
    H2, W2 = 2 * h, 2 * w
    for n, (Y, X) in enumerate(_pixels(H2, W2) + [(H2 - 1, W2 - 2), (1, 1)]):
        b, co = n % B, (37 * n + 5) % C
        dy = torch.zeros(B, C, H2, W2)
        dy[b, co, Y, X] = 1.0
        want_x, want_w = torch.zeros(B, C, h, w), torch.zeros(C, C, 3, 3)
        for ky in range(3):
            for kx in range(3):
                P, Q = Y + ky - 1, X + kx - 1
                if 0 <= P < H2 and 0 <= Q < W2:
                    want_x[b, :, P >> 1, Q >> 1] += wt[co, :, ky, kx]
                    want_w[co, :, ky, kx] = x[b, :, P >> 1, Q >> 1]
        for r in ROUTES:
            with route(vb, 22, r):
                got = up_dgrad(vb, dy, wt)
            assert torch.equal(got, want_x), f"dgrad ({r}) pixel {(Y, X)}: max|d| {(got - want_x).abs().max()}"
        got = up_wgrad(vb, dy, x)
        assert torch.equal(got[co], want_w[co]), f"wgrad pixel {(Y, X)}"
        assert torch.equal(got, want_w), f"wgrad pixel {(Y, X)}: other couts are not zero"


# ---- integer data, exact; the adjoint identity ---------------------------------------------------------------------------------------------------
def _autograd64(forward, x, w, dy):
    x, w = x.double().requires_grad_(True), w.double().requires_grad_(True)
    return torch.autograd.grad(forward(x, w), [x, w], dy.double())


@pytest.mark.parametrize("B,Cin,Cout,H,W", DOWN)
def test_stride2_integer_data_exact(vb, B, Cin, Cout, H, W):
    """dy, W in {-1, 0, 1}, a in {-2..2}: every partial sum is an integer below 2^24, so both routes, any split and any order give the fp64 result;
    and on the same data sum dy * forward(a) == sum a * dgrad(dy) exactly, with the forward operator"""
    Ho, Wo = H // 2, W // 2
    dy, a, w = _randint((B, Cout, Ho, Wo), -1, 1, 1), _randint((B, Cin, H, W), -2, 2, 2), _randint((Cout, Cin, 3, 3), -1, 1, 3)
    want_x, want_w = _autograd64(down_forward_ref, a, w, dy)
    assert 2 * B * Ho * Wo < 2 ** 24 and 9 * Cout < 2 ** 24 and 2 * 9 * Cin < 2 ** 24        # the largest possible sums of |products|
    assert want_w.abs().max() < 2 ** 24 and want_x.abs().max() < 2 ** 24
    tiles = B * cdiv(Ho, 2) * cdiv(Wo, 32)
    for sp in (1, 2, 3, 0, tiles + 1):
        got = s2_wgrad(vb, dy, a, splits=sp)
        assert torch.equal(got.double(), want_w), f"splits {sp}: max|d| {(got.double() - want_w).abs().max()}"
    add = _randint((B, Cin, H, W), -3, 3, 4)
    y = vb.downsample_forward(w.to(DEV).contiguous(), torch.zeros(Cout, device=DEV), dev16(a))
    torch.cuda.synchronize()
    y = nchw(y.cpu()).double()
    assert torch.equal(y, down_forward_ref(a.double(), w.double()))
    for r in ROUTES:
        with route(vb, 23, r):
            got = s2_dgrad(vb, dy, w, H, W)
            got_add = s2_dgrad(vb, dy, w, H, W, dx_add=add)
        assert torch.equal(got.double(), want_x), f"{r}: max|d| {(got.double() - want_x).abs().max()}"
        assert torch.equal(got_add.double(), want_x + add.double()), f"{r} with dx_add"
        assert (dy.double() * y).sum().item() == (a.double() * got.double()).sum().item(), f"{r}: adjoint identity"


@pytest.mark.parametrize("B,C,h,w", UP)
def test_upsample_integer_data_exact(vb, B, C, h, w):
    """the same for Upsample2D: folded sums of at most four taps in {-1, 0, 1} are exact in bf16, so the folded and the literal route agree exactly; the
    adjoint identity holds against the forward operator of the same route (flag 22 off and on)"""
    dy, x, wt = _randint((B, C, 2 * h, 2 * w), -1, 1, 5), _randint((B, C, h, w), -2, 2, 6), _randint((C, C, 3, 3), -1, 1, 7)
    want_x, want_w = _autograd64(up_forward_ref, x, wt, dy)
    assert 2 * B * 4 * h * w < 2 ** 24 and 4 * 16 * C < 2 ** 24 and 2 * 9 * C < 2 ** 24
    assert want_w.abs().max() < 2 ** 24 and want_x.abs().max() < 2 ** 24
    tiles = B * cdiv(2 * h, 6) * cdiv(2 * w, 32)
    for sp in (1, 2, 3, 0, tiles + 1):
        got = up_wgrad(vb, dy, x, splits=sp)
        assert torch.equal(got.double(), want_w), f"splits {sp}: max|d| {(got.double() - want_w).abs().max()}"
    add = _randint((B, C, h, w), -3, 3, 8)
    for r in ROUTES:
        with route(vb, 22, r):
            y = vb.upsample_forward(wt.to(DEV).contiguous(), torch.zeros(C, device=DEV), dev16(x))
            got = up_dgrad(vb, dy, wt)
            got_add = up_dgrad(vb, dy, wt, dx_add=add)
        y = nchw(y.cpu()).double()
        assert torch.equal(y, up_forward_ref(x.double(), wt.double())), r
        assert torch.equal(got.double(), want_x), f"{r}: max|d| {(got.double() - want_x).abs().max()}"
        assert torch.equal(got_add.double(), want_x + add.double()), f"{r} with dx_add"
        assert (dy.double() * y).sum().item() == (x.double() * got.double()).sum().item(), f"{r}: adjoint identity"


# ---- random data ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Cin,Cout,H,W", DOWN)
def test_stride2_random_data(vb, B, Cin, Cout, H, W):
    """operands rounded to bf16 beforehand; against the fp32 evaluation of the same numbers, with the forward operators' bound"""
    Ho, Wo = H // 2, W // 2
    dy_w = bf16_round(_rand((B, Cout, Ho, Wo), 11, (B * Ho * Wo) ** -0.5))
    dy_x = bf16_round(_rand((B, Cout, Ho, Wo), 12))
    a = bf16_round(_rand((B, Cin, H, W), 13))
    w = _rand((Cout, Cin, 3, 3), 14, (9 * Cout) ** -0.5)
    want_w, want_x = s2_wgrad_ref(dy_w, a), s2_dgrad_phase_ref(dy_x, bf16_round(w), H, W)
    got_w = s2_wgrad(vb, dy_w, a)
    print(f"stride 2 {B}x{Cin}->{Cout}x{H}x{W}: wgrad max|d| = {(got_w - want_w).abs().max():.3e} (max|ref| {want_w.abs().max():.3f})")
    assert torch.allclose(got_w, want_w, rtol=1e-4, atol=2e-4), (got_w - want_w).abs().max()
    assert torch.equal(s2_wgrad(vb, dy_w, a), got_w), "wgrad: not bit-identical from run to run"
    for r in ROUTES:
        with route(vb, 23, r):
            got_x, again = s2_dgrad(vb, dy_x, w, H, W), s2_dgrad(vb, dy_x, w, H, W)
        print(f"    dgrad ({r}): max|d| = {(got_x - want_x).abs().max():.3e} (max|ref| {want_x.abs().max():.3f})")
        assert torch.allclose(got_x, want_x, rtol=1e-4, atol=2e-4), (r, (got_x - want_x).abs().max())
        assert torch.equal(again, got_x), f"dgrad ({r}): not bit-identical from run to run"


@pytest.mark.parametrize("B,C,h,w", UP)
def test_upsample_random_data(vb, B, C, h, w):
    """as above; the folded route's reference holds the folded weights as the packer rounds them (fp32 sum, ky-major then kx, one rounding to bf16), the
    literal route's holds bf16(W)"""
    dy_w = bf16_round(_rand((B, C, 2 * h, 2 * w), 15, (B * 4 * h * w) ** -0.5))
    dy_x = bf16_round(_rand((B, C, 2 * h, 2 * w), 16))
    x = bf16_round(_rand((B, C, h, w), 17))
    wt = _rand((C, C, 3, 3), 18, (9 * C) ** -0.5)
    want_w = up2_wgrad_ref(dy_w, x)
    got_w = up_wgrad(vb, dy_w, x)
    print(f"upsample {B}x{C}x{h}x{w}: wgrad max|d| = {(got_w - want_w).abs().max():.3e} (max|ref| {want_w.abs().max():.3f})")
    assert torch.allclose(got_w, want_w, rtol=1e-4, atol=2e-4), (got_w - want_w).abs().max()
    assert torch.equal(up_wgrad(vb, dy_w, x), got_w), "wgrad: not bit-identical from run to run"
    wants = {"kernel": up2_dgrad_gather_ref(dy_x, up2_fold(wt, bf16_round)),
             "literal": sum2x2(torch.nn.grad.conv2d_input((B, C, 2 * h, 2 * w), bf16_round(wt), dy_x, padding=1))}
    for r in ROUTES:
        with route(vb, 22, r):
            got_x, again = up_dgrad(vb, dy_x, wt), up_dgrad(vb, dy_x, wt)
        want_x = wants[r]
        print(f"    dgrad ({r}): max|d| = {(got_x - want_x).abs().max():.3e} (max|ref| {want_x.abs().max():.3f})")
        assert torch.allclose(got_x, want_x, rtol=1e-4, atol=2e-4), (r, (got_x - want_x).abs().max())
        assert torch.equal(again, got_x), f"dgrad ({r}): not bit-identical from run to run"


# ---- a down block and an up block ------------------------------------------------------------------------------------------------------------------
BLOCKS = {"down": (2, 64, 128, 10, 14), "up": (2, 128, 64, 5, 7)}


@pytest.fixture(scope="module")
def block_refs():
    """per block: parameters, inputs, the exact fp64 gradients, the fp32 autograd ones and the fp64 restatement with the device's rounding points"""
    refs = {}
    for i, (kind, (B, cin, cout, H, W)) in enumerate(BLOCKS.items()):
        p = rs_block_params(kind, cin, cout, seed=70 + 10 * i, dtype=torch.float32)
        x = _rand((B, cin, H, W), 80 + i) + 0.5
        oh, ow = (H // 2, W // 2) if kind == "down" else (2 * H, 2 * W)
        dy = _rand((B, cout, oh, ow), 90 + i)
        p64 = {k: v.double() for k, v in p.items()}
        _, dx64, g64 = rs_block_autograd(kind, p64, x.double(), dy.double())
        _, dx32, g32 = rs_block_autograd(kind, p, x, dy)
        fold = bf16_round_keep if kind == "up" else None          # the default route of Upsample2D is the folded one
        _, saved = rs_block_forward_ref(kind, p64, x.double(), rnd=bf16_round_keep, fold_rnd=fold)
        dxe, ge = rs_block_backward_ref(kind, p64, saved, dy.double(), rnd=bf16_round_keep, fold_rnd=fold)
        refs[kind] = dict(p=p, x=x, dy=dy, exact=dict(g64, dx=dx64), f32=dict(g32, dx=dx32), emu=dict(ge, dx=dxe))
    return refs


def _rel(a, ref):
    return ((a.double() - ref).abs().max() / ref.abs().max()).item()


@pytest.mark.parametrize("kind", list(BLOCKS))
def test_block_backward(vb, block_refs, kind):
    """one resnet with a channel change, one without, and the resampling layer: every gradient within max(1.5 d_emu, 4 e32, 1e-7) of fp64 autograd"""
    r = block_refs[kind]
    p = {k: v.to(DEV).contiguous() for k, v in r["p"].items()}
    x, dy = dev32(r["x"]), dev32(r["dy"])
    fwd, bwd = (vb.down_block_forward_train, vb.down_block_backward) if kind == "down" else (vb.up_block_forward_train, vb.up_block_backward)
    y, saved = fwd(p, x)
    assert tuple(y.shape) == tuple(dy.shape)
    dx, grads = bwd(p, saved, dy)
    dx2, grads2 = bwd(p, saved, dy)
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
        print(f"    {kind} {k}: d_hip {d_hip:.3e}  d_emu {d_emu:.3e}  e32 {e32:.3e}  d_hip / bound {d_hip / bound:.3f}")
        if not d_hip <= bound:
            failed.append(k)
    assert not failed, failed


def test_groupnorm_backward_two_channels_per_group(vb):
    """the 64-channel resnet of the down block has 2 channels per group (a lane's 4 channels span two groups): statistics and GroupNorm + SiLU
    backward against autograd, by the rule"""
    from test_train_device import check
    B, C, H, W = 2, 64, 5, 7
    x, da = _rand((B, C, H, W), 101) + 3.0, _rand((B, C, H, W), 102)
    gamma, beta = 1 + 0.2 * _rand((C,), 103), 0.2 * _rand((C,), 104)

    def autograd(dtype):
        xs, g, b = (t.to(dtype).clone().requires_grad_(True) for t in (x, gamma, beta))
        return torch.autograd.grad(F.silu(F.group_norm(xs, 32, g, b, 1e-6)), [xs, g, b], da.to(dtype))

    xd = dev32(x)
    stats = vb.groupnorm_stats(xd)
    dx, _, dg, db = vb.groupnorm_silu_backward(xd, stats, gamma.to(DEV), beta.to(DEV), dev32(da))
    torch.cuda.synchronize()
    xg = x.double().reshape(B, 32, -1)
    check("mean", stats[:, :, 0].cpu(), xg.mean(2), xg.float().mean(2))
    want64, want32 = autograd(torch.float64), autograd(torch.float32)
    check("dx", nchw(dx.cpu()), want64[0], want32[0])
    check("dgamma", dg.cpu(), want64[1], want32[1])
    check("dbeta", db.cpu(), want64[2], want32[2])


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(vb):
    """the error code, a message, and nothing written"""
    from vae_tagger_amd._lib import VTError
    ctx = vb.context(DEV)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    bf, SENT = torch.bfloat16, 7.0
    z16 = lambda *s: torch.zeros(*s, device=DEV, dtype=bf)
    out = lambda *s: torch.full(s, SENT, device=DEV)
    untouched = lambda t: bool((t == SENT).all())
    # channels not a multiple of 8
    dx = out(1, 4, 4, 12)
    with pytest.raises(VTError, match="multiples of 8"):
        ctx.call("vt_op_conv_s2_backward_data", vp(z16(1, 2, 2, 64)), vp(torch.zeros(64, 12, 3, 3, device=DEV)), None, vp(dx), 1, 4, 4, 12, 64, None)
    assert untouched(dx)
    dx = out(1, 2, 2, 12)
    with pytest.raises(VTError, match="multiple of 8"):
        ctx.call("vt_op_upsample2x_conv3x3_backward_data", vp(z16(1, 4, 4, 12)), vp(torch.zeros(12, 12, 3, 3, device=DEV)), None, vp(dx), 1, 2, 2, 12, None)
    assert untouched(dx)
    # the weight gradients take multiples of 64 only
    with pytest.raises(VTError, match="multiples of 64"):
        vb.downsample_backward_weight(z16(1, 2, 2, 64), z16(1, 4, 4, 72))
    with pytest.raises(VTError, match="multiples of 64"):
        vb.upsample_backward_weight(z16(1, 4, 4, 72), z16(1, 2, 2, 72))
    # H < 2
    dx, w64 = out(1, 1, 4, 64), torch.zeros(64, 64, 3, 3, device=DEV)
    with pytest.raises(VTError, match="H, W >= 2"):
        ctx.call("vt_op_conv_s2_backward_data", vp(z16(1, 1, 2, 64)), vp(w64), None, vp(dx), 1, 1, 4, 64, 64, None)
    assert untouched(dx)
    dw, ws = out(64, 64, 3, 3), torch.zeros(1 << 20, device=DEV, dtype=torch.uint8)
    with pytest.raises(VTError, match="2 x 2"):
        ctx.call("vt_op_conv_s2_backward_weight", vp(z16(1, 1, 2, 64)), vp(z16(1, 1, 4, 64)), vp(dw), 1, 1, 4, 64, 64, 0, vp(ws), ws.numel(), None)
    assert untouched(dw)
    # a null buffer
    dx = out(1, 4, 4, 64)
    with pytest.raises(VTError, match="null"):
        ctx.call("vt_op_conv_s2_backward_data", None, vp(w64), None, vp(dx), 1, 4, 4, 64, 64, None)
    with pytest.raises(VTError, match="null"):
        ctx.call("vt_op_upsample2x_conv3x3_backward_data", vp(z16(1, 8, 8, 64)), None, None, vp(dx), 1, 4, 4, 64, None)
    assert untouched(dx)
    with pytest.raises(VTError, match="null"):
        ctx.call("vt_op_conv_s2_backward_weight", vp(z16(1, 2, 2, 64)), None, vp(dw), 1, 4, 4, 64, 64, 0, vp(ws), ws.numel(), None)
    with pytest.raises(VTError, match="null"):
        ctx.call("vt_op_upsample2x_conv3x3_backward_weight", None, vp(z16(1, 4, 4, 64)), vp(dw), 1, 4, 4, 64, 0, vp(ws), ws.numel(), None)
    assert untouched(dw)
    # a workspace one byte short
    for name, args, need in (("vt_op_conv_s2_backward_weight", (vp(z16(1, 2, 2, 64)), vp(z16(1, 4, 4, 64)), vp(dw), 1, 4, 4, 64, 64, 0),
                              ctx.lib.vt_op_conv_s2_backward_weight_workspace_bytes(1, 4, 4, 64, 64, 0)),
                             ("vt_op_upsample2x_conv3x3_backward_weight", (vp(z16(1, 8, 8, 64)), vp(z16(1, 4, 4, 64)), vp(dw), 1, 4, 4, 64, 0),
                              ctx.lib.vt_op_upsample2x_conv3x3_backward_weight_workspace_bytes(1, 4, 4, 64, 0))):
        assert 0 < need <= ws.numel()
        with pytest.raises(VTError, match="workspace"):
            ctx.call(name, *args, vp(ws), need - 1, None)
        torch.cuda.synchronize()
        assert untouched(dw), name
        ctx.call(name, *args, vp(ws), need, None)
        torch.cuda.synchronize()
        assert not dw.any(), name              # zero operands: the accepted call wrote zeros
        dw.fill_(SENT)
    # the block functions while flag 18 is on
    p = {k: v.to(DEV) for k, v in rs_block_params("down", 64, 64, seed=1, dtype=torch.float32).items()}
    x = torch.zeros(1, 4, 4, 64, device=DEV)
    y, saved = vb.down_block_forward_train(p, x)
    pu = {k: v.to(DEV) for k, v in rs_block_params("up", 64, 64, seed=2, dtype=torch.float32).items()}
    yu, savedu = vb.up_block_forward_train(pu, x)
    ctx.call("vt_set_flag", 18, 1)
    try:
        for fn, args in ((vb.down_block_forward_train, (p, x)), (vb.down_block_backward, (p, saved, torch.zeros_like(y))),
                         (vb.up_block_forward_train, (pu, x)), (vb.up_block_backward, (pu, savedu, torch.zeros_like(yu)))):
            with pytest.raises(VTError, match="fp16"):
                fn(*args)
    finally:
        ctx.call("vt_set_flag", 18, 0)
    torch.cuda.synchronize()
