"""Upsample2D (nearest 2x + conv3x3) on the device, through vt_op_upsample2x_conv3x3: the folded kernel (conv3x3_up2.hip) and the
literal route (vt_set_flag 22).  Exact where the arithmetic is exact (one-hot taps, small integers); elsewhere against the fp32 evaluation of
the same operand-rounded numbers, so the tolerance is accumulation order (test_conv2d_matches_torch's bound)."""
import pytest
import torch
import torch.nn.functional as F

from _util import Ops, bf16_round, nchw, nhwc, vp
from _vae_decode_ref import fold_weights, folded_upsample_conv, literal_upsample_conv

pytestmark = pytest.mark.gpu

# B, C, h, w: tiny; ragged; exactly one 16-wide tile; one row and one column past a tile edge; several cout tiles and images
SHAPES = [(1, 64, 5, 7), (2, 128, 9, 13), (1, 256, 16, 16), (1, 256, 17, 33), (3, 512, 8, 24)]
MODES = ["bf16", "fp16"]


@pytest.fixture(scope="module")
def ops():
    return Ops()


def f16_round(t):
    return t.to(torch.float16).to(torch.float32)


def _round(mode):
    return f16_round if mode == "fp16" else bf16_round


def up2(ops, x_nchw, w_oihw, bias, mode="bf16", literal=False, gn=None):
    """x: values already representable in the operand type.  -> fp32 NCHW [B, C, 2h, 2w] (and, with gn = (gamma, beta), the (scale, shift))"""
    B, C, h, w = x_nchw.shape
    x = nhwc(x_nchw).to(ops.dev, torch.float16 if mode == "fp16" else torch.bfloat16)
    wd = w_oihw.to(ops.dev, torch.float32).contiguous()
    b = bias.to(ops.dev, torch.float32).contiguous() if bias is not None else None
    out = torch.full((B, 2 * h, 2 * w, C), float("nan"), device=ops.dev, dtype=torch.float32)
    ops.ctx.call("vt_set_flag", 18, int(mode == "fp16"))
    ops.ctx.call("vt_set_flag", 22, int(literal))
    try:
        if gn is None:
            ops.ctx.call("vt_op_upsample2x_conv3x3", vp(x), vp(wd), vp(b), vp(out), B, h, w, C, ops.stream)
        else:
            g, bt = (t.to(ops.dev, torch.float32).contiguous() for t in gn)
            ss = torch.zeros(B, C, 2, device=ops.dev, dtype=torch.float32)
            ops.ctx.call("vt_op_upsample2x_conv3x3_gn", vp(x), vp(wd), vp(b), vp(out), B, h, w, C, 32, 1e-6, vp(g), vp(bt), vp(ss), ops.stream)
        torch.cuda.synchronize()
    finally:
        ops.ctx.call("vt_set_flag", 18, 0)
        ops.ctx.call("vt_set_flag", 22, 0)
    return nchw(out.cpu()) if gn is None else (nchw(out.cpu()), ss.cpu())


def _rand(shape, seed, scale=1.0):
    return scale * torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _randint(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def test_fold_restatement_is_exact_on_integers():
    """(the CPU restatement the other tests lean on, checked where it runs beside them too)"""
    x = _randint((2, 64, 5, 7), -2, 2, 1)
    w = _randint((64, 64, 3, 3), -1, 1, 2)
    assert torch.equal(folded_upsample_conv(x, w), literal_upsample_conv(x, w))


@pytest.mark.parametrize("literal", [False, True], ids=["folded", "literal"])
def test_one_hot_taps_exact(ops, literal):
    """w[o, o, ky, kx] = 1, one tap at a time, on an asymmetric integer ramp: a swapped phase, shift or folded-tap index is a wrong pixel."""
    C = 128
    x = torch.arange(2 * C * 7 * 19, dtype=torch.float32).reshape(2, C, 7, 19) % 251 - 125.0
    for tap in range(9):
        w = torch.zeros(C, C, 3, 3)
        w[torch.arange(C), torch.arange(C), tap // 3, tap % 3] = 1.0
        got = up2(ops, x, w, None, literal=literal)
        assert torch.equal(got, literal_upsample_conv(x, w)), f"tap {tap}"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,C,h,w", SHAPES)
def test_integer_data_exact(ops, B, C, h, w, mode):
    """inputs in {-2..2}, weights in {-1, 0, 1}, integer bias: folded weights are integers of magnitude <= 4, every partial sum an integer
    below 2^24, so the fp32 output equals the torch reference exactly"""
    x = _randint((B, C, h, w), -2, 2, 11)
    wt = _randint((C, C, 3, 3), -1, 1, 12)
    b = _randint((C,), -3, 3, 13)
    ref = literal_upsample_conv(x, wt, b)
    assert ref.abs().max() < 2 ** 24
    got = up2(ops, x, wt, b, mode=mode)
    assert got.shape == ref.shape and torch.equal(got, ref), (got - ref).abs().max()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,C,h,w", SHAPES)
def test_random_data_matches_folded_reference(ops, B, C, h, w, mode):
    rnd = _round(mode)
    x = rnd(_rand((B, C, h, w), 21))
    wt = _rand((C, C, 3, 3), 22, (C * 9) ** -0.5)
    b = _rand((C,), 23, 0.1)
    ref = folded_upsample_conv(x, wt, b, round_fn=rnd)
    got = up2(ops, x, wt, b, mode=mode)
    print(f"{mode} {B}x{C}x{h}x{w}: max|d| = {(got - ref).abs().max():.3e}")
    assert torch.allclose(got, ref, rtol=1e-4, atol=2e-4), (got - ref).abs().max()


def _dyadic_weights(C, seed):
    """multiples of 2^-9 in [-2^-5, 2^-5]: every weight AND every folded sum of up to four of them is exact in bf16 and fp16, so the two
    routes evaluate the same numbers and differ by accumulation order only"""
    wt = _randint((C, C, 3, 3), -16, 16, seed) / 512.0
    assert torch.equal(bf16_round(fold_weights(wt)), fold_weights(wt))
    return wt


ROUTE_CASES = [(s, m) for s in SHAPES for m in MODES if not (m == "fp16" and s[1] < 128)]     # (the literal route has no fp16 kernel at 64 channels)


@pytest.mark.parametrize("shape,mode", ROUTE_CASES)
def test_routes_agree_and_are_deterministic(ops, shape, mode):
    B, C, h, w = shape
    x = _round(mode)(_rand((B, C, h, w), 31))
    wt = _dyadic_weights(C, 32)
    b = _rand((C,), 33, 0.1)
    ref = folded_upsample_conv(x, wt, b)
    outs = {}
    for literal in (False, True):
        got = up2(ops, x, wt, b, mode=mode, literal=literal)
        again = up2(ops, x, wt, b, mode=mode, literal=literal)
        assert torch.equal(got, again), ("literal" if literal else "folded", "not bit-identical from run to run")
        assert torch.allclose(got, ref, rtol=1e-4, atol=2e-4), ("literal" if literal else "folded", (got - ref).abs().max())
        outs[literal] = got
    assert torch.allclose(outs[False], outs[True], rtol=1e-4, atol=2e-4)


def test_literal_route_without_an_fp16_kernel_is_an_error(ops):
    from vae_tagger_amd._lib import VTError
    x = torch.zeros(1, 64, 4, 4)
    with pytest.raises(VTError, match="fp16"):
        up2(ops, x, torch.zeros(64, 64, 3, 3), None, mode="fp16", literal=True)


@pytest.mark.parametrize("literal", [False, True], ids=["folded", "literal"])
@pytest.mark.parametrize("B,C,h,w", [(2, 128, 9, 13), (1, 256, 17, 33)])
def test_epilogue_groupnorm_partials(ops, B, C, h, w, literal):
    """the (n, mean, M2) partials of the epilogue, finalised by the existing kernel, reproduce GroupNorm of the output
    (test_conv_epilogue_groupnorm_statistics' setting and tolerance: a large common offset, mean >> std inside groups)"""
    x = bf16_round(_rand((B, C, h, w), 41))
    wt = _rand((C, C, 3, 3), 42, (C * 9) ** -0.5)
    b = _rand((C,), 43, 0.1) + 3.0
    g = 1 + 0.1 * _rand((C,), 44)
    bt = 0.1 * _rand((C,), 45)
    out, ss = up2(ops, x, wt, b, literal=literal, gn=(g, bt))
    ref = literal_upsample_conv(x, bf16_round(wt), b) if literal else folded_upsample_conv(x, wt, b, round_fn=bf16_round)
    assert torch.allclose(out, ref, rtol=1e-4, atol=2e-4), (out - ref).abs().max()
    want = F.group_norm(ref, 32, g, bt, eps=1e-6)
    got = out * ss[:, :, 0].view(B, C, 1, 1) + ss[:, :, 1].view(B, C, 1, 1)
    assert torch.allclose(got, want, rtol=1e-3, atol=1e-3), (got - want).abs().max()
