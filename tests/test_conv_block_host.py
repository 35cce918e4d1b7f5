"""CPU: the fp64 reference the device suite (test_conv_block_device.py) holds vt_op_conv3x3_block to is itself checked here, against
torch.nn.functional.conv2d in fp64 and against the layout the header documents."""
import pytest
import torch
import torch.nn.functional as F

from _conv_block_ref import conv_block_ref, conv_sum, group_norm, planar_pack, planar_unpack


def _rand(shape, seed, scale=1.0):
    return scale * torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


@pytest.mark.parametrize("B,H,W,Cin,Cout,sc", [(2, 9, 7, 32, 128, 64), (1, 5, 6, 64, 128, 0), (2, 1, 1, 32, 128, 32)])
def test_stride1_reference_is_conv2d_plus_shortcut_conv_plus_residual(B, H, W, Cin, Cout, sc):
    x, w, b = _rand((B, H, W, Cin), 1), _rand((Cout, Cin, 3, 3), 2, 0.1), _rand((Cout,), 3)
    res = _rand((B, H, W, Cout), 4)
    want = F.conv2d(_nchw(x), w, b, padding=1) + _nchw(res)
    sx = sw = None
    if sc:
        sx, sw = _rand((B, H, W, sc), 5), _rand((Cout, sc), 6, 0.1)
        want = want + F.conv2d(_nchw(sx), sw.view(Cout, sc, 1, 1))
    got = conv_sum(x, w, b, 1, sx, sw, res)
    assert got.dtype == torch.float64 and got.shape == (B, H, W, Cout)
    assert torch.allclose(_nchw(got), want, rtol=1e-12, atol=1e-12), (_nchw(got) - want).abs().max()


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 10, 8, 32, 128), (1, 11, 7, 64, 128), (1, 2, 3, 32, 128)])
def test_stride2_reference_is_downsample2d(B, H, W, Cin, Cout):
    """Downsample2D(padding=0): F.pad(x, (0, 1, 0, 1)) then a stride-2 conv; out = floor(in / 2), even and odd sizes"""
    x, w, b = _rand((B, H, W, Cin), 7), _rand((Cout, Cin, 3, 3), 8, 0.1), _rand((Cout,), 9)
    res = _rand((B, H // 2, W // 2, Cout), 10)
    want = F.conv2d(F.pad(_nchw(x), (0, 1, 0, 1)), w, b, stride=2) + _nchw(res)
    got = conv_sum(x, w, b, 2, residual=res)
    assert got.shape == (B, H // 2, W // 2, Cout)
    assert torch.allclose(_nchw(got), want, rtol=1e-12, atol=1e-12), (_nchw(got) - want).abs().max()


def test_asymmetric_one_hot_taps_read_the_right_pixel():
    """the reference itself must not have a swapped tap: one-hot weights on the integer ramp the device tests use"""
    Cin = Cout = 32
    x = (torch.arange(2 * 6 * 10 * Cin, dtype=torch.float64).reshape(2, 6, 10, Cin) % 251) - 125.0
    for stride in (1, 2):
        for tap in range(9):
            w = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64)
            w[torch.arange(Cout), torch.arange(Cin), tap // 3, tap % 3] = 1.0
            pad = (1, 1, 1, 1) if stride == 1 else (0, 1, 0, 1)
            want = F.conv2d(F.pad(_nchw(x), pad), w, stride=stride)
            assert torch.equal(_nchw(conv_sum(x, w, torch.zeros(Cout), stride)), want), (stride, tap)


def test_group_norm_reference_is_torch_group_norm():
    v, g, b = _rand((2, 7, 5, 128), 11) + 3.0, 1 + 0.1 * _rand((128,), 12), 0.1 * _rand((128,), 13)
    want = F.group_norm(_nchw(v), 32, g, b, eps=1e-6)
    assert torch.allclose(_nchw(group_norm(v, 32, g, b, 1e-6)), want, rtol=1e-11, atol=1e-11)


def test_planar_layout_round_trips_and_matches_the_documented_index():
    """Conv3x3Args::out16_planar: [Cout/32][H][W][32] per image -- element (b, y, x, c) at (((b * (C/32) + c/32) * H + y) * W + x) * 32 + c % 32"""
    B, H, W, C = 2, 5, 7, 128
    t = torch.arange(B * H * W * C, dtype=torch.int32).reshape(B, H, W, C)
    p = planar_pack(t)
    assert p.shape == (B, C // 32, H, W, 32) and p.is_contiguous()
    assert torch.equal(planar_unpack(p), t)
    assert torch.equal(planar_pack(planar_unpack(p)), p)
    b, y, x, c = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W), torch.arange(C), indexing="ij")
    idx = (((b * (C // 32) + c // 32) * H + y) * W + x) * 32 + c % 32
    assert torch.equal(p.reshape(-1)[idx.reshape(-1)].reshape(B, H, W, C), t)          # reading the documented address gives the NHWC element
    flat = torch.empty(B * H * W * C, dtype=torch.int32)
    flat[idx.reshape(-1)] = t.reshape(-1)                                               # writing it there gives the packed tensor
    assert torch.equal(flat.reshape(p.shape), p)


def test_block_reference_returns_every_stored_form():
    x = _rand((1, 4, 5, 32), 14).bfloat16().double()
    w = _rand((128, 32, 3, 3), 15, 0.06).bfloat16().double()
    res = _rand((1, 4, 5, 128), 16).half().double()
    g, bt = torch.ones(128), torch.zeros(128)
    r = conv_block_ref(x, w, _rand((128,), 17), residual=res, copy_f16=False, groups=32, gamma=g, beta=bt)
    assert r["v"].dtype == torch.float64 and r["f16"].dtype == torch.float16 and r["copy"].dtype == torch.bfloat16
    assert torch.equal(r["f16"], r["v"].float().half()) and torch.equal(r["copy"], r["v"].float().bfloat16())
    assert torch.equal(planar_unpack(r["copy_planar"]), r["copy"])
    assert torch.equal(r["gn"], group_norm(r["v"], 32, g, bt))
    assert conv_block_ref(x, w, torch.zeros(128), copy_f16=True)["copy"].dtype == torch.float16
