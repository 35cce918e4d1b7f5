"""Host-side checks of the resampling layers' backward (Downsample2D's stride-2 conv, Upsample2D): the CPU restatements the device tests lean on
against fp64 autograd, the ABI surface, the workspace arithmetic, and a compile-only look at the new kernels' code objects (needs only hipcc)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from _resample_backward_ref import (down_forward_ref, rs_block_autograd, rs_block_backward_ref, rs_block_forward_ref, rs_block_params, s2_dgrad_literal_ref,
                                    s2_dgrad_phase_ref, s2_wgrad_ref, up2_dgrad_gather_ref, up2_dgrad_literal_ref, up2_fold, up2_forward_folded_ref,
                                    up2_wgrad_ref, up_forward_ref)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vae_tagger_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

NEW_ENTRIES = ["vt_op_conv_s2_backward_data", "vt_op_conv_s2_backward_weight_workspace_bytes", "vt_op_conv_s2_backward_weight",
               "vt_op_upsample2x_conv3x3_backward_data", "vt_op_upsample2x_conv3x3_backward_weight_workspace_bytes",
               "vt_op_upsample2x_conv3x3_backward_weight"]
DOWN_SIZES = [(2, 2), (3, 2), (5, 7), (6, 8)]
UP_SIZES = [(1, 1), (2, 3), (3, 5)]
TOL = 1e-12           # fp64, a few dozen terms of size ~1 per sum


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _autograd(forward, x, w, dy):
    x, w = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    return torch.autograd.grad(forward(x, w), [x, w], dy)


def _close(name, got, want):
    err = (got - want).abs().max().item()
    print(f"{name}: max|d| = {err:.3e}")
    assert got.shape == want.shape and err <= TOL, name


@pytest.mark.parametrize("H,W", DOWN_SIZES)
def test_stride2_formulations_match_autograd(H, W):
    """the 9-product phase data gradient, the scatter-to-odd-positions literal route and the weight gradient, odd and even sizes down to 2 x 2"""
    x, w, dy = _rand((2, 3, H, W), 1), _rand((4, 3, 3, 3), 2), _rand((2, 4, H // 2, W // 2), 3)
    gx, gw = _autograd(down_forward_ref, x, w, dy)
    _close("dgrad, 9 products", s2_dgrad_phase_ref(dy, w, H, W), gx)
    _close("dgrad, literal", s2_dgrad_literal_ref(dy, w, H, W), gx)
    _close("wgrad", s2_wgrad_ref(dy, x), gw)


@pytest.mark.parametrize("h,w", UP_SIZES)
def test_upsample_formulations_match_autograd(h, w):
    """the folded forward, the folded 16-product gather, the literal route with its 2x2 sum and the weight gradient, down to 1 x 1"""
    x, wt, dy = _rand((2, 3, h, w), 4), _rand((3, 3, 3, 3), 5), _rand((2, 3, 2 * h, 2 * w), 6)
    gx, gw = _autograd(up_forward_ref, x, wt, dy)
    wf = up2_fold(wt)
    _close("folded forward", up2_forward_folded_ref(x, wf), up_forward_ref(x, wt))
    _close("dgrad, 16-product gather", up2_dgrad_gather_ref(dy, wf), gx)
    _close("dgrad, literal", up2_dgrad_literal_ref(dy, wt), gx)
    _close("wgrad", up2_wgrad_ref(dy, x), gw)


@pytest.mark.parametrize("kind,cin,cout,H,W", [("down", 32, 64, 5, 6), ("up", 128, 64, 3, 4)])
def test_block_restatement_matches_autograd(kind, cin, cout, H, W):
    p = rs_block_params(kind, cin, cout, seed=21)
    x = 0.5 + _rand((2, cin, H, W), 22)
    y_ref, _ = rs_block_forward_ref(kind, p, x)
    dy = _rand(tuple(y_ref.shape), 23)
    _, dx_ref, g_ref = rs_block_autograd(kind, p, x, dy)
    for fold in ([None] if kind == "down" else [None, lambda t: t]):
        y, saved = rs_block_forward_ref(kind, p, x, fold_rnd=fold)
        dx, g = rs_block_backward_ref(kind, p, saved, dy, fold_rnd=fold)
        assert list(g) == list(p)
        # (the folded route sums the taps in fp32: its restatement is exact to fp32's rounding of those sums only)
        tol = 1e-12 if fold is None else 1e-6
        for name, got, want in [("y", y, y_ref), ("dx", dx, dx_ref)] + [(k, g[k], g_ref[k]) for k in p]:
            err = ((got - want).abs().max() / want.abs().max()).item()
            assert got.shape == want.shape and err <= tol, (name, err)


def test_abi_surface():
    """every new entry is declared in the header, bound in _lib.PROTOTYPES with the header's number of arguments and result type, and exported by the
    built library"""
    from vae_tagger_amd import _lib
    text = open(os.path.join(ROOT, "include", "vae_tagger_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRIES:
        m = re.search(r"\b(int|size_t)\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} is not declared in include/vae_tagger_hip.h"
        args = [a.strip() for a in m.group(2).split(",") if a.strip() and a.strip() != "void"]
        assert name in _lib.PROTOTYPES, f"{name} is not in _lib.PROTOTYPES"
        res, bound = _lib.PROTOTYPES[name]
        assert len(bound) == len(args), (name, len(bound), len(args))
        assert res is (ctypes.c_size_t if m.group(1) == "size_t" else ctypes.c_int), name
        for a, t in zip(args, bound):
            if "*" in a:
                assert t is ctypes.c_void_p, (name, a)
            elif a.startswith("size_t"):
                assert t is ctypes.c_size_t, (name, a)
            else:
                assert a.startswith("int ") and t is ctypes.c_int, (name, a)
        assert hasattr(lib, name), f"{name} is not exported by {_lib.LIB_PATH}"


def test_workspace_sizes_are_host_arithmetic():
    """no device, no context: tiles of (2 x 32) dy pixels for the stride-2 form and (6 x 32) for the upsample form, `splits` clamped to the tile count,
    0 = two workgroups per CU, rounded up to 256 bytes"""
    from vae_tagger_amd import _lib
    lib = _lib.load()
    s2, up = lib.vt_op_conv_s2_backward_weight_workspace_bytes, lib.vt_op_upsample2x_conv3x3_backward_weight_workspace_bytes
    cdiv = lambda a, b: -(-a // b)
    al = lambda n: cdiv(n, 256) * 256
    for B, H, W, Cin, Cout in [(1, 5, 7, 64, 64), (2, 10, 14, 128, 128), (1, 34, 66, 256, 256), (1, 9, 12, 64, 128), (16, 1024, 1024, 128, 128)]:
        tiles = B * cdiv(H // 2, 2) * cdiv(W // 2, 32)
        auto = max(1, min(tiles, 512 // ((Cin // 64) * (Cout // 64))))
        for splits, eff in [(1, 1), (2, min(2, tiles)), (3, min(3, tiles)), (0, auto), (tiles + 1, tiles), (2 ** 30, tiles)]:
            assert s2(B, H, W, Cin, Cout, splits) == al(eff * Cout * Cin * 9 * 4), (B, H, W, Cin, Cout, splits)
        assert s2(B, H, W, Cin, Cout, 3) == s2(B, H, W, Cin, Cout, 3)
    for B, h, w, C in [(1, 3, 5, 64), (2, 5, 7, 128), (1, 9, 17, 256), (2, 4, 12, 512), (1, 512, 512, 256)]:
        tiles = B * cdiv(2 * h, 6) * cdiv(2 * w, 32)
        auto = max(1, min(tiles, 512 // ((C // 64) ** 2)))
        for splits, eff in [(1, 1), (2, min(2, tiles)), (3, min(3, tiles)), (0, auto), (tiles + 1, tiles)]:
            assert up(B, h, w, C, splits) == al(eff * C * C * 9 * 4), (B, h, w, C, splits)
    # refused shapes have no workspace
    assert s2(1, 1, 8, 64, 64, 0) == 0 and s2(1, 8, 8, 48, 64, 0) == 0 and s2(1, 8, 8, 64, 64, -1) == 0
    assert up(1, 0, 4, 64, 0) == 0 and up(1, 4, 4, 40, 0) == 0 and up(0, 4, 4, 64, 0) == 0


def _metadata(tmp_path, unit):
    out = tmp_path / (unit + ".s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "-S", "--cuda-device-only", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), "-o", str(out), os.path.join(CSRC, unit + ".hip")],
                   check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    blocks, cur = [], None
    for l in out.read_text().split("\n"):
        if re.match(r"^\s+- \.\w+:", l):
            cur = {}; blocks.append(cur)
        m = re.match(r"^\s+(?:- )?\.(\w+):\s+(\S+)\s*$", l)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
    return {b["name"]: b for b in blocks if "name" in b and "vgpr_count" in b}


CU_LDS = 160 * 1024        # MI355X


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
@pytest.mark.parametrize("unit,kernel,lds", [("conv3x3_s2_dgrad", "conv3x3_s2_dgrad_kernel", 10 * 1024 + 9 * 4096),
                                             ("conv3x3_up2_dgrad", "conv3x3_up2_dgrad_kernel", 2 * 12 * 1024 + 8 * 4096)])
def test_dgrad_code_objects(tmp_path, unit, kernel, lds):
    """no scratch, no spills; the (static) LDS is what the header comment counts and lets two workgroups share a CU, as do the registers
    (4 waves per workgroup = one per SIMD: two workgroups need <= 256 registers per lane)"""
    kernels = _metadata(tmp_path, unit)
    mine = [k for k in kernels if kernel in k]
    assert len(mine) == 1, sorted(kernels)
    b = kernels[mine[0]]
    print({k: b[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size") if k in b})
    assert int(b["private_segment_fixed_size"]) == 0
    assert int(b["vgpr_spill_count"]) == 0 and int(b["sgpr_spill_count"]) == 0
    assert int(b["group_segment_fixed_size"]) == lds and 2 * lds <= CU_LDS
    assert int(b["vgpr_count"]) + int(b.get("agpr_count", 0)) <= 256


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_wgrad_resample_code_objects(tmp_path):
    """the two staging variants: no scratch, no spills, <= 256 registers (two workgroups per CU); their LDS is dynamic (62 240 and 74 240 bytes, set by
    the launcher), so the code object must hold no static LDS in front of it"""
    kernels = _metadata(tmp_path, "conv_wgrad")
    mine = [k for k in kernels if "conv_wgrad_rs_kernel" in k]
    assert len(mine) == 2, sorted(kernels)
    for k in mine:
        b = kernels[k]
        print(k, {f: b[f] for f in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
        assert int(b["private_segment_fixed_size"]) == 0
        assert int(b["vgpr_spill_count"]) == 0 and int(b["sgpr_spill_count"]) == 0
        assert int(b["group_segment_fixed_size"]) == 0
        assert int(b["vgpr_count"]) + int(b.get("agpr_count", 0)) <= 256
