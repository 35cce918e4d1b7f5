"""Host-side checks of the resnet block's backward: the ABI surface, the CPU restatements the device tests lean on (fp64, against autograd), and a
compile-only look at the weight-gradient kernel (needs only hipcc)."""
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

from _conv_backward_ref import (bf16_round_keep, block_autograd, block_backward_ref, block_forward_ref, block_params, dgrad_ref, gn_silu_backward_ref,
                                wgrad_ref)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vae_tagger_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

NEW_ENTRIES = ["vt_op_cast_bias_grad_workspace_bytes", "vt_op_cast_bias_grad", "vt_op_conv_backward_data", "vt_op_conv_backward_weight_workspace_bytes",
               "vt_op_conv_backward_weight", "vt_op_backward_operands_check", "vt_op_groupnorm_stats_workspace_bytes", "vt_op_groupnorm_stats",
               "vt_op_groupnorm_silu_backward_workspace_bytes",
               "vt_op_groupnorm_silu_backward"]


def _randint(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).double()


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def test_abi_surface():
    """every new entry is declared in the header and bound in _lib.PROTOTYPES with the header's number of arguments"""
    from vae_tagger_amd import _lib
    text = open(os.path.join(ROOT, "include", "vae_tagger_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in NEW_ENTRIES:
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} is not declared in include/vae_tagger_hip.h"
        args = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
        assert name in _lib.PROTOTYPES, f"{name} is not in _lib.PROTOTYPES"
        assert len(_lib.PROTOTYPES[name][1]) == len(args), (name, len(_lib.PROTOTYPES[name][1]), len(args))


@pytest.mark.parametrize("k", [1, 3])
def test_dgrad_restatement_is_exact_on_integers(k):
    dy, w = _randint((2, 6, 5, 7), -1, 1, 1), _randint((6, 4, k, k), -2, 2, 2)
    want = torch.nn.grad.conv2d_input((2, 4, 5, 7), w, dy, padding=k // 2)
    assert torch.equal(dgrad_ref(dy, w), want)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("slices", [1, 3, 7])
def test_wgrad_restatement_is_exact_on_integers(k, slices):
    dy, a = _randint((2, 6, 5, 7), -1, 1, 3), _randint((2, 4, 5, 7), -2, 2, 4)
    want = torch.nn.grad.conv2d_weight(a, (6, 4, k, k), dy, padding=k // 2)
    assert torch.equal(wgrad_ref(dy, a, k, slices=slices), want)


@pytest.mark.parametrize("C,zero_gamma", [(128, False), (256, True)])
def test_groupnorm_silu_backward_formulas_match_autograd(C, zero_gamma):
    x = (5.0 + _rand((2, C, 3, 5), 5)).requires_grad_(True)
    gamma = (1 + 0.3 * _rand((C,), 6))
    if zero_gamma:
        gamma[[0, 7, 130]] = 0.0
    gamma.requires_grad_(True)
    beta = (0.3 * _rand((C,), 7)).requires_grad_(True)
    da, add = _rand((2, C, 3, 5), 8), _rand((2, C, 3, 5), 9)
    a = F.silu(F.group_norm(x, 32, gamma, beta, 1e-6))
    gx, gg, gb = torch.autograd.grad(a, [x, gamma, beta], da)
    dx, dg, db = gn_silu_backward_ref(x.detach(), gamma.detach(), beta.detach(), da, dx_add=add)
    for name, got, want in (("dx", dx - add, gx), ("dgamma", dg, gg), ("dbeta", db, gb)):
        err = (got - want).abs().max().item()
        print(f"{name}: max|d| = {err:.3e}")
        assert err <= 1e-12, name


@pytest.mark.parametrize("cin,cout", [(64, 64), (64, 128)], ids=["identity", "conv_shortcut"])
def test_block_restatement_matches_autograd(cin, cout):
    p = block_params(cin, cout, seed=11)
    x, dy = 0.5 + _rand((2, cin, 5, 6), 12), _rand((2, cout, 5, 6), 13)
    y_ref, dx_ref, g_ref = block_autograd(p, x, dy)
    y, saved = block_forward_ref(p, x)
    dx, g = block_backward_ref(p, saved, dy)
    assert torch.equal(y, y_ref)
    assert list(g) == list(p) and all(g[k].shape == p[k].shape for k in p)
    for name, got, want in [("dx", dx, dx_ref)] + [(k, g[k], g_ref[k]) for k in p]:
        err = ((got - want).abs().max() / want.abs().max()).item()
        print(f"{name}: relative error {err:.3e}")
        assert err <= 1e-12, name
    # with the device's rounding points the restatement stays a small perturbation of the exact gradient
    y16, saved16 = block_forward_ref(p, x, rnd=bf16_round_keep)
    dx16, _ = block_backward_ref(p, saved16, dy, rnd=bf16_round_keep)
    assert ((dx16 - dx_ref).abs().max() / dx_ref.abs().max()).item() < 0.05


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_wgrad_unit_compiles_to_transposed_reads_without_scratch(tmp_path):
    out = tmp_path / "conv_wgrad.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "-S", "--cuda-device-only", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), "-o", str(out), os.path.join(CSRC, "conv_wgrad.hip")],
                   check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    text = out.read_text()
    blocks, cur = [], None
    for l in text.split("\n"):
        if re.match(r"^\s+- \.\w+:", l):
            cur = {}; blocks.append(cur)
        m = re.match(r"^\s+(?:- )?\.(\w+):\s+(\S+)\s*$", l)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
    kernels = {b["name"]: b for b in blocks if "name" in b and "vgpr_count" in b}
    wgrad = [k for k in kernels if "conv_wgrad_kernel" in k]
    assert len(wgrad) == 2, sorted(kernels)                      # the 3x3 and the 1x1 form
    for k in wgrad:
        b = kernels[k]
        assert int(b["private_segment_fixed_size"]) == 0, (k, b["private_segment_fixed_size"])
        assert int(b["vgpr_spill_count"]) == 0 and int(b["sgpr_spill_count"]) == 0, k
        assert int(b["group_segment_fixed_size"]) % 16 == 0, k    # no static LDS in front of the dynamic region
        body = text[text.index(k + ":"):]
        body = body[:body.index("s_endpgm")]
        assert "ds_read_b64_tr_b16" in body, k
        assert re.search(r"v_mfma_f32_(16x16x32|32x32x16)_bf16", body), k
