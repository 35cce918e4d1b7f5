"""Host-side checks of the mid-block attention's backward: the formulas the device test relies on (fp64, against autograd), the ABI surface, the
workspace functions, and the built code object's resource metadata for the new kernels."""
import os
import re
import shutil
import subprocess

import pytest
import torch

from _attention_backward_ref import (attn_params, bf16_round_keep, block_autograd, block_backward_ref, block_forward_ref, core_autograd, core_backward_ref,
                                     core_forward_ref, gn_backward_ref)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vae_tagger_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

NEW_ENTRIES = ["vt_op_groupnorm_backward_workspace_bytes", "vt_op_groupnorm_backward", "vt_op_attention_vt_pitch", "vt_op_attention_forward_train_workspace_bytes",
               "vt_op_attention_forward_train", "vt_op_attention_core_backward_workspace_bytes", "vt_op_attention_core_backward",
               "vt_op_attention_core_backward_stages"]


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _rel(a, ref):
    return ((a - ref).abs().max() / ref.abs().max()).item()


def test_block_restatement_matches_autograd():
    """rnd = identity: the hand-written backward equals fp64 autograd on every gradient, B = 2, S = 6 x 7"""
    B, S, C = 2, 6 * 7, 64
    p = attn_params(C, seed=3)
    x, dy = 0.5 + _rand((B, S, C), 4), _rand((B, S, C), 5)
    y_ref, dx_ref, g_ref = block_autograd(p, x, dy)
    y, saved = block_forward_ref(p, x)
    dx, g = block_backward_ref(p, saved, dy)
    assert _rel(y, y_ref) <= 1e-12
    assert list(g) == list(p) and all(g[k].shape == p[k].shape for k in p)
    # (the exact to_k.bias gradient is ZERO -- a bias on k shifts every score of a row alike and softmax does not see it -- so its error has no scale
    #  of its own: it is measured against to_q.bias's gradient, the same kind of sum over the other index)
    for name, got, want in [("dx", dx, dx_ref)] + [(k, g[k], g_ref[k]) for k in p]:
        err = _rel(got, want) if name != "to_k.bias" else ((got - want).abs().max() / g_ref["to_q.bias"].abs().max()).item()
        print(f"{name}: relative error {err:.3e}")
        assert err <= 1e-10, name
    # with the device's rounding points the restatement stays a small perturbation of the exact gradient
    _, saved16 = block_forward_ref(p, x, rnd=bf16_round_keep)
    dx16, _ = block_backward_ref(p, saved16, dy, rnd=bf16_round_keep)
    assert _rel(dx16, dx_ref) < 0.05


def test_core_restatement_matches_autograd():
    q, k, v, do = (_rand((2, 42, 64), s) for s in (6, 7, 8, 9))
    o_ref, *want = core_autograd(q, k, v, do)
    o, sv = core_forward_ref(q, k, v)
    assert _rel(o, o_ref) <= 1e-12
    for name, got, ref in zip(("dq", "dk", "dv"), core_backward_ref(q, k, v, o, do, sv), want):
        assert _rel(got, ref) <= 1e-10, name


def test_groupnorm_backward_formulas_match_autograd():
    x = (5.0 + _rand((2, 15, 128), 10)).requires_grad_(True)
    gamma = 1 + 0.3 * _rand((128,), 11)
    gamma[[0, 7, 100]] = 0.0
    gamma.requires_grad_(True)
    beta = (0.3 * _rand((128,), 12)).requires_grad_(True)
    dh, add = _rand((2, 15, 128), 13), _rand((2, 15, 128), 14)
    h = torch.nn.functional.group_norm(x.transpose(1, 2), 32, gamma, beta, 1e-6).transpose(1, 2)
    gx, gg, gb = torch.autograd.grad(h, [x, gamma, beta], dh)
    dx, dg, db = gn_backward_ref(x.detach(), gamma.detach(), beta.detach(), dh, dx_add=add)
    for name, got, want in (("dx", dx - add, gx), ("dgamma", dg, gg), ("dbeta", db, gb)):
        assert (got - want).abs().max().item() <= 1e-12, name


def test_abi_surface_and_exports():
    """every new entry is declared in the header, bound in _lib.PROTOTYPES with the header's number of arguments, and exported by the built library"""
    from vae_tagger_amd import _lib
    text = open(os.path.join(ROOT, "include", "vae_tagger_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    lib = _lib.load()
    for name in NEW_ENTRIES:
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} is not declared in include/vae_tagger_hip.h"
        args = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
        assert name in _lib.PROTOTYPES, f"{name} is not in _lib.PROTOTYPES"
        assert len(_lib.PROTOTYPES[name][1]) == len(args), (name, len(_lib.PROTOTYPES[name][1]), len(args))
        assert hasattr(lib, name), f"{name} is not exported by the library"


def test_workspace_functions():
    from vae_tagger_amd import _lib
    lib = _lib.load()
    for fn in (lib.vt_op_attention_core_backward_workspace_bytes, lib.vt_op_attention_forward_train_workspace_bytes):
        for bad in ((0, 64, 512), (1, 0, 512), (-1, 64, 512), (1, -5, 512), (1, 64, 0), (1, 64, 256)):
            assert fn(*bad) == 0, bad
        sizes = [fn(1, S, 512) for S in (1, 99, 320, 561, 2112, 4096)]
        assert all(s > 0 for s in sizes) and sizes == sorted(set(sizes)), sizes
        assert fn(2, 561, 512) > fn(1, 561, 512)
    assert lib.vt_op_groupnorm_backward_workspace_bytes(0, 64, 512) == 0 and lib.vt_op_groupnorm_backward_workspace_bytes(2, 64, 512) > 0
    assert lib.vt_op_attention_vt_pitch(0) == 0
    for S in (1, 99, 1024, 4096):
        ld = lib.vt_op_attention_vt_pitch(S)
        assert ld >= (S + 7) // 8 * 8 and ld % 8 == 0


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_new_kernels_use_no_scratch_and_fit_one_workgroup_per_cu(tmp_path):
    """the kernels of attn_bwd.hip: no private segment, no spills; the two MFMA skeletons take their tiles as dynamic LDS (128 KB / 64 KB per workgroup of
    8 waves at two waves per SIMD, i.e. one workgroup per CU like the forward's kernels), so their static LDS is 0; the transpose's static tile is small"""
    out = tmp_path / "attn_bwd.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "-S", "--cuda-device-only", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), "-o", str(out), os.path.join(CSRC, "attn_bwd.hip")],
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
    skeleton = [k for k in kernels if "attn_bwd_qk_kernel" in k or "attn_bwd_pv_kernel" in k]
    assert len(skeleton) == 5, sorted(kernels)                    # three epilogue modes, two channel widths
    assert any("attn_bwd_rows_kernel" in k for k in kernels) and any("transpose16_kernel" in k for k in kernels)
    for k, b in kernels.items():
        assert int(b["private_segment_fixed_size"]) == 0, (k, b["private_segment_fixed_size"])
        assert int(b["vgpr_spill_count"]) == 0 and int(b["sgpr_spill_count"]) == 0, k
        if k in skeleton:
            assert int(b["group_segment_fixed_size"]) == 0, k     # dynamic only: 2 x 64 KB (Q.K^T skeleton) / 2 x 32 KB (P.V skeleton) <= 160 KB
            assert int(b["vgpr_count"]) <= 256, k                  # two waves per SIMD
        else:
            assert int(b["group_segment_fixed_size"]) <= 16 * 1024, k
