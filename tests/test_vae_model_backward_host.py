"""Host-side checks of the end convs and the whole-model backward: the thin-side formulas and the transpose_rotate identity
against fp64 autograd, the hi + lo split, the structure parsing, the saved-bytes formulas against a hand count, the functional models the device tests
lean on, and the ABI surface of the new entries."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

from _vae_model_backward_ref import (bf16_round_keep, decoder_backward_ref, decoder_forward_ref, encoder_backward_ref, encoder_forward_ref, model_autograd, rel,
                                     rotate_transpose, split_hilo, thin_wgrad_ref)
from vae_tagger_amd import synth, vae_backward as vb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["vt_op_conv_thin_backward_weight_workspace_bytes", "vt_op_conv_thin_backward_weight", "vt_op_conv_thin_forward_workspace_bytes",
               "vt_op_conv_thin_forward"]
SMALL = dict(block_out=(64, 128, 512), layers_per_block=1)
TOL = 1e-12


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("B,C,H,W", [(2, 8, 5, 7), (1, 8, 1, 1)])
def test_thin_formulas(B, C, H, W):
    """both tap-offset formulas and the transpose_rotate identity against fp64 autograd; at 1 x 1 all eight outer taps are zero"""
    # conv_in: thin is the conv's input, wide its output gradient
    x, w, dy = _rand((B, 3, H, W), 1), _rand((C, 3, 3, 3), 2).requires_grad_(True), _rand((B, C, H, W), 3)
    want, = torch.autograd.grad(F.conv2d(x, w, padding=1), [w], dy)
    got = thin_wgrad_ref(x, dy, True)
    print(f"conv_in dW: max|d| = {(got - want).abs().max():.3e}")
    assert got.shape == want.shape and (got - want).abs().max() <= TOL
    # conv_out: thin is the output gradient, wide the conv's input
    a, w = _rand((B, C, H, W), 4).requires_grad_(True), _rand((3, C, 3, 3), 5).requires_grad_(True)
    dy = _rand((B, 3, H, W), 6)
    want_a, want_w = torch.autograd.grad(F.conv2d(a, w, padding=1), [a, w], dy)
    got_w = thin_wgrad_ref(dy, a.detach(), False)
    got_a = F.conv2d(dy, rotate_transpose(w.detach()), padding=1)
    print(f"conv_out dW: max|d| = {(got_w - want_w).abs().max():.3e}  dx: {(got_a - want_a).abs().max():.3e}")
    assert got_w.shape == want_w.shape and (got_w - want_w).abs().max() <= TOL
    assert got_a.shape == want_a.shape and (got_a - want_a).abs().max() <= TOL
    if H == 1 and W == 1:
        outer = torch.ones(3, 3, dtype=torch.bool)
        outer[1, 1] = False
        assert not got[:, :, outer].any() and not got_w[:, :, outer].any()


def test_split_is_exact_for_16_bits():
    """hi + lo carries 16 significant bits: exact for k 2^-15, |k| < 2^16; on random normals the residual is below 2^-17 relative"""
    gen = torch.Generator().manual_seed(7)
    k = torch.randint(-(2 ** 16) + 1, 2 ** 16, (100000,), generator=gen)
    for dtype in (torch.float32, torch.float64):
        v = k.to(dtype) * 2.0 ** -15
        assert torch.equal(split_hilo(v), v)
        assert not torch.equal(bf16_round_keep(v), v)              # one bf16 does not carry them
    v = torch.randn(100000, generator=gen, dtype=torch.float64)
    res = ((split_hilo(v) - v).abs() / v.abs()).max().item()
    print(f"split residual on normals: {res:.3e}")
    assert res <= 2.0 ** -17


@pytest.mark.parametrize("cfg", [{}, SMALL], ids=["flux", "small"])
def test_structure_from_key_names(cfg):
    block_out = cfg.get("block_out", synth.FLUX_BLOCK_OUT)
    n = cfg.get("layers_per_block", synth.FLUX_LAYERS_PER_BLOCK)
    enc = vb.model_structure(synth.encoder_manifest(**cfg), "encoder.")
    assert [b["resample"] for b in enc["blocks"]] == [True] * (len(block_out) - 1) + [False]
    cin = block_out[0]
    for b, co in zip(enc["blocks"], block_out):
        assert b["resnets"] == [(cin, co)] + [(co, co)] * (n - 1)
        cin = co
    assert enc["mid"] == block_out[-1] and enc["conv_in"] == (block_out[0], 3) and enc["conv_out"] == (32, block_out[-1])
    dec = vb.model_structure(synth.image_decoder_manifest(**cfg), "decoder.")
    rev = block_out[::-1]
    assert [b["resample"] for b in dec["blocks"]] == [True] * (len(rev) - 1) + [False]
    cin = rev[0]
    for b, co in zip(dec["blocks"], rev):
        assert b["resnets"] == [(cin, co)] + [(co, co)] * n
        cin = co
    assert dec["mid"] == rev[0] and dec["conv_in"] == (rev[0], 16) and dec["conv_out"] == (3, rev[-1])


def test_flux_tensor_counts():
    assert len(synth.encoder_manifest()) == 106 and len(synth.image_decoder_manifest()) == 138


@pytest.mark.parametrize("key", ["encoder.quant_conv.weight", "decoder.conv_in.weight", "encoder.down_blocks.0.attentions.0.to_q.weight",
                                 "encoder.mid_block.resnets.2.conv1.weight", "encoder.conv_in.scale", "conv_in.weight"])
def test_foreign_keys_are_refused(key):
    m = dict(synth.encoder_manifest(**SMALL))
    m[key] = (1,)
    with pytest.raises(ValueError):
        vb.model_structure(m, "encoder.")
    with pytest.raises(ValueError):
        vb.encoder_saved_bytes(m, 1, 8, 8)


def test_missing_end_is_refused():
    m = dict(synth.image_decoder_manifest(**SMALL))
    del m["decoder.conv_out.bias"]
    with pytest.raises(ValueError):
        vb.model_structure(m, "decoder.")


def test_saved_bytes_hand_count():
    """block_out = (64, 512), one layer per block, batch 1.  Encoder at 4 x 4: the image 192; resnet 64 -> 64 at 16 pixels 4096 + 4096 + 2048 + 2048 + 512
    = 12800; the downsampler's operand 2048; resnet 64 -> 512 at 4 pixels 1024 + 8192 + 512 + 4096 + 512 + 512 (x16) = 14848; the mid block at 2 x 2:
    two resnets of 25088 and the attention 40960 + 16 + 64 + 256 = 41296 (v^T at pitch 8: 8192); conv_norm_out 8192 + 4096 + 256 = 12544."""
    cfg = dict(block_out=(64, 512), layers_per_block=1)
    assert vb.attention_vt_pitch(4) == 8 and vb.attention_vt_pitch(1024) == 1024 + 2048 + 64 and vb.attention_vt_pitch(1021) == 1024 + 2048 + 64
    assert vb.encoder_saved_bytes(cfg, 1, 4, 4) == 192 + 12800 + 2048 + 14848 + 2 * 25088 + 41296 + 12544
    # decoder from 2 x 2 latents: z16 512; the mid block 91472; up block 0: two resnets 512 -> 512 of 25088, the upsampler's operand 4096; up block 1 at
    # 4 x 4: resnet 512 -> 64 32768 + 4096 + 16384 + 2048 + 512 + 16384 = 72192, resnet 64 -> 64 12800; conv_norm_out 4096 + 2048 + 256 = 6400
    assert vb.decoder_saved_bytes(cfg, 1, 2, 2) == 512 + 91472 + 2 * 25088 + 4096 + 72192 + 12800 + 6400
    # the parameters themselves (shapes) give the same numbers as the configuration
    assert vb.encoder_saved_bytes(synth.encoder_manifest(**cfg), 1, 4, 4) == vb.encoder_saved_bytes(cfg, 1, 4, 4)
    assert vb.decoder_saved_bytes(synth.image_decoder_manifest(**cfg), 3, 5, 7) == vb.decoder_saved_bytes(cfg, 3, 5, 7)
    # odd sizes: the stride-2 conv floors
    assert vb.encoder_saved_bytes(cfg, 1, 5, 5) - vb.encoder_saved_bytes(cfg, 1, 4, 4) == 9 * (3 * 4 + 64 * 12 + 64 * 2)


@pytest.mark.parametrize("kind", ["encoder", "decoder"])
def test_functional_model_restatement(kind):
    """the backward restatement with no rounding is the exact gradient: against fp64 autograd of the functional model"""
    cfg = dict(block_out=(64, 512), layers_per_block=1)
    man = (synth.encoder_manifest if kind == "encoder" else synth.image_decoder_manifest)(**cfg)
    p = {k: v.double() for k, v in synth.synth_state_dict(man, seed=3).items()}
    x = _rand((1, 3, 6, 5), 11) if kind == "encoder" else _rand((1, 16, 2, 3), 12)
    fwd = encoder_forward_ref if kind == "encoder" else decoder_forward_ref
    y, saved = fwd(p, x)
    dy = _rand(tuple(y.shape), 13)
    y2, dx, want = model_autograd(kind, p, x, dy)
    assert torch.equal(y, y2)
    if kind == "encoder":
        got, _ = encoder_backward_ref(p, saved, dy)
    else:
        dz, got, _ = decoder_backward_ref(p, saved, dy)
        assert (dz - dx).abs().max() <= 1e-10 * dx.abs().max()
    assert list(got) == list(p)
    for k in p:
        assert rel(got[k], want, k) <= 1e-10, (k, rel(got[k], want, k))


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
    """sized by the slices actually used: clamped to the tile count, 0 for shapes the operator refuses"""
    lib = vb._lib.load()
    f = lib.vt_op_conv_thin_backward_weight_workspace_bytes
    assert f(1, 1, 1, 64, 0) == f(1, 1, 1, 64, 1) == f(1, 1, 1, 64, 9) > 0
    assert f(2, 10, 14, 128, 3) > f(2, 10, 14, 128, 2) > f(2, 10, 14, 128, 1) >= 32 * 128 * 4
    assert f(1, 5, 7, 96, 0) == 0 and f(1, 5, 7, 576, 0) == 0 and f(0, 5, 7, 64, 0) == 0 and f(1, 5, 7, 64, -1) == 0
    g = lib.vt_op_conv_thin_forward_workspace_bytes
    assert g(128) >= 2 * 128 * 32 * 2 + 128 * 4 and g(64) >= 27 * 64 * 4 + 64 * 4 and g(12) == 0
