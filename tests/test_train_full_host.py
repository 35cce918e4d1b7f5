"""train_full on the host: the CLI's flags against the reference's names and defaults (a settings-only fixture), every refusal with the flag it
names, the two new entries of the C ABI (header, _lib.PROTOTYPES, the built library), the host mirror of the joint clip's 16 bytes, and the bytes
the encoder-only step keeps between its forward and its backward."""
import ctypes
import json
import os
import re
import struct

import numpy as np
import pytest

from vae_tagger_amd import _lib, synth, train_full, vae_backward

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(block_out=(64, 128, 512), layers_per_block=1)
REQUIRED = ["--json_path", "j", "--tags_csv_path", "t"]


def test_parser_has_every_flag_of_the_reference_with_its_default():
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "train_full_flags.json")))
    args = train_full.build_parser().parse_args(REQUIRED)
    assert len(want) == 48
    for name, default in want.items():
        assert hasattr(args, name), name
        assert getattr(args, name) == default and type(getattr(args, name)) is type(default), name
    with pytest.raises(SystemExit):
        train_full.build_parser().parse_args([])                                                 # --json_path and --tags_csv_path are required
    # this project's own flags, off by default
    assert (args.full_loss, args.resume_from, args.stop_after_epochs, args.workers, args.sharded) == (False, None, 0, 0, False)
    assert train_full.ignored_arguments(args) == []
    args = train_full.build_parser().parse_args(REQUIRED + ["--mixed_precision", "bf16", "--cudnn_benchmark", "--num_workers", "8", "--use_safetensors"])
    assert train_full.ignored_arguments(args) == ["mixed_precision", "cudnn_benchmark", "num_workers", "use_safetensors"]
    assert train_full.check_args(train_full.build_parser().parse_args(REQUIRED + ["--no_attention"])).use_attention is False


@pytest.mark.parametrize("flags, named", [
    (["--gradient_accumulation_steps", "2"], "--gradient_accumulation_steps"),
    (["--use_adaptive_weights"], "--use_adaptive_weights"),
    (["--use_quant_conv"], "--use_quant_conv"),
    (["--use_post_quant_conv"], "--use_post_quant_conv"),
    (["--sharded"], "--sharded"),
    (["--triplet_weight", "0"], "--triplet_weight"),
    (["--attention_heads", "3"], "--attention_heads"),
    (["--lr_scheduler_type", "polynomial"], "--lr_scheduler_type"),
])
def test_every_refusal_names_its_flag(flags, named):
    args = train_full.build_parser().parse_args(REQUIRED + flags)
    with pytest.raises(RuntimeError, match=re.escape(named)):
        train_full.check_args(args)
    with pytest.raises(SystemExit, match=re.escape(named)):                                       # main refuses before any device work
        train_full.main(REQUIRED + flags)


def test_what_is_not_refused():
    for flags in ([], ["--full_loss"], ["--full_loss", "--triplet_weight", "0"], ["--use_cross_attention"], ["--no_attention", "--attention_heads", "3"],
                  ["--use_focal_loss"], ["--gradient_accumulation_steps", "1"]):
        train_full.check_args(train_full.build_parser().parse_args(REQUIRED + flags))


def _header_argument_count(header, name):
    m = re.search(r"\b" + name + r"\s*\(", header)
    assert m, f"{name} is not declared in the header"
    depth, i = 1, m.end()
    while depth:
        depth += {"(": 1, ")": -1}.get(header[i], 0)
        i += 1
    body = re.sub(r"/\*.*?\*/", "", header[m.end():i - 1], flags=re.S)
    return len([a for a in body.split(",") if a.strip()])


def test_the_two_new_entries_in_header_prototypes_and_library():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "vae_tagger_hip.h")).read()
    for name, count in (("vt_full_optim_norm", 16), ("vt_posterior_mode_latent", 11)):
        res, args = _lib.PROTOTYPES[name]
        declared = [m.start() for m in re.finditer(r"\bint " + name + r"\(", header)]          # (the comment above names the entry without a type)
        assert len(declared) == 1, name
        assert _header_argument_count(header[declared[0]:], name) == len(args) == count, name
        fn = getattr(lib, name)
        assert fn.restype == res == ctypes.c_int and list(fn.argtypes) == list(args), name
    # vt_full_optim_norm takes vt_vae_optim_norm's arguments, then three (state, bytes) pairs before the stream
    norm, full = _lib.PROTOTYPES["vt_vae_optim_norm"][1], _lib.PROTOTYPES["vt_full_optim_norm"][1]
    assert list(full[:len(norm) - 1]) == list(norm[:-1]) and list(full[len(norm) - 1:]) == [ctypes.c_void_p, ctypes.c_size_t] * 3 + [ctypes.c_void_p]
    one = (ctypes.c_longlong * 1)(4)
    assert lib.vt_full_optim_norm(None, None, one, 1, 1.0, None, None, 0, 0, None, 0, None, 0, None, 0, None) == 1          # no context
    assert lib.vt_posterior_mode_latent(None, None, 1, 1, 1, 1.0, 0, 0.0, 0, None, None) == 1


def _unpack(raw):
    assert len(raw) == 16
    return struct.unpack("<dff", raw)


def test_joint_clip_host_reproduces_the_16_bytes():
    f32 = np.float32
    # clipping: every operation of the coefficient is an fp32 one, the 1e-6 included
    sq, norm, coef = _unpack(train_full.joint_clip_host(9.0, 16.0, 1.0))
    assert (sq, norm) == (25.0, 5.0) and f32(coef) == f32(1.0) / (f32(5.0) + f32(1e-6)) and coef < 0.2
    # the sum is ONE fp64 add, the VAE first: a block term below half an ulp of the VAE's leaves it unchanged
    sq, _, _ = _unpack(train_full.joint_clip_host(1.0, 2.0 ** -54, 1.0))
    assert sq == 1.0
    sq, _, _ = _unpack(train_full.joint_clip_host(1.0, 2.0 ** -52, 1.0))
    assert sq == 1.0 + 2.0 ** -52
    # the norm is rounded to fp32 BEFORE the division
    sq, norm, coef = _unpack(train_full.joint_clip_host(2.0, 0.0, 1.0))
    assert f32(norm) == f32(np.sqrt(2.0)) and f32(coef) == f32(1.0) / (f32(np.sqrt(2.0)) + f32(1e-6))
    # coef >= 1 -> exactly 1: inside the bound, at norm 0, and just below the bound where max_norm / (norm + 1e-6f) rounds to 1
    for sq_v, sq_b, bound in ((0.25, 0.0, 1.0), (0.0, 0.0, 1.0), (3.0, 1.0, 2.5), (1e-30, 0.0, 1e30)):
        assert _unpack(train_full.joint_clip_host(sq_v, sq_b, bound))[2] == 1.0
    one_ulp_below = float(np.nextafter(f32(1.0), f32(0.0)))
    sq, norm, coef = _unpack(train_full.joint_clip_host(1.0, 0.0, one_ulp_below))
    assert coef < 1.0 and f32(coef) == f32(one_ulp_below) / (f32(1.0) + f32(1e-6))
    # a NaN norm compares false with 1: the coefficient is 1, as on the device
    assert _unpack(train_full.joint_clip_host(float("nan"), 0.0, 1.0))[2] == 1.0
    # the packing: fp64 at byte 0, fp32 at 8 and 12 (TrainScalars)
    raw = train_full.joint_clip_host(9.0, 16.0, 1.0)
    assert np.frombuffer(raw[:8], np.float64)[0] == 25.0 and np.frombuffer(raw[8:], np.float32)[0] == 5.0


@pytest.mark.parametrize("cfg, B, H, W", [(SMALL, 2, 16, 24), ({}, 1, 64, 64), (SMALL, 3, 32, 32)])
def test_saved_bytes_of_the_encoder_only_step(cfg, B, H, W):
    shapes = {**synth.encoder_manifest(**cfg), **synth.image_decoder_manifest(**cfg)}
    enc = {k: v for k, v in shapes.items() if k.startswith("encoder.")}
    levels = len(cfg.get("block_out", synth.FLUX_BLOCK_OUT)) - 1
    moments = 3 * B * 2 * 16 * (H >> levels) * (W >> levels) * 4
    want = vae_backward.encoder_saved_bytes(enc, 3 * B, H, W) + moments
    assert vae_backward.vae_triplet_saved_bytes(shapes, B, H, W) == want == vae_backward.vae_triplet_saved_bytes(cfg, B, H, W)
    # what the full step keeps on top: the image decoder's `saved`, the decoded latent and the reconstruction
    full = vae_backward.vae_train_saved_bytes(shapes, B, H, W)
    dec = vae_backward.decoder_saved_bytes({k: v for k, v in shapes.items() if k.startswith("decoder.")}, B, H >> levels, W >> levels)
    assert full - want == dec + (B * 16 * (H >> levels) * (W >> levels) + B * 3 * H * W) * 4 > 0
