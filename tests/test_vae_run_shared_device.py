"""The run layer that the VAE encoder's and the image decoder's schedules share (VaeRun, csrc/vae_run.hip): what sharing it must not change.

  - decode has no fp8 form.  The shared resnet / attention steps have fp8 branches, so vt_decode_image switches the mode off for its own
    run: the image must not depend on vt_set_flag 11, and the encoder must find the mode as it left it.
  - the workspace sizes are part of the ABI's observable behaviour (DESIGN.md 4.17 documents 5.74 GiB per 1024^2 image): they are pinned to
    tests/golden/vae_workspace_bytes.json, recorded from the commit before the layer was shared with workspace_sizes() below."""
import ctypes
import json
import os

import pytest
import torch

from _util import GOLDEN
from vae_tagger_amd import _lib, synth
from vae_tagger_amd.autoencoder_kl import AutoencoderKL

pytestmark = pytest.mark.gpu

CONFIGS = {"small": dict(block_out=(64, 128), layers=1), "flux": dict(block_out=(128, 256, 512, 512), layers=2)}
IMAGE_SHAPES = [(64, 64), (72, 88), (96, 160), (100, 76), (512, 512), (1024, 1024)]
LATENT_SHAPES = [(1, 1), (5, 7), (9, 13), (16, 16), (128, 128)]


def _vae(cfg):
    """an AutoencoderKL on cuda:0 with seeded synthetic weights in both halves"""
    n = len(cfg["block_out"])
    vae = AutoencoderKL(block_out_channels=cfg["block_out"], down_block_types=("DownEncoderBlock2D",) * n, up_block_types=("UpDecoderBlock2D",) * n,
                        layers_per_block=cfg["layers"], latent_channels=16, use_quant_conv=False, use_post_quant_conv=False,
                        scaling_factor=0.3611, shift_factor=0.1159)
    vae.load_state_dict(synth.synth_state_dict(synth.encoder_manifest(cfg["block_out"], 3, 16, cfg["layers"]), seed=0), strict=False)
    missing, unexpected = vae.load_decoder_state_dict(synth.synth_state_dict(synth.image_decoder_manifest(cfg["block_out"], 3, 16, cfg["layers"]), seed=3))
    assert not missing and not unexpected
    return vae.to("cuda:0").eval()


def _latents(shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(0)).cuda()


def test_decode_ignores_and_preserves_fp8_mode():
    vae = _vae(CONFIGS["small"])
    ctx = vae._context()
    x, z = synth.synth_images(2, 96, 80).cuda(), _latents((3, 16, 5, 7))
    try:
        image_off = vae.decode(z).sample
        latent_off = vae.encode(x).latent_dist.parameters
        assert vae.status() == 0
        ctx.call("vt_set_flag", 11, 1)
        image_on = vae.decode(z).sample
        assert vae.status() == 0
        before = vae.encode(x).latent_dist.parameters
        assert vae.status() == 0
        vae.decode(z)
        after = vae.encode(x).latent_dist.parameters
        assert vae.status() == 0
    finally:
        ctx.call("vt_set_flag", 11, 0)
    assert torch.equal(image_on, image_off), "decode depends on the fp8 flag"
    assert torch.equal(before, after), "decode changed the encoder's fp8 mode"
    assert not torch.equal(before, latent_off), "the fp8 flag did not reach the encoder"

    flux = _vae(CONFIGS["flux"])
    ctx = flux._context()
    z = _latents((1, 16, 9, 13))
    try:
        image_off = flux.decode(z).sample
        ctx.call("vt_set_flag", 11, 1)
        image_on = flux.decode(z).sample
        assert flux.status() == 0
    finally:
        ctx.call("vt_set_flag", 11, 0)
    assert torch.equal(image_on, image_off), "decode depends on the fp8 flag (FLUX configuration)"


def workspace_sizes():
    """{configuration: {entry: {"BxHxW": bytes}}}: size computations on configured (weightless) contexts; nothing of that size is allocated"""
    out = {}
    for name, cfg in CONFIGS.items():
        ctx = _lib.Context(0)
        blocks = (ctypes.c_int * len(cfg["block_out"]))(*cfg["block_out"])
        ctx.call("vt_encoder_configure", 3, 16, blocks, len(blocks), cfg["layers"], 32, 0.3611, 1, 0.1159, 1)
        ctx.call("vt_image_decoder_configure", 3, 16, blocks, len(blocks), cfg["layers"], 32, 0.3611, 1, 0.1159, 1)
        ctx.call("vt_decoder_configure", 100, 16, 0, 1, 1, 0, 8)          # the tag decoder: attention, spatial + self
        lib, h = ctx.lib, ctx.handle
        out[name] = {
            "vt_encode_workspace_bytes": {f"{B}x{H}x{W}": lib.vt_encode_workspace_bytes(h, B, H, W) for B in (1, 3) for H, W in IMAGE_SHAPES},
            "vt_encode_tag_workspace_bytes": {f"{B}x{H}x{W}": lib.vt_encode_tag_workspace_bytes(h, B, H, W) for B in (1, 3) for H, W in IMAGE_SHAPES},
            "vt_decode_image_workspace_bytes": {f"{B}x{H}x{W}": lib.vt_decode_image_workspace_bytes(h, B, H, W) for B in (1, 3) for H, W in LATENT_SHAPES},
        }
        ctx.close()
    return out


def test_workspace_sizes_are_the_recorded_ones():
    with open(os.path.join(GOLDEN, "vae_workspace_bytes.json")) as f:
        want = json.load(f)
    got = workspace_sizes()
    assert all(v > 0 for cfg in got.values() for entry in cfg.values() for v in entry.values())
    assert got == want
