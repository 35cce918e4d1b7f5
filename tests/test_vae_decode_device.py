"""VAE decode on the device, end to end: AutoencoderKL.decode / DiffusersVAEWrapper.decode / .forward against the torch-CPU fp32
restatement of the decoder (tests/_vae_decode_ref.py), in both operand modes and both Upsample2D routes.

Bound (the form and factor of tests/test_cli.py's encoder check): max|d| <= max(1e-2, 1.5 d_emu), d_emu = the restatement's own error
with that mode's operand rounding; 1e-2 is the project's tensor tolerance."""
import ctypes

import pytest
import torch

from _vae_decode_ref import decode_image
from vae_tagger_amd import synth
from vae_tagger_amd._lib import VTError
from vae_tagger_amd._runtime import stream_ptr, vp
from vae_tagger_amd.autoencoder_kl import AutoencoderKL
from vae_tagger_amd.diffusers_vae_loader import DiffusersVAEWrapper

pytestmark = pytest.mark.gpu

VT_ERR_INVALID, VT_ERR_WORKSPACE = 1, 5
SCALING, SHIFT = 0.3611, 0.1159

CONFIGS = {"small": dict(block_out=(64, 128), layers=1), "flux": dict(block_out=(128, 256, 512, 512), layers=2)}
CASES = {"small_3x5x7": ("small", (3, 16, 5, 7)), "flux_2x16x16": ("flux", (2, 16, 16, 16)), "flux_1x9x13": ("flux", (1, 16, 9, 13))}


def _latents(shape, seed=0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def models():
    """one AutoencoderKL per configuration on cuda:0 with seeded synthetic decoder weights (and their CPU state dict)"""
    out = {}
    for name, cfg in CONFIGS.items():
        n = len(cfg["block_out"])
        sd = synth.synth_state_dict(synth.image_decoder_manifest(cfg["block_out"], 3, 16, cfg["layers"]), seed=3)
        vae = AutoencoderKL(block_out_channels=cfg["block_out"], down_block_types=("DownEncoderBlock2D",) * n, up_block_types=("UpDecoderBlock2D",) * n,
                            layers_per_block=cfg["layers"], latent_channels=16, use_quant_conv=False, use_post_quant_conv=False,
                            scaling_factor=SCALING, shift_factor=SHIFT)
        missing, unexpected = vae.load_decoder_state_dict(sd)
        assert not missing and not unexpected
        out[name] = (vae.to("cuda:0").eval(), sd, cfg)
    return out


@pytest.fixture(scope="module")
def references(models):
    """per case: the fp32 restatement and its operand-rounded forms, computed once"""
    out = {}
    for case, (cfg_name, shape) in CASES.items():
        _, sd, cfg = models[cfg_name]
        z = _latents(shape)
        kw = dict(n_blocks=len(cfg["block_out"]), layers_per_block=cfg["layers"])
        ref = decode_image(sd, z, **kw)
        out[case] = (z, ref, {m: (decode_image(sd, z, operands=m, **kw) - ref).abs().max().item() for m in ("bf16", "fp16")})
    return out


def _set_modes(vae, mode, literal):
    dec = vae.image_decoder()
    dec.set_fp16_operands(mode == "fp16")
    dec.set_literal_upsample(literal)


@pytest.mark.parametrize("literal", [False, True], ids=["folded", "literal"])
@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_decode_matches_the_fp32_restatement(models, references, case, mode, literal):
    vae = models[CASES[case][0]][0]
    z, ref, d_emu = references[case]
    _set_modes(vae, mode, literal)
    try:
        got = vae.decode(z.cuda()).sample
        again = vae.decode(z.cuda(), return_dict=False)[0]
        torch.cuda.synchronize()
        assert vae.status() == 0
    finally:
        _set_modes(vae, "bf16", False)
    assert got.shape == ref.shape and got.dtype == torch.float32
    assert torch.equal(got, again), "two runs differ"
    d_hip = (got.cpu() - ref).abs().max().item()
    print(f"{case} {mode} {'literal' if literal else 'folded'}: d_hip {d_hip:.3e}  d_emu {d_emu[mode]:.3e}  ratio {d_hip / d_emu[mode]:.2f}")
    assert d_hip <= max(1e-2, 1.5 * d_emu[mode])


def test_abi_checks_the_sizes_it_is_given(models):
    vae = models["small"][0]
    dec = vae.image_decoder()
    ctx = dec._context()
    z = _latents((1, 16, 5, 7)).cuda()
    out = torch.zeros(1, 3, 10, 14, device="cuda:0")
    need = ctx.lib.vt_decode_image_workspace_bytes(ctx.handle, 1, 5, 7)
    assert need > 0 and ctx.lib.vt_decode_image_workspace_bytes(ctx.handle, 0, 5, 7) == 0
    ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda:0")
    ptr = ctypes.c_void_p((ws.data_ptr() + 255) // 256 * 256)
    s = stream_ptr(z.device)
    call = ctx.lib.vt_decode_image
    assert call(ctx.handle, vp(z), 1, 5, 7, 0, vp(out), out.numel() * 4 - 4, ptr, need, s) == VT_ERR_INVALID
    assert call(ctx.handle, vp(z), 1, 5, 7, 0, vp(out), out.numel() * 4, ptr, need - 256, s) == VT_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert torch.count_nonzero(out) == 0                               # nothing was launched
    assert call(ctx.handle, vp(z), 1, 5, 7, 0, vp(out), out.numel() * 4, ptr, need, s) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, vae.decode(z).sample)


def test_wrapper_decode_unscales_then_decodes(models):
    vae = models["flux"][0]
    wrapper = DiffusersVAEWrapper(vae)
    z = _latents((2, 16, 16, 16), seed=5) * SCALING + SHIFT
    got = wrapper.decode(z.cuda())
    want = vae.decode(((z - SHIFT) / SCALING).cuda()).sample         # (IEEE fp32 on the host, as the staging pass computes it)
    assert torch.equal(got, want)


def test_wrapper_forward_reconstructs(models):
    vae = models["flux"][0]
    wrapper = DiffusersVAEWrapper(vae)
    x = synth.synth_images(2, 64, 64, seed=1).cuda()
    recon, posterior = wrapper(x)
    assert recon.shape == (2, 3, 64, 64) and recon.dtype == torch.float32 and bool(torch.isfinite(recon).all())
    want = vae.encode(x).latent_dist
    assert torch.equal(posterior.mean, want.mean) and torch.equal(posterior.logvar, want.logvar)
    assert vae.status() == 0


def test_post_quant_conv_is_refused_at_decode_time():
    vae = AutoencoderKL(block_out_channels=(64, 128), down_block_types=("DownEncoderBlock2D",) * 2, layers_per_block=1, use_quant_conv=False)
    assert vae.config.use_post_quant_conv is True                     # the constructor's default, accepted
    with pytest.raises(NotImplementedError, match="use_post_quant_conv"):
        vae.to("cuda:0").decode(torch.zeros(1, 16, 2, 2, device="cuda:0"))


def test_decode_without_a_device_is_an_error():
    vae = AutoencoderKL(block_out_channels=(64, 128), down_block_types=("DownEncoderBlock2D",) * 2, layers_per_block=1, use_quant_conv=False,
                        use_post_quant_conv=False)
    with pytest.raises(VTError, match="no CPU fallback"):
        vae.decode(torch.zeros(1, 16, 2, 2))
