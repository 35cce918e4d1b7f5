"""SHA-256 digests of what the VAE encoder's and image decoder's launch schedules compute, under every flag setting that selects another
kernel or operand type: what a change to the host layer that drives them (encoder.hip, image_decoder.hip, weights.hip) must leave bit
for bit (profiles/r16/README.md describes the items).

    cd <root of the tree to be measured> && python <this file> > digests.txt

The package is imported from the current directory, so the same file measures a checkout of another commit (built there) when it is
run from that checkout's root; two trees agree when their outputs are identical (`cmp`)."""
import contextlib
import ctypes
import hashlib
import io
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch
from vae_tagger_amd import synth
from vae_tagger_amd.autoencoder_kl import AutoencoderKL
from vae_tagger_amd.modules import create_attention_decoder
from vae_tagger_amd.pipeline import EncodeTagPipeline

CONFIGS = {"small": dict(block_out=(64, 128), layers=1), "flux": dict(block_out=(128, 256, 512, 512), layers=2)}
DEFAULTS = {0: 1, 2: 0, 4: 1, 8: 1, 11: 0, 13: 1, 16: 0, 18: 0, 19: 1, 20: 1, 22: 0}       # of every flag set below
ENCODER = {"flux": ([(2, 96, 160), (2, 72, 88)],
                    [{}, {11: 1}, {18: 1}, {2: 1}, {8: 0}, {0: 0}, {4: 0}, {13: 0}, {19: 0}, {20: 0}, {11: 1, 16: 5}]),
           "small": ([(2, 96, 80)], [{}, {11: 1}, {18: 1}, {8: 0}])}
DECODER = [("small", (3, 16, 5, 7)), ("flux", (2, 16, 16, 16)), ("flux", (1, 16, 9, 13))]
DECODER_FLAGS = [{}, {18: 1}, {22: 1}, {18: 1, 22: 1}, {8: 0}, {0: 0}, {4: 0}, {20: 0}]


def make_vae(cfg):
    """one AutoencoderKL on cuda:0 with seeded synthetic weights in both halves"""
    n = len(cfg["block_out"])
    vae = AutoencoderKL(block_out_channels=cfg["block_out"], down_block_types=("DownEncoderBlock2D",) * n, up_block_types=("UpDecoderBlock2D",) * n,
                        layers_per_block=cfg["layers"], latent_channels=16, use_quant_conv=False, use_post_quant_conv=False,
                        scaling_factor=0.3611, shift_factor=0.1159)
    vae.load_state_dict(synth.synth_state_dict(synth.encoder_manifest(cfg["block_out"], 3, 16, cfg["layers"]), seed=0), strict=False)
    vae.load_decoder_state_dict(synth.synth_state_dict(synth.image_decoder_manifest(cfg["block_out"], 3, 16, cfg["layers"]), seed=3))
    return vae.to("cuda:0").eval()


def dig(name, data):
    if isinstance(data, torch.Tensor):
        data = data.detach().cpu().contiguous().numpy()
    print(name, hashlib.sha256(np.ascontiguousarray(data).tobytes()).hexdigest(), flush=True)


def tag(flags):
    return "defaults" if not flags else "+".join(f"flag{f}={v}" for f, v in flags.items())


@contextlib.contextmanager
def flags_set(ctx, flags):
    try:
        for f, v in flags.items():
            ctx.call("vt_set_flag", f, v)
        yield
    finally:
        for f, v in DEFAULTS.items():
            ctx.call("vt_set_flag", f, v)


def traced(ctx, name, run):
    """the vt_debug_trace checksums (launch order) and the per-slot launch counts of one default-setting run"""
    ctx.call("vt_debug_trace", 1, None, 0, None)
    run()
    buf, n = (ctypes.c_ulonglong * 256)(), ctypes.c_int(0)
    ctx.call("vt_debug_trace", 0, buf, 256, ctypes.byref(n))
    dig(f"{name} gn-trace[{n.value}]", np.array(buf[: n.value], dtype=np.uint64))
    ctx.call("vt_profile_begin")
    run()
    k = ctx.lib.vt_profile_num_configs()
    launches, ms, fl = (ctypes.c_longlong * k)(), (ctypes.c_double * k)(), (ctypes.c_double * k)()
    ctx.call("vt_profile_end", k, launches, ms, fl, None)
    dig(f"{name} launch-counts[{sum(launches)}]", np.array(list(launches), dtype=np.int64))


vaes = {name: make_vae(cfg) for name, cfg in CONFIGS.items()}
for cfg, (shapes, settings) in ENCODER.items():
    vae = vaes[cfg]
    ctx = vae._context()
    for B, H, W in shapes:
        x = synth.synth_images(B, H, W, seed=H + 2 * W).cuda()
        for flags in settings:
            with flags_set(ctx, flags):
                dig(f"encode/{cfg} {B}x{H}x{W} {tag(flags)} moments", vae.encode(x).latent_dist.parameters)
                dig(f"encode/{cfg} {B}x{H}x{W} {tag(flags)} scaled", vae.encode_mode_scaled(x))
    B, H, W = shapes[0]
    x = synth.synth_images(B, H, W, seed=H + 2 * W).cuda()
    traced(ctx, f"encode/{cfg} {B}x{H}x{W}", lambda: vae.encode(x))
for cfg, shape in DECODER:
    vae = vaes[cfg]
    ctx = vae.image_decoder()._context()
    name = f"decode/{cfg} " + "x".join(str(v) for v in shape)
    z = torch.randn(shape, generator=torch.Generator().manual_seed(0)).cuda()
    for flags in DECODER_FLAGS:
        with flags_set(ctx, flags):
            dig(f"{name} {tag(flags)}", vae.decode(z).sample)
    dig(f"{name} unscale", vae.decode_unscaled(z * 0.3611 + 0.1159))
    traced(ctx, name, lambda: vae.decode(z))
for cfg, vae in vaes.items():
    print(f"status/{cfg}", vae.status(), flush=True)       # the sticky health word over everything above
# the tag path: vt_encode_tag reuses the encoder's workspace for the tag decoder
with contextlib.redirect_stdout(io.StringIO()):          # (the decoders' constructors print their configuration)
    dec = create_attention_decoder(16, 16, 16, 100, {"use_spatial_attention": True, "use_self_attention": True})
dec.load_state_dict(synth.synth_state_dict(synth.attention_decoder_manifest(100), seed=1), strict=False)
pipe = EncodeTagPipeline(vaes["flux"], dec.to("cuda:0").eval())
logits, lat = pipe.logits(synth.synth_images(2, 96, 160, seed=7).cuda(), return_latent=True)
dig("encode_tag/flux 2x96x160 logits", logits)
dig("encode_tag/flux 2x96x160 latent", lat)
