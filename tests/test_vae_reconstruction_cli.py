"""python -m vae_tagger_amd.vae_reconstruction_test on the device: the four files, the latent's shape, and the printed MSE against the
MSE recomputed from what the run saved (original.png -> input tensor, latent_vector.pt -> decode)."""
import os
import re
import subprocess
import sys

import pytest
import torch
from PIL import Image

from vae_tagger_amd import synth
from vae_tagger_amd.diffusers_vae_loader import get_diffusers_vae_config, load_diffusers_vae_from_config
from vae_tagger_amd.vae_reconstruction_test import preprocess_image

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ("original.png", "reconstructed.png", "vae_reconstruction_comparison.png", "latent_vector.pt")


def _run(ckpt, out_dir, *extra):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "vae_tagger_amd.vae_reconstruction_test", "--vae_checkpoint", str(ckpt), "--output_dir", str(out_dir),
                        "--resolution", "64", *extra], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


def test_reconstruction_cli(tmp_path):
    from safetensors.torch import save_file
    sd = synth.synth_state_dict(synth.encoder_manifest(), seed=0)
    sd.update(synth.synth_state_dict(synth.image_decoder_manifest(), seed=3))
    ckpt = tmp_path / "vae.safetensors"
    save_file({k: v.contiguous() for k, v in sd.items()}, str(ckpt))
    out = _run(ckpt, tmp_path / "a")
    for f in FILES:
        assert (tmp_path / "a" / f).exists(), f
    latent = torch.load(tmp_path / "a" / "latent_vector.pt", weights_only=True)
    assert tuple(latent.shape) == (1, 16, 8, 8) and latent.dtype == torch.float32
    for line in ("使用生成的测试图像", "输入图像形状: torch.Size([1, 3, 64, 64])", "潜在向量形状: torch.Size([1, 16, 8, 8])",
                 "重建图像形状: torch.Size([1, 3, 64, 64])", "压缩比: 12.00:1", "VAE 重建测试完成！"):
        assert line in out, line
    mse = float(re.search(r"重建误差 \(MSE\): ([0-9.]+)", out).group(1))
    assert re.search(r"PSNR: -?[0-9.]+ dB", out)
    # recomputed from the saved files: the same model, the same operand mode (fp16 by default), decode is bit-identical from run to run
    vae = load_diffusers_vae_from_config(get_diffusers_vae_config(), str(ckpt)).to("cuda:0").eval()
    vae.set_fp16_operands(True)
    x = preprocess_image(Image.open(tmp_path / "a" / "original.png").convert("RGB"), 64).cuda()
    want = torch.nn.functional.mse_loss(x, vae.decode(latent.cuda()).sample).item()
    assert vae.status() == 0
    assert abs(mse - want) <= 5e-7 + 1e-5 * want, (mse, want)             # the printed value has six decimals
    assert Image.open(tmp_path / "a" / "reconstructed.png").size == (64, 64)
    out_b = _run(ckpt, tmp_path / "b", "--bf16_operands")
    mse_b = float(re.search(r"重建误差 \(MSE\): ([0-9.]+)", out_b).group(1))
    lat_b = torch.load(tmp_path / "b" / "latent_vector.pt", weights_only=True)
    assert mse_b != mse or not torch.equal(lat_b, latent)
