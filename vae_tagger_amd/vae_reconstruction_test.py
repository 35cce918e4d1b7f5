"""Counterpart of the reference's vae_reconstruction_test.py: is a loaded VAE checkpoint sane?  encode -> sample -> decode -> MSE / PSNR.

Same arguments (--vae_checkpoint --vae_config_path --image_path --output_dir --resolution --show_result), same files
(original.png, reconstructed.png, vae_reconstruction_comparison.png, latent_vector.pt), same printed lines.  Differences:
  * torchvision is not required: Resize + ToTensor + Normalize and ToPILImage are restated with PIL and torch;
  * matplotlib is imported lazily; without it the comparison figure is a three-panel PIL composite;
  * the reference runs in fp32; here the convolutions multiply fp16 operands by default (--bf16_operands opts out), see --help;
  * the device health word is checked after encode and after decode, with infer_full's fall-back order (bf16 operands and fp32
    residual-stream storage, then an error).
"""
import argparse
import os

import numpy as np
import torch
from PIL import Image

from .diffusers_vae_loader import (DiffusersVAEWrapper, create_vae_from_config_file, get_diffusers_vae_config,
                                   load_diffusers_vae_from_config)

OPERAND_NOTE = ("卷积操作数精度: 默认fp16 (11位有效数字)。CPU上对fp32参考的实测重建误差 (FLUX配置, 合成权重, 2x16x16x16潜变量, 输出|max| 1.9): "
                "fp16操作数 max|d| 4.0e-3, bf16操作数 2.7e-2 -- 因此默认fp16; --bf16_operands 改回bf16")


def load_vae_model(args, device="cuda"):
    if args.vae_config_path and os.path.exists(args.vae_config_path):
        print(f"从配置文件创建VAE: {args.vae_config_path}")
        model = create_vae_from_config_file(args.vae_config_path, args.vae_checkpoint)
    elif args.vae_checkpoint and os.path.exists(args.vae_checkpoint):
        print(f"直接加载预训练VAE模型: {args.vae_checkpoint}")
        model = DiffusersVAEWrapper(load_diffusers_vae_from_config(get_diffusers_vae_config(), args.vae_checkpoint))
    else:
        print("使用默认配置创建新的VAE模型")
        cfg = get_diffusers_vae_config()
        cfg["sample_size"] = args.resolution
        model = DiffusersVAEWrapper(load_diffusers_vae_from_config(cfg))
    model.to(device)
    model.eval()
    return model


def create_test_image(size=(512, 512)):
    """The reference's generated picture: red ramps left to right, green ramps top to bottom (255 -> 0), blue 128, a white disc of radius
    min/6 and a red square of half-side min/8 in the centre."""
    width, height = size
    img = np.empty((height, width, 3), dtype=np.uint8)
    img[:, :, 0] = np.linspace(0, 255, width).astype(np.uint8)[None, :]
    img[:, :, 1] = np.linspace(255, 0, height).astype(np.uint8)[:, None]
    img[:, :, 2] = 128
    cx, cy = width // 2, height // 2
    yy, xx = np.ogrid[:height, :width]
    img[(xx - cx) ** 2 + (yy - cy) ** 2 <= (min(width, height) // 6) ** 2] = (255, 255, 255)
    half = min(width, height) // 8
    img[cy - half:cy + half, cx - half:cx + half] = (255, 0, 0)
    return Image.fromarray(img)


def load_image(image_path, target_size=(512, 512)):
    if image_path and os.path.exists(image_path):
        image = Image.open(image_path).convert("RGB")
        print(f"加载图像: {image_path}")
    else:
        image = create_test_image(target_size)
        print("使用生成的测试图像")
    return image.resize(target_size, Image.Resampling.LANCZOS)


def preprocess_image(image, resolution=512):
    """Resize((r, r)) (bilinear on a PIL image) + ToTensor + Normalize(0.5, 0.5) -> [1, 3, r, r] in [-1, 1]"""
    if image.size != (resolution, resolution):
        image = image.resize((resolution, resolution), Image.BILINEAR)
    t = torch.from_numpy(np.asarray(image.convert("RGB"), dtype=np.uint8).copy()).permute(2, 0, 1).to(torch.float32).div(255.0)
    return ((t - 0.5) / 0.5).unsqueeze(0)


def postprocess_image(tensor):
    """[-1, 1] -> PIL (ToPILImage of a float tensor: mul(255).byte())"""
    t = torch.clamp(tensor * 0.5 + 0.5, 0, 1).squeeze(0).cpu()
    return Image.fromarray(t.mul(255).byte().permute(1, 2, 0).contiguous().numpy())


def _comparison_figure(original, reconstructed, diff_image, mse_loss, path, show):
    try:
        import matplotlib
        if not show:
            matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        # three panels side by side: original | reconstruction | normalised absolute difference
        w, h = original.size
        sheet = Image.new("RGB", (3 * w, h))
        sheet.paste(original, (0, 0))
        sheet.paste(reconstructed, (w, 0))
        sheet.paste(Image.fromarray((np.clip(diff_image, 0, 1) * 255).astype(np.uint8)), (2 * w, 0))
        sheet.save(path)
        return None
    fig, axes = plt.subplots(1, 3, figsize=(15, 5))
    for ax, im, title in zip(axes, (original, reconstructed, diff_image),
                             ("Original Image", f"VAE restruction\nMSE Loss: {mse_loss:.6f}", "difference (abs)")):
        ax.imshow(im)
        ax.set_title(title, fontsize=14)
        ax.axis("off")
    plt.tight_layout()
    plt.savefig(path, dpi=300, bbox_inches="tight")
    return plt


def _encode_sample_decode(vae, x):
    """-> (latent, reconstruction, status word) of one pass; the word is read once, after decode (it is sticky)"""
    posterior = vae.encode(x).latent_dist
    st = vae.status()
    latent = posterior.sample()
    recon = vae.decode(latent).sample
    return latent, recon, st | vae.status()


def reconstruct(vae_model, input_tensor, f16=True):
    """encode -> sample -> decode on the device with the health word's fall-backs: a raised word is retried once on the most conservative
    setting (bf16 operands, fp32 residual-stream storage), which is kept if it cures it; otherwise it is the input or the checkpoint."""
    vae = vae_model.vae
    vae.set_fp16_operands(f16)
    print("开始 VAE 编码...")
    latent, recon, st = _encode_sample_decode(vae, input_tensor)
    if st:
        vae.set_fp16_operands(False)
        vae.set_fp32_residual(True)
        latent, recon, st2 = _encode_sample_decode(vae, input_tensor)
        if st2:
            raise FloatingPointError("non-finite activations even with bf16 operands and fp32 residual storage (inf / NaN pixels or weights?)")
        print("警告: 激活值超出fp16范围，改用fp32残差存储" + ("和bf16卷积操作数" if f16 else "") + "重新计算")
    print(f"潜在向量形状: {latent.shape}")
    print(f"潜在向量统计: mean={latent.mean().item():.4f}, std={latent.std().item():.4f}")
    print("开始 VAE 解码...")
    print(f"重建图像形状: {recon.shape}")
    return latent, recon


def test_vae_reconstruction(args):
    device = "cuda" if torch.cuda.is_available() else "cpu"
    print(f"使用设备: {device}")
    vae_model = load_vae_model(args, device)
    print("VAE 模型加载完成")
    original_image = load_image(args.image_path, (args.resolution, args.resolution))
    input_tensor = preprocess_image(original_image, args.resolution).to(device)
    print(f"输入图像形状: {input_tensor.shape}")
    with torch.no_grad():
        latent, reconstructed_tensor = reconstruct(vae_model, input_tensor, f16=not args.bf16_operands)
    reconstructed_image = postprocess_image(reconstructed_tensor)
    mse_loss = torch.nn.functional.mse_loss(input_tensor, reconstructed_tensor).item()
    print(f"重建 MSE 损失: {mse_loss:.6f}")
    diff = np.abs(np.array(original_image).astype(float) - np.array(reconstructed_image).astype(float))
    diff_image = diff / diff.max() if diff.max() > 0 else diff
    os.makedirs(args.output_dir, exist_ok=True)
    comparison_path = os.path.join(args.output_dir, "vae_reconstruction_comparison.png")
    plt = _comparison_figure(original_image, reconstructed_image, diff_image, mse_loss, comparison_path, args.show_result)
    print(f"对比图已保存到: {comparison_path}")
    original_image.save(os.path.join(args.output_dir, "original.png"))
    reconstructed_image.save(os.path.join(args.output_dir, "reconstructed.png"))
    latent_path = os.path.join(args.output_dir, "latent_vector.pt")
    torch.save(latent.cpu(), latent_path)
    print(f"潜在向量已保存到: {latent_path}")
    if args.show_result and plt is not None:
        plt.show()
    print("VAE 重建测试完成！")
    print(f"输入分辨率: {args.resolution}x{args.resolution}")
    print(f"潜在空间维度: {latent.shape}")
    print(f"压缩比: {(input_tensor.numel() / latent.numel()):.2f}:1")
    print(f"重建误差 (MSE): {mse_loss:.6f}")
    psnr = 20 * torch.log10(torch.tensor(2.0)) - 10 * torch.log10(torch.tensor(mse_loss))
    print(f"PSNR: {psnr.item():.2f} dB")
    return mse_loss


def build_parser():
    parser = argparse.ArgumentParser(description="VAE 图片重建测试", epilog=OPERAND_NOTE)
    parser.add_argument("--vae_checkpoint", type=str, default=None, help="预训练VAE模型文件路径 (.safetensors)")
    parser.add_argument("--vae_config_path", type=str, default=None, help="VAE配置文件路径 (JSON格式)")
    parser.add_argument("--image_path", type=str, default=None, help="输入图像路径 (可选，不提供则使用生成的测试图像)")
    parser.add_argument("--output_dir", type=str, default="vae_reconstruction_output", help="输出目录")
    parser.add_argument("--resolution", type=int, default=512, help="图像分辨率")
    parser.add_argument("--show_result", action="store_true", help="显示结果图像")
    parser.add_argument("--bf16_operands", action="store_true", help="卷积使用bf16操作数 (默认fp16)。" + OPERAND_NOTE)
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not args.vae_checkpoint and not args.vae_config_path:
        print("警告: 未提供VAE模型或配置，将使用默认配置创建新模型")
    test_vae_reconstruction(args)


if __name__ == "__main__":
    main()
