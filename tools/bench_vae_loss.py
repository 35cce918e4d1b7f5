"""The VAE validation loss on the device at the flagship batch: 16 x 1024^2 (moments [16][32][128][128] x 3, images [16][3][1024][1024] x 2).

    python tools/bench_vae_loss.py                  # vt_posterior_sample, vt_vae_loss_update in flight and given z
    python tools/bench_vae_loss.py --cli --n 32     # evaluate_vae's images/s against three encodes + one decode on resident batches
    python tools/bench_vae_loss.py --backward       # vt_vae_loss_backward: the image pass, the latent pass and the whole call

Each call is event-timed next to (a) the torch-eager sequence the reference's classes would run on the same device tensors (randn + the
element-wise chain of sample(), kl(), F.mse_loss, F.normalize / pairwise_distance and the hinge) and (b) a torch device-to-device copy of
the bytes the call reads (the copy also writes them: 2 x the traffic), interleaved --reps times in one process; one JSON line per
measurement with the median and the best milliseconds.  --cli writes --n generated PNGs, runs the CLI's pass in this process and then the
bare encode / decode loop on batches that stay in HBM.  --backward times the loss's gradient beside (a) a torch copy that moves the bytes the
call reads PLUS writes (a copy of half of them: it reads and writes each) and (b) torch eager autograd of the same loss on fp32 tensors."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vae_tagger_amd import _lib, synth  # noqa: E402
from vae_tagger_amd.autoencoder_kl import DiagonalGaussianDistribution  # noqa: E402
from vae_tagger_amd.vae_losses import DeviceVAELossAccumulator  # noqa: E402


def timed(fns, reps):
    """{name: (median ms, best ms)} of the callables, interleaved reps times after one warm-up each."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: (statistics.median(v), min(v)) for k, v in ms.items()}


def eager_loss(moments, recon, target, la, lp, margin=1.0):
    """What the reference's validation step runs for the loss, in torch eager on the device."""
    post = [DiagonalGaussianDistribution(m) for m in moments]
    z = [p.sample().reshape(m.shape[0], -1) for p, m in zip(post, moments)]
    mse = F.mse_loss(recon, target)
    kl = torch.log(1 + ((post[0].kl() + post[1].kl() + post[2].kl()) / 3).mean() / 10000)
    an, pn, nn_ = (F.normalize(x, p=2, dim=1) for x in z)
    basic = F.relu((1 - (an * pn).sum(1)) - (1 - (an * nn_).sum(1)) + margin)
    trip = (basic * (1.0 + 0.5 * ((la * lp).sum(1) / (la.sum(1) + 1e-8)))).mean()
    return mse, kl, trip


def bench_kernels(args):
    B, C, h, res = args.batch, 16, args.res // 8, args.res
    g = torch.Generator().manual_seed(0)
    moments = [torch.randn(B, 2 * C, h, h, generator=g).cuda() for _ in range(3)]
    recon, target = (torch.rand(B, 3, res, res, generator=g).cuda() * 2 - 1 for _ in range(2))
    la, lp = ((torch.rand(B, args.tags, generator=g) < 0.02).float().cuda() for _ in range(2))
    ctx = _lib.Context(0)
    acc = DeviceVAELossAccumulator("cuda", context=ctx)
    dist = [DiagonalGaussianDistribution(m, ctx) for m in moments]
    z = [d.sample_device(1, k + 1, 0) for k, d in enumerate(dist)]
    lat_copy = [torch.empty_like(m) for m in moments]
    z_copy = [torch.empty_like(t) for t in z]
    img_copy = [torch.empty_like(recon), torch.empty_like(target)]

    def copy_latents(with_z):
        for d, s in zip(lat_copy, moments):
            d.copy_(s)
        if with_z:
            for d, s in zip(z_copy, z):
                d.copy_(s)

    def copy_all(with_z):
        copy_latents(with_z)
        img_copy[0].copy_(recon)
        img_copy[1].copy_(target)
    ins = lambda given: [(m, zz if given else None, k + 1) for k, (m, zz) in enumerate(zip(moments, z))]
    mb = lambda ts: sum(t.numel() * t.element_size() for t in ts) / 1e6
    groups = {
        "posterior_sample": ({"device": lambda: dist[0].sample_device(1, 1, 0), "eager": lambda: DiagonalGaussianDistribution(moments[0]).sample(),
                              "copy_of_bytes_read": lambda: lat_copy[0].copy_(moments[0])}, mb(moments[:1])),
        "posterior_kl": ({"device": lambda: dist[0].kl_device(), "eager": lambda: DiagonalGaussianDistribution(moments[0]).kl(),
                          "copy_of_bytes_read": lambda: lat_copy[0].copy_(moments[0])}, mb(moments[:1])),
        "update_in_flight": ({"device": lambda: acc.update(*ins(False), recon, target, la, lp), "eager": lambda: eager_loss(moments, recon, target, la, lp),
                              "copy_of_bytes_read": lambda: copy_all(False)}, mb(moments + [recon, target])),
        "update_given_z": ({"device": lambda: acc.update(*ins(True), recon, target, la, lp), "eager": lambda: eager_loss(moments, recon, target, la, lp),
                            "copy_of_bytes_read": lambda: copy_all(True)}, mb(moments + z + [recon, target])),
        "update_in_flight_latents_only": ({"device": lambda: acc.update(*ins(False), labels_a=la, labels_p=lp),
                                           "copy_of_bytes_read": lambda: copy_latents(False)}, mb(moments)),
        "update_given_z_latents_only": ({"device": lambda: acc.update(*ins(True), labels_a=la, labels_p=lp),
                                         "copy_of_bytes_read": lambda: copy_latents(True)}, mb(moments + z)),
    }
    for name, (fns, mbytes) in groups.items():
        r = timed(fns, args.reps)
        out = {"measurement": name, "batch": B, "res": res, "mb_read": round(mbytes, 1), "reps": args.reps}
        for k, (med, best) in r.items():
            out[k + "_ms_median"], out[k + "_ms_best"] = round(med, 4), round(best, 4)
        out["device_gb_per_s"] = round(mbytes / 1e3 / (r["device"][0] / 1e3), 1)
        out["device_over_copy"] = round(r["device"][0] / r["copy_of_bytes_read"][0], 2)
        print(json.dumps(out), flush=True)


def bench_backward(args):
    from vae_tagger_amd.vae_losses import backward_workspace_bytes, loss_backward_device
    B, C, h, res = args.batch, 16, args.res // 8, args.res
    g = torch.Generator().manual_seed(0)
    moments = [torch.randn(B, 2 * C, h, h, generator=g).cuda() for _ in range(3)]
    recon, target = (torch.rand(B, 3, res, res, generator=g).cuda() * 2 - 1 for _ in range(2))
    dz = (torch.randn(B, C, h, h, generator=g) * 1e-3).cuda()
    la, lp = ((torch.rand(B, args.tags, generator=g) < 0.02).float().cuda() for _ in range(2))
    ctx = _lib.Context(0)
    d_recon, d_moments = torch.empty_like(recon), torch.empty(3 * B, 2 * C, h, h, device="cuda")
    dm = [d_moments[i * B:(i + 1) * B] for i in range(3)]
    loss_out = torch.empty(4, dtype=torch.float64, device="cuda")
    ws = torch.empty(backward_workspace_bytes(B, C, h * h, res, res) + 256, dtype=torch.uint8, device="cuda")
    weights = {"reconstruction": 0.01, "kl": 1e-2, "triplet": 1.0}
    ins = [(m, k + 1) for k, m in enumerate(moments)]
    common = dict(weights=weights, workspace=ws, context=ctx)
    nbytes = lambda ts: sum(t.numel() * t.element_size() for t in ts)
    image_bytes = nbytes([recon, target, d_recon])                      # read recon, target; write d_recon
    latent_bytes = nbytes(moments + [dz, d_moments])                    # read the moments and dz_dec once; write the three d_moments
    copies = {k: (torch.empty(n // 2, dtype=torch.uint8, device="cuda"), torch.empty(n // 2, dtype=torch.uint8, device="cuda"))
              for k, n in (("image", image_bytes), ("latent", latent_bytes), ("both", image_bytes + latent_bytes))}
    q = [m.clone().requires_grad_(True) for m in moments]
    qr = recon.clone().requires_grad_(True)

    def eager():
        mse, kl, trip = eager_loss(q, qr, target, la, lp)
        total = weights["reconstruction"] * mse + weights["kl"] * kl + weights["triplet"] * trip
        return torch.autograd.grad(total, q + [qr])
    groups = {
        "backward_image_pass": ({"device": lambda: loss_backward_device(*ins, recon=recon, target=target, d_recon=d_recon, **common),
                                 "copy_of_bytes_read_and_written": lambda: copies["image"][1].copy_(copies["image"][0])}, image_bytes),
        "backward_latent_pass": ({"device": lambda: loss_backward_device(*ins, dz_dec=dz, labels_a=la, labels_p=lp, d_moments=dm, loss_out=loss_out, **common),
                                  "copy_of_bytes_read_and_written": lambda: copies["latent"][1].copy_(copies["latent"][0])}, latent_bytes),
        "backward_whole_call": ({"device": lambda: loss_backward_device(*ins, dz_dec=dz, recon=recon, target=target, labels_a=la, labels_p=lp,
                                                                        d_recon=d_recon, d_moments=dm, loss_out=loss_out, **common),
                                 "copy_of_bytes_read_and_written": lambda: copies["both"][1].copy_(copies["both"][0]), "eager_autograd_fp32": eager},
                                image_bytes + latent_bytes),
    }
    for name, (fns, n) in groups.items():
        r = timed(fns, args.reps)
        out = {"measurement": name, "batch": B, "res": res, "mb_read_and_written": round(n / 1e6, 1), "reps": args.reps}
        for k, (med, best) in r.items():
            out[k + "_ms_median"], out[k + "_ms_best"] = round(med, 4), round(best, 4)
        out["device_gb_per_s"] = round(n / 1e9 / (r["device"][0] / 1e3), 1)
        out["device_over_copy"] = round(r["device"][0] / r["copy_of_bytes_read_and_written"][0], 2)
        if "eager_autograd_fp32" in r:
            out["device_over_eager"] = round(r["device"][0] / r["eager_autograd_fp32"][0], 3)
        print(json.dumps(out), flush=True)


def bench_cli(args):
    from PIL import Image
    from vae_tagger_amd import evaluate_vae
    from vae_tagger_amd.diffusers_vae_loader import DiffusersVAEWrapper, get_diffusers_vae_config, load_diffusers_vae_from_config
    from safetensors.torch import save_file
    res, n, B = args.res, args.n, args.batch
    with tempfile.TemporaryDirectory() as tmp:
        rng = np.random.default_rng(0)
        paths = []
        for i in range(n):
            paths.append(os.path.join(tmp, f"{i}.png"))
            Image.fromarray(rng.integers(0, 256, (res, res, 3), dtype=np.uint8)).save(paths[-1], compress_level=1)
        tags = [f"t{k}" for k in range(8)]
        with open(os.path.join(tmp, "tags.csv"), "w") as fh:
            fh.write("name\n" + "\n".join(tags) + "\n")
        with open(os.path.join(tmp, "val.json"), "w") as fh:
            json.dump({p: ", ".join(tags[j] for j in range(8) if (i >> j) & 1 or j == i % 8) for i, p in enumerate(paths)}, fh)
        sd = synth.synth_state_dict(synth.encoder_manifest(), seed=0)
        sd.update(synth.synth_state_dict(synth.image_decoder_manifest(), seed=3))
        ckpt = os.path.join(tmp, "vae.safetensors")
        save_file({k: v.contiguous() for k, v in sd.items()}, ckpt)
        argv = ["--vae_checkpoint", ckpt, "--json_path", os.path.join(tmp, "val.json"), "--tags_csv_path", os.path.join(tmp, "tags.csv"),
                "--resolution", str(res), "--batch_size", str(B), "--output_dir", os.path.join(tmp, "out")]
        cli_args = evaluate_vae.build_parser().parse_args(argv)
        from vae_tagger_amd.evaluate import TaggedImageList
        data = TaggedImageList(cli_args.json_path, cli_args.tags_csv_path)
        labels = np.stack([data.labels[p] for p in data.image_paths]).astype(np.float32)
        triplets = evaluate_vae.triplet_lists(labels, cli_args.seed)
        batches = evaluate_vae.plan_batches(data.image_paths, B)
        model = DiffusersVAEWrapper(load_diffusers_vae_from_config(get_diffusers_vae_config(), ckpt)).to("cuda:0").eval()
        model.check_finite = False
        vae = model.vae
        run = lambda: evaluate_vae.run_checkpoint(cli_args, model, data, labels, triplets, batches, device=torch.device("cuda", 0))
        run()                                                            # warm-up: kernels loaded, workspaces grown, files in the page cache
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()                                                            # the CLI's pass over the data: image files -> parsed state and rows
        torch.cuda.synchronize()
        cli_s = time.perf_counter() - t0
        x = [synth.synth_images(B, res, res, seed=s).cuda() for s in range(3)]

        def step():
            post = [vae.encode(t).latent_dist for t in x]
            return vae.decode(post[0].sample_device(1, 0, 0)).sample
        step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(max(1, n // B)):
            step()
        torch.cuda.synchronize()
        bare_s = time.perf_counter() - t0
    steps = max(1, n // B)
    print(json.dumps({"measurement": "cli", "n": n, "batch": B, "res": res, "cli_pass_seconds": round(cli_s, 3),
                      "cli_anchor_images_per_s": round(n / cli_s, 2), "bare_three_encodes_one_decode_ms_per_batch": round(1e3 * bare_s / steps, 2),
                      "bare_anchor_images_per_s": round(steps * B / bare_s, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--tags", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--backward", action="store_true")
    args = ap.parse_args()
    (bench_cli if args.cli else bench_backward if args.backward else bench_kernels)(args)


if __name__ == "__main__":
    main()
