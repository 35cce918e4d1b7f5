"""Step time of the classifier-head trainer against the same step in torch eager on the same GPU, interleaved.

    python tools/bench_train.py [--classes 10000] [--batch 16] [--plain] [--steps 200] [--rounds 5]

One step = forward (with dropout) + loss + backward + clip_grad_norm_ + AdamW, from cached feature rows.  Both sides run `steps`
steps between two device events, alternating for `rounds` rounds after a warm-up of each; the median round is reported with the
spread.  Also printed: the launches of one hand-written step (counted from the head's shape; copies included) and the bytes the step
must move at least -- about ten passes over the parameters: forward read, backward read of W, gradient read + write, clip (none
when nothing is clipped), AdamW's read of p, g, m, v and write of p, g, m, v -- against the measured time.
Prints one JSON line.

    python tools/bench_train.py --cli [--images 256] [--classes 10000] [--batch 16] [--epochs 3]

times the training CLI end to end on `--images` synthetic 1024 x 1024 JPEG files: first `evaluate --threshold 0.5` (ONE pass of encode ->
decoder -> metrics; the evaluate path is the parent commit's, unchanged) over the same files for its images/s, then
`train_decoder --no_attention` for `--epochs` epochs; reports epoch 1's images/s against evaluate's, and epoch 2's seconds against
epoch 1's (train_report.json).  A short warm-up run of each on 2 batches comes first."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def torch_head(sd, plain, rates, device):
    import torch.nn as nn
    nh = 2 if plain else 3
    layers = []
    for i in range(nh):
        w = sd[f"classifier.{4 * i}.weight"]
        layers += [nn.Linear(w.shape[1], w.shape[0]), nn.LayerNorm(w.shape[0]), nn.LeakyReLU(0.2) if plain else nn.ReLU(), nn.Dropout(rates[i])]
    w = sd[f"classifier.{4 * nh}.weight"]
    layers.append(nn.Linear(w.shape[1], w.shape[0]))
    head = nn.Sequential(*layers)
    head.load_state_dict({k[len("classifier."):]: v for k, v in sd.items() if k.startswith("classifier.")})
    return head.to(device).train()


def cli_mode(args):
    import shutil
    import tempfile
    import numpy as np
    from PIL import Image
    from safetensors.torch import save_file
    from vae_tagger_amd import evaluate, synth, train_decoder
    tmp = tempfile.mkdtemp(prefix="bench_train_")
    try:
        rng = np.random.default_rng(0)
        N, n = args.classes, args.images
        tags = [f"tag_{i:05d}" for i in range(N)]
        yy, xx = np.mgrid[0:1024, 0:1024].astype(np.float32) / 1024.0
        data = {}
        for i in range(n):
            f = rng.uniform(1, 6, size=6)
            img = np.stack([0.5 + 0.4 * np.sin(2 * np.pi * (f[2 * c] * xx + f[2 * c + 1] * yy)) for c in range(3)], -1)
            img = np.clip(img + rng.normal(0, 0.03, img.shape), 0, 1)
            path = os.path.join(tmp, f"img{i:04d}.jpg")
            Image.fromarray((img * 255).astype(np.uint8)).save(path, quality=90)
            data[path] = ", ".join(tags[(17 * i + 31 * k) % N] for k in range(12))
        names = list(data)
        for name, keys in (("data", names), ("warm", names[:2 * args.batch + 2])):
            with open(os.path.join(tmp, name + ".json"), "w") as fh:
                json.dump({k: data[k] for k in keys}, fh)
        with open(os.path.join(tmp, "tags.csv"), "w") as fh:
            fh.write("name\n" + "\n".join(tags) + "\n")
        save_file(synth.synth_state_dict(synth.encoder_manifest(), seed=0), os.path.join(tmp, "vae.safetensors"))
        torch.save(synth.synth_state_dict(synth.plain_decoder_manifest(N), seed=1), os.path.join(tmp, "dec.pth"))
        common = ["--vae_checkpoint", os.path.join(tmp, "vae.safetensors"), "--tags_csv_path", os.path.join(tmp, "tags.csv"), "--resolution", "1024",
                  "--no_attention"]
        ev = common + ["--decoder_checkpoint", os.path.join(tmp, "dec.pth"), "--batch_size", str(args.batch), "--threshold", "0.5"]
        trn = common + ["--train_batch_size", str(args.batch), "--save_steps", "1000", "--lr_warmup_steps", "10"]
        evaluate.main(ev + ["--json_path", os.path.join(tmp, "warm.json"), "--output_dir", os.path.join(tmp, "ev_warm")])
        evaluate.main(ev + ["--json_path", os.path.join(tmp, "data.json"), "--output_dir", os.path.join(tmp, "ev")])
        st = dict(evaluate.LAST_RUN_STATS)
        train_decoder.main(trn + ["--json_path", os.path.join(tmp, "warm.json"), "--output_dir", os.path.join(tmp, "tr_warm"), "--num_epochs", "2"])
        r = train_decoder.main(trn + ["--json_path", os.path.join(tmp, "data.json"), "--output_dir", os.path.join(tmp, "tr"),
                                      "--num_epochs", str(args.epochs)])
        ep = r["report"]["epochs"]
        eval_ips = st["images"] / st["loop_seconds"]
        out = {"bench": "train_cli", "images": n, "classes": N, "batch": args.batch, "evaluate_images_per_second": eval_ips,
               "epoch1_images_per_second": ep[0]["images_per_second"], "epoch1_over_evaluate": ep[0]["images_per_second"] / eval_ips,
               "epoch_seconds": [e["seconds"] for e in ep], "epoch2_over_epoch1_seconds": ep[1]["seconds"] / ep[0]["seconds"],
               "encoder_batches": [e["encoder_batches"] for e in ep], "steps": [e["steps"] for e in ep],
               "feature_cache_bytes": r["report"]["feature_cache_bytes"], "train_loss": r["history"]["train_loss"]}
        print(json.dumps(out))
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cli", action="store_true", help="time the training CLI's epochs against the evaluate CLI on the same files")
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--classes", type=int, default=10000)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args(argv)
    if args.cli:
        return cli_mode(args)
    from vae_tagger_amd import synth
    from vae_tagger_amd.modules import AttentionClassificationDecoder, ClassificationDecoder
    from vae_tagger_amd.train import HeadTrainer, head_dropout_rates
    dev = torch.device("cuda:0")
    N, B = args.classes, args.batch
    if args.plain:
        dec, sd = ClassificationDecoder(16, 16, 16, N), synth.synth_state_dict(synth.plain_decoder_manifest(N), seed=1)
    else:
        dec, sd = AttentionClassificationDecoder(16, 16, 16, N), synth.synth_state_dict(synth.attention_decoder_manifest(N), seed=1)
    dec.load_state_dict(sd, strict=False)
    dec = dec.to(dev).eval()
    rates = head_dropout_rates(dec)
    tr = HeadTrainer(dec)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, tr.F, generator=g).to(dev)
    y = (torch.rand(B, N, generator=g) < 0.01).float().to(dev)
    head = torch_head(sd, args.plain, rates, dev)
    opt = torch.optim.AdamW(head.parameters(), lr=1e-3, weight_decay=1e-6)
    loss_fn = torch.nn.BCEWithLogitsLoss()

    def ours(n):
        for _ in range(n):
            tr.forward_backward(x, y)
            tr.clip(1.0)
            tr.step(1e-3, 1e-6)

    def theirs(n):
        for _ in range(n):
            loss = loss_fn(head(x), y)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(head.parameters(), 1.0)
            opt.step()
            opt.zero_grad()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(args.steps)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.steps            # microseconds per step

    ours(20); theirs(20)
    torch.cuda.synchronize()
    t_ours, t_torch = [], []
    for _ in range(args.rounds):
        t_ours.append(timed(ours))
        t_torch.append(timed(theirs))
    nh = len(rates)
    params = sum(v.numel() for k, v in sd.items() if k.startswith("classifier."))
    # forward: linear + copy + layer norm + dropout per hidden layer, last linear; loss + fold; backward: linear per layer, layer norm per
    # hidden layer; clip: norm + scale; step: 1
    launches = 4 * nh + 1 + 2 + (nh + 1) + nh + 2 + 1
    floor_bytes = 4 * params * (1 + 1 + 2 + 8)
    out = {"bench": "train_step", "classes": N, "batch": B, "layout": "plain" if args.plain else "attention", "steps": args.steps,
           "rounds": args.rounds, "hip_us_per_step": statistics.median(t_ours), "hip_us_min_max": [min(t_ours), max(t_ours)],
           "torch_us_per_step": statistics.median(t_torch), "torch_us_min_max": [min(t_torch), max(t_torch)],
           "torch_over_hip": statistics.median(t_torch) / statistics.median(t_ours), "launches_per_step": launches,
           "head_parameters": params, "floor_bytes": floor_bytes,
           "achieved_GBps_against_floor": floor_bytes / (statistics.median(t_ours) * 1e-6) / 1e9}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
