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
epoch 1's (train_report.json).  A short warm-up run of each on 2 batches comes first.

    python tools/bench_train.py --front [--classes 10000] [--batch 16] [--latent 128] [--steps 100] [--rounds 5]

One FULL step of the attention decoder (train.DecoderTrainer: front forward in training mode, head forward / loss / backward with
d loss / d features, front backward, one clip over both blocks, AdamW on both) from a cached latent batch [batch][16][latent][latent],
against the head-only step (train.HeadTrainer on cached feature rows: the step the trainer had before the front could be trained) and
against the same full step in torch eager on the same GPU -- the three interleaved in one process, median round reported.

    python tools/bench_train.py --front --cross [--classes 10000] [--batch 16] [--latent 128] [--steps 50] [--rounds 5]

The full step of a decoder WITH cross-attention (front, cross-attention, head; one clip over three blocks, AdamW on three) against the
full step of the decoder without it and against the same cross-attention step in torch eager, interleaved in one process as above.

    python tools/bench_train.py --cli --train_front [--images 256] ...

times `train_decoder --train_front` (attention decoder from scratch): epoch 2's rate from the latent cache against epoch 1's.

    python tools/bench_train.py --merge 8 [--classes 10000] [--batch 16] [--latent 128] [--steps 50] [--rounds 5]

The gradient exchange of `train_decoder --sharded` on one GPU: export + merge (+ clip) of the three blocks over K synthetic gradient sets
against a torch device-to-device copy of the same K x P_total x 4 bytes, and the full step with a forced exchange on a one-rank RCCL
group against the plain step.  No multi-GPU figure can come from it."""
import argparse
import json
import math
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


class TorchAttentionDecoder(torch.nn.Module):
    """AttentionClassificationDecoder (spatial + self attention, cross-attention on request) in torch, for the eager comparison."""

    def __init__(self, N, heads=8, p=0.1, cross=False):
        import torch.nn as nn
        super().__init__()
        self.heads, self.cross = heads, cross
        if cross:
            self.qg, self.cq, self.co = nn.Linear(512, 512), nn.Linear(512, 256), nn.Linear(256, 512)
            self.ck, self.cv = nn.Linear(8, 256), nn.Linear(8, 256)
        self.ca = nn.Sequential(nn.Conv2d(16, 2, 1, bias=False), nn.ReLU(), nn.Conv2d(2, 16, 1, bias=False))
        self.sp = nn.Conv2d(2, 1, 7, padding=3, bias=False)
        self.compress = nn.Sequential(nn.Conv2d(16, 8, 3, 1, 1), nn.BatchNorm2d(8), nn.ReLU(), nn.AdaptiveAvgPool2d((8, 8)))
        self.norm, self.drop = nn.LayerNorm(8), nn.Dropout(p)
        self.q, self.k, self.v, self.o = (nn.Linear(8, 8) for _ in range(4))
        self.classifier = nn.Sequential(nn.Linear(512, 1024), nn.LayerNorm(1024), nn.ReLU(), nn.Dropout(0.3), nn.Linear(1024, 512), nn.LayerNorm(512),
                                        nn.ReLU(), nn.Dropout(0.2), nn.Linear(512, 256), nn.LayerNorm(256), nn.ReLU(), nn.Dropout(0.1),
                                        nn.Linear(256, N))

    def forward(self, x):
        import torch.nn.functional as F
        x = x * torch.sigmoid(self.ca(F.adaptive_avg_pool2d(x, 1)) + self.ca(F.adaptive_max_pool2d(x, 1)))
        x = x * torch.sigmoid(self.sp(torch.cat([x.mean(1, keepdim=True), x.max(1, keepdim=True)[0]], 1)))
        y = self.compress(x)
        B, hd = y.shape[0], 8 // self.heads
        t = y.view(B, 8, 64).transpose(1, 2)
        tn = self.norm(t)
        q, k, v = (m(tn).view(B, 64, self.heads, hd).transpose(1, 2) for m in (self.q, self.k, self.v))
        a = self.drop(torch.softmax(q @ k.transpose(-2, -1) / hd ** 0.5, dim=-1))
        o = self.o((a @ v).transpose(1, 2).reshape(B, 64, 8)) + t
        flat = o.transpose(1, 2).reshape(B, 512)
        if self.cross:
            hd = 256 // self.heads
            query = self.qg(flat)
            tok = flat.view(B, 8, 64).transpose(1, 2)
            u = self.cq(query).view(B, 1, self.heads, hd).transpose(1, 2)
            k, v = (m(tok).view(B, 64, self.heads, hd).transpose(1, 2) for m in (self.ck, self.cv))
            w = torch.softmax(u @ k.transpose(-2, -1) / hd ** 0.5, dim=-1)
            att = self.co((w @ v).transpose(1, 2).reshape(B, 256)) + query
            flat = flat + att.mean(dim=1, keepdim=True)
        return self.classifier(flat)


def front_mode(args):
    from vae_tagger_amd import synth
    from vae_tagger_amd.modules import AttentionClassificationDecoder
    from vae_tagger_amd.train import DecoderTrainer, HeadTrainer
    dev = torch.device("cuda:0")
    N, B, L = args.classes, args.batch, args.latent
    sd = synth.synth_state_dict(synth.attention_decoder_manifest(N), seed=1)
    dec = AttentionClassificationDecoder(16, L, L, N)
    dec.load_state_dict(sd, strict=False)
    dec = dec.to(dev).eval()
    full, head = DecoderTrainer(dec), HeadTrainer(dec)
    full_cross = None
    if args.cross:
        dec_x = AttentionClassificationDecoder(16, L, L, N, True, True, True, 8)
        dec_x.load_state_dict(synth.synth_state_dict(synth.attention_decoder_manifest(N, 16, True, True, True), seed=1), strict=False)
        full_cross = DecoderTrainer(dec_x.to(dev).eval())
    g = torch.Generator().manual_seed(0)
    lat = (0.1 + 0.8 * torch.randn(B, 16, L, L, generator=g)).to(dev)
    y = (torch.rand(B, N, generator=g) < 0.01).float().to(dev)
    feats = head.features(lat)
    ref = TorchAttentionDecoder(N, cross=args.cross).to(dev).train()
    opt = torch.optim.AdamW(ref.parameters(), lr=1e-3, weight_decay=1e-6)
    loss_fn = torch.nn.BCEWithLogitsLoss()

    def step_full(n):
        for _ in range(n):
            full.forward_backward(lat, y)
            full.clip(1.0)
            full.step(1e-3, 1e-6)

    def step_full_cross(n):
        for _ in range(n):
            full_cross.forward_backward(lat, y)
            full_cross.clip(1.0)
            full_cross.step(1e-3, 1e-6)

    def step_head(n):
        for _ in range(n):
            head.forward_backward(feats, y)
            head.clip(1.0)
            head.step(1e-3, 1e-6)

    def step_torch(n):
        for _ in range(n):
            loss_fn(ref(lat), y).backward()
            torch.nn.utils.clip_grad_norm_(ref.parameters(), 1.0)
            opt.step()
            opt.zero_grad()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(args.steps)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.steps            # microseconds per step

    fns = {"full": step_full, "head_only": step_head, "torch_full": step_torch}
    if args.cross:
        fns = {"full_cross": step_full_cross, "full": step_full, "torch_full_cross": step_torch}
    for fn in fns.values():
        fn(10)
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            times[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in times.items()}
    if args.cross:
        out = {"bench": "train_step_cross", "classes": N, "batch": B, "latent": [L, L], "steps": args.steps, "rounds": args.rounds,
               "full_cross_us_per_step": med["full_cross"], "full_us_per_step": med["full"], "torch_full_cross_us_per_step": med["torch_full_cross"],
               "us_min_max": {k: [min(v), max(v)] for k, v in times.items()}, "full_cross_over_full": med["full_cross"] / med["full"],
               "torch_over_full_cross": med["torch_full_cross"] / med["full_cross"], "cross_parameters": sum(math.prod(v) for v in full_cross.cross.shapes.values()),
               "latent_batch_bytes": lat.numel() * 4}
        print(json.dumps(out))
        return out
    out = {"bench": "train_step_front", "classes": N, "batch": B, "latent": [L, L], "steps": args.steps, "rounds": args.rounds,
           "full_us_per_step": med["full"], "head_only_us_per_step": med["head_only"], "torch_full_us_per_step": med["torch_full"],
           "us_min_max": {k: [min(v), max(v)] for k, v in times.items()}, "full_over_head_only": med["full"] / med["head_only"],
           "torch_over_full": med["torch_full"] / med["full"], "latent_batch_bytes": lat.numel() * 4}
    print(json.dumps(out))
    return out


def merge_mode(args):
    """--merge K: the gradient exchange of sharded training on ONE GPU.  (a) export + merge + clip, and the merge alone, of the three
    blocks of the decoder with cross-attention over K synthetic gradient sets [K][P_total], against a torch device-to-device copy of the
    same K P_total 4 bytes; (b) the full step with a forced exchange on a ONE-rank RCCL group (export, all_gather_into_tensor, the read
    of the count, merge of K = 1) against the plain step.  No collective between GPUs runs here: nothing about scaling follows."""
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(29800 + os.getpid() % 100))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda:0")
    dist.init_process_group("nccl", world_size=1, rank=0, device_id=dev)      # before any other GPU call of this process
    torch.cuda.set_device(dev)
    from vae_tagger_amd import synth
    from vae_tagger_amd.modules import AttentionClassificationDecoder
    from vae_tagger_amd.train import DecoderTrainer, GradientExchange
    N, B, L, K = args.classes, args.batch, args.latent, args.merge
    dec = AttentionClassificationDecoder(16, L, L, N, True, True, True, 8)
    dec.load_state_dict(synth.synth_state_dict(synth.attention_decoder_manifest(N, 16, True, True, True), seed=1), strict=False)
    dec = dec.to(dev).eval()
    tr, plain = DecoderTrainer(dec), DecoderTrainer(dec)
    ex = GradientExchange(tr, dist.group.WORLD, force_collective=True)
    P = tr.grads_floats()
    g = torch.Generator().manual_seed(0)
    src = (1e-3 * torch.randn(K, P, generator=g)).to(dev)
    dst, mine = torch.empty_like(src), torch.empty(P, dtype=torch.float32, device=dev)
    w = [(r + 1) / (K * (K + 1) / 2) for r in range(K)]
    lat = (0.1 + 0.8 * torch.randn(B, 16, L, L, generator=g)).to(dev)
    y = (torch.rand(B, N, generator=g) < 0.01).float().to(dev)

    def exchange_side(n):
        for _ in range(n):
            tr.export_gradients(mine)
            tr.merge_gradients(src, P, w)
            tr.clip(1.0)

    def merge_only(n):
        for _ in range(n):
            tr.merge_gradients(src, P, w)

    def torch_copy(n):
        for _ in range(n):
            dst.copy_(src)

    def step_plain(n):
        for _ in range(n):
            plain.forward_backward(lat, y)
            plain.clip(1.0)
            plain.step(1e-3, 1e-6)

    def step_exchange(n):
        for _ in range(n):
            tr.forward_backward(lat, y)
            ex.exchange(B)
            tr.clip(1.0)
            tr.step(1e-3, 1e-6)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(args.steps)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.steps            # microseconds per iteration

    fns = {"export_merge_clip": exchange_side, "merge": merge_only, "torch_copy": torch_copy, "step_plain": step_plain,
           "step_forced_exchange": step_exchange}
    for fn in fns.values():
        fn(5)
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            times[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"bench": "train_merge", "classes": N, "batch": B, "latent": [L, L], "ranks": K, "steps": args.steps, "rounds": args.rounds,
           "grads_floats": P, "blocks": [b.grads_floats() for b in tr.blocks()], "gathered_bytes": K * P * 4,
           "received_bytes_per_step_formula": "(K - 1) * 4 * (P_total + 4)", "received_bytes_per_step": (K - 1) * 4 * ex.row,
           "us": med, "us_min_max": {k: [min(v), max(v)] for k, v in times.items()},
           "merge_over_torch_copy": med["merge"] / med["torch_copy"], "export_merge_clip_over_torch_copy": med["export_merge_clip"] / med["torch_copy"],
           "merge_GBps": (K + 1) * P * 4 / (med["merge"] * 1e-6) / 1e9, "torch_copy_GBps": 2 * K * P * 4 / (med["torch_copy"] * 1e-6) / 1e9,
           "forced_exchange_step_over_plain_step": med["step_forced_exchange"] / med["step_plain"],
           "forced_exchange_overhead_us": med["step_forced_exchange"] - med["step_plain"], "backend": dist.get_backend()}
    print(json.dumps(out))
    dist.destroy_process_group()
    return out


def cli_front_mode(args, tmp, common, trn):
    from vae_tagger_amd import train_decoder
    common = [a for a in common if a != "--no_attention"]
    trn = [a for a in trn if a != "--no_attention"] + ["--train_front"]
    train_decoder.main(trn + ["--json_path", os.path.join(tmp, "warm.json"), "--output_dir", os.path.join(tmp, "trf_warm"), "--num_epochs", "2"])
    r = train_decoder.main(trn + ["--json_path", os.path.join(tmp, "data.json"), "--output_dir", os.path.join(tmp, "trf"),
                                  "--num_epochs", str(args.epochs)])
    ep = r["report"]["epochs"]
    out = {"bench": "train_cli_front", "images": args.images, "classes": args.classes, "batch": args.batch,
           "epoch_images_per_second": [e["images_per_second"] for e in ep], "epoch_seconds": [e["seconds"] for e in ep],
           "epoch2_over_epoch1_rate": ep[1]["images_per_second"] / ep[0]["images_per_second"],
           "encoder_batches": [e["encoder_batches"] for e in ep], "steps": [e["steps"] for e in ep], "latent_cache": r["report"]["latent_cache"],
           "train_loss": r["history"]["train_loss"]}
    print(json.dumps(out))
    return out


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
        if args.train_front:
            return cli_front_mode(args, tmp, common, trn)
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
    ap.add_argument("--front", action="store_true", help="time the full attention-decoder step against the head-only step and torch eager")
    ap.add_argument("--cross", action="store_true", help="with --front: the full step WITH cross-attention against the step without it and torch eager")
    ap.add_argument("--train_front", action="store_true", help="with --cli: time train_decoder --train_front (epoch 2 from the latent cache)")
    ap.add_argument("--latent", type=int, default=128, help="with --front: the latent's height and width")
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--classes", type=int, default=10000)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--merge", type=int, default=0, help="time the sharded run's gradient export + merge of this many synthetic ranks (1..64) and exit")
    args = ap.parse_args(argv)
    if args.merge:
        return merge_mode(args)
    if args.cli:
        return cli_mode(args)
    if args.front:
        return front_mode(args)
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
