"""evaluate_model + find_optimal_threshold over a synthetic HBM-resident loader, host metrics against device metrics.

    python tools/bench_eval.py --n 2048 --leg host      # one leg per process: a driver script interleaves the legs, each under its own time limit
    python tools/bench_eval.py --n 2048 --leg device
    python tools/bench_eval.py --n 2048                 # both legs, host first

Per leg one JSON line: the loop's images/s (first batch requested -> last batch finished on the GPU, both passes) and the seconds between
the last batch and the return of the two calls (the metric finish: host numpy, or the device kernels + the final reads)."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vae_tagger_amd import synth  # noqa: E402
from vae_tagger_amd.diffusers_vae_loader import DiffusersVAEWrapper, get_diffusers_vae_config, load_diffusers_vae_from_config  # noqa: E402
from vae_tagger_amd.evaluation import evaluate_model, find_optimal_threshold  # noqa: E402
from vae_tagger_amd.modules import create_attention_decoder  # noqa: E402


class Loader:
    """n images in batches of `batch`, drawn from four resident batches; labels resident too.  Keeps the time stamps of the loop."""

    def __init__(self, n, batch, res, tags, device):
        self.n, self.batch = n, batch
        self.dataset = range(n)
        self.images = [synth.synth_images(batch, res, res, seed=10 + i).to(device) for i in range(4)]
        g = torch.Generator().manual_seed(1)
        self.labels = [(torch.rand(batch, tags, generator=g) < 0.02).float().to(device) for _ in range(4)]
        self.loop_s = 0.0
        self.t_end = None

    def __iter__(self):
        t0 = time.perf_counter()
        for lo in range(0, self.n, self.batch):
            b = min(self.batch, self.n - lo)
            k = (lo // self.batch) % 4
            yield {"pixel_values": self.images[k][:b], "labels": self.labels[k][:b]}
        torch.cuda.synchronize()                             # the tool's own fence: the loop ends when its last batch has
        self.t_end = time.perf_counter()
        self.loop_s += self.t_end - t0


def run_leg(leg, vae, dec, names, args):
    loader = Loader(args.n, args.batch, args.res, args.tags, "cuda")
    device_metrics = leg == "device"
    tail = 0.0
    with contextlib.redirect_stdout(io.StringIO()):
        m = evaluate_model(vae, dec, loader, names, device="cuda", device_metrics=device_metrics)
        tail += time.perf_counter() - loader.t_end
        r = find_optimal_threshold(vae, dec, loader, names, device="cuda", device_metrics=device_metrics)
        tail += time.perf_counter() - loader.t_end
    return {"leg": leg, "n": args.n, "tags": args.tags, "batch": args.batch, "res": args.res,
            "loop_images_per_s": round(2 * args.n / loader.loop_s, 2), "seconds_after_last_batch": round(tail, 3),
            "mAP": m["mAP"], "mAP_micro": m["mAP_micro"], "f1_micro": m["f1_micro"], "global_threshold": r["global_threshold"],
            "global_f1": r["global_f1"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--tags", type=int, default=10000)
    ap.add_argument("--leg", choices=["host", "device", "both"], default="both")
    args = ap.parse_args()
    vae = load_diffusers_vae_from_config(get_diffusers_vae_config())
    vae.load_state_dict(synth.synth_state_dict(synth.encoder_manifest(), seed=0), strict=False)
    vae = DiffusersVAEWrapper(vae).to("cuda").eval()
    with contextlib.redirect_stdout(io.StringIO()):
        dec = create_attention_decoder(16, 16, 16, args.tags, {"use_spatial_attention": True, "use_self_attention": True})
    dec.load_state_dict(synth.synth_state_dict(synth.attention_decoder_manifest(args.tags), seed=1), strict=False)
    dec = dec.to("cuda").eval()
    names = [f"tag_{i:05d}" for i in range(args.tags)]
    with torch.no_grad():                                    # warm-up: weights uploaded, kernels loaded
        torch.sigmoid(dec(vae.encode(synth.synth_images(args.batch, args.res, args.res, seed=0).cuda())))
    torch.cuda.synchronize()
    for leg in (["host", "device"] if args.leg == "both" else [args.leg]):
        print(json.dumps(run_leg(leg, vae, dec, names, args)), flush=True)


if __name__ == "__main__":
    main()
