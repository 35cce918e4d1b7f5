"""Timings of the VAE optimiser (vt_vae_optim_norm / vt_vae_optim_step) on the 244 tensor shapes of the FLUX configuration
with random data: the norm pass, the step pass, clip + step together; torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW (default and fused=True)
on the same tensors; and a torch device copy that moves the same bytes (the yardstick of profiles/r22: a copy of n bytes reads n and writes n).
Everything is warmed first and timed by device events in interleaved rounds; the figures are medians over the rounds.

Usage: python tools/bench_vae_optim.py [--rounds 7] [--iters 5] [--skip-torch] [--out FILE]
Prints text lines and, last, one JSON line (also written to --out)."""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from vae_tagger_amd import synth  # noqa: E402
from vae_tagger_amd.train_vae import VAETrainer  # noqa: E402

DEV = "cuda:0"


def time_calls(call, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def interleaved(calls, rounds, iters):
    for c in calls.values():
        c(); c()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(rounds):
        for k, c in calls.items():
            ms[k].append(time_calls(c, iters))
    return {k: statistics.median(v) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vae_optim needs a HIP device")
    manifest = {**synth.encoder_manifest(), **synth.image_decoder_manifest()}
    g = torch.Generator(device=DEV).manual_seed(0)
    params = {k: 0.05 * torch.randn(tuple(s), generator=g, device=DEV) for k, s in manifest.items()}
    grads = {k: 0.01 * torch.randn(tuple(s), generator=g, device=DEV) for k, s in manifest.items()}
    elements = sum(math.prod(s) for s in manifest.values())
    trainer = VAETrainer(params, weights={"reconstruction": 1.0, "triplet": 1.0}, device=DEV)
    norm_bytes, step_bytes = 4 * elements, 28 * elements                     # norm: reads g; step: reads g, p, m, v and writes p, m, v
    lr, wd, max_norm = 1e-6, 1e-6, 1.0

    def clip_and_step():
        trainer.clip(grads, max_norm)
        trainer.step(grads, lr, wd)

    def step_only():
        trainer._clipped = False
        trainer.step(grads, lr, wd)
    calls = {"norm": lambda: trainer.clip(grads, max_norm), "step": step_only, "clip_and_step": clip_and_step}
    # the copy yardstick: a copy of n bytes moves 2 n, so the pass that moves `bytes` is compared with a copy of bytes / 2
    src = torch.empty(step_bytes // 2, dtype=torch.uint8, device=DEV)
    dst = torch.empty_like(src)
    calls["copy_of_norm_bytes"] = lambda: dst[:norm_bytes // 2].copy_(src[:norm_bytes // 2])
    calls["copy_of_step_bytes"] = lambda: dst.copy_(src)
    if not a.skip_torch:
        for name, kw in (("torch_clip_adamw", {}), ("torch_clip_adamw_fused", {"fused": True})):
            ps = [p.clone().requires_grad_(True) for p in params.values()]
            for p, gr in zip(ps, grads.values()):
                p.grad = gr.clone()
            opt = torch.optim.AdamW(ps, lr=lr, weight_decay=wd, **kw)

            def torch_step(ps=ps, opt=opt):
                torch.nn.utils.clip_grad_norm_(ps, max_norm)
                opt.step()
            calls[name] = torch_step
    ms = interleaved(calls, a.rounds, a.iters)
    gbs = lambda nbytes, t: round(nbytes / t / 1e6, 1)  # noqa: E731
    rec = {"tool": "bench_vae_optim", "device": torch.cuda.get_device_name(0), "tensors": len(manifest), "elements": elements, "arena_floats": trainer.total,
           "rounds": a.rounds, "iters": a.iters, "ms": {k: round(v, 4) for k, v in ms.items()},
           "gbs": {"norm": gbs(norm_bytes, ms["norm"]), "step": gbs(step_bytes, ms["step"]), "copy_of_norm_bytes": gbs(norm_bytes, ms["copy_of_norm_bytes"]),
                   "copy_of_step_bytes": gbs(step_bytes, ms["copy_of_step_bytes"])},
           "norm_over_copy": round(ms["norm"] / ms["copy_of_norm_bytes"], 3), "step_over_copy": round(ms["step"] / ms["copy_of_step_bytes"], 3)}
    if "torch_clip_adamw_fused" in ms:
        rec["clip_and_step_over_torch_fused"] = round(ms["clip_and_step"] / ms["torch_clip_adamw_fused"], 3)
        rec["clip_and_step_over_torch_default"] = round(ms["clip_and_step"] / ms["torch_clip_adamw"], 3)
    print("  ".join(f"{k} {v:.4f} ms" for k, v in ms.items()), flush=True)
    print(f"norm {rec['gbs']['norm']} GB/s ({rec['norm_over_copy']} x the copy of its bytes at {rec['gbs']['copy_of_norm_bytes']} GB/s moved); "
          f"step {rec['gbs']['step']} GB/s ({rec['step_over_copy']} x the copy of its bytes at {rec['gbs']['copy_of_step_bytes']} GB/s moved)", flush=True)
    line = json.dumps(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
