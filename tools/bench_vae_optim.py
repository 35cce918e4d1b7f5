"""Timings of the VAE optimiser (vt_vae_optim_norm / vt_vae_optim_step) on the 244 tensor shapes of the FLUX configuration
with random data: the norm pass, the step pass, clip + step together; torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW (default and fused=True)
on the same tensors; and a torch device copy that moves the same bytes (the yardstick of profiles/r22: a copy of n bytes reads n and writes n).
Everything is warmed first and timed by device events in interleaved rounds; the figures are medians over the rounds.

--exchange K times the gradient exchange of a sharded train_vae on ONE device instead, with synthetic rows: the export
(vt_vae_grads_export) against a copy of the bytes it reads plus writes, the merge (vt_vae_grads_merge) of an owner's K slices for K = 2 and 8
against a copy of the same bytes, and export + owned-slice merge at K ranks + norm + step against norm + step alone.  No collective runs: this
yields no multi-GPU scaling figure.

Usage: python tools/bench_vae_optim.py [--rounds 7] [--iters 5] [--skip-torch] [--exchange K] [--out FILE]
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


def exchange_calls(trainer, grads, K, lr, wd, max_norm):
    """-> (calls, bytes moved per call): the exchange's device passes at K ranks, the owners' merges at 2 and 8, and their copy yardsticks"""
    from vae_tagger_amd.train_vae import TILE, owner_split
    elements = sum(trainer.numels)
    calls, moved, keep = {}, {}, []
    for k in sorted({2, 8, K}):
        S, row_floats = owner_split(trainer.total, k)
        slices = trainer._aligned(k * S * TILE)                                  # what the all-to-all leaves on a rank: K copies of its range
        slices.normal_(0.0, 0.01)
        out = trainer._aligned(S * TILE)
        w = [1.0 / k] * k
        keep.append((slices, out))
        calls[f"merge_k{k}"] = lambda slices=slices, out=out, w=w, S=S: trainer.merge_gradients(slices, S * TILE, w, 0, S * TILE, out)
        moved[f"merge_k{k}"] = 4 * (k + 1) * S * TILE
    S, row_floats = owner_split(trainer.total, K)
    row, merged = trainer._aligned(row_floats), trainer._aligned(row_floats)
    slices, w = keep[sorted({2, 8, K}).index(K)][0], [1.0 / K] * K
    views = trainer.gradient_views(merged)
    calls["export"] = lambda: trainer.export_gradients(grads, row)
    moved["export"] = 4 * (elements + row_floats)

    def plain_step():
        trainer.clip(grads, max_norm)
        trainer.step(grads, lr, wd)

    def exchanged_step():
        trainer.export_gradients(grads, row)
        trainer.merge_gradients(slices, S * TILE, w, 0, S * TILE, merged[:S * TILE])
        trainer.clip(views, max_norm)
        trainer.step(views, lr, wd)
    trainer.export_gradients(grads, merged)                                      # (the other owners' ranges of the merged row: any finite data)
    calls["clip_and_step"], calls["export_merge_clip_and_step"] = plain_step, exchanged_step
    src = torch.empty(max(moved.values()) // 2, dtype=torch.uint8, device=DEV)
    dst = torch.empty_like(src)
    for name, nbytes in list(moved.items()):                                     # a copy of n bytes moves 2 n
        calls["copy_of_" + name + "_bytes"] = lambda n=nbytes // 2: dst[:n].copy_(src[:n])
    return calls, moved


def exchange_main(a, trainer, grads, manifest, elements, lr, wd, max_norm):
    calls, moved = exchange_calls(trainer, grads, a.exchange, lr, wd, max_norm)
    ms = interleaved(calls, a.rounds, a.iters)
    ratios = {k: round(ms[k] / ms["copy_of_" + k + "_bytes"], 3) for k in moved}
    rec = {"tool": "bench_vae_optim --exchange", "device": torch.cuda.get_device_name(0), "tensors": len(manifest), "elements": elements,
           "arena_floats": trainer.total, "ranks": a.exchange, "rounds": a.rounds, "iters": a.iters, "ms": {k: round(v, 4) for k, v in ms.items()},
           "bytes": moved, "gbs": {k: round(moved[k] / ms[k] / 1e6, 1) for k in moved}, "over_copy": ratios,
           "exchange_device_passes_ms": round(ms["export_merge_clip_and_step"] - ms["clip_and_step"], 4)}
    print("  ".join(f"{k} {v:.4f} ms" for k, v in ms.items()), flush=True)
    for k in moved:
        print(f"{k}: {rec['gbs'][k]} GB/s, {ratios[k]} x the copy of its bytes", flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--exchange", type=int, default=0, metavar="K", help="time the sharded run's export and merge at K ranks instead (one device)")
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

    if a.exchange:
        if not 1 <= a.exchange <= 64:
            raise SystemExit("--exchange K: 1 to 64 ranks")
        rec = exchange_main(a, trainer, grads, manifest, elements, lr, wd, max_norm)
        line = json.dumps(rec)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        print(line)
        return

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
