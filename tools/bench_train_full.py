"""Timings of train_full's joint step (vae_tagger_amd/train_full.py) on the FLUX VAE and a 10 000-tag attention decoder with
synthetic weights, batch 1 at 512 x 512 and 1024 x 1024: FullTrainer.train_step under the simplified and under the full loss, each beside the sum of a
VAETrainer.train_step (train_vae) and a DecoderTrainer step (train_decoder --train_front) timed in the same process; the joint norm
(vt_full_optim_norm) against vt_vae_optim_norm + vt_train_clip and against a torch device copy of the bytes it reads; vt_posterior_mode_latent
against a copy of its bytes.  Everything is warmed first and timed by device events in interleaved rounds; the figures are medians over the rounds.

Usage: python tools/bench_train_full.py [--sizes 512 1024] [--tags 10000] [--rounds 5] [--iters 2] [--out FILE]
       python tools/bench_train_full.py --accumulate A ...      gradient accumulation instead (accumulate_bench)
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
from vae_tagger_amd.train import DecoderTrainer  # noqa: E402
from vae_tagger_amd.train_full import FullTrainer  # noqa: E402
from vae_tagger_amd.train_vae import VAETrainer  # noqa: E402

DEV = "cuda:0"
WEIGHTS = {"reconstruction": 0.01, "kl": 1e-7, "triplet": 1.0, "classification": 1.0}       # the reference parser's defaults
LR, WD, MAX_NORM = 1e-7, 1e-6, 1.0


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


def make_decoder(tags, seed):
    from vae_tagger_amd.modules import AttentionClassificationDecoder
    d = AttentionClassificationDecoder(16, 128, 128, tags)
    d.load_state_dict(synth.synth_state_dict(synth.attention_decoder_manifest(tags), seed=seed), strict=False)
    return d.to(DEV).eval()


def accumulate_bench(a):
    """--accumulate A: vt_vae_grads_accumulate, starting a sum and adding to one under a pending coefficient, against a torch device copy of the
    bytes it moves (first: n read + n written; adding: 2 n read + n written) and against the eager sequence it replaces on the same tensors
    (torch._foreach_mul_ by the coefficient, then torch._foreach_add_(..., alpha=scale)); and FullTrainer.micro_step, not stepping and
    stepping, against train_step of the same trainer class -- the step a run without accumulation takes."""
    import struct
    import numpy as np
    A = a.accumulate
    manifest = {**synth.encoder_manifest(), **synth.image_decoder_manifest()}
    params = synth.synth_state_dict(manifest, seed=0)
    kw = dict(margin=1.0, similarity_type="cosine", seed=0, scaling_factor=0.3611, shift_factor=0.1159)
    rec = {"tool": "bench_train_full --accumulate", "device": torch.cuda.get_device_name(0), "tags": a.tags, "accumulation_steps": A,
           "rounds": a.rounds, "iters": a.iters, "shapes": {}}
    g = torch.Generator().manual_seed(3)
    labels = (torch.rand(1, a.tags, generator=g) < 0.01).float().to(DEV)
    health = 0
    for loss in ("simplified", "full_loss"):
        plain = FullTrainer(params, make_decoder(a.tags, 1), weights=WEIGHTS, simplified=loss == "simplified", **kw)
        accum = FullTrainer(params, make_decoder(a.tags, 1), weights=WEIGHTS, simplified=loss == "simplified", **kw)
        v = accum.vae
        n_floats = sum(v.numels[:accum.n])
        for size in a.sizes:
            x = [t.to(DEV).contiguous() for t in synth.synth_images(3, size, size, seed=4).split(1)]
            step = {"n": 0}

            def parent_step():
                plain.train_step(x[0], x[1], x[2], labels, labels, step["n"], lr=LR, weight_decay=WD, max_grad_norm=MAX_NORM)
                step["n"] += 1

            def micro(now):
                accum.micro_step(x[0], x[1], x[2], labels, labels, step["n"], accumulation_steps=A, step_now=now, lr=LR, weight_decay=WD,
                                 max_grad_norm=MAX_NORM)
                step["n"] += 1
            micro(False)                                                         # (so that a stepping micro-step adds to a pending sum, as in a run)
            ms = interleaved({"train_step": parent_step, "micro_step_not_stepping": lambda: micro(False), "micro_step_stepping": lambda: micro(True)},
                             a.rounds, a.iters)
            # the pass alone, on the gradients of one backward
            _, grads, _ = accum.vae_forward_backward(x[0], x[1], x[2], labels, labels, 0)
            v._scalars.copy_(torch.from_numpy(np.frombuffer(struct.pack("<dff", 4.0, 2.0, 0.37), dtype=np.float64).copy()).to(DEV))
            views = list(v.accumulated(accum.n).values())
            glist = list(grads.values())
            src = torch.empty(6 * n_floats, dtype=torch.uint8, device=DEV)       # a copy of k bytes moves 2 k
            dst = torch.empty_like(src)

            def add_pending():
                v._clipped = True
                v.accumulate(grads, scale=1.0 / A, first=False, n=accum.n)

            def eager():
                torch._foreach_mul_(views, 0.37)
                torch._foreach_add_(views, glist, alpha=1.0 / A)
            calls = {"accumulate_first": lambda: v.accumulate(grads, scale=1.0 / A, first=True, n=accum.n), "accumulate_add_with_coef": add_pending,
                     "eager_foreach_mul_add": eager, "copy_of_first_bytes": lambda: dst[:4 * n_floats].copy_(src[:4 * n_floats]),
                     "copy_of_add_bytes": lambda: dst.copy_(src)}
            nms = interleaved(calls, a.rounds, max(a.iters, 10))
            v._clipped, accum.pending = False, 0
            del grads, glist, src, dst
            r = {"ms": {k: round(t, 4) for k, t in {**ms, **nms}.items()}, "gradient_floats": n_floats,
                 "first_over_copy": round(nms["accumulate_first"] / nms["copy_of_first_bytes"], 4),
                 "add_over_copy": round(nms["accumulate_add_with_coef"] / nms["copy_of_add_bytes"], 4),
                 "add_over_eager": round(nms["accumulate_add_with_coef"] / nms["eager_foreach_mul_add"], 4),
                 "stepping_minus_train_step_ms": round(ms["micro_step_stepping"] - ms["train_step"], 4),
                 "not_stepping_over_train_step": round(ms["micro_step_not_stepping"] / ms["train_step"], 4)}
            rec["shapes"][f"{loss} 1x{size}x{size}"] = r
            print(f"{loss} 1 x {size} x {size}: " + "  ".join(f"{k} {t:.3f} ms" for k, t in {**ms, **nms}.items()), flush=True)
            print(f"  first / copy = {r['first_over_copy']}; add / copy = {r['add_over_copy']}; add / eager = {r['add_over_eager']}; stepping micro-step "
                  f"- train_step = {r['stepping_minus_train_step_ms']} ms", flush=True)
        health |= v.ctx.status()
        del plain, accum, v
        torch.cuda.empty_cache()
    rec["health_word"] = health
    line = json.dumps(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--tags", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--accumulate", type=int, default=0, help="A > 0: time gradient accumulation at A micro-steps instead (accumulate_bench)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_full needs a HIP device")
    if a.accumulate > 0:
        return accumulate_bench(a)
    manifest = {**synth.encoder_manifest(), **synth.image_decoder_manifest()}
    params = synth.synth_state_dict(manifest, seed=0)
    elements = sum(math.prod(s) for s in manifest.values())
    encoder_elements = sum(math.prod(s) for k, s in manifest.items() if k.startswith("encoder."))
    kw = dict(margin=1.0, similarity_type="cosine", seed=0)
    simplified = FullTrainer(params, make_decoder(a.tags, 1), weights=WEIGHTS, simplified=True, scaling_factor=0.3611, shift_factor=0.1159, **kw)
    full = FullTrainer(params, make_decoder(a.tags, 1), weights=WEIGHTS, simplified=False, scaling_factor=0.3611, shift_factor=0.1159, **kw)
    vae = VAETrainer(params, weights={k: WEIGHTS[k] for k in ("reconstruction", "kl", "triplet")}, device=DEV, **kw)
    dec = DecoderTrainer(make_decoder(a.tags, 1), seed=0)
    rec = {"tool": "bench_train_full", "device": torch.cuda.get_device_name(0), "tags": a.tags, "vae_tensors": len(manifest), "vae_elements": elements,
           "encoder_elements": encoder_elements, "rounds": a.rounds, "iters": a.iters, "shapes": {}}
    g = torch.Generator().manual_seed(3)
    labels = (torch.rand(1, a.tags, generator=g) < 0.01).float().to(DEV)
    for size in a.sizes:
        x = [t.to(DEV).contiguous() for t in synth.synth_images(3, size, size, seed=4).split(1)]
        latent = torch.randn(1, 16, size // 8, size // 8, generator=g).to(DEV)
        step = {"n": 0}

        def joint_step(tr):
            tr.train_step(x[0], x[1], x[2], labels, labels, step["n"], lr=LR, weight_decay=WD, max_grad_norm=MAX_NORM)
            step["n"] += 1

        def vae_step():
            vae.train_step(x[0], x[1], x[2], labels, labels, step["n"], lr=LR, weight_decay=WD, max_grad_norm=MAX_NORM)

        def decoder_step():
            dec.forward_backward(latent, labels)
            dec.clip(MAX_NORM)
            dec.step(LR, WD)
        calls = {"full_step_simplified": lambda: joint_step(simplified), "full_step_full_loss": lambda: joint_step(full), "train_vae_step": vae_step,
                 "decoder_step": decoder_step}
        ms = interleaved(calls, a.rounds, a.iters)
        # the norm alone, on the gradients of one backward of each kind (kept alive for the calls below)
        _, grads, moments = full.vae_forward_backward(x[0], x[1], x[2], labels, labels, 0)
        full.decoder_forward_backward(full.mode_latent(moments, 1), labels, full.t)
        _, grads_e, _ = simplified.vae_forward_backward(x[0], x[1], x[2], labels, labels, 0)
        simplified.decoder_forward_backward(simplified.mode_latent(moments, 1), labels, simplified.t)

        def two_clips():
            full.vae.clip(grads, MAX_NORM)
            full.dec.clip(MAX_NORM)
        block_parts = 8 * 4096                                                # (the blocks' fp64 partials: a few KB beside the gradients' 335 MB)
        src = torch.empty(2 * elements + block_parts, dtype=torch.uint8, device=DEV)      # a copy of n bytes moves 2 n: half the bytes read
        dst = torch.empty_like(src)
        m_bytes = 16 * (size // 8) ** 2 * 4
        msrc, mdst = torch.empty(m_bytes, dtype=torch.uint8, device=DEV), torch.empty(m_bytes, dtype=torch.uint8, device=DEV)
        norm_calls = {"joint_norm_244": lambda: full.clip(grads, MAX_NORM), "two_separate_clips": two_clips,
                      "joint_norm_106": lambda: simplified.clip(grads_e, MAX_NORM), "copy_of_norm_bytes": lambda: dst.copy_(src),
                      "copy_of_encoder_norm_bytes": lambda: dst[:2 * encoder_elements].copy_(src[:2 * encoder_elements]),
                      "mode_latent": lambda: full.mode_latent(moments, 1), "copy_of_mode_latent_bytes": lambda: mdst.copy_(msrc)}
        nms = interleaved(norm_calls, a.rounds, max(a.iters, 10))
        full.vae._clipped = simplified.vae._clipped = False
        del grads, grads_e, moments
        separate = ms["train_vae_step"] + ms["decoder_step"]
        r = {"ms": {k: round(v, 4) for k, v in {**ms, **nms}.items()}, "separate_steps_sum_ms": round(separate, 4),
             "full_loss_over_separate": round(ms["full_step_full_loss"] / separate, 4),
             "simplified_over_full_loss": round(ms["full_step_simplified"] / ms["full_step_full_loss"], 4),
             "joint_norm_over_two_clips": round(nms["joint_norm_244"] / nms["two_separate_clips"], 4),
             "joint_norm_over_copy": round(nms["joint_norm_244"] / nms["copy_of_norm_bytes"], 4),
             "joint_norm_106_over_copy": round(nms["joint_norm_106"] / nms["copy_of_encoder_norm_bytes"], 4),
             "mode_latent_over_copy": round(nms["mode_latent"] / nms["copy_of_mode_latent_bytes"], 4),
             "saved_bytes": {"simplified": simplified.saved_bytes(x[0].shape), "full_loss": full.saved_bytes(x[0].shape)}}
        rec["shapes"][f"1x{size}x{size}"] = r
        print(f"1 x {size} x {size}: " + "  ".join(f"{k} {v:.3f} ms" for k, v in {**ms, **nms}.items()), flush=True)
        print(f"  full loss / (train_vae + decoder) = {r['full_loss_over_separate']}; simplified / full loss = {r['simplified_over_full_loss']}; "
              f"joint norm / two clips = {r['joint_norm_over_two_clips']}; joint norm / copy = {r['joint_norm_over_copy']}; "
              f"mode latent / copy = {r['mode_latent_over_copy']}", flush=True)
    st = simplified.vae.ctx.status()
    rec["health_word"] = st
    line = json.dumps(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
