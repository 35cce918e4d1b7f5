"""Timings of the VAE's end convs and whole-model backward on the device (vae_tagger_amd/vae_backward.py), batch 1.

(a) The thin-side weight gradient (vt_op_conv_thin_backward_weight) in both forms at 1 x side^2 x 128, beside a torch device copy of the number of
    bytes it reads (the copy moves them twice) and the PADDED ROUTE: the thin side cast to bf16 and zero-padded to 64 NHWC channels on the existing
    vt_op_conv_backward_weight -- the operator call alone, and with the staging (cast + pad, torch) it needs.
(b) conv_out's data gradient (vt_op_conv_thin_forward, transpose_rotate) beside torch.nn.grad.conv2d_input on bf16 tensors.
(c) encoder_backward and decoder_backward of the FLUX configuration on synth weights at the given image sides, beside torch autograd's backward of the
    same model under bf16 autocast; torch.cuda.max_memory_allocated of a forward + backward beside encoder_saved_bytes / decoder_saved_bytes.
(d) --joined: vae_loss_and_grads (one step of train_vae: three encodes, the anchor's decode, the loss, all 244 gradients) at
    batch 1, beside the reference-shaped torch step -- three encodes, sample, one decode, the loss, backward() -- under bf16 autocast, with the peak
    allocated memory of both and vae_train_saved_bytes; then the whole train step (VAETrainer.train_step: the same backward, clip_grad_norm_ and AdamW over the
    244 gradients where they lie) and the optimiser's share of it.  With --joined only (d) runs.
Everything is warmed first and timed in interleaved rounds; the figures are medians over the rounds.

Usage: python tools/bench_vae_backward.py [--rounds 5] [--iters 3] [--side 1024] [--model-sides 512,1024] [--skip-torch] [--skip-models] [--joined] [--out FILE]
Prints text lines and, last, one JSON line (also written to --out)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from vae_tagger_amd import synth, vae_backward as vb  # noqa: E402

DEV = "cuda:0"
CW = 128


def time_calls(call, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def interleaved(calls, rounds, iters):
    """calls: name -> callable.  Warm each twice, then `rounds` rounds of every call in turn; -> name -> median ms"""
    for c in calls.values():
        c(); c()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(rounds):
        for k, c in calls.items():
            ms[k].append(time_calls(c, iters))
    return {k: statistics.median(v) for k, v in ms.items()}


def rnd(*shape, scale=1.0, dtype=torch.float32, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (scale * torch.randn(*shape, generator=g, device=DEV)).to(dtype)


def bench_thin(side, rounds, iters, with_torch):
    n = side * side
    thin = rnd(1, 3, side, side, seed=1)
    wide = rnd(1, side, side, CW, dtype=torch.bfloat16, seed=2)
    w_out = rnd(3, CW, 3, 3, scale=(9 * CW) ** -0.5, seed=3)
    read_bytes = wide.numel() * 2 + thin.numel() * 4
    copy_src = torch.empty(read_bytes, dtype=torch.uint8, device=DEV)
    copy_dst = torch.empty_like(copy_src)
    stage = lambda: F.pad(thin.permute(0, 2, 3, 1).to(torch.bfloat16), (0, 61))  # noqa: E731
    thin16 = stage()
    calls = {"thin_wgrad_conv_in": lambda: vb.conv_thin_backward_weight(thin, wide, True),
             "thin_wgrad_conv_out": lambda: vb.conv_thin_backward_weight(thin, wide, False, want_sums=True),
             "torch_copy_read_bytes": lambda: copy_dst.copy_(copy_src),
             "padded_wgrad_conv_in": lambda: vb.conv_backward_weight(wide, thin16, 3),
             "padded_wgrad_conv_out": lambda: vb.conv_backward_weight(thin16, wide, 3),
             "padded_staging": stage,
             "conv_out_dgrad": lambda: vb.conv_thin_forward(thin, w_out, transpose_rotate=True)}
    auto = int(vb.context(DEV).lib.vt_op_conv_thin_backward_weight_workspace_bytes(1, side, side, CW, 0) // (32 * CW * 4 + 24))
    for sp in (max(1, auto // 2), auto * 2):                  # the split the library chose against its two neighbours
        calls[f"thin_wgrad_conv_in_splits_{sp}"] = lambda sp=sp: vb.conv_thin_backward_weight(thin, wide, True, splits=sp)
    note = None
    if with_torch:
        try:
            td = thin.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            tw = w_out.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            calls["torch_conv2d_input_bf16"] = lambda: torch.nn.grad.conv2d_input((1, CW, side, side), tw, td, padding=1)
            calls["torch_conv2d_input_bf16"]()
            torch.cuda.synchronize()
        except Exception as e:  # noqa: BLE001
            calls.pop("torch_conv2d_input_bf16", None)
            note = f"torch conv2d_input not measured: {type(e).__name__}: {e}"
    ms = interleaved(calls, rounds, iters)
    rec = {"side": side, "channels": CW, "auto_splits": int(auto), "read_mb": round(read_bytes / 1e6, 1), "ms": {k: round(v, 4) for k, v in ms.items()},
           "gbs": {k: round(read_bytes / ms[k] / 1e6, 1) for k in ("thin_wgrad_conv_in", "thin_wgrad_conv_out")},
           "copy_gbs_moved": round(2 * read_bytes / ms["torch_copy_read_bytes"] / 1e6, 1)}
    for f in ("conv_in", "conv_out"):
        rec[f"{f}_over_copy"] = round(ms[f"thin_wgrad_{f}"] / ms["torch_copy_read_bytes"], 3)
        rec[f"{f}_over_padded"] = round(ms[f"thin_wgrad_{f}"] / ms[f"padded_wgrad_{f}"], 3)
        rec[f"{f}_over_padded_with_staging"] = round(ms[f"thin_wgrad_{f}"] / (ms[f"padded_wgrad_{f}"] + ms["padded_staging"]), 3)
    if "torch_conv2d_input_bf16" in ms:
        rec["conv_out_dgrad_over_torch"] = round(ms["conv_out_dgrad"] / ms["torch_conv2d_input_bf16"], 3)
    if note:
        rec["note"] = note
    print(f"thin ends @ {side}^2 x {CW}: " + "  ".join(f"{k} {v:.3f} ms" for k, v in ms.items()), flush=True)
    print(f"    {rec['gbs']} GB/s read; copy moves {rec['copy_gbs_moved']} GB/s; conv_in / copy {rec['conv_in_over_copy']}, / padded {rec['conv_in_over_padded']}; "
          f"conv_out / copy {rec['conv_out_over_copy']}, / padded {rec['conv_out_over_padded']}", flush=True)
    return rec


# ---- torch's own model, for the autograd comparison ------------------------------------------------------------------------------------------------
def t_resnet(p, n, x):
    h = F.conv2d(F.silu(F.group_norm(x, 32, p[n + "norm1.weight"], p[n + "norm1.bias"], 1e-6)), p[n + "conv1.weight"], p[n + "conv1.bias"], padding=1)
    h = F.conv2d(F.silu(F.group_norm(h, 32, p[n + "norm2.weight"], p[n + "norm2.bias"], 1e-6)), p[n + "conv2.weight"], p[n + "conv2.bias"], padding=1)
    return h + (F.conv2d(x, p[n + "conv_shortcut.weight"], p[n + "conv_shortcut.bias"]) if n + "conv_shortcut.weight" in p else x)


def t_mid(p, n, x):
    x = t_resnet(p, n + "resnets.0.", x)
    B, C, H, W = x.shape
    a = n + "attentions.0."
    h = F.group_norm(x, 32, p[a + "group_norm.weight"], p[a + "group_norm.bias"], 1e-6).reshape(B, C, H * W).transpose(1, 2)
    q, k, v = (F.linear(h, p[a + f"to_{s}.weight"], p[a + f"to_{s}.bias"]) for s in "qkv")
    o = F.scaled_dot_product_attention(q.unsqueeze(1), k.unsqueeze(1), v.unsqueeze(1)).squeeze(1)
    x = x + F.linear(o, p[a + "to_out.0.weight"], p[a + "to_out.0.bias"]).transpose(1, 2).reshape(B, C, H, W)
    return t_resnet(p, n + "resnets.1.", x)


def t_blocks(p, prefix, x, up):
    i = 0
    while f"{prefix}{i}.resnets.0.norm1.weight" in p:
        j = 0
        while f"{prefix}{i}.resnets.{j}.norm1.weight" in p:
            x = t_resnet(p, f"{prefix}{i}.resnets.{j}.", x)
            j += 1
        rs = f"{prefix}{i}." + ("upsamplers" if up else "downsamplers") + ".0.conv."
        if rs + "weight" in p:
            if up:
                x = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), p[rs + "weight"], p[rs + "bias"], padding=1)
            else:
                x = F.conv2d(F.pad(x, (0, 1, 0, 1)), p[rs + "weight"], p[rs + "bias"], stride=2)
        i += 1
    return x


def t_encoder(p, x):
    x = F.conv2d(x, p["encoder.conv_in.weight"], p["encoder.conv_in.bias"], padding=1)
    x = t_mid(p, "encoder.mid_block.", t_blocks(p, "encoder.down_blocks.", x, False))
    x = F.silu(F.group_norm(x, 32, p["encoder.conv_norm_out.weight"], p["encoder.conv_norm_out.bias"], 1e-6))
    return F.conv2d(x, p["encoder.conv_out.weight"], p["encoder.conv_out.bias"], padding=1)


def t_decoder(p, z):
    x = F.conv2d(z, p["decoder.conv_in.weight"], p["decoder.conv_in.bias"], padding=1)
    x = t_blocks(p, "decoder.up_blocks.", t_mid(p, "decoder.mid_block.", x), True)
    x = F.silu(F.group_norm(x, 32, p["decoder.conv_norm_out.weight"], p["decoder.conv_norm_out.bias"], 1e-6))
    return F.conv2d(x, p["decoder.conv_out.weight"], p["decoder.conv_out.bias"], padding=1)


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def bench_model(kind, side, rounds, iters, with_torch):
    enc = kind == "encoder"
    man = synth.encoder_manifest() if enc else synth.image_decoder_manifest()
    p = {k: v.to(DEV) for k, v in synth.synth_state_dict(man, seed=5).items()}
    x = synth.synth_images(1, side, side, seed=6).to(DEV) if enc else rnd(1, 16, side // 8, side // 8, seed=8)
    dy = rnd(1, 32, side // 8, side // 8, seed=7) if enc else rnd(1, 3, side, side, scale=1.0 / side, seed=9)
    fwd, bwd = (vb.encoder_forward_train, vb.encoder_backward) if enc else (vb.decoder_forward_train, vb.decoder_backward)
    formula = (vb.encoder_saved_bytes(p, 1, side, side) if enc else vb.decoder_saved_bytes(p, 1, side // 8, side // 8))
    peak = peak_of(lambda: bwd(p, fwd(p, x)[1], dy))
    y, saved = fwd(p, x)
    calls = {"forward_train": lambda: fwd(p, x), "backward": lambda: bwd(p, saved, dy)}
    rec = {"model": kind, "side": side, "saved_bytes": int(formula), "peak_allocated_forward_backward": int(peak)}
    note = None
    if with_torch:
        try:
            q = {k: v.clone().requires_grad_(True) for k, v in p.items()}
            tx = x.clone().requires_grad_(not enc)
            tmodel = t_encoder if enc else t_decoder

            def t_forward():
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    return tmodel(q, tx)

            leaves = list(q.values()) + ([] if enc else [tx])
            rec["torch_peak_allocated_forward_backward"] = int(peak_of(lambda: torch.autograd.grad(t_forward(), leaves, dy.to(torch.bfloat16))))
            ty = t_forward()
            tdy = dy.to(ty.dtype)
            calls["torch_forward_bf16"] = t_forward
            calls["torch_autograd_bf16"] = lambda: torch.autograd.grad(ty, leaves, tdy, retain_graph=True)
            calls["torch_autograd_bf16"]()
            torch.cuda.synchronize()
        except Exception as e:  # noqa: BLE001
            calls.pop("torch_forward_bf16", None); calls.pop("torch_autograd_bf16", None)
            note = f"torch autograd not measured: {type(e).__name__}: {e}"
    ms = interleaved(calls, rounds, iters)
    rec["ms"] = {k: round(v, 3) for k, v in ms.items()}
    if "torch_autograd_bf16" in ms:
        rec["backward_over_torch"] = round(ms["backward"] / ms["torch_autograd_bf16"], 3)
    if note:
        rec["note"] = note
    print(f"{kind} @ {side}^2: " + "  ".join(f"{k} {v:.2f} ms" for k, v in ms.items()) + f"  saved {formula / 2 ** 20:.0f} MiB, peak {peak / 2 ** 20:.0f} MiB"
          + (f", torch peak {rec['torch_peak_allocated_forward_backward'] / 2 ** 20:.0f} MiB" if "torch_peak_allocated_forward_backward" in rec else ""), flush=True)
    return rec


def t_step(q, a, pos, neg, weights, margin=1.0):
    """the reference's training step in torch: encode three times, sample, decode the anchor's latent, CombinedLoss without labels"""
    with torch.autocast("cuda", dtype=torch.bfloat16):
        moments = [t_encoder(q, x).float() for x in (a, pos, neg)]
    mean, lv = zip(*((m[:, :16], torch.clamp(m[:, 16:], -30.0, 20.0)) for m in moments))
    z = [mu + torch.exp(0.5 * l) * torch.randn_like(mu) for mu, l in zip(mean, lv)]
    with torch.autocast("cuda", dtype=torch.bfloat16):
        recon = t_decoder(q, mean[0] + torch.exp(0.5 * lv[0]) * torch.randn_like(mean[0])).float()
    kl = [0.5 * torch.sum(mu * mu + torch.exp(l) - 1.0 - l, dim=(1, 2, 3)) for mu, l in zip(mean, lv)]
    za, zp, zn = (F.normalize(t.flatten(1), p=2, dim=1) for t in z)
    trip = F.relu((1 - (za * zp).sum(1)) - (1 - (za * zn).sum(1)) + margin).mean()
    return (weights["reconstruction"] * F.mse_loss(recon, a) + weights["kl"] * torch.log(1 + ((kl[0] + kl[1] + kl[2]) / 3).mean() / 10000)
            + weights["triplet"] * trip)


def bench_joined(side, rounds, iters, with_torch):
    p = {k: v.to(DEV) for k, v in synth.synth_state_dict({**synth.encoder_manifest(), **synth.image_decoder_manifest()}, seed=5).items()}
    a, pos, neg = (synth.synth_images(1, side, side, seed=s).to(DEV) for s in (6, 7, 8))
    weights = {"reconstruction": 0.01, "kl": 1e-2, "triplet": 1.0}
    ours = lambda: vb.vae_loss_and_grads(p, a, pos, neg, weights=weights)  # noqa: E731
    rec = {"side": side, "saved_bytes": int(vb.vae_train_saved_bytes(p, 1, side, side)), "peak_allocated": int(peak_of(ours))}
    calls = {"vae_loss_and_grads": ours}
    # the whole train step: the same backward on the trainer's parameter views, then clip and AdamW where the gradients lie
    from vae_tagger_amd.train_vae import VAETrainer
    trainer = VAETrainer(p, weights=weights, device=DEV)
    calls["train_step"] = lambda: trainer.train_step(a, pos, neg, lr=1e-6, weight_decay=1e-6, max_grad_norm=1.0)  # noqa: E731
    held = vb.vae_loss_and_grads(trainer.params, a, pos, neg, weights=weights)[1]

    def optimiser_only():
        trainer.clip(held, 1.0)
        trainer.step(held, 1e-6, 1e-6)
    calls["clip_and_adamw"] = optimiser_only
    print(f"joined step @ {side}^2: saved {rec['saved_bytes'] / 2 ** 20:.0f} MiB, peak {rec['peak_allocated'] / 2 ** 20:.0f} MiB; torch's step next", flush=True)
    if with_torch:
        try:
            q = {k: v.clone().requires_grad_(True) for k, v in p.items()}
            leaves = list(q.values())
            t_call = lambda: torch.autograd.grad(t_step(q, a, pos, neg, weights), leaves)  # noqa: E731
            rec["torch_peak_allocated"] = int(peak_of(t_call))
            print(f"joined step @ {side}^2: torch's first step done, peak {rec['torch_peak_allocated'] / 2 ** 20:.0f} MiB; timing next", flush=True)
            calls["torch_step_bf16_autocast"] = t_call
        except Exception as e:  # noqa: BLE001
            calls.pop("torch_step_bf16_autocast", None)
            rec["note"] = f"torch step not measured: {type(e).__name__}: {e}"
    ms = interleaved(calls, rounds, iters)
    rec["ms"] = {k: round(v, 3) for k, v in ms.items()}
    rec["optimiser_share_of_train_step"] = round(ms["clip_and_adamw"] / ms["train_step"], 4)
    print(f"train step @ {side}^2: {ms['train_step']:.2f} ms, of which clip + AdamW {ms['clip_and_adamw']:.3f} ms ({100 * rec['optimiser_share_of_train_step']:.2f} %)", flush=True)
    if "torch_step_bf16_autocast" in ms:
        rec["step_over_torch"] = round(ms["vae_loss_and_grads"] / ms["torch_step_bf16_autocast"], 3)
    print(f"joined step @ {side}^2: " + "  ".join(f"{k} {v:.2f} ms" for k, v in ms.items()) + f"  saved {rec['saved_bytes'] / 2 ** 20:.0f} MiB, peak "
          f"{rec['peak_allocated'] / 2 ** 20:.0f} MiB" + (f", torch peak {rec['torch_peak_allocated'] / 2 ** 20:.0f} MiB" if "torch_peak_allocated" in rec else ""),
          flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--side", type=int, default=1024, help="image side of the thin-end measurements")
    ap.add_argument("--model-sides", default="512,1024")
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--skip-models", action="store_true")
    ap.add_argument("--joined", action="store_true", help="only the joined train step, (d)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vae_backward needs a HIP device")
    if a.joined:
        res = {"tool": "bench_vae_backward --joined", "batch": 1, "rounds": a.rounds, "iters": a.iters, "device": torch.cuda.get_device_name(0), "joined": []}
        for side in [int(s) for s in a.model_sides.split(",") if s]:
            res["joined"].append(bench_joined(side, a.rounds, a.iters, not a.skip_torch))
            torch.cuda.empty_cache()
        line = json.dumps(res)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        print(line)
        return
    res = {"tool": "bench_vae_backward", "batch": 1, "rounds": a.rounds, "iters": a.iters, "device": torch.cuda.get_device_name(0),
           "thin": bench_thin(a.side, a.rounds, a.iters, not a.skip_torch), "models": []}
    torch.cuda.empty_cache()
    if not a.skip_models:
        for side in [int(s) for s in a.model_sides.split(",") if s]:
            for kind in ("encoder", "decoder"):
                res["models"].append(bench_model(kind, side, a.rounds, a.iters, not a.skip_torch))
                torch.cuda.empty_cache()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
