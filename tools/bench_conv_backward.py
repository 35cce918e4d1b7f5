"""Timings of the resnet block's backward operators on the device (vae_tagger_amd/vae_backward.py), batch 1, at the FLUX VAE's layer shapes.

Per layer shape (C -> C at side^2): the weight gradient with the split the library chose and its two neighbours (half, double), the data gradient,
the GroupNorm + SiLU backward, the cast + bias-gradient pass -- beside (a) this library's forward conv of the same shape (same FLOPs), (b) torch's
own weight gradient on bf16 tensors, (c) a torch device copy, as the rate the HBM-bound passes are held against (their algorithmic bytes / time).
Per block (C -> C of each layer shape, 128 -> 256 and 512 -> 256 at 512^2): the whole resnet_block_backward beside torch autograd's backward of the
same block under bf16 autocast.  Everything is warmed first and timed in interleaved rounds; the figures are medians over the rounds.

--resample times the two resampling layers instead, batch 1, at the FLUX VAE's resample layers -- Downsample2D at 128 ch
1024^2 -> 512^2, 256 ch 512^2 -> 256^2, 512 ch 256^2 -> 128^2; Upsample2D at 512 ch 128^2 -> 256^2, 512 ch 256^2 -> 512^2, 256 ch 512^2 -> 1024^2:
each data gradient on both of its routes (the new kernel and the literal route, flag 23 / flag 22) in the same interleaved rounds, the weight gradient
beside the stride-1 weight gradient at the same output size, the forward layer, torch's conv2d_input / conv2d_weight on bf16 tensors and a torch copy
of the operand bytes.

Usage: python tools/bench_conv_backward.py [--resample] [--rounds 5] [--iters 5] [--scale 1024] [--skip-torch] [--out FILE]
Prints text lines and, last, one JSON line (also written to --out)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from vae_tagger_amd import vae_backward as vb  # noqa: E402

vp = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)  # noqa: E731
DEV = "cuda:0"
LAYERS = [(128, 1024), (256, 512), (512, 256), (512, 128)]             # channels, side at a 1024^2 image
BLOCKS = [(128, 128, 1024), (256, 256, 512), (512, 512, 256), (512, 512, 128), (128, 256, 512), (512, 256, 512)]


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


def block_params(cin, cout):
    p = {"norm1.weight": 1 + 0.1 * rnd(cin, seed=1), "norm1.bias": 0.1 * rnd(cin, seed=2), "conv1.weight": rnd(cout, cin, 3, 3, scale=(9 * cin) ** -0.5, seed=3),
         "conv1.bias": 0.1 * rnd(cout, seed=4), "norm2.weight": 1 + 0.1 * rnd(cout, seed=5), "norm2.bias": 0.1 * rnd(cout, seed=6),
         "conv2.weight": rnd(cout, cout, 3, 3, scale=(9 * cout) ** -0.5, seed=7), "conv2.bias": 0.1 * rnd(cout, seed=8)}
    if cin != cout:
        p["conv_shortcut.weight"] = rnd(cout, cin, 1, 1, scale=cin ** -0.5, seed=9)
        p["conv_shortcut.bias"] = 0.1 * rnd(cout, seed=10)
    return p


def bench_layer(C, side, rounds, iters, with_torch):
    ctx = vb.context(DEV)
    n = side * side
    dy = rnd(1, side, side, C, scale=n ** -0.5, seed=11)
    x = rnd(1, side, side, C, seed=12) + 0.5
    dy16, a16 = dy.to(torch.bfloat16), rnd(1, side, side, C, dtype=torch.bfloat16, seed=13)
    w = rnd(C, C, 3, 3, scale=(9 * C) ** -0.5, seed=14)
    w16 = w.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
    gamma, beta = 1 + 0.1 * rnd(C, seed=15), 0.1 * rnd(C, seed=16)
    stats = vb.groupnorm_stats(x)
    out = torch.empty(1, side, side, C, device=DEV)
    copy_src, copy_dst = torch.empty(n * C, device=DEV), torch.empty(n * C, device=DEV)
    auto = ctx.lib.vt_op_conv_backward_weight_workspace_bytes(1, side, side, C, C, 3, 0) // (C * C * 9 * 4)
    splits = sorted({max(1, auto // 2), auto, auto * 2})
    calls = {f"wgrad_splits_{s}": (lambda s=s: vb.conv_backward_weight(dy16, a16, 3, splits=s)) for s in splits}
    calls["dgrad"] = lambda: vb.conv_backward_data(dy16, w)
    calls["forward_conv"] = lambda: ctx.call("vt_op_conv2d", vp(a16), vp(w16), None, None, vp(out), None, 1, side, side, C, C, 3, 1, 1, 1, None)
    calls["gn_silu_backward"] = lambda: vb.groupnorm_silu_backward(x, stats, gamma, beta, dy, want_dx16=True)
    calls["cast_bias_grad"] = lambda: vb.cast_bias_grad(dy)
    calls["torch_copy"] = lambda: copy_dst.copy_(copy_src)
    torch_note = None
    if with_torch:
        try:
            tx = a16.permute(0, 3, 1, 2)                  # NCHW views of the NHWC buffers (channels_last)
            tdy = dy16.permute(0, 3, 1, 2)
            tw = w.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            calls["torch_wgrad_bf16"] = lambda: torch.ops.aten.convolution_backward(tdy, tx, tw, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [False, True, False])
            calls["torch_wgrad_bf16"]()
            torch.cuda.synchronize()
        except Exception as e:  # noqa: BLE001
            calls.pop("torch_wgrad_bf16", None)
            torch_note = f"torch weight gradient not measured: {type(e).__name__}: {e}"
    ms = interleaved(calls, rounds, iters)
    flops = 2.0 * n * C * C * 9
    nb = n * C
    bytes_gn = nb * (2 * 8 + 4 + 2)                        # x and da read in both passes, dx fp32 + bf16 written
    bytes_cast = nb * (4 + 2)
    copy_gbs = 2 * nb * 4 / ms["torch_copy"] / 1e6
    rec = {"channels": C, "side": side, "auto_splits": int(auto), "ms": {k: round(v, 4) for k, v in ms.items()},
           "tflops": {k: round(flops / v / 1e9, 1) for k, v in ms.items() if k.startswith(("wgrad", "dgrad", "forward", "torch_wgrad"))},
           "gbs": {"gn_silu_backward": round(bytes_gn / ms["gn_silu_backward"] / 1e6, 1), "cast_bias_grad": round(bytes_cast / ms["cast_bias_grad"] / 1e6, 1),
                   "torch_copy": round(copy_gbs, 1)}}
    best = min(v for k, v in ms.items() if k.startswith("wgrad"))
    rec["wgrad_over_forward"] = round(ms[f"wgrad_splits_{auto}"] / ms["forward_conv"], 3)
    rec["best_wgrad_over_forward"] = round(best / ms["forward_conv"], 3)
    if "torch_wgrad_bf16" in ms:
        rec["wgrad_over_torch"] = round(ms[f"wgrad_splits_{auto}"] / ms["torch_wgrad_bf16"], 3)
    if torch_note:
        rec["note"] = torch_note
    print(f"{C} ch @ {side}^2: " + "  ".join(f"{k} {v:.3f} ms" for k, v in ms.items()), flush=True)
    print(f"    TFLOP/s {rec['tflops']}  GB/s {rec['gbs']}", flush=True)
    return rec


RESAMPLE = [("down", 128, 1024), ("down", 256, 512), ("down", 512, 256), ("up", 512, 128), ("up", 512, 256), ("up", 256, 512)]      # kind, channels, input side


def bench_resample(kind, C, side, rounds, iters, with_torch):
    """side: the layer's INPUT side; the gradient dy has side // 2 (down) or 2 * side (up)"""
    ctx = vb.context(DEV)
    down = kind == "down"
    oside = side // 2 if down else 2 * side
    n_out = oside * oside
    dy16 = rnd(1, oside, oside, C, scale=n_out ** -0.5, dtype=torch.bfloat16, seed=31)
    x16 = rnd(1, side, side, C, dtype=torch.bfloat16, seed=32)
    s1_a16 = rnd(1, oside, oside, C, dtype=torch.bfloat16, seed=33)        # the stride-1 weight gradient at the same output size
    w = rnd(C, C, 3, 3, scale=(9 * C) ** -0.5, seed=34)
    bias = torch.zeros(C, device=DEV)
    flag = 23 if down else 22

    def routed(v, fn):
        def call():
            ctx.call("vt_set_flag", flag, v)
            try:
                return fn()
            finally:
                ctx.call("vt_set_flag", flag, 0)
        return call

    if down:
        dgrad = lambda: vb.downsample_backward_data(dy16, w, side, side)  # noqa: E731
        calls = {"wgrad": lambda: vb.downsample_backward_weight(dy16, x16), "forward": lambda: vb.downsample_forward(w, bias, x16)}
    else:
        dgrad = lambda: vb.upsample_backward_data(dy16, w)  # noqa: E731
        calls = {"wgrad": lambda: vb.upsample_backward_weight(dy16, x16), "forward": lambda: vb.upsample_forward(w, bias, x16)}
    calls["dgrad_kernel"], calls["dgrad_literal"] = routed(0, dgrad), routed(1, dgrad)
    calls["wgrad_stride1_same_output"] = lambda: vb.conv_backward_weight(dy16, s1_a16, 3)
    operand_bytes = (dy16.numel() + x16.numel()) * 2 + side * side * C * 4      # dy16 and the layer's input read, dx fp32 written
    copy_src = torch.empty(operand_bytes // 2, dtype=torch.uint8, device=DEV)
    copy_dst = torch.empty_like(copy_src)
    calls["torch_copy_operand_bytes"] = lambda: copy_dst.copy_(copy_src)
    note = None
    if with_torch:
        try:
            tdy = dy16.permute(0, 3, 1, 2)
            tw = w.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            if down:
                tx = F.pad(x16.permute(0, 3, 1, 2), (0, 1, 0, 1)).contiguous(memory_format=torch.channels_last)
                stride = [2, 2]
            else:
                tx = F.interpolate(x16.permute(0, 3, 1, 2), scale_factor=2, mode="nearest").contiguous(memory_format=torch.channels_last)
                stride = [1, 1]
            pad = [0, 0] if down else [1, 1]
            calls["torch_conv2d_input_bf16"] = lambda: torch.ops.aten.convolution_backward(tdy, tx, tw, None, stride, pad, [1, 1], False, [0, 0], 1, [True, False, False])
            calls["torch_conv2d_weight_bf16"] = lambda: torch.ops.aten.convolution_backward(tdy, tx, tw, None, stride, pad, [1, 1], False, [0, 0], 1, [False, True, False])
            calls["torch_conv2d_input_bf16"](); calls["torch_conv2d_weight_bf16"]()
            torch.cuda.synchronize()
        except Exception as e:  # noqa: BLE001
            calls.pop("torch_conv2d_input_bf16", None); calls.pop("torch_conv2d_weight_bf16", None)
            note = f"torch gradients not measured: {type(e).__name__}: {e}"
    ms = interleaved(calls, rounds, iters)
    flops = 2.0 * n_out * C * C * 9                         # the layer's own multiply-adds: 9 taps per output pixel
    rec = {"kind": kind, "channels": C, "in_side": side, "out_side": oside, "ms": {k: round(v, 4) for k, v in ms.items()},
           "dgrad_kernel_over_literal": round(ms["dgrad_kernel"] / ms["dgrad_literal"], 3),
           "wgrad_over_stride1_same_output": round(ms["wgrad"] / ms["wgrad_stride1_same_output"], 3),
           "wgrad_tflops": round(flops / ms["wgrad"] / 1e9, 1), "wgrad_stride1_tflops": round(flops / ms["wgrad_stride1_same_output"] / 1e9, 1),
           "copy_gbs": round(2 * copy_src.numel() / ms["torch_copy_operand_bytes"] / 1e6, 1)}
    if "torch_conv2d_weight_bf16" in ms:
        rec["wgrad_over_torch"] = round(ms["wgrad"] / ms["torch_conv2d_weight_bf16"], 3)
        rec["dgrad_kernel_over_torch"] = round(ms["dgrad_kernel"] / ms["torch_conv2d_input_bf16"], 3)
    if note:
        rec["note"] = note
    print(f"{kind} {C} ch {side}^2 -> {oside}^2: " + "  ".join(f"{k} {v:.3f} ms" for k, v in ms.items()), flush=True)
    print(f"    kernel / literal {rec['dgrad_kernel_over_literal']}  wgrad / stride-1 wgrad {rec['wgrad_over_stride1_same_output']}", flush=True)
    return rec


def torch_block(p, x):
    h = F.conv2d(F.silu(F.group_norm(x, 32, p["norm1.weight"], p["norm1.bias"], 1e-6)), p["conv1.weight"], p["conv1.bias"], padding=1)
    h = F.conv2d(F.silu(F.group_norm(h, 32, p["norm2.weight"], p["norm2.bias"], 1e-6)), p["conv2.weight"], p["conv2.bias"], padding=1)
    return h + (F.conv2d(x, p["conv_shortcut.weight"], p["conv_shortcut.bias"]) if "conv_shortcut.weight" in p else x)


def bench_block(cin, cout, side, rounds, iters, with_torch):
    p = block_params(cin, cout)
    x = rnd(1, side, side, cin, seed=21) + 0.5
    dy = rnd(1, side, side, cout, scale=(side * side) ** -0.5, seed=22)
    y, saved = vb.resnet_block_forward_train(p, x)
    calls = {"block_backward": lambda: vb.resnet_block_backward(p, saved, dy)}
    note = None
    if with_torch:
        try:
            q = {k: v.clone().requires_grad_(True) for k, v in p.items()}
            tx = x.permute(0, 3, 1, 2).requires_grad_(True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                ty = torch_block(q, tx)
            tdy = dy.permute(0, 3, 1, 2).to(ty.dtype)
            leaves = [tx] + list(q.values())
            calls["torch_autograd_bf16"] = lambda: torch.autograd.grad(ty, leaves, tdy, retain_graph=True)
            calls["torch_autograd_bf16"]()
            torch.cuda.synchronize()
        except Exception as e:  # noqa: BLE001
            calls.pop("torch_autograd_bf16", None)
            note = f"torch autograd not measured: {type(e).__name__}: {e}"
    ms = interleaved(calls, rounds, iters)
    rec = {"cin": cin, "cout": cout, "side": side, "ms": {k: round(v, 4) for k, v in ms.items()}}
    if "torch_autograd_bf16" in ms:
        rec["block_over_torch"] = round(ms["block_backward"] / ms["torch_autograd_bf16"], 3)
    if note:
        rec["note"] = note
    print(f"block {cin} -> {cout} @ {side}^2: " + "  ".join(f"{k} {v:.3f} ms" for k, v in ms.items()), flush=True)
    del saved, y
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--scale", type=int, default=1024, help="image side the layer sides are scaled to (1024: the real ones)")
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--skip-blocks", action="store_true")
    ap.add_argument("--resample", action="store_true", help="time the two resampling layers' backward instead (both routes of each data gradient)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv_backward needs a HIP device")
    sc = lambda s: max(8, s * a.scale // 1024)  # noqa: E731
    res = {"tool": "bench_conv_backward", "batch": 1, "rounds": a.rounds, "iters": a.iters, "scale": a.scale, "device": torch.cuda.get_device_name(0),
           "layers": [], "blocks": []}
    if a.resample:
        res["resample"] = []
        for kind, C, side in RESAMPLE:
            res["resample"].append(bench_resample(kind, C, sc(side), a.rounds, a.iters, not a.skip_torch))
            torch.cuda.empty_cache()
    for C, side in ([] if a.resample else LAYERS):
        res["layers"].append(bench_layer(C, sc(side), a.rounds, a.iters, not a.skip_torch))
        torch.cuda.empty_cache()
    if not a.skip_blocks and not a.resample:
        for cin, cout, side in BLOCKS:
            res["blocks"].append(bench_block(cin, cout, sc(side), a.rounds, a.iters, not a.skip_torch))
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
