"""VAE decode timings on the device.

  1. the three Upsample2D convs of the FLUX decoder as single layers (vt_op_upsample2x_conv3x3), folded kernel against literal route
     (vt_set_flag 22), interleaved round by round; ms, effective TFLOP/s counting the folded 4 taps per output pixel, and the ratio.
     Both routes pack their weights inside the call (a few MB, on the stream), and the literal route includes its upsample pass: that
     is the route.
  2. one whole decode at --resolution^2 (--batch images): ms per image, images/s, workspace bytes per image and the per-kernel split of
     vt_profile_begin / vt_profile_end.

Usage: python tools/bench_vae_decode.py [--batch 4] [--resolution 1024] [--rounds 5] [--iters 5] [--f16] [--skip-layers] [--skip-decode]
Prints text lines and, last, one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from vae_tagger_amd import _lib, synth  # noqa: E402
from vae_tagger_amd.vae_decoder import VAEImageDecoder  # noqa: E402

vp = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)  # noqa: E731
LAYERS = [(512, 128), (512, 256), (256, 512)]          # (channels, low-resolution side) of up_blocks.0-2 for a 1024^2 image


def time_calls(call, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def bench_layers(ctx, B, rounds, iters, f16, scale):
    dev = torch.device("cuda:0")
    out = []
    ctx.call("vt_set_flag", 18, int(f16))
    for C, side in LAYERS:
        side = max(1, side * scale // 1024)
        g = torch.Generator().manual_seed(0)
        x = torch.randn(B, side, side, C, generator=g).to(dev, torch.float16 if f16 else torch.bfloat16)
        w = (torch.randn(C, C, 3, 3, generator=g) * (C * 9) ** -0.5).to(dev)
        b = torch.zeros(C, device=dev)
        o = torch.empty(B, 2 * side, 2 * side, C, device=dev)

        def call():
            ctx.call("vt_op_upsample2x_conv3x3", vp(x), vp(w), vp(b), vp(o), B, side, side, C, None)
        ms = {0: [], 1: []}
        for literal in (0, 1):                            # warm-up: code objects, the operator scratch at its final size
            ctx.call("vt_set_flag", 22, literal)
            call(); call()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for literal in (0, 1):
                ctx.call("vt_set_flag", 22, literal)
                ms[literal].append(time_calls(call, iters))
        ctx.call("vt_set_flag", 22, 0)
        fl4 = 2.0 * B * (4 * side * side) * C * 4 * C
        mf, ml = statistics.median(ms[0]), statistics.median(ms[1])
        rec = {"channels": C, "low_res": side, "batch": B, "folded_ms": round(mf, 3), "literal_ms": round(ml, 3),
               "folded_tflops_4tap": round(fl4 / mf / 1e9, 1), "literal_tflops_4tap": round(fl4 / ml / 1e9, 1),
               "literal_over_folded": round(ml / mf, 3), "folded_ms_rounds": [round(v, 3) for v in ms[0]],
               "literal_ms_rounds": [round(v, 3) for v in ms[1]]}
        print(f"up conv {C} ch {side}^2 -> {2 * side}^2, batch {B}: folded {mf:.3f} ms ({rec['folded_tflops_4tap']} TF/s at 4 taps)  "
              f"literal {ml:.3f} ms ({rec['literal_tflops_4tap']} TF/s)  literal / folded = {rec['literal_over_folded']}", flush=True)
        out.append(rec)
        del x, w, o
        torch.cuda.empty_cache()
    ctx.call("vt_set_flag", 18, 0)
    return out


def bench_decode(B, res, iters, f16, literal):
    dec = VAEImageDecoder().to("cuda:0")
    dec.load_state_dict(synth.synth_state_dict(synth.image_decoder_manifest(), seed=3), strict=False)
    dec.set_fp16_operands(f16)
    dec.set_literal_upsample(literal)
    ctx = dec._context()
    z = torch.randn(B, 16, res // 8, res // 8, generator=torch.Generator().manual_seed(0)).cuda()
    ws_bytes = ctx.lib.vt_decode_image_workspace_bytes(ctx.handle, B, res // 8, res // 8)
    for _ in range(2):
        img = dec.decode(z)
    torch.cuda.synchronize()
    ms = time_calls(lambda: dec.decode(z), iters)
    st = dec.status()
    ctx.call("vt_profile_begin")
    dec.decode(z)
    n = ctx.lib.vt_profile_num_configs()
    launches, tot_ms, tot_fl, names = (ctypes.c_longlong * n)(), (ctypes.c_double * n)(), (ctypes.c_double * n)(), (ctypes.c_char_p * n)()
    ctx.call("vt_profile_end", n, launches, tot_ms, tot_fl, names)
    split = {}
    for i in range(n):
        if launches[i]:
            k = names[i].decode()
            e = split.setdefault(k, {"launches": 0, "ms": 0.0, "count": 0.0})
            e["launches"] += int(launches[i]); e["ms"] += tot_ms[i]; e["count"] += tot_fl[i]
    for k, e in split.items():
        unit = "GB/s" if k == "gn_apply_kernel" else "TFLOP/s"
        e["rate"] = round(e["count"] / e["ms"] / (1e6 if unit == "GB/s" else 1e9), 1) if e["ms"] else 0.0
        e["unit"] = unit; e["ms"] = round(e["ms"], 3); del e["count"]
    rec = {"batch": B, "resolution": res, "f16_operands": bool(f16), "literal_upsample": bool(literal), "ms_per_batch": round(ms, 2),
           "ms_per_image": round(ms / B, 2), "images_per_s": round(B / ms * 1e3, 2), "workspace_bytes_per_image": int(ws_bytes // B),
           "status": st, "output_absmax": round(img.abs().max().item(), 3), "profiled_ms": round(sum(e["ms"] for e in split.values()), 2),
           "per_kernel": split}
    print(f"decode {B} x {res}^2 ({'fp16' if f16 else 'bf16'} operands, {'literal' if literal else 'folded'} upsample): {rec['ms_per_image']} ms / image, "
          f"{rec['images_per_s']} images/s, workspace {ws_bytes / B / 2**30:.2f} GiB / image, status {st}", flush=True)
    for k, e in sorted(split.items(), key=lambda kv: -kv[1]["ms"]):
        print(f"    {k:40s} {e['launches']:4d} launches {e['ms']:9.3f} ms  {e['rate']} {e['unit']}", flush=True)
    del dec, z, img
    torch.cuda.empty_cache()
    return rec


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=4)
    p.add_argument("--resolution", type=int, default=1024)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--iters", type=int, default=5)
    p.add_argument("--f16", action="store_true", help="fp16 instead of bf16 operands (vt_set_flag 18)")
    p.add_argument("--skip-layers", action="store_true")
    p.add_argument("--skip-decode", action="store_true")
    a = p.parse_args()
    result = {"tool": "bench_vae_decode", "device": torch.cuda.get_device_name(0)}
    if not a.skip_layers:
        result["upsample_layers"] = bench_layers(_lib.Context(0), a.batch, a.rounds, a.iters, a.f16, a.resolution)
    if not a.skip_decode:
        result["decode"] = [bench_decode(a.batch, a.resolution, a.iters, a.f16, literal) for literal in (0, 1)]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
