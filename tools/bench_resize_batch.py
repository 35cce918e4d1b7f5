"""Input-side cost of one batch: 16 decoded images already on the device -> the encoder's fp32 NCHW input, by
  new:   ONE vt_resize_normalize_batch call (pipe.load_batch: a table copy + two launches whatever the batch size), and
  old:   the per-image route (pipe.resize_u8_into x B into a uint8 batch buffer + pipe.normalize_u8: about 3 B + 1 launches and a host
         wait per image on the context's single table-staging buffer),
interleaved on one box, for a 832x640 and a 1024x1024 bucket (SmartResize's crop + LANCZOS).  Prints stream time (HIP events) and host
time per batch; under `rocprofv3 --kernel-trace --stats -- python tools/bench_resize_batch.py` the kernel table gives the launch counts.

    python tools/bench_resize_batch.py [--batch 16] [--iters 20]
"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from vae_tagger_amd import synth
from vae_tagger_amd.diffusers_vae_loader import DiffusersVAEWrapper, get_diffusers_vae_config, load_diffusers_vae_from_config
from vae_tagger_amd.modules import smart_crop_box
from vae_tagger_amd.pipeline import EncodeTagPipeline

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--iters", type=int, default=20)
a = ap.parse_args()

vm = DiffusersVAEWrapper(load_diffusers_vae_from_config(get_diffusers_vae_config())).to("cuda").eval()
pipe = EncodeTagPipeline.input_side(vm)
side = torch.cuda.Stream()
rng = np.random.default_rng(0)
out = {}
for tw, th in ((832, 640), (1024, 1024)):
    # sources of the bucket's aspect, more or less, and of different sizes (every image has its own crop box and tables)
    sizes = [(int(tw * f) + 7 * k, int(th * f) + 5 * (k % 3)) for k, f in enumerate(np.linspace(0.8, 2.2, a.batch))]
    raws = [torch.from_numpy(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).cuda() for w, h in sizes]

    def new():
        return pipe.load_batch(raws, bucket=(tw, th), tag="bench")

    def old():
        u8 = torch.empty(len(raws), th, tw, 3, dtype=torch.uint8, device="cuda")
        for k, r in enumerate(raws):
            pipe.resize_u8_into(r, u8[k], pipe.FILTER_LANCZOS, box=smart_crop_box(r.shape[1], r.shape[0], tw, th), tag="bench_old")
        return pipe.normalize_u8(u8)

    with torch.cuda.stream(side):
        assert torch.equal(new(), old())
        res = {"new": {"stream_ms": [], "host_ms": []}, "old": {"stream_ms": [], "host_ms": []}}
        for it in range(a.iters + 2):
            for name, fn in (("new", new), ("old", old)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                side.synchronize()
                t0 = time.perf_counter()
                e0.record(side)
                fn()
                e1.record(side)
                host = (time.perf_counter() - t0) * 1e3
                side.synchronize()
                if it >= 2:
                    res[name]["stream_ms"].append(e0.elapsed_time(e1))
                    res[name]["host_ms"].append(host)
    out[f"{tw}x{th}"] = {k: {m: round(float(np.median(v)), 3) for m, v in r.items()} for k, r in res.items()}
    out[f"{tw}x{th}"]["source_megapixels"] = round(sum(w * h for w, h in sizes) / 1e6, 1)
print(json.dumps({"batch": a.batch, "iters": a.iters, "median_per_batch": out}), flush=True)
