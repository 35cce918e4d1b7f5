"""evaluate_model + find_optimal_threshold over a synthetic HBM-resident loader, host metrics against device metrics.

    python tools/bench_eval.py --n 2048 --leg host      # one leg per process: a driver script interleaves the legs, each under its own time limit
    python tools/bench_eval.py --n 2048 --leg device
    python tools/bench_eval.py --n 2048                 # both legs, host first
    python tools/bench_eval.py --merge 8                # sharded evaluation's merge: W synthetic shards on one GPU (no model is loaded)

    python tools/bench_eval.py --recount                # vt_eval_recount on a synthetic --tags x --n store (default 10000 x 8192; no model)
    python tools/bench_eval.py --sweep 10 --n 512       # the checkpoint sweep: K decoders per encode, interleaved with the one-decoder one-pass loop
    python tools/bench_eval.py --samples                # per-image metrics: vt_sample_from_keys against vt_eval_recount on the same store, update, finish

Per leg one JSON line: the loop's images/s (first batch requested -> last batch finished on the GPU, both passes) and the seconds between
the last batch and the return of the two calls (the metric finish: host numpy, or the device kernels + the final reads).
--merge W: at N = --tags and n = 2048 and 8192 samples per shard, event-timed milliseconds of the W exports, of the merge (head + key
kernel) and of the finish (sort + AP) on the merged state, next to a torch device-to-device copy of the same key bytes in the same
process -- the yardstick: the key kernel reads and writes every key once, 2 x key bytes -- with 16-B and with 8-B accesses (flag 21).
--recount: event-timed milliseconds of one vt_eval_recount call (the memset of its workspace, the key pass, the fold and the emit) on a store
of --tags classes x --n samples, at a scalar and at a per-class threshold vector, on the unsorted store and again after
vt_eval_average_precision has sorted the rows (the mismatch atomics then land scattered), next to a torch device-to-device copy of the
same key bytes: the recount only reads them, the copy reads and writes them.
--sweep K: images/s of evaluation.sweep_checkpoints' loop over K decoders (seeds 1..K; loss accumulators on) and of the one-decoder one-pass loop
(evaluate_and_search, the code of the single-checkpoint run), legs interleaved --reps times in one process; K x the one-decoder loop's time is what
K separate runs cost.  Also the event-timed milliseconds of one vt_loss_update against one vt_eval_update at (--batch, --tags), each over 20 calls.
--samples: on the store of --recount, event-timed milliseconds of vt_sample_from_keys, of vt_eval_recount and of a torch copy of the key bytes,
interleaved three times; of one vt_sample_update at B = 16, T = 19 (over 20 calls); and of vt_sample_finish at 8192 and 65536 images."""
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


def _timed(fn, reps):
    """Best and median event-timed milliseconds of fn() over `reps` runs after one warm-up."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[0], ms[len(ms) // 2]


def run_merge(W, tags, reps):
    import ctypes
    from vae_tagger_amd.evaluation import DeviceMultiLabelEvaluator
    names = [f"tag_{i:05d}" for i in range(tags)]
    g = torch.Generator(device="cuda").manual_seed(1)
    out = {"merge": W, "tags": tags, "reps": reps, "shards": []}
    for n in (2048, 8192):
        p = torch.rand(4096, tags, generator=g, device="cuda")
        y = (torch.rand(4096, tags, generator=g, device="cuda") < 0.02).to(torch.uint8)
        base = DeviceMultiLabelEvaluator(names, "cuda", capacity=n + 1)      # an odd pitch: the export compacts to n
        for lo in range(0, n, 4096):
            base.update(p[:min(4096, n - lo)], y[:min(4096, n - lo)])
        parts = [base] * W                                                   # W sources with one content: the traffic is what is timed
        key_bytes = W * n * tags * 8
        res = {"n_per_shard": n, "key_bytes": key_bytes}
        for vec in (1, 0):
            base.ctx.call("vt_set_flag", 21, vec)
            blocks = []

            def export():
                blocks.clear()
                blocks.extend(e.export_state(n) for e in parts)
            best_e, med_e = _timed(export, reps)
            merged = DeviceMultiLabelEvaluator(names, "cuda", capacity=W * n, context=base.ctx)

            def merge():
                merged.n_seen = 0
                merged.merge_from(blocks)
            best_m, med_m = _timed(merge, reps)
            # the timed runs added the counts reps + 1 times: start over and merge once, for the finish below
            merged.ctx.call("vt_eval_reset", ctypes.c_void_p(merged._ptr), merged._bytes, merged.N, merged.T,
                            (ctypes.c_double * merged.T)(*merged.thr.tolist()), merged.t_main, merged.capacity, merged._stream())
            merge()
            tag = "16B" if vec else "8B"
            res[f"export_ms_{tag}"] = round(best_e, 3)
            res[f"merge_ms_{tag}"] = round(best_m, 3)
            res[f"merge_ms_median_{tag}"] = round(med_m, 3)
            res[f"merge_key_bytes_per_s_{tag}"] = round(2 * key_bytes / (best_m * 1e-3), 0)       # read + write of every key
        base.ctx.call("vt_set_flag", 21, 1)
        src = torch.empty(key_bytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        best_c, med_c = _timed(lambda: dst.copy_(src), reps)
        res["torch_copy_ms"] = round(best_c, 3)
        res["torch_copy_bytes_per_s"] = round(2 * key_bytes / (best_c * 1e-3), 0)
        res["merge_over_copy_16B"] = round(res["merge_ms_16B"] / best_c, 3)
        res["merge_over_copy_8B"] = round(res["merge_ms_8B"] / best_c, 3)
        del src, dst
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        m = merged.compute_metrics()                                         # the existing finish: sort + AP (+ the final reads)
        b.record()
        b.synchronize()
        res["finish_ms"] = round(a.elapsed_time(b), 3)
        res["mAP"] = m["mAP"]
        out["shards"].append(res)
        del merged, blocks, base, parts
        torch.cuda.empty_cache()
    return out


def run_recount(n, tags, reps):
    import ctypes
    import numpy as np
    from vae_tagger_amd.evaluation import DeviceMultiLabelEvaluator
    names = [f"tag_{i:05d}" for i in range(tags)]
    g = torch.Generator(device="cuda").manual_seed(1)
    ev = DeviceMultiLabelEvaluator(names, "cuda", capacity=n)
    # what a trained tagger's outputs look like to the counter: ~2 % positives, few predictions above the threshold (squared uniforms)
    for lo in range(0, n, 2048):
        b = min(2048, n - lo)
        ev.update(torch.rand(b, tags, generator=g, device="cuda") ** 6, (torch.rand(b, tags, generator=g, device="cuda") < 0.02).to(torch.uint8))
    key_bytes = n * tags * 8
    vec = np.random.default_rng(0).choice(ev.grid, size=tags)
    res = {"recount": True, "n": n, "tags": tags, "reps": reps, "key_bytes": key_bytes}
    first = {}
    vp = ctypes.c_void_p                                                  # the C call itself is timed, on buffers allocated once
    counts = torch.empty(tags, 2, dtype=torch.int32, device="cuda")
    rows = torch.empty(3, dtype=torch.int64, device="cuda")
    ws_bytes = ev.ctx.lib.vt_eval_recount_workspace_bytes(tags, n)
    ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device="cuda")
    wp = (ws.data_ptr() + 255) // 256 * 256
    for state in ("unsorted", "sorted"):
        for name, thr in (("scalar", 0.5), ("per_class", vec), ("scalar_0.99", 0.99)):     # 0.99: few predictions, so few mismatch atomics
            first.setdefault(name, ev.recount(thr))
            again = ev.recount(thr)
            assert all(np.array_equal(x, y) for x, y in zip(first[name], again)), "recount changed with the order of the keys"
            thr_dev = torch.from_numpy(np.broadcast_to(np.asarray(thr, dtype=np.float64), (tags,)).copy()).cuda()
            best, med = _timed(lambda: ev.ctx.call("vt_eval_recount", vp(ev._ptr), ev._bytes, ev.N, ev.T, ev.capacity, ev.n_seen, vp(thr_dev.data_ptr()),
                                                   vp(counts.data_ptr()), counts.numel() * 4, vp(rows.data_ptr()), 24, vp(wp), ws_bytes, ev._stream()), reps)
            assert np.array_equal(counts.cpu().numpy().view(np.uint32), first[name][0]) and np.array_equal(rows.cpu().numpy().view(np.uint64), first[name][1])
            res[f"recount_ms_{state}_{name}"] = round(best, 3)
            res[f"recount_ms_median_{state}_{name}"] = round(med, 3)
            res[f"recount_read_bytes_per_s_{state}_{name}"] = round(key_bytes / (best * 1e-3), 0)
        if state == "unsorted":
            for name in first:
                res[f"mismatching_elements_{name}"] = int(first[name][1][1])
            ev.read_state(with_ap=True)                                      # sorts the class rows in place
    src = torch.empty(key_bytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    best_c, med_c = _timed(lambda: dst.copy_(src), reps)
    res["torch_copy_ms"] = round(best_c, 3)
    res["torch_copy_bytes_per_s"] = round(2 * key_bytes / (best_c * 1e-3), 0)
    for state in ("unsorted", "sorted"):
        res[f"recount_over_copy_{state}_per_class"] = round(res[f"recount_ms_{state}_per_class"] / best_c, 3)
    return res


def run_samples(n, tags, reps):
    """Per-image metrics: vt_sample_from_keys against vt_eval_recount and a torch copy on the same key store; vt_sample_update at
    B = 16, T = 19; vt_sample_finish at 8192 and 65536 images."""
    import ctypes
    import numpy as np
    from vae_tagger_amd.evaluation import DeviceMultiLabelEvaluator
    from vae_tagger_amd.sample_metrics import SEARCH_GRID, DeviceSampleEvaluator
    names = [f"tag_{i:05d}" for i in range(tags)]
    g = torch.Generator(device="cuda").manual_seed(1)
    ev = DeviceMultiLabelEvaluator(names, "cuda", capacity=n)
    for lo in range(0, n, 2048):                                             # the store of run_recount
        b = min(2048, n - lo)
        ev.update(torch.rand(b, tags, generator=g, device="cuda") ** 6, (torch.rand(b, tags, generator=g, device="cuda") < 0.02).to(torch.uint8))
    key_bytes = n * tags * 8
    vec = np.random.default_rng(0).choice(ev.grid, size=tags)
    res = {"samples": True, "n": n, "tags": tags, "reps": reps, "key_bytes": key_bytes}
    vp = ctypes.c_void_p
    counts = torch.empty(tags, 2, dtype=torch.int32, device="cuda")
    rows = torch.empty(3, dtype=torch.int64, device="cuda")
    ws_bytes = ev.ctx.lib.vt_eval_recount_workspace_bytes(tags, n)
    ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device="cuda")
    wp = (ws.data_ptr() + 255) // 256 * 256
    se = DeviceSampleEvaluator([float("nan")], "gt", "cuda", capacity=n, context=ev.ctx)
    src = torch.empty(key_bytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    for state in ("unsorted", "sorted"):
        for name, thr in (("scalar", 0.5), ("per_class", vec), ("scalar_0.99", 0.99)):
            thr_dev = torch.from_numpy(np.broadcast_to(np.asarray(thr, dtype=np.float64), (tags,)).copy()).cuda()
            rec = lambda: ev.ctx.call("vt_eval_recount", vp(ev._ptr), ev._bytes, ev.N, ev.T, ev.capacity, ev.n_seen, vp(thr_dev.data_ptr()),
                                      vp(counts.data_ptr()), counts.numel() * 4, vp(rows.data_ptr()), 24, vp(wp), ws_bytes, ev._stream())
            fk = lambda: ev.ctx.call("vt_sample_from_keys", vp(ev._ptr), ev._bytes, ev.N, ev.T, ev.capacity, ev.n_seen, vp(thr_dev.data_ptr()), 0,
                                     None, vp(se._ptr), se._bytes, se.capacity, ev._stream())
            r_ms, f_ms, c_ms = [], [], []
            for _ in range(3):                                               # interleaved on one box
                r_ms.append(_timed(rec, reps)[0]); f_ms.append(_timed(fk, reps)[0]); c_ms.append(_timed(lambda: dst.copy_(src), reps)[0])
            res[f"recount_ms_{state}_{name}"] = round(min(r_ms), 3)
            res[f"from_keys_ms_{state}_{name}"] = round(min(f_ms), 3)
            res[f"torch_copy_ms_{state}_{name}"] = round(min(c_ms), 3)
            res[f"from_keys_over_recount_{state}_{name}"] = round(min(f_ms) / min(r_ms), 4)
            res[f"from_keys_read_bytes_per_s_{state}_{name}"] = round(key_bytes / (min(f_ms) * 1e-3), 0)
        if state == "unsorted":
            se.n_seen = n
            first = se.read_rows()
            ev.read_state(with_ap=True)                                      # sorts the class rows in place
        else:
            again = se.read_rows()
            assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]), "from_keys changed with the order of the keys"
    del src, dst, ws
    # one update at the CLI's shape under --search, and the finish
    B, T = 16, len(SEARCH_GRID)
    probs = torch.rand(B, tags, device="cuda") ** 6
    labels = (torch.rand(B, tags, device="cuda") < 0.02).to(torch.uint8)
    for cap in (8192, 65536):
        su = DeviceSampleEvaluator(SEARCH_GRID, "ge", "cuda", capacity=cap)
        for lo in range(0, cap, B):                                          # fill the state with real rows
            su.ctx.call("vt_sample_update", vp(su._ptr), su._bytes, su.T, su.capacity, vp(probs.data_ptr()), vp(labels.data_ptr()), 3, None, B, tags,
                        lo, su._stream())
        su.n_seen = cap
        if cap == 8192:
            def updates():
                for k in range(20):
                    su.ctx.call("vt_sample_update", vp(su._ptr), su._bytes, su.T, su.capacity, vp(probs.data_ptr()), vp(labels.data_ptr()), 3, None, B,
                                tags, k * B, su._stream())
            best_u, med_u = _timed(updates, reps)
            res.update(update_B=B, update_T=T, update_ms=round(best_u / 20, 4), update_ms_median=round(med_u / 20, 4),
                       update_bytes=B * tags * 5 + B * (4 + 8 * T))
        out = torch.empty(su.ctx.lib.vt_sample_finish_bytes(T), dtype=torch.uint8, device="cuda")
        best_f, med_f = _timed(lambda: su.ctx.call("vt_sample_finish", vp(su._ptr), su._bytes, su.T, su.capacity, cap, vp(out.data_ptr()), out.numel(),
                                                   su._stream()), reps)
        res[f"finish_ms_{cap}"] = round(best_f, 4)
        res[f"finish_ms_median_{cap}"] = round(med_f, 4)
        res[f"finish_bytes_{cap}"] = cap * (4 + 8) * T                      # every workgroup reads `true` and its own column of the rows
    return res


def run_sweep(K, vae, names, args):
    import ctypes
    from vae_tagger_amd.evaluation import DeviceMultiLabelEvaluator, evaluate_and_search, sweep_checkpoints
    from vae_tagger_amd.losses import DeviceLossAccumulator, class_balanced_weights
    decs = []
    with contextlib.redirect_stdout(io.StringIO()):
        for k in range(K):
            d = create_attention_decoder(16, 16, 16, args.tags, {"use_spatial_attention": True, "use_self_attention": True})
            d.load_state_dict(synth.synth_state_dict(synth.attention_decoder_manifest(args.tags), seed=1 + k), strict=False)
            decs.append(d.to("cuda").eval())
    x = synth.synth_images(args.batch, args.res, args.res, seed=0).cuda()
    with torch.no_grad():
        lat = vae.encode(x)
        for d in decs:
            torch.sigmoid(d(lat))
    torch.cuda.synchronize()
    weights = class_balanced_weights(torch.arange(1, args.tags + 1).numpy())
    one_s, sweep_s = [], []
    for _ in range(args.reps):                               # interleaved: one-decoder loop, sweep loop, ...
        loader = Loader(args.n, args.batch, args.res, args.tags, "cuda")
        with contextlib.redirect_stdout(io.StringIO()):
            evaluate_and_search(vae, decs[0], loader, names, device="cuda")
        one_s.append(loader.loop_s)
        loader = Loader(args.n, args.batch, args.res, args.tags, "cuda")
        with contextlib.redirect_stdout(io.StringIO()):
            res = sweep_checkpoints(vae, decs, loader, names, device="cuda", class_weights=weights)
        sweep_s.append(loader.loop_s)
    one, sw = min(one_s), min(sweep_s)
    out = {"sweep": K, "n": args.n, "tags": args.tags, "batch": args.batch, "res": args.res, "reps": args.reps,
           "one_decoder_loop_images_per_s": round(args.n / one, 2), "sweep_loop_images_per_s": round(args.n / sw, 2),
           "one_decoder_loop_s": [round(v, 4) for v in one_s], "sweep_loop_s": [round(v, 4) for v in sweep_s],
           "sweep_over_one": round(sw / one, 4), "K_separate_runs_over_sweep": round(K * one / sw, 3),
           "val_loss_bce": [r["loss"]["bce"]["mean_of_batch_means"] for r in res]}
    # one vt_loss_update against one vt_eval_update at the same shape
    logits = torch.randn(args.batch, args.tags, device="cuda") * 3
    probs = torch.sigmoid(logits)
    labels = (torch.rand(args.batch, args.tags, device="cuda") < 0.02).float()
    acc = DeviceLossAccumulator(args.tags, "cuda", class_weights=weights)
    ev = DeviceMultiLabelEvaluator(names, "cuda", capacity=args.batch * 21 * (args.reps + 1))
    vp = ctypes.c_void_p

    def loss_calls():
        for _ in range(20):
            acc.ctx.call("vt_loss_update", vp(acc._ptr), acc._bytes, acc.N, vp(logits.data_ptr()), vp(labels.data_ptr()), 0, args.batch, acc._stream())

    def eval_calls():
        for _ in range(20):
            ev.ctx.call("vt_eval_update", vp(ev._ptr), ev._bytes, ev.N, ev.T, ev.t_main, ev.capacity, vp(probs.data_ptr()), vp(labels.data_ptr()), 0,
                        args.batch, ev.n_seen, ev._stream())
            ev.n_seen += args.batch
    best_l, med_l = _timed(loss_calls, args.reps)
    best_e, med_e = _timed(eval_calls, args.reps)
    out.update(loss_update_ms=round(best_l / 20, 4), loss_update_ms_median=round(med_l / 20, 4), eval_update_ms=round(best_e / 20, 4),
               eval_update_ms_median=round(med_e / 20, 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--tags", type=int, default=10000)
    ap.add_argument("--leg", choices=["host", "device", "both"], default="both")
    ap.add_argument("--merge", type=int, default=0, help="time export / merge / finish of this many synthetic shards (1..64) and exit")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", type=int, default=0, help="time the checkpoint sweep over this many decoders against the one-decoder one-pass loop and exit")
    ap.add_argument("--recount", action="store_true", help="time vt_eval_recount on a synthetic --tags x --n store (--n defaults to 8192 here) and exit")
    ap.add_argument("--samples", action="store_true",
                    help="per-image metrics: time vt_sample_from_keys against vt_eval_recount and a torch copy on a synthetic --tags x --n store "
                         "(--n defaults to 8192 here), vt_sample_update and vt_sample_finish, and exit")
    args = ap.parse_args()
    if args.samples:
        print(json.dumps(run_samples(8192 if args.n == 2048 else args.n, args.tags, args.reps)), flush=True)
        return
    if args.recount:
        print(json.dumps(run_recount(8192 if args.n == 2048 else args.n, args.tags, args.reps)), flush=True)
        return
    if args.merge:
        print(json.dumps(run_merge(args.merge, args.tags, args.reps)), flush=True)
        return
    vae = load_diffusers_vae_from_config(get_diffusers_vae_config())
    vae.load_state_dict(synth.synth_state_dict(synth.encoder_manifest(), seed=0), strict=False)
    vae = DiffusersVAEWrapper(vae).to("cuda").eval()
    with contextlib.redirect_stdout(io.StringIO()):
        dec = create_attention_decoder(16, 16, 16, args.tags, {"use_spatial_attention": True, "use_self_attention": True})
    dec.load_state_dict(synth.synth_state_dict(synth.attention_decoder_manifest(args.tags), seed=1), strict=False)
    dec = dec.to("cuda").eval()
    names = [f"tag_{i:05d}" for i in range(args.tags)]
    if args.sweep:
        print(json.dumps(run_sweep(args.sweep, vae, names, args)), flush=True)
        return
    with torch.no_grad():                                    # warm-up: weights uploaded, kernels loaded
        torch.sigmoid(dec(vae.encode(synth.synth_images(args.batch, args.res, args.res, seed=0).cuda())))
    torch.cuda.synchronize()
    for leg in (["host", "device"] if args.leg == "both" else [args.leg]):
        print(json.dumps(run_leg(leg, vae, dec, names, args)), flush=True)


if __name__ == "__main__":
    main()
