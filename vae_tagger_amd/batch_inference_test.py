"""Counterpart of the reference's batch_inference_test.py (same arguments and defaults, same batch_test_results.json, same printed
summary): per-image precision / recall / F1 of the tagger over a directory of images against the ground truth of a data JSON.

    python -m vae_tagger_amd.batch_inference_test --vae_checkpoint ae.safetensors --decoder_checkpoint dec.pth \
        --tags_csv_path tags.csv --image_dir imgs/ --data_json_path data.json [--max_images 10000] [--search]

The reference starts `infer_full.py` in a subprocess once per image and pays a model load per picture.  Here the images go through the
batched feeder and EncodeTagPipeline in ONE pass at the rate of `infer_full`, and the metric -- a reduction of the [B][N] probability
matrix along the classes -- is accumulated on the GPU in stream order (vt_sample_*, sample_metrics.DeviceSampleEvaluator).
Differences from the reference:
  * the `*.jpg` files of --image_dir are taken SORTED BY NAME (the reference takes directory order, which is not reproducible);
  * no result_NNN/classification_results.json per image is written;
  * --thresholds_json decides every tag at its own threshold (per_class_thresholds of an optimal_thresholds.json), --search scores the
    19 thresholds 0.05 ... 0.95 in the same pass and reports the best by avg_f1, --host_metrics computes the metric with numpy.
Ground truth as in the reference: the first entry of the JSON whose basename equals the image's; an image without one is skipped with
the reference's warning.  An image's true tags are the SET of names in its entry, whatever their weights; names outside the tag list
count in |true| (they lower recall) and can never be predicted.
Reference: batch_inference_test.py:6-46 (the per-image subprocess loop), :48-61 (load_ground_truth), :63-137 (calculate_metrics).
"""
import argparse
import json
from collections import deque
from pathlib import Path

import numpy as np

from .sample_metrics import SEARCH_GRID, best_threshold, per_image_values, sample_tallies_host, finish_host

TOP_K = 64              # (confidence, tag) pairs fetched per image; an image with more predicted tags fetches its prefix


def list_images(image_dir, max_images):
    """The first max_images `*.jpg` files of image_dir, sorted by name."""
    return [str(p) for p in sorted(Path(image_dir).glob("*.jpg"), key=lambda p: p.name)[:max_images]]


def load_ground_truth(data_json_path):
    """{path: [tag names]} -- the names of `tag:weight, tag:weight` in entry order (batch_inference_test.py:48-61)."""
    with open(data_json_path, "r", encoding="utf-8") as fh:
        data = json.load(fh)
    return {str(Path(p).as_posix()): [part.split(":")[0].strip() for part in str(label).split(", ")] for p, label in data.items()}


def match_ground_truth(image_path, ground_truth):
    """The tags of the first entry whose basename equals the image's, or None."""
    name = Path(str(Path(image_path).as_posix())).name
    for gt_path, tags in ground_truth.items():
        if Path(gt_path).name == name:
            return tags
    return None


def label_row(true_tags, tag_to_idx):
    """(uint8 [N] row of the true tags that are in the tag list, number of distinct true tags that are not)."""
    row = np.zeros(len(tag_to_idx), dtype=np.uint8)
    extra = 0
    for t in set(true_tags):
        k = tag_to_idx.get(t)
        if k is None:
            extra += 1
        else:
            row[k] = 1
    return row, extra


def build_results(names, true_tags, pred_tags, true, tp, predicted, sums=None):
    """The reference's metrics dict (keys in its order) from the integer tallies.  `sums`: (sum P, sum R, sum F1, exact matches) taken
    on the device; None sums on the host, in image order."""
    P, R, F, exact = per_image_values(tp, predicted, true)
    detailed = [{"image": Path(n).name, "true_tags": list(tt), "pred_tags": list(pt), "precision": float(P[i]), "recall": float(R[i]),
                 "f1": float(F[i]), "exact_match": int(exact[i])} for i, (n, tt, pt) in enumerate(zip(names, true_tags, pred_tags))]
    n = len(names)
    if sums is None:
        sp = sr = sf = 0.0
        for i in range(n):
            sp += float(P[i]); sr += float(R[i]); sf += float(F[i])
        sums = (sp, sr, sf, int(exact.sum()))
    if n:
        head = {"avg_precision": sums[0] / n, "avg_recall": sums[1] / n, "avg_f1": sums[2] / n, "exact_match_rate": sums[3] / n}
    else:
        head = {"avg_precision": 0, "avg_recall": 0, "avg_f1": 0, "exact_match_rate": 0}
    return dict(head, total_images=n, detailed_results=detailed)


def print_summary(metrics):
    print("\n整体性能指标")
    print(f"平均精确率: {metrics['avg_precision']:.4f}")
    print(f"平均召回率: {metrics['avg_recall']:.4f}")
    print(f"平均F1分数: {metrics['avg_f1']:.4f}")
    print(f"完全匹配率: {metrics['exact_match_rate']:.4f}")
    print(f"测试图像数: {metrics['total_images']}")
    print("\n详细结果")
    for r in metrics["detailed_results"]:
        print(f"{r['image']}:")
        print(f"  真实标签: {r['true_tags']}")
        print(f"  预测标签: {r['pred_tags']}")
        print(f"  精确率: {r['precision']:.3f}, 召回率: {r['recall']:.3f}, F1: {r['f1']:.3f}")
        print()


LAST_RUN_STATS = {}     # seconds spent in the image loop and the images it covered (tools/bench_cli.py reads it)


def run(args):
    import time
    import torch
    from .infer_full import load_class_thresholds, load_models
    from .modules import AspectRatioBucketing, get_image_transform
    from .pipeline import EncodeTagPipeline
    from .prefetch import BatchFeeder
    from .sample_metrics import DeviceSampleEvaluator
    if args.search and args.thresholds_json:
        raise RuntimeError("--search scores global thresholds; with --thresholds_json every tag has its own (drop one of the two flags)")
    if not torch.cuda.is_available():
        raise RuntimeError("vae_tagger_amd needs an MI355X (no HIP device visible; there is no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device())
    print("批量推理测试开始")
    vae_model, decoder, tag_names = load_models(args, device)
    tag_to_idx = {t: k for k, t in enumerate(tag_names)}
    N = len(tag_names)
    ground_truth = load_ground_truth(args.data_json_path)
    paths, truth = [], {}
    for p in list_images(args.image_dir, args.max_images):
        tags = match_ground_truth(p, ground_truth)
        if tags is None:
            print(f"警告: 找不到 {p} 的真实标签")
            continue
        paths.append(p)
        truth[p] = (tags,) + label_row(tags, tag_to_idx)
    print(f"开始对 {len(paths)} 张图像进行推理测试...")

    pipe = EncodeTagPipeline(vae_model, decoder)
    pipe.check_finite = False                 # the batches' health words are read in stream order (status_async), one batch late
    if args.fp8:
        pipe.set_fp8(True)
    elif args.fp16_operands:
        pipe.set_fp16_operands(True)
    thr = float(args.confidence_threshold)
    class_thr = load_class_thresholds(args.thresholds_json, tag_names, thr) if args.thresholds_json else None      # fp32 [N]
    grid = [float(t) for t in SEARCH_GRID] if args.search else []
    thresholds = grid + [thr]
    t_main = len(grid)
    host = bool(args.host_metrics)
    sample_ev = key_ev = None
    if not host:
        if class_thr is None:
            sample_ev = DeviceSampleEvaluator(thresholds, "ge", device, capacity=max(1, len(paths)), context=pipe.ctx)
        else:
            from .evaluation import DeviceMultiLabelEvaluator
            key_ev = DeviceMultiLabelEvaluator(tag_names, device, thresholds=[thr], threshold=thr, capacity=max(1, len(paths)), context=pipe.ctx)
    thr_dev = torch.from_numpy(class_thr).to(device) if class_thr is not None else None
    bucketing = AspectRatioBucketing(args.base_resolution, args.max_resolution, args.bucket_step) if args.use_bucketing else None
    feeder = BatchFeeder(pipe, paths, max(1, args.batch_size), args.resolution, workers=args.workers or None, host_resize=args.host_resize,
                         transform=get_image_transform(args.resolution), bucketing=bucketing)
    main_stream = torch.cuda.current_stream(device)
    done_names, pred_ids, summary_counts, host_probs, failed_all = [], [], [], [], []
    inflight = deque()

    def enqueue(names, x):
        b = len(names)
        logits = pipe.logits(x)
        conf, idx = pipe.confidence(logits)                                  # sorted descending (ties: ascending tag index)
        probs = torch.empty_like(conf).scatter_(1, idx, conf)                # the same bits in tag order: the metric's input
        rec = {"names": names, "conf": conf, "idx": idx}
        if host:
            rec["probs"] = torch.empty(b, N, dtype=torch.float32, pin_memory=True)
            rec["probs"].copy_(probs, non_blocking=True)
        else:
            labels = torch.from_numpy(np.stack([truth[p][1] for p in names])).pin_memory().to(device, non_blocking=True)
            if sample_ev is not None:
                extra = torch.tensor([truth[p][2] for p in names], dtype=torch.int32).pin_memory().to(device, non_blocking=True)
                n0 = sample_ev.n_seen
                sample_ev.update(probs, labels, extra)
                # this batch's `predicted` at the operating threshold, straight from the state's rows: the list below is cut to it
                rows = sample_ev.rows_view()
                rec["count"] = torch.empty(b, dtype=torch.int32, pin_memory=True)
                rec["count"].copy_(rows[n0:n0 + b, t_main, 1], non_blocking=True)
            else:
                key_ev.update(probs, labels)
            rec["host"], rec["K"] = pipe.summarize_async(conf, idx, thr_dev if thr_dev is not None else thr, TOP_K)
        rec["word"] = torch.empty(1, dtype=torch.int32, pin_memory=True)
        pipe.status_async(rec["word"])
        rec["ev"] = torch.cuda.Event()
        rec["ev"].record(main_stream)
        return rec

    def finish(rec):
        rec["ev"].synchronize()
        word = int(rec["word"][0])
        if word & 1:
            raise FloatingPointError("non-finite activations in the encoder: the fp16 residual-stream storage overflowed or the checkpoint / an image holds inf / NaN")
        if word & 2:
            raise FloatingPointError("fp8 mode: activations exceeded the e4m3 range and were clamped (run without --fp8)")
        done_names.extend(rec["names"])
        if host:
            host_probs.append(rec["probs"].numpy().copy())
            return
        top_conf, top_idx, stats = pipe.unpack_summary(rec["host"], rec["K"])
        for b in range(len(rec["names"])):
            count = int(rec["count"][b]) if "count" in rec else int(stats[b, 0])
            summary_counts.append(int(stats[b, 0]))
            if count <= top_idx.shape[1]:
                ids = top_idx[b, :count].tolist()
            elif class_thr is None:                 # more predicted tags than the summary carries: the prefix of the sorted list
                ids = rec["idx"][b, :count].cpu().tolist()
            else:                                   # per-tag thresholds: the passing tags are no prefix -- the whole row, filtered here
                cs, ix = rec["conf"][b].cpu().numpy(), rec["idx"][b].cpu().numpy()
                ids = ix[cs >= class_thr[ix]].tolist()
            pred_ids.append(ids)

    t_loop = time.perf_counter()
    for names, x, ready, failed in feeder:
        for p, e in failed:
            failed_all.append(p)
            print(f"跳过图像 {p}，错误原因: {e}")
        if names:
            main_stream.wait_event(ready)
            x.record_stream(main_stream)
            inflight.append(enqueue(names, x))
        while len(inflight) > 1:
            finish(inflight.popleft())
    while inflight:
        finish(inflight.popleft())
    torch.cuda.synchronize()
    LAST_RUN_STATS.update(loop_seconds=time.perf_counter() - t_loop, images=len(done_names))

    n = len(done_names)
    true_tags = [truth[p][0] for p in done_names]
    search = None
    if host:
        probs = np.concatenate(host_probs) if host_probs else np.zeros((0, N), dtype=np.float32)
        labels = np.stack([truth[p][1] for p in done_names]) if n else np.zeros((0, N), dtype=np.uint8)
        extra = np.asarray([truth[p][2] for p in done_names], dtype=np.uint32)
        if not np.isfinite(probs).all():
            raise FloatingPointError("non-finite confidences")
        thr_arg = class_thr.astype(np.float64)[None, :] if class_thr is not None else thresholds
        true, rows = sample_tallies_host(probs, labels, thr_arg, "ge", extra)
        order = np.argsort(-probs, axis=1, kind="stable")
        for i in range(n):
            ids = order[i]
            if class_thr is not None:
                pred_ids.append(ids[probs[i, ids] >= class_thr[ids]].tolist())
            else:
                pred_ids.append(ids[:rows[i, t_main, 1]].tolist())
        results = finish_host(true, rows) if n else []
        sums = None
    else:
        ev = sample_ev
        if key_ev is not None:
            extra = np.asarray([truth[p][2] for p in done_names], dtype=np.uint32)
            ev = DeviceSampleEvaluator.from_evaluator(key_ev, class_thr.astype(np.float64), "ge", extra) if n else None
        results = ev.finish() if ev is not None and n else []
        true, rows = ev.read_rows() if ev is not None and n else (np.zeros(0, np.uint32), np.zeros((0, len(thresholds), 2), np.uint32))
        if results and results[0]["nonfinite_probabilities"]:
            raise FloatingPointError(f"{results[0]['nonfinite_probabilities']} non-finite confidences")
        if key_ev is not None:
            t_main = 0
            # the list (vt_summarize_confidence_per_class) and the counts (the key store) were taken separately: they must agree
            assert summary_counts == rows[:, 0, 1].tolist(), "per-tag thresholds: the summary's counts differ from the recounted rows"
        sums = (results[t_main]["sum_precision"], results[t_main]["sum_recall"], results[t_main]["sum_f1"], results[t_main]["exact_matches"]) if n else None
    pred_tags = [[tag_names[k] for k in ids] for ids in pred_ids]
    metrics = build_results(done_names, true_tags, pred_tags, true, rows[:, t_main, 0], rows[:, t_main, 1], sums)
    if args.search and n:
        best = best_threshold(results[:len(grid)])
        keys = ("avg_precision", "avg_recall", "avg_f1", "exact_match_rate", "samples_recall_sklearn", "total_images")
        search = {"criterion": "avg_f1", "rule": "confidence >= threshold", "best_threshold": grid[best], "best_index": best,
                  "thresholds": [dict({"threshold": grid[k]}, **{key: results[k][key] for key in keys}) for k in range(len(grid))]}

    print_summary(metrics)
    out_dir = Path(args.output_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    out_file = out_dir / "batch_test_results.json"
    with open(out_file, "w", encoding="utf-8") as fh:
        json.dump(metrics, fh, indent=2, ensure_ascii=False)
    print(f"详细结果已保存到: {out_file}")
    if search is not None:
        with open(out_dir / "threshold_search.json", "w", encoding="utf-8") as fh:
            json.dump(search, fh, indent=2, ensure_ascii=False)
        print(f"最优阈值 (avg_f1): {search['best_threshold']:.2f}  avg_f1 = {search['thresholds'][search['best_index']]['avg_f1']:.4f}")
    return {"metrics": metrics, "search": search, "skipped": failed_all}


def build_parser():
    p = argparse.ArgumentParser(description="批量推理测试")
    p.add_argument("--vae_checkpoint", type=str, default="full_output/best_vae/diffusion_pytorch_model.safetensors")
    p.add_argument("--vae_config_path", type=str, default="full_output/best_vae/config.json")
    p.add_argument("--decoder_checkpoint", type=str, default="full_output/best_decoder/pytorch_model.bin")
    p.add_argument("--tags_csv_path", type=str, default="test_dataset/tags.csv")
    p.add_argument("--image_dir", type=str, default="test_dataset/images",
                   help="the *.jpg files of this directory, SORTED BY NAME (the reference takes directory order, which is not reproducible)")
    p.add_argument("--data_json_path", type=str, default="test_dataset/data.json")
    p.add_argument("--output_dir", type=str, default="batch_inference_results")
    p.add_argument("--max_images", type=int, default=10, help="测试的最大图像数量")
    p.add_argument("--confidence_threshold", type=float, default=0.3)
    p.add_argument("--resolution", type=int, default=256)
    # the decoder flags of infer_full
    p.add_argument("--use_attention", action="store_true", default=True, help="使用注意力机制 (默认开启)")
    p.add_argument("--no_attention", action="store_true", help="禁用注意力机制")
    p.add_argument("--use_spatial_attention", action="store_true", default=True, help="启用空间注意力")
    p.add_argument("--use_self_attention", action="store_true", default=True, help="启用自注意力")
    p.add_argument("--use_cross_attention", action="store_true", help="启用交叉注意力")
    p.add_argument("--attention_heads", type=int, default=8, help="注意力头数")
    p.add_argument("--attention_dropout", type=float, default=0.1, help="注意力dropout率")
    # this project's own
    p.add_argument("--batch_size", type=int, default=8, help="images per device batch (not in the reference)")
    p.add_argument("--use_bucketing", action="store_true", help="aspect-ratio buckets (SmartResize) instead of the square resize")
    p.add_argument("--base_resolution", type=int, default=512, help="分桶的基础分辨率")
    p.add_argument("--max_resolution", type=int, default=1024, help="分桶的最大分辨率")
    p.add_argument("--bucket_step", type=int, default=64, help="分桶的步长")
    p.add_argument("--workers", type=int, default=0, help="image decode threads (0 = min(16, cores))")
    p.add_argument("--host_resize", action="store_true", help="PIL resize + normalise on the CPU (the reference's route; same numbers, slower)")
    p.add_argument("--fp8", action="store_true", help="3x3 convs of the encoder on fp8 (e4m3) operands")
    p.add_argument("--fp16_operands", action="store_true", help="fp16 instead of bf16 MFMA operands for the convolutions")
    p.add_argument("--thresholds_json", type=str, default=None,
                   help="optimal_thresholds.json of a threshold search: every tag is decided at its own per_class_thresholds entry "
                        "(confidence >= threshold); tags the file does not name use --confidence_threshold")
    p.add_argument("--search", action="store_true",
                   help="also score the 19 thresholds 0.05 ... 0.95 in the same pass and write threshold_search.json (best by avg_f1)")
    p.add_argument("--host_metrics", action="store_true", help="compute the metric with numpy on probabilities copied back (same file)")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.no_attention:
        args.use_attention = False
    return run(args)


if __name__ == "__main__":
    main()
