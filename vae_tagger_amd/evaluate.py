"""Dataset evaluation CLI: what the reference's train_decoder.py runs after training (train_decoder.py:266-278) --
`find_optimal_threshold` over the labelled set, then `evaluate_model` at the global threshold -- as a command of its own, fed by the
pipelined loader of prefetch.py instead of a torch DataLoader over PIL transforms.

    python -m vae_tagger_amd.evaluate --vae_checkpoint ae.safetensors --decoder_checkpoint dec.pth --json_path data.json \
        --tags_csv_path tags.csv --use_bucketing [--base_resolution 512 --max_resolution 1024 --bucket_step 64] [--batch_size 8]

Writes `optimal_thresholds.json`, `evaluation_results.csv` and `evaluation_results_overall.json` into --output_dir, as the reference
does.  With --use_bucketing every image is centre-cropped to the aspect-ratio bucket of its own size and LANCZOS-resized (the
reference's SmartResize; on the GPU, Pillow's arithmetic bit for bit) and batches are formed per bucket; without it every image is
squashed to --resolution squared, as the inference CLIs do.  The data set is read TWICE unless --threshold or --single_pass is given:
once for the threshold search and once for the metrics at the threshold it found.  --single_pass keeps one sort key per (class, image)
on the GPU during the search pass and recounts the metrics at the threshold found from them (vt_eval_recount): same files, every image
encoded once.  --per_class_thresholds adds the metrics under the searched per-class thresholds (evaluation_results_per_class_thresholds.csv).  Metrics are accumulated on the GPU (DeviceMultiLabelEvaluator); --host_metrics is the host evaluator, same files.
One process by default; `torchrun ... -m vae_tagger_amd.evaluate ... --sharded` runs one rank per GPU: rank r takes paths[r::world], the
evaluator states are merged on rank 0 (evaluation.merge_across_ranks) after each pass and rank 0 writes the files.
--val_loss also reports the validation loss train_decoder.py keeps its best checkpoint by (BCE-with-logits, Focal and class-balanced
BCE, accumulated on the GPU from the logits: validation_loss.json); --decoder_checkpoints A B C ... scores several checkpoints of one
architecture in ONE pass -- every image is encoded once, each checkpoint's files go to output_dir/ckpt_<index>_<file stem>/ and
output_dir/checkpoint_sweep.json ranks them.  Reference: modules.py:487-548 (the JSON format), evaluation.py:173-275, train_decoder.py:284-333 (flags).
"""
import argparse
import json
import os

import numpy as np
import torch


class TaggedImageList:
    """The reference's training JSON, `{image path: "tag:weight, tag:weight"}`, against the tag vocabulary of a CSV's `name` column
    (what TaggedImageDataset.__init__ reads): `labels[path]` is an fp32 row holding each known tag's weight (1.0 when the entry has
    no weight or one that does not parse; an unknown tag is ignored; a repeated tag keeps its last weight).  Paths whose file does
    not exist are listed in `missing` and left out of `image_paths` (the reference fails on them when the image is opened)."""

    def __init__(self, json_path, tags_csv_path, check_files=True):
        import pandas as pd
        with open(json_path, "r", encoding="utf-8") as fh:
            data = json.load(fh)
        self.tags = [str(t) for t in pd.read_csv(tags_csv_path)["name"]]
        self.tag_to_idx = {t: i for i, t in enumerate(self.tags)}
        self.labels, self.image_paths, self.missing = {}, [], []
        for path, prompt in data.items():
            if check_files and not os.path.isfile(path):
                self.missing.append(path)
                continue
            self.image_paths.append(path)
            self.labels[path] = self.parse_prompt(prompt)

    def parse_prompt(self, prompt):
        row = np.zeros(len(self.tags), dtype=np.float32)
        # (a prompt without a comma is one entry, with or without a weight: the same rule as for each entry of a list)
        for entry in str(prompt).split(","):
            tag, sep, weight = entry.strip().partition(":")
            value = 1.0
            if sep:
                try:
                    value = float(weight.strip())
                except ValueError:
                    value = 1.0
            k = self.tag_to_idx.get(tag.strip())
            if k is not None:
                row[k] = value
        return row

    def __len__(self):
        return len(self.image_paths)


def build_loader(args, pipe, data):
    from .modules import AspectRatioBucketing, get_image_transform
    from .prefetch import FeederLoader
    bucketing = AspectRatioBucketing(args.base_resolution, args.max_resolution, args.bucket_step) if args.use_bucketing else None
    return FeederLoader(pipe, data.image_paths, data.labels, args.batch_size, args.resolution, workers=args.workers or None,
                        host_resize=args.host_resize, transform=get_image_transform(args.resolution), bucketing=bucketing,
                        max_pending=args.max_pending or None)


LAST_RUN_STATS = {}    # seconds spent in the passes over the data and the images they covered (tools/bench_cli.py reads it)


def shard_paths(paths, rank, world):
    """Rank r's share of the image list: paths[r::world].  Over r the shares partition the list; deterministic, balanced in the number
    of images (not in their cost: see DESIGN.md section 4.15)."""
    return list(paths[rank::world])


def check_mode(args, world_size):
    """The flag combinations that are refused, before any GPU or process-group work."""
    sharded = getattr(args, "sharded", False)
    if sharded and args.host_metrics:
        raise RuntimeError("--sharded merges the device evaluator's state; the host matrix of --host_metrics is not merged "
                           "(drop one of the two flags)")
    sweep = getattr(args, "decoder_checkpoints", None)
    if (sweep or getattr(args, "val_loss", False)) and args.host_metrics:
        raise RuntimeError("--val_loss and --decoder_checkpoints accumulate on the GPU (the loss from the logits, one evaluator per "
                           "checkpoint); the host matrix of --host_metrics keeps neither (drop one of the flags)")
    if sweep and args.threshold is not None:
        raise RuntimeError("--decoder_checkpoints searches every checkpoint's own threshold in its one pass; with --threshold there is "
                           "no search (drop one of the two flags)")
    if sweep:
        check_same_tag_count(sweep)
    if getattr(args, "single_pass", False) and args.threshold is not None:
        raise RuntimeError("--single_pass merges the threshold search and the evaluation into one pass; with --threshold there is no "
                           "search and the run is one pass already (drop one of the two flags)")
    if getattr(args, "per_class_thresholds", False) and args.threshold is not None:
        raise RuntimeError("--per_class_thresholds reports the metrics under the thresholds the search finds; with --threshold there "
                           "is no search (drop one of the two flags)")
    if world_size > 1 and not sharded:
        raise RuntimeError("vae_tagger_amd.evaluate runs in a single process unless --sharded is given: the metrics are accumulated on "
                           "one GPU (start it without torchrun / with WORLD_SIZE=1, or pass --sharded to merge the ranks' states)")


def checkpoint_tag_count(path):
    """The number of tags a decoder checkpoint scores: the rows of the classifier's last linear layer (the 2-D `classifier.<k>.weight`
    of the highest k), read on the host."""
    from .infer_full import load_state_dict_file
    heads = {}
    for k, v in load_state_dict_file(path).items():
        parts = k.split(".")
        if len(parts) == 3 and parts[0] == "classifier" and parts[2] == "weight" and parts[1].isdigit() and getattr(v, "ndim", 0) == 2:
            heads[int(parts[1])] = int(v.shape[0])
    if not heads:
        raise RuntimeError(f"{path}: no classifier.<k>.weight matrix found, cannot tell the number of tags")
    return heads[max(heads)]


def check_same_tag_count(paths, count=checkpoint_tag_count):
    """Refuse a sweep over checkpoints that score different numbers of tags (host only: before any GPU work)."""
    for p in paths:
        if not os.path.exists(p):
            raise RuntimeError(f"解码器模型文件不存在: {p}")
    counts = [count(p) for p in paths]
    if len(set(counts)) > 1:
        raise RuntimeError("--decoder_checkpoints: the checkpoints score different numbers of tags ("
                           + ", ".join(f"{os.path.basename(str(p))}: {c}" for p, c in zip(paths, counts)) + ")")
    return counts[0] if counts else None


def _load_sweep_decoders(args, decoder, device):
    """One decoder per checkpoint of --decoder_checkpoints, each with its own device context (the architecture of `decoder`)."""
    import copy
    from .infer_full import load_state_dict_file
    decoders = []
    for path in args.decoder_checkpoints:
        ctx, decoder._ctx = getattr(decoder, "_ctx", None), None      # the copy gets a device context of its own on first use
        try:
            d = copy.deepcopy(decoder).cpu()
        finally:
            decoder._ctx = ctx
        try:
            d.load_state_dict(load_state_dict_file(path), strict=False)
        except Exception as e:  # noqa: BLE001 - reference behaviour (load_models)
            raise RuntimeError(f"无法加载Decoder模型: {e}")
        decoders.append(d.to(device).eval())
    return decoders


def _run_val_loss(args, vae_model, decoder, tag_names, data, all_labels, loader, device, group, rank, per_class):
    """--val_loss / --decoder_checkpoints: the passes that go through evaluation.sweep_checkpoints.  Returns (threshold, optimal,
    metrics, per_class_metrics, passes, extra result keys)."""
    from .evaluation import find_optimal_threshold, sweep_checkpoints
    from .losses import class_balanced_weights, class_distribution, select_loss, sweep_dir_name, sweep_summary
    selected = select_loss(args.use_class_balanced, args.use_focal_loss)
    # class weights from the WHOLE JSON (every entry, as compute_class_distribution sees the dataset), before any sharding
    weights = class_balanced_weights(class_distribution(all_labels, len(tag_names)))
    kw = dict(group=group, focal_alpha=args.focal_alpha, focal_gamma=args.focal_gamma, class_weights=weights, selected_loss=selected)
    if args.decoder_checkpoints:
        decoders = _load_sweep_decoders(args, decoder, device)
        dirs = [os.path.join(args.output_dir, sweep_dir_name(i, p)) for i, p in enumerate(args.decoder_checkpoints)]
        if rank == 0:
            print(f"检查点扫描: {len(decoders)} 个解码器, 单次遍历...")
        results = sweep_checkpoints(vae_model, decoders, loader, tag_names, device, dirs, per_class=per_class, **kw)
        summary = sweep_summary([dict(r, path=p) for r, p in zip(results, args.decoder_checkpoints)], selected)
        if rank == 0:
            with open(os.path.join(args.output_dir, "checkpoint_sweep.json"), "w", encoding="utf-8") as fh:
                json.dump(summary, fh, indent=2, ensure_ascii=False)
            print(f"best_by_val_loss: {summary['best_by_val_loss']}  best_by_macro_f1: {summary['best_by_macro_f1']}")
        best = results[summary["best_by_val_loss"]["index"] if summary["best_by_val_loss"] else 0]
        return (best["optimal"]["global_threshold"], best["optimal"], best["metrics"], best["per_class_metrics"], 1,
                {"sweep": summary, "checkpoints": results, "validation_loss": best["loss"]})
    passes, optimal, threshold = 1, None, args.threshold
    if not args.single_pass and args.threshold is None:
        if rank == 0:
            print("寻找最优分类阈值...")
        optimal = find_optimal_threshold(vae_model, decoder, loader, tag_names, device, args.output_dir, device_metrics=True, group=group)
        threshold, passes = optimal["global_threshold"], 2
    if rank == 0:
        print("寻找最优分类阈值并进行最终评估 (单次遍历)..." if args.single_pass else "使用最优阈值进行最终评估...")
    r = sweep_checkpoints(vae_model, [decoder], loader, tag_names, device, [args.output_dir], threshold=None if args.single_pass else float(threshold),
                          per_class=per_class, per_class_thresholds=optimal if (per_class and not args.single_pass) else None, **kw)[0]
    if args.single_pass:
        optimal, threshold = r["optimal"], r["optimal"]["global_threshold"]
    return float(threshold), optimal, r["metrics"], r["per_class_metrics"], passes, {"validation_loss": r["loss"]}


def evaluate(args):
    import time
    from .evaluation import evaluate_and_search, evaluate_model, find_optimal_threshold
    from .infer_full import load_models
    from .pipeline import EncodeTagPipeline
    check_mode(args, int(os.environ.get("WORLD_SIZE", "1")))
    world, rank, dev_index, group = 1, 0, None, None
    if getattr(args, "sharded", False):
        from .infer_full import _dist_setup
        world, rank, dev_index = _dist_setup()           # creates the process group BEFORE any GPU call of this process
        if dev_index is not None:
            import torch.distributed as dist
            group = dist.group.WORLD
    if not torch.cuda.is_available():
        raise RuntimeError("vae_tagger_amd needs an MI355X (no HIP device visible; there is no CPU fallback)")
    if dev_index is not None:
        torch.cuda.set_device(dev_index)
    device = torch.device("cuda", torch.cuda.current_device())
    vae_model, decoder, tag_names = load_models(args, device)
    data = TaggedImageList(args.json_path, args.tags_csv_path)
    val_loss = bool(getattr(args, "val_loss", False) or getattr(args, "decoder_checkpoints", None))
    # every entry of the JSON, as the reference's compute_class_distribution sees the dataset (a missing file is still an entry there)
    all_labels = TaggedImageList(args.json_path, args.tags_csv_path, check_files=False).labels if val_loss else None
    if rank == 0:
        for p in data.missing:
            print(f"跳过图像 {p}，错误原因: 文件不存在")
    if not data.image_paths:
        raise RuntimeError(f"{args.json_path} 中没有可用的图像")
    if group is not None:
        data.image_paths = shard_paths(data.image_paths, rank, world)
    if args.fp8:
        vae_model.vae._context().call("vt_set_flag", 11, 1)
    elif args.fp16_operands:
        vae_model.vae.set_fp16_operands(True)
    pipe = EncodeTagPipeline.input_side(vae_model)
    loader = build_loader(args, pipe, data)
    device_metrics = not args.host_metrics
    os.makedirs(args.output_dir, exist_ok=True)
    t0 = time.perf_counter()
    passes = 0
    per_class = bool(getattr(args, "per_class_thresholds", False))
    per_class_metrics = None
    extra = {}
    if val_loss:
        threshold, optimal, metrics, per_class_metrics, passes, extra = _run_val_loss(args, vae_model, decoder, tag_names, data, all_labels,
                                                                                      loader, device, group, rank, per_class)
    elif getattr(args, "single_pass", False):
        if rank == 0:
            print("寻找最优分类阈值并进行最终评估 (单次遍历)...")
        optimal, metrics, per_class_metrics = evaluate_and_search(vae_model, decoder, loader, tag_names, device, args.output_dir,
                                                                  device_metrics=device_metrics, group=group, per_class=per_class)
        threshold = optimal["global_threshold"]
        passes += 1
    else:
        if args.threshold is None:
            if rank == 0:
                print("寻找最优分类阈值...")
            optimal = find_optimal_threshold(vae_model, decoder, loader, tag_names, device, args.output_dir, device_metrics=device_metrics,
                                             group=group)
            threshold = optimal["global_threshold"]          # with a group: rank 0's dict, broadcast -- the same threshold on every rank
            passes += 1
        else:
            optimal, threshold = None, float(args.threshold)
        if rank == 0:
            print("使用最优阈值进行最终评估...")
        metrics = evaluate_model(vae_model, decoder, loader, tag_names, device, threshold, args.output_dir, device_metrics=device_metrics,
                                 group=group, per_class_thresholds=optimal if per_class else None)
        if per_class:
            metrics, per_class_metrics = metrics
        passes += 1
    torch.cuda.synchronize()
    LAST_RUN_STATS.update(loop_seconds=time.perf_counter() - t0, images=sum(len(n) for n, _ in loader.batches), passes=passes,
                          batches=list(loader.batches))
    failed, images = [(p, str(e)) for p, e in loader.failed], LAST_RUN_STATS["images"]
    if group is not None:
        import torch.distributed as dist
        objs = [None] * world if rank == 0 else None
        dist.gather_object((failed, images), objs, dst=0, group=group)
        if rank != 0:
            return {"threshold": threshold, "optimal_thresholds": optimal, "metrics": metrics, "skipped": None,
                    **({"per_class_metrics": per_class_metrics} if per_class else {}), **extra}
        failed = [f for part, _ in objs for f in part]   # every file belongs to one rank: each failure is counted once
        images = sum(n for _, n in objs)
    for p, e in failed:
        print(f"跳过图像 {p}，错误原因: {e}")
    print(f"评估完成！图像: {images}, 跳过: {len(failed) + len(data.missing)}, 阈值: {threshold:.3f}")
    return {"threshold": threshold, "optimal_thresholds": optimal, "metrics": metrics, "skipped": len(failed) + len(data.missing),
            **({"per_class_metrics": per_class_metrics} if per_class else {}), **extra}


def build_parser(distributed=False, recount=False, val_loss=False):
    """The single-process flag set; distributed=True adds --sharded, recount=True the flags that rest on the device recount
    (--single_pass, --per_class_thresholds), val_loss=True the validation loss and the checkpoint sweep (--val_loss, the loss flags of
    train_decoder.py, --decoder_checkpoints).  `main` parses with all three."""
    p = argparse.ArgumentParser(description="在带标签的数据集上评估VAE + 分类解码器 (阈值搜索 + 多标签指标)。")
    p.add_argument("--vae_checkpoint", type=str, required=True, help="预训练VAE模型文件路径 (.safetensors)")
    p.add_argument("--vae_config_path", type=str, default=None, help="VAE配置文件路径 (JSON格式)")
    p.add_argument("--decoder_checkpoint", type=str, required=True, help="Decoder模型文件路径 (.bin/.pth)")
    p.add_argument("--json_path", type=str, required=True, help='{image path: "tag:weight, tag:weight"}')
    p.add_argument("--tags_csv_path", type=str, required=True, help="包含所有分类头的CSV文件")
    p.add_argument("--output_dir", type=str, default="decoder_output")
    p.add_argument("--resolution", type=int, default=1024)
    p.add_argument("--use_attention", action="store_true", default=True, help="启用注意力机制 (默认开启)")
    p.add_argument("--no_attention", action="store_true", help="禁用注意力机制")
    p.add_argument("--use_spatial_attention", action="store_true", default=True, help="启用空间注意力")
    p.add_argument("--use_self_attention", action="store_true", default=True, help="启用自注意力")
    p.add_argument("--use_cross_attention", action="store_true", help="启用交叉注意力")
    p.add_argument("--attention_heads", type=int, default=8, help="注意力头数")
    p.add_argument("--attention_dropout", type=float, default=0.1, help="注意力dropout率")
    p.add_argument("--use_bucketing", action="store_true", help="启用长宽比分桶功能")
    p.add_argument("--base_resolution", type=int, default=512, help="分桶的基础分辨率")
    p.add_argument("--max_resolution", type=int, default=1024, help="分桶的最大分辨率")
    p.add_argument("--bucket_step", type=int, default=64, help="分桶的步长")
    p.add_argument("--batch_size", type=int, default=8, help="images per device batch (one bucket per batch with --use_bucketing)")
    p.add_argument("--workers", type=int, default=0, help="image decode threads (0 = min(16, cores))")
    p.add_argument("--max_pending", type=int, default=0,
                   help="with --use_bucketing: images that may wait in partly filled buckets before the fullest one is sent short "
                        "(0 = 4 x batch_size)")
    p.add_argument("--host_resize", action="store_true",
                   help="the reference's own input route: PIL transforms on the CPU, fp32 tensors over PCIe (same files, slower)")
    p.add_argument("--fp16_operands", action="store_true", help="fp16 instead of bf16 MFMA operands for the convolutions")
    p.add_argument("--fp8", action="store_true", help="3x3 convs of the encoder on fp8 (e4m3) operands")
    p.add_argument("--host_metrics", action="store_true",
                   help="accumulate the metrics on the host (the probabilities of every batch are copied back) instead of on the GPU")
    p.add_argument("--threshold", type=float, default=None,
                   help="skip the threshold search and evaluate at this threshold: ONE pass over the images instead of two "
                        "(search pass + metrics pass at the threshold found)")
    if recount:
        p.add_argument("--single_pass", action="store_true",
                       help="threshold search and evaluation in ONE pass over the images: the metrics at the threshold found are recounted "
                            "on the GPU from the evaluator's stored keys (same files as the two-pass run; not with --threshold)")
        p.add_argument("--per_class_thresholds", action="store_true",
                       help="also report the metrics under the searched per-class thresholds and write them as "
                            "evaluation_results_per_class_thresholds.csv / _overall.json (no extra pass over the images; not with --threshold)")
    if val_loss:
        p.add_argument("--val_loss", action="store_true",
                       help="also report the validation loss train_decoder.py selects checkpoints by -- BCE-with-logits, Focal and "
                            "class-balanced BCE, accumulated on the GPU from the logits -- and write validation_loss.json "
                            "(not with --host_metrics)")
        p.add_argument("--use_focal_loss", action="store_true", help="使用Focal Loss处理类别不平衡 (selects the loss reported as val_loss)")
        p.add_argument("--use_class_balanced", action="store_true", help="使用类别平衡损失 (selects the loss reported as val_loss)")
        p.add_argument("--focal_alpha", type=float, default=1.0, help="Focal Loss的alpha参数")
        p.add_argument("--focal_gamma", type=float, default=2.0, help="Focal Loss的gamma参数")
        p.add_argument("--decoder_checkpoints", type=str, nargs="+", default=None,
                       help="checkpoint sweep: score these decoder checkpoints (one architecture, one tag count) in ONE pass -- every "
                            "image is encoded once; implies --single_pass and --val_loss; files go to output_dir/ckpt_<index>_<stem>/ "
                            "and output_dir/checkpoint_sweep.json (not with --threshold or --host_metrics).  --decoder_checkpoint stays "
                            "required and names the architecture's checkpoint.  Memory: every checkpoint keeps its own key store of "
                            "tags x images x 8 bytes on the GPU -- 655 MB at 10 000 tags x 8 192 images, about 6.6 GB for ten checkpoints")
    if distributed:
        p.add_argument("--sharded", action="store_true",
                       help="under torchrun: one rank per GPU, rank r evaluates paths[r::world], the device evaluator's states are "
                            "merged on rank 0, which writes the files (not with --host_metrics)")
    return p


def main(argv=None):
    args = build_parser(distributed=True, recount=True, val_loss=True).parse_args(argv)
    if args.no_attention:
        args.use_attention = False
    if args.decoder_checkpoints:
        args.single_pass = args.val_loss = True
    return evaluate(args)


if __name__ == "__main__":
    main()
