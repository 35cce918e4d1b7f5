"""Counterpart of the reference's infer_full.py (same flags, same classification_results.json schema,
same skip-and-count behaviour), running encode+tag on MI355X through libvae_tagger_hip.so.

    python -m vae_tagger_amd.infer_full --vae_checkpoint ae.safetensors --decoder_checkpoint dec.pth \
        --image_path imgs/ --tags_csv_path tags.csv [--batch_size 8]

Differences from the reference, all outside the numbers it writes (`--fp8` is the exception: an opt-in faster mode whose logits
stay within 1e-2 of the default path's):
  * images are processed in same-shape batches (`--batch_size`, new flag; the reference runs one at a time), PIPELINED: a thread pool
    decodes files ahead, a side stream uploads uint8 pixels and resizes / normalises them on the GPU (Pillow's arithmetic, bit for bit)
    while the previous batch is in the encoder, and a batch's results are read after the next one has been enqueued (prefetch.py);
    `--host_resize` is the reference's CPU transform route, `--serial` its one-at-a-time loop shape -- the JSON is the same either way;
  * under `torchrun` (WORLD_SIZE > 1) the image list is sharded over the ranks (one GPU each) and rank 0 writes the merged file;
  * sigmoid + sort run on the device and come back in one copy per batch (the reference does 2*N .item() syncs
    per image, infer_full.py:109-111);
  * checkpoints are read with tensor-only loaders (safetensors / torch.load(weights_only=True)).
Reference: infer_full.py:16-71 (load_models), :73-141 (infer_and_classify), :143-186 (flags).
"""
import argparse
import contextlib
import json
import os
from pathlib import Path

import torch

from .diffusers_vae_loader import (DiffusersVAEWrapper, create_vae_from_config_file, get_diffusers_vae_config,
                                   load_diffusers_vae_from_config)
from .modules import (ClassificationDecoder, create_attention_decoder, get_image_paths, get_image_transform,
                      get_vae_latent_info)
from ._lib import VT_STATUS_FP8_SATURATED, VT_STATUS_NONFINITE
from .pipeline import EncodeTagPipeline


def load_state_dict_file(path):
    if str(path).endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(str(path))
    return torch.load(path, map_location="cpu", weights_only=True)


def load_models(args, device="cuda"):
    if args.vae_config_path and os.path.exists(args.vae_config_path):
        print(f"从配置文件创建VAE: {args.vae_config_path}")
        vae_model = create_vae_from_config_file(args.vae_config_path, args.vae_checkpoint)
    elif args.vae_checkpoint and os.path.exists(args.vae_checkpoint):
        print(f"直接加载预训练VAE模型: {args.vae_checkpoint}")
        vae_model = DiffusersVAEWrapper(load_diffusers_vae_from_config(get_diffusers_vae_config(), args.vae_checkpoint))
    else:
        raise RuntimeError("必须提供 VAE 模型检查点或配置文件")
    vae_model.to(device)
    vae_model.eval()
    latent_info = get_vae_latent_info(args.resolution)
    print(f"VAE潜在空间信息: {latent_info}")
    import pandas as pd
    tags_df = pd.read_csv(args.tags_csv_path)
    num_classes = len(tags_df)
    if args.use_attention:
        print("使用注意力分类解码器")
        decoder = create_attention_decoder(
            latent_channels=latent_info["latent_channels"], latent_height=latent_info["latent_height"],
            latent_width=latent_info["latent_width"], num_classes=num_classes,
            attention_config={"use_spatial_attention": getattr(args, "use_spatial_attention", True),
                              "use_self_attention": getattr(args, "use_self_attention", True),
                              "use_cross_attention": getattr(args, "use_cross_attention", False),
                              "attention_heads": getattr(args, "attention_heads", 8),
                              "attention_dropout": getattr(args, "attention_dropout", 0.1)})
    else:
        print("使用标准分类解码器")
        decoder = ClassificationDecoder(latent_info["latent_channels"], latent_info["latent_height"],
                                        latent_info["latent_width"], num_classes, use_adaptive_pooling=True)
    if not os.path.exists(args.decoder_checkpoint):
        raise RuntimeError(f"解码器模型文件不存在: {args.decoder_checkpoint}")
    try:
        decoder.load_state_dict(load_state_dict_file(args.decoder_checkpoint), strict=False)
        print(f"成功加载Decoder模型: {args.decoder_checkpoint}")
    except Exception as e:  # noqa: BLE001 - reference behaviour
        raise RuntimeError(f"无法加载Decoder模型: {e}")
    decoder.to(device)
    decoder.eval()
    return vae_model, decoder, tags_df["name"].tolist()


LAST_RUN_STATS = {}   # filled by infer_and_classify: seconds spent in the image loop of this rank and its image count (tools/bench_cli.py reads it)
TOP_K = 64          # (confidence, tag) pairs fetched per image with the summary; images with more tags above the threshold fetch their prefix


def summarize(conf_row, idx_row, tag_names, threshold):
    """One image's JSON entry from its sorted confidences / indices on the host (infer_full.py:106-125) -- the reference
    formulation; the CLI uses `summarize_batch`, which takes the same numbers from the device-side summary."""
    predicted = []
    for c, i in zip(conf_row, idx_row):
        c = float(c)
        if c < threshold:
            break                                   # sorted descending: nothing further passes
        predicted.append({"tag": tag_names[int(i)], "confidence": float(f"{c:.4f}")})
    top5 = [float(c) for c in conf_row[:5]]
    return {"predicted_tags": predicted, "total_tags_above_threshold": len(predicted),
            "max_confidence": float(f"{float(conf_row[0]):.4f}"),
            "avg_confidence_top5": float(f"{sum(top5) / 5:.4f}")}      # always divides by 5, like the reference


def summarize_per_class(conf_row, idx_row, tag_names, thresholds):
    """`summarize` with one threshold per tag (`thresholds[i]` for tag i): a tag passes when its confidence >= its own threshold, so a
    lower-ranked tag may pass where a higher-ranked one does not; the whole sorted list is looked at.  The host reference of
    vt_summarize_confidence_per_class."""
    predicted = []
    for c, i in zip(conf_row, idx_row):
        c = float(c)
        if c >= float(thresholds[int(i)]):          # (a NaN confidence fails the test)
            predicted.append({"tag": tag_names[int(i)], "confidence": float(f"{c:.4f}")})
    top5 = [float(c) for c in conf_row[:5]]
    return {"predicted_tags": predicted, "total_tags_above_threshold": len(predicted),
            "max_confidence": float(f"{float(conf_row[0]):.4f}"),
            "avg_confidence_top5": float(f"{sum(top5) / 5:.4f}")}


def load_class_thresholds(path, tag_names, default):
    """fp32 [N] from the `per_class_thresholds` of an optimal_thresholds.json (what the threshold search of vae_tagger_amd.evaluate, or
    the reference's find_optimal_threshold, writes); a tag the file does not name uses `default` (--confidence_threshold)."""
    import numpy as np
    from .evaluation import threshold_vector
    with open(path, "r", encoding="utf-8") as fh:
        data = json.load(fh)
    if not isinstance(data, dict) or not isinstance(data.get("per_class_thresholds"), dict):
        raise ValueError(f"{path}: no per_class_thresholds mapping (expected the optimal_thresholds.json of a threshold search)")
    return threshold_vector(data["per_class_thresholds"], tag_names, default).astype(np.float32)


def _entries_from_summary(summary, conf, idx, tag_names, copy_stream=None, class_thresholds=None):
    """JSON entries from the host arrays of the device-side summary (formatting only).  Raises FloatingPointError on non-finite confidences.
    `class_thresholds`: the host fp32 [N] copy of the per-tag thresholds the summary was taken under (None: one scalar threshold).
    `copy_stream`: the stream a longer prefix is fetched on (the pipelined loop passes one of its own, so that the copy of batch n's finished
    arrays does not queue behind batch n + 1's kernels on the compute stream)."""
    top_conf, top_idx, stats = summary
    out = []
    for b in range(stats.shape[0]):
        count, mx, avg5, bad = int(stats[b, 0]), float(stats[b, 1]), float(stats[b, 2]), int(stats[b, 3])
        if bad:
            raise FloatingPointError(f"{bad} non-finite confidences: activations left the fp16 range of the residual stream "
                                     "or the checkpoint holds inf / NaN")
        if count <= top_conf.shape[1]:
            cs, ix = top_conf[b, :count], top_idx[b, :count]
        elif class_thresholds is not None:          # rare, per-tag thresholds: the passing tags are no prefix -- the whole row, filtered here
            with torch.cuda.stream(copy_stream) if copy_stream is not None else contextlib.nullcontext():
                cs, ix = conf[b].cpu().numpy(), idx[b].cpu().numpy()
            keep = cs >= class_thresholds[ix]
            cs, ix = cs[keep], ix[keep]
        else:                                       # rare: more tags above the threshold than the summary carries
            with torch.cuda.stream(copy_stream) if copy_stream is not None else contextlib.nullcontext():
                cs, ix = conf[b, :count].cpu().numpy(), idx[b, :count].cpu().numpy()
        predicted = [{"tag": tag_names[int(i)], "confidence": float(f"{float(c):.4f}")} for c, i in zip(cs, ix)]
        out.append({"predicted_tags": predicted, "total_tags_above_threshold": count,
                    "max_confidence": float(f"{mx:.4f}"), "avg_confidence_top5": float(f"{avg5:.4f}")})
    return out


def summarize_batch(pipe, conf, idx, tag_names, threshold, top_k=TOP_K, class_thresholds=None):
    """conf / idx: sorted device tensors [B,N] (pipe.tag).  Threshold count, top-k, max and top-5 mean come from the
    device (vt_summarize_confidence): formatting only on the host.  Raises FloatingPointError on non-finite confidences.
    `threshold` may be a device fp32 [N] tensor of per-tag thresholds; `class_thresholds` is then its host copy (numpy)."""
    return _entries_from_summary(pipe.summarize(conf, idx, threshold, top_k), conf, idx, tag_names, class_thresholds=class_thresholds)


def _dist_setup():
    """(world, rank, device index).  Under torchrun (WORLD_SIZE > 1) the process group is created here, BEFORE any GPU call of this
    process: "nccl" (= RCCL) with one GPU per rank, "gloo" when the ranks have to share GPUs (a rehearsal on a one-GPU box,
    VT_CLI_GLOO=1).  The image list is split by `sharding.shard_range`; the only exchange is a gather of the finished entries.
    VT_CLI_ONE_RANK_GROUP=1 creates the (RCCL) group even for ONE rank, so that the object collectives of the sharded path -- list
    broadcast, fp8-abandoned all-reduce, result gather -- execute on the real backend on a one-GPU box."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    one_rank_group = world <= 1 and os.environ.get("VT_CLI_ONE_RANK_GROUP") == "1"
    if world <= 1 and not one_rank_group:
        return 1, 0, None
    import torch.distributed as dist
    rank, local = int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    ngpu = torch.cuda.device_count()                       # (counting devices does not initialise the GPU)
    if ngpu < 1:
        raise RuntimeError("vae_tagger_amd needs an MI355X (no HIP device visible; there is no CPU fallback)")
    gloo = os.environ.get("VT_CLI_GLOO") == "1" or ngpu < int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if not dist.is_initialized():
        if gloo:
            dist.init_process_group("gloo", world_size=max(world, 1), rank=rank)
        else:
            dist.init_process_group("nccl", world_size=max(world, 1), rank=rank, device_id=torch.device("cuda", local % ngpu))
    return max(world, 1), rank, local % ngpu


def _grouped():
    """A process group exists (torchrun, or the one-rank rehearsal): the sharded path's collectives run."""
    import torch.distributed as dist
    return dist.is_available() and dist.is_initialized()


def gather_results(items, processed, errors, world, rank):
    """Rank 0 receives every rank's [(path, entry)] and counters (torch.distributed.gather_object); the others get (None, 0, 0)."""
    if world == 1 and not _grouped():
        return items, processed, errors
    import torch.distributed as dist
    objs = [None] * world if rank == 0 else None
    dist.gather_object((items, processed, errors), objs, dst=0)
    if rank != 0:
        return None, 0, 0
    merged = [it for part in objs for it in part[0]]
    return merged, sum(part[1] for part in objs), sum(part[2] for part in objs)


class _Tagger:
    """The device leg of the loop: one batch -> JSON entries, with the health word's fall-backs (fp16 -> fp32 residual storage, fp8 -> bf16) and the
    reference's error granularity (a failure costs ONE image: infer_full.py:130-132)."""

    def __init__(self, pipe, tag_names, threshold, fp8, f16=False, class_thresholds=None):
        self.pipe, self.tag_names, self.thr = pipe, tag_names, threshold
        self.class_thr = None           # per-tag thresholds (host fp32 [N]); uploaded once, self.thr is then the device vector
        if class_thresholds is not None:
            import numpy as np
            self.class_thr = np.ascontiguousarray(class_thresholds, dtype=np.float32)
            if self.class_thr.shape != (len(tag_names),):
                raise ValueError(f"expected {len(tag_names)} per-tag thresholds, got shape {self.class_thr.shape}")
            self.thr = torch.from_numpy(self.class_thr).to(pipe.device)
        self.f16 = bool(f16)            # fp16 instead of bf16 conv operands (vt_set_flag 18): values must fit fp16
        self.fp8 = bool(fp8)            # current numeric mode of the context
        self.fp32_res = False
        self.epoch = 0                  # bumped by every permanent mode switch: batches enqueued before it are redone
        self.copy_stream = torch.cuda.Stream(device=pipe.device)
        if self.fp8:
            pipe.set_fp8(True)

    def _run(self, x):
        conf, idx = self.pipe.tag(x)
        return conf, idx, self.pipe.status()

    def tag_batch(self, x):
        """Synchronous: one device batch -> (entries, fp8 mode they were computed in).  A raised health word is resolved here:
          * bad INPUT (NaN / inf pixels) raises bit 0 whatever the storage -- and in fp8 mode bit 1 as well, because the e4m3 conversion
            clamps a NaN to +-448 and counts it as a clamp: if the batch is still non-finite on the most conservative setting (bf16
            operands, fp32 residual storage) it is the input, every setting is restored and the caller skips the image;
          * otherwise the switch that cured it is permanent (a property of the checkpoint): fp32 residual storage for bit 0, and
            bf16 operands if fp8 mode still clamps with it."""
        pipe = self.pipe
        conf, idx, st = self._run(x)
        if st:
            was_fp8, was_res = self.fp8, self.fp32_res
            if st & VT_STATUS_NONFINITE or (st & VT_STATUS_FP8_SATURATED and not was_fp8):
                pipe.set_fp8(False); pipe.set_fp32_residual(True); pipe.set_fp16_operands(False)
                conf, idx, st2 = self._run(x)
                if st2 & VT_STATUS_NONFINITE:
                    pipe.set_fp8(was_fp8); pipe.set_fp32_residual(was_res); pipe.set_fp16_operands(self.f16)   # not the checkpoint: one bad image must not change the run
                    raise FloatingPointError("non-finite activations even with bf16 operands and fp32 residual storage (inf / NaN pixels or weights?)")
                print("警告: 激活值超出fp16范围，改用fp32残差存储" + ("和bf16卷积操作数" if self.f16 else "") + "重新计算该批次")
                self.fp32_res = True
                self.f16 = False            # (an overflow of the fp16 storage is an overflow of fp16 operands too: the precision mode ends with it)
                self.epoch += 1
                if was_fp8:
                    pipe.set_fp8(True)
                    c8, i8, st8 = self._run(x)
                    if st8 == 0:
                        conf, idx = c8, i8
                    else:
                        pipe.set_fp8(False)
                        print("警告: 激活值超出fp8(e4m3)范围，改用bf16路径")
                        self.fp8 = False
            else:
                # fp8 mode and this checkpoint's activations exceed the e4m3 range: the clamped values are not worth tags; bf16 from here on
                print("警告: 激活值超出fp8(e4m3)范围，改用bf16路径重新计算该批次")
                pipe.set_fp8(False)
                self.fp8 = False
                self.epoch += 1
                conf, idx, st2 = self._run(x)
                if st2 & VT_STATUS_NONFINITE:
                    pipe.set_fp32_residual(True)
                    conf, idx, st3 = self._run(x)
                    if st3 & VT_STATUS_NONFINITE:
                        pipe.set_fp32_residual(self.fp32_res)
                        raise FloatingPointError("non-finite activations even with fp32 residual storage (inf / NaN pixels or weights?)")
                    print("警告: 激活值超出fp16范围，改用fp32残差存储")
                    self.fp32_res = True
        return summarize_batch(pipe, conf, idx, self.tag_names, self.thr, class_thresholds=self.class_thr), self.fp8

    def clear_status(self):
        try:
            self.pipe.status(clear=True)                 # the sticky word must not leak into the next healthy batch
        except Exception:  # noqa: BLE001
            pass

    def device_leg(self, x, names):
        """Tag one batch synchronously; when the batch fails, retry it image by image so that an error costs ONE image, as in the
        reference's per-image loop (infer_full.py:130-132).  Returns [(path, entry, fp8 mode of the entry)] and the number of images lost."""
        try:
            entries, f8 = self.tag_batch(x)
            return [(p, e, f8) for p, e in zip(names, entries)], 0
        except Exception as e:  # noqa: BLE001
            self.clear_status()
            if len(names) == 1:
                print(f"跳过图像 {names[0]}，错误原因: {e}")
                return [], 1
        done, lost = [], 0
        for k, p in enumerate(names):
            try:
                entries, f8 = self.tag_batch(x[k:k + 1])
                done.append((p, entries[0], f8))
            except Exception as e:  # noqa: BLE001 - skip-and-count (infer_full.py:130-132)
                self.clear_status()
                lost += 1
                print(f"跳过图像 {p}，错误原因: {e}")
        return done, lost

    # ---- pipelined form: enqueue batch n, read its word and summary while batch n + 1 runs ----
    def enqueue(self, x, names):
        pipe = self.pipe
        rec = {"x": x, "names": names, "epoch": self.epoch, "fp8": self.fp8, "ok": False}
        try:
            conf, idx = pipe.tag(x)
            host, K = pipe.summarize_async(conf, idx, self.thr, TOP_K)
            word = torch.empty(1, dtype=torch.int32, pin_memory=True)
            pipe.status_async(word)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(pipe.device))
            rec.update(conf=conf, idx=idx, host=host, K=K, word=word, ev=ev, ok=True)
        except Exception as e:  # noqa: BLE001 - resolved by the synchronous leg in finish()
            rec["error"] = e
        return rec

    def finish(self, rec):
        """-> ([(path, entry, fp8 mode)], images lost).  The fast path only formats; anything unusual -- a raised word, a failed call, non-finite
        confidences, a mode switch since the batch was enqueued -- goes through the synchronous leg on the same device tensor."""
        if rec["ok"]:
            rec["ev"].synchronize()
            if rec["epoch"] == self.epoch and int(rec["word"][0]) == 0:
                try:
                    # (the event has passed: conf / idx are final, so a longer prefix can be copied on a stream that does not wait for batch n + 1)
                    entries = _entries_from_summary(self.pipe.unpack_summary(rec["host"], rec["K"]), rec["conf"], rec["idx"], self.tag_names,
                                                    self.copy_stream, self.class_thr)
                    return [(p, e, rec["fp8"]) for p, e in zip(rec["names"], entries)], 0
                except Exception:  # noqa: BLE001
                    pass
        return self.device_leg(rec["x"], rec["names"])


def infer_and_classify(args):
    world, rank, dev_index = _dist_setup()
    if not torch.cuda.is_available():
        raise RuntimeError("vae_tagger_amd needs an MI355X (no HIP device visible; there is no CPU fallback)")
    device = "cuda" if dev_index is None else f"cuda:{dev_index}"
    if dev_index is not None:
        torch.cuda.set_device(dev_index)
    print(f"Using device: {device}")
    vae_model, decoder, tag_names = load_models(args, device)
    transform = get_image_transform(args.resolution)
    if not os.path.exists(args.image_path):
        raise FileNotFoundError(f"图像路径未找到: {args.image_path}")
    image_paths = get_image_paths(args.image_path)
    if _grouped():
        import torch.distributed as dist
        box = [image_paths]                              # the reference's order is a set's: every rank works from rank 0's list
        dist.broadcast_object_list(box, src=0)
        image_paths = box[0]
    if not image_paths:
        print("未找到任何图像文件，请检查路径。")
        return
    from . import sharding
    from .prefetch import BatchFeeder
    lo, hi = sharding.shard_range(len(image_paths), rank, world)
    my_paths = image_paths[lo:hi]
    pipe = EncodeTagPipeline(vae_model, decoder)
    pipe.check_finite = False                 # the batches' health words are read in stream order (status_async), one batch late
    f16 = bool(getattr(args, "fp16_operands", False)) and not getattr(args, "fp8", False)
    if f16:
        pipe.set_fp16_operands(True)
    class_thr = None
    if getattr(args, "thresholds_json", None):
        class_thr = load_class_thresholds(args.thresholds_json, tag_names, args.confidence_threshold)
        print(f"使用每个标签各自的阈值: {args.thresholds_json}")
    tg = _Tagger(pipe, tag_names, args.confidence_threshold, getattr(args, "fp8", False), f16, class_thresholds=class_thr)
    bs = max(1, int(getattr(args, "batch_size", 8)))
    host_resize = bool(getattr(args, "host_resize", False))
    serial = bool(getattr(args, "serial", False))
    results, entry_fp8 = {}, {}
    counts = {"processed": 0, "errors": 0}
    main = torch.cuda.current_stream(pipe.device)

    def take(done, lost):
        counts["errors"] += lost
        for p, entry, f8 in done:
            if str(p) not in results:
                counts["processed"] += 1
            results[str(p)] = entry
            entry_fp8[str(p)] = f8

    def run(paths, progress=True):
        """paths -> entries, pipelined: the decode pool and the side stream build batch n + 1 while batch n is in the encoder, and batch n's
        health word + summary are read after batch n + 1 has been enqueued (`--serial`: one batch at a time, as the reference's loop)."""
        from collections import deque
        inflight, seen = deque(), 0
        feeder = BatchFeeder(pipe, paths, bs, args.resolution, workers=getattr(args, "workers", None) or None,
                             host_resize=host_resize, transform=transform)
        for names, x, ready, failed in feeder:
            for p, e in failed:
                counts["errors"] += 1
                print(f"跳过图像 {p}，错误原因: {e}")
            if names:
                main.wait_event(ready)
                x.record_stream(main)
                inflight.append(tg.enqueue(x, names))
            while len(inflight) > (0 if serial else 1):
                take(*tg.finish(inflight.popleft()))
            seen += len(names) + len(failed)
            if progress and (seen // bs) % max(1, 100 // bs) == 0:
                print(f"已处理 {counts['processed']}/{len(paths)} 图像 (跳过 {counts['errors']} 个错误)")
        while inflight:
            take(*tg.finish(inflight.popleft()))

    import time
    t_loop = time.perf_counter()
    run(my_paths)
    torch.cuda.synchronize()
    LAST_RUN_STATS.update(loop_seconds=time.perf_counter() - t_loop, images=len(my_paths), rank=rank, world=world)
    # ONE output file holds ONE numeric mode: if fp8 was abandoned anywhere (on any rank), the entries computed in fp8 mode are redone in bf16
    fp8_asked = bool(getattr(args, "fp8", False))
    abandoned = fp8_asked and not tg.fp8
    if _grouped() and fp8_asked:
        import torch.distributed as dist
        flag = torch.tensor([1 if abandoned else 0], dtype=torch.int32, device="cpu" if dist.get_backend() == "gloo" else device)
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        abandoned = bool(int(flag.item()))
        if abandoned and tg.fp8:
            pipe.set_fp8(False); tg.fp8 = False; tg.epoch += 1
    if abandoned:
        redo = [p for p in my_paths if entry_fp8.get(str(p))]
        if redo:
            print(f"重新以bf16计算之前的 {len(redo)} 张图像")
            for p in redo:
                results.pop(str(p), None)
            counts["processed"] -= len(redo)             # take() counts them again as they come back; images lost in the redo count as errors
            run(redo, progress=False)
    items = [(str(p), results[str(p)]) for p in my_paths if str(p) in results]
    items, processed, errors = gather_results(items, counts["processed"], counts["errors"], world, rank)
    if rank != 0:
        return None
    results = dict(items)
    print(f"处理完成！成功: {processed}, 失败: {errors}, 总计: {len(image_paths)}")
    out = Path(args.output_dir) / "classification_results.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "w") as f:
        json.dump(results, f, indent=4, ensure_ascii=False)
    print(f"分类结果已保存到: {out}")
    return results


def build_parser(per_class=False):
    """per_class=True (what `main` parses with) adds --thresholds_json."""
    p = argparse.ArgumentParser(description="使用VAE和分类解码器进行图像分类。")
    p.add_argument("--vae_checkpoint", type=str, required=True, help="预训练VAE模型文件路径 (.safetensors)")
    p.add_argument("--vae_config_path", type=str, default=None, help="VAE配置文件路径 (JSON格式)")
    p.add_argument("--decoder_checkpoint", type=str, required=True, help="Decoder模型文件路径 (.bin/.pth)")
    p.add_argument("--image_path", type=str, required=True, help="单个图像文件或包含图像的目录")
    p.add_argument("--tags_csv_path", type=str, required=True, help="包含所有分类头的CSV文件")
    p.add_argument("--output_dir", type=str, default="inference_output", help="结果保存目录")
    p.add_argument("--resolution", type=int, default=1024, help="模型训练时的分辨率")
    p.add_argument("--confidence_threshold", type=float, default=0.5, help="置信度阈值")
    if per_class:
        p.add_argument("--thresholds_json", type=str, default=None,
                       help="optimal_thresholds.json of a threshold search: every tag is decided at its own per_class_thresholds entry "
                            "(confidence >= threshold); tags the file does not name use --confidence_threshold (not in the reference)")
    p.add_argument("--use_attention", action="store_true", default=True, help="使用注意力机制 (默认开启)")
    p.add_argument("--no_attention", action="store_true", help="禁用注意力机制")
    p.add_argument("--use_spatial_attention", action="store_true", default=True, help="启用空间注意力")
    p.add_argument("--use_self_attention", action="store_true", default=True, help="启用自注意力")
    p.add_argument("--use_cross_attention", action="store_true", help="启用交叉注意力")
    p.add_argument("--attention_heads", type=int, default=8, help="注意力头数")
    p.add_argument("--attention_dropout", type=float, default=0.1, help="注意力dropout率")
    p.add_argument("--model_checkpoint", type=str, default=None, help="(已弃用) 包含VAE和Decoder权重的父目录")
    p.add_argument("--batch_size", type=int, default=8, help="images per device batch (not in the reference)")
    p.add_argument("--device_resize", action="store_true",
                   help="resize + normalise on the GPU (bit-exact with the PIL transform; not in the reference).  This is the default since the "
                        "pipelined loader: the flag is accepted and changes nothing")
    p.add_argument("--host_resize", action="store_true",
                   help="the reference's own route: PIL Resize + ToTensor + Normalize on the CPU, fp32 tensors over PCIe (same JSON, slower)")
    p.add_argument("--workers", type=int, default=0, help="image decode threads (0 = min(16, cores); not in the reference)")
    p.add_argument("--serial", action="store_true",
                   help="one batch at a time: wait for batch n's results before batch n + 1 is enqueued (the reference's loop shape; same JSON)")
    p.add_argument("--fp16_operands", action="store_true",
                   help="fp16 instead of bf16 MFMA operands for the convolutions: latents ~6x closer to the fp32 reference (smooth pictures stay "
                        "inside 1e-2), ~4 %% slower (not in the reference)")
    p.add_argument("--fp8", action="store_true",
                   help="3x3 convs of the encoder on fp8 (e4m3) operands / the fp8 MFMA: ~1.35x faster, logits within 1e-2 of the "
                        "bf16 path's reference, latents only to ~1e-1 (tagging only; not in the reference)")
    return p


def main(argv=None):
    args = build_parser(per_class=True).parse_args(argv)
    if args.no_attention:
        args.use_attention = False
    if args.model_checkpoint and (not args.vae_checkpoint or not args.decoder_checkpoint):
        print("使用向后兼容模式，从model_checkpoint参数推导VAE和Decoder路径")
        args.vae_checkpoint = args.model_checkpoint
        args.decoder_checkpoint = args.model_checkpoint
    return infer_and_classify(args)


if __name__ == "__main__":
    main()
