"""Decoder training CLI: the reference's train_decoder.py (train_decoder.py:30-278) with the decoder trained on the GPU behind the
frozen encoder: the classifier head alone (train.HeadTrainer) or, with --train_front, the whole attention decoder (train.DecoderTrainer),
cross-attention included under --train_cross_attention.

    python -m vae_tagger_amd.train_decoder --vae_checkpoint ae.safetensors --json_path data.json --tags_csv_path tags.csv \
        --no_attention --num_epochs 10 --train_batch_size 16 [--use_bucketing] [--decoder_checkpoint start.bin]

--no_attention trains ClassificationDecoder in full (its front is the parameter-free 4x4 pool).  An attention decoder needs one of
two flags.  --freeze_front: its front (spatial attention, feature_compress, self- / cross-attention) runs as in inference and only
`classifier.*` changes -- e.g. to adapt a trained checkpoint to a new tag list.  --train_front: the front is trained too, from scratch
if no checkpoint is given: spatial_attention.*, feature_compress.* (BatchNorm on batch statistics, its running statistics updated) and
self_attention_post.* with --attention_dropout on the softmax weights; validation runs the front in eval mode on the running
statistics, as the reference's decoder.eval() does.  The channel max of the spatial attention passes its gradient to the arg-max
channel, the lowest index on a tie.  With --use_cross_attention, --train_front needs --train_cross_attention as well: query_generator.*
and cross_attention.* are then trained too (train.CrossTrainer) and the decoder is trained in full; without the flag the combination
stays refused, with a message that names it.  (The refusal is a pinned behaviour of this CLI; folding --train_cross_attention into
--use_cross_attention under --train_front is a later change that may edit the test that pins it.)
Epoch 1 encodes every image once and keeps the front's feature row and the labels of each on the GPU (train.FeatureCache); later epochs
train from that cache without calling the encoder (--no_feature_cache re-encodes every epoch).  The dataset applies no random
augmentation (modules.py:688-729), so a cached row is what a re-encode would give.  With --train_front the feature rows change every
step, so the encoder's LATENTS are cached instead (train.LatentCache: one flat fp32 arena, 16 (resolution / 8)^2 floats per image, 1 MB at
1024 x 1024): if that bound for all training and validation images plus their labels exceeds --latent_cache_gb (default 16), nothing is
cached and every epoch re-encodes; train_report.json records which happened and the bytes used.  Epochs from the cache form their
batches from the epoch's order grouped by latent shape (batch statistics need one shape per batch).
Files, as the reference writes them: best_pytorch_model.bin (strictly lower validation loss), pytorch_model.bin (every --save_steps
epochs), training_history.json, then the threshold search and the metrics on the validation set (optimal_thresholds.json,
evaluation_results.csv, evaluation_results_overall.json); plus train_report.json (per epoch: seconds, images/s, encoder batches, steps).

    torchrun --nproc-per-node 8 -m vae_tagger_amd.train_decoder ... --sharded

trains data-parallel, one rank per GPU.  Ownership is static: rank r owns train_paths[r::world] and val_paths[r::world], encodes its
share once into a cache sized for that share alone (so K ranks cache K times the data set one --latent_cache_gb allows), shuffles it
with epoch_order(len(share), seed, epoch) and forms its batches locally (with --train_front grouped by latent shape).  The ranks agree
once per epoch on the number of steps, the largest local batch count; a step is forward_backward -> the gradient exchange
(train.GradientExchange: one all-gather, then every rank merges the rows in rank order at weights n_r / sum n, so the merged gradient
is the concatenated batch's and every rank's parameters and Adam moments stay bit-identical without a broadcast) -> clip -> step; a
rank that has run out of batches joins with zero gradients at weight 0.  The learning-rate schedule counts these global steps.
Rank r's trainer seed is seed + 1000003 r (other dropout masks); BatchNorm runs on each rank's own batch statistics, and rank 0's
running statistics are written on every rank before each validation (what DDP's broadcast_buffers amounts to).  Every rank scores
its validation share; the loss blocks are gathered and merged in rank order on rank 0 (the checkpoint sweep's path), which computes
val_loss and broadcasts it; train_loss is the mean over all ranks' step losses.  Rank 0 alone prints the progress lines and writes the
files; the final evaluation is the sharded pass of `evaluate --sharded`; train_report.json gains "sharded" (world, backend, steps per
epoch, per-rank images, cache bytes and a SHA-256 over each rank's parameters and Adam moments).  Refused, before any GPU or
process-group work: --sharded with --gradient_accumulation_steps > 1 or --no_feature_cache, and a split that leaves a rank fewer than 2
training images or no validation image.  Without --sharded nothing changes, under torchrun included.
"""
import argparse
import json
import os
import time

import torch

IGNORED_ARGUMENTS = ("mixed_precision", "cudnn_benchmark", "cudnn_deterministic", "num_workers", "prefetch_factor", "use_safetensors")
FRONT_MESSAGE = ("an attention decoder needs --freeze_front or --train_front: training the decoder front without a choice between them is "
                 "not implemented; --freeze_front trains classifier.* on the frozen front, --no_attention trains the plain decoder in "
                 "full; --train_front trains the front as well (with --use_cross_attention add --train_cross_attention, which trains "
                 "query_generator.* and cross_attention.* too)")


def build_parser(distributed=False):
    """The single-process flag set; distributed=True adds --sharded (`main` parses with it)."""
    p = argparse.ArgumentParser(description="训练分类解码器 (decoder on the GPU behind the frozen encoder; see --freeze_front / --train_front)")
    p.add_argument("--vae_checkpoint", type=str, required=True, help="预训练VAE模型文件路径 (.safetensors)")
    p.add_argument("--vae_config_path", type=str, default=None, help="VAE配置文件路径 (JSON格式)")
    p.add_argument("--decoder_checkpoint", type=str, default=None, help="预训练Decoder模型文件路径 (.bin/.pth)")
    p.add_argument("--json_path", type=str, required=True)
    p.add_argument("--tags_csv_path", type=str, required=True)
    p.add_argument("--output_dir", type=str, default="decoder_output")
    p.add_argument("--resolution", type=int, default=1024)
    p.add_argument("--train_batch_size", type=int, default=1)
    p.add_argument("--num_epochs", type=int, default=10)
    p.add_argument("--learning_rate", type=float, default=1e-3)
    p.add_argument("--weight_decay", type=float, default=1e-6)
    p.add_argument("--mixed_precision", type=str, default=None, help="ignored: the head trains in fp32")
    p.add_argument("--use_attention", action="store_true", default=True, help="启用注意力机制 (默认开启)")
    p.add_argument("--no_attention", action="store_true", help="禁用注意力机制")
    p.add_argument("--use_spatial_attention", action="store_true", default=True, help="启用空间注意力")
    p.add_argument("--use_self_attention", action="store_true", default=True, help="启用自注意力")
    p.add_argument("--use_cross_attention", action="store_true", help="启用交叉注意力")
    p.add_argument("--attention_heads", type=int, default=8, help="注意力头数")
    p.add_argument("--attention_dropout", type=float, default=0.1, help="注意力dropout率")
    p.add_argument("--use_simplified_decoder_loss", action="store_true", default=True, help="使用简化的解码器损失（推荐）")
    p.add_argument("--use_focal_loss", action="store_true", help="使用Focal Loss处理类别不平衡")
    p.add_argument("--use_class_balanced", action="store_true", help="使用类别平衡损失")
    p.add_argument("--focal_alpha", type=float, default=1.0, help="Focal Loss的alpha参数")
    p.add_argument("--focal_gamma", type=float, default=2.0, help="Focal Loss的gamma参数")
    p.add_argument("--lr_scheduler_type", type=str, default="cosine", help="constant, constant_with_warmup, linear, cosine")
    p.add_argument("--lr_warmup_steps", type=int, default=500, help="学习率预热步数")
    p.add_argument("--max_grad_norm", type=float, default=1.0, help="梯度裁剪阈值")
    p.add_argument("--logging_steps", type=int, default=100, help="日志记录间隔")
    p.add_argument("--save_steps", type=int, default=5, help="模型保存间隔（epochs）")
    p.add_argument("--use_quant_conv", action="store_true", help="VAE config: use_quant_conv")
    p.add_argument("--use_post_quant_conv", action="store_true", help="VAE config: use_post_quant_conv")
    p.add_argument("--use_safetensors", action="store_true", help="ignored: checkpoints are written with torch.save")
    p.add_argument("--use_bucketing", action="store_true", help="启用长宽比分桶功能")
    p.add_argument("--base_resolution", type=int, default=512, help="分桶的基础分辨率")
    p.add_argument("--max_resolution", type=int, default=1024, help="分桶的最大分辨率")
    p.add_argument("--bucket_step", type=int, default=64, help="分桶的步长")
    p.add_argument("--num_workers", type=int, default=None, help="ignored: see --workers")
    p.add_argument("--prefetch_factor", type=int, default=None, help="ignored: the feeder pipelines by itself")
    p.add_argument("--gradient_accumulation_steps", type=int, default=1, help="梯度累积步数")
    p.add_argument("--seed", type=int, default=42,
                   help="随机种子: the validation split is the first max(1, int(0.1 n)) entries of torch.randperm(n) under a generator "
                        "seeded with it, and every epoch's training order is drawn from it -- reproducible from the seed alone, NOT "
                        "the permutation the reference's random_split draws from the global RNG")
    p.add_argument("--cudnn_benchmark", action="store_true", default=None, help="ignored")
    p.add_argument("--cudnn_deterministic", action="store_true", default=None, help="ignored: the training step is deterministic")
    # this project's own
    p.add_argument("--freeze_front", action="store_true",
                   help="attention decoders: train classifier.* only, on the front as it runs in inference (required for them)")
    p.add_argument("--train_front", action="store_true",
                   help="attention decoders: train the front too (spatial attention, feature_compress, self-attention); with "
                        "--use_cross_attention it needs --train_cross_attention")
    p.add_argument("--train_cross_attention", action="store_true",
                   help="with --train_front --use_cross_attention: train query_generator.* and cross_attention.* too (the whole decoder)")
    p.add_argument("--latent_cache_gb", type=float, default=16.0,
                   help="with --train_front: device memory for the cached latents and labels; if the set does not fit, or at 0, "
                        "every epoch re-encodes")
    p.add_argument("--no_feature_cache", action="store_true", help="re-encode every image every epoch instead of caching its feature row")
    p.add_argument("--workers", type=int, default=0, help="image decode threads (0 = min(16, cores))")
    p.add_argument("--max_pending", type=int, default=0, help="with --use_bucketing: images that may wait in partly filled buckets")
    p.add_argument("--host_resize", action="store_true", help="PIL transforms on the CPU (the reference's input route)")
    p.add_argument("--fp16_operands", action="store_true", help="fp16 instead of bf16 MFMA operands for the encoder's convolutions")
    p.add_argument("--fp8", action="store_true", help="3x3 convs of the encoder on fp8 (e4m3) operands")
    if distributed:
        p.add_argument("--sharded", action="store_true",
                       help="under torchrun: data-parallel training, one rank per GPU; rank r owns every world-th image from the r-th on, "
                            "the ranks' gradients are all-gathered and merged in rank order on every rank; rank 0 writes the files")
    return p


def ignored_arguments(args):
    """The reference's arguments that were given and mean nothing here."""
    return [k for k in IGNORED_ARGUMENTS if getattr(args, k, None) not in (None, False)]


def check_args(args):
    """What is refused, before any GPU work."""
    from .train import SCHEDULES
    if args.no_attention:
        args.use_attention = False
    if args.train_cross_attention:
        if args.freeze_front:
            raise RuntimeError("--train_cross_attention and --freeze_front exclude each other: --freeze_front trains classifier.* alone")
        if not args.train_front:
            raise RuntimeError("--train_cross_attention needs --train_front: cross-attention is trained together with the front")
        if not args.use_cross_attention:
            raise RuntimeError("--train_cross_attention needs --use_cross_attention: the decoder has no cross-attention without it")
    if args.train_front:
        if not args.use_attention:
            raise RuntimeError("--train_front trains the front of an attention decoder; with --no_attention there is none (the plain "
                               "decoder is trained in full as it is)")
        if args.freeze_front:
            raise RuntimeError("--train_front and --freeze_front exclude each other")
        if args.use_cross_attention and not args.train_cross_attention:
            raise RuntimeError("--train_front with --use_cross_attention: backward through cross-attention is not implemented without "
                               "--train_cross_attention, which trains query_generator.* and cross_attention.* too; --freeze_front "
                               "trains classifier.* on the frozen front")
        if args.attention_heads not in (1, 2, 4, 8):
            raise RuntimeError("--train_front: --attention_heads must be 1, 2, 4 or 8")
        if not 0.0 <= args.attention_dropout < 1.0 or args.latent_cache_gb < 0:
            raise RuntimeError("--attention_dropout must be in [0, 1) and --latent_cache_gb non-negative")
    elif args.use_attention and not args.freeze_front:
        raise RuntimeError(FRONT_MESSAGE)
    if args.lr_scheduler_type not in SCHEDULES:
        raise RuntimeError(f"--lr_scheduler_type {args.lr_scheduler_type}: one of {', '.join(SCHEDULES)} expected")
    if args.train_batch_size < 1 or args.num_epochs < 1 or args.save_steps < 1 or args.logging_steps < 1:
        raise RuntimeError("--train_batch_size, --num_epochs, --save_steps and --logging_steps must be at least 1")
    if getattr(args, "sharded", False):
        if args.gradient_accumulation_steps > 1:
            raise RuntimeError("--sharded with --gradient_accumulation_steps > 1 is not implemented: the loop clips every micro-step, "
                               "which has no clean meaning when the gradients are merged across ranks once per optimizer step")
        if args.no_feature_cache:
            raise RuntimeError("--sharded with --no_feature_cache is not implemented: a rank forms its batches, and the ranks agree on "
                               "the steps of an epoch, from what each has cached of its own share")
    return args


def check_shares(n_train, n_val, world):
    """--sharded, before any GPU or process-group work: every rank must own at least 2 training images and 1 validation image
    (rank r owns every world-th image from the r-th on, so the LAST rank owns the fewest)."""
    world = int(world)
    fewest_train, fewest_val = int(n_train) // world, int(n_val) // world
    if fewest_train < 2 or fewest_val < 1:
        raise RuntimeError(f"--sharded over {world} ranks: {n_train} training and {n_val} validation images leave a rank with "
                           f"{fewest_train} training and {fewest_val} validation image(s); every rank needs at least 2 and 1 "
                           "(run fewer ranks, or without --sharded)")


def _load_models(args, device):
    from .diffusers_vae_loader import DiffusersVAEWrapper, get_diffusers_vae_config, load_diffusers_vae_from_config
    from .infer_full import create_vae_from_config_file, load_state_dict_file
    from .modules import ClassificationDecoder, create_attention_decoder, get_vae_latent_info
    import pandas as pd
    if args.vae_config_path and os.path.exists(args.vae_config_path):
        vae_model = create_vae_from_config_file(args.vae_config_path, args.vae_checkpoint)
    elif args.vae_checkpoint and os.path.exists(args.vae_checkpoint):
        vae_model = DiffusersVAEWrapper(load_diffusers_vae_from_config(get_diffusers_vae_config(), args.vae_checkpoint))
    else:
        raise RuntimeError("必须提供 VAE 模型检查点或配置文件")
    vae_model.to(device).eval()
    info = get_vae_latent_info(args.resolution)
    tag_names = [str(t) for t in pd.read_csv(args.tags_csv_path)["name"]]
    if args.use_attention:
        decoder = create_attention_decoder(info["latent_channels"], info["latent_height"], info["latent_width"], len(tag_names),
                                           {"use_spatial_attention": args.use_spatial_attention, "use_self_attention": args.use_self_attention,
                                            "use_cross_attention": args.use_cross_attention, "attention_heads": args.attention_heads,
                                            "attention_dropout": args.attention_dropout})
    else:
        print("使用标准分类解码器")
        decoder = ClassificationDecoder(info["latent_channels"], info["latent_height"], info["latent_width"], len(tag_names))
    if args.decoder_checkpoint and os.path.exists(args.decoder_checkpoint):
        print(f"加载预训练Decoder: {args.decoder_checkpoint}")
        try:
            decoder.load_state_dict(load_state_dict_file(args.decoder_checkpoint), strict=False)
        except Exception as e:  # noqa: BLE001 - reference behaviour (train_decoder.py:91-92)
            print(f"Decoder模型加载失败，从零开始训练: {e}")
    else:
        print("从零开始训练Decoder")
    return vae_model, decoder.to(device).eval(), tag_names


class _LossReader:
    """The per-step losses of the device ring, read only when asked (logging steps, the end of an epoch) or when the ring is full."""

    def __init__(self, trainer, ring):
        self.trainer, self.ring, self.read_to, self.values = trainer, ring, 0, []

    def drain(self, upto):
        if upto > self.read_to:
            ring = self.trainer.losses()
            self.values.extend(float(ring[s % self.ring]) for s in range(self.read_to, upto))
            self.read_to = upto
        return self.values

    def before_step(self, step):
        if step - self.read_to >= self.ring:
            self.drain(step)


def train(args):
    """`args`: a namespace of build_parser() that has passed check_args (main does both)."""
    from . import _lib
    from .evaluate import TaggedImageList
    from .evaluation import _merge_losses_across_ranks, evaluate_and_search
    from .losses import DeviceLossAccumulator, class_balanced_weights, class_distribution, loss_report, select_loss
    from .modules import AspectRatioBucketing, get_image_transform
    from .pipeline import EncodeTagPipeline
    from .prefetch import FeederLoader
    from .train import DecoderTrainer, FeatureCache, HeadTrainer, LatentCache, epoch_order, lr_schedule, split_indices
    world, rank, group, dist = 1, 0, None, None
    if getattr(args, "sharded", False):
        # the shares are refused or accepted from the lists alone; then the process group, BEFORE any GPU call of this process
        from .infer_full import _dist_setup
        data = TaggedImageList(args.json_path, args.tags_csv_path)
        train_idx, val_idx = split_indices(len(data.image_paths), args.seed)
        check_shares(len(train_idx), len(val_idx), max(1, int(os.environ.get("WORLD_SIZE", "1"))))
        world, rank, dev_index = _dist_setup()
        if dev_index is not None:
            import torch.distributed as dist
            group = dist.group.WORLD
    sharded, chief = group is not None, rank == 0      # (--sharded in a single process without a group is the plain run)
    ignored = ignored_arguments(args)
    if ignored and chief:
        print("ignored arguments (no meaning here): " + ", ".join("--" + k for k in ignored))
    if not torch.cuda.is_available():
        raise RuntimeError("vae_tagger_amd needs an MI355X (no HIP device visible; there is no CPU fallback)")
    if sharded:
        torch.cuda.set_device(dev_index)
    device = torch.device("cuda", torch.cuda.current_device())
    vae_model, decoder, tag_names = _load_models(args, device)
    if sharded:
        # one set of initial parameters: rank 0's (a decoder trained from scratch is initialised from each process's own generator)
        box = [{k: v.detach().cpu() for k, v in decoder.state_dict().items()} if chief else None]
        dist.broadcast_object_list(box, src=0, group=group)
        if not chief:
            decoder.load_state_dict(box[0])
            decoder.to(device).eval()
    data = TaggedImageList(args.json_path, args.tags_csv_path)
    if chief:
        for p in data.missing:
            print(f"跳过图像 {p}，错误原因: 文件不存在")
    train_idx, val_idx = split_indices(len(data.image_paths), args.seed)
    train_paths, val_paths = [data.image_paths[i] for i in train_idx], [data.image_paths[i] for i in val_idx]
    if chief:
        print(f"训练集大小: {len(train_paths)}, 验证集大小: {len(val_paths)}")
    all_train = train_paths
    if sharded:
        from .train import RANK_SEED_STRIDE, GradientExchange, agreed_steps, batch_count, owned
        train_paths, val_paths = owned(train_paths, rank, world), owned(val_paths, rank, world)
    n_owned = len(train_paths) + len(val_paths) if sharded else len(data.image_paths)      # what this process may cache
    trainer_seed = args.seed + (RANK_SEED_STRIDE * rank if sharded else 0)                 # other dropout masks on every rank
    N = len(tag_names)
    selected = select_loss(args.use_class_balanced, args.use_focal_loss)
    weights = None
    if args.use_class_balanced:
        all_labels = TaggedImageList(args.json_path, args.tags_csv_path, check_files=False).labels
        weights = class_balanced_weights(class_distribution(all_labels, N))
    if args.fp8:
        vae_model.vae._context().call("vt_set_flag", 11, 1)
    elif args.fp16_operands:
        vae_model.vae.set_fp16_operands(True)
    vae_model.check_finite = False                     # the health word is read once per pass instead of once per batch
    pipe = EncodeTagPipeline.input_side(vae_model)
    bucketing = AspectRatioBucketing(args.base_resolution, args.max_resolution, args.bucket_step) if args.use_bucketing else None

    def loader(paths):
        return FeederLoader(pipe, paths, data.labels, args.train_batch_size, args.resolution, workers=args.workers or None,
                            host_resize=args.host_resize, transform=get_image_transform(args.resolution), bucketing=bucketing,
                            max_pending=args.max_pending or None)

    full = bool(args.train_front)                      # the trainer's inputs are latents (full) or the frozen front's feature rows
    if full:
        trainer = DecoderTrainer(decoder, loss=selected, focal_alpha=args.focal_alpha, focal_gamma=args.focal_gamma, class_weights=weights,
                                 attention_dropout=args.attention_dropout, seed=trainer_seed)
        side = (args.max_resolution if args.use_bucketing else args.resolution) // 8
        latent_numel = 16 * side * side              # the largest latent: a bucket's area never exceeds max_resolution^2
        budget = int(args.latent_cache_gb * (1 << 30))
        fits = not args.no_feature_cache and LatentCache.fits(n_owned, latent_numel, N, budget)
        cache = LatentCache(n_owned, latent_numel, N, device) if fits else None
    else:
        trainer = HeadTrainer(decoder, loss=selected, focal_alpha=args.focal_alpha, focal_gamma=args.focal_gamma, class_weights=weights,
                              seed=trainer_seed)
        cache = None if args.no_feature_cache else FeatureCache(n_owned, trainer.F, N, device)
    if sharded and cache is None:
        raise RuntimeError(f"--sharded: the latents of this rank's {n_owned} images do not fit --latent_cache_gb {args.latent_cache_gb}; "
                           "a sharded run trains from each rank's cache (raise the budget or run more ranks)")
    acc = DeviceLossAccumulator(N, device, args.focal_alpha, args.focal_gamma, weights, context=decoder._context())
    accum = max(1, args.gradient_accumulation_steps)
    bs = args.train_batch_size
    # (--sharded: the largest share's batches; every rank computes the same figure from the lists)
    total_steps = args.num_epochs * (batch_count(len(owned(all_train, 0, world)), bs) if sharded else (len(train_paths) + bs - 1) // bs)
    os.makedirs(args.output_dir, exist_ok=True)
    history = {"train_loss": [], "val_loss": [], "learning_rates": []}
    report = {"epochs": [], "feature_cache_bytes": cache.nbytes if cache is not None and not full else 0, "feature_dim": trainer.F,
              "train_images": len(train_paths), "val_images": len(val_paths)}
    if full:
        report["latent_cache"] = {"cached": cache is not None, "budget_bytes": budget,
                                  "bytes_needed": LatentCache.bytes_needed(n_owned, latent_numel, N), "bytes_used": 0}
    reader = _LossReader(trainer, _lib.HEAD_RING)
    micro, sched, best, current_lr = 0, 0, float("inf"), args.learning_rate * lr_schedule(args.lr_scheduler_type, 0, args.lr_warmup_steps, total_steps)
    val_batches = None                                 # the validation batches of the first pass, by name: every epoch scores the same ones

    failures = []                                      # (path, error) of the files a pass could not read

    def encoded(paths, counter):
        source = loader(paths)
        for batch in source:
            latent = vae_model.encode(batch["pixel_values"])
            feats = latent if full else trainer.features(latent)
            counter[0] += 1
            if cache is not None:
                cache.put(batch["names"], feats, batch["labels"])
            yield batch["names"], feats, batch["labels"]
        failures.extend((str(p), str(e)) for p, e in source.failed)

    def cached(batches):
        for names in batches:
            names = [n for n in names if n in cache]
            if names:
                yield (names, *cache.gather(names))

    # ---- --sharded: one epoch of the data-parallel loop (see the module docstring) ----
    exchange = GradientExchange(trainer, group, force_collective=True) if sharded else None
    agreed, local_steps = [], []                       # per epoch: the agreed step count; the steps this rank had a batch for

    def gather_objects(obj):
        out = [None] * world
        dist.all_gather_object(out, obj, group=group)
        return out

    def sync_batch_norm_buffers():
        """Rank 0's BatchNorm buffers on every rank (each rank's running statistics follow its own batches, as under DDP without
        SyncBatchNorm; this has the net effect of DDP's broadcast_buffers)."""
        if not full:
            return
        box = [{k: trainer.front.buffer(k) for k in trainer.front.buffers} if chief else None]
        dist.broadcast_object_list(box, src=0, group=group)
        if not chief:
            for k, t in box[0].items():
                trainer.front.write_buffer(k, t)

    def sharded_epoch(epoch):
        nonlocal micro, sched, best, current_lr, val_batches
        t0, enc, first, images = time.perf_counter(), [0], micro, 0
        order = [train_paths[i] for i in epoch_order(len(train_paths), args.seed, epoch)]
        if epoch == 0:
            for _ in encoded(order, enc):              # this rank's share through the encoder, once: into its cache
                pass
        if full:
            batches = cache.batches(order, bs)
        else:
            have = [p for p in order if p in cache]
            batches = [have[i:i + bs] for i in range(0, len(have), bs)]
        steps = agreed_steps(gather_objects(len(batches)))      # the ranks agree on the epoch's steps, once
        agreed.append(steps)
        for step in range(steps):
            reader.before_step(micro)
            n_local = 0
            if step < len(batches):                    # a rank that has run out joins the exchange with its zero gradients at weight 0
                names, feats, labels = batches[step], *cache.gather(batches[step])
                trainer.forward_backward(feats, labels, loss_scale=1.0, train=True, step=micro)
                n_local = len(names)
                local_steps.append(micro)
            exchange.exchange(n_local)
            if args.max_grad_norm > 0:
                trainer.clip(args.max_grad_norm)
            trainer.step(current_lr, args.weight_decay)
            sched += 1
            current_lr = args.learning_rate * lr_schedule(args.lr_scheduler_type, sched, args.lr_warmup_steps, total_steps)
            micro += 1
            images += n_local
            if chief and n_local and step % args.logging_steps == 0:
                every = reader.drain(micro)
                vals = [every[m] for m in local_steps if m >= first]
                print(f"Epoch: {epoch}, Step: {step}, Loss: {vals[-1]:.4f}, Avg Loss: {sum(vals) / len(vals):.4f}, LR: {current_lr:.2e}")
        sync_batch_norm_buffers()                      # before the validation; nothing trains between it and the saves below
        acc.reset()
        if val_batches is None:
            seen = []
            for names, feats, labels in encoded(val_paths, enc):
                acc.update(trainer.forward(feats), labels)
                seen.append(list(names))
            val_batches = seen
        else:
            for names, feats, labels in cached(val_batches):
                acc.update(trainer.forward(feats), labels)
        vae_model.vae.raise_on_status()
        every = reader.drain(micro)
        vals = [every[m] for m in local_steps if m >= first]
        per_rank = gather_objects((vals, acc.steps))
        if any(not v or not s for v, s in per_rank):
            raise RuntimeError("a rank could read no image of its share of the training or the validation set")
        merged = _merge_losses_across_ranks([acc], group)       # one all-gather; merged in rank order on rank 0
        box = [loss_report(merged[0].read(tag_names), selected)["val_loss"] if chief else None]
        dist.broadcast_object_list(box, src=0, group=group)
        val_loss = box[0]
        seconds = time.perf_counter() - t0
        every_loss = [x for v, _ in per_rank for x in v]        # the mean over all ranks' step losses, in rank order
        history["train_loss"].append(sum(every_loss) / len(every_loss))
        history["val_loss"].append(val_loss)
        history["learning_rates"].append(current_lr)
        n_img = images + sum(len(b) for b in val_batches)       # (this rank's)
        report["epochs"].append({"epoch": epoch, "seconds": seconds, "images_per_second": n_img / seconds, "images": n_img,
                                 "encoder_batches": enc[0], "steps": steps, "optimizer_steps": sched})
        if chief:
            print(f"Epoch {epoch} completed - Train Loss: {history['train_loss'][-1]:.4f}, Val Loss: {val_loss:.4f}")
        if val_loss < best:
            best = val_loss
            if chief:
                print(f"New best validation loss: {best:.4f}")
                torch.save(trainer.state_dict(), os.path.join(args.output_dir, "best_pytorch_model.bin"))
        if chief and (epoch + 1) % args.save_steps == 0:
            torch.save(trainer.state_dict(), os.path.join(args.output_dir, "pytorch_model.bin"))

    for epoch in range(args.num_epochs):
        if sharded:
            sharded_epoch(epoch)
            continue
        t0, enc, first, images = time.perf_counter(), [0], micro, 0
        order = [train_paths[i] for i in epoch_order(len(train_paths), args.seed, epoch)]
        from_cache = cache is not None and epoch > 0
        if from_cache:
            source = cached(cache.batches(order, bs) if full else [order[i:i + bs] for i in range(0, len(order), bs)])
        else:
            source = encoded(order, enc)
        for step, (names, feats, labels) in enumerate(source):
            reader.before_step(micro)
            trainer.forward_backward(feats, labels, loss_scale=1.0 / accum, train=True, step=micro)
            if args.max_grad_norm > 0:
                trainer.clip(args.max_grad_norm)
            if (step + 1) % accum == 0:
                trainer.step(current_lr, args.weight_decay)
                sched += 1
                current_lr = args.learning_rate * lr_schedule(args.lr_scheduler_type, sched, args.lr_warmup_steps, total_steps)
            micro += 1
            images += len(names)
            if step % args.logging_steps == 0:
                vals = reader.drain(micro)[first:]
                print(f"Epoch: {epoch}, Step: {step}, Loss: {vals[-1]:.4f}, Avg Loss: {sum(vals) / len(vals):.4f}, LR: {current_lr:.2e}")
        train_steps = micro - first
        # validation: eval mode (the head on the frozen front's rows; with --train_front the front on its running statistics)
        acc.reset()
        if val_batches is None or cache is None:
            seen = []
            for names, feats, labels in encoded(val_paths, enc):
                acc.update(trainer.forward(feats), labels)
                seen.append(list(names))
            val_batches = seen
        else:
            for names, feats, labels in cached(val_batches):
                acc.update(trainer.forward(feats), labels)
        vae_model.vae.raise_on_status()                # the encoder's health word, once per epoch (synchronises)
        vals = reader.drain(micro)[first:]
        seconds = time.perf_counter() - t0
        if not vals or not acc.steps:
            raise RuntimeError("no image of the training or the validation set could be read")
        val_loss = loss_report(acc.read(tag_names), selected)["val_loss"]
        history["train_loss"].append(sum(vals) / len(vals))
        history["val_loss"].append(val_loss)
        history["learning_rates"].append(current_lr)
        n_img = images + sum(len(b) for b in val_batches)
        report["epochs"].append({"epoch": epoch, "seconds": seconds, "images_per_second": n_img / seconds, "images": n_img,
                                 "encoder_batches": enc[0], "steps": train_steps, "optimizer_steps": sched})
        print(f"Epoch {epoch} completed - Train Loss: {history['train_loss'][-1]:.4f}, Val Loss: {val_loss:.4f}")
        if val_loss < best:
            best = val_loss
            print(f"New best validation loss: {best:.4f}")
            torch.save(trainer.state_dict(), os.path.join(args.output_dir, "best_pytorch_model.bin"))
        if (epoch + 1) % args.save_steps == 0:
            torch.save(trainer.state_dict(), os.path.join(args.output_dir, "pytorch_model.bin"))
    if chief:
        print("训练完成，开始最终评估...")
    if full and cache is not None:
        report["latent_cache"]["bytes_used"] = cache.nbytes
    if sharded:
        # what every rank reports of itself, in rank order; state_sha256: the parameters, Adam m and v of every block after the last step
        mine = {"train_images": len(train_paths), "val_images": len(val_paths), "cache_bytes": cache.nbytes,
                "state_sha256": trainer.optimizer_state_sha256().hexdigest(), "failures": failures}
        ranks = gather_objects(mine)
        report["train_images"], report["val_images"] = len(all_train), sum(r["val_images"] for r in ranks)
        report["sharded"] = {"world": world, "backend": exchange.backend, "steps_per_epoch": agreed,
                             "exchange_bytes_received_per_step": exchange.bytes_received_per_step,
                             **{k: [r[k] for r in ranks] for k in ("train_images", "val_images", "cache_bytes", "state_sha256")}}
        if chief:
            for p, e in sorted({p: e for r in ranks for p, e in r["failures"]}.items()):      # every file belongs to one rank: each once
                print(f"跳过图像 {p}，错误原因: {e}")
    if chief:
        with open(os.path.join(args.output_dir, "training_history.json"), "w") as fh:
            json.dump(history, fh, indent=2)
        with open(os.path.join(args.output_dir, "train_report.json"), "w") as fh:
            json.dump(report, fh, indent=2)
    trainer.commit()
    decoder.load_state_dict(trainer.state_dict(), strict=False)   # the module's own tensors follow the device tables
    decoder.to(device).eval()
    optimal, metrics, _ = evaluate_and_search(vae_model, decoder, loader(val_paths), tag_names, device, args.output_dir, group=group)
    if chief:
        print("训练和评估完成！")
    return {"history": history, "report": report, "optimal_thresholds": optimal, "metrics": metrics, "best_val_loss": best}


def main(argv=None):
    args = build_parser(distributed=True).parse_args(argv)
    try:
        check_args(args)
    except RuntimeError as e:
        raise SystemExit(str(e))
    return train(args)


if __name__ == "__main__":
    main()
