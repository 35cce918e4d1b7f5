"""VAE validation loss CLI: the number the reference's train_vae.py keeps `best_vae` by (train_vae.py:216-268) -- reconstruction MSE,
KL of the three posteriors, the triplet loss on sampled latents -- and, with --decoder_checkpoint, train_full.py's total
(train_full.py:290-338), over EVERY entry of the JSON given (pass the validation split: the reference's random_split is not reproduced).

    python -m vae_tagger_amd.evaluate_vae --vae_checkpoint ae.safetensors --json_path val.json --tags_csv_path tags.csv \
        [--vae_checkpoints A B C] [--use_bucketing] [--use_simplified_vae_loss] [--decoder_checkpoint dec.pth]

Per batch: three encodes (moments), one vt_posterior_sample (draw 0) and one decode for the anchor, one vt_vae_loss_update that samples
the three latents of the triplet loss in flight (draws 1, 2, 3).  The reference also decodes the positive and the negative and throws
the result away; that is skipped, and so is the anchor's decode where no reconstruction term enters the total (train_full's simplified
loss).  Nothing is read back per batch; the health word is read once per checkpoint.  Images are decoded and resized with PIL on a
thread pool (the reference's transforms), cross PCIe as uint8 and are normalised on the device (vt_preprocess_u8: the host transform's
values bit for bit); the next batch loads while the GPU works on this one.

Triplets: the reference's _sample_triplet_paths / _online_triplet_mining (modules.py:599-686) restated over TaggedImageList, with ONE
difference: each anchor draws from its own random.Random(seed * 2**32 + anchor index), so a triplet depends neither on the order of
evaluation nor on the batch size.  This is NOT the reference's stream -- it draws from the global `random` inside DataLoader worker
processes, which no two runs share.  The candidate set is walked in the order drawn (the reference walks a Python set).
With --use_bucketing the positive and the negative are resized to the ANCHOR's bucket: reshape(B, -1) rows need one D (the reference
cannot collate mixed buckets at all).  The noise of an image is keyed on its position in the evaluation order (JSON order, grouped by
bucket with --use_bucketing), which does not depend on the batch size either.

Writes vae_validation_loss.json (every component as the mean of batch means and per image, both similarity types, the selected total,
counters, settings) and per_image.json (sorted by mse, worst first); with --vae_checkpoints each checkpoint's files go to
output_dir/ckpt_<index>_<stem>/ and output_dir/checkpoint_sweep.json ranks them by the selected total.
"""
import argparse
import json
import math
import os
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import vae_losses
from .losses import sweep_dir_name

MAX_CANDIDATES = 100


# ---- triplets (host) ------------------------------------------------------------------------------------------------------------------
def mine_candidates(rng, anchor_idx, label_matrix, max_candidates=MAX_CANDIDATES):
    """_online_triplet_mining: up to max_candidates distinct other indices drawn with rng.randrange, split by overlap > 0 with the
    anchor's labels.  Returns (positive indices, negative indices) in the order drawn."""
    n = len(label_matrix)
    k = min(max_candidates, max(0, n - 1))
    seen, order = set(), []
    while len(order) < k:
        j = rng.randrange(0, n)
        if j != anchor_idx and j not in seen:
            seen.add(j)
            order.append(j)
    anchor = label_matrix[anchor_idx]
    pos = [j for j in order if float((label_matrix[j] * anchor).sum()) > 0]
    neg = [j for j in order if not float((label_matrix[j] * anchor).sum()) > 0]
    return pos, neg


def sample_triplet(seed, anchor_idx, label_matrix, max_candidates=MAX_CANDIDATES):
    """_sample_triplet_paths for one anchor with its own generator: (positive index, negative index).  With more than one tag on the
    anchor and more than one positive candidate, the highest overlap is taken with probability 0.7 (the first of equal overlaps, as the
    reference's stable sort), else a random positive; without a positive candidate the anchor itself; without a negative candidate a
    random other image (the anchor itself in a set of one)."""
    rng = random.Random(int(seed) * 2 ** 32 + int(anchor_idx))
    n = len(label_matrix)
    anchor = label_matrix[anchor_idx]
    pos, neg = mine_candidates(rng, anchor_idx, label_matrix, max_candidates)
    if float(anchor.sum()) > 1 and pos:
        scores = sorted(((j, float((label_matrix[j] * anchor).sum())) for j in pos), key=lambda t: t[1], reverse=True)
        positive = scores[0][0] if (rng.random() < 0.7 and len(scores) > 1) else rng.choice(pos)
    elif pos:
        positive = rng.choice(pos)
    else:
        positive = anchor_idx
    if neg:
        negative = rng.choice(neg)
    elif n > 1:
        negative = anchor_idx
        while negative == anchor_idx:
            negative = rng.randrange(0, n)
    else:
        negative = anchor_idx
    return positive, negative


def triplet_lists(label_matrix, seed, max_candidates=MAX_CANDIDATES):
    """[(positive index, negative index)] for every anchor of the list."""
    return [sample_triplet(seed, i, label_matrix, max_candidates) for i in range(len(label_matrix))]


def plan_batches(paths, batch_size, buckets=None):
    """The evaluation order and its batches: [(bucket or None, [anchor indices])].  Without buckets the JSON order; with them the
    anchors grouped by bucket (buckets ascending, JSON order inside), so an image's position does not depend on the batch size."""
    order = list(range(len(paths)))
    if buckets is not None:
        order.sort(key=lambda i: (buckets[i], i))
    out = []
    for i in order:
        b = buckets[i] if buckets is not None else None
        if out and out[-1][0] == b and len(out[-1][1]) < batch_size:
            out[-1][1].append(i)
        else:
            out.append((b, [i]))
    return out


# ---- report arithmetic (host) ----------------------------------------------------------------------------------------------------------
def psnr(mse):
    """20 log10(2) - 10 log10(mse) for images in [-1, 1]; inf for a perfect reconstruction."""
    return float("inf") if mse <= 0 else 20.0 * math.log10(2.0) - 10.0 * math.log10(mse)


def loss_weights(args):
    return {"reconstruction": args.reconstruction_weight, "kl": args.kl_weight, "triplet": args.triplet_weight}


def build_report(state, args, classification=None):
    """vae_validation_loss.json from a parsed VAE loss state: finish_state's report; with a classification loss (losses.finish_state's
    dict and the selected name) train_full's total joins: the simplified one is triplet + classification, the full one adds
    reconstruction and KL."""
    simplified = bool(args.use_simplified_vae_loss)
    if classification is not None and simplified:
        weights = {"reconstruction": 0.0, "kl": 0.0, "triplet": args.triplet_weight}
    else:
        weights = loss_weights(args)
    rep = vae_losses.finish_state(state, weights, args.similarity_type, simplified)
    rep["val_loss_train_vae"] = rep["val_loss"]
    if classification is not None:
        loss, selected = classification
        rep["classification"] = {"selected_loss": selected, **{k: loss[k] for k in ("bce", "focal", "class_balanced")},
                                 "weight": float(args.classification_weight)}
        rep["val_loss_train_full"] = rep["val_loss"] + float(args.classification_weight) * loss[selected]["mean_of_batch_means"]
        rep["val_loss"] = rep["val_loss_train_full"]
        del rep["val_loss_train_vae"]
    return rep


def per_image_table(rows, paths, order, triplets, similarity_type="cosine", with_recon=True):
    """per_image.json: one entry per anchor in evaluation order `order` (rows[k] belongs to paths[order[k]]), sorted by mse descending
    (ties: evaluation order).  Without a reconstruction (train_full's simplified loss decodes nothing) mse and psnr are None and the
    evaluation order stands."""
    names = vae_losses.ROW_NAMES
    sim = "cosine" if similarity_type == "cosine" else "euclidean"
    out = []
    for k, i in enumerate(order):
        r = dict(zip(names, (float(v) for v in rows[k])))
        out.append({"path": paths[i], "positive": paths[triplets[i][0]], "negative": paths[triplets[i][1]], "mse": r["mse"] if with_recon else None,
                    "psnr": psnr(r["mse"]) if with_recon else None,
                    "kl": r["kl_a"], "pos_cosine": r["pos_cosine"], "neg_cosine": r["neg_cosine"], "pos_euclidean": r["pos_euclidean"],
                    "neg_euclidean": r["neg_euclidean"], "triplet": r["triplet_" + sim], "position": k})
    if with_recon:
        out.sort(key=lambda e: (-e["mse"] if e["mse"] == e["mse"] else float("-inf"), e["position"]))
    return out


def sweep_summary(rows):
    """checkpoint_sweep.json from [{path, report}]: ranked by the selected total; a tie goes to the earlier checkpoint, a NaN never wins."""
    table = [{"index": i, "path": str(r["path"]), "val_loss": r["report"]["val_loss"], "val_loss_per_image": r["report"]["val_loss_per_image"],
              "components": r["report"]["components"], "non_finite": r["report"]["non_finite"]} for i, r in enumerate(rows)]
    finite = [t for t in table if t["val_loss"] == t["val_loss"]]
    ranking = [t["index"] for t in sorted(finite, key=lambda t: (t["val_loss"], t["index"]))]
    best = None if not ranking else {"index": ranking[0], "path": table[ranking[0]]["path"]}
    return {"selected_loss": "val_loss", "checkpoints": table, "ranking": ranking, "best_by_val_loss": best}


# ---- the device pass ---------------------------------------------------------------------------------------------------------------
def _load_batch(pool, paths, indices, resolution, bucket, normalize):
    """The images of `indices` as one fp32 NCHW device batch in [-1, 1]: decode and resize with PIL on the pool's threads (the
    reference's SmartResize for a bucket, else the distorting bilinear resize), uint8 pixels over PCIe, ToTensor + Normalize on the
    device (vt_preprocess_u8: bit for bit the host transform's values)."""
    import torch
    from PIL import Image
    from .modules import SmartResize
    resize = SmartResize(*bucket) if bucket is not None else (lambda img: img.resize((resolution, resolution), Image.BILINEAR))

    def one(i):
        with Image.open(paths[i]) as img:
            return np.asarray(resize(img.convert("RGB")), dtype=np.uint8)
    return normalize(torch.from_numpy(np.stack(list(pool.map(one, indices)))))


def run_checkpoint(args, vae_model, data, labels, triplets, batches, decoder=None, class_weights=None, selected=None, device="cuda"):
    """One pass over the data for the loaded model: (parsed state, rows [images, ROW] in evaluation order, classification loss or None)."""
    import torch
    from .infer_vae import _EncoderInput
    from .losses import DeviceLossAccumulator
    vae = vae_model.vae
    simplified = bool(args.use_simplified_vae_loss)
    want_recon = not (decoder is not None and simplified)
    acc = vae_losses.DeviceVAELossAccumulator(device, args.triplet_margin, 1.0, seed=args.seed, context=vae._context())
    cls = None
    if decoder is not None:
        cls = DeviceLossAccumulator(labels.shape[1], device, args.focal_alpha, args.focal_gamma, class_weights)
    total = sum(len(b) for _, b in batches)
    rows = torch.zeros(total, vae_losses.ROW, dtype=torch.float64, device=device)
    label_t = torch.from_numpy(labels).to(device)
    paths = data.image_paths
    cfg = vae.config
    inputs = _EncoderInput(vae_model)
    load = lambda pool, indices, bucket: _load_batch(pool, paths, indices, args.resolution, bucket,
                                                     lambda u8: inputs.normalize_u8(u8.to(device, non_blocking=True)))
    first = 0
    with ThreadPoolExecutor(max_workers=max(1, args.workers or min(16, os.cpu_count() or 1))) as pool, torch.no_grad():
        for bucket, idx in batches:
            xa = load(pool, idx, bucket)
            xp = load(pool, [triplets[i][0] for i in idx], bucket)
            xn = load(pool, [triplets[i][1] for i in idx], bucket)
            pa, pp, pn = (vae.encode(x).latent_dist for x in (xa, xp, xn))
            recon = vae.decode(pa.sample_device(args.seed, 0, first)).sample if want_recon else None
            ia = torch.as_tensor(idx, device=device)
            ip = torch.as_tensor([triplets[i][0] for i in idx], device=device)
            acc.update(anchor=(pa.parameters, None, 1), positive=(pp.parameters, None, 2), negative=(pn.parameters, None, 3), recon=recon,
                       target=xa if want_recon else None, labels_a=label_t[ia], labels_p=label_t[ip], first_image=first,
                       rows_out=rows[first:first + len(idx)])
            if decoder is not None:
                latent = pa.mode()
                if getattr(cfg, "scaling_factor", None) is not None:
                    latent = latent * cfg.scaling_factor
                if getattr(cfg, "shift_factor", None) is not None:
                    latent = latent + cfg.shift_factor
                cls.update(decoder(latent), label_t[ia])
            first += len(idx)
    state = acc.read_state()                                             # the one synchronisation of the pass
    st = vae.status()
    if st:
        raise FloatingPointError(f"device health word {st}: non-finite activations in the VAE (fp32 residual storage or bf16 operands may cure it)")
    return state, rows.cpu().numpy(), (None if cls is None else (cls.read(), selected))


def _write(path, obj):
    with open(path, "w", encoding="utf-8") as fh:
        json.dump(obj, fh, indent=2, ensure_ascii=False, sort_keys=True)


def evaluate(args):
    import torch
    from .evaluate import TaggedImageList
    from .modules import AspectRatioBucketing
    from .vae_reconstruction_test import load_vae_model
    if not torch.cuda.is_available():
        raise RuntimeError("vae_tagger_amd needs an MI355X (no HIP device visible; there is no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device())
    data = TaggedImageList(args.json_path, args.tags_csv_path)
    for p in data.missing:
        print(f"跳过图像 {p}，错误原因: 文件不存在")
    if not data.image_paths:
        raise RuntimeError(f"{args.json_path} 中没有可用的图像")
    paths = data.image_paths
    labels = np.stack([data.labels[p] for p in paths]).astype(np.float32)
    triplets = triplet_lists(labels, args.seed)
    buckets = None
    if args.use_bucketing:
        bucketing = AspectRatioBucketing(args.base_resolution, args.max_resolution, args.bucket_step)
        buckets = [bucketing.assign_bucket(p) for p in paths]
    batches = plan_batches(paths, args.batch_size, buckets)
    order = [i for _, b in batches for i in b]
    checkpoints = args.vae_checkpoints or [args.vae_checkpoint]
    decoder = class_weights = selected = None
    os.makedirs(args.output_dir, exist_ok=True)
    results = []
    for k, ckpt in enumerate(checkpoints):
        args.vae_checkpoint = ckpt
        if args.decoder_checkpoint:
            from .infer_full import load_models
            from .losses import class_balanced_weights, class_distribution, select_loss
            args.use_attention = not args.no_attention
            vae_model, decoder, _ = load_models(args, device)
            selected = select_loss(args.use_class_balanced, args.use_focal_loss)
            class_weights = class_balanced_weights(class_distribution(TaggedImageList(args.json_path, args.tags_csv_path, check_files=False).labels,
                                                                      labels.shape[1]))
        else:
            vae_model = load_vae_model(args, device)
        vae_model.check_finite = False
        if args.bf16_operands:
            vae_model.vae.set_fp16_operands(False)
        elif args.fp16_operands:
            vae_model.vae.set_fp16_operands(True)
        state, rows, classification = run_checkpoint(args, vae_model, data, labels, triplets, batches, decoder, class_weights, selected, device)
        report = build_report(state, args, classification)
        report["settings"] = {"vae_checkpoint": str(ckpt), "json_path": args.json_path, "images": len(order), "batch_size": args.batch_size,
                              "resolution": args.resolution, "use_bucketing": bool(args.use_bucketing), "seed": args.seed,
                              "triplet_margin": args.triplet_margin, "operands": "bf16" if args.bf16_operands else ("fp16" if args.fp16_operands else "default")}
        out_dir = os.path.join(args.output_dir, sweep_dir_name(k, ckpt)) if args.vae_checkpoints else args.output_dir
        os.makedirs(out_dir, exist_ok=True)
        _write(os.path.join(out_dir, "vae_validation_loss.json"), report)
        _write(os.path.join(out_dir, "per_image.json"), per_image_table(rows, paths, order, triplets, args.similarity_type, with_recon=state["recon_images"] > 0))
        print(f"{ckpt}: val_loss {report['val_loss']:.6f}  images {report['images']}  non_finite {report['non_finite']}")
        results.append({"path": ckpt, "report": report})
    if args.vae_checkpoints:
        summary = sweep_summary(results)
        _write(os.path.join(args.output_dir, "checkpoint_sweep.json"), summary)
        print(f"best_by_val_loss: {summary['best_by_val_loss']}")
    return results


def build_parser():
    p = argparse.ArgumentParser(description="VAE 验证损失 (重建 MSE + KL + 三元组损失), 在GPU上累积。")
    p.add_argument("--vae_checkpoint", type=str, default=None, help="预训练VAE模型文件路径 (.safetensors)")
    p.add_argument("--vae_checkpoints", type=str, nargs="+", default=None,
                   help="sweep: score these VAE checkpoints one after the other; files go to output_dir/ckpt_<index>_<stem>/ and "
                        "output_dir/checkpoint_sweep.json ranks them by the selected total")
    p.add_argument("--vae_config_path", type=str, default=None, help="VAE配置文件路径 (JSON格式)")
    p.add_argument("--json_path", type=str, required=True, help='{image path: "tag:weight, tag:weight"}: EVERY entry is evaluated')
    p.add_argument("--tags_csv_path", type=str, required=True, help="包含所有分类头的CSV文件")
    p.add_argument("--output_dir", type=str, default="vae_output")
    p.add_argument("--resolution", type=int, default=1024)
    p.add_argument("--batch_size", type=int, default=4, help="train_vae.py's --train_batch_size")
    p.add_argument("--reconstruction_weight", type=float, default=0.01, help="重建损失权重")
    p.add_argument("--kl_weight", type=float, default=1e-2, help="KL损失权重")
    p.add_argument("--triplet_weight", type=float, default=1.0, help="三元组损失权重")
    p.add_argument("--triplet_margin", type=float, default=1.0, help="三元组损失的margin")
    p.add_argument("--similarity_type", type=str, default="cosine", choices=["cosine", "euclidean"], help="相似度类型")
    p.add_argument("--use_simplified_vae_loss", action="store_true", help="重建 + 三元组 (KL只作监控)")
    p.add_argument("--use_bucketing", action="store_true", help="启用长宽比分桶功能")
    p.add_argument("--base_resolution", type=int, default=512, help="分桶的基础分辨率")
    p.add_argument("--max_resolution", type=int, default=1024, help="分桶的最大分辨率")
    p.add_argument("--bucket_step", type=int, default=64, help="分桶的步长")
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--workers", type=int, default=0, help="image decode threads (0 = min(16, cores))")
    p.add_argument("--decoder_checkpoint", type=str, default=None,
                   help="also form train_full.py's total: logits from mode() * scaling + shift through this decoder, the classification "
                        "loss accumulated on the GPU; with --use_simplified_vae_loss the total is triplet + classification and nothing is decoded")
    p.add_argument("--classification_weight", type=float, default=1.0, help="分类损失权重")
    p.add_argument("--use_focal_loss", action="store_true", help="使用Focal Loss处理类别不平衡")
    p.add_argument("--use_class_balanced", action="store_true", help="使用类别平衡损失")
    p.add_argument("--focal_alpha", type=float, default=1.0, help="Focal Loss的alpha参数")
    p.add_argument("--focal_gamma", type=float, default=2.0, help="Focal Loss的gamma参数")
    p.add_argument("--no_attention", action="store_true", help="禁用注意力机制 (--decoder_checkpoint)")
    p.add_argument("--use_cross_attention", action="store_true", help="启用交叉注意力 (--decoder_checkpoint)")
    p.add_argument("--fp16_operands", action="store_true", help="fp16 MFMA operands for the convolutions")
    p.add_argument("--bf16_operands", action="store_true", help="bf16 MFMA operands for the convolutions")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not args.vae_checkpoint and not args.vae_checkpoints and not args.vae_config_path:
        raise SystemExit("必须提供 --vae_checkpoint, --vae_checkpoints 或 --vae_config_path")
    if args.fp16_operands and args.bf16_operands:
        raise SystemExit("--fp16_operands and --bf16_operands exclude each other")
    return evaluate(args)


if __name__ == "__main__":
    main()
