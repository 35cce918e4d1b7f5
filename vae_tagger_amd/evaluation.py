"""Batched evaluation caller of the encode+tag path: the counterpart of the reference's evaluation.py
(MultiLabelEvaluator :13-170, evaluate_model :173-200, find_optimal_threshold :202-275) -- SURVEY.md section 8(f) item 4.

Same call surface (`model.encode(pixel_values)` -> `decoder(latents)` -> sigmoid -> threshold, same metric keys and
output files); different mechanics: per batch only the probabilities leave the GPU (one copy), and every metric is
computed once at the end from vectorised numpy -- confusion counts for precision / recall / F1, a rank-based average
precision -- instead of per-class scikit-learn calls.  tests/test_host.py checks the numbers against scikit-learn.
"""
import json
import os

import numpy as np
import torch


def _average_precision(y_true, y_prob):
    """Per-column AP = sum_k (R_k - R_{k-1}) P_k over the distinct score thresholds (scikit-learn's definition);
    columns without a positive get nan."""
    n, c = y_true.shape
    ap = np.full(c, np.nan)
    for j in range(c):
        t = y_true[:, j] > 0
        npos = int(t.sum())
        if npos == 0:
            continue
        order = np.argsort(-y_prob[:, j], kind="stable")
        s, t = y_prob[order, j], t[order]
        last = np.r_[s[1:] != s[:-1], True]              # last element of every run of tied scores
        tp = np.cumsum(t)[last]
        k = (np.nonzero(last)[0] + 1).astype(np.float64)
        recall = tp / npos
        ap[j] = float(np.sum(np.diff(np.r_[0.0, recall]) * (tp / k)))
    return ap


def _prf(tp, fp, fn):
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.where(tp + fp > 0, tp / (tp + fp), 0.0)
        r = np.where(tp + fn > 0, tp / (tp + fn), 0.0)
        f = np.where(2 * tp + fp + fn > 0, 2 * tp / (2 * tp + fp + fn), 0.0)
    return p, r, f


class MultiLabelEvaluator:
    def __init__(self, class_names=None, device="cuda"):
        self.class_names = class_names
        self.device = device
        self.reset_metrics()

    def reset_metrics(self):
        self.all_predictions, self.all_targets, self.all_probabilities = [], [], []

    @staticmethod
    def _np(x):
        return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)

    def update(self, predictions, targets, probabilities=None):
        """predictions / targets / probabilities: (batch, num_classes) tensors or arrays."""
        self.all_predictions.append(self._np(predictions))
        self.all_targets.append(self._np(targets))
        if probabilities is not None:
            self.all_probabilities.append(self._np(probabilities))

    def compute_metrics(self, threshold=0.5):
        if not self.all_targets:
            raise ValueError("no data: call update() first")
        y_true = np.vstack(self.all_targets) > 0
        y_pred = np.vstack(self.all_predictions) > 0
        y_prob = np.vstack(self.all_probabilities) if self.all_probabilities else y_pred.astype(np.float64)
        n, c = y_true.shape
        tp = (y_true & y_pred).sum(0).astype(np.float64)
        fp = (~y_true & y_pred).sum(0).astype(np.float64)
        fn = (y_true & ~y_pred).sum(0).astype(np.float64)
        support = y_true.sum(0).astype(np.float64)
        p, r, f = _prf(tp, fp, fn)
        m = {"accuracy": float((y_true == y_pred).all(1).mean()), "hamming_loss": float((y_true != y_pred).mean())}
        mp, mr, mf = _prf(tp.sum(), fp.sum(), fn.sum())
        w = support / support.sum() if support.sum() > 0 else np.zeros(c)
        for name, per, micro in (("precision", p, mp), ("recall", r, mr), ("f1", f, mf)):
            m[f"{name}_micro"] = float(micro)
            m[f"{name}_macro"] = float(per.mean())
            m[f"{name}_weighted"] = float((per * w).sum())
        # scikit-learn (what the reference calls, evaluation.py:65-67) scores a class without a positive sample as AP 0 (with a
        # warning) and still averages: macro over all classes, weighted by support, micro over the flattened matrix
        ap = np.nan_to_num(_average_precision(y_true, y_prob), nan=0.0)
        m["mAP"] = float(ap.mean())
        m["mAP_micro"] = float(np.nan_to_num(_average_precision(y_true.reshape(-1, 1), y_prob.reshape(-1, 1)), nan=0.0)[0])
        m["mAP_weighted"] = float((ap * w).sum())
        per_class = {}
        for i in range(c):
            name = self.class_names[i] if self.class_names else f"Class_{i}"
            if support[i] == 0:
                per_class[name] = {"precision": 0.0, "recall": 0.0, "f1": 0.0, "ap": 0.0, "support": 0}
            elif support[i] == n:                        # every sample positive: AP is 1 by convention
                q = float(y_pred[:, i].mean())
                per_class[name] = {"precision": q, "recall": 1.0, "f1": 2 * q / (1 + q) if q > 0 else 0.0, "ap": 1.0,
                                   "support": int(support[i])}
            else:
                per_class[name] = {"precision": float(p[i]), "recall": float(r[i]), "f1": float(f[i]),
                                   "ap": float(ap[i]), "support": int(support[i])}
        m["per_class"] = per_class
        return m

    def print_metrics(self, metrics, detailed=True):
        print(f"subset accuracy {metrics['accuracy']:.4f}   hamming loss {metrics['hamming_loss']:.4f}")
        for k in ("precision", "recall", "f1"):
            print(f"  {k:9s} micro {metrics[k + '_micro']:.4f}  macro {metrics[k + '_macro']:.4f}  weighted {metrics[k + '_weighted']:.4f}")
        print(f"  mAP       macro {metrics['mAP']:.4f}  micro {metrics['mAP_micro']:.4f}  weighted {metrics['mAP_weighted']:.4f}")
        if detailed and "per_class" in metrics:
            print(f"{'':<20} {'Precision':<10} {'Recall':<10} {'F1':<10} {'AP':<10} {'Support':<10}")
            for name, v in metrics["per_class"].items():
                print(f"{name:<20} {v['precision']:<10.4f} {v['recall']:<10.4f} {v['f1']:<10.4f} {v['ap']:<10.4f} {v['support']:<10}")

    def save_metrics(self, metrics, output_path):
        """`<name>_overall.json` + a per-class CSV, as the reference writes them."""
        with open(output_path.replace(".csv", "_overall.json"), "w", encoding="utf-8") as fh:
            json.dump({k: v for k, v in metrics.items() if k != "per_class"}, fh, indent=2, ensure_ascii=False)
        if "per_class" in metrics:
            with open(output_path, "w", encoding="utf-8") as fh:
                fh.write("class_name,precision,recall,f1,ap,support\n")
                for name, v in metrics["per_class"].items():
                    fh.write(f"{name},{v['precision']},{v['recall']},{v['f1']},{v['ap']},{v['support']}\n")


def _check_status(model):
    """After the batch's host copy (a synchronisation point anyway): the encoder's sticky health word (vt_status)."""
    vae = getattr(model, "vae", model)
    ctx = vae._context() if hasattr(vae, "_context") else None
    st = vae.status() if ctx is not None else 0     # on torch's current stream of the model's device: ordered after the encode
    if st & 1:
        raise FloatingPointError("non-finite activations in the encoder: the fp16 residual-stream storage overflowed "
                                 "(vt_set_flag(ctx, 4, 0) stores it as fp32) or the checkpoint holds inf / NaN")
    if st & 2:
        raise FloatingPointError("fp8 mode: activations exceeded the e4m3 range and were clamped (vt_set_flag(ctx, 11, 0) returns to bf16)")


def _probabilities(model, decoder, loader, device):
    """The batched hot path: encode -> decoder -> sigmoid on the GPU; one host copy of the probabilities per batch."""
    probs, labels = [], []
    # this loop reads the health word itself, after the batch's host copy: the wrapper's own per-encode check (a stream synchronise and a
    # 4-byte copy between the encoder's and the decoder's launches, and a read that clears the word before ours) is switched off meanwhile
    had_check = getattr(model, "check_finite", None)
    if had_check is not None:
        model.check_finite = False
    try:
        with torch.no_grad():
            for batch in loader:
                lat = model.encode(batch["pixel_values"].to(device))
                probs.append(torch.sigmoid(decoder(lat)).cpu().numpy())
                labels.append(MultiLabelEvaluator._np(batch["labels"]))
                _check_status(model)
    finally:
        if had_check is not None:
            model.check_finite = had_check
    return np.vstack(probs), np.vstack(labels)


RESULTS_CSV = "evaluation_results.csv"
PER_CLASS_RESULTS_CSV = "evaluation_results_per_class_thresholds.csv"     # the metrics under the searched per-class thresholds


def threshold_vector(per_class, class_names, default):
    """fp64 [N] in class order from find_optimal_threshold's dict (or its `per_class_thresholds` entry, or a plain {name: threshold}
    mapping); a class the mapping does not name gets `default`.  An array is returned as it is."""
    if isinstance(per_class, dict):
        per_class = per_class.get("per_class_thresholds", per_class)
        out = np.full(len(class_names), np.float64(default))
        for i, name in enumerate(class_names):
            v = per_class.get(name)
            if v is not None:
                out[i] = float(v["threshold"]) if isinstance(v, dict) else float(v)
        return out
    out = np.asarray(per_class, dtype=np.float64)
    if out.shape != (len(class_names),):
        raise ValueError(f"expected {len(class_names)} per-class thresholds, got an array of shape {out.shape}")
    return out


def _host_metrics(y_prob, y_true, class_names, device, threshold):
    """The host evaluator on the whole probability matrix: `threshold` is a Python float (compared as `y_prob > 0.5` is) or an fp64
    vector with one entry per class (float32 matrix > float64 row: compared in fp64)."""
    ev = MultiLabelEvaluator(class_names, device)
    ev.update((y_prob > threshold).astype(np.float32), y_true, y_prob)
    return ev.compute_metrics()


def _report(metrics, output_dir, filename):
    """Print the metrics and write `<filename>` + its `_overall.json` (MultiLabelEvaluator's own formats)."""
    ev = MultiLabelEvaluator.__new__(MultiLabelEvaluator)
    ev.print_metrics(metrics)
    if output_dir:
        os.makedirs(output_dir, exist_ok=True)
        ev.save_metrics(metrics, os.path.join(output_dir, filename))
    return metrics


def _host_search(y_prob, y_true, class_names):
    """find_optimal_threshold's search on the host matrix."""
    y_true = y_true > 0
    thresholds = np.arange(0.1, 0.9, 0.05)
    c = y_true.shape[1]
    best_f, best_t = np.zeros(c), np.full(c, 0.5)
    g_f, g_t = 0.0, 0.5
    for t in thresholds:
        y_pred = y_prob > t
        tp = (y_true & y_pred).sum(0).astype(np.float64)
        fp = (~y_true & y_pred).sum(0).astype(np.float64)
        fn = (y_true & ~y_pred).sum(0).astype(np.float64)
        f = _prf(tp, fp, fn)[2]
        better = (f > best_f) & (y_true.sum(0) > 0)
        best_f[better], best_t[better] = f[better], t
        if f.mean() > g_f:
            g_f, g_t = float(f.mean()), float(t)
    return {"global_threshold": g_t, "global_f1": g_f,
            "per_class_thresholds": {n: {"threshold": float(best_t[i]), "f1_score": float(best_f[i])}
                                     for i, n in enumerate(class_names)}}


def _report_search(results, output_dir):
    print(f"global threshold {results['global_threshold']:.3f} (macro F1 {results['global_f1']:.4f})")
    if output_dir:
        os.makedirs(output_dir, exist_ok=True)
        with open(os.path.join(output_dir, "optimal_thresholds.json"), "w", encoding="utf-8") as fh:
            json.dump(results, fh, indent=2, ensure_ascii=False)
    return results


def evaluate_model(model, decoder, test_loader, class_names, device="cuda", threshold=0.5, output_dir=None, device_metrics=False,
                   group=None, per_class_thresholds=None):
    """device_metrics=True: the probabilities never leave the GPU (DeviceMultiLabelEvaluator); same dict, prints and files.
    group (with device_metrics only; torch.distributed.group.WORLD for the default group): `test_loader` is this rank's share; the
    states are merged on rank 0, which finishes, prints and writes the files; every rank returns the same dict.
    per_class_thresholds (find_optimal_threshold's dict, a {name: threshold} mapping or an fp64 vector; a class it does not name is
    decided at `threshold`): the metrics under them are reported as well -- recounted from the same pass's key store on the device
    routes -- and written as evaluation_results_per_class_thresholds.csv / _overall.json; the return value is then
    (metrics, per_class_metrics)."""
    model.eval(); decoder.eval()

    def finish(ev):
        metrics = _report(ev.compute_metrics(), output_dir, RESULTS_CSV)
        if per_class_thresholds is None:
            return metrics
        vec = threshold_vector(per_class_thresholds, class_names, threshold)
        return metrics, _report(ev.compute_metrics_at(vec), output_dir, PER_CLASS_RESULTS_CSV)
    if device_metrics and group is not None and _use_group(group):
        return _finish_on_rank0(_sharded_device_pass(model, decoder, test_loader, class_names, device, threshold, group), group, finish)
    if device_metrics:
        return finish(_device_pass(model, decoder, test_loader, class_names, device, threshold))
    y_prob, y_true = _probabilities(model, decoder, test_loader, device)
    metrics = _report(_host_metrics(y_prob, y_true, class_names, device, threshold), output_dir, RESULTS_CSV)
    if per_class_thresholds is None:
        return metrics
    vec = threshold_vector(per_class_thresholds, class_names, threshold)
    return metrics, _report(_host_metrics(y_prob, y_true, class_names, device, vec), output_dir, PER_CLASS_RESULTS_CSV)


def find_optimal_threshold(model, decoder, val_loader, class_names, device="cuda", output_dir=None, device_metrics=False, group=None):
    """Per-class and global (macro-F1) threshold search over 0.10, 0.15 ... 0.85, all classes at once per threshold.
    device_metrics=True: from the device evaluator's integer counts (counts only: no key store is kept).
    group: as in evaluate_model -- the counts are merged on rank 0, every rank returns the same dict."""
    model.eval(); decoder.eval()
    if device_metrics and group is not None and _use_group(group):
        def finish(ev):
            return _report_search(ev.optimal_thresholds(), output_dir)
        return _finish_on_rank0(_sharded_device_pass(model, decoder, val_loader, class_names, device, 0.5, group, keys=False), group, finish)
    if device_metrics:
        return _report_search(_device_pass(model, decoder, val_loader, class_names, device, 0.5, capacity=0).optimal_thresholds(), output_dir)
    y_prob, y_true = _probabilities(model, decoder, val_loader, device)
    return _report_search(_host_search(y_prob, y_true, class_names), output_dir)


def evaluate_and_search(model, decoder, loader, class_names, device="cuda", output_dir=None, device_metrics=True, group=None,
                        per_class=False):
    """find_optimal_threshold followed by evaluate_model at the threshold found, in ONE pass over `loader`: the key-keeping device
    evaluator is fed once on the search grid, the search runs on its counts, and the metrics at the global threshold -- with
    per_class=True also those under the searched per-class thresholds -- are recounted from the stored keys
    (DeviceMultiLabelEvaluator.compute_metrics_at); the encoder, about 99 % of the work per image, runs once per image.  Prints and
    writes what the two functions print and write (optimal_thresholds.json, evaluation_results.csv, evaluation_results_overall.json;
    per_class: evaluation_results_per_class_thresholds.csv / _overall.json as well).  Returns (optimal, metrics, per_class_metrics or
    None).  group: the sharded pass with keys, merged and finished on rank 0; every rank returns rank 0's dicts.
    device_metrics=False: the one host probability matrix serves the search and both evaluations."""
    model.eval(); decoder.eval()

    def finish(ev):
        optimal = _report_search(ev.optimal_thresholds(), output_dir)
        metrics = _report(ev.compute_metrics_at(optimal["global_threshold"]), output_dir, RESULTS_CSV)
        pc = None
        if per_class:
            vec = threshold_vector(optimal, class_names, optimal["global_threshold"])
            pc = _report(ev.compute_metrics_at(vec), output_dir, PER_CLASS_RESULTS_CSV)
        return optimal, metrics, pc
    if device_metrics and group is not None and _use_group(group):
        return tuple(_finish_on_rank0(_sharded_device_pass(model, decoder, loader, class_names, device, 0.5, group, keys=True), group, finish))
    if device_metrics:
        return finish(_device_pass(model, decoder, loader, class_names, device, 0.5))
    y_prob, y_true = _probabilities(model, decoder, loader, device)
    optimal = _report_search(_host_search(y_prob, y_true, class_names), output_dir)
    metrics = _report(_host_metrics(y_prob, y_true, class_names, device, optimal["global_threshold"]), output_dir, RESULTS_CSV)
    pc = None
    if per_class:
        vec = threshold_vector(optimal, class_names, optimal["global_threshold"])
        pc = _report(_host_metrics(y_prob, y_true, class_names, device, vec), output_dir, PER_CLASS_RESULTS_CSV)
    return optimal, metrics, pc


# ---- device-side evaluator ---------------------------------------------------------------------------------------------------------
# The state (integer confusion counts for every threshold, support, row statistics, one sort key per class and sample) lives in HBM and
# is fed in stream order (vt_eval_update); nothing is read back per batch.  The host finishes in fp64 from the integers with the formulas
# of MultiLabelEvaluator.compute_metrics / find_optimal_threshold above -- same integers in, same floats out.

THRESHOLD_GRID = np.arange(0.1, 0.9, 0.05)       # find_optimal_threshold's grid


def finish_from_counts(counts, support, row_stats, n, ap=None, micro_ap=None, t_main=0, class_names=None, search=None):
    """Pure numpy: metrics from the evaluator's integers.  counts [c][T][2] = (tp, fp) per class and threshold, support [c],
    row_stats = (exactly matching rows, mismatching elements, non-finite probabilities) at threshold index t_main, n samples,
    ap [c] with nan for a class without a positive (None: the AP keys are left out), micro_ap a float.
    Returns (metrics, optimal): `metrics` is MultiLabelEvaluator.compute_metrics' dict at threshold t_main; `optimal` is
    find_optimal_threshold's dict over the (threshold value, index into T) pairs of `search`, or None without `search`."""
    counts = np.asarray(counts)
    c = counts.shape[0]
    n = int(n)
    if int(row_stats[2]) != 0:
        raise FloatingPointError(f"{int(row_stats[2])} non-finite probabilities reached the evaluator")
    support = np.asarray(support).astype(np.float64)
    tp = counts[:, t_main, 0].astype(np.float64)
    fp = counts[:, t_main, 1].astype(np.float64)
    fn = support - tp
    p, r, f = _prf(tp, fp, fn)
    m = {"accuracy": float(int(row_stats[0]) / n), "hamming_loss": float(int(row_stats[1]) / (n * c))}
    mp, mr, mf = _prf(tp.sum(), fp.sum(), fn.sum())
    w = support / support.sum() if support.sum() > 0 else np.zeros(c)
    for name, per, micro in (("precision", p, mp), ("recall", r, mr), ("f1", f, mf)):
        m[f"{name}_micro"] = float(micro)
        m[f"{name}_macro"] = float(per.mean())
        m[f"{name}_weighted"] = float((per * w).sum())
    if ap is not None:
        ap = np.nan_to_num(np.asarray(ap, dtype=np.float64), nan=0.0)
        m["mAP"] = float(ap.mean())
        m["mAP_micro"] = float(np.nan_to_num(np.float64(micro_ap), nan=0.0))
        m["mAP_weighted"] = float((ap * w).sum())
    per_class = {}
    for i in range(c):
        name = class_names[i] if class_names else f"Class_{i}"
        if support[i] == 0:
            d = {"precision": 0.0, "recall": 0.0, "f1": 0.0, "ap": 0.0, "support": 0}
        elif support[i] == n:                            # every sample positive: AP is 1 by convention
            q = float((tp[i] + fp[i]) / n)
            d = {"precision": q, "recall": 1.0, "f1": 2 * q / (1 + q) if q > 0 else 0.0, "ap": 1.0, "support": int(support[i])}
        else:
            d = {"precision": float(p[i]), "recall": float(r[i]), "f1": float(f[i]),
                 "ap": float(ap[i]) if ap is not None else None, "support": int(support[i])}
        if ap is None:
            del d["ap"]
        per_class[name] = d
    m["per_class"] = per_class
    optimal = None
    if search is not None:
        best_f, best_t = np.zeros(c), np.full(c, 0.5)
        g_f, g_t = 0.0, 0.5
        for t, k in search:
            tp_t = counts[:, k, 0].astype(np.float64)
            fp_t = counts[:, k, 1].astype(np.float64)
            f_t = _prf(tp_t, fp_t, support - tp_t)[2]
            better = (f_t > best_f) & (support > 0)
            best_f[better], best_t[better] = f_t[better], t
            if f_t.mean() > g_f:
                g_f, g_t = float(f_t.mean()), float(t)
        names = class_names if class_names else [f"Class_{i}" for i in range(c)]
        optimal = {"global_threshold": g_t, "global_f1": g_f,
                   "per_class_thresholds": {nm: {"threshold": float(best_t[i]), "f1_score": float(best_f[i])}
                                            for i, nm in enumerate(names)}}
    return m, optimal


class EvalStateBlock:
    """An exported evaluator state: `data` is the block (uint8 device tensor, 256-B aligned, vt_eval_state_bytes(N, T, capacity) bytes),
    `n_seen` the samples it holds, `thresholds` / `t_main` the table it was taken at (host values, compared before a merge)."""

    def __init__(self, data, capacity, n_seen, thresholds, t_main):
        self.data, self.capacity, self.n_seen = data, int(capacity), int(n_seen)
        self.thresholds, self.t_main = np.asarray(thresholds, dtype=np.float64), int(t_main)


def rank_descriptor(ev, error=None):
    """What a rank tells the others before the merge: small, host-only, picklable."""
    if ev is None:
        return {"N": None, "T": None, "t_main": None, "thresholds": None, "keys": None, "n_seen": 0, "error": error or "no evaluator state"}
    return {"N": ev.N, "T": ev.T, "t_main": ev.t_main, "thresholds": ev.thr.tobytes(), "keys": ev.capacity > 0, "n_seen": int(ev.n_seen),
            "error": error}


def check_rank_descriptors(descs):
    """Pure function of the gathered descriptors (identical on every rank, so every rank raises the same exception or none): a rank
    that carries an error, or ranks that disagree on the classes, the thresholds, the operating point or on keeping keys."""
    bad = [(r, d["error"]) for r, d in enumerate(descs) if d["error"]]
    if bad:
        raise RuntimeError("sharded evaluation failed on " + "; ".join(f"rank {r}: {e}" for r, e in bad))
    first = descs[0]
    for key, what in (("N", "number of classes"), ("T", "number of thresholds"), ("t_main", "operating point"),
                      ("thresholds", "threshold table"), ("keys", "key store (capacity 0 on some ranks only)")):
        for r, d in enumerate(descs):
            if d[key] != first[key]:
                shown = "" if key == "thresholds" else f" ({first[key]} vs {d[key]})"
                raise ValueError(f"sharded evaluation: rank {r} differs from rank 0 in the {what}{shown}")
    if sum(d["n_seen"] for d in descs) > 0x7fffffff:
        raise ValueError("sharded evaluation: 2^31 samples or more in all")


def _use_group(group, force_collective=False):
    import torch.distributed as dist
    if not dist.is_available() or not dist.is_initialized():
        return False
    return dist.get_world_size(group) > 1 or force_collective


def merge_across_ranks(ev, group=None, force_collective=False, error=None):
    """Merge every rank's DeviceMultiLabelEvaluator on rank 0: returns the merged evaluator there (a fresh state of capacity sum n_r)
    and None on the other ranks.  Without a process group, or on a one-rank group without `force_collective`, `ev` is returned.
    `error`: what went wrong during this rank's pass (a string), or None -- it travels in the first exchange, so that every rank
    raises the same exception instead of one rank leaving the others waiting in the collective.  Steps: all_gather_object of the host
    descriptors (checked by check_rank_descriptors); every rank exports at the maximum n_seen, so all blocks have one size; ONE
    all-gather of the blocks (all_gather_into_tensor; under gloo the list form, staged through the host); rank 0 merges in rank order.
    Every rank receives the gather: world x block bytes beside its own state (and, on rank 0, the merged one)."""
    import torch.distributed as dist
    if not _use_group(group, force_collective):
        if error:
            raise RuntimeError(f"evaluation failed: {error}")
        return ev
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    descs = [None] * world
    dist.all_gather_object(descs, rank_descriptor(ev, error), group=group)
    check_rank_descriptors(descs)
    counts = [d["n_seen"] for d in descs]
    cap = max(counts) if descs[0]["keys"] else 0
    block = ev.export_state(cap)
    nbytes = block.data.numel()
    if dist.get_backend(group) == "gloo":                    # the rehearsal backend (ranks sharing a GPU) moves host memory
        parts = [torch.empty(nbytes, dtype=torch.uint8) for _ in range(world)]
        dist.all_gather(parts, block.data.cpu(), group=group)
        if rank != 0:
            return None
        gathered = torch.empty(world * nbytes + 256, dtype=torch.uint8, device=ev.device)
        off = -gathered.data_ptr() % 256
        gathered = gathered[off:off + world * nbytes]
        for r, part in enumerate(parts):
            gathered[r * nbytes:(r + 1) * nbytes].copy_(part, non_blocking=False)
    else:
        gathered = torch.empty(world * nbytes + 256, dtype=torch.uint8, device=ev.device)
        off = -gathered.data_ptr() % 256
        gathered = gathered[off:off + world * nbytes]
        dist.all_gather_into_tensor(gathered, block.data, group=group)
        if rank != 0:
            return None
    merged = DeviceMultiLabelEvaluator(ev.class_names, ev.device, thresholds=ev.grid, threshold=ev.threshold,
                                       capacity=sum(counts) if cap else 0, context=ev.ctx)
    merged.merge_from([EvalStateBlock(gathered[r * nbytes:(r + 1) * nbytes], cap, counts[r], ev.thr, ev.t_main) for r in range(world)])
    return merged


def _finish_on_rank0(merged, group, finish):
    """finish(merged) on rank 0 (merged is None elsewhere); its result -- or its exception -- reaches every rank."""
    import torch.distributed as dist
    box = [None, None]
    if merged is not None:
        try:
            box[0] = finish(merged)
        except Exception as e:  # noqa: BLE001 - carried to every rank, raised below
            box[1] = f"{type(e).__name__}: {e}"
    dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
    if box[1]:
        raise RuntimeError(f"sharded evaluation: the finish on rank 0 failed: {box[1]}")
    return box[0]


def _sharded_device_pass(model, decoder, loader, class_names, device, threshold, group, keys=True):
    """This rank's pass + the merge.  An exception of the pass is held back until the first exchange (merge_across_ranks)."""
    ev, error = None, None
    try:
        n = None
        if hasattr(loader, "dataset"):
            try:
                n = max(1, len(loader.dataset))              # a rank without a sample still keeps a (one-column) key store
            except TypeError:
                n = None
        ev = _device_pass(model, decoder, loader, class_names, device, threshold, capacity=(n if keys else 0))
    except Exception as e:  # noqa: BLE001
        error = f"{type(e).__name__}: {e}"
    return merge_across_ranks(ev, group, error=error)


class DeviceMultiLabelEvaluator(MultiLabelEvaluator):
    """MultiLabelEvaluator whose accumulation runs on the GPU (vt_eval_* of the C ABI).  `thresholds` is the search grid (default: the grid
    of find_optimal_threshold, compared in fp64 as numpy compares a float32 array with a float64 scalar); `threshold` is the operating
    point of compute_metrics (compared in fp32, as `y_prob > 0.5` is).  capacity: samples the key store holds -- None grows it
    geometrically, 0 keeps counts only (no average precision)."""

    def __init__(self, class_names, device="cuda", thresholds=None, threshold=0.5, capacity=None, context=None):
        from . import _lib
        self.class_names = list(class_names)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.VTError("DeviceMultiLabelEvaluator runs on a HIP device; MultiLabelEvaluator is the host evaluator")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        grid = THRESHOLD_GRID if thresholds is None else np.asarray(thresholds, dtype=np.float64)
        self.grid = grid
        self.threshold = threshold
        self.thr = np.concatenate([grid, [np.float64(np.float32(threshold))]])
        self.t_main = len(grid)
        if len(self.thr) > 32:
            raise ValueError("at most 31 search thresholds")
        self.ctx = context if context is not None else _lib.Context(self.device.index)
        self.N, self.T = len(self.class_names), len(self.thr)
        self.auto_grow = capacity is None
        self.capacity = 1024 if capacity is None else int(capacity)
        self.reset_metrics()

    def _stream(self):
        import ctypes
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _alloc(self, capacity):
        nbytes = self.ctx.lib.vt_eval_state_bytes(self.N, self.T, capacity)
        if nbytes == 0:
            raise ValueError(f"evaluator state of {self.N} classes x {self.T} thresholds x capacity {capacity} is not supported")
        buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        return buf, (buf.data_ptr() + 255) // 256 * 256, nbytes

    def reset_metrics(self):
        import ctypes
        self.n_seen = 0
        self._buf, self._ptr, self._bytes = self._alloc(self.capacity)
        thr = (ctypes.c_double * self.T)(*self.thr.tolist())
        self.ctx.call("vt_eval_reset", ctypes.c_void_p(self._ptr), self._bytes, self.N, self.T, thr, self.t_main, self.capacity, self._stream())

    def _grow(self, need):
        import ctypes
        cap = self.capacity
        while cap < need:
            cap *= 2
        buf, ptr, nbytes = self._alloc(cap)
        self.ctx.call("vt_eval_grow", ctypes.c_void_p(self._ptr), self._bytes, self.capacity, ctypes.c_void_p(ptr), nbytes, cap, self.N, self.T,
                      self.n_seen, self._stream())
        self._buf.record_stream(torch.cuda.current_stream(self.device))      # the old block is read by the copy just queued
        self._buf, self._ptr, self._bytes, self.capacity = buf, ptr, nbytes, cap

    def update(self, probabilities, targets):
        """probabilities fp32 [B, N], targets [B, N] (positive: > 0); device tensors, or host tensors uploaded without blocking.
        Queues work on the current stream and returns: no host synchronisation."""
        import ctypes
        from . import _lib
        p = probabilities.detach()
        if p.device != self.device:
            p = p.to(self.device, non_blocking=True)
        p = p.to(torch.float32).contiguous()
        y = targets.detach() if isinstance(targets, torch.Tensor) else torch.as_tensor(np.asarray(targets))
        if y.device != self.device:
            y = y.to(self.device, non_blocking=True)
        if y.dtype == torch.bool:
            y = y.view(torch.uint8)
        elif y.dtype not in (torch.float32, torch.uint8):
            y = (y > 0).view(torch.uint8)
        y = y.contiguous()
        if p.dim() != 2 or p.shape[1] != self.N or y.shape != p.shape:
            raise ValueError(f"expected [B, {self.N}] probabilities and targets, got {tuple(p.shape)} and {tuple(y.shape)}")
        dt = _lib.VT_U8 if y.dtype == torch.uint8 else _lib.VT_F32
        for lo in range(0, p.shape[0], 4096):
            pb, yb = p[lo:lo + 4096], y[lo:lo + 4096]
            B = pb.shape[0]
            if self.capacity and self.n_seen + B > self.capacity:
                if not self.auto_grow:
                    raise ValueError(f"evaluator capacity {self.capacity} exceeded by sample {self.n_seen + B}")
                self._grow(self.n_seen + B)
            self.ctx.call("vt_eval_update", ctypes.c_void_p(self._ptr), self._bytes, self.N, self.T, self.t_main, self.capacity,
                          ctypes.c_void_p(pb.data_ptr()), ctypes.c_void_p(yb.data_ptr()), dt, B, self.n_seen, self._stream())
            self.n_seen += B

    def export_state(self, capacity=None):
        """The state as a block of `capacity` key columns (default: n_seen; 0: head only, no keys) -- an EvalStateBlock whose bytes are
        a function of the data only: what a rank sends to the merge.  Queued on the current stream; no host synchronisation."""
        import ctypes
        cap = (self.n_seen if self.capacity else 0) if capacity is None else int(capacity)
        buf, ptr, nbytes = self._alloc(cap)
        self.ctx.call("vt_eval_export", ctypes.c_void_p(self._ptr), self._bytes, self.N, self.T, self.capacity, self.n_seen,
                      ctypes.c_void_p(ptr), nbytes, cap, self._stream())
        off = ptr - buf.data_ptr()
        return EvalStateBlock(buf[off:off + nbytes], cap, self.n_seen, self.thr, self.t_main)

    def merge_from(self, blocks):
        """Append the samples of `blocks` (EvalStateBlock, in the order given) to this state: counts, support and row statistics are
        added, the keys appended with their sample indices moved behind this state's samples -- afterwards the state is what one
        evaluator fed everything in that order would hold.  One vt_eval_merge call (two launches); no host synchronisation."""
        import ctypes
        from . import _lib
        blocks = list(blocks)
        for b in blocks:
            if b.t_main != self.t_main or np.asarray(b.thresholds, dtype=np.float64).tobytes() != self.thr.tobytes():
                raise ValueError("merge_from: a block was taken at other thresholds than this evaluator's")
            if b.data.device != self.device or b.data.dtype != torch.uint8 or not b.data.is_contiguous() or b.data.data_ptr() % 256:
                raise ValueError("merge_from: a block is a contiguous, 256-B aligned uint8 tensor on the evaluator's device")
        total = self.n_seen + sum(b.n_seen for b in blocks)
        if self.capacity and total > self.capacity:
            if not self.auto_grow:
                raise ValueError(f"evaluator capacity {self.capacity} exceeded by the merged {total} samples")
            self._grow(total)
        src = (_lib.EvalSource * len(blocks))(*[_lib.EvalSource(b.data.data_ptr(), b.data.numel(), b.capacity, b.n_seen) for b in blocks])
        self.ctx.call("vt_eval_merge", ctypes.c_void_p(self._ptr), self._bytes, self.N, self.T, self.capacity, self.n_seen, src, len(blocks),
                      self._stream())
        self.n_seen = total

    def read_state(self, with_ap=True):
        """(counts [N][T][2], support [N], row_stats [3], ap [N] or None, micro_ap or None) on the host: the one synchronisation."""
        import ctypes
        if self.n_seen == 0:
            raise ValueError("no data: call update() first")
        counts = torch.empty(self.N, self.T, 2, dtype=torch.int32, pin_memory=True)
        support = torch.empty(self.N, dtype=torch.int32, pin_memory=True)
        row_stats = torch.empty(3, dtype=torch.int64, pin_memory=True)
        s = self._stream()
        vp = lambda t: ctypes.c_void_p(t.data_ptr())
        self.ctx.call("vt_eval_read_counts", ctypes.c_void_p(self._ptr), self._bytes, self.N, self.T, self.capacity, vp(counts),
                      counts.numel() * 4, vp(support), support.numel() * 4, vp(row_stats), 24, s)
        ap_host = micro = None
        keys_host = None
        if with_ap and self.capacity:
            ws_bytes = self.ctx.lib.vt_eval_ap_workspace_bytes(self.N, self.n_seen)
            ap = torch.empty(self.N + 1, dtype=torch.float64, device=self.device)
            if ws_bytes:
                ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device=self.device)
                wp = ctypes.c_void_p((ws.data_ptr() + 255) // 256 * 256)
                mp = ctypes.c_void_p(ap.data_ptr() + 8 * self.N)
            else:                                           # n * c >= 2^31: the store comes back once and the host routine ranks it
                wp, mp = ctypes.c_void_p(0), ctypes.c_void_p(0)
            self.ctx.call("vt_eval_average_precision", ctypes.c_void_p(self._ptr), self._bytes, self.N, self.T, self.capacity, self.n_seen,
                          vp(ap), self.N * 8, mp, wp, ws_bytes, s)
            ap_host = torch.empty(self.N + 1, dtype=torch.float64, pin_memory=True)
            ap_host.copy_(ap, non_blocking=True)
            if not ws_bytes:
                head = self.ctx.lib.vt_eval_state_bytes(self.N, self.T, 0)
                off = self._ptr - self._buf.data_ptr() + head
                keys_host = self._buf[off:off + self.N * self.capacity * 8].view(torch.int64).view(self.N, self.capacity)[:, :self.n_seen].cpu()
        torch.cuda.current_stream(self.device).synchronize()
        if ap_host is not None:
            a = ap_host.numpy()
            ap_host, micro = a[:self.N].copy(), float(a[self.N])
            if keys_host is not None:
                micro = self._host_micro_ap(keys_host.numpy().view(np.uint64))
        return (counts.numpy().view(np.uint32).copy(), support.numpy().view(np.uint32).copy(), row_stats.numpy().view(np.uint64).copy(),
                ap_host, micro)

    @staticmethod
    def _host_micro_ap(keys):
        hi = (keys >> np.uint64(32)).astype(np.uint32)
        bits = np.where(hi & np.uint32(0x80000000), hi & np.uint32(0x7fffffff), ~hi)
        prob = bits.view(np.float32).reshape(-1, 1)
        return float(_average_precision((keys & np.uint64(1)).reshape(-1, 1) > 0, prob)[0])

    def compute_metrics(self, threshold=None):
        """MultiLabelEvaluator.compute_metrics' dict at the constructor's `threshold`.  Without a key store (capacity 0) the AP keys are
        left out rather than invented."""
        if threshold is not None and np.float32(threshold) != np.float32(self.threshold):
            raise ValueError(f"the counts were taken at threshold {self.threshold}; pass threshold= to the constructor")
        counts, support, row_stats, ap, micro = self.read_state()
        if ap is None:
            import warnings
            warnings.warn("DeviceMultiLabelEvaluator(capacity=0) keeps no ranking: mAP, mAP_micro, mAP_weighted and the per-class ap are omitted")
        return finish_from_counts(counts, support, row_stats, self.n_seen, ap, micro, self.t_main, self.class_names)[0]

    def _recount_async(self, thresholds):
        """Queue vt_eval_recount on the current stream: (counts int32 [N][2], row_stats int64 [3]) pinned tensors, valid after a sync."""
        import ctypes
        if self.n_seen == 0:
            raise ValueError("no data: call update() first")
        if not self.capacity:
            raise ValueError("recount needs the key store: this evaluator keeps counts only (capacity 0)")
        thr = np.asarray(thresholds, dtype=np.float64)
        if thr.ndim == 0:
            thr = np.full(self.N, thr)
        if thr.shape != (self.N,):
            raise ValueError(f"expected a scalar or {self.N} thresholds, got an array of shape {thr.shape}")
        thr_dev = torch.from_numpy(np.ascontiguousarray(thr)).to(self.device)
        counts = torch.empty(self.N, 2, dtype=torch.int32, pin_memory=True)
        row_stats = torch.empty(3, dtype=torch.int64, pin_memory=True)
        ws_bytes = self.ctx.lib.vt_eval_recount_workspace_bytes(self.N, self.n_seen)
        ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device=self.device)
        vp = lambda t: ctypes.c_void_p(t.data_ptr())
        self.ctx.call("vt_eval_recount", ctypes.c_void_p(self._ptr), self._bytes, self.N, self.T, self.capacity, self.n_seen, vp(thr_dev),
                      vp(counts), counts.numel() * 4, vp(row_stats), 24, ctypes.c_void_p((ws.data_ptr() + 255) // 256 * 256), ws_bytes,
                      self._stream())
        stream = torch.cuda.current_stream(self.device)
        thr_dev.record_stream(stream); ws.record_stream(stream)
        return counts, row_stats

    def recount(self, thresholds):
        """Re-decide every stored prediction as (double)p > thresholds[class] (a scalar serves every class; fp64, compared as given)
        from the key store: (counts uint32 [N][2] = (tp, fp), row_stats uint64 [3] = (exactly matching rows, mismatching elements,
        non-finite probabilities)).  The state is not modified; the result does not depend on whether the rows have been ranked."""
        counts, row_stats = self._recount_async(thresholds)
        torch.cuda.current_stream(self.device).synchronize()
        return counts.numpy().view(np.uint32).copy(), row_stats.numpy().view(np.uint64).copy()

    def compute_metrics_at(self, thresholds, with_ap=True):
        """compute_metrics' dict at another operating point, recounted from the key store.  A scalar is an operating point as the
        constructor's `threshold` is (compared in fp32, as `y_prob > 0.5` is: it is rounded to fp32 first); an array holds one
        threshold per class, compared in fp64 as given (numpy's float32 matrix > float64 row)."""
        thr = np.asarray(thresholds, dtype=np.float64)
        if thr.ndim == 0:
            thr = np.float64(np.float32(thr))
        counts, row_stats = self._recount_async(thr)
        _, support, _, ap, micro = self.read_state(with_ap=with_ap)          # (synchronises: the recount's outputs are final too)
        counts = counts.numpy().view(np.uint32).reshape(self.N, 1, 2)
        return finish_from_counts(counts, support, row_stats.numpy().view(np.uint64), self.n_seen, ap, micro, 0, self.class_names)[0]

    def optimal_thresholds(self):
        """find_optimal_threshold's dict over the search grid."""
        counts, support, row_stats, _, _ = self.read_state(with_ap=False)
        search = [(t, k) for k, t in enumerate(self.grid)]
        return finish_from_counts(counts, support, row_stats, self.n_seen, None, None, self.t_main, self.class_names, search)[1]


def _raise_on_word(st):
    if st & 1:
        raise FloatingPointError("non-finite activations in the encoder: the fp16 residual-stream storage overflowed "
                                 "(vt_set_flag(ctx, 4, 0) stores it as fp32) or the checkpoint holds inf / NaN")
    if st & 2:
        raise FloatingPointError("fp8 mode: activations exceeded the e4m3 range and were clamped (vt_set_flag(ctx, 11, 0) returns to bf16)")


def _device_pass(model, decoder, loader, class_names, device, threshold, capacity=None):
    """encode -> decoder -> sigmoid -> DeviceMultiLabelEvaluator.update, batch after batch without a host synchronisation: the encoder's
    health word is copied in stream order into pinned memory (vt_status_async) and looked at one batch late and at the end."""
    import ctypes
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    vae = getattr(model, "vae", model)
    ctx = vae._context() if hasattr(vae, "_context") else None
    if capacity is None and hasattr(loader, "dataset"):
        try:
            capacity = len(loader.dataset)
        except TypeError:
            capacity = None
    ev = DeviceMultiLabelEvaluator(class_names, dev, threshold=threshold, capacity=capacity, context=ctx)
    had_check = getattr(model, "check_finite", None)
    if had_check is not None:
        model.check_finite = False
    # two pinned words and their numpy views, made before the loop: batch n's word is looked at while batch n + 1 is queued
    words = [torch.zeros(1, dtype=torch.int32, pin_memory=True) for _ in range(2)] if ctx is not None else []
    views = [w.numpy() for w in words]
    pending, i = None, 0
    try:
        with torch.no_grad():
            for batch in loader:
                lat = model.encode(batch["pixel_values"].to(dev, non_blocking=True))
                ev.update(torch.sigmoid(decoder(lat)), batch["labels"])
                if ctx is not None:
                    stream = torch.cuda.current_stream(dev)
                    ctx.call("vt_status_async", 1, ctypes.c_void_p(words[i & 1].data_ptr()), ctypes.c_void_p(stream.cuda_stream))
                    done = torch.cuda.Event()
                    done.record(stream)
                    if pending is not None:                  # batch n - 1's word: its event passed while batch n was queued
                        pending[1].synchronize()
                        _raise_on_word(int(pending[0][0]))
                    pending = (views[i & 1], done)
                    i += 1
            if pending is not None:
                pending[1].synchronize()
                _raise_on_word(int(pending[0][0]))
    finally:
        if had_check is not None:
            model.check_finite = had_check
    return ev


# ---- checkpoint sweep: several decoders scored per encode, validation loss on the device --------------------------------------------
VALIDATION_LOSS_JSON = "validation_loss.json"


def _sweep_pass(model, decoders, loader, class_names, device, threshold, capacity, loss_kw):
    """_device_pass for several decoders: per batch ONE model.encode, then per decoder its logits, one DeviceLossAccumulator.update on
    them (loss_kw is not None) and one DeviceMultiLabelEvaluator.update on their sigmoid -- no host synchronisation per batch; the
    encoder's health word is read one batch late, as in _device_pass.  Returns (evaluators, accumulators or Nones)."""
    import ctypes
    from .losses import DeviceLossAccumulator
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    vae = getattr(model, "vae", model)
    ctx = vae._context() if hasattr(vae, "_context") else None
    if capacity is None and hasattr(loader, "dataset"):
        try:
            capacity = len(loader.dataset)
        except TypeError:
            capacity = None
    evs = [DeviceMultiLabelEvaluator(class_names, dev, threshold=threshold, capacity=capacity, context=ctx) for _ in decoders]
    accs = [DeviceLossAccumulator(len(class_names), dev, context=ctx, **loss_kw) if loss_kw is not None else None for _ in decoders]
    had_check = getattr(model, "check_finite", None)
    if had_check is not None:
        model.check_finite = False
    words = [torch.zeros(1, dtype=torch.int32, pin_memory=True) for _ in range(2)] if ctx is not None else []
    views = [w.numpy() for w in words]
    pending, i = None, 0
    try:
        with torch.no_grad():
            for batch in loader:
                lat = model.encode(batch["pixel_values"].to(dev, non_blocking=True))
                labels = batch["labels"]
                if isinstance(labels, torch.Tensor) and labels.device != dev:
                    labels = labels.to(dev, non_blocking=True)       # one upload for every decoder's two updates
                for decoder, ev, acc in zip(decoders, evs, accs):
                    logits = decoder(lat)
                    if acc is not None:
                        acc.update(logits, labels)
                    ev.update(torch.sigmoid(logits), labels)
                if ctx is not None:
                    stream = torch.cuda.current_stream(dev)
                    ctx.call("vt_status_async", 1, ctypes.c_void_p(words[i & 1].data_ptr()), ctypes.c_void_p(stream.cuda_stream))
                    done = torch.cuda.Event()
                    done.record(stream)
                    if pending is not None:
                        pending[1].synchronize()
                        _raise_on_word(int(pending[0][0]))
                    pending = (views[i & 1], done)
                    i += 1
            if pending is not None:
                pending[1].synchronize()
                _raise_on_word(int(pending[0][0]))
    finally:
        if had_check is not None:
            model.check_finite = had_check
    return evs, accs


def _merge_losses_across_ranks(accs, group):
    """ONE all-gather of this rank's loss blocks (every accumulator's block, concatenated); on rank 0 every accumulator's blocks are
    merged IN RANK ORDER into a fresh accumulator, which is returned in its place; None on the other ranks."""
    import torch.distributed as dist
    from .losses import DeviceLossAccumulator, LossStateBlock, exchange_loss_blocks
    blocks = [a.export_state() for a in accs]
    nbytes = blocks[0].data.numel()                          # (a multiple of 256: the parts of the gather stay 256-B aligned)
    parts = exchange_loss_blocks(torch.cat([b.data for b in blocks]), group)
    if dist.get_rank(group) != 0:
        return None
    merged = []
    for k, a in enumerate(accs):
        m = DeviceLossAccumulator(a.N, a.device, a.alpha, a.gamma, a.class_weights, context=a.ctx)
        stage = torch.empty(len(parts) * nbytes + 256, dtype=torch.uint8, device=a.device)
        off = -stage.data_ptr() % 256
        stage = stage[off:off + len(parts) * nbytes]
        for r, part in enumerate(parts):
            stage[r * nbytes:(r + 1) * nbytes].copy_(part[k * nbytes:(k + 1) * nbytes], non_blocking=False)
        m.merge_from([LossStateBlock(stage[r * nbytes:(r + 1) * nbytes], a.alpha, a.gamma, a.class_weights) for r in range(len(parts))])
        merged.append(m)
    return merged


def sweep_checkpoints(model, decoders, loader, class_names, device="cuda", output_dirs=None, threshold=None, per_class=False,
                      per_class_thresholds=None, group=None, val_loss=True, focal_alpha=1.0, focal_gamma=2.0, class_weights=None,
                      selected_loss="bce"):
    """Score several decoders of one architecture in ONE pass over `loader`: the encoder -- nearly all of the work per image -- runs
    once per batch, and every decoder gets its own key-keeping device evaluator and (val_loss) its own DeviceLossAccumulator, fed the
    logits: train_decoder.py's validation loss (train_decoder.py:218-241) beside the metrics.
    threshold=None: per decoder the one-pass finish of evaluate_and_search (search, metrics at the global threshold found, per_class:
    also under the searched per-class thresholds); a float: evaluate_model's finish at that threshold (per_class_thresholds as there).
    The files evaluate_and_search / evaluate_model write go to output_dirs[i], plus validation_loss.json (losses.loss_report;
    `selected_loss` is the one the reference's rule picks: losses.select_loss).  class_weights: losses.class_balanced_weights(...) of
    the WHOLE label set, or None (no class-balanced loss).  group: every rank passes its share of the data; the evaluators are merged
    with merge_across_ranks, the loss blocks with one all-gather and vt_loss_merge in rank order, and rank 0 finishes; every rank
    returns rank 0's result.  Returns one dict per decoder: optimal (None with a threshold), metrics, per_class_metrics (or None),
    loss (losses.finish_state's dict, or None).  Memory: every decoder keeps its own key store of N x capacity x 8 bytes."""
    from .losses import loss_report
    model.eval()
    for d in decoders:
        d.eval()
    decoders = list(decoders)
    output_dirs = list(output_dirs) if output_dirs is not None else [None] * len(decoders)
    if len(output_dirs) != len(decoders) or not decoders:
        raise ValueError("sweep_checkpoints: one output directory (or None) per decoder, and at least one decoder")
    loss_kw = {"alpha": focal_alpha, "gamma": focal_gamma, "class_weights": class_weights} if val_loss else None

    def finish_one(ev, acc, output_dir):
        if threshold is None:
            optimal = _report_search(ev.optimal_thresholds(), output_dir)
            metrics = _report(ev.compute_metrics_at(optimal["global_threshold"]), output_dir, RESULTS_CSV)
            pc = None
            if per_class:
                pc = _report(ev.compute_metrics_at(threshold_vector(optimal, class_names, optimal["global_threshold"])), output_dir,
                             PER_CLASS_RESULTS_CSV)
        else:
            optimal, pc = None, None
            metrics = _report(ev.compute_metrics(), output_dir, RESULTS_CSV)
            if per_class_thresholds is not None:
                pc = _report(ev.compute_metrics_at(threshold_vector(per_class_thresholds, class_names, threshold)), output_dir,
                             PER_CLASS_RESULTS_CSV)
        loss = None
        if acc is not None:
            loss = acc.read(class_names)
            report = loss_report(loss, selected_loss)
            print(f"validation loss ({selected_loss}) {report['val_loss']:.6f} over {loss['steps']} batches"
                  + (f"; {loss['non_finite']} non-finite logits" if loss["non_finite"] else ""))
            if output_dir:
                os.makedirs(output_dir, exist_ok=True)
                with open(os.path.join(output_dir, VALIDATION_LOSS_JSON), "w", encoding="utf-8") as fh:
                    json.dump(report, fh, indent=2, ensure_ascii=False)
        return {"optimal": optimal, "metrics": metrics, "per_class_metrics": pc, "loss": loss}

    def finish(pairs):
        return [finish_one(ev, acc, d) for (ev, acc), d in zip(pairs, output_dirs)]
    t = 0.5 if threshold is None else threshold
    if group is not None and _use_group(group):
        evs, accs, error = [None] * len(decoders), None, None
        try:
            n = None
            if hasattr(loader, "dataset"):
                try:
                    n = max(1, len(loader.dataset))
                except TypeError:
                    n = None
            evs, accs = _sweep_pass(model, decoders, loader, class_names, device, t, n, loss_kw)
        except Exception as e:  # noqa: BLE001 - travels in the first exchange, so that every rank raises
            error = f"{type(e).__name__}: {e}"
        merged = [merge_across_ranks(ev, group, error=error) for ev in evs]
        merged_accs = _merge_losses_across_ranks(accs, group) if loss_kw is not None else None
        pairs = None if merged[0] is None else list(zip(merged, merged_accs if merged_accs is not None else [None] * len(merged)))
        return _finish_on_rank0(pairs, group, finish)
    evs, accs = _sweep_pass(model, decoders, loader, class_names, device, t, None, loss_kw)
    return finish(list(zip(evs, accs)))
