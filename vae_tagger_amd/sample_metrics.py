"""Per-image (example-based) precision / recall / F1: the numbers of the reference's batch_inference_test.py (calculate_metrics,
batch_inference_test.py:63-137) -- for every image precision_i = |true & pred| / |pred|, recall_i = |true & pred| / |true|, F1_i and
the exact match, averaged over the images -- from the [n][N] probability matrix instead of one `infer_full.py` process per picture.

    sample_metrics_host      numpy fp64, sequential in-order sums: the host route and the test oracle
    DeviceSampleEvaluator    the same on the GPU (vt_sample_* of the C ABI), fed batch by batch in stream order

Conventions (the reference's): precision is 0 when nothing is predicted, recall is 1 when the image has no true tag,
F1 = 2 P R / (P + R) or 0 when P + R = 0, exact match when the predicted set equals the true set.  `true_extra[i]` counts image i's
ground-truth tags that are not in the tag list: they are in |true| (so they lower recall and rule out an exact match) but can never be
predicted.  A prediction is p > thr ("gt", the evaluator's rule) or p >= thr ("ge", infer_full.py's), decided in fp64; a NaN never predicts.
"""
import ctypes

import numpy as np

RULES = {"gt": 0, "ge": 1}
MAX_T, MAX_B = 32, 4096
SEARCH_GRID = np.round(np.arange(1, 20) * 0.05, 2)          # --search: 0.05 ... 0.95


def _rule(rule):
    if rule not in RULES:
        raise ValueError(f"rule must be 'gt' or 'ge', got {rule!r}")
    return RULES[rule]


def per_image_values(tp, predicted, true):
    """(precision, recall, f1, exact) fp64 / bool arrays from integer tallies, with the reference's conventions."""
    tp, predicted, true = (np.asarray(a, dtype=np.float64) for a in (tp, predicted, true))
    with np.errstate(divide="ignore", invalid="ignore"):
        P = np.where(predicted > 0, tp / predicted, 0.0)
        R = np.where(true > 0, tp / true, 1.0)
        F = np.where(P + R > 0, 2 * P * R / (P + R), 0.0)
    return P, R, F, (tp == predicted) & (predicted == true)


def sample_tallies_host(probs, labels, thresholds, rule, true_extra=None):
    """(true uint32 [n], rows uint32 [n][T][2] = (tp, predicted)).  `thresholds`: [T] (one threshold for every class) or [T][N]."""
    p = np.asarray(probs, dtype=np.float32).astype(np.float64)
    y = np.asarray(labels) > 0
    thr = np.asarray(thresholds, dtype=np.float64)
    thr = thr.reshape(-1, 1) if thr.ndim <= 1 else thr
    with np.errstate(invalid="ignore"):
        pred = (p[:, None, :] >= thr[None]) if _rule(rule) else (p[:, None, :] > thr[None])          # [n][T][N]; NaN compares false
    true = y.sum(axis=1).astype(np.uint32)
    if true_extra is not None:
        true = true + np.asarray(true_extra, dtype=np.uint32)
    rows = np.stack([(pred & y[:, None, :]).sum(axis=2), pred.sum(axis=2)], axis=2).astype(np.uint32)
    return true, rows


def finish_host(true, rows, nonfinite=0):
    """The per-threshold dicts of DeviceSampleEvaluator.finish from the integer tallies: sequential in-order fp64 sums."""
    n, T = rows.shape[0], rows.shape[1]
    out = []
    for t in range(T):
        P, R, F, exact = per_image_values(rows[:, t, 0], rows[:, t, 1], true)
        sp = sr = sf = 0.0
        for i in range(n):
            sp += float(P[i]); sr += float(R[i]); sf += float(F[i])
        out.append(_finish_dict(n, sp, sr, sf, int(exact.sum()), int((rows[:, t, 1] == 0).sum()), int((np.asarray(true) == 0).sum()), int(nonfinite)))
    return out


def _finish_dict(n, sp, sr, sf, exact, no_pred, no_true, nonfinite):
    d = {"avg_precision": sp / n if n else 0, "avg_recall": sr / n if n else 0, "avg_f1": sf / n if n else 0,
         "exact_match_rate": exact / n if n else 0,
         # scikit-learn's recall_score(average="samples") scores an image without a true tag 0 where the reference scores it 1
         "samples_recall_sklearn": (sr - no_true) / n if n else 0,
         "total_images": n, "sum_precision": sp, "sum_recall": sr, "sum_f1": sf, "exact_matches": exact,
         "images_without_prediction": no_pred, "images_without_true_tag": no_true, "nonfinite_probabilities": nonfinite}
    return d


def sample_metrics_host(probs, labels, thresholds, rule, true_extra=None):
    """probs fp32 [n][N], labels [n][N] (positive: > 0), thresholds [T] -> a list of T dicts (see DeviceSampleEvaluator.finish)."""
    p = np.asarray(probs, dtype=np.float32)
    true, rows = sample_tallies_host(p, labels, thresholds, rule, true_extra)
    return finish_host(true, rows, int((~np.isfinite(p)).sum()))


def best_threshold(results):
    """Index of the highest avg_f1, the lowest index on ties."""
    best = 0
    for k, r in enumerate(results):
        if r["avg_f1"] > results[best]["avg_f1"]:
            best = k
    return best


def sample_layout(T, capacity):
    """Byte offsets of the device block's sections (csrc/vt_samples.h)."""
    al = lambda x: (x + 255) // 256 * 256
    l = {"thr": 0, "totals": al(8 * MAX_T)}
    l["true"] = l["totals"] + al(8 * 32 + 4 * MAX_B)
    l["head_bytes"] = l["true"]
    l["rows"] = l["true"] + al(4 * capacity)
    l["total"] = l["rows"] + al(8 * T * capacity)
    return l


class DeviceSampleEvaluator:
    """Per-image tallies on the GPU for up to 32 thresholds at once.  capacity: images the state holds -- None grows it by doubling
    through a device copy.  update() queues work on the current stream and returns; finish() / per_image() synchronise once."""

    def __init__(self, thresholds, rule="ge", device="cuda", capacity=None, context=None):
        import torch
        from . import _lib
        self.thresholds = np.atleast_1d(np.asarray(thresholds, dtype=np.float64))
        if self.thresholds.ndim != 1 or not 1 <= len(self.thresholds) <= MAX_T:
            raise ValueError(f"1 to {MAX_T} thresholds expected")
        self.rule, self._rule = rule, _rule(rule)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.VTError("DeviceSampleEvaluator runs on a HIP device; sample_metrics_host is the host route")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.ctx = context if context is not None else _lib.Context(self.device.index)
        self.T = len(self.thresholds)
        self.auto_grow = capacity is None
        self.capacity = 1024 if capacity is None else int(capacity)
        self.n_seen = 0
        self._buf, self._ptr, self._bytes = self._alloc(self.capacity)
        thr = (ctypes.c_double * self.T)(*self.thresholds.tolist())
        self.ctx.call("vt_sample_reset", ctypes.c_void_p(self._ptr), self._bytes, self.T, thr, self._rule, self.capacity, self._stream())

    def _stream(self):
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _alloc(self, capacity):
        import torch
        nbytes = self.ctx.lib.vt_sample_state_bytes(self.T, capacity)
        if nbytes == 0:
            raise ValueError(f"sample state of {self.T} thresholds x capacity {capacity} is not supported")
        buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        return buf, (buf.data_ptr() + 255) // 256 * 256, nbytes

    def _view(self, buf, ptr, lo, nbytes):
        off = ptr - buf.data_ptr() + lo
        return buf[off:off + nbytes]

    def rows_view(self):
        """The state's rows as a device int32 view [capacity][T][2] = (tp, predicted): valid in stream order, until the state grows."""
        import torch
        lay = sample_layout(self.T, self.capacity)
        return self._view(self._buf, self._ptr, lay["rows"], 8 * self.T * self.capacity).view(torch.int32).view(self.capacity, self.T, 2)

    def _grow(self, need):
        import torch
        cap = self.capacity
        while cap < need:
            cap *= 2
        buf, ptr, nbytes = self._alloc(cap)
        lo, ln = sample_layout(self.T, self.capacity), sample_layout(self.T, cap)
        for a, b, n in ((0, 0, lo["head_bytes"]), (lo["true"], ln["true"], 4 * self.n_seen), (lo["rows"], ln["rows"], 8 * self.T * self.n_seen)):
            if n:
                self._view(buf, ptr, b, n).copy_(self._view(self._buf, self._ptr, a, n), non_blocking=True)
        self._buf.record_stream(torch.cuda.current_stream(self.device))
        self._buf, self._ptr, self._bytes, self.capacity = buf, ptr, nbytes, cap

    def _extra(self, true_extra, n):
        import torch
        if true_extra is None:
            return None
        e = true_extra if isinstance(true_extra, torch.Tensor) else torch.as_tensor(np.asarray(true_extra, dtype=np.int64))
        if e.shape != (n,):
            raise ValueError(f"true_extra: {n} counts expected, got shape {tuple(e.shape)}")
        return e.to(self.device, torch.int32, non_blocking=True).contiguous()         # (the bits of a uint32 count below 2^31)

    def update(self, probs, labels, true_extra=None):
        """probs fp32 [B, N], labels [B, N] (positive: > 0; float32 / uint8 / bool), true_extra [B] counts or None; device tensors, or
        host tensors / arrays uploaded without blocking."""
        import torch
        from . import _lib
        p = probs.detach() if isinstance(probs, torch.Tensor) else torch.as_tensor(np.asarray(probs))
        p = p.to(self.device, torch.float32, non_blocking=True).contiguous()
        y = labels.detach() if isinstance(labels, torch.Tensor) else torch.as_tensor(np.asarray(labels))
        if y.device != self.device:
            y = y.to(self.device, non_blocking=True)
        if y.dtype == torch.bool:
            y = y.view(torch.uint8)
        elif y.dtype not in (torch.float32, torch.uint8):
            y = (y > 0).view(torch.uint8)
        y = y.contiguous()
        if p.dim() != 2 or y.shape != p.shape:
            raise ValueError(f"expected [B, N] probabilities and labels, got {tuple(p.shape)} and {tuple(y.shape)}")
        e = self._extra(true_extra, p.shape[0])
        dt = _lib.VT_U8 if y.dtype == torch.uint8 else _lib.VT_F32
        N = p.shape[1]
        for lo in range(0, p.shape[0], MAX_B):
            pb, yb = p[lo:lo + MAX_B], y[lo:lo + MAX_B]
            eb = e[lo:lo + MAX_B] if e is not None else None
            B = pb.shape[0]
            if self.n_seen + B > self.capacity:
                if not self.auto_grow:
                    raise ValueError(f"sample evaluator capacity {self.capacity} exceeded by image {self.n_seen + B}")
                self._grow(self.n_seen + B)
            self.ctx.call("vt_sample_update", ctypes.c_void_p(self._ptr), self._bytes, self.T, self.capacity, ctypes.c_void_p(pb.data_ptr()),
                          ctypes.c_void_p(yb.data_ptr()), dt, ctypes.c_void_p(eb.data_ptr() if eb is not None else 0), B, N, self.n_seen,
                          self._stream())
            self.n_seen += B

    @classmethod
    def from_evaluator(cls, dev_eval, class_thresholds, rule="gt", true_extra=None):
        """The per-image tallies under ONE THRESHOLD PER CLASS (a scalar serves every class) from the key store of a
        DeviceMultiLabelEvaluator (vt_sample_from_keys): a T = 1 evaluator holding dev_eval.n_seen images.  dev_eval is only read."""
        import torch
        if not dev_eval.capacity:
            raise ValueError("from_evaluator needs the key store: this evaluator keeps counts only (capacity 0)")
        thr = np.asarray(class_thresholds, dtype=np.float64)
        if thr.ndim == 0:
            thr = np.full(dev_eval.N, thr)
        if thr.shape != (dev_eval.N,):
            raise ValueError(f"expected a scalar or {dev_eval.N} thresholds, got an array of shape {thr.shape}")
        self = cls([np.nan], rule, dev_eval.device, capacity=max(1, dev_eval.n_seen), context=dev_eval.ctx)
        self.class_thresholds = thr
        thr_dev = torch.from_numpy(np.ascontiguousarray(thr)).to(self.device)
        e = self._extra(true_extra, dev_eval.n_seen)
        self.ctx.call("vt_sample_from_keys", ctypes.c_void_p(dev_eval._ptr), dev_eval._bytes, dev_eval.N, dev_eval.T, dev_eval.capacity,
                      dev_eval.n_seen, ctypes.c_void_p(thr_dev.data_ptr()), self._rule, ctypes.c_void_p(e.data_ptr() if e is not None else 0),
                      ctypes.c_void_p(self._ptr), self._bytes, self.capacity, self._stream())
        thr_dev.record_stream(torch.cuda.current_stream(self.device))
        self.n_seen = dev_eval.n_seen
        return self

    def finish_raw(self):
        """vt_sample_finish's output block as a pinned uint8 tensor, valid after a synchronisation of the current stream."""
        import torch
        nbytes = self.ctx.lib.vt_sample_finish_bytes(self.T)
        out = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        self.ctx.call("vt_sample_finish", ctypes.c_void_p(self._ptr), self._bytes, self.T, self.capacity, self.n_seen,
                      ctypes.c_void_p(out.data_ptr()), nbytes, self._stream())
        return out

    def finish(self):
        """A dict per threshold: avg_precision, avg_recall, avg_f1, exact_match_rate, samples_recall_sklearn, total_images (and the raw
        sums and counts they come from).  Synchronises the current stream."""
        import torch
        raw = self.finish_raw()
        torch.cuda.current_stream(self.device).synchronize()
        a = raw.numpy()
        T = self.T
        sums = a[:24 * T].view(np.float64).reshape(T, 3)
        counts = a[24 * T:40 * T].view(np.uint64).reshape(T, 2)
        once = a[40 * T:40 * T + 16].view(np.uint64)
        return [_finish_dict(self.n_seen, float(sums[t, 0]), float(sums[t, 1]), float(sums[t, 2]), int(counts[t, 0]), int(counts[t, 1]),
                             int(once[0]), int(once[1])) for t in range(T)]

    def read_rows(self):
        """(true uint32 [n], rows uint32 [n][T][2] = (tp, predicted)) on the host.  Synchronises the current stream."""
        import torch
        n = self.n_seen
        true = torch.empty(max(n, 1), dtype=torch.int32, pin_memory=True)
        rows = torch.empty(max(n, 1), self.T, 2, dtype=torch.int32, pin_memory=True)
        self.ctx.call("vt_sample_read_rows", ctypes.c_void_p(self._ptr), self._bytes, self.T, self.capacity, n, ctypes.c_void_p(true.data_ptr()),
                      true.numel() * 4, ctypes.c_void_p(rows.data_ptr()), rows.numel() * 4, self._stream())
        torch.cuda.current_stream(self.device).synchronize()
        return true.numpy().view(np.uint32)[:n].copy(), rows.numpy().view(np.uint32)[:n].copy()

    def per_image(self):
        """The per-image report: arrays true [n], tp / predicted [n][T], precision / recall / f1 fp64 [n][T], exact_match bool [n][T]."""
        true, rows = self.read_rows()
        P, R, F, exact = per_image_values(rows[:, :, 0], rows[:, :, 1], true[:, None])
        return {"true": true, "tp": rows[:, :, 0], "predicted": rows[:, :, 1], "precision": P, "recall": R, "f1": F, "exact_match": exact}

    def best_threshold(self, results=None):
        return best_threshold(self.finish() if results is None else results)
