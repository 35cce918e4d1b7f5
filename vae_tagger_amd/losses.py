"""Validation loss of the decoder: the number train_decoder.py keeps the best checkpoint by (train_decoder.py:218-241), for the three
losses it chooses from -- nn.BCEWithLogitsLoss, FocalLoss and ClassBalancedLoss (improved_losses.py:39-72).  Forward only.

Host side: numpy fp64 mirrors of the three losses, the class-balanced weights exactly as the reference computes them, a host model of
the device state block (HostLossState: same layout, same read-out) and the pure-Python parts of the checkpoint sweep (directory names,
ranking).  Device side: DeviceLossAccumulator, fed the decoder's logits batch by batch (vt_loss_* of the C ABI); nothing is read back
per batch.
"""
import os

import numpy as np

LOSS_NAMES = ("bce", "focal", "class_balanced")


# ---- numpy fp64 mirrors ---------------------------------------------------------------------------------------------------------------
def bce_elements(logits, labels):
    """binary_cross_entropy_with_logits(reduction='none') in fp64: max(x, 0) - x y + log1p(exp(-|x|)).  A label is used as its value."""
    x = np.asarray(logits).astype(np.float64)
    y = np.asarray(labels).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.maximum(x, 0.0) - x * y + np.log1p(np.exp(-np.abs(x)))


def focal_elements(logits, labels, alpha=1.0, gamma=2.0):
    """FocalLoss(reduction='none') in fp64: alpha (1 - exp(-bce))^gamma bce."""
    bce = bce_elements(logits, labels)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.float64(alpha) * np.power(1.0 - np.exp(-bce), np.float64(gamma)) * bce


def bce_loss(logits, labels):
    """nn.BCEWithLogitsLoss()(logits, labels): the mean over every element."""
    return float(bce_elements(logits, labels).mean())


def focal_loss(logits, labels, alpha=1.0, gamma=2.0):
    """FocalLoss(alpha, gamma)(logits, labels)."""
    return float(focal_elements(logits, labels, alpha, gamma).mean())


def class_balanced_weights(samples_per_class, beta=0.9999):
    """ClassBalancedLoss' class weights, computed as the reference computes them (improved_losses.py:66-69): numpy
    (1 - beta) / (1 - beta**n), normalised to sum to the number of classes, then ROUNDED TO fp32 (the reference builds a float32
    tensor); returned as float32 -- bit for bit the reference's tensor when every class has a sample.
    A class without a sample has 1 - beta**0 = 0 and gets an INFINITE weight; the sum is then infinite and every populated class's
    weight normalises to 0.  The reference's own normalisation goes on to divide that infinite weight by the infinite sum (NaN), so
    its loss is NaN for such a distribution; here the weight stays inf and the class-balanced loss is reported as infinite.  Either
    way the loss is not finite and nothing is clamped: such a distribution has no usable class-balanced loss."""
    n = np.asarray(samples_per_class)
    with np.errstate(divide="ignore", invalid="ignore"):
        effective_num = 1.0 - np.power(beta, n)
        weights = (1.0 - beta) / effective_num
        empty = np.isinf(weights)
        weights = weights / weights.sum() * len(weights)
    weights[empty] = np.inf
    return weights.astype(np.float32)


def class_balanced_loss(logits, labels, samples_per_class, beta=0.9999):
    """ClassBalancedLoss(beta)(logits, labels, samples_per_class): mean of bce x the class weight."""
    w = class_balanced_weights(samples_per_class, beta).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return float((bce_elements(logits, labels) * w[None, :]).mean())


def class_distribution(label_rows, num_classes=None):
    """compute_class_distribution (improved_losses.py:341-348): per class the number of rows whose label is > 0, as float64.  Taken
    from the WHOLE label set (every row of the JSON), before any sharding: every rank must weigh the classes alike."""
    rows = list(label_rows.values()) if isinstance(label_rows, dict) else list(label_rows)
    if not rows:
        return np.zeros(int(num_classes or 0))
    return (np.asarray(rows) > 0).sum(0).astype(np.float64)


def select_loss(use_class_balanced=False, use_focal_loss=False):
    """The reference's rule (train_decoder.py:232-235): class-balanced if asked for, else focal if asked for, else BCE."""
    return "class_balanced" if use_class_balanced else ("focal" if use_focal_loss else "bce")


# ---- the state block (csrc/vt_loss.h) -------------------------------------------------------------------------------------------------
def _align(x):
    return (x + 255) // 256 * 256


def state_layout(num_classes):
    """Byte offsets of the sections of a vt_loss state block, and its size."""
    n = int(num_classes)
    groups = (n + 63) // 64
    lay = {"params": 0, "totals": _align(32)}
    lay["weights"] = lay["totals"] + _align(48)
    lay["sums"] = lay["weights"] + _align(8 * n)
    lay["partials"] = lay["sums"] + _align(16 * n)
    lay["total"] = lay["partials"] + _align(32 * groups)
    return lay


def parse_state(block, num_classes):
    """A state block (bytes / uint8 array of state_layout(N)['total'] bytes) as a dict of host values: alpha, gamma, has_weights,
    batch_mean_sums fp64 [3], steps, elements, non_finite, weights fp64 [N], class_sums fp64 [N][2]."""
    n = int(num_classes)
    lay = state_layout(n)
    raw = np.frombuffer(bytes(block) if not isinstance(block, np.ndarray) else np.ascontiguousarray(block).view(np.uint8).tobytes(), dtype=np.uint8)
    if raw.size < lay["total"]:
        raise ValueError(f"a loss state of {n} classes holds {lay['total']} bytes, got {raw.size}")
    f8 = lambda off, k: raw[off:off + 8 * k].view(np.float64).copy()
    u8 = lambda off, k: raw[off:off + 8 * k].view(np.uint64).copy()
    params_u = u8(lay["params"] + 16, 2)
    if int(params_u[1]) != n:
        raise ValueError(f"the block was reset for {int(params_u[1])} classes, not {n}")
    alpha, gamma = f8(lay["params"], 2)
    counters = u8(lay["totals"] + 24, 3)
    return {"alpha": float(alpha), "gamma": float(gamma), "has_weights": bool(params_u[0]), "batch_mean_sums": f8(lay["totals"], 3),
            "steps": int(counters[0]), "elements": int(counters[1]), "non_finite": int(counters[2]),
            "weights": f8(lay["weights"], n), "class_sums": f8(lay["sums"], 2 * n).reshape(n, 2)}


def pack_state(state):
    """The inverse of parse_state (the partials section is left zero): bytes."""
    n = len(state["weights"])
    lay = state_layout(n)
    raw = np.zeros(lay["total"], dtype=np.uint8)
    raw[0:16] = np.array([state["alpha"], state["gamma"]], dtype=np.float64).view(np.uint8)
    raw[16:32] = np.array([int(state["has_weights"]), n], dtype=np.uint64).view(np.uint8)
    t = lay["totals"]
    raw[t:t + 24] = np.asarray(state["batch_mean_sums"], dtype=np.float64).view(np.uint8)
    raw[t + 24:t + 48] = np.array([state["steps"], state["elements"], state["non_finite"]], dtype=np.uint64).view(np.uint8)
    raw[lay["weights"]:lay["weights"] + 8 * n] = np.asarray(state["weights"], dtype=np.float64).view(np.uint8)
    raw[lay["sums"]:lay["sums"] + 16 * n] = np.ascontiguousarray(state["class_sums"], dtype=np.float64).reshape(-1).view(np.uint8)
    return raw.tobytes()


def same_parameters(a, b):
    """alpha, gamma and the class weights of two parsed states, compared bit-wise (what vt_loss_merge insists on)."""
    return (np.float64(a["alpha"]).tobytes() == np.float64(b["alpha"]).tobytes() and np.float64(a["gamma"]).tobytes() == np.float64(b["gamma"]).tobytes()
            and a["has_weights"] == b["has_weights"] and np.asarray(a["weights"]).tobytes() == np.asarray(b["weights"]).tobytes())


def sum_states(states):
    """fp64 sum of parsed states IN THE ORDER GIVEN, starting from zero -- what vt_loss_merge leaves in a freshly reset block, bit for
    bit.  ValueError when alpha, gamma or the weights differ."""
    states = list(states)
    first = states[0]
    out = dict(first, batch_mean_sums=np.zeros(3), class_sums=np.zeros_like(first["class_sums"]), steps=0, elements=0, non_finite=0)
    for s in states:
        if not same_parameters(first, s):
            raise ValueError("loss states taken with different alpha, gamma or class weights cannot be added")
        with np.errstate(invalid="ignore", over="ignore"):
            out["batch_mean_sums"] = out["batch_mean_sums"] + s["batch_mean_sums"]
            out["class_sums"] = out["class_sums"] + s["class_sums"]
        for k in ("steps", "elements", "non_finite"):
            out[k] += s[k]
    return out


def finish_state(state, class_names=None):
    """The read-out dict from a parsed state.  For each of bce / focal / class_balanced: `mean_of_batch_means` -- the reference's
    val_loss / val_steps for the batching the state was fed with -- and `per_element`, the mean over every element, which does not
    depend on the batching; class_balanced is None when the state carries no class weights.  Plus steps, elements, non_finite, alpha,
    gamma and `per_class`: {name: {bce, focal}} means over the rows seen."""
    n = len(state["weights"])
    steps, elements = state["steps"], state["elements"]
    if steps == 0 or elements == 0:
        raise ValueError("no data: call update() first")
    rows = elements // n
    sums = state["class_sums"]
    with np.errstate(invalid="ignore", over="ignore"):
        # (the three totals in one fixed order: classes ascending)
        totals = [float(np.sum(sums[:, 0])), float(np.sum(sums[:, 1])), float(np.sum(state["weights"] * sums[:, 0]))]
    out = {}
    for k, name in enumerate(LOSS_NAMES):
        if name == "class_balanced" and not state["has_weights"]:
            out[name] = None
            continue
        out[name] = {"mean_of_batch_means": float(state["batch_mean_sums"][k]) / steps, "per_element": totals[k] / elements}
    out.update(steps=steps, elements=elements, non_finite=state["non_finite"], alpha=state["alpha"], gamma=state["gamma"])
    names = class_names if class_names else [f"Class_{i}" for i in range(n)]
    out["per_class"] = {nm: {"bce": float(sums[i, 0]) / rows, "focal": float(sums[i, 1]) / rows} for i, nm in enumerate(names)}
    return out


class HostLossState:
    """Numpy fp64 model of the device accumulator: the same state, fed the same way.  Its sums are taken in numpy's order, not the
    kernel's: equal to the device's within rounding (1e-9 relative is asserted by the GPU tests), not bit for bit."""

    def __init__(self, num_classes, alpha=1.0, gamma=2.0, class_weights=None):
        n = int(num_classes)
        w = np.ones(n) if class_weights is None else np.asarray(class_weights).astype(np.float64)
        if w.shape != (n,):
            raise ValueError(f"expected {n} class weights, got an array of shape {w.shape}")
        self.state = {"alpha": float(alpha), "gamma": float(gamma), "has_weights": class_weights is not None, "batch_mean_sums": np.zeros(3),
                      "steps": 0, "elements": 0, "non_finite": 0, "weights": w, "class_sums": np.zeros((n, 2))}

    def update(self, logits, labels):
        s = self.state
        x = np.asarray(logits, dtype=np.float32)
        bce = bce_elements(x, labels)
        focal = focal_elements(x, labels, s["alpha"], s["gamma"])
        with np.errstate(invalid="ignore", over="ignore"):
            cb, cf = bce.sum(0), focal.sum(0)
            s["class_sums"] = s["class_sums"] + np.stack([cb, cf], axis=1)
            s["batch_mean_sums"] = s["batch_mean_sums"] + np.array([cb.sum(), cf.sum(), (s["weights"] * cb).sum()]) / float(x.size)
        s["steps"] += 1
        s["elements"] += int(x.size)
        s["non_finite"] += int((~np.isfinite(x)).sum())

    def read(self, class_names=None):
        return finish_state(self.state, class_names)

    def to_bytes(self):
        return pack_state(self.state)


def exchange_loss_blocks(block, group=None):
    """ONE all-gather of every rank's loss block(s) (a contiguous uint8 tensor of the same size on every rank): the list of the ranks'
    blocks IN RANK ORDER, on every rank.  Under gloo (the rehearsal backend) host tensors travel; otherwise the tensor is gathered on
    its device into a 256-B aligned buffer, so that each part can be handed to vt_loss_merge as it is when the block size is a multiple
    of 256 bytes."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)
    n = block.numel()
    if dist.get_backend(group) == "gloo":
        parts = [torch.empty(n, dtype=torch.uint8) for _ in range(world)]
        dist.all_gather(parts, block.cpu().contiguous(), group=group)
        return parts
    gathered = torch.empty(world * n + 256, dtype=torch.uint8, device=block.device)
    off = -gathered.data_ptr() % 256
    gathered = gathered[off:off + world * n]
    dist.all_gather_into_tensor(gathered, block.contiguous(), group=group)
    return [gathered[r * n:(r + 1) * n] for r in range(world)]


# ---- device accumulator ---------------------------------------------------------------------------------------------------------------
class LossStateBlock:
    """An exported loss state: `data` (uint8 device tensor, 256-B aligned) and the HOST parameters it was reset with."""

    def __init__(self, data, alpha, gamma, class_weights):
        self.data, self.alpha, self.gamma, self.class_weights = data, float(alpha), float(gamma), class_weights


class DeviceLossAccumulator:
    """The validation loss accumulated on the GPU from the decoder's LOGITS (vt_loss_* of the C ABI): update() queues two small
    launches on the current stream and returns -- no host synchronisation; read() is the one synchronisation.  class_weights: fp64 [N]
    or None (class_balanced_weights(...) for the reference's ClassBalancedLoss); alpha, gamma: FocalLoss' parameters."""

    def __init__(self, num_classes, device="cuda", alpha=1.0, gamma=2.0, class_weights=None, context=None):
        import torch
        from . import _lib
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.VTError("DeviceLossAccumulator runs on a HIP device; HostLossState is the host model")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.N = int(num_classes)
        self.alpha, self.gamma = float(alpha), float(gamma)
        self.class_weights = None if class_weights is None else np.ascontiguousarray(np.asarray(class_weights).astype(np.float64))
        if self.class_weights is not None and self.class_weights.shape != (self.N,):
            raise ValueError(f"expected {self.N} class weights, got an array of shape {self.class_weights.shape}")
        self.ctx = context if context is not None else _lib.Context(self.device.index)
        self.reset()

    def _stream(self):
        import ctypes
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _weights_ptr(self, w=None):
        import ctypes
        w = self.class_weights if w is None else w
        return ctypes.c_void_p(w.ctypes.data) if w is not None else ctypes.c_void_p(0)

    def _alloc(self):
        import torch
        nbytes = self.ctx.lib.vt_loss_state_bytes(self.N)
        if nbytes == 0:
            raise ValueError(f"a loss state of {self.N} classes is not supported")
        buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        return buf, (buf.data_ptr() + 255) // 256 * 256, nbytes

    def reset(self):
        import ctypes
        self.steps = 0
        self._buf, self._ptr, self._bytes = self._alloc()
        self.ctx.call("vt_loss_reset", ctypes.c_void_p(self._ptr), self._bytes, self.N, self.alpha, self.gamma, self._weights_ptr(), self._stream())

    def update(self, logits, labels):
        """logits fp32 [B, N] (the decoder's output BEFORE the sigmoid), labels [B, N]: fp32 labels are used as their value, uint8 /
        bool labels are 0 or 1; device tensors, or host tensors uploaded without blocking.  One vt_loss_update per 4096 rows -- each
        is one step (one batch mean), as a batch of the reference's loop is."""
        import ctypes
        import torch
        from . import _lib
        x = logits.detach()
        if x.device != self.device:
            x = x.to(self.device, non_blocking=True)
        x = x.to(torch.float32).contiguous()
        y = labels.detach() if isinstance(labels, torch.Tensor) else torch.as_tensor(np.asarray(labels))
        if y.device != self.device:
            y = y.to(self.device, non_blocking=True)
        if y.dtype == torch.bool:
            y = y.view(torch.uint8)
        elif y.dtype not in (torch.float32, torch.uint8):
            y = y.to(torch.float32)
        y = y.contiguous()
        if x.dim() != 2 or x.shape[1] != self.N or y.shape != x.shape:
            raise ValueError(f"expected [B, {self.N}] logits and labels, got {tuple(x.shape)} and {tuple(y.shape)}")
        dt = _lib.VT_U8 if y.dtype == torch.uint8 else _lib.VT_F32
        for lo in range(0, x.shape[0], 4096):
            xb, yb = x[lo:lo + 4096], y[lo:lo + 4096]
            self.ctx.call("vt_loss_update", ctypes.c_void_p(self._ptr), self._bytes, self.N, ctypes.c_void_p(xb.data_ptr()),
                          ctypes.c_void_p(yb.data_ptr()), dt, xb.shape[0], self._stream())
            self.steps += 1

    def export_state(self):
        """A copy of the state as it stands in stream order (a LossStateBlock): what a rank sends to the merge.  No synchronisation."""
        import ctypes
        buf, ptr, nbytes = self._alloc()
        self.ctx.call("vt_loss_read", ctypes.c_void_p(self._ptr), self._bytes, self.N, ctypes.c_void_p(ptr), nbytes, self._stream())
        off = ptr - buf.data_ptr()
        return LossStateBlock(buf[off:off + nbytes], self.alpha, self.gamma, self.class_weights)

    def merge_from(self, blocks):
        """Add `blocks` (LossStateBlock) into this state IN THE ORDER GIVEN: one vt_loss_merge call, one launch; it refuses blocks
        taken with another alpha, gamma or other class weights.  No host synchronisation."""
        import ctypes
        import torch
        from . import _lib
        blocks = list(blocks)
        for b in blocks:
            if b.data.device != self.device or b.data.dtype != torch.uint8 or not b.data.is_contiguous() or b.data.data_ptr() % 256:
                raise ValueError("merge_from: a block is a contiguous, 256-B aligned uint8 tensor on the accumulator's device")
        keep = [None if b.class_weights is None else np.ascontiguousarray(np.asarray(b.class_weights).astype(np.float64)) for b in blocks]
        src = (_lib.LossSource * len(blocks))(*[_lib.LossSource(b.data.data_ptr(), b.data.numel(), b.alpha, b.gamma,
                                                                 self._weights_ptr(w).value if w is not None else None)
                                                for b, w in zip(blocks, keep)])
        self.ctx.call("vt_loss_merge", ctypes.c_void_p(self._ptr), self._bytes, self.N, self.alpha, self.gamma, self._weights_ptr(), src, len(blocks),
                      self._stream())

    def read_state(self):
        """The parsed state on the host (parse_state): the one synchronisation."""
        import ctypes
        import torch
        out = torch.empty(self._bytes, dtype=torch.uint8, pin_memory=True)
        self.ctx.call("vt_loss_read", ctypes.c_void_p(self._ptr), self._bytes, self.N, ctypes.c_void_p(out.data_ptr()), self._bytes, self._stream())
        torch.cuda.current_stream(self.device).synchronize()
        return parse_state(out.numpy(), self.N)

    def read(self, class_names=None):
        """finish_state's dict of this accumulator's state."""
        return finish_state(self.read_state(), class_names)


# ---- checkpoint sweep: the pure-Python parts -----------------------------------------------------------------------------------------
def sweep_dir_name(index, checkpoint_path):
    """`ckpt_<index>_<file stem>`: the directory of one checkpoint's files under the sweep's output directory."""
    stem = os.path.splitext(os.path.basename(str(checkpoint_path)))[0]
    return f"ckpt_{int(index)}_{stem}"


def loss_report(loss, selected):
    """validation_loss.json: the read-out without the per-class table, plus which loss the reference's rule selects and its value."""
    if loss.get(selected) is None:
        raise ValueError(f"the selected loss '{selected}' was not accumulated (class weights are needed for class_balanced)")
    out = {"selected_loss": selected, "val_loss": loss[selected]["mean_of_batch_means"]}
    out.update({k: v for k, v in loss.items() if k != "per_class"})
    return out


def sweep_summary(rows, selected):
    """checkpoint_sweep.json from one dict per checkpoint (path, loss = finish_state's dict, optimal = find_optimal_threshold's dict,
    metrics = compute_metrics' dict).  best_by_val_loss: the lowest `mean_of_batch_means` of the SELECTED loss, the reference's
    criterion (train_decoder.py:250); best_by_macro_f1: the highest f1_macro at the global threshold.  A tie goes to the earlier
    checkpoint (strict comparison, as the reference's `<`); a NaN never wins."""
    table = []
    for i, r in enumerate(rows):
        loss = r["loss"]
        if loss.get(selected) is None:
            raise ValueError(f"the selected loss '{selected}' was not accumulated (class weights are needed for class_balanced)")
        table.append({"index": i, "path": str(r["path"]), "selected_loss": selected, "val_loss": loss[selected]["mean_of_batch_means"],
                      **{name: loss[name] for name in LOSS_NAMES},
                      "global_threshold": r["optimal"]["global_threshold"], "global_f1": r["optimal"]["global_f1"],
                      "f1_macro": r["metrics"]["f1_macro"], "f1_micro": r["metrics"]["f1_micro"], "mAP": r["metrics"].get("mAP"),
                      "non_finite": loss["non_finite"]})
    best_loss = best_f1 = None
    for t in table:
        if t["val_loss"] == t["val_loss"] and (best_loss is None or t["val_loss"] < table[best_loss]["val_loss"]):
            best_loss = t["index"]
        if t["f1_macro"] == t["f1_macro"] and (best_f1 is None or t["f1_macro"] > table[best_f1]["f1_macro"]):
            best_f1 = t["index"]
    pick = lambda i: None if i is None else {"index": i, "path": table[i]["path"]}
    return {"selected_loss": selected, "checkpoints": table, "best_by_val_loss": pick(best_loss), "best_by_macro_f1": pick(best_f1)}
