"""Validation loss of the VAE: the number train_vae.py keeps `best_vae` by (train_vae.py:216-268; train_full.py:290-338) --
reconstruction MSE, KL of the three posteriors, the triplet loss on sampled latents (and the contrastive term) -- accumulated batch by
batch.  Forward only.

Host side: HostVAELossState, a numpy fp64 model of the device block fed the same way (from improved_losses' mirrors), the block's
layout, and finish_state, the report.  Device side: DeviceVAELossAccumulator over vt_vae_loss_* of the C ABI; nothing is read back per
batch.  The totals of train_vae (simplified or full) and train_full are linear in the per-batch components, so they are formed here, on
the host, from the components; no weight enters a kernel.
"""
import ctypes

import numpy as np

from . import improved_losses as il

COMPONENTS = ("mse", "kl_mean", "kl_log", "triplet_cosine", "triplet_euclidean", "contrastive_cosine", "contrastive_euclidean")
COUNTERS = ("updates", "images", "non_finite", "recon_updates", "recon_images", "negative_updates", "negative_images")
ROW_NAMES = ("mse", "kl_a", "kl_p", "kl_n", "kl_mean", "kl_log", "pos_cosine", "neg_cosine", "pos_euclidean", "neg_euclidean", "triplet_cosine",
             "triplet_euclidean", "contrastive_cosine", "contrastive_euclidean", "label_sum", "overlap", "union", "triplet_weight", "label_similarity")
ROW = len(ROW_NAMES)                         # VT_VAE_LOSS_ROW
HEAD_BYTES = 512                             # VT_VAE_LOSS_HEAD_BYTES: params | totals
CHUNK = 4096                                 # elements of one partial (csrc/vt_vae_loss.h)
_COMPONENT_ROW = (0, 4, 5, 10, 11, 12, 13)   # the row entry a component is the mean of


def _align(x):
    return (x + 255) // 256 * 256


def state_bytes(B, C, hw, H=0, W=0):
    """vt_vae_loss_state_bytes in host arithmetic: head, rows (+ one counter per image), latent partials, image partials."""
    d, e = int(C) * int(hw), 3 * int(H) * int(W)
    chunks = lambda n: (n + CHUNK - 1) // CHUNK
    return HEAD_BYTES + _align(8 * (ROW + 1) * B) + _align(8 * 12 * B * chunks(d)) + _align(8 * 2 * B * chunks(e))


def parse_state(block):
    """The head of a block (>= 512 bytes) as host values."""
    raw = np.frombuffer(bytes(block) if not isinstance(block, np.ndarray) else np.ascontiguousarray(block).view(np.uint8).tobytes(), dtype=np.uint8)
    if raw.size < HEAD_BYTES:
        raise ValueError(f"a VAE loss state's head holds {HEAD_BYTES} bytes, got {raw.size}")
    f8 = lambda off, k: raw[off:off + 8 * k].view(np.float64).copy()
    u8 = lambda off, k: raw[off:off + 8 * k].view(np.uint64).copy()
    p = f8(0, 3)
    k = len(COMPONENTS)
    out = {"margin_triplet": float(p[0]), "margin_contrastive": float(p[1]), "jaccard_threshold": float(p[2]), "seed": int(u8(24, 1)[0]),
           "batch_sums": f8(256, k), "image_sums": f8(256 + 8 * k, k)}
    out.update({name: int(v) for name, v in zip(COUNTERS, u8(256 + 16 * k, len(COUNTERS)))})
    return out


def pack_state(state):
    """The inverse of parse_state: the 512 bytes of the head."""
    raw = np.zeros(HEAD_BYTES, dtype=np.uint8)
    raw[0:24] = np.array([state["margin_triplet"], state["margin_contrastive"], state["jaccard_threshold"]], dtype=np.float64).view(np.uint8)
    raw[24:32] = np.array([state["seed"]], dtype=np.uint64).view(np.uint8)
    k = len(COMPONENTS)
    raw[256:256 + 8 * k] = np.asarray(state["batch_sums"], dtype=np.float64).view(np.uint8)
    raw[256 + 8 * k:256 + 16 * k] = np.asarray(state["image_sums"], dtype=np.float64).view(np.uint8)
    raw[256 + 16 * k:256 + 16 * k + 8 * len(COUNTERS)] = np.array([state[c] for c in COUNTERS], dtype=np.uint64).view(np.uint8)
    return raw.tobytes()


def selected_total(components, weights, similarity_type="cosine", simplified=False):
    """train_vae.py's total from a dict of components: reconstruction_weight mse + kl_weight kl_log (not when simplified) +
    triplet_weight triplet of the chosen similarity.  (train_full's classification term is added by the caller: evaluate_vae.build_report.)"""
    sim = "cosine" if similarity_type == "cosine" else "euclidean"
    total = float(weights.get("reconstruction", 0.0)) * components["mse"] + float(weights.get("triplet", 0.0)) * components["triplet_" + sim]
    if not simplified:
        total += float(weights.get("kl", 0.0)) * components["kl_log"]
    return total


def finish_state(state, weights, similarity_type="cosine", simplified=False):
    """The report from a parsed state: every component as `mean_of_batch_means` (the reference's val_loss / val_steps for the batching
    fed) and as `per_image` (independent of the batching), the selected total of both, the counters and the settings.  A component
    that was never fed (no recon, no negative) is None."""
    if state["updates"] == 0:
        raise ValueError("no data: call update() first")
    den = {"mse": ("recon_updates", "recon_images"), "triplet_cosine": ("negative_updates", "negative_images"),
           "triplet_euclidean": ("negative_updates", "negative_images")}
    batch, image = {}, {}
    for k, name in enumerate(COMPONENTS):
        du, di = den.get(name, ("updates", "images"))
        batch[name] = float(state["batch_sums"][k]) / state[du] if state[du] else None
        image[name] = float(state["image_sums"][k]) / state[di] if state[di] else None
    zero = lambda d: {k: (0.0 if v is None else v) for k, v in d.items()}
    out = {"components": {name: {"mean_of_batch_means": batch[name], "per_image": image[name]} for name in COMPONENTS},
           "similarity_type": similarity_type, "simplified": bool(simplified), "weights": {k: float(v) for k, v in weights.items()},
           "val_loss": selected_total(zero(batch), weights, similarity_type, simplified),
           "val_loss_per_image": selected_total(zero(image), weights, similarity_type, simplified)}
    out.update({c: state[c] for c in COUNTERS})
    out.update({k: state[k] for k in ("margin_triplet", "margin_contrastive", "jaccard_threshold", "seed")})
    return out


def rows_from_mirrors(za, zp, zn=None, kl=(None, None, None), recon=None, target=None, labels_a=None, labels_p=None, margin_triplet=1.0,
                      margin_contrastive=1.0, threshold=il.JACCARD_THRESHOLD):
    """The fp64 [B, ROW] table of one update from improved_losses' mirrors: what the device writes to rows_out."""
    b = np.asarray(za).shape[0]
    r = np.zeros((b, ROW))
    if recon is not None:
        r[:, 0] = il.mse_elements(recon, target)
    present = [k for k in kl if k is not None]
    for i, k in enumerate(kl):
        if k is not None:
            r[:, 1 + i] = k
    if present:
        r[:, 4] = (r[:, 1] + r[:, 2] + r[:, 3]) / float(len(present))
    r[:, 5] = il.kl_log(r[:, 4])
    for j, sim in enumerate(("cosine", "euclidean")):
        r[:, 6 + 2 * j] = il.distance_elements(za, zp, sim)
        if zn is not None:
            r[:, 7 + 2 * j] = il.distance_elements(za, zn, sim)
            r[:, 10 + j] = il.triplet_elements(za, zp, zn, labels_a, labels_p, margin_triplet, sim)
        r[:, 12 + j] = il.contrastive_elements(za, zp, labels_a, labels_p, margin_contrastive, sim, threshold)
    if labels_a is not None:
        r[:, 14], r[:, 15], r[:, 16] = il.label_sums(labels_a, labels_p)
    r[:, 17] = il.triplet_weight(labels_a, labels_p, b)
    r[:, 18] = r[:, 15] / (r[:, 16] + 1e-8)
    return r


class HostVAELossState:
    """Numpy fp64 model of the device accumulator: the same state, fed the same way.  Latents are given (`z`), or sampled from `moments`
    with improved_losses.sample_elements and this state's seed.  Its sums are numpy's, equal to the device's within rounding."""

    def __init__(self, margin_triplet=1.0, margin_contrastive=1.0, jaccard_threshold=il.JACCARD_THRESHOLD, seed=0):
        k = len(COMPONENTS)
        self.state = {"margin_triplet": float(margin_triplet), "margin_contrastive": float(margin_contrastive),
                      "jaccard_threshold": float(jaccard_threshold), "seed": int(seed), "batch_sums": np.zeros(k), "image_sums": np.zeros(k)}
        self.state.update({c: 0 for c in COUNTERS})

    def _latent(self, item, first_image):
        moments, z, draw = item
        kl = None if moments is None else il.kl_elements(moments)
        if z is None:
            z = il.sample_elements(moments, self.state["seed"], draw, first_image)[0].astype(np.float32)
        return np.asarray(z), kl

    def update(self, anchor, positive, negative=None, recon=None, target=None, labels_a=None, labels_p=None, first_image=0):
        """anchor / positive / negative: (moments or None, z or None, draw).  Returns the [B, ROW] table."""
        s = self.state
        (za, ka), (zp, kp) = self._latent(anchor, first_image), self._latent(positive, first_image)
        zn, kn = self._latent(negative, first_image) if negative is not None else (None, None)
        rows = rows_from_mirrors(za, zp, zn, (ka, kp, kn), recon, target, labels_a, labels_p, s["margin_triplet"], s["margin_contrastive"],
                                 s["jaccard_threshold"])
        b = rows.shape[0]
        for k, col in enumerate(_COMPONENT_ROW):
            if (k == 0 and recon is None) or (k in (3, 4) and negative is None):
                continue
            s["batch_sums"][k] += il.kl_log(rows[:, 4].mean()) if k == 2 else rows[:, col].mean()
            for v in rows[:, col]:
                s["image_sums"][k] += v
        s["updates"] += 1
        s["images"] += b
        bad = 0
        for item in (anchor, positive, negative):
            if item is not None:
                bad += sum(int((~np.isfinite(np.asarray(t, dtype=np.float64))).sum()) for t in item[:2] if t is not None)
        for t in (recon, target):
            if t is not None:
                bad += int((~np.isfinite(np.asarray(t, dtype=np.float64))).sum())
        s["non_finite"] += bad
        if recon is not None:
            s["recon_updates"] += 1
            s["recon_images"] += b
        if negative is not None:
            s["negative_updates"] += 1
            s["negative_images"] += b
        return rows

    def read(self, weights, similarity_type="cosine", simplified=False):
        return finish_state(self.state, weights, similarity_type, simplified)

    def to_bytes(self):
        return pack_state(self.state)


class DeviceVAELossAccumulator:
    """The VAE's validation loss accumulated on the GPU (vt_vae_loss_* of the C ABI): update() queues four small launches on the current
    stream and returns -- no host synchronisation; read_state() is the one synchronisation.  The block grows with the largest update."""

    def __init__(self, device="cuda", margin_triplet=1.0, margin_contrastive=1.0, jaccard_threshold=il.JACCARD_THRESHOLD, seed=0, context=None):
        import torch
        from . import _lib
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.VTError("DeviceVAELossAccumulator runs on a HIP device; HostVAELossState is the host model")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.params = (float(margin_triplet), float(margin_contrastive), float(jaccard_threshold), int(seed) & 0xFFFFFFFFFFFFFFFF)
        self.ctx = context if context is not None else _lib.Context(self.device.index)
        self._buf = None
        self._grow(HEAD_BYTES)
        self.ctx.call("vt_vae_loss_reset", ctypes.c_void_p(self._ptr), self._bytes, *self.params, self._stream())

    def _stream(self):
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _grow(self, nbytes):
        """A block of at least nbytes; the head (params and totals) moves along in stream order."""
        import torch
        if self._buf is not None and self._bytes >= nbytes:
            return
        buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        off = -buf.data_ptr() % 256
        if self._buf is not None:
            buf[off:off + HEAD_BYTES].copy_(self._buf[self._off:self._off + HEAD_BYTES])
        self._buf, self._off, self._ptr, self._bytes = buf, off, buf.data_ptr() + off, nbytes

    def _f32(self, t):
        import torch
        if t is None:
            return None
        t = t.detach() if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t))
        if t.device != self.device:
            t = t.to(self.device, non_blocking=True)
        return t.to(torch.float32).contiguous()

    def _labels(self, y):
        import torch
        y = y.detach() if isinstance(y, torch.Tensor) else torch.as_tensor(np.asarray(y))
        if y.device != self.device:
            y = y.to(self.device, non_blocking=True)
        if y.dtype == torch.bool:
            y = y.view(torch.uint8)
        elif y.dtype not in (torch.float32, torch.uint8):
            y = y.to(torch.float32)
        return y.contiguous()

    def update(self, anchor, positive, negative=None, recon=None, target=None, labels_a=None, labels_p=None, first_image=0, rows_out=None):
        """anchor / positive / negative: (moments [B, 2C, h, w] or None, z [B, C, h, w] or [B, D] or None, draw); a missing z is sampled
        in flight from the moments with this accumulator's seed.  recon / target fp32 [B, 3, H, W]; labels [B, N] fp32 or uint8 / bool.
        rows_out: a float64 device tensor [B, ROW] for the per-image values, or None."""
        import torch
        from . import _lib
        keep, ins, shape = [], [], None
        for item in (anchor, positive, negative):
            if item is None:
                ins.append(None)
                continue
            m, z, draw = self._f32(item[0]), self._f32(item[1]), int(item[2])
            if m is None and z is None:
                raise ValueError("a stream needs its moments, its latent, or both")
            if m is not None:
                sh = (m.shape[0], m.shape[1] // 2, int(np.prod(m.shape[2:])))
            else:
                sh = (z.shape[0], 1, int(np.prod(z.shape[1:])))
            if z is not None and z.numel() != sh[0] * sh[1] * sh[2]:
                raise ValueError(f"latent of shape {tuple(z.shape)} does not fit moments of shape {tuple(m.shape)}")
            if shape is not None and (sh[0], sh[1] * sh[2]) != (shape[0], shape[1] * shape[2]):
                raise ValueError("anchor, positive and negative must have one batch size and one latent size")
            shape = shape or sh
            keep += [m, z]
            ins.append(_lib.VAELossInput(m.data_ptr() if m is not None else None, z.data_ptr() if z is not None else None, draw))
        B, C, hw = shape
        recon, target = self._f32(recon), self._f32(target)
        H = W = 0
        if recon is not None:
            if recon.dim() != 4 or recon.shape[1] != 3 or target is None or target.shape != recon.shape or recon.shape[0] != B:
                raise ValueError("recon and target are [B, 3, H, W] tensors of one shape")
            H, W = recon.shape[2], recon.shape[3]
        N, dt = 0, _lib.VT_F32
        if labels_a is not None and labels_p is not None:
            labels_a, labels_p = self._labels(labels_a), self._labels(labels_p)
            if labels_p.dtype != labels_a.dtype:
                labels_a, labels_p = labels_a.float(), labels_p.float()
            if labels_a.dim() != 2 or labels_a.shape != labels_p.shape or labels_a.shape[0] != B:
                raise ValueError("labels are [B, N] tensors of one shape")
            N, dt = labels_a.shape[1], (_lib.VT_U8 if labels_a.dtype.itemsize == 1 else _lib.VT_F32)
        else:
            labels_a = labels_p = None
        if rows_out is not None and (rows_out.dtype != torch.float64 or rows_out.device != self.device or not rows_out.is_contiguous()
                                     or rows_out.numel() != B * ROW):
            raise ValueError(f"rows_out is a contiguous float64 tensor [{B}, {ROW}] on the accumulator's device")
        need = self.ctx.lib.vt_vae_loss_state_bytes(B, C, hw, H, W)
        if need == 0:
            raise ValueError(f"an update of {B} images of {C} x {hw} latents and {H} x {W} pixels is not supported")
        self._grow(need)
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        ref = lambda s: ctypes.byref(s) if s is not None else None
        self.ctx.call("vt_vae_loss_update", ctypes.c_void_p(self._ptr), self._bytes, ref(ins[0]), ref(ins[1]), ref(ins[2]), ptr(recon), ptr(target),
                      H, W, ptr(labels_a), ptr(labels_p), dt, N, B, C, hw, int(first_image), ptr(rows_out), self._stream())

    def device_head(self):
        """A copy of the head as it stands in stream order: a uint8 device tensor of 512 bytes.  No synchronisation."""
        import torch
        out = torch.empty(HEAD_BYTES + 256, dtype=torch.uint8, device=self.device)
        off = -out.data_ptr() % 256
        out = out[off:off + HEAD_BYTES]
        self.ctx.call("vt_vae_loss_read", ctypes.c_void_p(self._ptr), self._bytes, ctypes.c_void_p(out.data_ptr()), HEAD_BYTES, self._stream())
        return out

    def device_components(self):
        """The sums of the per-batch components as a float64 device tensor [7] (after one update: that batch's losses).  No synchronisation."""
        import torch
        return self.device_head()[256:256 + 8 * len(COMPONENTS)].view(torch.float64)

    def read_state(self):
        """The parsed head on the host: the one synchronisation."""
        import torch
        out = torch.empty(HEAD_BYTES, dtype=torch.uint8, pin_memory=True)
        self.ctx.call("vt_vae_loss_read", ctypes.c_void_p(self._ptr), self._bytes, ctypes.c_void_p(out.data_ptr()), HEAD_BYTES, self._stream())
        torch.cuda.current_stream(self.device).synchronize()
        return parse_state(out.numpy())

    def read(self, weights, similarity_type="cosine", simplified=False):
        return finish_state(self.read_state(), weights, similarity_type, simplified)
