"""Validation loss of the VAE: the number train_vae.py keeps `best_vae` by (train_vae.py:216-268; train_full.py:290-338) --
reconstruction MSE, KL of the three posteriors, the triplet loss on sampled latents (and the contrastive term) -- accumulated batch by
batch -- and the gradient of the training loss, the same formulas differentiated (loss_backward_host / loss_backward_device).

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


# ---- the gradient of the training loss (vt_vae_loss_backward) --------------------------------------------------------------
LOSS_NAMES = ("reconstruction", "kl", "triplet", "total")      # loss_out


def _stream(item):
    """(moments, draw) or update()'s (moments, None, draw) -> (moments, draw): the gradient samples in flight and takes no stored z"""
    if len(item) == 3:
        if item[1] is not None:
            raise ValueError("the loss's gradient regenerates z from the counter and takes no stored z")
        item = (item[0], item[2])
    if item[0] is None:
        raise ValueError("a stream needs its moments")
    return item[0], int(item[1])


def _weights(weights):
    w = tuple(float(weights.get(k, 0.0)) for k in ("reconstruction", "kl", "triplet"))
    if not all(np.isfinite(w)):
        raise ValueError("the weights must be finite")
    return w


def backward_workspace_bytes(B, C, hw, H=0, W=0):
    """vt_vae_loss_backward_workspace_bytes in host arithmetic: the forward's scratch, a coefficient record per image, one for the batch."""
    return state_bytes(B, C, hw, H, W) - HEAD_BYTES + _align(8 * 8 * B) + _align(8 * 8)


def forward_z(mean, std32, eps):
    """z = fma(std, eps, mean) of fp32 values rounded once to fp32, as the device forms it (csrc/vt_vae_loss.h vae_z_of), exactly: the product of
    two fp32 values is exact in fp64; the fp64 sum s and its rounding error (TwoSum) give the exact value, and the error decides the one case in
    which rounding s again would go wrong -- s exactly half way between two fp32 values."""
    a = np.asarray(mean, dtype=np.float32).astype(np.float64)
    p = np.asarray(std32, dtype=np.float32).astype(np.float64) * np.asarray(eps, dtype=np.float32).astype(np.float64)
    s = a + p
    t = s - a
    err = (a - (s - t)) + (p - t)
    with np.errstate(over="ignore", invalid="ignore"):
        r = s.astype(np.float32)
        down, up = np.nextafter(r, np.float32(-np.inf)), np.nextafter(r, np.float32(np.inf))
        r64 = r.astype(np.float64)
        tie_down, tie_up = s == 0.5 * (r64 + down.astype(np.float64)), s == 0.5 * (r64 + up.astype(np.float64))
        # at a tie astype took the even neighbour; the exact value lies on err's side of s
        r = np.where(tie_down & (err > 0), r, np.where(tie_down & (err < 0), down, r))
        r = np.where(tie_up & (err < 0), r, np.where(tie_up & (err > 0), up, r))
    return r.astype(np.float32)


def loss_backward_host(anchor, positive, negative, *, weights, margin=1.0, similarity_type="cosine", seed=0, first_image=0, dz_dec=None,
                       dz_draw=0, recon=None, target=None, labels_a=None, labels_p=None, eps=None, z_forward=None):
    """The fp64 numpy mirror of vt_vae_loss_backward.  anchor / positive / negative: (moments [B, 2C, h, w], draw).  weights: a dict with
    "reconstruction", "kl", "triplet".  eps (optional): (eps_a, eps_p, eps_n, eps_dec) fp32 arrays to use instead of the host model of the
    counter-based normal (improved_losses.normal_draw); z_forward (optional): the three streams' fp32 z as the device's forward formed them
    (vt_posterior_sample), instead of forward_z.  -> {"d_recon", "d_moments": [a, p, n], "rows" [B, ROW], "losses" [4]}; z is the
    forward's fp32 z and std its fp32 std, as on the device."""
    if negative is None:
        raise ValueError("a negative stream is required: the contrastive term has no gradient here")
    w_rec, w_kl, w_tri = _weights(weights)
    if not np.isfinite(margin):
        raise ValueError("the margin must be finite")
    streams = [_stream(s) for s in (anchor, positive, negative)]
    shape = np.asarray(streams[0][0]).shape
    B, C = shape[0], shape[1] // 2
    D = int(np.prod(shape[1:])) // 2
    draws = [d for _, d in streams] + [int(dz_draw)]
    if eps is None:
        eps = [np.stack([il.normal_draw(seed, d, first_image + i, D) for i in range(B)]) for d in draws]
    eps = [np.asarray(e, dtype=np.float32).reshape(B, D) for e in eps]
    mean, lv, sd, std32, z = [], [], [], [], []
    for (m, _), e in zip(streams, eps):
        m = np.asarray(m, dtype=np.float32).reshape(B, 2, D)
        mean.append(m[:, 0]), lv.append(m[:, 1])
        sd.append(np.exp(0.5 * np.clip(lv[-1].astype(np.float64), -30.0, 20.0)))
        std32.append(sd[-1].astype(np.float32))
        z.append(forward_z(mean[-1], std32[-1], e).astype(np.float64) if z_forward is None else
                 np.asarray(z_forward[len(z)], dtype=np.float32).reshape(B, D).astype(np.float64))
    rows = rows_from_mirrors(z[0], z[1], z[2], tuple(il.kl_elements(np.asarray(m).reshape(B, 2 * C, -1)) for m, _ in streams), recon, target,
                             labels_a, labels_p, margin_triplet=margin)
    rows[:, 12:14] = 0.0
    euclid = similarity_type != "cosine"
    col = 11 if euclid else 10
    sums = np.zeros(3)
    for r in rows:                                                            # (one image after the other, as the device adds them)
        sums += (r[0], r[4], r[col])
    losses = np.array([sums[0] / B, float(il.kl_log(sums[1] / B)), sums[2] / B, 0.0])
    losses[3] = w_rec * losses[0] + w_kl * losses[1] + w_tri * losses[2]
    c_kl = w_kl / (3.0 * B * 10000.0 * (1.0 + sums[1] / B / 10000.0))
    x = rows[:, 8 if euclid else 6] - rows[:, 9 if euclid else 7] + float(margin)
    t = (w_tri * rows[:, 17] / B * np.where(x <= 0.0, 0.0, 1.0))[:, None]
    a, p, n = z
    if euclid:
        dp, dn = a - p + 1e-6, a - n + 1e-6
        with np.errstate(divide="ignore", invalid="ignore"):
            tp = np.where(rows[:, 8:9] > 0.0, t / rows[:, 8:9], 0.0)
            tn = np.where(rows[:, 9:10] > 0.0, t / rows[:, 9:10], 0.0)
        g = [dp * tp - dn * tn, -(dp * tp), dn * tn]
    else:
        r_ = [np.sqrt((v * v).sum(1, keepdims=True)) for v in z]
        N_ = [np.maximum(v, 1e-12) for v in r_]
        ap, an = (a * p).sum(1, keepdims=True), (a * n).sum(1, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            ka = np.where(r_[0] >= 1e-12, t * (ap / N_[1] - an / N_[2]) / (N_[0] * N_[0] * r_[0]), 0.0)
            kp = np.where(r_[1] >= 1e-12, t * ap / (N_[0] * N_[1] * N_[1] * r_[1]), 0.0)
            kn = np.where(r_[2] >= 1e-12, t * an / (N_[0] * N_[2] * N_[2] * r_[2]), 0.0)
        ipn, inn = t / (N_[0] * N_[1]), t / (N_[0] * N_[2])
        g = [a * ka - p * ipn + n * inn, p * kp - a * ipn, a * inn - n * kn]
    d_moments = []
    for s in range(3):
        d_mean, sampled = g[s], g[s] * std32[s] * eps[s].astype(np.float64)
        if s == 0 and dz_dec is not None:
            dz = np.asarray(dz_dec, dtype=np.float64).reshape(B, D)
            d_mean, sampled = d_mean + dz, sampled + dz * std32[0] * eps[3].astype(np.float64)
        inside = (lv[s] >= -30.0) & (lv[s] <= 20.0)
        d_lv = np.where(inside, 0.5 * sampled + c_kl * (0.5 * (sd[s] * sd[s] - 1.0)), 0.0)
        d_moments.append(np.stack([d_mean + c_kl * mean[s], d_lv], 1).reshape(shape))
    d_recon = None
    if recon is not None:
        r64, t64 = np.asarray(recon, dtype=np.float64), np.asarray(target, dtype=np.float64)
        d_recon = w_rec * 2.0 / (float(B) * float(r64[0].size)) * (r64 - t64)
    return {"d_recon": d_recon, "d_moments": d_moments, "rows": rows, "losses": losses}


def loss_backward_device(anchor, positive, negative, *, weights, margin=1.0, similarity_type="cosine", seed=0, first_image=0, dz_dec=None,
                         dz_draw=0, recon=None, target=None, labels_a=None, labels_p=None, d_recon=None, d_moments=None, rows_out=None,
                         loss_out=None, workspace=None, context=None):
    """One vt_vae_loss_backward on torch's current stream; no host synchronisation.  anchor / positive / negative: (moments, draw) (or
    update()'s (moments, None, draw)) with moments contiguous fp32 device tensors [B, 2C, h, w].  Outputs are written only where given:
    d_recon fp32 like recon; d_moments a sequence of three fp32 tensors like the moments, each or all None (they may be the three slices
    of one [3B, 2C, h, w] tensor); rows_out float64 [B, ROW]; loss_out float64 [4] (LOSS_NAMES).  workspace: a uint8 device tensor of
    at least backward_workspace_bytes + 256 bytes, or None to allocate one."""
    import torch
    from . import _lib
    if negative is None:
        raise ValueError("a negative stream is required: the contrastive term has no gradient here")
    w = _weights(weights)
    if not np.isfinite(margin):
        raise ValueError("the margin must be finite")
    streams = [_stream(s) for s in (anchor, positive, negative)]
    m0 = streams[0][0]
    dev = m0.device

    def f32(t, shape, what):
        if t is None:
            return None
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != dev or not t.is_contiguous() or (
                shape is not None and tuple(t.shape) != tuple(shape)):
            raise ValueError(f"{what}: expected a contiguous fp32 tensor{'' if shape is None else ' ' + str(tuple(shape))} on {dev}")
        return t

    if not isinstance(m0, torch.Tensor) or m0.dim() < 3 or m0.shape[1] % 2 or not m0.is_cuda:
        raise ValueError("moments are [B, 2C, h, w] tensors on a HIP device")
    for m, _ in streams:
        f32(m, m0.shape, "moments")
    B, C, hw = m0.shape[0], m0.shape[1] // 2, int(np.prod(m0.shape[2:]))
    f32(dz_dec, (B, C) + tuple(m0.shape[2:]), "dz_dec")
    H = W = 0
    if recon is not None or target is not None or d_recon is not None:
        if recon is None or target is None or recon.dim() != 4 or recon.shape[1] != 3 or recon.shape[0] != B:
            raise ValueError("recon and target are [B, 3, H, W] tensors of one shape")
        f32(recon, None, "recon"), f32(target, recon.shape, "target"), f32(d_recon, recon.shape, "d_recon")
        H, W = recon.shape[2], recon.shape[3]
    dm = list(d_moments) if d_moments is not None else [None] * 3
    if len(dm) != 3:
        raise ValueError("d_moments holds three tensors (or None): anchor, positive, negative")
    for t in dm:
        f32(t, m0.shape, "d_moments")
    N, dt = 0, _lib.VT_F32
    if labels_a is not None and labels_p is not None:
        if labels_a.dtype == torch.bool:
            labels_a, labels_p = labels_a.view(torch.uint8), labels_p.view(torch.uint8)
        if labels_a.dtype != labels_p.dtype or labels_a.dtype not in (torch.float32, torch.uint8) or labels_a.dim() != 2 or (
                labels_a.shape != labels_p.shape or labels_a.shape[0] != B or labels_a.device != dev or labels_p.device != dev
                or not labels_a.is_contiguous() or not labels_p.is_contiguous()):
            raise ValueError("labels are contiguous [B, N] tensors of one shape, fp32 or uint8 / bool, on the moments' device")
        N, dt = labels_a.shape[1], (_lib.VT_U8 if labels_a.dtype == torch.uint8 else _lib.VT_F32)
    else:
        labels_a = labels_p = None
    for t, n, what in ((rows_out, B * ROW, "rows_out"), (loss_out, 4, "loss_out")):
        if t is not None and (t.dtype != torch.float64 or t.device != dev or not t.is_contiguous() or t.numel() != n):
            raise ValueError(f"{what} is a contiguous float64 tensor of {n} elements on {dev}")
    if context is None:
        from .vae_backward import context as backward_context          # the package's one cache of per-device contexts for the backward entry points
        context = backward_context(dev)
    ctx = context
    need = ctx.lib.vt_vae_loss_backward_workspace_bytes(B, C, hw, H, W)
    if need == 0:
        raise ValueError(f"{B} images of {C} x {hw} latents and {H} x {W} pixels are not supported")
    if workspace is None:
        workspace = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    off = -workspace.data_ptr() % 256
    ins = [_lib.VAELossInput(m.data_ptr(), None, d) for m, d in streams]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    ctx.call("vt_vae_loss_backward", ctypes.byref(ins[0]), ctypes.byref(ins[1]), ctypes.byref(ins[2]), ptr(dz_dec), int(dz_draw), ptr(recon), ptr(target),
             H, W, ptr(labels_a), ptr(labels_p), dt, N, B, C, hw, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_image), w[0], w[1], w[2], float(margin),
             _lib.VAE_COSINE if similarity_type == "cosine" else _lib.VAE_EUCLIDEAN, ptr(d_recon), ptr(dm[0]), ptr(dm[1]), ptr(dm[2]), ptr(rows_out),
             ptr(loss_out), ctypes.c_void_p(workspace.data_ptr() + off), max(workspace.numel() - off, 0),
             ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))

