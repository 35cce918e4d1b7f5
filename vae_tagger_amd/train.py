"""Training of the decoder's classifier head on the GPU (vt_head_* of the C ABI; csrc/train_head.hip): what the loop body of the
reference's train_decoder.py (train_decoder.py:173-216) does to `classifier.*`.

  lr_schedule    the four learning-rate schedules of the reference's get_scheduler call, as closed forms evaluated on the host
  split_indices / epoch_order    the train / validation split and the per-epoch training order, from the seed alone
  FeatureCache   the decoder front's feature rows and the labels of every image, kept on the device after the first epoch
  HeadTrainer    the device state (parameters, gradients, Adam moments, loss ring) and its forward_backward / clip / step / commit
                 (what it shares with FrontTrainer -- the state block, step, commit, read, write -- is _BlockTrainer)
  FrontTrainer   the same for the attention decoder's front (vt_front_*; csrc/train_front.hip): training-mode forward (BatchNorm on
                 batch statistics, dropout on the softmax weights), backward from d loss / d features, AdamW, commit
  CrossTrainer   the same for query_generator.* / cross_attention.* (vt_cross_*; csrc/train_cross.hip): the piece between the front's
                 rows and the head's feature rows of a decoder with cross-attention
  DecoderTrainer front (+ cross-attention) + head: one forward_backward, ONE clip_grad_norm_ over all blocks (vt_train_clip /
                 vt_train_clip3), one step / commit
  LatentCache    the encoder's latents of every image in one flat device arena, so that later epochs skip the encoder
  GradientExchange   sharded training's one cross-rank operation: export the gradients, ONE all-gather, and the merge of the ranks'
                 rows in rank order on every rank (vt_*_grads_export / vt_*_grads_merge; merge_gradients_host states the arithmetic);
                 owned / batch_count / agreed_steps are the static ownership and the epoch's step count

With HeadTrainer alone the decoder's FRONT (everything before `classifier`) is frozen: for ClassificationDecoder it is the
parameter-free 4x4 pool, so the head is the whole model; for AttentionClassificationDecoder it runs as in inference (BatchNorm on its
running statistics).  DecoderTrainer trains the attention decoder in full -- spatial_attention.*, feature_compress.* (running
statistics included), self_attention_post.* and, on a decoder with cross-attention, query_generator.* and cross_attention.*.  The channel
max of the spatial attention gives its gradient to the arg-max channel, the lowest index on a tie.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._runtime import stream_ptr, vp, workspace

SCHEDULES = ("constant", "constant_with_warmup", "linear", "cosine")
ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-8          # torch.optim.AdamW's defaults: the reference passes lr and weight_decay only


def lr_schedule(kind, step, warmup_steps, total_steps):
    """The factor the base learning rate is multiplied by at optimizer step `step` (0-based: the number of scheduler steps taken).
    constant: 1.  constant_with_warmup: step / max(1, warmup) below warmup, then 1.  linear: the same warm-up, then
    max(0, (T - step) / max(1, T - warmup)).  cosine: the same warm-up, then max(0, 0.5 (1 + cos(pi progress))) with
    progress = (step - warmup) / max(1, T - warmup)."""
    if kind not in SCHEDULES:
        raise ValueError(f"lr_scheduler_type {kind!r}: one of {', '.join(SCHEDULES)} expected")
    step, warmup, total = int(step), int(warmup_steps), int(total_steps)
    if kind == "constant":
        return 1.0
    if step < warmup:
        return step / max(1, warmup)
    if kind == "constant_with_warmup":
        return 1.0
    if kind == "linear":
        return max(0.0, (total - step) / max(1, total - warmup))
    progress = (step - warmup) / max(1, total - warmup)
    return max(0.0, 0.5 * (1.0 + math.cos(math.pi * progress)))


def split_indices(n, seed):
    """(train, val) index lists: val = the first max(1, int(0.1 n)) entries of torch.randperm(n) under a generator seeded with `seed`,
    train the rest.  (The reference's random_split draws from the global RNG, whose state depends on everything seeded before it:
    this permutation is reproducible from the seed alone and is NOT the reference's.)"""
    n = int(n)
    if n < 2:
        raise ValueError(f"{n} image(s): at least 2 are needed for a training and a validation set")
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(int(seed))).tolist()
    n_val = max(1, int(n * 0.1))
    return perm[n_val:], perm[:n_val]


def epoch_order(n_train, seed, epoch):
    """The order in which epoch `epoch` visits the positions 0 .. n_train - 1 of the training list: a fresh permutation per epoch."""
    g = torch.Generator().manual_seed(int(seed) * 1000003 + int(epoch) + 1)
    return torch.randperm(int(n_train), generator=g).tolist()


class FeatureCache:
    """Feature rows [capacity][F] fp32 and label rows [capacity][N] of the images, by slot, on `device` (host tensors work too: the
    index logic is the same).  `put` stores a batch under its keys, `gather` returns the rows of a list of keys in that order."""

    def __init__(self, capacity, feature_dim, num_classes, device="cuda", label_dtype=torch.float32):
        self.features = torch.zeros(int(capacity), int(feature_dim), dtype=torch.float32, device=device)
        self.labels = torch.zeros(int(capacity), int(num_classes), dtype=label_dtype, device=device)
        self.slot = {}

    def __len__(self):
        return len(self.slot)

    def __contains__(self, key):
        return key in self.slot

    @property
    def nbytes(self):
        return self.features.numel() * self.features.element_size() + self.labels.numel() * self.labels.element_size()

    def put(self, keys, features, labels):
        keys = list(keys)
        if features.shape[0] != len(keys) or labels.shape[0] != len(keys):
            raise ValueError("FeatureCache.put: one feature row and one label row per key")
        slots = []
        for k in keys:
            if k not in self.slot:
                if len(self.slot) >= self.features.shape[0]:
                    raise IndexError("FeatureCache is full")
                self.slot[k] = len(self.slot)
            slots.append(self.slot[k])
        idx = torch.as_tensor(slots, dtype=torch.long, device=self.features.device)
        self.features.index_copy_(0, idx, features.to(self.features.device, torch.float32))
        self.labels.index_copy_(0, idx, labels.to(self.labels.device, self.labels.dtype))

    def gather(self, keys):
        idx = torch.as_tensor([self.slot[k] for k in keys], dtype=torch.long, device=self.features.device)
        return self.features.index_select(0, idx), self.labels.index_select(0, idx)


class LatentCache:
    """The encoder's latents [16][h][w] fp32 of the images, one after the other in ONE flat fp32 arena on `device`, with (offset, h, w)
    per image, and their label rows -- what the full decoder trainer needs to skip the encoder after the first epoch (the front is
    trained, so its feature rows change; the latents do not).  The arena is sized up front for `capacity` images of at most
    `max_numel` floats each (16 (resolution / 8)^2: 1 MB at 1024 x 1024); `LatentCache.fits` is the memory rule: when that bound plus
    the labels exceeds the budget NOTHING is cached and every epoch re-encodes.  Host tensors work too: the index logic is the same."""

    def __init__(self, capacity, max_numel, num_classes, device="cuda", label_dtype=torch.float32):
        self.max_numel = int(max_numel)
        self.arena = torch.zeros(int(capacity) * self.max_numel, dtype=torch.float32, device=device)
        self.labels = torch.zeros(int(capacity), int(num_classes), dtype=label_dtype, device=device)
        self.entry, self.used = {}, 0                # key -> (slot, offset, C, h, w); floats of the arena in use

    @staticmethod
    def bytes_needed(capacity, max_numel, num_classes, label_bytes=4):
        return int(capacity) * (int(max_numel) * 4 + int(num_classes) * int(label_bytes))

    @classmethod
    def fits(cls, capacity, max_numel, num_classes, budget_bytes, label_bytes=4):
        return cls.bytes_needed(capacity, max_numel, num_classes, label_bytes) <= int(budget_bytes)

    def __len__(self):
        return len(self.entry)

    def __contains__(self, key):
        return key in self.entry

    @property
    def nbytes(self):
        """Bytes in use: the latents stored so far and their label rows."""
        return self.used * 4 + len(self.entry) * self.labels.shape[1] * self.labels.element_size()

    def shape(self, key):
        return self.entry[key][3:]

    def put(self, keys, latents, labels):
        keys = list(keys)
        if latents.dim() != 4 or latents.shape[0] != len(keys) or labels.shape[0] != len(keys):
            raise ValueError("LatentCache.put: latents [B, C, h, w] and one label row per key")
        _, C, h, w = latents.shape
        n = C * h * w
        if n > self.max_numel:
            raise ValueError(f"LatentCache.put: a latent of {n} floats exceeds the {self.max_numel} the arena was sized for")
        lat = latents.detach().to(self.arena.device, torch.float32).reshape(len(keys), n)
        for i, k in enumerate(keys):
            if k in self.entry:
                slot, off = self.entry[k][:2]
                if self.entry[k][2:] != (C, h, w):
                    raise ValueError(f"LatentCache.put: {k} was stored as {self.entry[k][2:]}, now {(C, h, w)}")
            else:
                if len(self.entry) >= self.labels.shape[0] or self.used + n > self.arena.numel():
                    raise IndexError("LatentCache is full")
                slot, off = len(self.entry), self.used
                self.entry[k] = (slot, off, C, h, w)
                self.used += n
            self.arena[off:off + n].copy_(lat[i])
            self.labels[slot].copy_(labels[i].to(self.labels.device, self.labels.dtype))

    def gather(self, keys):
        """(latents [B][C][h][w], labels [B][N]) of keys that share one latent shape, in that order."""
        keys = list(keys)
        shapes = {self.entry[k][2:] for k in keys}
        if len(shapes) != 1:
            raise ValueError(f"LatentCache.gather: one latent shape per batch expected, got {sorted(shapes)}")
        (C, h, w), = shapes
        n = C * h * w
        lat = torch.stack([self.arena[self.entry[k][1]:self.entry[k][1] + n] for k in keys]).view(len(keys), C, h, w)
        idx = torch.as_tensor([self.entry[k][0] for k in keys], dtype=torch.long, device=self.labels.device)
        return lat, self.labels.index_select(0, idx)

    def batches(self, order, batch_size):
        """The keys of `order` that are cached, as batches of up to batch_size keys of ONE latent shape each (batch statistics need
        one shape per batch): the bucket feeder's grouping (prefetch.BucketGrouper) keyed by (h, w), nothing forced out early."""
        from .prefetch import BucketGrouper
        keys = [k for k in order if k in self.entry]
        grouper = BucketGrouper(batch_size, max(1, len(keys)))
        out = []
        for k in keys:
            out.extend([key for key, _ in group] for _, group in grouper.add(k, self.shape(k), None))
        out.extend([key for key, _ in group] for _, group in grouper.flush())
        return out


def head_dropout_rates(decoder):
    """The Dropout rates of `classifier` (modules.py:401-418 / :318-331): 0.3, 0.2, 0.1 for the attention decoder, 0.3, 0.2 plain."""
    return (0.3, 0.2) if decoder._cfg[0] else (0.3, 0.2, 0.1)


def head_parameter_names(decoder):
    return [k for k in decoder.state_dict() if k.startswith("classifier.")]


def export_state_dict(decoder, read, names=None):
    """The decoder's full state_dict with every tensor of `names` (default: `classifier.*`) replaced by read(name) (a host tensor of the
    same shape): the keys torch.save writes for a checkpoint, in the decoder's order and dtypes; the other tensors are the decoder's
    own, unchanged."""
    names = set(head_parameter_names(decoder) if names is None else names)
    out = {}
    for k, v in decoder.state_dict().items():
        if k in names:
            t = read(k)
            if tuple(t.shape) != tuple(v.shape):
                raise ValueError(f"{k}: read {tuple(t.shape)}, the decoder holds {tuple(v.shape)}")
            out[k] = t.detach().to("cpu", v.dtype).clone()
        else:
            out[k] = v.detach().to("cpu").clone()
    return out


class _BlockTrainer:
    """What HeadTrainer and FrontTrainer share: one 256-B aligned device state block (parameters, gradients, Adam moments, the clip
    scalars) behind the entries `PREFIX + init / step / commit / read / write` of the C ABI.  A subclass sets PREFIX and `shapes`
    ({parameter name: shape}) and calls `_allocate`."""
    PREFIX = None

    def __init__(self, decoder, seed):
        self.decoder = decoder
        self.ctx = decoder._context()
        self.device = next(decoder.parameters()).device
        self.F = self.ctx.lib.vt_decoder_feature_dim(self.ctx.handle)
        self.seed, self.calls, self.t = int(seed), 0, 0

    def _allocate(self, unsupported):
        self._bytes = getattr(self.ctx.lib, self.PREFIX + "state_bytes")(self.ctx.handle)
        if self._bytes == 0:
            raise _lib.VTError(unsupported)
        self._buf = torch.empty(self._bytes + 256, dtype=torch.uint8, device=self.device)
        self._ptr = (self._buf.data_ptr() + 255) // 256 * 256
        self._call("init")

    def _state(self):
        return ctypes.c_void_p(self._ptr), self._bytes

    def _call(self, entry, *args):
        self.ctx.call(self.PREFIX + entry, *self._state(), *args, stream_ptr(self.device))

    def step(self, lr, weight_decay=0.0, betas=ADAM_BETAS, eps=ADAM_EPS):
        self.t += 1
        self._call("step", float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), self.t)

    def commit(self):
        """Write the state's tensors into the decoder's device tables: decoder(latent) then runs what was trained."""
        self._call("commit")

    def _read(self, kind, name, shape, dtype):
        out = torch.empty(shape, dtype=dtype, pin_memory=True)
        self._call("read", kind, name.encode() if name else None, ctypes.c_void_p(out.data_ptr()), out.numel() * out.element_size())
        torch.cuda.current_stream(self.device).synchronize()
        return out.clone()

    def parameter(self, name):
        return self._read(_lib.HEAD_PARAM, name, self.shapes[name], torch.float32)

    def gradient(self, name):
        return self._read(_lib.HEAD_GRAD, name, self.shapes[name], torch.float32)

    def write(self, kind, name, tensor):
        t = tensor.detach().to(self.device, torch.float32).contiguous()
        if tuple(t.shape) != self.shapes[name]:
            raise ValueError(f"{name}: expected {self.shapes[name]}, got {tuple(t.shape)}")
        self._call("write", kind, name.encode(), vp(t), t.numel() * 4)
        torch.cuda.current_stream(self.device).synchronize()        # (t may be freed when this returns)

    def grad_norm(self):
        """(total L2 norm, clip coefficient) of the last clip(): bytes 8..16 of the block's scalars { fp64 squared norm, fp32 norm,
        fp32 coefficient } (TrainScalars of csrc/vt_train.h, the one layout fact this module repeats)."""
        raw = self._read(_lib.HEAD_NORM, None, (16,), torch.uint8).numpy()
        return float(raw[8:12].view(np.float32)[0]), float(raw[12:16].view(np.float32)[0])

    def state_bytes(self):
        """The whole state block (for bit comparisons)."""
        torch.cuda.current_stream(self.device).synchronize()
        off = self._ptr - self._buf.data_ptr()
        return self._buf[off:off + self._bytes].cpu()

    # -- the gradient exchange of a sharded run (GradientExchange) --
    def grads_floats(self):
        """P: the floats of the block's gradient section, padding included."""
        return int(getattr(self.ctx.lib, self.PREFIX + "grads_floats")(self.ctx.handle))

    def export_gradients(self, out):
        """out (a contiguous fp32 device tensor or view of at least P floats, 16-B aligned) <- the gradient section, in stream order."""
        if out.dtype != torch.float32 or out.device != self.device or not out.is_contiguous():
            raise ValueError("export_gradients: a contiguous fp32 tensor on the trainer's device is expected")
        self._call("grads_export", vp(out), out.numel() * 4)

    def merge_gradients(self, src, stride, weights):
        """gradients <- the in-order weighted sum of K = len(weights) ranks' sections, rank r's at src[r * stride:] (merge_gradients_host
        states the arithmetic); every squared-norm partial is rewritten, so clip() and step() follow as after a backward.  `src` is an
        fp32 device tensor that holds all K sections and is not changed."""
        w = [float(x) for x in weights]
        K, P = len(w), self.grads_floats()
        if src.dtype != torch.float32 or src.device != self.device or not src.is_contiguous():
            raise ValueError("merge_gradients: a contiguous fp32 tensor on the trainer's device is expected")
        if 1 <= K <= 64 and int(stride) >= P and src.numel() < (K - 1) * int(stride) + P:      # (a K out of range is the library's to refuse)
            raise ValueError(f"merge_gradients: src holds {src.numel()} floats, {(K - 1) * int(stride) + P} needed")
        self._call("grads_merge", vp(src), int(stride), K, (ctypes.c_double * max(1, K))(*w))

    def optimizer_state_sha256(self, h=None):
        """SHA-256 over the parameters, Adam m and Adam v of every tensor, in the order of `shapes` (ranks of a sharded run compare it)."""
        import hashlib
        h = hashlib.sha256() if h is None else h
        for kind in (_lib.HEAD_PARAM, _lib.HEAD_ADAM_M, _lib.HEAD_ADAM_V):
            for name, shape in self.shapes.items():
                h.update(self._read(kind, name, shape, torch.float32).numpy().tobytes())
        return h


class HeadTrainer(_BlockTrainer):
    """Device state of the classifier head of `decoder` (on a HIP device) and the calls that train it.  Every method queues work on the
    current stream and returns; `losses()`, `grad_norm()`, `parameter()` and `gradient()` synchronise."""
    PREFIX = "vt_head_"

    def __init__(self, decoder, loss="bce", focal_alpha=1.0, focal_gamma=2.0, class_weights=None, dropout=None, seed=0):
        super().__init__(decoder, seed)
        self.N = decoder.num_classes
        if loss not in _lib.HEAD_LOSS_KINDS:
            raise ValueError(f"loss {loss!r}: one of {', '.join(_lib.HEAD_LOSS_KINDS)} expected")
        self.loss_kind, self.alpha, self.gamma = _lib.HEAD_LOSS_KINDS[loss], float(focal_alpha), float(focal_gamma)
        self.class_weights = None
        if class_weights is not None:
            self.class_weights = torch.as_tensor(np.asarray(class_weights, dtype=np.float32)).to(self.device).contiguous()
            if self.class_weights.shape != (self.N,):
                raise ValueError(f"expected {self.N} class weights")
        if loss == "class_balanced" and self.class_weights is None:
            raise ValueError("the class-balanced loss needs class_weights (losses.class_balanced_weights)")
        rates = head_dropout_rates(decoder) if dropout is None else tuple(float(p) for p in dropout)
        if len(rates) != len(head_dropout_rates(decoder)):
            raise ValueError(f"{len(head_dropout_rates(decoder))} dropout rates expected")
        self.dropout = (ctypes.c_float * len(rates))(*rates)
        self.shapes = {k: tuple(v.shape) for k, v in decoder.state_dict().items() if k.startswith("classifier.")}
        self._allocate("this decoder's head cannot be trained on the device: every linear layer's input width must be a multiple "
                       f"of 256 (feature width {self.F}; latent_channels = 16 gives 256 / 512)")

    def _ws(self, B):
        need = self.ctx.lib.vt_head_workspace_bytes(self.ctx.handle, int(B))
        if need == 0:
            raise _lib.VTError(f"unsupported head batch size {B}")
        _, ptr = workspace(self.device, need, "head")
        return ctypes.c_void_p(ptr), need

    def features(self, latent):
        """The decoder front's rows [B][F] of a latent batch (vt_decode_features)."""
        x = self.decoder._latent(latent)
        B, _, h, w = x.shape
        out = torch.empty(B, self.F, dtype=torch.float32, device=x.device)
        need = self.ctx.lib.vt_decode_workspace_bytes(self.ctx.handle, B, h, w)
        _, ptr = workspace(x.device, need)
        self.ctx.call("vt_decode_features", vp(x), B, h, w, vp(out), ctypes.c_void_p(ptr), need, stream_ptr(x.device))
        return out

    def _features_in(self, features):
        f = features.detach().to(self.device, torch.float32).contiguous()
        if f.dim() != 2 or f.shape[1] != self.F:
            raise ValueError(f"expected features [B, {self.F}], got {tuple(f.shape)}")
        return f

    def forward(self, features):
        """Eval-mode logits [B][N] of the state's parameters."""
        f = self._features_in(features)
        out = torch.empty(f.shape[0], self.N, dtype=torch.float32, device=self.device)
        self._call("forward", vp(f), f.shape[0], vp(out), *self._ws(f.shape[0]))
        return out

    def forward_backward(self, features, labels, loss_scale=1.0, train=True, step=None, return_logits=False, return_masks=False,
                         return_d_features=False):
        """One micro-batch: forward (train: with dropout), loss, backward, gradients ADDED to the state's.  loss_scale x loss goes
        into the ring at slot step % HEAD_RING; `step` (default: the number of calls so far) also keys the dropout masks.  Returns
        those of (logits, masks, d loss / d features) that were asked for: None, the one, or a tuple in this order."""
        f = self._features_in(features)
        y = labels.detach().to(self.device)
        if y.dtype == torch.bool:
            y = y.view(torch.uint8)
        elif y.dtype not in (torch.float32, torch.uint8):
            y = y.to(torch.float32)
        y = y.contiguous()
        B = f.shape[0]
        if tuple(y.shape) != (B, self.N):
            raise ValueError(f"expected labels [{B}, {self.N}], got {tuple(y.shape)}")
        step = self.calls if step is None else int(step)
        logits = torch.empty(B, self.N, dtype=torch.float32, device=self.device) if return_logits else None
        masks = None
        if return_masks:
            widths = [self.shapes[f"classifier.{4 * i}.bias"][0] for i in range(len(self.dropout))]
            masks = torch.empty(B * sum(widths), dtype=torch.uint8, device=self.device)
        d = torch.empty(B, self.F, dtype=torch.float32, device=self.device) if return_d_features else None
        self._call("forward_backward_dx" if return_d_features else "forward_backward", vp(f), vp(y),
                   _lib.VT_U8 if y.dtype == torch.uint8 else _lib.VT_F32, B, self.loss_kind, self.alpha, self.gamma, vp(self.class_weights),
                   float(loss_scale), int(bool(train)), self.dropout, self.seed, step, vp(logits), vp(masks),
                   *([vp(d)] if return_d_features else []), *self._ws(B))
        self.calls = step + 1
        if return_masks:
            out, off = [], 0
            for wd in widths:
                out.append(masks[off:off + B * wd].view(B, wd))
                off += B * wd
            masks = out
        asked = [v for v, want in ((logits, return_logits), (masks, return_masks), (d, return_d_features)) if want]
        return None if not asked else asked[0] if len(asked) == 1 else tuple(asked)

    def clip(self, max_norm):
        self._call("clip", float(max_norm))

    def losses(self):
        """The loss ring, fp64 [HEAD_RING]: slot s holds loss_scale x loss of the last call whose step % HEAD_RING was s."""
        return self._read(_lib.HEAD_LOSS_RING, None, (_lib.HEAD_RING,), torch.float64)

    def state_dict(self):
        """The decoder's full state_dict with the trained head (export_state_dict)."""
        return export_state_dict(self.decoder, self.parameter, self.shapes)


# ---- the attention decoder's front -------------------------------------------------------------------------------------------------
FRONT_PREFIXES = ("spatial_attention.", "feature_compress.", "self_attention_post.")
FRONT_BUFFERS = {"feature_compress.1.running_mean": _lib.FRONT_BN_MEAN, "feature_compress.1.running_var": _lib.FRONT_BN_VAR,
                 "feature_compress.1.num_batches_tracked": _lib.FRONT_BN_TRACKED}


CROSS_PREFIXES = ("query_generator.", "cross_attention.")


def front_trainable(decoder):
    """Can train.FrontTrainer train this decoder's front?  The attention decoder, with or without cross-attention (vt_front_state_bytes);
    with it, train.CrossTrainer trains the piece behind the front."""
    return not decoder._cfg[0]


class FrontTrainer(_BlockTrainer):
    """Device state of the FRONT of an attention decoder (spatial_attention.*, feature_compress.*, self_attention_post.*; vt_front_* of
    the C ABI, csrc/train_front.hip) and the calls that train it.  `forward(latent, train=True)` runs BatchNorm on the batch's
    statistics (and updates the running ones) and drops softmax weights at `attention_dropout`; `backward(d_features)` belongs to the
    last training-mode forward and ADDS the gradients of every front tensor.  The channel max of the spatial attention sends its
    gradient to the arg-max channel, the lowest index on a tie.  On a decoder with cross-attention the same 17 tensors are trained and
    the rows `forward` returns, in both modes, are the rows cross-attention reads (CrossTrainer.forward turns them into the head's feature
    rows), and `backward` takes the gradient with respect to those rows (CrossTrainer.backward's result).  grad_norm() is that of the last
    DecoderTrainer.clip()."""
    PREFIX = "vt_front_"

    def __init__(self, decoder, attention_dropout=0.1, seed=0):
        super().__init__(decoder, seed)
        self.heads = decoder._cfg[4]
        self.p = float(attention_dropout)
        if not 0.0 <= self.p < 1.0:
            raise ValueError(f"attention_dropout {attention_dropout} outside [0, 1)")
        sd = decoder.state_dict()
        self.shapes = {k: tuple(v.shape) for k, v in sd.items() if k.startswith(FRONT_PREFIXES) and k not in FRONT_BUFFERS}
        self.buffers = {k: tuple(sd[k].shape) for k in FRONT_BUFFERS}
        self._last = None
        self._allocate("this decoder's front cannot be trained on the device: an attention decoder with latent_channels = 16 and "
                       "attention_heads in {1, 2, 4, 8} is expected")
        self.write_buffer("feature_compress.1.num_batches_tracked", sd["feature_compress.1.num_batches_tracked"])

    def _ws(self, B, h, w):
        need = self.ctx.lib.vt_front_workspace_bytes(self.ctx.handle, int(B), int(h), int(w))
        if need == 0:
            raise _lib.VTError(f"unsupported front batch {B} x {h} x {w}")
        _, ptr = workspace(self.device, need, "front")
        return ctypes.c_void_p(ptr), need

    def forward(self, latent, train=False, step=None, return_mask=False):
        """Feature rows [B][F].  train=True keeps what backward() needs (until the next forward)."""
        x = self.decoder._latent(latent)
        B, _, h, w = x.shape
        step = self.calls if step is None else int(step)
        out = torch.empty(B, self.F, dtype=torch.float32, device=self.device)
        mask = torch.empty(B, self.heads, 64, 64, dtype=torch.uint8, device=self.device) if return_mask and train else None
        self._call("forward", vp(x), B, h, w, int(bool(train)), self.p, self.seed, step, vp(out), vp(mask), *self._ws(B, h, w))
        self._last = (x, step) if train else None
        if train:
            self.calls = step + 1
        return (out, mask) if return_mask else out

    def backward(self, d_features):
        if self._last is None:
            raise RuntimeError("FrontTrainer.backward needs the training-mode forward of the same batch before it")
        x, step = self._last
        B, _, h, w = x.shape
        d = d_features.detach().to(self.device, torch.float32).contiguous()
        if tuple(d.shape) != (B, self.F):
            raise ValueError(f"expected d_features [{B}, {self.F}], got {tuple(d.shape)}")
        self._call("backward", vp(x), vp(d), B, h, w, self.p, self.seed, step, *self._ws(B, h, w))
        self._last = None

    def buffer(self, name):
        """feature_compress.1.running_mean / running_var (fp32 [8]) or num_batches_tracked (int64 scalar)."""
        tracked = FRONT_BUFFERS[name] == _lib.FRONT_BN_TRACKED
        return self._read(FRONT_BUFFERS[name], None, self.buffers[name], torch.int64 if tracked else torch.float32)

    def write_buffer(self, name, tensor):
        tracked = FRONT_BUFFERS[name] == _lib.FRONT_BN_TRACKED
        t = tensor.detach().to(self.device, torch.int64 if tracked else torch.float32).contiguous()
        self._call("write", FRONT_BUFFERS[name], None, vp(t), t.numel() * t.element_size())
        torch.cuda.current_stream(self.device).synchronize()

    def tensor(self, name):
        """A front entry of the state_dict, parameter or BatchNorm buffer, as a host tensor."""
        return self.buffer(name) if name in self.buffers else self.parameter(name)

    def state_dict(self):
        """The decoder's full state_dict with the trained front (the reference's keys, the three BatchNorm buffers included); the head's
        tensors are the decoder's own."""
        return export_state_dict(self.decoder, self.tensor, [*self.shapes, *self.buffers])


class CrossTrainer(_BlockTrainer):
    """Device state of query_generator.* and cross_attention.* of an attention decoder with cross-attention (vt_cross_* of the C ABI,
    csrc/train_cross.hip) and the calls that train it.  `forward(x)` takes the front's rows [B][512] (FrontTrainer.forward) and returns
    the head's feature rows; the piece has no dropout and no normalisation layer, so there is one mode.  `backward(d_features)` belongs
    to the last forward, ADDS the gradients of the ten tensors and returns d loss / d x for FrontTrainer.backward.  The workspace that
    carries q, u and o from forward to backward is this trainer's own, so several trainers on one device may interleave their calls."""
    PREFIX = "vt_cross_"

    def __init__(self, decoder, seed=0):
        super().__init__(decoder, seed)
        self.shapes = {k: tuple(v.shape) for k, v in decoder.state_dict().items() if k.startswith(CROSS_PREFIXES)}
        self._last, self._wsbuf = None, None
        self._allocate("this decoder has no cross-attention that can be trained on the device: an attention decoder with cross-attention, "
                       "latent_channels = 16 and attention_heads in {1, 2, 4, 8} is expected")

    def _ws(self, B):
        need = self.ctx.lib.vt_cross_workspace_bytes(self.ctx.handle, int(B))
        if need == 0:
            raise _lib.VTError(f"unsupported cross-attention batch size {B}")
        if self._wsbuf is None or self._wsbuf.numel() < need + 256:     # this trainer's own: backward reads what ITS forward left
            self._wsbuf = torch.empty(int(need) + 256, dtype=torch.uint8, device=self.device)
        return ctypes.c_void_p((self._wsbuf.data_ptr() + 255) // 256 * 256), need

    def _rows(self, t, what):
        r = t.detach().to(self.device, torch.float32).contiguous()
        if r.dim() != 2 or r.shape[1] != self.F:
            raise ValueError(f"expected {what} [B, {self.F}], got {tuple(r.shape)}")
        return r

    def forward(self, x):
        """Feature rows [B][F] of the front's rows x; keeps what backward() needs (until the next forward)."""
        x = self._rows(x, "x")
        out = torch.empty_like(x)
        self._call("forward", vp(x), x.shape[0], vp(out), *self._ws(x.shape[0]))
        self._last = x
        return out

    def backward(self, d_features):
        if self._last is None:
            raise RuntimeError("CrossTrainer.backward needs the forward of the same batch before it")
        x = self._last
        d = self._rows(d_features, "d_features")
        if d.shape != x.shape:
            raise ValueError(f"expected d_features {tuple(x.shape)}, got {tuple(d.shape)}")
        d_x = torch.empty_like(x)
        self._call("backward", vp(x), vp(d), x.shape[0], vp(d_x), *self._ws(x.shape[0]))
        self._last = None
        return d_x

    def state_dict(self):
        """The decoder's full state_dict with the trained cross-attention tensors; the others are the decoder's own."""
        return export_state_dict(self.decoder, self.parameter, self.shapes)


class DecoderTrainer:
    """The attention decoder trained in full: FrontTrainer + HeadTrainer, and CrossTrainer between them when the decoder has
    cross-attention.  One forward_backward runs latent -> front (training mode) [-> cross-attention] -> head forward / loss / backward
    with d loss / d features [-> cross-attention backward] -> front backward; clip() is ONE clip_grad_norm_ over all blocks."""

    def __init__(self, decoder, loss="bce", focal_alpha=1.0, focal_gamma=2.0, class_weights=None, dropout=None, attention_dropout=0.1, seed=0):
        self.decoder = decoder
        self.head = HeadTrainer(decoder, loss, focal_alpha, focal_gamma, class_weights, dropout, seed)
        self.front = FrontTrainer(decoder, attention_dropout, seed)
        self.cross = CrossTrainer(decoder, seed) if decoder._cfg[3] else None
        self.ctx, self.device, self.N, self.F = self.head.ctx, self.head.device, self.head.N, self.head.F

    def forward(self, latent):
        """Eval-mode logits: the front on its running statistics, no dropout (the reference's decoder.eval())."""
        rows = self.front.forward(latent, train=False)
        return self.head.forward(rows if self.cross is None else self.cross.forward(rows))

    def forward_backward(self, latent, labels, loss_scale=1.0, train=True, step=None, return_logits=False):
        step = self.head.calls if step is None else int(step)
        feats = self.front.forward(latent, train=True, step=step)
        if self.cross is not None:
            feats = self.cross.forward(feats)
        out = self.head.forward_backward(feats, labels, loss_scale, train, step, return_logits, return_d_features=True)
        logits, d_feats = out if return_logits else (None, out)
        self.front.backward(d_feats if self.cross is None else self.cross.backward(d_feats))
        return logits

    def clip(self, max_norm):
        if self.cross is None:
            self.ctx.call("vt_train_clip", *self.head._state(), *self.front._state(), float(max_norm), stream_ptr(self.device))
        else:
            self.ctx.call("vt_train_clip3", *self.head._state(), *self.front._state(), *self.cross._state(), float(max_norm),
                          stream_ptr(self.device))

    def step(self, lr, weight_decay=0.0, betas=ADAM_BETAS, eps=ADAM_EPS):
        self.head.step(lr, weight_decay, betas, eps)
        self.front.step(lr, weight_decay, betas, eps)
        if self.cross is not None:
            self.cross.step(lr, weight_decay, betas, eps)

    def commit(self):
        self.front.commit()
        if self.cross is not None:
            self.cross.commit()
        self.head.commit()

    def losses(self):
        return self.head.losses()

    def grad_norm(self):
        return self.head.grad_norm()

    def _tensor(self, k):
        if k in self.head.shapes:
            return self.head.parameter(k)
        if self.cross is not None and k in self.cross.shapes:
            return self.cross.parameter(k)
        return self.front.tensor(k)

    def state_dict(self):
        """The decoder's full state_dict with the head's, the front's and the cross-attention's tensors read from the device."""
        names = [*self.head.shapes, *self.front.shapes, *self.front.buffers, *(self.cross.shapes if self.cross is not None else ())]
        return export_state_dict(self.decoder, self._tensor, names)

    # -- the gradient exchange of a sharded run: the blocks side by side in ONE fp32 buffer [P_front (+ P_cross) + P_head] --
    def blocks(self):
        return [b for b in (self.front, self.cross, self.head) if b is not None]

    def grads_floats(self):
        return sum(b.grads_floats() for b in self.blocks())

    def export_gradients(self, out):
        off = 0
        for b in self.blocks():
            P = b.grads_floats()
            b.export_gradients(out[off:off + P])
            off += P

    def merge_gradients(self, src, stride, weights):
        """Every block from its range of the K rows of `src` (row r starts at float r * stride; stride >= grads_floats())."""
        if not src.is_contiguous():
            raise ValueError("merge_gradients: a contiguous fp32 tensor on the trainer's device is expected")
        flat, off = src.view(-1), 0
        for b in self.blocks():
            b.merge_gradients(flat[off:], stride, weights)
            off += b.grads_floats()

    def optimizer_state_sha256(self):
        h = None
        for b in self.blocks():
            h = b.optimizer_state_sha256(h)
        return h


# ---- sharded training: static ownership and the gradient exchange -------------------------------------------------------------------
RANK_SEED_STRIDE = 1000003                             # the trainer seed of rank r is seed + RANK_SEED_STRIDE * r: other dropout masks
EXCHANGE_TAIL = 4                                      # floats behind a rank's gradients in the exchanged row: its image count (int32) + 3 spare


def owned(items, rank, world):
    """Rank `rank`'s share of a list under static ownership: items[rank::world]."""
    return list(items)[int(rank)::int(world)]


def batch_count(n_items, batch_size):
    return (int(n_items) + int(batch_size) - 1) // int(batch_size)


def agreed_steps(local_batch_counts):
    """The optimizer steps of one epoch: the maximum over the ranks of their local batch counts (a rank that has run out of batches
    joins the remaining exchanges with weight 0)."""
    return max(int(c) for c in local_batch_counts)


def merge_gradients_host(blocks, weights):
    """What vt_*_grads_merge computes, in numpy: blocks [K][P] fp32 (or a list of K arrays), weights K floats ->
    fp32 [P] with out[e] = (float) acc, acc = 0.0 (fp64); for r = 0 .. K-1 in that order: acc = acc + w[r] * (double)blocks[r][e] --
    the product rounded to fp64, then the sum rounded to fp64, one final cast to fp32."""
    rows = [np.asarray(b, dtype=np.float32).reshape(-1) for b in blocks]
    w = [np.float64(x) for x in weights]
    if len(rows) != len(w) or not rows:
        raise ValueError("merge_gradients_host: one weight per block, at least one block")
    acc = np.zeros(rows[0].shape, dtype=np.float64)
    for r, row in enumerate(rows):
        prod = w[r] * row.astype(np.float64)           # (numpy rounds each ufunc's result: nothing is fused)
        acc = acc + prod
    return acc.astype(np.float32)


def exchange_weights(counts):
    """w[r] = n_r / sum n: the merged gradient of per-rank batch-mean gradients is then the concatenated batch's mean gradient."""
    total = sum(int(c) for c in counts)
    if total <= 0:
        raise ValueError("no rank brought an image to this step")
    return [int(c) / total for c in counts]


class GradientExchange:
    """The one cross-rank operation of a training step: every rank exports its gradients (all blocks of `trainer`, HeadTrainer or
    DecoderTrainer) and its image count into one row, ONE collective gathers the rows (all_gather_into_tensor on RCCL, all_gather into
    chunks on gloo, as sharding.all_gather_logits chooses), and every rank merges them itself, on the device, in rank order.  Same
    bytes in, same kernel: the ranks' states stay bit-identical and nothing is broadcast.  Reading the K counts is the step's one host
    synchronisation.  Without a process group, or on a one-rank group without force_collective, exchange() does nothing."""

    def __init__(self, trainer, group=None, force_collective=False):
        import torch.distributed as dist
        self.trainer, self.group, self.device = trainer, group, trainer.device
        grouped = group is not None and dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size(group) if grouped else 1
        self.active = grouped and (self.world > 1 or bool(force_collective))
        self.backend = dist.get_backend(group) if grouped else None
        if self.world > 64:
            raise ValueError(f"{self.world} ranks: the gradient merge takes at most 64")
        self.P = trainer.grads_floats()
        self.row = self.P + EXCHANGE_TAIL
        self.calls, self.last_counts = 0, None
        if self.active:
            self._mine = torch.zeros(self.row, dtype=torch.float32, device=self.device)
            self._all = torch.zeros(self.world * self.row, dtype=torch.float32, device=self.device)

    @property
    def bytes_received_per_step(self):
        return (self.world - 1) * 4 * self.row

    def exchange(self, n_local):
        """After forward_backward (or none: n_local = 0, the gradients are the zeros the last step left), before clip / step.
        Returns the ranks' image counts."""
        if not self.active:
            return [int(n_local)]
        import torch.distributed as dist
        self.trainer.export_gradients(self._mine[:self.P])
        self._mine[self.P:].view(torch.int32).copy_(torch.tensor([int(n_local), 0, 0, 0], dtype=torch.int32), non_blocking=True)
        if self.backend == "gloo":
            parts = [torch.empty(self.row, dtype=torch.float32) for _ in range(self.world)]
            dist.all_gather(parts, self._mine.cpu(), group=self.group)
            counts = [int(p[self.P:].view(torch.int32)[0]) for p in parts]
            self._all.copy_(torch.cat(parts))
        else:
            dist.all_gather_into_tensor(self._all, self._mine, group=self.group)
            counts = self._all.view(self.world, self.row)[:, self.P:].contiguous().view(torch.int32)[:, 0].cpu().tolist()
        self.trainer.merge_gradients(self._all, self.row, exchange_weights(counts))
        self.calls += 1
        self.last_counts = counts
        return counts
