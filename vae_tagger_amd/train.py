"""Training of the decoder's classifier head on the GPU (vt_head_* of the C ABI; csrc/train_head.hip): what the loop body of the
reference's train_decoder.py (train_decoder.py:173-216) does to `classifier.*`.

  lr_schedule    the four learning-rate schedules of the reference's get_scheduler call, as closed forms evaluated on the host
  split_indices / epoch_order    the train / validation split and the per-epoch training order, from the seed alone
  FeatureCache   the decoder front's feature rows and the labels of every image, kept on the device after the first epoch
  HeadTrainer    the device state (parameters, gradients, Adam moments, loss ring) and its forward_backward / clip / step / commit

The decoder's FRONT (everything before `classifier`) is frozen: for ClassificationDecoder it is the parameter-free 4x4 pool, so the
head is the whole model; for AttentionClassificationDecoder it runs as in inference (BatchNorm on its running statistics).
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


def head_dropout_rates(decoder):
    """The Dropout rates of `classifier` (modules.py:401-418 / :318-331): 0.3, 0.2, 0.1 for the attention decoder, 0.3, 0.2 plain."""
    return (0.3, 0.2) if decoder._cfg[0] else (0.3, 0.2, 0.1)


def head_parameter_names(decoder):
    return [k for k in decoder.state_dict() if k.startswith("classifier.")]


def export_state_dict(decoder, read_parameter):
    """The decoder's full state_dict with every `classifier.*` tensor replaced by read_parameter(name) (a host fp32 tensor of the same
    shape): the keys torch.save writes for a checkpoint; the frozen tensors are the decoder's own, unchanged."""
    out = {}
    for k, v in decoder.state_dict().items():
        if k.startswith("classifier."):
            t = read_parameter(k)
            if tuple(t.shape) != tuple(v.shape):
                raise ValueError(f"{k}: read {tuple(t.shape)}, the decoder holds {tuple(v.shape)}")
            out[k] = t.detach().to("cpu", v.dtype).clone()
        else:
            out[k] = v.detach().to("cpu").clone()
    return out


class HeadTrainer:
    """Device state of the classifier head of `decoder` (on a HIP device) and the calls that train it.  Every method queues work on the
    current stream and returns; `losses()`, `grad_norm()`, `parameter()` and `gradient()` synchronise."""

    def __init__(self, decoder, loss="bce", focal_alpha=1.0, focal_gamma=2.0, class_weights=None, dropout=None, seed=0):
        self.decoder = decoder
        self.ctx = decoder._context()
        self.device = next(decoder.parameters()).device
        self.N = decoder.num_classes
        self.F = self.ctx.lib.vt_decoder_feature_dim(self.ctx.handle)
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
        self.seed, self.calls, self.t = int(seed), 0, 0
        self.shapes = {k: tuple(v.shape) for k, v in decoder.state_dict().items() if k.startswith("classifier.")}
        self._bytes = self.ctx.lib.vt_head_state_bytes(self.ctx.handle)
        if self._bytes == 0:
            raise _lib.VTError("this decoder's head cannot be trained on the device: every linear layer's input width must be a multiple "
                               f"of 256 (feature width {self.F}; latent_channels = 16 gives 256 / 512)")
        self._buf = torch.empty(self._bytes + 256, dtype=torch.uint8, device=self.device)
        self._ptr = (self._buf.data_ptr() + 255) // 256 * 256
        self.ctx.call("vt_head_init", ctypes.c_void_p(self._ptr), self._bytes, stream_ptr(self.device))

    def _state(self):
        return ctypes.c_void_p(self._ptr), self._bytes

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
        ws, need = self._ws(f.shape[0])
        self.ctx.call("vt_head_forward", *self._state(), vp(f), f.shape[0], vp(out), ws, need, stream_ptr(self.device))
        return out

    def forward_backward(self, features, labels, loss_scale=1.0, train=True, step=None, return_logits=False, return_masks=False):
        """One micro-batch: forward (train: with dropout), loss, backward, gradients ADDED to the state's.  loss_scale x loss goes
        into the ring at slot step % HEAD_RING; `step` (default: the number of calls so far) also keys the dropout masks."""
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
        ws, need = self._ws(B)
        self.ctx.call("vt_head_forward_backward", *self._state(), vp(f), vp(y), _lib.VT_U8 if y.dtype == torch.uint8 else _lib.VT_F32, B,
                      self.loss_kind, self.alpha, self.gamma, vp(self.class_weights), float(loss_scale), int(bool(train)), self.dropout,
                      self.seed, step, vp(logits), vp(masks), ws, need, stream_ptr(self.device))
        self.calls = step + 1
        if return_masks:
            out, off = [], 0
            for wd in widths:
                out.append(masks[off:off + B * wd].view(B, wd))
                off += B * wd
            masks = out
        if return_logits and return_masks:
            return logits, masks
        return logits if return_logits else masks

    def clip(self, max_norm):
        self.ctx.call("vt_head_clip", *self._state(), float(max_norm), stream_ptr(self.device))

    def step(self, lr, weight_decay=0.0, betas=ADAM_BETAS, eps=ADAM_EPS):
        self.t += 1
        self.ctx.call("vt_head_step", *self._state(), float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), self.t,
                      stream_ptr(self.device))

    def commit(self):
        """Write the parameters into the decoder's device tables: decoder(latent) then runs the trained head."""
        self.ctx.call("vt_head_commit", *self._state(), stream_ptr(self.device))

    def _read(self, kind, name, shape, dtype):
        out = torch.empty(shape, dtype=dtype, pin_memory=True)
        self.ctx.call("vt_head_read", *self._state(), kind, name.encode() if name else None, ctypes.c_void_p(out.data_ptr()),
                      out.numel() * out.element_size(), stream_ptr(self.device))
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
        self.ctx.call("vt_head_write", *self._state(), kind, name.encode(), vp(t), t.numel() * 4, stream_ptr(self.device))
        torch.cuda.current_stream(self.device).synchronize()        # (t may be freed when this returns)

    def losses(self):
        """The loss ring, fp64 [HEAD_RING]: slot s holds loss_scale x loss of the last call whose step % HEAD_RING was s."""
        return self._read(_lib.HEAD_LOSS_RING, None, (_lib.HEAD_RING,), torch.float64)

    def grad_norm(self):
        """(total L2 norm, clip coefficient) of the last clip()."""
        raw = self._read(_lib.HEAD_NORM, None, (16,), torch.uint8).numpy()
        return float(raw[8:12].view(np.float32)[0]), float(raw[12:16].view(np.float32)[0])

    def state_dict(self):
        """The decoder's full state_dict with the trained head (export_state_dict)."""
        return export_state_dict(self.decoder, self.parameter)
