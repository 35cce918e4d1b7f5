"""Training of the VAE on the GPU: the reference's train_vae.py (lines 28-299) -- three encodes, the anchor's decode, reconstruction + KL +
triplet loss, clip_grad_norm_, AdamW under a learning-rate schedule, validation and checkpoints per epoch.

    python -m vae_tagger_amd.train_vae --json_path data.json --tags_csv_path tags.csv [--vae_checkpoint ae.safetensors | --vae_config_path cfg.json]
        [--use_bucketing] [--max_grad_norm 1.0] [--resume_from vae_output/checkpoint-4] ...
    torchrun --nproc-per-node 8 -m vae_tagger_amd.train_vae ... --train_batch_size 1 --sharded

  optim_layout   where every tensor lies in the optimiser's arenas (the mirror of vt_vae_optim_layout)
  VAETrainer     the parameters and the Adam moments in three fp32 arenas, and the step on them: forward_backward
                 (vae_backward.vae_loss_and_grads on views of the parameter arena: no copy), clip (vt_vae_optim_norm: clip_grad_norm_ over the
                 244 gradient tensors where they lie), step (vt_vae_optim_step: AdamW with the clip's scale folded in), commit into a loaded model
  VAEGradientExchange   --sharded's one cross-rank operation per step: export into a row of the arenas' layout (vt_vae_grads_export), the
                 ranks' slices cross, every rank merges the tiles it owns in rank order (vt_vae_grads_merge; merge_rows_host is its mirror), the
                 merged slices are gathered; clip and step then run on views into the merged row
  accumulate_rows_host   the numpy mirror of vt_vae_grads_accumulate, the pass behind VAETrainer.accumulate / accumulated: the gradients of
                 train_full's micro-steps summed in one row of the arenas' layout (train_vae's own CLI has no accumulation: the reference's has none)
  train / main   the CLI: the reference's flags and defaults; per epoch a validation pass (evaluate_vae.run_checkpoint) and the reference's files

What differs from the reference, on purpose.  The train / validation split and the epoch order come from the seed alone (train.split_indices,
train.epoch_order), triplets are drawn per epoch and anchor (evaluate_vae.sample_triplet with seed * 1000003 + epoch + 1 over the training list),
and the posterior's noise is the device's counter-based normal keyed on --seed and on the count of anchors consumed since step 0 -- so two runs, and
a run that was resumed, write the same bytes.  With --use_bucketing a batch has one bucket and the positive and the negative are resized to the
ANCHOR's bucket (evaluate_vae's rule).  The positive and the negative are not decoded (the reference decodes them and throws the result away).
Nothing is read back per step: the running loss sum stays on the device and is read, with the health word, every --logging_steps and at the end
of an epoch.  fp32 parameters and moments, bf16 MFMA operands: --mixed_precision and the other flags of IGNORED_ARGUMENTS are accepted and ignored.
Not here: gradient accumulation (train_full has it: VAETrainer.accumulate is its VAE side) or checkpointing, the contrastive term,
AdaptiveLossWeights.

--sharded (under torchrun, one rank per GPU; the reference runs under `accelerate`).  --train_batch_size is per rank.  The epoch is planned as
without the flag, at the global batch B * world, and rank r takes the contiguous slice [r B, (r + 1) B) of every global batch with
first_image = images + r B: a run at world K and batch B sees the batches of the one-device run at batch K B -- the same triplets, the same
noise (keyed on the global image index), steps_per_epoch, learning rates and `images` -- and differs from it in summation order only.  Rank r of K
owns tiles [r S, (r + 1) S) of the gradient row, S = ceil(T / K): per step it sends and receives 2 (K - 1) / K of the row (a ring all-reduce's
traffic; a formula -- no multi-GPU scaling figure has been measured).  The weights w_r = n_r / sum n come from the plan, so nothing is read
back and no count is exchanged; a rank whose slice is empty skips forward and backward and joins at weight 0.  What is optimised is
sum_r w_r L_r: with kl = 0 (the default simplified loss) the concatenated batch's loss, since MSE and the triplet term are batch means; under
--full_vae_loss the log(1 + mean KL / 10000) term is taken PER RANK (what DDP computes), which is not the concatenated batch's.  Every rank
keeps the whole state and applies the same bytes: nothing is broadcast, and the run fails if the ranks' state digests differ.  Rank 0 alone
prints, validates and writes files (train_report.json gains "sharded"); the others wait at a barrier.  VT_CLI_GLOO=1 (ranks share a GPU; the
rows go through the CPU) and VT_CLI_ONE_RANK_GROUP=1 (one rank, the exchange forced) are rehearsals, as in train_decoder.  Sharded
validation and a ZeRO-style sharded optimiser are not here.
"""
import argparse
import ctypes
import hashlib
import json
import math
import os
import time
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from .train import ADAM_BETAS, ADAM_EPS, SCHEDULES, epoch_order, lr_schedule, split_indices

TILE, CHUNK = _lib.VAE_OPTIM_TILE, _lib.VAE_OPTIM_CHUNK
IGNORED_ARGUMENTS = ("mixed_precision", "cudnn_benchmark", "cudnn_deterministic", "num_workers", "prefetch_factor",
                     "enable_xformers_memory_efficient_attention")
TRIPLET_SEED_STRIDE = 1000003
MODEL_FILE, OPTIMIZER_FILE, STATE_FILE = "diffusion_pytorch_model.safetensors", "optimizer.safetensors", "state.json"


# ---- the arenas' layout (host) ---------------------------------------------------------------------------------------------------------
def optim_layout(numels):
    """(offsets, total) in floats: tensor i owns ceil(numel / TILE) tiles of TILE floats, slots follow each other in the order given.
    The mirror of vt_vae_optim_layout (tests compare the two)."""
    numels = [int(n) for n in numels]
    if not numels or any(n <= 0 for n in numels):
        raise ValueError("optim_layout: at least one tensor, every numel positive")
    offsets, off = [], 0
    for n in numels:
        offsets.append(off)
        off += (n + TILE - 1) // TILE * TILE
    return offsets, off


def manifest_order(sd, keys):
    """`keys` in the order of synth's manifests for the configuration the shapes spell out (a file read back from disk comes sorted by name, and
    the arenas' layout -- with it the order the norm is summed in -- must not depend on that); a dict that is not such a model keeps its order."""
    from . import synth, vae_backward
    try:
        enc = vae_backward.model_structure({k: sd[k] for k in keys if k.startswith("encoder.")}, "encoder.")
        dec = vae_backward.model_structure({k: sd[k] for k in keys if k.startswith("decoder.")}, "decoder.")
        block_out = tuple(b["resnets"][-1][1] for b in enc["blocks"])
        layers, latent = len(enc["blocks"][0]["resnets"]), enc["conv_out"][0] // 2
        manifest = {**synth.encoder_manifest(block_out, enc["conv_in"][1], latent, layers),
                    **synth.image_decoder_manifest(block_out, dec["conv_out"][0], latent, layers)}
    except (ValueError, KeyError, IndexError):
        return keys
    if set(manifest) != set(keys) or any(tuple(manifest[k]) != tuple(sd[k].shape) for k in keys):
        return keys
    return list(manifest)


def _ll_array(values):
    return (ctypes.c_longlong * len(values))(*values)


def save_optimizer_state(path, state):
    """optimizer_state_dict() -> one safetensors file (the step count as an int64 tensor)."""
    from safetensors.torch import save_file
    out = {"step": torch.tensor([int(state["step"])], dtype=torch.int64)}
    out.update({k: v.detach().cpu().contiguous() for k, v in state.items() if k != "step"})
    save_file(out, path)


def load_optimizer_state(path):
    from safetensors.torch import load_file
    raw = load_file(path)
    out = {"step": int(raw.pop("step")[0])}
    out.update(raw)
    return out


class VAETrainer:
    """The optimiser state of the whole VAE on one device and the train step on it.

    source: a state dict of `encoder.*` and `decoder.*` tensors (diffusers' names), or a loaded DiffusersVAEWrapper / AutoencoderKL.
    `params` holds one contiguous fp32 VIEW into the parameter arena per tensor, the encoder's in their order, then the decoder's: what
    forward_backward reads is what step writes.  Only grad_norm(), optimizer_state_sha256() and the memory check of a new batch shape
    talk to the host; everything else is queued on torch's current stream."""

    def __init__(self, source, *, weights, margin=1.0, similarity_type="cosine", seed=0, device=None):
        sd, device = self._source(source, device)
        keys = [k for k in sd if k.startswith("encoder.")] + [k for k in sd if k.startswith("decoder.")]
        if len(keys) != len(sd) or not any(k.startswith("encoder.") for k in keys) or not any(k.startswith("decoder.") for k in keys):
            raise ValueError("VAETrainer: the state dict holds the encoder.* and the decoder.* tensors and nothing else")
        keys = manifest_order(sd, keys)
        if similarity_type not in ("cosine", "euclidean"):
            raise ValueError(f"similarity_type {similarity_type!r}: cosine or euclidean expected")
        self.device = torch.device(device)
        self.weights = {k: float(weights.get(k, 0.0)) for k in ("reconstruction", "kl", "triplet")}
        self.margin, self.similarity_type, self.seed = float(margin), similarity_type, int(seed)
        self.shapes = {k: tuple(sd[k].shape) for k in keys}
        self.numels = [int(sd[k].numel()) for k in keys]
        self.offsets, self.total = optim_layout(self.numels)
        self._numel_arr = _ll_array(self.numels)
        self._arena = [self._aligned(self.total) for _ in range(3)]             # parameters, Adam m, Adam v: padding zero
        self.params, self.exp_avg, self.exp_avg_sq = ({k: a[o:o + n].view(self.shapes[k]) for k, o, n in zip(keys, self.offsets, self.numels)}
                                                      for a in self._arena)
        for k in keys:
            self.params[k].copy_(sd[k].detach().to(torch.float32))
        self._scalars = torch.zeros(2, dtype=torch.float64, device=self.device)      # TrainScalars: { fp64 norm^2, fp32 norm, fp32 coef }
        self._ws = None
        self._ctx = None
        self._clipped = False
        self._row = self._row_views = None                                       # the accumulation row (accumulate): absent until a trainer accumulates
        self._saved = {}                                                         # batch shape -> bytes kept between forward and backward
        self.t = 0

    @staticmethod
    def _source(source, device):
        vae = getattr(source, "vae", source)
        if hasattr(vae, "image_decoder") and hasattr(vae, "config"):
            if getattr(vae.config, "use_quant_conv", False) or getattr(vae.config, "use_post_quant_conv", False):
                raise ValueError("VAETrainer: use_quant_conv / use_post_quant_conv configurations have no backward here")
            sd = dict(vae.state_dict())
            sd.update(vae.image_decoder().state_dict())
            return sd, device if device is not None else next(vae.parameters()).device
        if not isinstance(source, dict):
            raise TypeError("VAETrainer: a state dict, a DiffusersVAEWrapper or an AutoencoderKL is expected")
        return source, device if device is not None else "cuda"

    def _aligned(self, floats):
        buf = torch.zeros(floats + 64, dtype=torch.float32, device=self.device)
        skip = (-buf.data_ptr() % 256) // 4
        return buf[skip:skip + floats]

    @property
    def ctx(self):
        """vae_backward's context of the device (made on first use: a trainer on the CPU can still hold, save and load state)."""
        if self._ctx is None:
            if self.device.type != "cuda":
                raise _lib.VTError("VAETrainer trains on a HIP device only: there is no CPU fallback")
            from . import vae_backward
            self._ctx = vae_backward.context(self.device)
            self._ctx.call("vt_op_backward_operands_check")                     # fp16 operands (flag 18) have no backward
        return self._ctx

    def arena_bytes(self):
        return 3 * 4 * self.total

    def check_memory(self, B, H, W):
        """Refuse a batch shape whose saved activations do not fit beside the arenas, before anything of the step is allocated.  The
        accumulation row (4 * total bytes) is counted by being there: once allocated it is outside `free`, FullTrainer.micro_step allocates
        it before a shape's first check, and accumulation_row() makes its own check where a caller allocates it later."""
        from . import vae_backward
        need = vae_backward.vae_train_saved_bytes(self.shapes, B, H, W)
        free = torch.cuda.mem_get_info(self.device)[0] + torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device)
        if need > free:
            raise MemoryError(f"VAETrainer: a [{B}, 3, {H}, {W}] batch keeps {need} bytes between forward and backward beside "
                              f"{self.arena_bytes() + self.row_bytes()} bytes of parameter and moment arenas"
                              f"{' and the accumulation row' if self.row_bytes() else ''}; the device has {free} bytes free")
        return need

    def saved_bytes(self, shape):
        """Bytes a batch of this shape keeps between forward and backward (known once forward_backward has seen the shape)."""
        return self._saved[tuple(shape)]

    # -- the step ---------------------------------------------------------------------------------------------------------------------------
    def forward_backward(self, anchor, positive, negative, labels_a=None, labels_p=None, first_image=0):
        """vae_backward.vae_loss_and_grads with the trainer's live parameters, weights, margin, similarity and seed -> (losses, grads)."""
        from . import vae_backward
        self.ctx
        shape = tuple(anchor.shape)
        if shape not in self._saved:
            self._saved[shape] = self.check_memory(shape[0], shape[2], shape[3])
        return vae_backward.vae_loss_and_grads(self.params, anchor, positive, negative, labels_a, labels_p, weights=self.weights, margin=self.margin,
                                               similarity_type=self.similarity_type, seed=self.seed, first_image=int(first_image))

    def _grad_pointers(self, grads):
        if list(grads.keys()) != list(self.params.keys()):
            raise ValueError("the gradients are keyed and ordered like params")
        ptrs = (ctypes.c_void_p * len(self.numels))()
        for i, (k, g) in enumerate(grads.items()):
            if g.dtype != torch.float32 or g.device != self.device or not g.is_contiguous() or tuple(g.shape) != self.shapes[k]:
                raise ValueError(f"{k}: a contiguous fp32 gradient of shape {self.shapes[k]} on {self.device} is expected")
            ptrs[i] = g.data_ptr()
        return ptrs

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def clip(self, grads, max_norm, chunk=0):
        """clip_grad_norm_(max_norm) over all gradients: the norm and the coefficient go to the trainer's scalars (grad_norm reads them); the
        gradients are not written -- the step that follows multiplies by the coefficient as it reads them."""
        ctx, ptrs = self.ctx, self._grad_pointers(grads)
        if self._ws is None:
            need = ctx.lib.vt_vae_optim_workspace_bytes(self._numel_arr, len(self.numels))
            self._ws = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
            self._ws_ptr, self._ws_bytes = (self._ws.data_ptr() + 255) // 256 * 256, need
        ctx.call("vt_vae_optim_norm", ptrs, self._numel_arr, len(self.numels), float(max_norm), ctypes.c_void_p(self._scalars.data_ptr()),
                 ctypes.c_void_p(self._ws_ptr), self._ws_bytes, int(chunk), self._stream())
        self._clipped = True

    def step(self, grads, lr, weight_decay=0.0, betas=ADAM_BETAS, eps=ADAM_EPS, chunk=0):
        """AdamW's next update of every tensor from `grads`; after a clip() of the same gradients, scaled by its coefficient in the same pass."""
        ctx, ptrs = self.ctx, self._grad_pointers(grads)
        scalars = ctypes.c_void_p(self._scalars.data_ptr()) if self._clipped else None
        ctx.call("vt_vae_optim_step", *(ctypes.c_void_p(a.data_ptr()) for a in self._arena), self.total, ptrs, self._numel_arr, len(self.numels),
                 scalars, float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), self.t + 1, int(chunk), self._stream())
        self.t += 1
        self._clipped = False

    def train_step(self, anchor, positive, negative, labels_a=None, labels_p=None, first_image=0, *, lr, weight_decay=0.0, max_grad_norm=1.0,
                   betas=ADAM_BETAS, eps=ADAM_EPS):
        """forward_backward, clip (only when max_grad_norm > 0, as the reference) and step -> losses (0-d float64 device tensors)."""
        losses, grads = self.forward_backward(anchor, positive, negative, labels_a, labels_p, first_image)
        if max_grad_norm > 0:
            self.clip(grads, max_grad_norm)
        self.step(grads, lr, weight_decay, betas, eps)
        return losses

    # -- the gradient exchange of a sharded run (VAEGradientExchange below) ---------------------------------------------------------------
    def export_gradients(self, grads, row, chunk=0):
        """The gradients packed into `row` (fp32, 256-B aligned, a multiple of TILE floats that is at least `total`) in the arenas' layout:
        every float of the row is written (vt_vae_grads_export)."""
        self.ctx.call("vt_vae_grads_export", self._grad_pointers(grads), self._numel_arr, len(self.numels), ctypes.c_void_p(row.data_ptr()),
                      row.numel(), int(chunk), self._stream())

    def merge_gradients(self, rows, row_stride, weights, first_float, floats, out):
        """out[e] = (float)(w[0] x_0 + ... + w[K-1] x_{K-1}) over e in [0, floats), x_r = rows[r * row_stride + first_float + e], in fp64 and in
        rank order (vt_vae_grads_merge; merge_rows_host states the arithmetic)."""
        w = [float(x) for x in weights]
        self.ctx.call("vt_vae_grads_merge", ctypes.c_void_p(rows.data_ptr()), int(row_stride), len(w), (ctypes.c_double * max(1, len(w)))(*w),
                      int(first_float), int(floats), ctypes.c_void_p(out.data_ptr()), self._stream())

    # -- gradient accumulation (train_full's micro-steps; accumulate_rows_host states the arithmetic) ---------------------------------------
    def accumulate(self, grads, *, scale, first, n=None, chunk=0):
        """The gradients of one micro-step, times `scale`, into the trainer's accumulation row (vt_vae_grads_accumulate): first=True starts
        the sum (every float of the row is written), first=False adds to it -- after the coefficient of a clip() since the last accumulate
        has been applied to the row, here and nowhere else.  `grads` is keyed and ordered like the first n of params (None: all)."""
        n = len(self.numels) if n is None else int(n)
        keys = list(self.params)[:n]
        if n < 1 or list(grads.keys()) != keys:
            raise ValueError("the gradients are keyed and ordered like the first n of params")
        ptrs = (ctypes.c_void_p * n)()
        for i, (k, g) in enumerate(grads.items()):
            if g.dtype != torch.float32 or g.device != self.device or not g.is_contiguous() or tuple(g.shape) != self.shapes[k]:
                raise ValueError(f"{k}: a contiguous fp32 gradient of shape {self.shapes[k]} on {self.device} is expected")
            ptrs[i] = g.data_ptr()
        row = self.accumulation_row()
        scalars = ctypes.c_void_p(self._scalars.data_ptr()) if self._clipped and not first else None
        self.ctx.call("vt_vae_grads_accumulate", ptrs, _ll_array(self.numels[:n]), n, ctypes.c_void_p(row.data_ptr()), row.numel(), float(scale),
                      scalars, int(bool(first)), int(chunk), self._stream())
        self._clipped = False

    def accumulation_row(self):
        """The fp32 row of the arenas' layout that holds the sum across micro-steps (allocated on first use: 4 * total bytes)."""
        if self._row is None:
            if self.device.type == "cuda":
                free = torch.cuda.mem_get_info(self.device)[0] + torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device)
                if 4 * self.total > free:
                    raise MemoryError(f"VAETrainer: the accumulation row takes {4 * self.total} bytes beside {self.arena_bytes()} bytes of parameter "
                                      f"and moment arenas; the device has {free} bytes free")
            self._row = self._aligned(self.total)
            self._row_views = self.gradient_views(self._row)
        return self._row

    def accumulated(self, n=None):
        """{key: view into the accumulation row} of the first n tensors (None: all): what clip and step take."""
        self.accumulation_row()
        views = self._row_views
        return views if n is None or n == len(views) else {k: views[k] for k in list(views)[:int(n)]}

    def row_bytes(self):
        return 0 if self._row is None else 4 * self.total

    def gradient_views(self, row):
        """{key: view of `row` at the tensor's slot}, keyed and ordered like params: what clip and step take after a merge."""
        return {k: row[o:o + n].view(self.shapes[k]) for k, o, n in zip(self.params, self.offsets, self.numels)}

    def grad_norm(self):
        """(total L2 norm, clip coefficient) of the last clip(): the one method of the step that synchronises."""
        raw = self._scalars.cpu().numpy().view(np.uint8)
        return float(raw[8:12].view(np.float32)[0]), float(raw[12:16].view(np.float32)[0])

    # -- state ------------------------------------------------------------------------------------------------------------------------------
    def state_dict(self):
        return {k: v.detach().clone() for k, v in self.params.items()}

    def load_state_dict(self, state):
        if set(state.keys()) != set(self.params.keys()):
            raise ValueError("load_state_dict: the trainer's own keys are expected")
        for k, v in self.params.items():
            v.copy_(state[k].to(torch.float32).reshape(v.shape))

    def optimizer_state_dict(self):
        out = {"step": self.t}
        out.update({"exp_avg." + k: v.detach().clone() for k, v in self.exp_avg.items()})
        out.update({"exp_avg_sq." + k: v.detach().clone() for k, v in self.exp_avg_sq.items()})
        return out

    def load_optimizer_state_dict(self, state):
        want = {"step"} | {"exp_avg." + k for k in self.params} | {"exp_avg_sq." + k for k in self.params}
        if set(state.keys()) != want:
            raise ValueError("load_optimizer_state_dict: step, exp_avg.* and exp_avg_sq.* of the trainer's own keys are expected")
        if int(state["step"]) < 0:
            raise ValueError("load_optimizer_state_dict: a negative step")
        for prefix, views in (("exp_avg.", self.exp_avg), ("exp_avg_sq.", self.exp_avg_sq)):
            for k, v in views.items():
                v.copy_(state[prefix + k].to(torch.float32).reshape(v.shape))
        self.t = int(state["step"])

    def optimizer_state_sha256(self, h=None):
        """SHA-256 over the parameters, Adam m and Adam v of every tensor, in the order of `params` (as the block trainers')."""
        h = hashlib.sha256() if h is None else h
        for views in (self.params, self.exp_avg, self.exp_avg_sq):
            for v in views.values():
                h.update(v.detach().cpu().numpy().tobytes())
        return h

    def commit(self, vae_model):
        """The trained tensors into a loaded model (DiffusersVAEWrapper or AutoencoderKL): both loads trigger the lazy re-upload."""
        vae = getattr(vae_model, "vae", vae_model)
        vae.load_state_dict({k: v for k, v in self.params.items() if k.startswith("encoder.")})
        vae.load_decoder_state_dict({k: v for k, v in self.params.items() if k.startswith("decoder.")}, strict=True)


# ---- sharded training: the batch's shards, the owners' ranges, the gradient exchange ------------------------------------------------------
MAX_RANKS = 64                                           # VT_MERGE_MAX_RANKS


def shard_of_batch(idx, rank, world, per_rank_batch):
    """Rank `rank`'s contiguous slice of a global batch of at most world * per_rank_batch positions (empty when the batch ends before it)."""
    if not 0 <= rank < world or per_rank_batch < 1:
        raise ValueError("shard_of_batch: 0 <= rank < world and a per-rank batch of at least 1 expected")
    return idx[rank * per_rank_batch:(rank + 1) * per_rank_batch]


def shard_weights(n_global, world, per_rank_batch):
    """w[r] = n_r / sum n over the ranks' slices of a global batch of n_global images: the merged gradient of per-rank batch-mean gradients is
    then the concatenated batch's mean gradient.  Known on every rank from the plan alone: no count is exchanged."""
    counts = [len(shard_of_batch(range(int(n_global)), r, world, per_rank_batch)) for r in range(world)]
    if n_global < 1 or sum(counts) != n_global:
        raise ValueError(f"a global batch of {n_global} images does not fit {world} ranks of {per_rank_batch}")
    return [c / n_global for c in counts]


def owner_split(total_floats, world):
    """(S, row_floats): rank r owns tiles [r S, (r + 1) S) of the gradient row, S = ceil(T / world) for the layout's T = total / TILE tiles, and
    the row is padded to world * S tiles so that every rank's range has the same size."""
    if total_floats < TILE or total_floats % TILE or not 1 <= world <= MAX_RANKS:
        raise ValueError(f"owner_split: a layout total (a multiple of {TILE}) and 1 to {MAX_RANKS} ranks expected")
    S = (total_floats // TILE + world - 1) // world
    return S, world * S * TILE


def merge_rows_host(rows, weights):
    """What vt_vae_grads_merge computes, in numpy: K fp32 arrays and K weights -> fp32, out[e] = (float)acc with acc = w[0] * (double)x_0, then
    acc = acc + w[r] * (double)x_r for r = 1 .. K-1 in that order -- train.merge_gradients_host with the first term taken as w[0] x_0 and not
    added to 0.0, so K = 1 at weight 1 returns its input bit for bit (-0.0 included)."""
    rows = [np.asarray(b, dtype=np.float32).reshape(-1) for b in rows]
    w = [np.float64(x) for x in weights]
    if len(rows) != len(w) or not rows:
        raise ValueError("merge_rows_host: one weight per row, at least one row")
    acc = w[0] * rows[0].astype(np.float64)              # (numpy rounds each ufunc's result: nothing is fused)
    for r in range(1, len(rows)):
        acc = acc + w[r] * rows[r].astype(np.float64)
    return acc.astype(np.float32)


def accumulate_rows_host(row, grads, offsets, numels, scale, coef, first):
    """What vt_vae_grads_accumulate computes, in numpy fp32 -> the new row (the one given is not changed).  Per element g of tensor i at
    offsets[i]: t = scale * g; first: row = t, zero everywhere else; otherwise a = row, a = coef * a when coef (None: no scalars) is < 1 -- a NaN
    or >= 1 coef multiplies nothing -- and row = a + t.  Two products and one add, each rounded to fp32 on its own (numpy rounds each ufunc's
    result: nothing is fused); what lies outside the tensors' elements keeps its bytes."""
    row = np.asarray(row, dtype=np.float32).reshape(-1)
    out = np.zeros_like(row) if first else row.copy()
    s = np.float32(scale)
    c = None if coef is None else np.float32(coef)
    clipped = c is not None and bool(c < np.float32(1.0))
    for g, o, n in zip(grads, offsets, numels):
        g = np.asarray(g, dtype=np.float32).reshape(-1)
        if g.size != n:
            raise ValueError("accumulate_rows_host: a gradient's size is not its numel")
        t = g if s == np.float32(1.0) else g * s
        if first:
            out[o:o + n] = t
        else:
            a = out[o:o + n]
            if clipped:
                a = a * c
            out[o:o + n] = a + t
    return out


class _DeviceTransport:
    """RCCL: the ranks' slices cross in ONE all_to_all_single with equal splits, the merged slices in ONE all_gather_into_tensor."""

    def __init__(self, ex, group):
        self.ex, self.group, self.in_place = ex, group, True
        self._recv = torch.empty(ex.world * ex.slice_floats, dtype=torch.float32, device=ex.device)
        self.bytes_sent = self.bytes_received = 2 * (ex.world - 1) * 4 * ex.slice_floats

    def scatter(self, mine):
        """-> (rows, row stride, first float) of the K ranks' copies of this rank's range: rank q's slice r goes to rank r"""
        import torch.distributed as dist
        dist.all_to_all_single(self._recv, mine, group=self.group)
        return self._recv, self.ex.slice_floats, 0

    def gather(self, merged):
        """every rank's merged range into every rank's merged row; in place when torch takes a slice of the output as the input"""
        import torch.distributed as dist
        own = merged[self.ex.first_float:self.ex.first_float + self.ex.slice_floats]
        if self.in_place:
            try:
                dist.all_gather_into_tensor(merged, own, group=self.group)
                return
            except (RuntimeError, ValueError):          # (refused at the argument check, before anything is sent)
                self.in_place = False
        dist.all_gather_into_tensor(merged, own.clone(), group=self.group)


class _HostTransport:
    """gloo, the rehearsal on shared GPUs only (as train.GradientExchange): whole rows and merged slices through the CPU with all_gather.
    The kernels and the merged bytes are the device transport's; the traffic is not."""

    def __init__(self, ex, group):
        self.ex, self.group = ex, group
        self._all = torch.empty(ex.world * ex.row_floats, dtype=torch.float32, device=ex.device)
        self.bytes_sent = self.bytes_received = (ex.world - 1) * 4 * (ex.row_floats + ex.slice_floats)

    def scatter(self, mine):
        import torch.distributed as dist
        parts = [torch.empty(self.ex.row_floats, dtype=torch.float32) for _ in range(self.ex.world)]
        dist.all_gather(parts, mine.cpu(), group=self.group)
        self._all.copy_(torch.cat(parts))
        return self._all, self.ex.row_floats, self.ex.first_float

    def gather(self, merged):
        import torch.distributed as dist
        own = merged[self.ex.first_float:self.ex.first_float + self.ex.slice_floats]
        parts = [torch.empty(self.ex.slice_floats, dtype=torch.float32) for _ in range(self.ex.world)]
        dist.all_gather(parts, own.cpu(), group=self.group)
        merged.copy_(torch.cat(parts))


class InProcessRanks:
    """The transport of K emulated ranks inside ONE process, without a process group (the device tests): the K exchanges are driven in
    lockstep -- every rank's export(), then every rank's merge(), then every rank's gather() -- and a rank reads the others' rows directly."""

    def __init__(self, world):
        self.world, self.exchanges = int(world), [None] * int(world)

    def scatter(self, ex, mine):
        lo, n = ex.first_float, ex.slice_floats
        return torch.cat([other.row[lo:lo + n] for other in self.exchanges]), n, 0

    def gather(self, ex, merged):
        n = ex.slice_floats
        for q, other in enumerate(self.exchanges):
            if other is not ex:
                merged[q * n:(q + 1) * n].copy_(other.merged[q * n:(q + 1) * n])


class _InProcessEndpoint:
    def __init__(self, ranks, ex):
        self.ranks, self.ex = ranks, ex
        ranks.exchanges[ex.rank] = ex
        self.bytes_sent = self.bytes_received = 2 * (ex.world - 1) * 4 * ex.slice_floats

    def scatter(self, mine):
        return self.ranks.scatter(self.ex, mine)

    def gather(self, merged):
        self.ranks.gather(self.ex, merged)


class VAEGradientExchange:
    """The cross-rank operation of a sharded train_vae step.  The gradient is 244 fresh tensors (84 M floats for FLUX), so no rank gathers
    every row: each rank exports its gradients into one row of the arenas' layout (padded to K S tiles), the ranks' slices cross so that rank r
    holds every rank's copy of ITS tiles [r S, (r + 1) S), it merges those K slices in rank order (fp64, weights from the plan), and the merged
    slices are gathered into every rank's merged row.  Per rank and step 2 (K - 1) / K of the row is sent and as much received -- a ring
    all-reduce's traffic (a formula: no multi-GPU scaling figure has been measured) -- with the summation order fixed by the rank count,
    the same bytes on every rank, no atomics, no all-reduce, no parameter broadcast and no host synchronisation.

    exchange(grads, weights) -> {key: view into the merged row}, keyed and ordered like trainer.params: what clip() and step() take.
    Without a group, or on a one-rank group without force_collective, it returns the gradients it was given and launches nothing.
    emulated = (InProcessRanks, rank): one of K ranks emulated inside one process (export / merge / gather are then driven in lockstep)."""

    def __init__(self, trainer, group=None, force_collective=False, *, emulated=None):
        import torch.distributed as dist
        self.trainer, self.group, self.device = trainer, group, trainer.device
        grouped = emulated is None and group is not None and dist.is_available() and dist.is_initialized()
        self.world, self.rank, self.backend = 1, 0, None
        if grouped:
            self.world, self.rank, self.backend = dist.get_world_size(group), dist.get_rank(group), dist.get_backend(group)
        elif emulated is not None:
            self.world, self.rank, self.backend = emulated[0].world, int(emulated[1]), "in-process"
        if self.world > MAX_RANKS:
            raise ValueError(f"{self.world} ranks: the gradient merge takes at most {MAX_RANKS}")
        self.active = emulated is not None or (grouped and (self.world > 1 or bool(force_collective)))
        self.calls, self.transport = 0, None
        if not self.active:
            return
        self.slice_tiles, self.row_floats = owner_split(trainer.total, self.world)
        self.slice_floats = self.slice_tiles * TILE
        self.first_float = self.rank * self.slice_floats
        self.row, self.merged = trainer._aligned(self.row_floats), trainer._aligned(self.row_floats)
        self.views = trainer.gradient_views(self.merged)
        if emulated is not None:
            self.transport = _InProcessEndpoint(emulated[0], self)
        else:
            self.transport = (_HostTransport if self.backend == "gloo" else _DeviceTransport)(self, group)

    @property
    def bytes_sent_per_step(self):
        return self.transport.bytes_sent if self.active else 0

    @property
    def bytes_received_per_step(self):
        return self.transport.bytes_received if self.active else 0

    def export(self, grads):
        """this rank's gradients into its row; None (the rank's slice of the batch is empty: no forward, no backward) is a row of zeros"""
        if grads is None:
            self.row.zero_()
        else:
            self.trainer.export_gradients(grads, self.row)

    def merge(self, weights):
        if len(weights) != self.world:
            raise ValueError(f"{len(weights)} weights for {self.world} ranks")
        rows, stride, first = self.transport.scatter(self.row)
        self.trainer.merge_gradients(rows, stride, weights, first, self.slice_floats,
                                     self.merged[self.first_float:self.first_float + self.slice_floats])

    def gather(self):
        self.transport.gather(self.merged)
        self.calls += 1
        return self.views

    def exchange(self, grads, weights):
        if not self.active:
            return grads
        self.export(grads)
        self.merge(weights)
        return self.gather()


# ---- the CLI --------------------------------------------------------------------------------------------------------------------------
def build_parser():
    p = argparse.ArgumentParser(description="VAE 训练 (重建 + KL + 三元组损失), 前向、反向与优化器都在GPU上。")
    p.add_argument("--vae_checkpoint", type=str, default=None, help="预训练VAE模型文件路径 (.safetensors)")
    p.add_argument("--vae_config_path", type=str, default=None, help="VAE配置文件路径 (JSON格式)")
    p.add_argument("--json_path", type=str, required=True)
    p.add_argument("--tags_csv_path", type=str, required=True)
    p.add_argument("--output_dir", type=str, default="vae_output")
    p.add_argument("--resolution", type=int, default=1024)
    p.add_argument("--train_batch_size", type=int, default=1)
    p.add_argument("--num_epochs", type=int, default=10)
    p.add_argument("--learning_rate", type=float, default=1e-4)
    p.add_argument("--weight_decay", type=float, default=1e-6)
    p.add_argument("--use_simplified_vae_loss", action="store_true", default=True, help="使用简化的VAE损失（重建+三元组）")
    p.add_argument("--reconstruction_weight", type=float, default=0.01)
    p.add_argument("--kl_weight", type=float, default=1e-2, help="KL散度损失权重（log变换后）")
    p.add_argument("--triplet_weight", type=float, default=1.0)
    p.add_argument("--triplet_margin", type=float, default=1.0)
    p.add_argument("--similarity_type", type=str, default="cosine", choices=["cosine", "euclidean"], help="三元组损失的相似性度量")
    p.add_argument("--lr_scheduler_type", type=str, default="cosine", help="学习率调度器类型")
    p.add_argument("--lr_warmup_steps", type=int, default=500, help="学习率预热步数")
    p.add_argument("--max_grad_norm", type=float, default=1.0, help="梯度裁剪阈值")
    p.add_argument("--logging_steps", type=int, default=100, help="日志记录间隔")
    p.add_argument("--save_steps", type=int, default=5, help="模型保存间隔（epochs）")
    p.add_argument("--mixed_precision", type=str, default="fp16")
    p.add_argument("--enable_xformers_memory_efficient_attention", action="store_true", help="启用 xformers 加速")
    p.add_argument("--use_bucketing", action="store_true", help="启用长宽比分桶功能")
    p.add_argument("--base_resolution", type=int, default=512, help="分桶的基础分辨率")
    p.add_argument("--max_resolution", type=int, default=1024, help="分桶的最大分辨率")
    p.add_argument("--bucket_step", type=int, default=64, help="分桶的步长")
    p.add_argument("--num_workers", type=int, default=4, help="DataLoader 工作线程数")
    p.add_argument("--prefetch_factor", type=int, default=2, help="DataLoader 预取倍数（每个worker）")
    p.add_argument("--seed", type=int, default=42, help="随机种子")
    p.add_argument("--cudnn_benchmark", action="store_true", help="启用cudnn benchmark以提高卷积性能（输入尺寸固定时建议开启）")
    p.add_argument("--cudnn_deterministic", action="store_true", help="启用确定性cuDNN以提高复现性（可能降低性能）")
    # this project's own
    p.add_argument("--full_vae_loss", action="store_true", help="the KL term enters the total (the reference's flag above cannot be switched off)")
    p.add_argument("--resume_from", type=str, default=None, help="continue from a best_checkpoint/ or checkpoint-{e}/ directory")
    p.add_argument("--stop_after_epochs", type=int, default=0, help="end the run after this many epochs of --num_epochs (0: all); the schedule is --num_epochs'")
    p.add_argument("--workers", type=int, default=0, help="image decode threads (0 = min(16, cores))")
    p.add_argument("--sharded", action="store_true", help="data-parallel run under torchrun, one rank per GPU: --train_batch_size is per rank")
    return p


def ignored_arguments(args):
    """The reference's flags that mean nothing here and were set to something."""
    defaults = build_parser().parse_args(["--json_path", "", "--tags_csv_path", ""])
    return [k for k in IGNORED_ARGUMENTS if getattr(args, k, None) != getattr(defaults, k)]


def check_sharded(args, environ=None):
    """--sharded is refused, by a message that names it, before any device work: without a process group to join (torchrun's WORLD_SIZE > 1, or
    the one-rank rehearsal VT_CLI_ONE_RANK_GROUP=1) and above the merge's 64 ranks."""
    if not getattr(args, "sharded", False):
        return
    env = os.environ if environ is None else environ
    world = int(env.get("WORLD_SIZE", "1"))
    if world > MAX_RANKS:
        raise SystemExit(f"--sharded: {world} ranks, the gradient merge takes at most {MAX_RANKS}")
    if world <= 1 and env.get("VT_CLI_ONE_RANK_GROUP") != "1":
        raise SystemExit("--sharded needs a process group: start the run under torchrun with one rank per GPU "
                         "(VT_CLI_ONE_RANK_GROUP=1 rehearses the exchange on one rank)")


def plan_train_batches(order, batch_size, buckets=None):
    """[(bucket or None, [positions])] of one epoch: `order` cut into batches; with buckets a batch has one bucket -- positions join their
    bucket's open batch in epoch order, a full batch is emitted at once, the rest at the end in bucket order -- so the number of batches,
    sum over buckets of ceil(count / batch_size), is the same every epoch."""
    if buckets is None:
        return [(None, order[i:i + batch_size]) for i in range(0, len(order), batch_size)]
    out, pending = [], {}
    for i in order:
        cur = pending.setdefault(buckets[i], [])
        cur.append(i)
        if len(cur) == batch_size:
            out.append((buckets[i], cur))
            pending[buckets[i]] = []
    out.extend((b, cur) for b, cur in sorted(pending.items()) if cur)
    return out


def steps_per_epoch(n_train, batch_size, buckets=None):
    if buckets is None:
        return (n_train + batch_size - 1) // batch_size
    counts = {}
    for b in buckets:
        counts[b] = counts.get(b, 0) + 1
    return sum((c + batch_size - 1) // batch_size for c in counts.values())


def _write_json(path, obj):
    with open(path, "w", encoding="utf-8") as fh:
        json.dump(obj, fh, indent=2, ensure_ascii=False, sort_keys=True)


def save_model(path, trainer, config):
    """config.json + diffusion_pytorch_model.safetensors: what load_diffusers_vae_from_pretrained and --vae_checkpoint read."""
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    _write_json(os.path.join(path, "config.json"), config)
    save_file({k: v.cpu().contiguous() for k, v in trainer.state_dict().items()}, os.path.join(path, MODEL_FILE))


def save_checkpoint(path, trainer, config, state):
    save_model(path, trainer, config)
    save_optimizer_state(os.path.join(path, OPTIMIZER_FILE), trainer.optimizer_state_dict())
    _write_json(os.path.join(path, STATE_FILE), state)


def model_config(vae):
    cfg = {"_class_name": "AutoencoderKL"}
    cfg.update(vars(vae.config))
    return cfg


def train(args):
    """The run; with --sharded, this rank's part of it: the process group is joined BEFORE any GPU call of this process, and every rank but
    rank 0 runs silently (rank 0 alone prints, validates and writes files)."""
    check_sharded(args)
    if not getattr(args, "sharded", False):
        return _train(args, None)
    import contextlib
    import torch.distributed as dist
    from .infer_full import _dist_setup
    world, rank, dev_index = _dist_setup()
    torch.cuda.set_device(dev_index)
    shard = SimpleNamespace(world=world, rank=rank, group=dist.group.WORLD, dist=dist)
    if rank == 0:
        return _train(args, shard)
    with open(os.devnull, "w") as null, contextlib.redirect_stdout(null):
        return _train(args, shard)


def _train(args, shard):
    from concurrent.futures import ThreadPoolExecutor
    from safetensors.torch import load_file
    from . import evaluate_vae
    from .evaluate import TaggedImageList
    from .infer_vae import _EncoderInput
    from .modules import AspectRatioBucketing
    from .vae_reconstruction_test import load_vae_model
    if not torch.cuda.is_available():
        raise RuntimeError("vae_tagger_amd needs an MI355X (no HIP device visible; there is no CPU fallback)")
    if args.lr_scheduler_type not in SCHEDULES:
        raise SystemExit(f"--lr_scheduler_type {args.lr_scheduler_type}: one of {', '.join(SCHEDULES)}")
    if args.train_batch_size < 1 or args.num_epochs < 1 or args.save_steps < 1 or args.logging_steps < 1:
        raise SystemExit("--train_batch_size, --num_epochs, --save_steps and --logging_steps are at least 1")
    ignored = ignored_arguments(args)
    if ignored:
        print("ignored arguments (they mean nothing on this device): " + ", ".join("--" + k for k in ignored))
    sharded = shard is not None
    world, rank = (shard.world, shard.rank) if sharded else (1, 0)
    chief, B = rank == 0, args.train_batch_size                                # --sharded: B is per rank, a global batch is B * world
    if chief:
        os.makedirs(args.output_dir, exist_ok=True)
    device = torch.device("cuda", torch.cuda.current_device())
    simplified = bool(args.use_simplified_vae_loss) and not args.full_vae_loss
    args.use_simplified_vae_loss = simplified                                  # (the validation pass reads it)

    data = TaggedImageList(args.json_path, args.tags_csv_path)
    for p in data.missing:
        print(f"跳过图像 {p}，错误原因: 文件不存在")
    paths = data.image_paths
    train_idx, val_idx = split_indices(len(paths), args.seed)
    print(f"训练集大小: {len(train_idx)}, 验证集大小: {len(val_idx)}")
    train_paths, val_paths = [paths[i] for i in train_idx], [paths[i] for i in val_idx]
    train_labels = np.stack([data.labels[p] for p in train_paths]).astype(np.float32)
    val_labels = np.stack([data.labels[p] for p in val_paths]).astype(np.float32)
    train_buckets = val_buckets = None
    if args.use_bucketing:
        bucketing = AspectRatioBucketing(args.base_resolution, args.max_resolution, args.bucket_step)
        train_buckets, val_buckets = [bucketing.assign_bucket(p) for p in train_paths], [bucketing.assign_bucket(p) for p in val_paths]
        print(f"启用分桶模式：基础分辨率{args.base_resolution}, 最大分辨率{args.max_resolution}")
    else:
        print(f"传统模式：固定分辨率{args.resolution}x{args.resolution}")
    val_data = SimpleNamespace(image_paths=val_paths)
    val_triplets = evaluate_vae.triplet_lists(val_labels, args.seed)
    val_batches = evaluate_vae.plan_batches(val_paths, args.train_batch_size, val_buckets)

    model = load_vae_model(args, device)
    model.check_finite = False
    weights = evaluate_vae.loss_weights(args)
    if simplified:
        weights["kl"] = 0.0
    trainer = VAETrainer(model, weights=weights, margin=args.triplet_margin, similarity_type=args.similarity_type, seed=args.seed)
    config = model_config(model.vae)
    exchange = VAEGradientExchange(trainer, shard.group, force_collective=True) if sharded else None

    def gather_objects(obj):
        out = [None] * world
        shard.dist.all_gather_object(out, obj, group=shard.group)
        return out

    def agreed_digest(what):
        """every rank's optimizer_state_sha256, in rank order; the run fails where they differ (nothing is broadcast to repair it)"""
        digests = gather_objects(trainer.optimizer_state_sha256().hexdigest())
        if len(set(digests)) != 1:
            raise RuntimeError(f"--sharded: the ranks' states differ {what}: {digests}")
        return digests

    spe = steps_per_epoch(len(train_idx), B * world, train_buckets)
    total_steps = args.num_epochs * spe
    run = {"step": 0, "epoch": 0, "images": 0, "best_val_loss": None, "history": {"train_loss": [], "val_loss": [], "learning_rates": []}}
    if args.resume_from:
        trainer.load_state_dict(load_file(os.path.join(args.resume_from, MODEL_FILE)))
        trainer.load_optimizer_state_dict(load_optimizer_state(os.path.join(args.resume_from, OPTIMIZER_FILE)))
        with open(os.path.join(args.resume_from, STATE_FILE), "r", encoding="utf-8") as fh:
            run = json.load(fh)
        if run["step"] != trainer.t or run["step"] != run["epoch"] * spe:
            raise SystemExit(f"{args.resume_from}: step {run['step']} does not match {run['epoch']} epochs of {spe} steps: other data or batch size")
        print(f"resumed from {args.resume_from}: epoch {run['epoch']}, step {run['step']}, {run['images']} images consumed")
    history = run["history"]
    best = math.inf if run["best_val_loss"] is None else float(run["best_val_loss"])
    report_path = os.path.join(args.output_dir, "train_report.json")
    report = {"epochs": [], "clip": args.max_grad_norm > 0, "max_grad_norm": args.max_grad_norm, "ignored_arguments": ignored,
              "steps_per_epoch": spe, "total_steps": total_steps, "simplified": simplified, "arena_bytes": trainer.arena_bytes()}
    if sharded:
        report["sharded"] = {"world": world, "backend": exchange.backend, "per_rank_batch": B, "bytes_sent_per_step": exchange.bytes_sent_per_step,
                             "bytes_received_per_step": exchange.bytes_received_per_step, "exchange_calls": 0,
                             "state_sha256": agreed_digest("before the first step")}
    if args.resume_from and os.path.exists(report_path):
        with open(report_path, "r", encoding="utf-8") as fh:
            report["epochs"] = json.load(fh).get("epochs", [])[:run["epoch"]]
    inputs = _EncoderInput(model)
    label_t = torch.from_numpy(train_labels).to(device)
    load = lambda pool, indices, bucket: evaluate_vae._load_batch(pool, train_paths, indices, args.resolution, bucket,
                                                                  lambda u8: inputs.normalize_u8(u8.to(device, non_blocking=True)))
    last_epoch = args.num_epochs if args.stop_after_epochs <= 0 else min(args.num_epochs, run["epoch"] + args.stop_after_epochs)
    step, images = run["step"], run["images"]

    def read_back(loss_sum, losses, what):
        """the one place the host waits for the device inside an epoch: the running sum, the last step's terms, the health word.  --sharded: a
        rank's running sum is of w_r L_r; the K sums are gathered and added in rank order on the host (the terms shown are this rank's own,
        zeros on a rank that has had no image yet), and every rank raises where any rank's numbers are bad."""
        terms = [losses[k] for k in ("total", "reconstruction", "kl", "triplet")] if losses is not None else [torch.zeros_like(loss_sum)] * 4
        values = torch.stack([loss_sum] + terms).cpu().tolist()
        st = trainer.ctx.status()
        if sharded:
            every = gather_objects((values[0], st, all(math.isfinite(v) for v in values)))
            values[0] = every[0][0]
            for other in every[1:]:
                values[0] = values[0] + other[0]
            bad = [(r, e) for r, e in enumerate(every) if e[1] or not e[2]]
            if bad:
                raise FloatingPointError(f"{what}: (rank, (running sum, device health word, finite)) {bad}")
        if st or not all(math.isfinite(v) for v in values):
            raise FloatingPointError(f"{what}: loss terms {values[1:]}, running sum {values[0]}, device health word {st}")
        return values

    with ThreadPoolExecutor(max_workers=max(1, args.workers or min(16, os.cpu_count() or 1))) as pool:
        for epoch in range(run["epoch"], last_epoch):
            t0 = time.perf_counter()
            order = epoch_order(len(train_idx), args.seed, epoch)
            triplets = {i: evaluate_vae.sample_triplet(args.seed * TRIPLET_SEED_STRIDE + epoch + 1, i, train_labels) for i in order}
            loss_sum = torch.zeros((), dtype=torch.float64, device=device)
            lrs, saved_bytes, epoch_images, losses = [], 0, 0, None
            for k, (bucket, batch) in enumerate(plan_train_batches(order, B * world, train_buckets)):
                idx = shard_of_batch(batch, rank, world, B) if sharded else batch      # this rank's contiguous slice of the global batch
                if idx:
                    xa = load(pool, idx, bucket)
                    xp = load(pool, [triplets[i][0] for i in idx], bucket)
                    xn = load(pool, [triplets[i][1] for i in idx], bucket)
                    ia = torch.as_tensor(idx, device=device)
                    ip = torch.as_tensor([triplets[i][0] for i in idx], device=device)
                lr = args.learning_rate * lr_schedule(args.lr_scheduler_type, step, args.lr_warmup_steps, total_steps)
                if not sharded:
                    losses = trainer.train_step(xa, xp, xn, label_t[ia], label_t[ip], images, lr=lr, weight_decay=args.weight_decay,
                                                max_grad_norm=args.max_grad_norm)
                    loss_sum = loss_sum + losses["total"]
                else:
                    w, grads = shard_weights(len(batch), world, B), None
                    if idx:                                                      # an empty slice: no forward, no backward, a zero row at weight 0
                        losses, grads = trainer.forward_backward(xa, xp, xn, label_t[ia], label_t[ip], images + rank * B)
                        loss_sum = loss_sum + w[rank] * losses["total"]
                    merged = exchange.exchange(grads, w)
                    if args.max_grad_norm > 0:
                        trainer.clip(merged, args.max_grad_norm)
                    trainer.step(merged, lr, args.weight_decay)
                if idx:
                    saved_bytes = max(saved_bytes, trainer.saved_bytes(xa.shape))
                idx = batch                                                      # (the counters below are the global batch's)
                lrs.append(lr)
                step, images, epoch_images = step + 1, images + len(idx), epoch_images + len(idx)
                if k % args.logging_steps == 0:
                    v = read_back(loss_sum, losses, f"epoch {epoch}, step {k}")
                    kl_name = "KL(监控)" if simplified else "KL"
                    print(f"Epoch: {epoch}, Step: {k}, Total: {v[1]:.4f}, Recon: {v[2]:.4f}, {kl_name}: {v[3]:.4f}, Triplet: {v[4]:.4f}, LR: {lr:.2e}")
            v = read_back(loss_sum, losses, f"epoch {epoch}")
            seconds = time.perf_counter() - t0
            train_loss = v[0] / len(lrs)
            if sharded:
                report["sharded"].update(state_sha256=agreed_digest(f"after epoch {epoch}"), exchange_calls=exchange.calls)
                if not chief:                                                    # rank 0 validates and writes; the others meet it at the barrier
                    shard.dist.barrier(group=shard.group)
                    continue
            trainer.commit(model)
            state, _, _ = evaluate_vae.run_checkpoint(args, model, val_data, val_labels, val_triplets, val_batches, device=device)
            val_loss = evaluate_vae.build_report(state, args)["val_loss"]
            next_lr = args.learning_rate * lr_schedule(args.lr_scheduler_type, step, args.lr_warmup_steps, total_steps)
            history["train_loss"].append(train_loss)
            history["val_loss"].append(val_loss)
            history["learning_rates"].append(next_lr)                        # (the reference reads the lr after its scheduler's step)
            print(f"Epoch {epoch} completed - Train Loss: {train_loss:.4f}, Val Loss: {val_loss:.4f}")
            norm = trainer.grad_norm() if args.max_grad_norm > 0 else None
            improved = val_loss < best
            if improved:
                best = val_loss
                print(f"New best validation loss: {best:.4f}")
            run = {"step": step, "epoch": epoch + 1, "images": images, "best_val_loss": None if math.isinf(best) else best, "history": history}
            if improved:
                save_checkpoint(os.path.join(args.output_dir, "best_checkpoint"), trainer, config, run)
                save_model(os.path.join(args.output_dir, "best_vae"), trainer, config)
                print(f"最佳模型已保存到: {os.path.join(args.output_dir, 'best_vae')}")
            if (epoch + 1) % args.save_steps == 0:
                save_checkpoint(os.path.join(args.output_dir, f"checkpoint-{epoch}"), trainer, config, run)
                save_model(os.path.join(args.output_dir, f"vae_checkpoint_epoch_{epoch}"), trainer, config)
                print(f"检查点已保存到: {os.path.join(args.output_dir, f'vae_checkpoint_epoch_{epoch}')}")
            report["epochs"].append({"epoch": epoch, "seconds": seconds, "images_per_second": epoch_images / seconds, "steps": len(lrs),
                                     "images": epoch_images, "learning_rates": lrs, "train_loss": train_loss, "val_loss": val_loss,
                                     "grad_norm": None if norm is None else {"norm": norm[0], "coef": norm[1]},
                                     "saved_bytes_per_step": saved_bytes, "optimizer_state_sha256": trainer.optimizer_state_sha256().hexdigest()})
            _write_json(report_path, report)
            if sharded:
                shard.dist.barrier(group=shard.group)
    if not chief:
        return report
    print("训练完成，保存训练历史...")
    _write_json(os.path.join(args.output_dir, "training_history.json"), history)
    print("VAE训练完成！")
    return report


def main(argv=None):
    return train(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
