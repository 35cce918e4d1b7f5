"""Joint training of the VAE and the tag decoder on the GPU: the reference's train_full.py (lines 30-399) -- three encodes, the classifier on
the anchor posterior's mode, triplet + classification loss (SimplifiedCombinedLoss, the reference CLI's only mode) or, with --full_loss,
reconstruction + KL + triplet + classification (CombinedLoss), ONE clip_grad_norm_ over both models, ONE AdamW.

    python -m vae_tagger_amd.train_full --json_path data.json --tags_csv_path tags.csv [--vae_checkpoint ae.safetensors | --vae_config_path cfg.json]
        [--decoder_checkpoint dec.bin] [--no_attention | --use_cross_attention] [--full_loss] [--resume_from full_output/checkpoint-4] ...

  joint_clip_host   the 16 bytes vt_full_optim_norm writes, from the two fp64 squared norms (the host mirror the tests compare with)
  FullTrainer       a train_vae.VAETrainer and a decoder-side trainer (train.DecoderTrainer for attention decoders, cross-attention included;
                    train.HeadTrainer for the plain decoder) and the joint step on them
  train / main      the CLI: the reference's flags and defaults; per epoch evaluate_vae.run_checkpoint(..., decoder=...) and the reference's files

What the simplified loss trains.  The reconstruction is computed by the reference and never enters SimplifiedCombinedLoss (train_full.py:227-234,
improved_losses.py:160-222), so every `decoder.*` tensor of the VAE has grad None there: clip_grad_norm_ skips it, and AdamW skips it too -- no moment
update, no weight decay.  Here that step decodes nothing (vae_backward.vae_triplet_loss_and_grads) and the clip and AdamW run over the encoder's
tensors alone, which come first in the VAE trainer's arenas: the same arenas, a smaller n, and the `decoder.*` ranges keep their bytes.  The
classifier reads mode() * scaling_factor + shift_factor of the anchor's moments under no_grad (train_full.py:217-224; vt_posterior_mode_latent), so
no gradient flows from the classification loss into the VAE and the two backward passes meet only in the gradient norm.

What differs from the reference, on purpose: everything train_vae's docstring lists (the split and the epoch order from the seed alone, triplets per
epoch and anchor, the counter-based noise, the bucketing rule, nothing read back per step), whose helpers this module imports.  Refused, each with a
message that names the flag: --gradient_accumulation_steps > 1 without --accumulate_gradients, --use_adaptive_weights, --use_quant_conv /
--use_post_quant_conv, --sharded, and --triplet_weight <= 0 under the simplified loss (the reference then drops the term and the whole VAE has no
gradient).

Gradient accumulation (--accumulate_gradients --gradient_accumulation_steps A; FullTrainer.micro_step, accumulation_plan) is the reference's loop
(train_full.py:246-255): every micro-step backpropagates loss / A into the accumulated gradient of both models and clips THAT; the optimiser, the
schedule and the zeroing run when (step + 1) % A == 0 with `step` counted inside the epoch, so an epoch's tail stays pending into the next one.
A checkpoint taken with micro-steps pending also holds pending_gradients.safetensors, and state.json the three counters.
"""
import argparse
import ctypes
import json
import math
import os
import struct
import time
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from .train import ADAM_BETAS, ADAM_EPS, SCHEDULES, DecoderTrainer, HeadTrainer, epoch_order, front_trainable, lr_schedule, split_indices
from .train_vae import (MODEL_FILE, OPTIMIZER_FILE, STATE_FILE, TRIPLET_SEED_STRIDE, VAETrainer, _write_json, load_optimizer_state, model_config,
                        plan_train_batches, save_model, save_optimizer_state, steps_per_epoch)

IGNORED_ARGUMENTS = ("mixed_precision", "cudnn_benchmark", "cudnn_deterministic", "num_workers", "prefetch_factor",
                     "enable_xformers_memory_efficient_attention", "use_safetensors")
DECODER_FILE, DECODER_OPTIMIZER_FILE, PENDING_FILE = "pytorch_model.bin", "decoder_optimizer.safetensors", "pending_gradients.safetensors"
_KINDS = ((_lib.HEAD_PARAM, "param."), (_lib.HEAD_ADAM_M, "exp_avg."), (_lib.HEAD_ADAM_V, "exp_avg_sq."))


def joint_clip_host(sq_vae, sq_blocks, max_norm):
    """The 16 bytes { fp64 norm^2, fp32 norm, fp32 coef } vt_full_optim_norm writes to every scalars block, from S_vae and S_blocks: one fp64 add
    (the VAE first), norm = (float)sqrt(total), coef = max_norm / (norm + 1e-6f) in fp32, 1 unless that is < 1."""
    total = np.float64(sq_vae) + np.float64(sq_blocks)
    norm = np.float32(np.sqrt(total))
    coef = np.float32(max_norm) / (norm + np.float32(1e-6))
    if not coef < np.float32(1.0):
        coef = np.float32(1.0)
    return struct.pack("<dff", float(total), float(norm), float(coef))


class FullTrainer:
    """The joint step of train_full on one device.

    vae_source: what VAETrainer takes (a state dict of `encoder.*` and `decoder.*`, a DiffusersVAEWrapper or an AutoencoderKL); decoder: a tag decoder
    module on the device -- an attention decoder is trained in full (DecoderTrainer), the plain one through its head (HeadTrainer: its front is the
    parameter-free pool).  weights: {"reconstruction", "kl", "triplet", "classification"}.  simplified=True is SimplifiedCombinedLoss: only the
    VAE's encoder is trained.  dropout (None: the reference's rates) and attention_dropout are the decoder side's.  scaling_factor / shift_factor
    (None: absent) shape the classifier's input; from a loaded model they default to its configuration's.  Everything is queued on torch's current stream; grad_norm() and the digests synchronise."""

    def __init__(self, vae_source, decoder, *, weights, simplified=True, margin=1.0, similarity_type="cosine", seed=0, loss="bce", focal_alpha=1.0,
                 focal_gamma=2.0, class_weights=None, dropout=None, attention_dropout=0.1, scaling_factor="config", shift_factor="config"):
        self.simplified = bool(simplified)
        w = {k: float(weights.get(k, 0.0)) for k in ("reconstruction", "kl", "triplet", "classification")}
        self.weights = w
        vae_weights = {"reconstruction": 0.0, "kl": 0.0, "triplet": w["triplet"]} if self.simplified else {k: w[k] for k in ("reconstruction", "kl", "triplet")}
        self.device = next(decoder.parameters()).device
        self.vae = VAETrainer(vae_source, weights=vae_weights, margin=margin, similarity_type=similarity_type, seed=seed, device=self.device)
        cfg = getattr(getattr(vae_source, "vae", vae_source), "config", None)
        self.scaling = getattr(cfg, "scaling_factor", None) if scaling_factor == "config" else scaling_factor
        self.shift = getattr(cfg, "shift_factor", None) if shift_factor == "config" else shift_factor
        self.decoder = decoder
        if front_trainable(decoder):
            self.dec = DecoderTrainer(decoder, loss, focal_alpha, focal_gamma, class_weights, dropout, attention_dropout, seed)
            self.blocks = [self.dec.head, self.dec.front] + ([self.dec.cross] if self.dec.cross is not None else [])
        else:
            self.dec = HeadTrainer(decoder, loss, focal_alpha, focal_gamma, class_weights, dropout, seed)
            self.blocks = [self.dec]
        self.head = self.blocks[0]
        keys = list(self.vae.params)
        self.n_encoder = sum(1 for k in keys if k.startswith("encoder."))
        if not all(k.startswith("encoder.") for k in keys[:self.n_encoder]):
            raise ValueError("FullTrainer: the encoder's tensors come first in the VAE trainer's arenas")
        self.n = self.n_encoder if self.simplified else len(keys)                # the tensors the clip and AdamW run over: a prefix
        self._numel_arr = (ctypes.c_longlong * self.n)(*self.vae.numels[:self.n])
        self._ring = torch.zeros(_lib.HEAD_RING, dtype=torch.float64, device=self.device)
        self._saved = {}
        self._ws = None
        self.t = 0
        self.micro = self.pending = 0                                            # micro_step's counters: micro-steps in all, and since the last step

    # -- the step ---------------------------------------------------------------------------------------------------------------------------
    def saved_bytes(self, shape):
        """Bytes the VAE side keeps between forward and backward for a batch of this shape (the decoder side's workspaces do not depend on it)."""
        from . import vae_backward
        shape = tuple(shape)
        if shape not in self._saved:
            B, _, H, W = shape
            if self.simplified:
                need = vae_backward.vae_triplet_saved_bytes(self.vae.shapes, B, H, W)
                free = torch.cuda.mem_get_info(self.device)[0] + torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device)
                if need > free:
                    raise MemoryError(f"FullTrainer: a [{B}, 3, {H}, {W}] batch keeps {need} bytes between forward and backward; the device has {free} bytes free")
            else:
                need = self.vae.check_memory(B, H, W)
            self._saved[shape] = need
        return self._saved[shape]

    def vae_forward_backward(self, anchor, positive, negative, labels_a=None, labels_p=None, first_image=0):
        """-> (losses, grads of the first n tensors keyed like them, moments [3B, 2L, h, w])"""
        from . import vae_backward
        v = self.vae
        v.ctx
        self.saved_bytes(anchor.shape)
        moments = []
        common = dict(margin=v.margin, similarity_type=v.similarity_type, seed=v.seed, first_image=int(first_image), moments_out=moments)
        if self.simplified:
            losses, grads = vae_backward.vae_triplet_loss_and_grads(v.params, anchor, positive, negative, labels_a, labels_p,
                                                                    triplet_weight=v.weights["triplet"], **common)
        else:
            losses, grads = vae_backward.vae_loss_and_grads(v.params, anchor, positive, negative, labels_a, labels_p, weights=v.weights, **common)
        return losses, grads, moments[0]

    def mode_latent(self, moments, B):
        """mode() * scaling_factor + shift_factor of the first B images' moments (vt_posterior_mode_latent): the decoder's input"""
        _, C2, h, w = moments.shape
        out = torch.empty(B, C2 // 2, h, w, dtype=torch.float32, device=moments.device)
        self.vae.ctx.call("vt_posterior_mode_latent", ctypes.c_void_p(moments.data_ptr()), B, C2 // 2, h * w,
                          float(self.scaling if self.scaling is not None else 1.0), int(self.scaling is not None),
                          float(self.shift if self.shift is not None else 0.0), int(self.shift is not None), ctypes.c_void_p(out.data_ptr()),
                          self.vae._stream())
        return out

    def decoder_forward_backward(self, latent, labels, step, loss_scale=None):
        """the decoder side's forward, loss (x loss_scale; None: the classification weight) and backward, which ADDS to the blocks' gradients;
        -> the scaled loss, a 0-d float64 device tensor"""
        scale = self.weights["classification"] if loss_scale is None else float(loss_scale)
        if isinstance(self.dec, DecoderTrainer):
            self.dec.forward_backward(latent, labels, loss_scale=scale, train=True, step=step)
        else:
            self.dec.forward_backward(self.dec.features(latent), labels, loss_scale=scale, train=True, step=step)
        self.head._call("read", _lib.HEAD_LOSS_RING, None, ctypes.c_void_p(self._ring.data_ptr()), 8 * _lib.HEAD_RING)      # device to device, in stream order
        return self._ring[step % _lib.HEAD_RING].clone()

    def _pointers(self, grads):
        keys = list(self.vae.params)[:self.n]
        if list(grads.keys()) != keys:
            raise ValueError("the gradients are keyed and ordered like the first n of the VAE trainer's params")
        ptrs = (ctypes.c_void_p * self.n)()
        for i, (k, g) in enumerate(grads.items()):
            if g.dtype != torch.float32 or g.device != self.device or not g.is_contiguous() or tuple(g.shape) != self.vae.shapes[k]:
                raise ValueError(f"{k}: a contiguous fp32 gradient of shape {self.vae.shapes[k]} on {self.device} is expected")
            ptrs[i] = g.data_ptr()
        return ptrs

    def _block_states(self):
        out = []
        for i in range(3):
            out.extend(self.blocks[i]._state() if i < len(self.blocks) else (None, 0))
        return out

    def clip(self, grads, max_norm, chunk=0):
        """ONE clip_grad_norm_ over the VAE's n gradient tensors and every decoder-side block (vt_full_optim_norm): the blocks' gradients are
        scaled in place, the VAE's are not written -- step() folds the coefficient in."""
        v, ptrs = self.vae, self._pointers(grads)
        if self._ws is None:
            need = v.ctx.lib.vt_vae_optim_workspace_bytes(self._numel_arr, self.n)
            self._ws = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
            self._ws_ptr, self._ws_bytes = (self._ws.data_ptr() + 255) // 256 * 256, need
        self.head.ctx.call("vt_full_optim_norm", ptrs, self._numel_arr, self.n, float(max_norm), ctypes.c_void_p(v._scalars.data_ptr()),
                           ctypes.c_void_p(self._ws_ptr), self._ws_bytes, int(chunk), *self._block_states(), v._stream())
        v._clipped = True

    def step(self, grads, lr, weight_decay=0.0, betas=ADAM_BETAS, eps=ADAM_EPS, chunk=0):
        """AdamW's next update of the VAE's n tensors and of every decoder-side block: one learning rate, one weight decay, one step count."""
        v, ptrs = self.vae, self._pointers(grads)
        scalars = ctypes.c_void_p(v._scalars.data_ptr()) if v._clipped else None
        v.ctx.call("vt_vae_optim_step", *(ctypes.c_void_p(a.data_ptr()) for a in v._arena), v.total, ptrs, self._numel_arr, self.n, scalars, float(lr),
                   float(betas[0]), float(betas[1]), float(eps), float(weight_decay), self.t + 1, int(chunk), v._stream())
        v.t = self.t + 1
        v._clipped = False
        for b in self.blocks:
            b.t = self.t
        self.dec.step(lr, weight_decay, betas, eps)
        self.t += 1

    def train_step(self, anchor, positive, negative, labels_a, labels_p=None, first_image=0, *, lr, weight_decay=0.0, max_grad_norm=1.0,
                   betas=ADAM_BETAS, eps=ADAM_EPS):
        """One step of train_full -> losses: the VAE's terms, "classification" (already x its weight) and "total", 0-d float64 device tensors."""
        losses, grads, moments = self.vae_forward_backward(anchor, positive, negative, labels_a, labels_p if labels_p is not None else labels_a, first_image)
        latent = self.mode_latent(moments, anchor.shape[0])
        losses = dict(losses)
        losses["classification"] = self.decoder_forward_backward(latent, labels_a, self.t)
        losses["total"] = losses["total"] + losses["classification"]
        if max_grad_norm > 0:
            self.clip(grads, max_grad_norm)
        self.step(grads, lr, weight_decay, betas, eps)
        return losses

    def micro_step(self, anchor, positive, negative, labels_a, labels_p=None, first_image=0, *, accumulation_steps, step_now, lr, weight_decay=0.0,
                   max_grad_norm=1.0, betas=ADAM_BETAS, eps=ADAM_EPS):
        """One micro-step of train_full under --gradient_accumulation_steps A, the reference's loop (train_full.py:246-255): the loss / A is
        backpropagated into the accumulated gradient of both models, clip_grad_norm_ runs on that accumulated gradient EVERY micro-step, and
        the optimiser steps (and zeroes the gradient) only when step_now.  The VAE's sum lives in its trainer's accumulation row
        (VAETrainer.accumulate at scale 1 / A); the coefficient a clip leaves is applied to the row by the NEXT accumulate, or folded into
        the step.  The blocks' backward adds into their gradients, the clip scales them in place, their step zeroes them.  `self.micro`
        counts micro-steps (it keys the decoder side's dropout masks and loss-ring slot; the front's BatchNorm statistics move every
        micro-step), `self.pending` those since the last optimiser step.  -> losses as train_step's, each x 1 / A (what the reference sums).
        At A = 1 with step_now this leaves the bytes train_step leaves."""
        A = int(accumulation_steps)
        if A < 1:
            raise ValueError("micro_step: accumulation_steps must be at least 1")
        row = self.vae.accumulation_row()                                        # (allocated before the memory check of a new batch shape)
        losses, grads, moments = self.vae_forward_backward(anchor, positive, negative, labels_a, labels_p if labels_p is not None else labels_a, first_image)
        latent = self.mode_latent(moments, anchor.shape[0])
        losses = {k: v / A for k, v in losses.items()}
        losses["classification"] = self.decoder_forward_backward(latent, labels_a, self.micro, self.weights["classification"] / A)
        losses["total"] = losses["total"] + losses["classification"]
        self.vae.accumulate(grads, scale=1.0 / A, first=self.pending == 0, n=self.n)
        del grads, row
        acc = self.vae.accumulated(self.n)
        if max_grad_norm > 0:
            self.clip(acc, max_grad_norm)
        self.micro += 1
        if step_now:
            self.step(acc, lr, weight_decay, betas, eps)
            self.pending = 0
        else:
            self.pending += 1
        return losses

    def pending_state_dict(self):
        """What a run interrupted between two optimiser steps carries: the accumulation row with the pending clip coefficient APPLIED (one fp32
        multiply on the device -- the multiply the next accumulate would have performed first, so a run that loads this with no coefficient
        pending continues on the same bits) and every block's accumulated gradients.  Host tensors; synchronises."""
        v = self.vae
        row = v.accumulation_row()
        if v._clipped:
            coef = v.grad_norm()[1]
            if coef < 1.0:
                row = row * coef                                                 # (coef is an fp32 value: the scalar multiply is that fp32 multiply)
        out = {"vae.row": row.detach().cpu().contiguous(), "pending": torch.tensor([self.pending], dtype=torch.int64)}
        for b in self.blocks:
            for name, shape in b.shapes.items():
                out["grad." + name] = b._read(_lib.HEAD_GRAD, name, shape, torch.float32)
        return out

    def load_pending_state_dict(self, state):
        want = {"vae.row", "pending"} | {"grad." + name for b in self.blocks for name in b.shapes}
        if set(state.keys()) != want or state["vae.row"].numel() != self.vae.total:
            raise ValueError("load_pending_state_dict: vae.row of the arenas' layout, pending and grad.* of this decoder's tensors are expected")
        self.vae.accumulation_row().copy_(state["vae.row"].to(torch.float32).reshape(-1))
        self.vae._clipped = False
        for b in self.blocks:
            for name in b.shapes:
                b.write(_lib.HEAD_GRAD, name, state["grad." + name].reshape(b.shapes[name]))
        self.pending = int(state["pending"][0])

    def grad_norm(self):
        """(joint L2 norm, clip coefficient) of the last clip(); synchronises."""
        return self.vae.grad_norm()

    # -- state ------------------------------------------------------------------------------------------------------------------------------
    def commit(self, vae_model=None):
        """The trained tensors into the loaded models: the decoder's device tables, and the VAE module when one is given."""
        if vae_model is not None:
            self.vae.commit(vae_model)
        self.dec.commit()

    def decoder_state_dict(self):
        return self.dec.state_dict()

    def decoder_optimizer_state_dict(self):
        """every decoder-side block's parameters and Adam moments, the front's BatchNorm buffers and the step count (host tensors)"""
        out = {"step": torch.tensor([self.t], dtype=torch.int64)}
        for b in self.blocks:
            for name, shape in b.shapes.items():
                for kind, tag in _KINDS:
                    out[tag + name] = b._read(kind, name, shape, torch.float32)
            for name in getattr(b, "buffers", {}):
                out["buffer." + name] = b.buffer(name).reshape(-1)
        return out

    def load_decoder_optimizer_state_dict(self, state):
        want = {"step"}
        for b in self.blocks:
            want |= {tag + name for name in b.shapes for _, tag in _KINDS} | {"buffer." + name for name in getattr(b, "buffers", {})}
        if set(state.keys()) != want:
            raise ValueError("load_decoder_optimizer_state_dict: step, param.*, exp_avg.*, exp_avg_sq.* and buffer.* of this decoder's tensors are expected")
        for b in self.blocks:
            for name in b.shapes:
                for kind, tag in _KINDS:
                    b.write(kind, name, state[tag + name].reshape(b.shapes[name]))
            for name, shape in getattr(b, "buffers", {}).items():
                b.write_buffer(name, state["buffer." + name].reshape(shape))
            b.t = b.calls = int(state["step"][0])

    def save(self, path, config=None):
        """Both models and both optimiser states into one directory: what --resume_from reads."""
        from safetensors.torch import save_file
        save_model(path, self.vae, config if config is not None else {})
        save_optimizer_state(os.path.join(path, OPTIMIZER_FILE), self.vae.optimizer_state_dict())
        torch.save(self.decoder_state_dict(), os.path.join(path, DECODER_FILE))
        save_file({k: v.contiguous() for k, v in self.decoder_optimizer_state_dict().items()}, os.path.join(path, DECODER_OPTIMIZER_FILE))
        pending = os.path.join(path, PENDING_FILE)
        if self.pending > 0:
            save_file(self.pending_state_dict(), pending)
        elif os.path.exists(pending):                                            # (a directory written before, at another point of the schedule)
            os.remove(pending)

    def load(self, path):
        from safetensors.torch import load_file
        self.vae.load_state_dict(load_file(os.path.join(path, MODEL_FILE)))
        self.vae.load_optimizer_state_dict(load_optimizer_state(os.path.join(path, OPTIMIZER_FILE)))
        self.load_decoder_optimizer_state_dict(load_file(os.path.join(path, DECODER_OPTIMIZER_FILE)))
        self.t = self.vae.t
        if any(b.t != self.t for b in self.blocks):
            raise ValueError(f"{path}: the two optimiser states are at different steps")
        self.pending = 0
        if os.path.exists(os.path.join(path, PENDING_FILE)):
            self.load_pending_state_dict(load_file(os.path.join(path, PENDING_FILE)))

    def state_sha256(self):
        """{"vae", "decoder"}: SHA-256 over the parameters and Adam moments of each model"""
        return {"vae": self.vae.optimizer_state_sha256().hexdigest(), "decoder": self.dec.optimizer_state_sha256().hexdigest()}


# ---- the CLI --------------------------------------------------------------------------------------------------------------------------
def build_parser():
    p = argparse.ArgumentParser(description="VAE + 分类解码器联合训练, 前向、反向与优化器都在GPU上。")
    p.add_argument("--json_path", type=str, required=True)
    p.add_argument("--tags_csv_path", type=str, required=True)
    p.add_argument("--output_dir", type=str, default="full_output")
    p.add_argument("--vae_checkpoint", type=str, default=None, help="预训练VAE模型文件路径 (.safetensors)")
    p.add_argument("--vae_config_path", type=str, default=None, help="VAE配置文件路径 (JSON格式)")
    p.add_argument("--decoder_checkpoint", type=str, default=None, help="预训练decoder模型文件路径 (.bin/.pth)")
    p.add_argument("--resolution", type=int, default=1024)
    p.add_argument("--train_batch_size", type=int, default=1)
    p.add_argument("--num_epochs", type=int, default=10)
    p.add_argument("--learning_rate", type=float, default=1e-4)
    p.add_argument("--weight_decay", type=float, default=1e-6)
    p.add_argument("--use_attention", action="store_true", default=True, help="启用注意力机制 (默认开启)")
    p.add_argument("--no_attention", action="store_true", help="禁用注意力机制")
    p.add_argument("--use_spatial_attention", action="store_true", default=True, help="启用空间注意力")
    p.add_argument("--use_self_attention", action="store_true", default=True, help="启用自注意力")
    p.add_argument("--use_cross_attention", action="store_true", help="启用交叉注意力")
    p.add_argument("--attention_heads", type=int, default=8, help="注意力头数")
    p.add_argument("--attention_dropout", type=float, default=0.1, help="注意力dropout率")
    p.add_argument("--reconstruction_weight", type=float, default=0.01)
    p.add_argument("--kl_weight", type=float, default=1e-7)
    p.add_argument("--triplet_weight", type=float, default=1.0)
    p.add_argument("--bce_weight", type=float, default=1.0)
    p.add_argument("--triplet_margin", type=float, default=1.0)
    p.add_argument("--use_simplified_loss", action="store_true", default=True, help="使用简化版损失函数（推荐）")
    p.add_argument("--use_focal_loss", action="store_true", help="使用Focal Loss处理类别不平衡")
    p.add_argument("--use_class_balanced", action="store_true", help="使用类别平衡损失")
    p.add_argument("--use_adaptive_weights", action="store_true", help="refused: AdaptiveLossWeights has no gradient here")
    p.add_argument("--focal_alpha", type=float, default=1.0, help="Focal Loss的alpha参数")
    p.add_argument("--focal_gamma", type=float, default=2.0, help="Focal Loss的gamma参数")
    p.add_argument("--similarity_type", type=str, default="cosine", choices=["cosine", "euclidean"], help="三元组损失的相似性度量")
    p.add_argument("--lr_scheduler_type", type=str, default="cosine", help="学习率调度器类型")
    p.add_argument("--lr_warmup_steps", type=int, default=500, help="学习率预热步数")
    p.add_argument("--max_grad_norm", type=float, default=1.0, help="梯度裁剪阈值")
    p.add_argument("--logging_steps", type=int, default=100, help="日志记录间隔")
    p.add_argument("--save_steps", type=int, default=5, help="模型保存间隔（epochs）")
    p.add_argument("--mixed_precision", type=str, default="fp16")
    p.add_argument("--enable_xformers_memory_efficient_attention", action="store_true", help="启用 xformers 加速")
    p.add_argument("--use_quant_conv", action="store_true", help="refused: VAE config use_quant_conv has no backward here")
    p.add_argument("--use_post_quant_conv", action="store_true", help="refused: VAE config use_post_quant_conv has no backward here")
    p.add_argument("--use_safetensors", action="store_true", help="使用SafeTensors格式保存模型")
    p.add_argument("--use_bucketing", action="store_true", help="启用长宽比分桶功能")
    p.add_argument("--base_resolution", type=int, default=512, help="分桶的基础分辨率")
    p.add_argument("--max_resolution", type=int, default=1024, help="分桶的最大分辨率")
    p.add_argument("--bucket_step", type=int, default=64, help="分桶的步长")
    p.add_argument("--num_workers", type=int, default=4, help="DataLoader 工作线程数")
    p.add_argument("--prefetch_factor", type=int, default=2, help="DataLoader 预取倍数（每个worker）")
    p.add_argument("--gradient_accumulation_steps", type=int, default=1, help="梯度累积步数 (above 1 only with --accumulate_gradients)")
    p.add_argument("--seed", type=int, default=42, help="随机种子")
    p.add_argument("--cudnn_benchmark", action="store_true", help="启用cudnn benchmark以提高卷积性能（输入尺寸固定时建议开启）")
    p.add_argument("--cudnn_deterministic", action="store_true", help="启用确定性cuDNN以提高复现性（可能降低性能）")
    # this project's own
    p.add_argument("--full_loss", action="store_true", help="CombinedLoss: reconstruction and KL enter the total and the VAE's image decoder is "
                                                            "trained (the reference's --use_simplified_loss cannot be switched off)")
    p.add_argument("--resume_from", type=str, default=None, help="continue from a best_checkpoint/ or checkpoint-{e}/ directory")
    p.add_argument("--stop_after_epochs", type=int, default=0, help="end the run after this many epochs of --num_epochs (0: all); the schedule is --num_epochs'")
    p.add_argument("--workers", type=int, default=0, help="image decode threads (0 = min(16, cores))")
    p.add_argument("--sharded", action="store_true", help="refused: the joint step is not sharded")
    p.add_argument("--accumulate_gradients", action="store_true", help="accept --gradient_accumulation_steps A: the reference's loop, the loss / A "
                                                                       "into an accumulated gradient that is clipped EVERY micro-step, an optimiser "
                                                                       "step when (step + 1) %% A == 0 inside an epoch")
    return p


def ignored_arguments(args):
    """The reference's flags that mean nothing here and were set to something."""
    defaults = build_parser().parse_args(["--json_path", "", "--tags_csv_path", ""])
    return [k for k in IGNORED_ARGUMENTS if getattr(args, k, None) != getattr(defaults, k)]


def check_args(args):
    """What is refused, before any GPU work; each message names its flag."""
    if args.no_attention:
        args.use_attention = False
    accumulate = getattr(args, "accumulate_gradients", False)
    if args.gradient_accumulation_steps > 1 and not accumulate:
        raise RuntimeError("--gradient_accumulation_steps > 1 needs --accumulate_gradients: the reference clips every micro-step on the accumulated "
                           "gradient and steps by the position inside the epoch, which is what that flag runs")
    if accumulate and args.gradient_accumulation_steps < 1:
        raise RuntimeError("--accumulate_gradients: --gradient_accumulation_steps must be at least 1")
    if args.use_adaptive_weights:
        from .improved_losses import CombinedLoss
        try:
            CombinedLoss(use_adaptive_weights=True)                              # improved_losses' own refusal, whatever it says
        except NotImplementedError as e:
            raise RuntimeError(f"--use_adaptive_weights: {e}")
    if args.use_quant_conv or args.use_post_quant_conv:
        raise RuntimeError("--use_quant_conv / --use_post_quant_conv: these VAE configurations have no backward here")
    if args.sharded:
        raise RuntimeError("--sharded is not implemented for train_full: the joint step runs on one device")
    simplified = bool(args.use_simplified_loss) and not args.full_loss
    if simplified and not args.triplet_weight > 0:
        raise RuntimeError("--triplet_weight must be positive under the simplified loss: the reference then drops the term and the whole VAE has no "
                           "gradient (train the decoder alone with train_decoder)")
    if args.use_attention and (args.attention_heads not in (1, 2, 4, 8) or not 0.0 <= args.attention_dropout < 1.0):
        raise RuntimeError("--attention_heads must be 1, 2, 4 or 8 and --attention_dropout in [0, 1)")
    if args.lr_scheduler_type not in SCHEDULES:
        raise RuntimeError(f"--lr_scheduler_type {args.lr_scheduler_type}: one of {', '.join(SCHEDULES)} expected")
    if args.train_batch_size < 1 or args.num_epochs < 1 or args.save_steps < 1 or args.logging_steps < 1:
        raise RuntimeError("--train_batch_size, --num_epochs, --save_steps and --logging_steps must be at least 1")
    return args


def accumulation_plan(steps_per_epoch, num_epochs, accumulation_steps):
    """(epoch, step, first, step_now) per micro-step of a run, the reference's rule taken literally (train_full.py:201, 252): `step` counts from 0
    inside every epoch and the optimiser steps iff (step + 1) % A == 0.  `first`: no micro-gradient is pending, this one starts a new sum.  A tail
    of an epoch that does not fill a group of A stays pending across the validation pass and into the next epoch, so the next optimiser step
    carries more than A micro-gradients; what is pending after the last epoch is dropped.  The specification of what train() does with its
    per-epoch batch index and FullTrainer.pending: the tests hold the run's counters against it."""
    spe, epochs, A = int(steps_per_epoch), int(num_epochs), int(accumulation_steps)
    if spe < 1 or epochs < 1 or A < 1:
        raise ValueError("accumulation_plan: steps_per_epoch, num_epochs and accumulation_steps are at least 1")
    pending = 0
    for epoch in range(epochs):
        for step in range(spe):
            step_now = (step + 1) % A == 0
            yield epoch, step, pending == 0, step_now
            pending = 0 if step_now else pending + 1


def _make_decoder(args, n_tags, device):
    from .infer_full import load_state_dict_file
    from .modules import ClassificationDecoder, create_attention_decoder, get_vae_latent_info
    info = get_vae_latent_info(args.resolution)
    if args.use_attention:
        decoder = create_attention_decoder(info["latent_channels"], info["latent_height"], info["latent_width"], n_tags,
                                           {"use_spatial_attention": args.use_spatial_attention, "use_self_attention": args.use_self_attention,
                                            "use_cross_attention": args.use_cross_attention, "attention_heads": args.attention_heads,
                                            "attention_dropout": args.attention_dropout})
    else:
        print("使用标准分类解码器")
        decoder = ClassificationDecoder(info["latent_channels"], info["latent_height"], info["latent_width"], n_tags)
    if args.decoder_checkpoint and os.path.exists(args.decoder_checkpoint):
        print(f"加载预训练decoder模型: {args.decoder_checkpoint}")
        try:
            decoder.load_state_dict(load_state_dict_file(args.decoder_checkpoint), strict=False)
        except Exception as e:  # noqa: BLE001 - reference behaviour (train_full.py:90-95)
            print(f"Decoder模型加载失败，从零开始训练: {e}")
    else:
        print("从零开始训练decoder模型")
    return decoder.to(device).eval()


def train(args):
    """`args`: a namespace of build_parser() that has passed check_args (main does both)."""
    from concurrent.futures import ThreadPoolExecutor
    import pandas as pd
    from . import evaluate_vae
    from .evaluate import TaggedImageList
    from .evaluation import evaluate_and_search
    from .infer_vae import _EncoderInput
    from .losses import class_balanced_weights, class_distribution, select_loss
    from .modules import AspectRatioBucketing, get_image_transform
    from .pipeline import EncodeTagPipeline
    from .prefetch import FeederLoader
    from .vae_reconstruction_test import load_vae_model
    if not torch.cuda.is_available():
        raise RuntimeError("vae_tagger_amd needs an MI355X (no HIP device visible; there is no CPU fallback)")
    ignored = ignored_arguments(args)
    if ignored:
        print("ignored arguments (they mean nothing on this device): " + ", ".join("--" + k for k in ignored))
    os.makedirs(args.output_dir, exist_ok=True)
    device = torch.device("cuda", torch.cuda.current_device())
    simplified = bool(args.use_simplified_loss) and not args.full_loss
    # what evaluate_vae.run_checkpoint / build_report read from the namespace
    args.use_simplified_vae_loss, args.classification_weight = simplified, args.bce_weight
    print("使用简化版损失函数" if simplified else "使用完整版损失函数")

    data = TaggedImageList(args.json_path, args.tags_csv_path)
    for p in data.missing:
        print(f"跳过图像 {p}，错误原因: 文件不存在")
    paths = data.image_paths
    tag_names = [str(t) for t in pd.read_csv(args.tags_csv_path)["name"]]
    train_idx, val_idx = split_indices(len(paths), args.seed)
    print(f"训练集大小: {len(train_idx)}, 验证集大小: {len(val_idx)}")
    train_paths, val_paths = [paths[i] for i in train_idx], [paths[i] for i in val_idx]
    train_labels = np.stack([data.labels[p] for p in train_paths]).astype(np.float32)
    val_labels = np.stack([data.labels[p] for p in val_paths]).astype(np.float32)
    train_buckets = val_buckets = bucketing = None
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
    decoder = _make_decoder(args, len(tag_names), device)
    selected = select_loss(args.use_class_balanced, args.use_focal_loss)
    class_weights = None
    if args.use_class_balanced:
        all_labels = TaggedImageList(args.json_path, args.tags_csv_path, check_files=False).labels
        class_weights = class_balanced_weights(class_distribution(all_labels, len(tag_names)))
    weights = {**evaluate_vae.loss_weights(args), "classification": args.bce_weight}
    trainer = FullTrainer(model, decoder, weights=weights, simplified=simplified, margin=args.triplet_margin, similarity_type=args.similarity_type,
                          seed=args.seed, loss=selected, focal_alpha=args.focal_alpha, focal_gamma=args.focal_gamma, class_weights=class_weights,
                          attention_dropout=args.attention_dropout)
    config = model_config(model.vae)
    spe = steps_per_epoch(len(train_idx), args.train_batch_size, train_buckets)
    total_steps = args.num_epochs * spe
    # `step` counts micro-steps (batches consumed); without accumulation every one of them is an optimiser step
    A = args.gradient_accumulation_steps if getattr(args, "accumulate_gradients", False) else 1
    run = {"step": 0, "epoch": 0, "images": 0, "best_val_loss": None, "history": {"train_loss": [], "val_loss": [], "learning_rates": []},
           "micro_steps": 0, "optimizer_steps": 0, "pending_micro_steps": 0}
    if args.resume_from:
        trainer.load(args.resume_from)
        with open(os.path.join(args.resume_from, STATE_FILE), "r", encoding="utf-8") as fh:
            run = json.load(fh)
        if run.get("optimizer_steps", run["step"]) != trainer.t or run["step"] != run["epoch"] * spe:
            raise SystemExit(f"{args.resume_from}: step {run['step']} does not match {run['epoch']} epochs of {spe} steps: other data or batch size")
        if run.get("pending_micro_steps", 0) != trainer.pending or (A == 1 and trainer.pending):
            raise SystemExit(f"{args.resume_from}: {run.get('pending_micro_steps', 0)} pending micro-steps in {STATE_FILE}, {trainer.pending} in "
                             f"{PENDING_FILE}, under --gradient_accumulation_steps {A}")
        trainer.micro = run.get("micro_steps", run["step"])
        print(f"resumed from {args.resume_from}: epoch {run['epoch']}, step {run['step']}, {run['images']} images consumed")
    history = run["history"]
    best = math.inf if run["best_val_loss"] is None else float(run["best_val_loss"])
    report_path = os.path.join(args.output_dir, "train_report.json")
    report = {"epochs": [], "clip": args.max_grad_norm > 0, "max_grad_norm": args.max_grad_norm, "ignored_arguments": ignored, "steps_per_epoch": spe,
              "total_steps": total_steps, "simplified": simplified, "arena_bytes": trainer.vae.arena_bytes(), "vae_tensors_trained": trainer.n,
              "decoder_blocks": len(trainer.blocks), "selected_loss": selected}
    if args.resume_from and os.path.exists(report_path):
        with open(report_path, "r", encoding="utf-8") as fh:
            report["epochs"] = json.load(fh).get("epochs", [])[:run["epoch"]]
    inputs = _EncoderInput(model)
    label_t = torch.from_numpy(train_labels).to(device)
    load = lambda pool, indices, bucket: evaluate_vae._load_batch(pool, train_paths, indices, args.resolution, bucket,
                                                                  lambda u8: inputs.normalize_u8(u8.to(device, non_blocking=True)))
    last_epoch = args.num_epochs if args.stop_after_epochs <= 0 else min(args.num_epochs, run["epoch"] + args.stop_after_epochs)
    step, images = run["step"], run["images"]
    terms = ("total", "reconstruction", "kl", "triplet", "classification")

    def read_back(loss_sum, losses, what):
        """the one place the host waits for the device inside an epoch: the running sum, the last step's terms, the health word"""
        values = torch.stack([loss_sum] + [losses[k] for k in terms]).cpu().tolist()
        st = trainer.vae.ctx.status()
        if st or not all(math.isfinite(v) for v in values):
            raise FloatingPointError(f"{what}: loss terms {values[1:]}, running sum {values[0]}, device health word {st}")
        return values

    def save_pair(vae_dir, dec_dir):
        save_model(os.path.join(args.output_dir, vae_dir), trainer.vae, config)
        os.makedirs(os.path.join(args.output_dir, dec_dir), exist_ok=True)
        torch.save(trainer.decoder_state_dict(), os.path.join(args.output_dir, dec_dir, DECODER_FILE))

    def save_checkpoint(name, state):
        path = os.path.join(args.output_dir, name)
        trainer.save(path, config)
        _write_json(os.path.join(path, STATE_FILE), state)

    with ThreadPoolExecutor(max_workers=max(1, args.workers or min(16, os.cpu_count() or 1))) as pool:
        for epoch in range(run["epoch"], last_epoch):
            t0 = time.perf_counter()
            order = epoch_order(len(train_idx), args.seed, epoch)
            triplets = {i: evaluate_vae.sample_triplet(args.seed * TRIPLET_SEED_STRIDE + epoch + 1, i, train_labels) for i in order}
            loss_sum = torch.zeros((), dtype=torch.float64, device=device)
            lrs, saved_bytes, epoch_images, losses, opt_before = [], 0, 0, None, trainer.t
            for k, (bucket, idx) in enumerate(plan_train_batches(order, args.train_batch_size, train_buckets)):
                xa = load(pool, idx, bucket)
                xp = load(pool, [triplets[i][0] for i in idx], bucket)
                xn = load(pool, [triplets[i][1] for i in idx], bucket)
                ia = torch.as_tensor(idx, device=device)
                ip = torch.as_tensor([triplets[i][0] for i in idx], device=device)
                # the schedule advances once per optimiser step over total_steps = num_epochs * steps_per_epoch (the reference's num_training_steps)
                lr = args.learning_rate * lr_schedule(args.lr_scheduler_type, trainer.t, args.lr_warmup_steps, total_steps)
                if A == 1:
                    losses = trainer.train_step(xa, xp, xn, label_t[ia], label_t[ip], images, lr=lr, weight_decay=args.weight_decay,
                                                max_grad_norm=args.max_grad_norm)
                else:                                                            # accumulation_plan's rule: k restarts every epoch
                    losses = trainer.micro_step(xa, xp, xn, label_t[ia], label_t[ip], images, accumulation_steps=A, step_now=(k + 1) % A == 0,
                                                lr=lr, weight_decay=args.weight_decay, max_grad_norm=args.max_grad_norm)
                loss_sum = loss_sum + losses["total"]
                saved_bytes = max(saved_bytes, trainer.saved_bytes(xa.shape))
                lrs.append(lr)
                step, images, epoch_images = step + 1, images + len(idx), epoch_images + len(idx)
                if k % args.logging_steps == 0:
                    v = read_back(loss_sum, losses, f"epoch {epoch}, step {k}")
                    vae_terms = "" if simplified else f"Recon: {v[2]:.4f}, KL: {v[3]:.4f}, "
                    print(f"Epoch: {epoch}, Step: {k}, Loss: {v[1]:.4f}, {vae_terms}Triplet: {v[4]:.4f}, Class: {v[5]:.4f}, LR: {lr:.2e}")
            v = read_back(loss_sum, losses, f"epoch {epoch}")
            seconds = time.perf_counter() - t0
            train_loss = v[0] / len(lrs)
            trainer.commit(model)
            state, _, classification = evaluate_vae.run_checkpoint(args, model, val_data, val_labels, val_triplets, val_batches, decoder=decoder,
                                                                   class_weights=class_weights, selected=selected, device=device)
            val_loss = evaluate_vae.build_report(state, args, classification)["val_loss_train_full"]
            next_lr = args.learning_rate * lr_schedule(args.lr_scheduler_type, trainer.t, args.lr_warmup_steps, total_steps)
            history["train_loss"].append(train_loss)
            history["val_loss"].append(val_loss)
            history["learning_rates"].append(next_lr)                        # (the reference reads the lr after its scheduler's step)
            print(f"Epoch {epoch} completed - Train Loss: {train_loss:.4f}, Val Loss: {val_loss:.4f}")
            norm = trainer.grad_norm() if args.max_grad_norm > 0 else None
            improved = val_loss < best
            if improved:
                best = val_loss
                print(f"New best validation loss: {best:.4f}")
            run = {"step": step, "epoch": epoch + 1, "images": images, "best_val_loss": None if math.isinf(best) else best, "history": history,
                   "micro_steps": step, "optimizer_steps": trainer.t, "pending_micro_steps": trainer.pending}
            if improved:
                save_checkpoint("best_checkpoint", run)
                save_pair("best_vae", "best_decoder")
                print(f"最佳VAE模型已保存到: {os.path.join(args.output_dir, 'best_vae')}")
                print(f"最佳decoder模型已保存到: {os.path.join(args.output_dir, 'best_decoder')}")
            if (epoch + 1) % args.save_steps == 0:
                save_checkpoint(f"checkpoint-{epoch}", run)
                save_pair("vae", "decoder")
                print(f"检查点VAE模型已保存到: {os.path.join(args.output_dir, 'vae')}")
                print(f"检查点decoder模型已保存到: {os.path.join(args.output_dir, 'decoder')}")
            report["epochs"].append({"epoch": epoch, "seconds": seconds, "images_per_second": epoch_images / seconds, "steps": len(lrs),
                                     "images": epoch_images, "learning_rates": lrs, "train_loss": train_loss, "val_loss": val_loss,
                                     "grad_norm": None if norm is None else {"norm": norm[0], "coef": norm[1]},
                                     "saved_bytes_per_step": saved_bytes, "state_sha256": trainer.state_sha256(), "accumulation_steps": A,
                                     "optimizer_steps": trainer.t - opt_before})
            _write_json(report_path, report)
    print("训练完成，开始最终评估...")
    _write_json(os.path.join(args.output_dir, "training_history.json"), history)
    trainer.commit(model)
    decoder.load_state_dict(trainer.decoder_state_dict(), strict=False)      # the module's own tensors follow the device tables
    decoder.to(device).eval()
    pipe = EncodeTagPipeline.input_side(model)
    loader = FeederLoader(pipe, val_paths, data.labels, args.train_batch_size, args.resolution, workers=args.workers or None, host_resize=False,
                          transform=get_image_transform(args.resolution), bucketing=bucketing, max_pending=None)
    optimal, metrics, _ = evaluate_and_search(model, decoder, loader, tag_names, device, args.output_dir)
    print("训练和评估完成！")
    return {"history": history, "report": report, "optimal_thresholds": optimal, "metrics": metrics}


def main(argv=None):
    args = build_parser().parse_args(argv)
    try:
        check_args(args)
    except RuntimeError as e:
        raise SystemExit(str(e))
    return train(args)


if __name__ == "__main__":
    main()
