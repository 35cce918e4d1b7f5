"""The VAE's image decoder (diffusers `decoder.*` tensors) over the HIP library: latents -> images.

AutoencoderKL holds one of these OUTSIDE its registered submodules (its state_dict() stays the encoder's), creates it on the first
decode() / load_decoder_state_dict() and moves it with .to()."""
import ctypes
import weakref

import torch

from . import _lib, synth
from ._runtime import HipModule, stream_ptr, vp, workspace


class DecoderOutput:
    def __init__(self, sample):
        self.sample = sample


class VAEImageDecoder(HipModule):
    def __init__(self, block_out_channels=synth.FLUX_BLOCK_OUT, out_channels=3, latent_channels=16, layers_per_block=2,
                 norm_num_groups=32, scaling_factor=None, shift_factor=None, seed=0):
        manifest = synth.image_decoder_manifest(tuple(block_out_channels), out_channels, latent_channels, layers_per_block)
        super().__init__(manifest, seed)
        self.block_out_channels = tuple(block_out_channels)
        self.out_channels, self.latent_channels = out_channels, latent_channels
        self.layers_per_block, self.norm_num_groups = layers_per_block, norm_num_groups
        self.scaling_factor, self.shift_factor = scaling_factor, shift_factor
        object.__setattr__(self, "_owner", None)

    def share_context_of(self, owner):
        """Run inside `owner`'s vt_context (an AutoencoderKL: one context, one set of flags, two allocation lists) instead of an own one."""
        object.__setattr__(self, "_owner", weakref.ref(owner))     # (not a registered submodule, in either direction)

    def _context(self):
        owner = self._owner() if self._owner is not None else None
        if owner is None:
            return super()._context()
        ctx = owner._context()
        if self._ctx is not ctx:
            self._ctx = ctx
            self._uploaded_version = None
        if self._uploaded_version is None:
            self._upload(ctx)
            self._uploaded_version = 1
        return ctx

    def _upload(self, ctx):
        blocks = (ctypes.c_int * len(self.block_out_channels))(*self.block_out_channels)
        sf, sh = self.scaling_factor, self.shift_factor
        ctx.call("vt_image_decoder_configure", self.out_channels, self.latent_channels, blocks, len(self.block_out_channels),
                 self.layers_per_block, self.norm_num_groups, float(sf if sf is not None else 1.0), int(sf is not None),
                 float(sh if sh is not None else 0.0), int(sh is not None))
        for k, v in self.state_dict().items():
            ctx.set_weight(k, v)
        ctx.call("vt_image_decoder_finalize")

    def set_fp16_operands(self, on=True):
        """fp16 instead of bf16 MFMA operands for the convolutions (vt_set_flag 18)."""
        self._context().call("vt_set_flag", 18, 1 if on else 0)

    def set_literal_upsample(self, on=True):
        """Upsample2D as a nearest-2x pass + the stride-1 conv instead of the folded kernel (vt_set_flag 22)."""
        self._context().call("vt_set_flag", 22, 1 if on else 0)

    def status(self, clear=True):
        dev = next(self.parameters()).device
        return self._context().status(clear, stream_ptr(dev))

    @torch.no_grad()
    def decode(self, z, unscale=False):
        """z [B, latent, h, w] -> fp32 [B, out_channels, h * 2^(blocks-1), w * 2^(blocks-1)]; unscale applies (z - shift) / scaling first."""
        ctx = self._context()                       # (raises the "no CPU fallback" VTError for CPU parameters)
        if z.dim() != 4 or z.shape[1] != self.latent_channels:
            raise ValueError(f"expected [B,{self.latent_channels},h,w], got {tuple(z.shape)}")
        z = z.detach().to(torch.float32).contiguous().to(next(self.parameters()).device)
        B, _, h, w = z.shape
        up = 1 << (len(self.block_out_channels) - 1)
        out = torch.empty(B, self.out_channels, h * up, w * up, dtype=torch.float32, device=z.device)
        need = ctx.lib.vt_decode_image_workspace_bytes(ctx.handle, B, h, w)
        if need == 0:
            raise _lib.VTError(f"vt_decode_image_workspace_bytes({B},{h},{w}) = 0: unsupported shape")
        ws, ptr = workspace(z.device, need)
        ctx.call("vt_decode_image", vp(z), B, h, w, int(bool(unscale)), vp(out), out.numel() * 4, ctypes.c_void_p(ptr), need,
                 stream_ptr(z.device))
        return out
