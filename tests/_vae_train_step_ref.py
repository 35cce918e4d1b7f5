"""One step of train_vae.py restated on the CPU, joined the way vae_backward.vae_loss_and_grads joins it: the functional encoder and decoder of
tests/_vae_model_backward_ref.py, the loss of tests/_vae_loss_backward_ref.py, the draws handed in (the device's own eps).  Three evaluations, as
for the models alone: fp64 autograd of the unrounded step (exact), the same in fp32 (the e32 yardstick), and the fp64 restatement with the device's
roundings composed from the per-model restatements (emu)."""
import torch

import _vae_loss_backward_ref as loss_ref
from _vae_model_backward_ref import (bf16_round_keep, decoder_backward_ref, decoder_forward_ref, encoder_backward_ref, encoder_forward_ref, split_hilo)


SMALL = dict(block_out=(64, 128, 512), layers_per_block=1)
# configuration, B, H, W: the shapes of the whole-model tests of tests/test_vae_model_backward_device.py
CASES = {"flux-1x16x24": ({}, 1, 16, 24), "small-2x16x24": (SMALL, 2, 16, 24)}
WEIGHTS = {"reconstruction": 1.0, "kl": 1e-2, "triplet": 1.0}
MARGIN, SIM, SEED, FIRST, N_LABELS, LATENT = 1.0, "cosine", 77, 3, 12, 16


def make_case(name, draw_eps, param_seed=5):
    """parameters, images, labels and the three CPU evaluations of a case.  draw_eps(B, L, h, w, draw) -> the fp32 eps tensor of that draw
    (the device's own).  param_seed: the synthetic weights' and images' seed (5 is the test's)."""
    from vae_tagger_amd import synth
    cfg, B, H, W = CASES[name]
    p = synth.synth_state_dict({**synth.encoder_manifest(**cfg), **synth.image_decoder_manifest(**cfg)}, seed=param_seed)
    images = synth.synth_images(3 * B, H, W, seed=param_seed + 1)
    g = torch.Generator().manual_seed(param_seed + 3)
    labels = tuple((torch.rand(B, N_LABELS, generator=g) < 0.5).float() for _ in range(2))
    labels[0][:, 0] = 1.0
    nb = len(cfg.get("block_out", synth.FLUX_BLOCK_OUT)) - 1
    eps = [draw_eps(B, LATENT, H >> nb, W >> nb, d) for d in range(4)]
    return dict(cfg=cfg, p=p, images=images, labels=labels, eps=eps, refs=step_refs(p, images, eps, labels, WEIGHTS, MARGIN, SIM))


def _sub(p, prefix):
    return {k: v for k, v in p.items() if k.startswith(prefix)}


def step_autograd(p, images, eps, labels, weights, margin, sim, bounds=None):
    """images [3B, 3, H, W] = [a; p; n], eps: draws 0, 1, 2, 3 as tensors [B, L, h, w], all of p's dtype -> (losses, grads keyed like p).  The plain
    step: z = mean + exp(0.5 clamp(logvar)) eps, nothing rounded.  bounds (optional dict) receives the gradient at every block boundary of both
    models ("encoder", "decoder") and at the decoded latent ("dz")."""
    q = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    B = images.shape[0] // 3
    moments, saved_e = encoder_forward_ref(_sub(q, "encoder."), images)
    z, kl = [], []
    for i, e in zip((0, 0, 1, 2), eps):
        m = moments[i * B:(i + 1) * B]
        mean, lc = m[:, :m.shape[1] // 2], torch.clamp(m[:, m.shape[1] // 2:], -30.0, 20.0)
        z.append(mean + torch.exp(0.5 * lc) * e)
        kl.append(0.5 * torch.sum(mean * mean + torch.exp(lc) - 1.0 - lc, dim=(1, 2, 3)))
    recon, saved_d = decoder_forward_ref(_sub(q, "decoder."), z[0])
    watched = {"encoder": saved_e["bounds"], "decoder": saved_d["bounds"], "dz": {"dz": z[0]}} if bounds is not None else {}
    for group in watched.values():
        for t in group.values():
            t.retain_grad()
    la, lp = (None, None) if labels is None else (labels[0].to(images.dtype), labels[1].to(images.dtype))
    total, parts = loss_ref.total_loss(z[1:], kl[1:], recon, images[:B], la, lp, weights, margin, sim)
    if bounds is None:
        grads = torch.autograd.grad(total, [q[k] for k in p])
    else:
        total.backward()
        grads = [q[k].grad for k in p]
        bounds.update({"encoder": {k: t.grad for k, t in watched["encoder"].items()}, "decoder": {k: t.grad for k, t in watched["decoder"].items()},
                       "dz": watched["dz"]["dz"].grad})
    return {k: v.detach() for k, v in dict(parts, total=total).items()}, dict(zip(p.keys(), grads))


def step_emulated(p, images, eps, labels, weights, margin, sim):
    """the device's arithmetic up to summation order: bf16 operands in both models, fp32 moments, z, reconstruction and gradients between them, the
    loss's gradient at the forward's fp32 z -> (grads keyed like p, dx at the block boundaries of both models)"""
    p64 = {k: v.double() for k, v in p.items()}
    enc, dec = _sub(p64, "encoder."), _sub(p64, "decoder.")
    f32 = lambda t: t.float().double()
    B = images.shape[0] // 3
    moments, saved_e = encoder_forward_ref(enc, images.double(), rnd=bf16_round_keep)
    moments = moments.float()
    m = [moments[i * B:(i + 1) * B].numpy() for i in range(3)]
    z0, _ = loss_ref.sample(moments[:B].double(), eps[0])
    recon, saved_d = decoder_forward_ref(dec, z0.detach(), rnd=bf16_round_keep, fold_rnd=bf16_round_keep)
    recon = recon.float()
    w_rec = float(weights.get("reconstruction", 0.0))
    d_recon = f32(w_rec * 2.0 / recon.numel() * (recon.double() - images[:B].double()))
    dz, g, at_d = decoder_backward_ref(dec, saved_d, d_recon, rnd=bf16_round_keep, fold_rnd=bf16_round_keep, split=split_hilo)
    la, lp = (None, None) if labels is None else (labels[0].numpy(), labels[1].numpy())
    out = loss_ref.autograd(m, [e.numpy() for e in eps[1:]], weights=weights, margin=margin, similarity_type=sim, dz_dec=dz.float().numpy(),
                            eps_dec=eps[0].numpy(), recon=recon.numpy(), target=images[:B].numpy(), labels_a=la, labels_p=lp)
    d_moments = f32(torch.cat([torch.from_numpy(d) for d in out["d_moments"]]))
    ge, at_e = encoder_backward_ref(enc, saved_e, d_moments, rnd=bf16_round_keep, split=split_hilo)
    g.update(ge)
    return {k: g[k] for k in p}, {"decoder": at_d, "encoder": at_e, "dz": dz}


def step_refs(p, images, eps, labels, weights, margin, sim):
    """-> dict(exact, f32, emu: gradients keyed like p; losses: the exact step's; emu_at)"""
    losses, g64 = step_autograd({k: v.double() for k, v in p.items()}, images.double(), [e.double() for e in eps], labels, weights, margin, sim)
    _, g32 = step_autograd(p, images, eps, labels, weights, margin, sim)
    ge, at = step_emulated(p, images, eps, labels, weights, margin, sim)
    return dict(exact=g64, f32=g32, emu=ge, losses=losses, emu_at=at)
