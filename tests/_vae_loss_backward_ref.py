"""The training loss of the VAE restated in torch fp64, for autograd (train_vae.py:131-179 of the reference with improved_losses.py's
CombinedLoss / ImprovedTripletLoss):

    total = w_rec mse_loss(recon, anchor) + w_kl log(1 + kl_mean / 10000) + w_tri triplet(z_a, z_p, z_n, labels_a, labels_p)

It is the loss the device evaluates, roundings included: the forward forms z = mean + fp32(std) eps in fp32 and sums it in fp64,
and the gradient is defined at THAT z with d z / d logvar = 0.5 fp32(std) eps.  Two roundings are therefore restated with
their value and their derivative apart:
    std  = fp32(exp(0.5 lc)) * exp(0.5 (lc - lc.detach()))      value fp32(std), derivative 0.5 fp32(std) (and 0 outside the clamp)
    z    = z64 + (z32 - z64).detach()                            value the forward's fp32 z, derivative that of mean + std eps
Everything else is plain fp64 torch: F.normalize (eps 1e-12), F.pairwise_distance (eps 1e-6), F.relu, torch.clamp, F.mse_loss.
"""
import numpy as np
import torch
import torch.nn.functional as F

from vae_tagger_amd.vae_losses import forward_z


def sample(moments, eps, z_forward=None):
    """moments fp64 [B, 2C, ...] (leaf), eps fp32 values [B, C, ...], z_forward: the forward's fp32 z (the device's own, from
    vt_posterior_sample; None: vae_losses.forward_z's model of it) -> (z, kl per image), differentiable in the moments"""
    mean, logvar = torch.chunk(moments, 2, dim=1)
    lc = torch.clamp(logvar, -30.0, 20.0)
    sd = torch.exp(0.5 * lc)
    std32 = sd.detach().to(torch.float32)
    e32 = eps.to(torch.float32)
    std = std32.to(torch.float64) * torch.exp(0.5 * (lc - lc.detach()))
    z64 = mean + std * e32.to(torch.float64)
    if z_forward is None:
        z32 = torch.from_numpy(forward_z(mean.detach().numpy(), std32.numpy(), e32.numpy())).to(torch.float64)
    else:
        z32 = torch.as_tensor(np.asarray(z_forward)).to(torch.float64).reshape(mean.shape)
    z = z64 + (z32 - z64).detach()
    kl = 0.5 * torch.sum(mean * mean + sd * sd - 1.0 - lc, dim=tuple(range(1, moments.dim())))
    return z, kl


def triplet(za, zp, zn, labels_a, labels_p, margin, similarity_type):
    a, p, n = (t.reshape(t.shape[0], -1) for t in (za, zp, zn))
    if similarity_type == "cosine":
        a, p, n = F.normalize(a, p=2, dim=1), F.normalize(p, p=2, dim=1), F.normalize(n, p=2, dim=1)
        pos, neg = 1 - (a * p).sum(1), 1 - (a * n).sum(1)
    else:
        pos, neg = F.pairwise_distance(a, p, p=2), F.pairwise_distance(a, n, p=2)
    loss = F.relu(pos - neg + margin)
    if labels_a is not None and labels_p is not None:
        overlap = (labels_a * labels_p).sum(1)
        loss = loss * (1.0 + 0.5 * (overlap / (labels_a.sum(1) + 1e-8)))
    return loss.mean()


def total_loss(z, kl, recon, target, labels_a, labels_p, weights, margin, similarity_type):
    """z, kl: three each.  -> (total, {reconstruction, kl, triplet})"""
    w_rec, w_kl, w_tri = (float(weights.get(k, 0.0)) for k in ("reconstruction", "kl", "triplet"))
    rec = F.mse_loss(recon, target) if recon is not None else torch.zeros((), dtype=torch.float64)
    kl_mean = ((kl[0] + kl[1] + kl[2]) / 3.0).mean()
    kl_log = torch.log(1 + kl_mean / 10000.0)
    tri = triplet(z[0], z[1], z[2], labels_a, labels_p, margin, similarity_type)
    return w_rec * rec + w_kl * kl_log + w_tri * tri, {"reconstruction": rec, "kl": kl_log, "triplet": tri}


def _t64(x, grad=False):
    return None if x is None else torch.as_tensor(np.asarray(x, dtype=np.float64)).clone().requires_grad_(grad)


def autograd(moments, eps, *, weights, margin=1.0, similarity_type="cosine", dz_dec=None, eps_dec=None, recon=None, target=None,
             labels_a=None, labels_p=None, z_forward=None):
    """moments: three fp32 arrays [B, 2C, h, w]; eps: the three streams' fp32 draws [B, C, h, w]; dz_dec with eps_dec: the gradient arriving
    at the latent decoded from the anchor's moments under eps_dec (it enters as the linear term sum(dz_dec z_dec)); z_forward: the three
    streams' z as the device's forward formed them.
    -> {"d_moments": [3 fp64 arrays], "d_recon", "losses": [reconstruction, kl, triplet, total]}"""
    m = [_t64(x, True) for x in moments]
    z, kl = zip(*(sample(mi, torch.as_tensor(np.asarray(e)), zf) for mi, e, zf in zip(m, eps, z_forward or (None,) * 3)))
    r, t = _t64(recon, recon is not None), _t64(target)
    la = None if labels_a is None else _t64((np.asarray(labels_a) != 0) if np.asarray(labels_a).dtype in (np.uint8, np.bool_) else labels_a)
    lp = None if labels_p is None else _t64((np.asarray(labels_p) != 0) if np.asarray(labels_p).dtype in (np.uint8, np.bool_) else labels_p)
    total, parts = total_loss(z, kl, r, t, la, lp, weights, margin, similarity_type)
    objective = total
    if dz_dec is not None:
        z_dec, _ = sample(m[0], torch.as_tensor(np.asarray(eps_dec)))
        objective = objective + (_t64(dz_dec) * z_dec).sum()
    objective.backward()
    zero = lambda x: np.zeros(tuple(x.shape))
    return {"d_moments": [mi.grad.numpy() if mi.grad is not None else zero(mi) for mi in m],
            "d_recon": None if r is None else (r.grad.numpy() if r.grad is not None else zero(r)),
            "losses": np.array([float(v.detach()) for v in (parts["reconstruction"], parts["kl"], parts["triplet"], total)])}


def make_case(B, C, h, w, H=0, W=0, n_labels=0, seed=0, labels_dtype=np.float32):
    """Random inputs of one call: moments of a plausible scale (|mean| ~ 1, logvar ~ -1 +- 1), images in [0, 1], sparse labels"""
    rng = np.random.default_rng(seed)
    case = {"moments": [np.concatenate([rng.normal(0.0, 1.0, (B, C, h, w)), rng.normal(-1.0, 1.0, (B, C, h, w))], 1).astype(np.float32) for _ in range(3)],
            "dz_dec": (rng.normal(0.0, 1.0, (B, C, h, w)) * 1e-3).astype(np.float32), "recon": None, "target": None, "labels_a": None, "labels_p": None}
    if H:
        case["recon"], case["target"] = (rng.random((B, 3, H, W)).astype(np.float32) for _ in range(2))
    if n_labels:
        la, lp = (rng.random((B, n_labels)) < 0.4 for _ in range(2))
        la[:, 0] = True
        case["labels_a"], case["labels_p"] = la.astype(labels_dtype), lp.astype(labels_dtype)
    return case


def bound_fp32_store(ref):
    """|d - ref| <= 2^-23 |ref| + 2^-40 max|ref| per element: fp64 arithmetic and one rounding to fp32 give half of the first term, the
    second covers the cancellation between the sampled and the KL part of d logvar"""
    ref = np.abs(np.asarray(ref, dtype=np.float64))
    return 2.0 ** -23 * ref + 2.0 ** -40 * (ref.max() if ref.size else 0.0)
