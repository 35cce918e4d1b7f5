"""Shared by the VAE loss tests: the reference's two latent losses written out in torch fp32, and the tolerance measured from them."""
import torch
import torch.nn.functional as F

from vae_tagger_amd import improved_losses as il

SIMS = ("cosine", "euclidean")


def _torch_fp32(fx, sim, labels):
    """The two losses written out in torch fp32 ops (the arithmetic the reference's training runs in) on the fixture's inputs."""
    a, p, n = (torch.from_numpy(fx[k]) for k in ("za", "zp", "zn"))
    la, lp = torch.from_numpy(fx["labels_a"]), torch.from_numpy(fx["labels_p"])
    if sim == "cosine":
        an = F.normalize(a, p=2, dim=1)
        pos, neg = 1 - (an * F.normalize(p, p=2, dim=1)).sum(1), 1 - (an * F.normalize(n, p=2, dim=1)).sum(1)
    else:
        pos, neg = F.pairwise_distance(a, p, p=2), F.pairwise_distance(a, n, p=2)
    trip = F.relu(pos - neg + 1.0)
    if labels:
        trip = trip * (1.0 + 0.5 * ((la * lp).sum(1) / (la.sum(1) + 1e-8)))
    s = (la * lp).sum(1) / ((la + lp - la * lp).sum(1) + 1e-8)
    m = s > 0.3
    con = (m.float() * pos ** 2 + (~m).float() * torch.clamp(1.0 - pos, min=0.0) ** 2) * torch.where(m, s, 1 - s)
    return float(trip.mean()), float(con.mean())


def measured_fp32_tolerance(fx):
    """4 x the largest distance of torch's fp32 result to the fp64 mirror on the fixture's inputs, per loss: the allowance for a
    comparison against the reference's fp32 outputs (the project's convention in the trainer tests)."""
    tol = {}
    for sim in SIMS:
        for labels in (True, False):
            t32, c32 = _torch_fp32(fx, sim, labels)
            la, lp = (fx["labels_a"], fx["labels_p"]) if labels else (None, None)
            t64 = il.triplet_elements(fx["za"], fx["zp"], fx["zn"], la, lp, 1.0, sim).mean()
            tol[f"triplet_{sim}_{'labels' if labels else 'nolabels'}"] = 4 * abs(t32 - t64)
        c64 = il.contrastive_elements(fx["za"], fx["zp"], fx["labels_a"], fx["labels_p"], 1.0, sim).mean()
        tol[f"contrastive_{sim}"] = 4 * abs(c32 - c64)
    return tol
