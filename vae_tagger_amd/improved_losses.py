"""The VAE's losses (improved_losses.py of the reference): ImprovedTripletLoss, ContrastiveLoss, SimplifiedCombinedLoss and CombinedLoss
with the reference's constructor arguments and forward signatures, evaluated on the device through a one-update accumulator
(vt_vae_loss_* of the C ABI; vae_losses.DeviceVAELossAccumulator).  Forward only: the returned 0-d tensors carry no graph.
AdaptiveLossWeights is not mirrored; use_adaptive_weights=True raises.

Host side: numpy fp64 mirrors of every formula and of the counter-based normal generator behind `posterior.sample_device()`.  They are
the tests' ground truth and need no GPU.
"""
import numpy as np

import torch

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
_GOLDEN, _ODD = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03
JACCARD_THRESHOLD = 0.3                      # the reference's hard-coded label-similarity threshold (improved_losses.py:29)


# ---- the generator (csrc/vt_vae_loss.h) -----------------------------------------------------------------------------------------------
def mix64(x):
    """vt_head_mix64 on uint64 arrays (wrapping arithmetic)."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def image_key(seed, draw, image):
    """The 64-bit key of one image's noise: mix64(mix64(seed + golden (draw + 1)) + odd (image + 1))."""
    stream = int(mix64((int(seed) + _GOLDEN * (int(draw) + 1)) & 0xFFFFFFFFFFFFFFFF))
    return int(mix64((stream + _ODD * (int(image) + 1)) & 0xFFFFFFFFFFFFFFFF))


def uniform_draws(seed, draw, image, n):
    """(u1, u2) fp64 [n] of the elements 0 .. n-1 of an image: u1 in (0, 1] -- it goes into the logarithm and is never 0 --, u2 in [0, 1)."""
    key = np.uint64(image_key(seed, draw, image))
    e = np.arange(int(n), dtype=np.uint64) * np.uint64(2)
    x1, x2 = mix64(key ^ e), mix64(key ^ (e + np.uint64(1)))
    u1 = ((x1 >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    u2 = (x2 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return u1, u2


def normal_draw(seed, draw, image, n):
    """The standard normals of an image's first n elements: Box-Muller in fp64, rounded to fp32 once -- what the device draws."""
    u1, u2 = uniform_draws(seed, draw, image, n)
    return (np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)).astype(np.float32)


# ---- the formulas, fp64 ---------------------------------------------------------------------------------------------------------------
def _split(moments):
    m = np.asarray(moments)
    c = m.shape[1] // 2
    mean = m[:, :c].astype(np.float64)
    with np.errstate(invalid="ignore"):
        logvar = np.clip(m[:, c:].astype(np.float64), -30.0, 20.0)      # (np.clip keeps a NaN)
    return mean, logvar


def sample_elements(moments, seed, draw=0, first_image=0):
    """posterior.sample_device() in fp64: (z, mean, std * eps), each [B, C, h, w]; eps is the fp32 draw of image first_image + b."""
    mean, logvar = _split(moments)
    b = mean.shape[0]
    d = int(np.prod(mean.shape[1:]))
    eps = np.stack([normal_draw(seed, draw, first_image + i, d) for i in range(b)]).astype(np.float64).reshape(mean.shape)
    noise = np.exp(0.5 * logvar) * eps
    return mean + noise, mean, noise


def kl_elements(moments):
    """posterior.kl() per image in fp64: 0.5 sum(mean^2 + var - 1 - logvar) with the logvar clamped to [-30, 20]."""
    mean, logvar = _split(moments)
    sd = np.exp(0.5 * logvar)
    return 0.5 * (mean * mean + sd * sd - 1.0 - logvar).reshape(mean.shape[0], -1).sum(1)


def _rows(x):
    x = np.asarray(x)
    return x.reshape(x.shape[0], -1).astype(np.float64)


def distance_elements(a, b, similarity_type="cosine"):
    """Per row: 1 - a.b / (max(|a|, 1e-12) max(|b|, 1e-12)) (F.normalize's clamp), or |a - b + 1e-6| (F.pairwise_distance's eps)."""
    a, b = _rows(a), _rows(b)
    if similarity_type == "cosine":
        na = np.maximum(np.sqrt((a * a).sum(1)), 1e-12)
        nb = np.maximum(np.sqrt((b * b).sum(1)), 1e-12)
        with np.errstate(invalid="ignore"):                              # (a non-finite latent gives a non-finite distance, as in torch)
            return 1.0 - (a * b).sum(1) / (na * nb)
    d = a - b + 1e-6
    return np.sqrt((d * d).sum(1))


def label_sums(labels_a, labels_p):
    """(sum labels_a, overlap, union) per row; fp32 labels are used as their value, uint8 / bool labels are 0 or 1."""
    def as64(y):
        y = np.asarray(y)
        return (y != 0).astype(np.float64) if y.dtype in (np.uint8, np.bool_) else y.astype(np.float64)
    la, lp = as64(labels_a), as64(labels_p)
    return la.sum(1), (la * lp).sum(1), (la + lp - la * lp).sum(1)


def triplet_weight(labels_a=None, labels_p=None, rows=None):
    """1 + 0.5 overlap / (sum labels_a + 1e-8); 1 without labels."""
    if labels_a is None or labels_p is None:
        return np.ones(rows)
    sa, ov, _ = label_sums(labels_a, labels_p)
    return 1.0 + 0.5 * (ov / (sa + 1e-8))


def triplet_margin_elements(a, p, n, margin=1.0, similarity_type="cosine"):
    """pos - neg + margin per row: what the hinge is applied to."""
    return distance_elements(a, p, similarity_type) - distance_elements(a, n, similarity_type) + float(margin)


def triplet_elements(a, p, n, labels_a=None, labels_p=None, margin=1.0, similarity_type="cosine"):
    """ImprovedTripletLoss per row (improved_losses.py:81-103) before the mean."""
    x = triplet_margin_elements(a, p, n, margin, similarity_type)
    hinge = np.where(x <= 0.0, 0.0, x)                                   # (a NaN stays)
    return hinge * triplet_weight(labels_a, labels_p, len(hinge))


def contrastive_elements(a, p, labels_a=None, labels_p=None, margin=1.0, similarity_type="cosine", threshold=JACCARD_THRESHOLD):
    """ContrastiveLoss per row (improved_losses.py:13-36) before the mean; without labels every pair is dissimilar with weight 1."""
    d = distance_elements(a, p, similarity_type)
    if labels_a is None or labels_p is None:
        ov = un = np.zeros(len(d))
    else:
        _, ov, un = label_sums(labels_a, labels_p)
    sim = ov / (un + 1e-8)
    similar = (sim > threshold).astype(np.float64)
    gap = float(margin) - d
    gap = np.where(gap <= 0.0, 0.0, gap)
    return (similar * (d * d) + (1.0 - similar) * (gap * gap)) * np.where(sim > threshold, sim, 1.0 - sim)


def mse_elements(recon, target):
    """Per image: mean (recon - target)^2."""
    d = _rows(recon) - _rows(target)
    return (d * d).mean(1)


def kl_log(kl_mean):
    """CombinedLoss' stabilised KL: log(1 + kl_mean / 10000)."""
    return np.log1p(np.asarray(kl_mean, dtype=np.float64) / 10000.0)


# ---- the reference's classes on the device ------------------------------------------------------------------------------------------
def _flat(z):
    return z.detach().reshape(z.size(0), -1)


def _one_update(za, zp, zn=None, labels_a=None, labels_p=None, recon=None, target=None, moments=None, triplet_margin=1.0,
                contrastive_margin=1.0):
    """One vt_vae_loss_update on the latents' device: the block's per-batch components as a float64 device tensor [7]."""
    from .vae_losses import DeviceVAELossAccumulator
    za = _flat(za)
    acc = DeviceVAELossAccumulator(za.device, triplet_margin, contrastive_margin)
    m = moments or (None, None, None)
    acc.update(anchor=(m[0], za, 0), positive=(m[1], _flat(zp), 0), negative=None if zn is None else (m[2], _flat(zn), 0),
               recon=recon, target=target, labels_a=labels_a, labels_p=labels_p)
    return acc.device_components()


_K = {"mse": 0, "kl_mean": 1, "kl_log": 2, "triplet_cosine": 3, "triplet_euclidean": 4, "contrastive_cosine": 5, "contrastive_euclidean": 6}


def _sim(similarity_type):
    return "cosine" if similarity_type == "cosine" else "euclidean"


def _classification(logits, targets, use_focal, alpha, gamma, use_class_balanced, samples_per_class):
    """The classification term through the existing DeviceLossAccumulator: a 0-d float64 device tensor."""
    from . import losses
    x = logits.detach()
    w = losses.class_balanced_weights(samples_per_class) if use_class_balanced and samples_per_class is not None else None
    acc = losses.DeviceLossAccumulator(x.shape[1], x.device, alpha, gamma, w)
    acc.update(x, targets)
    sums = acc.export_state().data[losses.state_layout(x.shape[1])["totals"]:][:24].view(torch.float64)
    return sums[2] if w is not None else (sums[1] if use_focal else sums[0])


class ContrastiveLoss(torch.nn.Module):
    def __init__(self, margin=1.0, similarity_type="cosine"):
        super().__init__()
        self.margin, self.similarity_type = margin, similarity_type

    def forward(self, embedding1, embedding2, labels1, labels2):
        c = _one_update(embedding1, embedding2, None, labels1, labels2, contrastive_margin=self.margin)
        return c[_K["contrastive_" + _sim(self.similarity_type)]]


class ImprovedTripletLoss(torch.nn.Module):
    def __init__(self, margin=1.0, similarity_type="cosine"):
        super().__init__()
        self.margin, self.similarity_type = margin, similarity_type

    def forward(self, anchor, positive, negative, anchor_labels=None, positive_labels=None):
        both = anchor_labels is not None and positive_labels is not None
        c = _one_update(anchor, positive, negative, anchor_labels if both else None, positive_labels if both else None, triplet_margin=self.margin)
        return c[_K["triplet_" + _sim(self.similarity_type)]]


class SimplifiedCombinedLoss(torch.nn.Module):
    def __init__(self, classification_weight=1.0, triplet_weight=0.5, contrastive_weight=0.0, use_focal_loss=True, use_class_balanced=False,
                 use_contrastive=False, focal_alpha=1.0, focal_gamma=2.0, triplet_margin=1.0, contrastive_margin=1.0, similarity_type="cosine"):
        super().__init__()
        self.classification_weight, self.triplet_weight, self.contrastive_weight = classification_weight, triplet_weight, contrastive_weight
        self.use_contrastive, self.use_focal_loss, self.use_class_balanced = use_contrastive, use_focal_loss, use_class_balanced
        self.focal_alpha, self.focal_gamma = focal_alpha, focal_gamma
        if use_contrastive:
            self.contrastive_loss_fn = ContrastiveLoss(contrastive_margin, similarity_type)
        else:
            self.triplet_loss_fn = ImprovedTripletLoss(triplet_margin, similarity_type)

    def forward(self, z_a, z_p, z_n=None, classification_logits=None, classification_targets=None, anchor_labels=None, positive_labels=None,
                negative_labels=None, samples_per_class=None):
        loss_dict, total = {}, 0
        if self.use_contrastive and self.contrastive_weight > 0:
            loss_dict["contrastive_loss"] = self.contrastive_loss_fn(z_a, z_p, anchor_labels, positive_labels)
            total = total + self.contrastive_weight * loss_dict["contrastive_loss"]
        elif self.triplet_weight > 0:
            loss_dict["triplet_loss"] = self.triplet_loss_fn(z_a, z_p, z_n, anchor_labels, positive_labels)
            total = total + self.triplet_weight * loss_dict["triplet_loss"]
        if classification_logits is not None and classification_targets is not None:
            loss_dict["classification_loss"] = _classification(classification_logits, classification_targets, self.use_focal_loss, self.focal_alpha,
                                                               self.focal_gamma, self.use_class_balanced, samples_per_class)
            total = total + self.classification_weight * loss_dict["classification_loss"]
        loss_dict["total_loss"] = total
        loss_dict["weights"] = torch.tensor([self.contrastive_weight if self.use_contrastive else self.triplet_weight, self.classification_weight])
        return loss_dict


class CombinedLoss(torch.nn.Module):
    def __init__(self, reconstruction_weight=0.01, kl_weight=1e-2, triplet_weight=1.0, classification_weight=1.0, use_focal_loss=True,
                 use_class_balanced=False, use_adaptive_weights=False, focal_alpha=1.0, focal_gamma=2.0, triplet_margin=1.0, similarity_type="cosine"):
        super().__init__()
        if use_adaptive_weights:
            raise NotImplementedError("AdaptiveLossWeights holds trained parameters and is not mirrored: use_adaptive_weights=True is not supported")
        self.reconstruction_weight, self.kl_weight = reconstruction_weight, kl_weight
        self.triplet_weight, self.classification_weight = triplet_weight, classification_weight
        self.use_focal_loss, self.use_class_balanced, self.focal_alpha, self.focal_gamma = use_focal_loss, use_class_balanced, focal_alpha, focal_gamma
        self.use_adaptive_weights = False
        self.triplet_loss_fn = ImprovedTripletLoss(triplet_margin, similarity_type)

    def forward(self, reconstruction, target_images, posterior_a, posterior_p, posterior_n, z_a, z_p, z_n, classification_logits,
                classification_targets, anchor_labels=None, positive_labels=None, samples_per_class=None):
        both = anchor_labels is not None and positive_labels is not None
        c = _one_update(z_a, z_p, z_n, anchor_labels if both else None, positive_labels if both else None, reconstruction, target_images,
                        (posterior_a.parameters, posterior_p.parameters, posterior_n.parameters), triplet_margin=self.triplet_loss_fn.margin)
        loss_dict = {"reconstruction_loss": c[_K["mse"]], "kl_loss": c[_K["kl_log"]],
                     "triplet_loss": c[_K["triplet_" + _sim(self.triplet_loss_fn.similarity_type)]],
                     "classification_loss": _classification(classification_logits, classification_targets, self.use_focal_loss, self.focal_alpha,
                                                            self.focal_gamma, self.use_class_balanced, samples_per_class)}
        loss_dict["total_loss"] = (self.reconstruction_weight * loss_dict["reconstruction_loss"] + self.kl_weight * loss_dict["kl_loss"]
                                   + self.triplet_weight * loss_dict["triplet_loss"] + self.classification_weight * loss_dict["classification_loss"])
        loss_dict["weights"] = torch.tensor([self.reconstruction_weight, self.kl_weight, self.triplet_weight, self.classification_weight])
        return loss_dict
