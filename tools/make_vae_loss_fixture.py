"""Writes tests/golden/vae_loss_reference.npz: small inputs and what the REFERENCE's own ImprovedTripletLoss / ContrastiveLoss return
for them (fp32 as its training runs, and the same classes on float64 tensors), both similarity types, with and without labels.

    python tools/make_vae_loss_fixture.py --reference /path/to/the/reference/checkout

Run once on a CPU; the reference is imported from the directory given, nothing of it is copied.  B = 5, D = 96, N = 7.  Rows: 0 and 4
ordinary, 1 with the hinge inactive for both similarity types (positive next to the anchor, negative opposite and far), 2 with
positive == anchor, 3 an all-zero anchor (F.normalize's 1e-12 clamp)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="directory holding the reference's improved_losses.py")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "vae_loss_reference.npz"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    import improved_losses as ref

    rng = np.random.default_rng(20240915)
    B, D, N = 5, 96, 7
    za = rng.standard_normal((B, D)).astype(np.float32)
    zp = (za + 0.8 * rng.standard_normal((B, D))).astype(np.float32)
    zn = rng.standard_normal((B, D)).astype(np.float32)
    zp[1] = za[1] + np.float32(0.01) * rng.standard_normal(D).astype(np.float32)
    zn[1] = np.float32(-3.0) * za[1]
    zp[2] = za[2]
    za[3] = 0.0
    la = (rng.random((B, N)) < 0.5).astype(np.float32)
    lp = (rng.random((B, N)) < 0.5).astype(np.float32)
    la[0], lp[0] = [1, 1, 0, 0, 1, 0, 0], [1, 1, 0, 0, 1, 0, 0]          # identical: similar pair
    la[1], lp[1] = [1, 0, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0, 1]          # disjoint
    la[3] = 0.0                                                          # an anchor without labels: the 1e-8 in the weight
    la[4], lp[4] = [0.5, 1, 0, 0.25, 0, 0, 1], [1, 0.75, 0, 0, 0, 1, 1]  # fractional `tag:weight` labels
    out = {"za": za, "zp": zp, "zn": zn, "labels_a": la, "labels_p": lp, "margin": np.float64(1.0)}
    for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        t = lambda a: torch.from_numpy(a).to(dt)
        for sim in ("cosine", "euclidean"):
            trip = ref.ImprovedTripletLoss(margin=1.0, similarity_type=sim)
            con = ref.ContrastiveLoss(margin=1.0, similarity_type=sim)
            out[f"triplet_{sim}_labels_{tag}"] = trip(t(za), t(zp), t(zn), t(la), t(lp)).numpy()
            out[f"triplet_{sim}_nolabels_{tag}"] = trip(t(za), t(zp), t(zn)).numpy()
            out[f"contrastive_{sim}_{tag}"] = con(t(za), t(zp), t(la), t(lp)).numpy()
    np.savez(args.out, **out)
    for k, v in out.items():
        if v.ndim == 0:
            print(k, float(v))


if __name__ == "__main__":
    main()
