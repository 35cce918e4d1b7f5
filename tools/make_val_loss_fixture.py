"""Generate tests/golden/val_loss_reference.npz: inputs and the values the REFERENCE's own loss classes return for them.

    python tools/make_val_loss_fixture.py --reference /path/to/reference [--out tests/golden/val_loss_reference.npz]

Development machines only: it imports `improved_losses` from the reference checkout given on the command line (FocalLoss,
ClassBalancedLoss) and torch's nn.BCEWithLogitsLoss, runs them in fp32 and in fp64 and stores DATA only -- the logits (with +-0, +-30,
+-88, +-1e4 and denormals among them), fractional and 0/1 labels, a samples_per_class vector with every class populated, the float32
class-weight tensor ClassBalancedLoss builds, and the returned losses.  tests/test_val_loss_host.py holds the numpy mirrors to them."""
import argparse
import os
import sys

import numpy as np
import torch

FOCAL_PARAMS = ((1.0, 2.0), (0.25, 2.0), (1.0, 0.5), (1.0, 0.0))
ROWS, CLASSES = 24, 12


def inputs():
    rng = np.random.default_rng(20240917)
    x = (rng.standard_normal((ROWS, CLASSES)) * 3.0).astype(np.float32)
    extremes = np.array([0.0, -0.0, 30.0, -30.0, 88.0, -88.0, 1e4, -1e4, 1e-40, -1e-40, 1.4e-45, -1.4e-45], dtype=np.float32)
    for k, v in enumerate(extremes):                         # each extreme twice, spread over rows and classes
        x[(5 * k) % ROWS, k % CLASSES] = v
        x[(5 * k + 11) % ROWS, (k + 5) % CLASSES] = v
    y01 = (rng.random((ROWS, CLASSES)) < 0.3).astype(np.uint8)
    frac = rng.choice(np.array([0.25, 0.5, 0.75, 1.0], dtype=np.float32), size=(ROWS, CLASSES))
    yf = (y01 * frac).astype(np.float32)                     # the `tag:weight` floats of the JSON: 0 or a weight in (0, 1]
    samples = rng.integers(1, 5000, size=CLASSES).astype(np.float64)
    return x, yf, y01, samples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout (the directory that holds improved_losses.py)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                                                  "val_loss_reference.npz"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    import improved_losses as ref

    x, yf, y01, samples = inputs()
    out = {"logits": x, "labels_float": yf, "labels_u8": y01, "samples_per_class": samples,
           "focal_params": np.array(FOCAL_PARAMS, dtype=np.float64), "beta": np.float64(ref.ClassBalancedLoss().beta)}
    captured = []
    real_tensor = torch.tensor

    def capturing_tensor(*a, **k):                           # the float32 weight tensor ClassBalancedLoss.forward builds
        t = real_tensor(*a, **k)
        captured.append(t.detach().cpu().numpy().copy())
        return t
    for kind, labels in (("float", yf), ("u8", y01.astype(np.float32))):
        for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
            xt, yt = torch.from_numpy(x).to(dt), torch.from_numpy(labels).to(dt)
            out[f"bce_{kind}_{name}"] = np.float64(torch.nn.BCEWithLogitsLoss()(xt, yt).item())
            out[f"focal_{kind}_{name}"] = np.array([ref.FocalLoss(alpha=a, gamma=g)(xt, yt).item() for a, g in FOCAL_PARAMS], dtype=np.float64)
            torch.tensor = capturing_tensor
            try:
                out[f"class_balanced_{kind}_{name}"] = np.float64(ref.ClassBalancedLoss()(xt, yt, samples).item())
            finally:
                torch.tensor = real_tensor
        xt, yt = torch.from_numpy(x).double(), torch.from_numpy(labels).double()
        out[f"focal_elements_{kind}_f64"] = ref.FocalLoss(alpha=1.0, gamma=2.0, reduction="none")(xt, yt).numpy()
        out[f"bce_elements_{kind}_f64"] = torch.nn.functional.binary_cross_entropy_with_logits(xt, yt, reduction="none").numpy()
    assert captured and all(c.dtype == np.float32 and np.array_equal(c, captured[0]) for c in captured)
    out["class_balanced_weights_f32"] = captured[0]
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {os.path.getsize(args.out)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
