"""Where the whole-model backward's distance from fp64 autograd comes from: dx at every block boundary of the cases of
tests/test_vae_model_backward_device.py, from the device (encoder_backward / decoder_backward, boundaries=), from the fp64 restatement with the
device's operand roundings (tests/_vae_model_backward_ref.py) and from fp64 autograd of the unrounded model.  Per boundary, in the order the backward
reaches them: d_hip and d_emu (relative max-norm distances from the exact gradient) and their ratio; then the largest d_hip / d_emu over the
parameter gradients.  A ratio that grows gradually along the chain is rounding noise decorrelating between two evaluation orders; a jump at one stage
is a bug in that stage.

Usage: python tools/vae_backward_boundaries.py [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import _vae_model_backward_ref as R  # noqa: E402
from test_vae_model_backward_device import MODELS, _model_case  # noqa: E402
from vae_tagger_amd import vae_backward as vb  # noqa: E402

DEV = "cuda:0"


def exact_boundaries(kind, p, x, dy):
    q = {k: v.double().requires_grad_(True) for k, v in p.items()}
    y, saved = (R.encoder_forward_ref if kind == "encoder" else R.decoder_forward_ref)(q, x.double())
    for t in saved["bounds"].values():
        t.retain_grad()
    y.backward(dy.double())
    return {k: t.grad for k, t in saved["bounds"].items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    worst = 0.0
    for name in MODELS:
        c = _model_case(name)
        kind, r = c["kind"], c["refs"]
        p = {k: v.to(DEV).contiguous() for k, v in c["p"].items()}
        x, dy = c["x"].to(DEV), c["dy"].to(DEV)
        at = {}
        if kind == "encoder":
            _, saved = vb.encoder_forward_train(p, x)
            grads = vb.encoder_backward(p, saved, dy, boundaries=at)
        else:
            _, saved = vb.decoder_forward_train(p, x)
            _, grads = vb.decoder_backward(p, saved, dy, boundaries=at)
        torch.cuda.synchronize()
        exact = exact_boundaries(kind, c["p"], c["x"], c["dy"])
        say(f"{name}: dx at the block boundaries, in backward order")
        for k, t in at.items():
            got = t.cpu().permute(0, 3, 1, 2).double()
            scale = exact[k].abs().max()
            d_hip, d_emu = ((got - exact[k]).abs().max() / scale).item(), ((r["emu_at"][k] - exact[k]).abs().max() / scale).item()
            say(f"    {k:16s} d_hip {d_hip:.3e}  d_emu {d_emu:.3e}  d_hip / d_emu {d_hip / d_emu:.3f}")
        # (where the restatement IS the exact value -- the last layer's bias sum -- there is no ratio)
        ratios = sorted(((R.rel(grads[k].cpu(), r["exact"], k) / R.rel(r["emu"][k], r["exact"], k), k) for k in p if R.rel(r["emu"][k], r["exact"], k) > 0),
                        reverse=True)
        worst = max(worst, ratios[0][0])
        say(f"    parameter gradients: largest d_hip / d_emu {ratios[0][0]:.3f} ({ratios[0][1]}), then {ratios[1][0]:.3f}, {ratios[2][0]:.3f}; "
            f"median {ratios[len(ratios) // 2][0]:.3f}; smallest {ratios[-1][0]:.3f}")
    say(f"largest d_hip / d_emu over all cases: {worst:.3f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
