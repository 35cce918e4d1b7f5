"""Where the joined train step's distance from fp64 autograd comes from: dx at every block boundary of both models and at the decoded latent, for the
cases of tests/test_vae_train_step_device.py, from the device (vae_loss_and_grads, boundaries=), from the fp64 restatement with the device's roundings
(tests/_vae_train_step_ref.py) and from fp64 autograd of the unrounded step.  Per boundary, in the order the backward reaches them: d_hip and d_emu
(relative max-norm distances from the exact gradient) and their ratio; then the largest d_hip / d_emu over the parameter gradients.  A ratio that
wanders is rounding noise decorrelating between two evaluations; a jump at one stage is a bug in that stage (DESIGN.md sections 4.23 and 4.24).

Usage: python tools/vae_train_step_boundaries.py [--param-seed N] [--out FILE]     (--param-seed: other synthetic weights, images and labels than the test's 5)"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import _vae_model_backward_ref as R  # noqa: E402
import _vae_train_step_ref as T  # noqa: E402
from vae_tagger_amd import vae_backward as vb  # noqa: E402

DEV = "cuda:0"


def device_eps(B, L, h, w, draw):
    """the device's own draw: vt_posterior_sample on all-zero moments has std exactly 1, so z is eps"""
    zero, z = torch.zeros(B, 2 * L, h, w, device=DEV), torch.empty(B, L, h, w, device=DEV)
    vb.context(DEV).call("vt_posterior_sample", ctypes.c_void_p(zero.data_ptr()), B, L, h * w, T.SEED, draw, T.FIRST, ctypes.c_void_p(z.data_ptr()), None, None)
    torch.cuda.synchronize()
    return z.cpu()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--param-seed", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    worst = 0.0
    for name in T.CASES:
        c = T.make_case(name, device_eps, a.param_seed)
        r = c["refs"]
        p = {k: v.to(DEV).contiguous() for k, v in c["p"].items()}
        B = c["images"].shape[0] // 3
        x = [c["images"][i * B:(i + 1) * B].to(DEV).contiguous() for i in range(3)]
        la, lp = (y.to(DEV) for y in c["labels"])
        at = {}
        _, grads = vb.vae_loss_and_grads(p, *x, la, lp, weights=T.WEIGHTS, margin=T.MARGIN, similarity_type=T.SIM, seed=T.SEED, first_image=T.FIRST,
                                         boundaries=at)
        torch.cuda.synchronize()
        eps = [e.double() for e in c["eps"]]
        exact = {}
        T.step_autograd({k: v.double() for k, v in c["p"].items()}, c["images"].double(), eps, c["labels"], T.WEIGHTS, T.MARGIN, T.SIM, bounds=exact)
        say(f"{name} (parameter seed {a.param_seed}): dx at the block boundaries, in backward order")
        stages = [("decoder", k, at["decoder"][k].cpu().permute(0, 3, 1, 2)) for k in at["decoder"]] + [("dz", "dz", at["dz"].cpu())]
        stages += [("encoder", k, at["encoder"][k].cpu().permute(0, 3, 1, 2)) for k in at["encoder"]]
        for model, k, got in stages:
            ex = exact[model] if model == "dz" else exact[model][k]
            em = r["emu_at"][model] if model == "dz" else r["emu_at"][model][k]
            scale = ex.abs().max()
            d_hip, d_emu = ((got.double() - ex).abs().max() / scale).item(), ((em - ex).abs().max() / scale).item()
            say(f"    {model + ' ' + k:28s} d_hip {d_hip:.3e}  d_emu {d_emu:.3e}  d_hip / d_emu {d_hip / d_emu:.3f}")
        ratios = sorted(((R.rel(grads[k].cpu(), r["exact"], k) / R.rel(r["emu"][k], r["exact"], k), k) for k in p if R.rel(r["emu"][k], r["exact"], k) > 0),
                        reverse=True)
        worst = max(worst, ratios[0][0])
        say(f"    parameter gradients: largest d_hip / d_emu {ratios[0][0]:.3f} ({ratios[0][1]}), then {ratios[1][0]:.3f} ({ratios[1][1]}), "
            f"{ratios[2][0]:.3f} ({ratios[2][1]}), {ratios[3][0]:.3f}; median {ratios[len(ratios) // 2][0]:.3f}; smallest {ratios[-1][0]:.3f}")
    say(f"largest d_hip / d_emu over all cases: {worst:.3f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
