"""GPU: the classifier-head trainer (vt_head_*, csrc/train_head.hip) against torch on the CPU in fp64.

The rule of every parity check: the same computation also runs with torch in fp32 on the CPU; its deviation from the fp64 result,
e32 = max |d| / max |ref| per tensor, is the yardstick, and the device must be within 4 x max(e32, 1e-7) per tensor (the factor covers
the different summation order).  Every check prints its ratio device / max(e32, 1e-7) before it asserts.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vae_tagger_amd import _lib, synth
from vae_tagger_amd.losses import class_balanced_weights
from vae_tagger_amd.train import HeadTrainer, lr_schedule

from _util import latent_input

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR, FACTOR = 1e-7, 4.0


# ---- the torch head and the losses (losses.py's definitions) -------------------------------------------------------------------------
def hidden_count(plain):
    return 2 if plain else 3


def head_params(sd, dtype, grad=True):
    return {k: v.detach().to(dtype).clone().requires_grad_(grad) for k, v in sd.items() if k.startswith("classifier.")}


def head_forward(p, x, plain, masks=None, rates=None):
    nh = hidden_count(plain)
    for i in range(nh):
        x = F.linear(x, p[f"classifier.{4 * i}.weight"], p[f"classifier.{4 * i}.bias"])
        x = F.layer_norm(x, x.shape[-1:], p[f"classifier.{4 * i + 1}.weight"], p[f"classifier.{4 * i + 1}.bias"], 1e-5)
        x = F.leaky_relu(x, 0.2) if plain else F.relu(x)
        if masks is not None:
            x = x * masks[i].to(x.dtype) * (1.0 / (1.0 - rates[i]))
    return F.linear(x, p[f"classifier.{4 * nh}.weight"], p[f"classifier.{4 * nh}.bias"])


def loss_fn(kind, logits, y, alpha=1.0, gamma=2.0, weights=None):
    bce = F.binary_cross_entropy_with_logits(logits, y, reduction="none")
    if kind == "focal":
        return (alpha * (1.0 - torch.exp(-bce)) ** gamma * bce).mean()
    if kind == "class_balanced":
        return (bce * weights.to(bce.dtype)[None, :]).mean()
    return bce.mean()


def torch_grads(sd, plain, dtype, x, y, kind, kw, masks=None, rates=None, scale=1.0):
    p = head_params(sd, dtype)
    loss = loss_fn(kind, head_forward(p, x.to(dtype), plain, masks, rates), y.to(dtype), **kw) * scale
    loss.backward()
    return loss.detach(), {k: v.grad for k, v in p.items()}


def rel(a, ref):
    ref = ref.double()
    return ((a.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def check(name, dev, r64, r32):
    """The rule for one tensor; returns the ratio device / yardstick."""
    e32 = max(rel(r32, r64), FLOOR)
    ratio = rel(dev, r64) / e32
    print(f"    {name}: device/e32 = {ratio:.3f} (e32 {e32:.2e})")
    assert ratio <= FACTOR, f"{name}: device error is {ratio:.2f} x the fp32 yardstick {e32:.2e}"
    return ratio


# ---- decoders ------------------------------------------------------------------------------------------------------------------------
_DECODERS = {}


def decoder(plain, N, seed=1):
    key = (plain, N, seed)
    if key not in _DECODERS:
        from vae_tagger_amd.modules import AttentionClassificationDecoder, ClassificationDecoder
        if plain:
            d = ClassificationDecoder(16, 16, 16, N)
            sd = synth.synth_state_dict(synth.plain_decoder_manifest(N), seed=seed)
        else:
            d = AttentionClassificationDecoder(16, 16, 16, N)
            sd = synth.synth_state_dict(synth.attention_decoder_manifest(N), seed=seed)
        d.load_state_dict(sd, strict=False)
        _DECODERS[key] = (d.to(DEV).eval(), sd)
    return _DECODERS[key]


def batch(plain, N, B, seed, labels="u8"):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 256 if plain else 512, generator=g)
    on = torch.rand(B, N, generator=g) < 0.3
    if labels == "u8":
        return x, on.to(torch.uint8)
    return x, on.float() * (0.05 + 0.95 * torch.rand(B, N, generator=g))


def uneven_weights(N):
    return torch.from_numpy(class_balanced_weights(1.0 + (np.arange(N) * 37 % 101) ** 2))


def all_gradients(tr):
    return {k: tr.gradient(k) for k in tr.shapes}


LOSSES = [("bce", {}), ("focal", {"alpha": 0.25, "gamma": 2.0}), ("focal", {"alpha": 1.0, "gamma": 1.5}), ("class_balanced", {})]


def make_trainer(dec, kind, kw, N, dropout=None, seed=0):
    return HeadTrainer(dec, loss=kind, focal_alpha=kw.get("alpha", 1.0), focal_gamma=kw.get("gamma", 2.0),
                       class_weights=uneven_weights(N) if kind == "class_balanced" else None, dropout=dropout, seed=seed)


# ---- 1. the split is exact -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plain", [True, False], ids=["plain", "attention"])
@pytest.mark.parametrize("hw", [(16, 16), (9, 20)])
@pytest.mark.parametrize("B", [1, 3, 9])
def test_features_then_head_equals_decode_logits(plain, hw, B):
    dec, _ = decoder(plain, 11)
    tr = HeadTrainer(dec)
    lat = latent_input((B, 16, *hw), seed=3 + B).to(DEV)
    whole = dec(lat)
    feats = tr.features(lat)
    assert feats.shape == (B, 256 if plain else 512)
    split = tr.forward(feats)
    torch.cuda.synchronize()
    assert torch.equal(whole, split)


# ---- 2. gradients --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plain", [True, False], ids=["plain", "attention"])
@pytest.mark.parametrize("N", [11, 70, 1000])
@pytest.mark.parametrize("B", [1, 3, 9])
def test_gradients_match_autograd(plain, N, B):
    dec, sd = decoder(plain, N)
    worst = 0.0
    for kind, kw in LOSSES:
        tkw = dict(kw, weights=uneven_weights(N)) if kind == "class_balanced" else kw
        for labels in ("u8", "f32"):
            print(f"  {kind} {kw} labels {labels}")
            x, y = batch(plain, N, B, seed=N + B, labels=labels)
            tr = make_trainer(dec, kind, kw, N)
            tr.forward_backward(x, y, train=False, step=5)
            l64, g64 = torch_grads(sd, plain, torch.float64, x, y, kind, tkw)
            l32, g32 = torch_grads(sd, plain, torch.float32, x, y, kind, tkw)
            worst = max(worst, check("loss", tr.losses()[5], l64, l32))
            dev = all_gradients(tr)
            for k in dev:
                worst = max(worst, check(k, dev[k], g64[k], g32[k]))
    print(f"gradients {'plain' if plain else 'attention'} N={N} B={B}: worst device/e32 = {worst:.3f}")


@pytest.mark.parametrize("plain", [True, False], ids=["plain", "attention"])
@pytest.mark.parametrize("B", [17, 40, 64])
def test_gradients_beyond_one_pass_of_the_backward_kernel(plain, B):
    """B > 16: head_linear_bwd_kernel walks its weight rows once per 16 batch rows, adding into the gradient on every pass and taking
    the squared norm on the last; 17 leaves a pass of one row, 40 a pass of eight, 64 is four full passes.  Dropout on."""
    N = 70
    dec, sd = decoder(plain, N)
    rates = (0.3, 0.2) if plain else (0.3, 0.2, 0.1)
    x, y = batch(plain, N, B, seed=100 + B, labels="f32")
    tr = make_trainer(dec, "focal", {"alpha": 1.0, "gamma": 0.5}, N, dropout=rates, seed=3)
    masks = [m.cpu() for m in tr.forward_backward(x, y, train=True, step=2, return_masks=True)]
    kw = {"alpha": 1.0, "gamma": 0.5}
    l64, g64 = torch_grads(sd, plain, torch.float64, x, y, "focal", kw, masks, rates)
    l32, g32 = torch_grads(sd, plain, torch.float32, x, y, "focal", kw, masks, rates)
    check("loss", tr.losses()[2], l64, l32)
    dev = all_gradients(tr)
    for k in dev:
        check(k, dev[k], g64[k], g32[k])
    norm64 = math.sqrt(sum((g.double() ** 2).sum().item() for g in dev.values()))
    tr.clip(1e9)
    assert abs(tr.grad_norm()[0] - norm64) <= 1e-6 * norm64


def test_focal_gamma_below_one_stays_finite_on_saturated_logits():
    """bce == 0 in fp64 (a saturated logit with the right label) makes u = 0 and u^(gamma - 1) infinite: the gradient there is 0."""
    N = 11
    dec, sd = decoder(True, N, seed=4)                        # (a decoder of its own: commit changes its device tables)
    tr = make_trainer(dec, "focal", {"alpha": 1.0, "gamma": 0.5}, N)
    big = torch.zeros(N)
    big[0], big[1] = 800.0, -800.0
    tr.write(_lib.HEAD_PARAM, "classifier.8.bias", sd["classifier.8.bias"] + big)
    x, y = batch(True, N, 3, seed=1)
    y[:, 0], y[:, 1] = 1, 0
    tr.forward_backward(x, y, train=False)
    assert all(torch.isfinite(g).all() for g in all_gradients(tr).values()) and torch.isfinite(tr.losses()[0])
    assert not tr.gradient("classifier.8.bias")[:2].any() and tr.gradient("classifier.8.bias")[2:].any()


# ---- 3. dropout ----------------------------------------------------------------------------------------------------------------------
def test_dropout_masks_are_reproducible_and_shared_by_backward():
    plain, N, B = False, 70, 9
    dec, sd = decoder(plain, N)
    rates = (0.3, 0.2, 0.1)
    x, y = batch(plain, N, B, seed=21)
    runs = []
    for step in (7, 7, 8):
        tr = make_trainer(dec, "bce", {}, N, dropout=rates, seed=1234)
        logits, masks = tr.forward_backward(x, y, train=True, step=step, return_logits=True, return_masks=True)
        runs.append((logits.cpu(), [m.cpu() for m in masks], all_gradients(tr)))
    assert torch.equal(runs[0][0], runs[1][0]) and all(torch.equal(runs[0][2][k], runs[1][2][k]) for k in runs[0][2])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    assert not any(torch.equal(a, b) for a, b in zip(runs[0][1], runs[2][1]))
    for p, m in zip(rates, runs[0][1]):
        n = m.numel()
        keep, sigma = m.float().mean().item(), math.sqrt(p * (1 - p) / n)
        print(f"  p = {p}: keep fraction {keep:.4f} of {n}, {(keep - (1 - p)) / sigma:+.2f} sigma")
        assert abs(keep - (1 - p)) <= 5 * sigma
    masks = runs[0][1]
    _, g64 = torch_grads(sd, plain, torch.float64, x, y, "bce", {}, masks, rates)
    _, g32 = torch_grads(sd, plain, torch.float32, x, y, "bce", {}, masks, rates)
    for k, g in runs[0][2].items():
        check(k, g, g64[k], g32[k])
    # eval mode ignores the rates
    tr = make_trainer(dec, "bce", {}, N, dropout=rates)
    assert torch.equal(tr.forward_backward(x, y, train=False, return_logits=True), tr.forward(x))


# ---- 4. accumulation and determinism ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plain", [True, False], ids=["plain", "attention"])
def test_accumulation_and_determinism(plain):
    N, B = 70, 8
    dec, sd = decoder(plain, N)
    x, y = batch(plain, N, B, seed=5)
    tr = make_trainer(dec, "bce", {}, N)
    tr.forward_backward(x[:4], y[:4], loss_scale=0.5, train=False)
    tr.forward_backward(x[4:], y[4:], loss_scale=0.5, train=False)
    _, g64 = torch_grads(sd, plain, torch.float64, x, y, "bce", {})
    _, g32 = torch_grads(sd, plain, torch.float32, x, y, "bce", {})
    for k, g in all_gradients(tr).items():
        check(k, g, g64[k], g32[k])
    ring = tr.losses()
    check("loss halves", ring[0] + ring[1], loss_fn("bce", head_forward(head_params(sd, torch.float64, False), x.double(), plain), y.double()),
          loss_fn("bce", head_forward(head_params(sd, torch.float32, False), x, plain), y.float()))
    outs = []
    for _ in range(2):
        t = make_trainer(dec, "focal", {"alpha": 0.25, "gamma": 2.0}, N, dropout=(0.3, 0.2) if plain else (0.3, 0.2, 0.1), seed=9)
        t.forward_backward(x, y)
        grads = all_gradients(t)
        t.clip(0.01)
        t.step(1e-3, 1e-2)
        t.forward_backward(x, y)
        t.clip(1.0)
        t.step(1e-3, 1e-2)
        outs.append((grads, {k: t.parameter(k) for k in t.shapes}))
    for k in outs[0][0]:
        assert torch.equal(outs[0][0][k], outs[1][0][k]) and torch.equal(outs[0][1][k], outs[1][1][k]), k


# ---- 5. clip -------------------------------------------------------------------------------------------------------------------------
def test_clip_norm_and_scaling():
    plain, N, B = False, 1000, 9
    dec, _ = decoder(plain, N)
    x, y = batch(plain, N, B, seed=8)
    tr = make_trainer(dec, "bce", {}, N)
    tr.forward_backward(x, y, train=False)
    before = all_gradients(tr)
    norm64 = math.sqrt(sum((g.double() ** 2).sum().item() for g in before.values()))
    tr.clip(10.0 * norm64)                                    # inside the bound: nothing moves
    norm, coef = tr.grad_norm()
    print(f"  norm {norm:.9g} vs fp64 {norm64:.9g}, coef {coef}")
    assert abs(norm - norm64) <= 1e-6 * norm64 and coef == 1.0
    after = all_gradients(tr)
    assert all(torch.equal(before[k], after[k]) for k in before)
    max_norm = 0.25 * norm64                                  # outside: scaled to max_norm norm / (norm + 1e-6)
    tr.clip(max_norm)
    norm, coef = tr.grad_norm()
    assert abs(norm - norm64) <= 1e-6 * norm64 and coef < 1.0
    clipped = math.sqrt(sum((g.double() ** 2).sum().item() for g in all_gradients(tr).values()))
    want = max_norm * norm64 / (norm64 + 1e-6)
    print(f"  clipped norm {clipped:.9g}, expected {want:.9g}")
    assert abs(clipped - want) <= 1e-6 * want
    # accumulated gradient: the norm covers both micro-batches
    tr2 = make_trainer(dec, "bce", {}, N)
    tr2.forward_backward(x, y, train=False)
    tr2.forward_backward(x, y, train=False)
    tr2.clip(1e9)
    assert abs(tr2.grad_norm()[0] - 2 * norm64) <= 2e-6 * norm64


# ---- 6. AdamW ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 1e-6, 1e-2])
def test_adamw_matches_torch(wd):
    plain, N = True, 70
    dec, sd = decoder(plain, N)
    tr = HeadTrainer(dec)
    g = torch.Generator().manual_seed(17)
    p0 = {k: torch.randn(s, generator=g) for k, s in tr.shapes.items()}
    for k, v in p0.items():
        tr.write(_lib.HEAD_PARAM, k, v)
    refs = {}
    for dtype in (torch.float64, torch.float32):
        ps = {k: v.to(dtype).clone().requires_grad_(True) for k, v in p0.items()}
        refs[dtype] = (ps, torch.optim.AdamW(list(ps.values()), lr=1e-3, weight_decay=wd))
    for step in range(5):
        grads = {k: torch.randn(s, generator=g) * (0.1 + step) for k, s in tr.shapes.items()}
        for k, v in grads.items():
            tr.write(_lib.HEAD_GRAD, k, v)
        tr.step(1e-3, wd)
        for dtype, (ps, opt) in refs.items():
            for k in ps:
                ps[k].grad = grads[k].to(dtype)
            opt.step()
        assert all(not tr.gradient(k).any() for k in tr.shapes)
    worst = 0.0
    for k in tr.shapes:
        worst = max(worst, check(k, tr.parameter(k), refs[torch.float64][0][k].detach(), refs[torch.float32][0][k].detach()))
    print(f"adamw wd={wd}: worst device/e32 = {worst:.3f}")


# ---- 7. trajectory -------------------------------------------------------------------------------------------------------------------
TRAJ = dict(rows=128, N=11, B=16, steps=40, lr=3e-3, wd=1e-6, warmup=4, max_norm=1.0)


def teacher_data():
    """Features and labels from a fixed random teacher head (the plain layout with other weights)."""
    sd_t = synth.synth_state_dict(synth.plain_decoder_manifest(TRAJ["N"]), seed=77)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(TRAJ["rows"], 256, generator=g)
    logits = head_forward(head_params(sd_t, torch.float64, False), x.double(), True)
    return x, (logits > logits.median()).to(torch.uint8)


def torch_trajectory(sd, x, y, dtype):
    p = head_params(sd, dtype)
    opt = torch.optim.AdamW(list(p.values()), lr=TRAJ["lr"], weight_decay=TRAJ["wd"])
    losses = []
    for s in range(TRAJ["steps"]):
        lo = (s * TRAJ["B"]) % TRAJ["rows"]
        for group in opt.param_groups:
            group["lr"] = TRAJ["lr"] * lr_schedule("cosine", s, TRAJ["warmup"], TRAJ["steps"])
        loss = loss_fn("bce", head_forward(p, x[lo:lo + TRAJ["B"]].to(dtype), True), y[lo:lo + TRAJ["B"]].to(dtype))
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(list(p.values()), TRAJ["max_norm"])
        opt.step()
        losses.append(loss.detach())
    return torch.stack(losses)


def test_trajectory_follows_torch():
    dec, sd = decoder(True, TRAJ["N"])
    x, y = teacher_data()
    r64, r32 = torch_trajectory(sd, x, y, torch.float64), torch_trajectory(sd, x, y, torch.float32)
    assert r64[-1] < 0.5 * r64[0], "the fp64 torch loop itself must halve the loss"
    tr = HeadTrainer(dec, dropout=(0.0, 0.0))
    xd, yd = x.to(DEV), y.to(DEV)
    for s in range(TRAJ["steps"]):
        lo = (s * TRAJ["B"]) % TRAJ["rows"]
        tr.forward_backward(xd[lo:lo + TRAJ["B"]], yd[lo:lo + TRAJ["B"]], step=s)
        tr.clip(TRAJ["max_norm"])
        tr.step(TRAJ["lr"] * lr_schedule("cosine", s, TRAJ["warmup"], TRAJ["steps"]), TRAJ["wd"])
    dev = tr.losses()[:TRAJ["steps"]]
    print(f"  first {dev[0]:.6f} last {dev[-1]:.6f} (fp64 torch: {r64[0]:.6f} .. {r64[-1]:.6f})")
    check("loss sequence", dev, r64, r32)
    assert dev[-1] < 0.5 * dev[0]


# ---- 8. commit -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plain", [True, False], ids=["plain", "attention"])
def test_commit_makes_the_decoder_run_the_trained_head(plain):
    N = 70
    dec, sd = decoder(plain, N, seed=2)                       # (a decoder of its own: commit changes its device tables)
    x, y = batch(plain, N, 9, seed=2)
    lat = latent_input((3, 16, 9, 20), seed=6).to(DEV)
    tr = HeadTrainer(dec)
    before = dec(lat).clone()
    for _ in range(3):
        tr.forward_backward(x, y)
        tr.clip(1.0)
        tr.step(1e-2, 1e-6)
    own = tr.forward(tr.features(lat))
    assert torch.equal(dec(lat), before)                      # nothing reaches the decoder before commit
    tr.commit()
    after = dec(lat)
    torch.cuda.synchronize()
    assert torch.equal(after, own) and not torch.equal(after, before)
    exported = tr.state_dict()
    assert set(exported) == set(dec.state_dict())
    assert all(torch.equal(exported[k], v.cpu()) for k, v in dec.state_dict().items() if not k.startswith("classifier."))
