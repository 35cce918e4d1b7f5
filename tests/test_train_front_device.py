"""GPU: the attention decoder's front trainer (vt_front_*, vt_head_forward_backward_dx, vt_train_clip; csrc/train_front.hip) against a
training-mode torch restatement of the front on the CPU, in fp64 and fp32.

The rule of every parity check is tests/test_train_device.py's `check`: the device's error against fp64 must be within 4 x torch's own
fp32 error against fp64 (floor 1e-7), per tensor; every check prints its ratio.  Inputs are continuous random data, so no max has a
tie (asserted on the CPU reference).
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vae_tagger_amd import _lib, synth
from vae_tagger_amd._runtime import stream_ptr, vp
from vae_tagger_amd.train import DecoderTrainer, FrontTrainer, HeadTrainer

from _util import latent_input
from test_train_device import FACTOR, FLOOR, check, head_forward, loss_fn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 11
RM, RV, NBT = "feature_compress.1.running_mean", "feature_compress.1.running_var", "feature_compress.1.num_batches_tracked"
# (spatial attention, self attention, heads): every combination in which a trainable piece remains (feature_compress always does)
CONFIGS = [(1, 1, 8), (1, 1, 2), (1, 0, 8), (0, 1, 8), (0, 0, 8)]
CONFIG_IDS = ["sp-sa8", "sp-sa2", "sp", "sa8", "compress"]
SHAPES = [(8, 8), (9, 20), (16, 16)]            # pool = identity; ragged, overlapping windows; even windows
BATCHES = [1, 3, 9]


# ---- the torch front, training or eval mode ----------------------------------------------------------------------------------------
def front_forward(p, x, cfg, train, rm=None, rv=None, mask=None, rate=0.0, ties=None):
    """p: state_dict-keyed tensors of x's dtype.  rm / rv are updated in place when train.  mask [B][heads][64][64] (1 = kept)."""
    spatial, self_att, heads = cfg
    if spatial:
        w0, w2 = p["spatial_attention.channel_att.0.weight"], p["spatial_attention.channel_att.2.weight"]
        mlp = lambda t: F.conv2d(F.relu(F.conv2d(t, w0)), w2)            # noqa: E731
        x = x * torch.sigmoid(mlp(F.adaptive_avg_pool2d(x, 1)) + mlp(F.adaptive_max_pool2d(x, 1)))
        mx = torch.max(x, dim=1, keepdim=True)[0]
        if ties is not None:
            ties.append(int(((x == mx).sum(1) > 1).sum()))
        sp = torch.cat([x.mean(1, keepdim=True), mx], 1)
        x = x * torch.sigmoid(F.conv2d(sp, p["spatial_attention.spatial_att.0.weight"], padding=3))
    z = F.conv2d(x, p["feature_compress.0.weight"], p["feature_compress.0.bias"], padding=1)
    y = F.batch_norm(z, rm, rv, p["feature_compress.1.weight"], p["feature_compress.1.bias"], training=train, momentum=0.1, eps=1e-5)
    y = F.adaptive_avg_pool2d(F.relu(y), (8, 8))
    if self_att:
        B, hd = y.shape[0], 8 // heads
        s = "self_attention_post."
        t = y.view(B, 8, 64).transpose(1, 2)
        tn = F.layer_norm(t, (8,), p[s + "norm.weight"], p[s + "norm.bias"], 1e-5)
        proj = lambda n: F.linear(tn, p[s + n + ".weight"], p[s + n + ".bias"]).view(B, 64, heads, hd).transpose(1, 2)   # noqa: E731
        q, k, v = proj("q_proj"), proj("k_proj"), proj("v_proj")
        a = F.softmax(q @ k.transpose(-2, -1) / math.sqrt(hd), dim=-1)
        if mask is not None:
            a = a * mask.to(a.dtype) * (1.0 / (1.0 - rate))
        o = (a @ v).transpose(1, 2).contiguous().view(B, 64, 8)
        y = (F.linear(o, p[s + "out_proj.weight"], p[s + "out_proj.bias"]) + t).transpose(1, 2)
    return y.reshape(y.shape[0], 512)


def front_params(sd, dtype, names):
    return {k: sd[k].detach().to(dtype).clone().requires_grad_(True) for k in names}


def torch_front(sd, names, cfg, lat, d_feat, dtype, mask=None, rate=0.0):
    """(features, gradients, running_mean, running_var, ties) of one training-mode forward + backward with d_features given."""
    p = front_params(sd, dtype, names)
    rm, rv, ties = sd[RM].to(dtype).clone(), sd[RV].to(dtype).clone(), []
    f = front_forward(p, lat.to(dtype), cfg, True, rm, rv, mask, rate, ties)
    (f * d_feat.to(dtype)).sum().backward()
    return f.detach(), {k: v.grad for k, v in p.items()}, rm, rv, sum(ties)


# ---- decoders ----------------------------------------------------------------------------------------------------------------------
_DECODERS = {}


def decoder(cfg, seed=1):
    key = (cfg, seed)
    if key not in _DECODERS:
        from vae_tagger_amd.modules import AttentionClassificationDecoder
        spatial, self_att, heads = cfg
        d = AttentionClassificationDecoder(16, 16, 16, N, bool(spatial), bool(self_att), False, heads)
        sd = synth.synth_state_dict(synth.attention_decoder_manifest(N, 16, bool(spatial), bool(self_att), False), seed=seed)
        d.load_state_dict(sd, strict=False)
        _DECODERS[key] = (d.to(DEV).eval(), sd)
    return _DECODERS[key]


def rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def labels(B, seed):
    return (torch.rand(B, N, generator=torch.Generator().manual_seed(seed)) < 0.3).to(torch.uint8)


def front_gradients(tr):
    return {k: tr.gradient(k) for k in tr.shapes}


# Two gradients are ZERO in exact arithmetic: a bias in front of a training-mode BatchNorm is removed by the mean subtraction, and a
# bias of k shifts every score of a query row alike, which softmax ignores.  Their fp64 reference is rounding noise (1e-16), so the
# rule's relative error has no denominator; for them the same rule is applied with the error measured against the largest gradient
# of the weight of the same layer -- the scale of the terms that cancel.
ZERO_GRADIENTS = {"feature_compress.0.bias": "feature_compress.0.weight", "self_attention_post.k_proj.bias": "self_attention_post.k_proj.weight"}


def check_gradients(dev, g64, g32):
    worst = 0.0
    for k, v in dev.items():
        if k in ZERO_GRADIENTS:
            scale = g64[ZERO_GRADIENTS[k]].abs().max().item()
            assert g64[k].abs().max().item() <= 1e-12 * scale, f"{k}: the fp64 gradient should vanish"
            e32 = max((g32[k].double() - g64[k]).abs().max().item() / scale, FLOOR)
            ratio = (v.double() - g64[k]).abs().max().item() / scale / e32
            print(f"    {k} (zero by construction, against {ZERO_GRADIENTS[k]}): device/e32 = {ratio:.3f} (e32 {e32:.2e})")
            assert ratio <= FACTOR, f"{k}: device error is {ratio:.2f} x the fp32 yardstick {e32:.2e}"
        else:
            ratio = check(k, v, g64[k], g32[k])
        worst = max(worst, ratio)
    print(f"  worst gradient device/e32 = {worst:.3f}")
    return worst


# ---- 1. eval mode is the inference front -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize("hw", SHAPES)
def test_eval_forward_is_decode_features_bit_for_bit(cfg, hw):
    dec, _ = decoder(cfg)
    tr, head = FrontTrainer(dec), HeadTrainer(dec)
    for B in BATCHES:
        lat = latent_input((B, 16, *hw), seed=3 + B).to(DEV)
        own, ref = tr.forward(lat, train=False), head.features(lat)
        torch.cuda.synchronize()
        assert torch.equal(own, ref)


# ---- 2. / 3. training-mode forward, running statistics and the gradients of every front tensor -------------------------------------
@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("B", BATCHES)
def test_training_forward_and_gradients_match_autograd(cfg, hw, B):
    dec, sd = decoder(cfg)
    tr = FrontTrainer(dec, attention_dropout=0.0)
    lat, d_feat = latent_input((B, 16, *hw), seed=11 + B), rand((B, 512), 5 + B)
    f64, g64, rm64, rv64, ties = torch_front(sd, tr.shapes, cfg, lat, d_feat, torch.float64)
    f32, g32, rm32, rv32, _ = torch_front(sd, tr.shapes, cfg, lat, d_feat, torch.float32)
    assert ties == 0, "the inputs must leave no tie in the channel max"
    feats = tr.forward(lat.to(DEV), train=True)
    tr.backward(d_feat.to(DEV))
    print(f"  {CONFIG_IDS[CONFIGS.index(cfg)]} {hw} B={B}")
    check("features", feats.cpu(), f64, f32)
    check("running_mean", tr.buffer(RM), rm64, rm32)
    check("running_var", tr.buffer(RV), rv64, rv32)
    assert int(tr.buffer(NBT)) == int(sd[NBT]) + 1
    check_gradients(front_gradients(tr), g64, g32)


# ---- 4. end to end through the head ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[1]], ids=CONFIG_IDS[:2])
@pytest.mark.parametrize("B,hw", [(3, (9, 20)), (9, (16, 16))])
def test_end_to_end_gradients_through_the_head(cfg, B, hw):
    dec, sd = decoder(cfg)
    tr = DecoderTrainer(dec, dropout=(0.0, 0.0, 0.0), attention_dropout=0.0)
    lat, y = latent_input((B, 16, *hw), seed=21 + B), labels(B, 9)
    refs = {}
    for dtype in (torch.float64, torch.float32):
        p = front_params(sd, dtype, tr.front.shapes)
        ph = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items() if k.startswith("classifier.")}
        f = front_forward(p, lat.to(dtype), cfg, True, sd[RM].to(dtype).clone(), sd[RV].to(dtype).clone())
        f.retain_grad()
        loss_fn("bce", head_forward(ph, f, False), y.to(dtype)).backward()
        refs[dtype] = ({k: v.grad for k, v in p.items()}, {k: v.grad for k, v in ph.items()}, f.grad)
    tr.forward_backward(lat.to(DEV), y.to(DEV))
    check_gradients(front_gradients(tr.front), refs[torch.float64][0], refs[torch.float32][0])
    for k in tr.head.shapes:
        check(k, tr.head.gradient(k), refs[torch.float64][1][k], refs[torch.float32][1][k])


@pytest.mark.parametrize("B", [1, 9, 17])
def test_head_dx_matches_autograd_and_leaves_the_head_gradients_bit_for_bit(B):
    dec, sd = decoder(CONFIGS[0])
    a, b = HeadTrainer(dec, dropout=(0.3, 0.2, 0.1), seed=4), HeadTrainer(dec, dropout=(0.3, 0.2, 0.1), seed=4)
    x, y = rand((B, 512), 31 + B), labels(B, 12)
    masks = a.forward_backward(x, y, step=0, return_masks=True)
    d = torch.empty(B, 512, dtype=torch.float32, device=DEV)
    ws, need = b._ws(B)
    xd, yd = x.to(DEV), y.to(DEV)
    b.ctx.call("vt_head_forward_backward_dx", *b._state(), vp(xd), vp(yd), _lib.VT_U8, B, b.loss_kind, b.alpha, b.gamma, None, 1.0, 1, b.dropout,
               b.seed, 0, None, None, vp(d), ws, need, stream_ptr(xd.device))
    torch.cuda.synchronize()
    for k in a.shapes:
        assert torch.equal(a.gradient(k), b.gradient(k)), k
    refs = {}
    for dtype in (torch.float64, torch.float32):
        ph = {k: v.detach().to(dtype) for k, v in sd.items() if k.startswith("classifier.")}
        f = x.to(dtype).requires_grad_(True)
        loss_fn("bce", head_forward(ph, f, False, [m.cpu() for m in masks], (0.3, 0.2, 0.1)), y.to(dtype)).backward()
        refs[dtype] = f.grad
    check("d_features", d.cpu(), refs[torch.float64], refs[torch.float32])


# ---- 5. dropout --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[1], CONFIGS[3]], ids=["sp-sa8", "sp-sa2", "sa8"])
def test_dropout_mask_replayed_in_torch_reproduces_the_gradients(cfg):
    dec, sd = decoder(cfg)
    B, hw, rate = 3, (9, 20), 0.25
    tr = FrontTrainer(dec, attention_dropout=rate, seed=7)
    lat, d_feat = latent_input((B, 16, *hw), seed=41), rand((B, 512), 42)
    feats, mask = tr.forward(lat.to(DEV), train=True, step=5, return_mask=True)
    tr.backward(d_feat.to(DEV))
    mask = mask.cpu()
    assert mask.shape == (B, cfg[2], 64, 64) and set(mask.unique().tolist()) <= {0, 1}
    n, kept = mask.numel(), int(mask.sum())
    sigma = math.sqrt(n * rate * (1.0 - rate))
    print(f"  kept {kept} of {n}: {(kept - n * (1 - rate)) / sigma:+.2f} sigma")
    assert abs(kept - n * (1.0 - rate)) <= 4.0 * sigma
    f64, g64, *_ = torch_front(sd, tr.shapes, cfg, lat, d_feat, torch.float64, mask, rate)
    f32, g32, *_ = torch_front(sd, tr.shapes, cfg, lat, d_feat, torch.float32, mask, rate)
    check("features", feats.cpu(), f64, f32)
    check_gradients(front_gradients(tr), g64, g32)
    again = FrontTrainer(dec, attention_dropout=rate, seed=7)
    _, same = again.forward(lat.to(DEV), train=True, step=5, return_mask=True)
    _, other = again.forward(lat.to(DEV), train=True, step=6, return_mask=True)
    assert torch.equal(same.cpu(), mask) and not torch.equal(other.cpu(), mask)


# ---- 6. accumulation and determinism -----------------------------------------------------------------------------------------------
def test_accumulation_and_determinism():
    cfg = CONFIGS[0]
    dec, _ = decoder(cfg)
    lats = [latent_input((3, 16, 9, 20), seed=51).to(DEV), latent_input((2, 16, 16, 16), seed=52).to(DEV)]
    ds = [rand((3, 512), 53).to(DEV), rand((2, 512), 54).to(DEV)]

    def run(which):
        tr = FrontTrainer(dec, attention_dropout=0.2, seed=3)
        for i in which:
            tr.forward(lats[i], train=True, step=i)
            tr.backward(ds[i])
        return tr

    one, two, both, again = run([0]), run([1]), run([0, 1]), run([0, 1])
    g1, g2, g12 = front_gradients(one), front_gradients(two), front_gradients(both)
    for k in g12:
        assert torch.equal(g12[k], g1[k] + g2[k]), k
    assert int(both.buffer(NBT)) == int(one.buffer(NBT)) + 1
    assert torch.equal(both.state_bytes(), again.state_bytes())


# ---- 7. one clip over both blocks --------------------------------------------------------------------------------------------------
def test_train_clip_norm_and_scaling():
    dec, _ = decoder(CONFIGS[0])
    tr = DecoderTrainer(dec, seed=2)
    lat, y = latent_input((5, 16, 9, 20), seed=61).to(DEV), labels(5, 62).to(DEV)
    tr.forward_backward(lat, y)

    def grads():
        return {**{k: tr.head.gradient(k) for k in tr.head.shapes}, **front_gradients(tr.front)}

    g0 = grads()
    want = math.sqrt(sum(float((v.double() ** 2).sum()) for v in g0.values()))
    tr.clip(1e9)
    raw = tr.front._read(_lib.HEAD_NORM, None, (16,), torch.uint8).numpy()
    sq = float(raw[:8].view(np.float64)[0])
    print(f"  norm {math.sqrt(sq):.9e} want {want:.9e}")
    assert abs(math.sqrt(sq) - want) <= 1e-12 * want
    assert tr.head.grad_norm() == tr.front.grad_norm() and tr.head.grad_norm()[1] == 1.0
    assert all(torch.equal(v, g0[k]) for k, v in grads().items()), "a gradient inside the bound keeps its bits"
    tr.clip(0.25 * want)
    norm, coef = tr.front.grad_norm()
    assert (norm, coef) == tr.head.grad_norm()
    assert coef == float(np.float32(np.float32(0.25 * want) / (np.float32(norm) + np.float32(1e-6)))) and coef < 1.0
    for k, v in grads().items():
        assert torch.equal(v, g0[k] * torch.tensor(coef, dtype=torch.float32)), k


# ---- 8. five steps of AdamW + clip -------------------------------------------------------------------------------------------------
TRAJ = dict(steps=5, B=6, hw=(9, 20), lr=3e-3, wd=1e-6, max_norm=1.0)


def torch_trajectory(sd, cfg, names, lats, ys, dtype):
    p = front_params(sd, dtype, names)
    p.update({k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items() if k.startswith("classifier.")})
    rm, rv = sd[RM].to(dtype).clone(), sd[RV].to(dtype).clone()
    opt = torch.optim.AdamW(list(p.values()), lr=TRAJ["lr"], weight_decay=TRAJ["wd"])
    losses = []
    for lat, y in zip(lats, ys):
        loss = loss_fn("bce", head_forward(p, front_forward(p, lat.to(dtype), cfg, True, rm, rv), False), y.to(dtype))
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(list(p.values()), TRAJ["max_norm"])
        opt.step()
        losses.append(loss.detach())
    return torch.stack(losses), {k: v.detach() for k, v in p.items()}, rm, rv


def test_five_step_trajectory_follows_torch():
    cfg = CONFIGS[0]
    dec, sd = decoder(cfg)
    tr = DecoderTrainer(dec, dropout=(0.0, 0.0, 0.0), attention_dropout=0.0)
    lats = [latent_input((TRAJ["B"], 16, *TRAJ["hw"]), seed=70 + s) for s in range(TRAJ["steps"])]
    ys = [labels(TRAJ["B"], 80 + s) for s in range(TRAJ["steps"])]
    l64, p64, rm64, rv64 = torch_trajectory(sd, cfg, tr.front.shapes, lats, ys, torch.float64)
    l32, p32, rm32, rv32 = torch_trajectory(sd, cfg, tr.front.shapes, lats, ys, torch.float32)
    for s in range(TRAJ["steps"]):
        tr.forward_backward(lats[s].to(DEV), ys[s].to(DEV), step=s)
        tr.clip(TRAJ["max_norm"])
        tr.step(TRAJ["lr"], TRAJ["wd"])
    check("loss sequence", tr.losses()[:TRAJ["steps"]], l64, l32)
    check("running_mean", tr.front.buffer(RM), rm64, rm32)
    check("running_var", tr.front.buffer(RV), rv64, rv32)
    for k in tr.front.shapes:
        if k not in ZERO_GRADIENTS:                           # (Adam divides their rounding noise by its own size: +-lr steps of no meaning)
            check(k, tr.front.parameter(k), p64[k], p32[k])
    assert int(tr.front.buffer(NBT)) == int(sd[NBT]) + TRAJ["steps"]


# ---- 9. commit ---------------------------------------------------------------------------------------------------------------------
def test_commit_makes_the_decoder_run_the_trained_front_and_head():
    cfg = CONFIGS[0]
    dec, sd = decoder(cfg, seed=2)                            # (a decoder of its own: commit changes its device tables)
    tr = DecoderTrainer(dec, seed=1)
    lat = latent_input((4, 16, 9, 20), seed=91).to(DEV)
    before = dec(lat).clone()
    for s in range(3):
        tr.forward_backward(latent_input((4, 16, 16, 16), seed=92 + s).to(DEV), labels(4, 95 + s).to(DEV))
        tr.clip(1.0)
        tr.step(1e-2, 1e-6)
    own = tr.forward(lat)
    assert torch.equal(dec(lat), before)                      # nothing reaches the decoder before commit
    tr.commit()
    after = dec(lat)
    torch.cuda.synchronize()
    assert torch.equal(after, own) and not torch.equal(after, before)
    exported = tr.state_dict()
    assert set(exported) == set(dec.state_dict())
    assert all(exported[k].dtype == v.dtype and exported[k].shape == v.shape for k, v in dec.state_dict().items())
    assert int(exported[NBT]) == int(sd[NBT]) + 3
    for k in list(tr.front.shapes) + [RM, RV]:
        if k != "self_attention_post.k_proj.bias":            # (its gradient is zero: nothing but the weight decay moves it)
            assert not torch.equal(exported[k], sd[k].reshape(exported[k].shape)), k
    # a decoder loaded from the exported state_dict folds the running statistics on the host: scale / shift may differ from the device's
    # fold by an ulp (6e-8 relative), which reaches the logits through four normalised layers; 1e-5 of the largest logit bounds that
    from vae_tagger_amd.modules import AttentionClassificationDecoder
    fresh = AttentionClassificationDecoder(16, 16, 16, N, True, True, False, 8)
    fresh.load_state_dict(exported, strict=False)
    again = fresh.to(DEV).eval()(lat)
    assert (again - after).abs().max().item() <= 1e-5 * after.abs().max().item()
