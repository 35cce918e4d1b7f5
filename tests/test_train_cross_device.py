"""GPU: the cross-attention trainer (vt_cross_*, vt_train_clip3; csrc/train_cross.hip; train.CrossTrainer and DecoderTrainer on a decoder
with cross-attention) against a torch restatement of the piece (modules.py:105-124, :451-459) on the CPU, in fp64 and fp32.

The rule of every parity check is tests/test_train_device.py's `check`: the device's error against fp64 must be within 4 x torch's own
fp32 error against fp64 (floor 1e-7), per tensor; every check prints its ratio.  With the synthetic weights as they come the softmax
over the 64 key tokens is nearly uniform and a wrong softmax backward would hide, so every decoder here has
cross_attention.q_proj.weight and k_proj.weight multiplied by 4 (the reference's largest softmax weight is asserted to lie in (0.1, 0.9)).
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vae_tagger_amd import _lib, synth
from vae_tagger_amd.train import CROSS_PREFIXES, CrossTrainer, DecoderTrainer, FrontTrainer, HeadTrainer

from _util import latent_input
from test_train_device import FACTOR, FLOOR, check, head_forward, loss_fn
from test_train_front_device import RM, RV, ZERO_GRADIENTS as FRONT_ZERO_GRADIENTS, front_forward, front_params, labels, rand

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 11
CX = "cross_attention."
# the bias of k shifts every score of the one query row alike, which softmax ignores: its gradient is zero in exact arithmetic, and the
# rule is applied with the error measured against the largest gradient of k_proj.weight (test_train_front_device.ZERO_GRADIENTS)
ZERO_GRADIENTS = {**FRONT_ZERO_GRADIENTS, CX + "k_proj.bias": CX + "k_proj.weight"}


# ---- the torch piece ---------------------------------------------------------------------------------------------------------------
def cross_forward(p, x, heads, weights=None):
    """x [B][512] (the front's rows) -> the head's feature rows.  p: state_dict-keyed tensors of x's dtype."""
    B, hd = x.shape[0], 256 // heads
    q = F.linear(x, p["query_generator.weight"], p["query_generator.bias"])
    t = x.view(B, 8, 64).transpose(1, 2)
    u = F.linear(q, p[CX + "q_proj.weight"], p[CX + "q_proj.bias"]).view(B, 1, heads, hd).transpose(1, 2)
    k = F.linear(t, p[CX + "k_proj.weight"], p[CX + "k_proj.bias"]).view(B, 64, heads, hd).transpose(1, 2)
    v = F.linear(t, p[CX + "v_proj.weight"], p[CX + "v_proj.bias"]).view(B, 64, heads, hd).transpose(1, 2)
    w = F.softmax(u @ k.transpose(-2, -1) / math.sqrt(hd), dim=-1)
    if weights is not None:
        weights.append(w.detach())
    o = (w @ v).transpose(1, 2).contiguous().view(B, 256)
    a = F.linear(o, p[CX + "out_proj.weight"], p[CX + "out_proj.bias"]) + q
    return x + a.mean(dim=1, keepdim=True).expand_as(x)


def cross_params(sd, dtype):
    return {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items() if k.startswith(CROSS_PREFIXES)}


# ---- decoders ----------------------------------------------------------------------------------------------------------------------
_DECODERS = {}


def decoder(cfg, seed=1, cross=True):
    key = (cfg, seed, cross)
    if key not in _DECODERS:
        from vae_tagger_amd.modules import AttentionClassificationDecoder
        spatial, self_att, heads = cfg
        d = AttentionClassificationDecoder(16, 16, 16, N, bool(spatial), bool(self_att), cross, heads)
        sd = synth.synth_state_dict(synth.attention_decoder_manifest(N, 16, bool(spatial), bool(self_att), cross), seed=seed)
        if cross:
            for k in (CX + "q_proj.weight", CX + "k_proj.weight"):
                sd[k] = sd[k] * 4.0
        d.load_state_dict(sd, strict=False)
        _DECODERS[key] = (d.to(DEV).eval(), sd)
    return _DECODERS[key]


def gradients(tr):
    return {k: tr.gradient(k) for k in tr.shapes}


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


# ---- 1. the piece alone against autograd -------------------------------------------------------------------------------------------
def torch_piece(sd, heads, x, d_feat, dtype):
    p = cross_params(sd, dtype)
    xx, weights = x.to(dtype).clone().requires_grad_(True), []
    f = cross_forward(p, xx, heads, weights)
    (f * d_feat.to(dtype)).sum().backward()
    return f.detach(), xx.grad, {k: v.grad for k, v in p.items()}, weights[0]


@pytest.mark.parametrize("heads", [8, 2, 1])
@pytest.mark.parametrize("B", [1, 3, 9, 70])     # 70: beyond one 64-image pass of the outer-product kernel, 9 passes of the mat-vec, and a
def test_piece_matches_autograd(B, heads):        # g [B] of doubles that no longer fits the 256 bytes 32 floats would take
    dec, sd = decoder((1, 1, heads))
    tr = CrossTrainer(dec)
    assert set(tr.shapes) == {k for k in sd if k.startswith(CROSS_PREFIXES)} and len(tr.shapes) == 10
    x, d_feat = F.relu(rand((B, 512), 110 + B)), rand((B, 512), 200 + B)     # (seeds at which the assertion on the reference below holds)
    f64, dx64, g64, w64 = torch_piece(sd, heads, x, d_feat, torch.float64)
    f32, dx32, g32, _ = torch_piece(sd, heads, x, d_feat, torch.float32)
    print(f"  heads={heads} B={B}: largest softmax weight {w64.max().item():.3f}, cross part of d_x {(dx64 - d_feat.double()).abs().max().item():.3f}")
    assert 0.1 < w64.max().item() < 0.9, "the reference's softmax must be neither uniform nor saturated"
    feats = tr.forward(x.to(DEV))
    d_x = tr.backward(d_feat.to(DEV)).cpu()
    check("features", feats.cpu(), f64, f32)
    check("d_x", d_x, dx64, dx32)
    check("d_x - d_features", d_x.double() - d_feat.double(), dx64 - d_feat.double(), dx32.double() - d_feat.double())
    dev = gradients(tr)
    check_gradients(dev, g64, g32)
    # what y = x + mean(a) 1 implies: every entry of d a is the same number per image
    ow, ob = dev[CX + "out_proj.weight"], dev[CX + "out_proj.bias"]
    assert torch.equal(ow, ow[:1].expand_as(ow)), "every row of the out_proj.weight gradient equals row 0"
    assert torch.equal(ob, ob[:1].expand_as(ob)), "every entry of the out_proj.bias gradient is equal"


def test_backward_needs_the_forward_of_the_same_batch():
    dec, _ = decoder((1, 1, 8))
    tr = CrossTrainer(dec)
    with pytest.raises(RuntimeError, match="forward of the same batch"):
        tr.backward(torch.zeros(2, 512))


def test_two_trainers_on_one_device_may_interleave():
    dec, _ = decoder((1, 1, 8))
    a, b, alone = CrossTrainer(dec), CrossTrainer(dec), CrossTrainer(dec)
    xa, xb = F.relu(rand((3, 512), 61)).to(DEV), F.relu(rand((5, 512), 62)).to(DEV)
    da = rand((3, 512), 63).to(DEV)
    a.forward(xa)
    b.forward(xb)                                             # must not disturb what a's backward reads
    got = a.backward(da)
    alone.forward(xa)
    want = alone.backward(da)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    for k in a.shapes:
        assert torch.equal(a.gradient(k), alone.gradient(k)), k


# ---- 2. the eval chain is inference, bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [(1, 1, 8), (1, 1, 2), (0, 1, 1), (0, 0, 8)], ids=["sp-sa8", "sp-sa2", "sa1", "compress"])
@pytest.mark.parametrize("hw", [(8, 8), (9, 20)])
def test_eval_chain_is_decode_features_bit_for_bit(cfg, hw):
    dec, _ = decoder(cfg)
    front, cross, head = FrontTrainer(dec), CrossTrainer(dec), HeadTrainer(dec)
    for B in (1, 3, 9):
        lat = latent_input((B, 16, *hw), seed=3 + B).to(DEV)
        rows = front.forward(lat, train=False)
        own, ref = cross.forward(rows), head.features(lat)
        torch.cuda.synchronize()
        assert torch.equal(own, ref) and not torch.equal(rows, ref)


# ---- 3. end to end through the head ------------------------------------------------------------------------------------------------
def torch_decoder_grads(sd, cfg, front_names, lat, y, dtype):
    p = front_params(sd, dtype, front_names)
    pc = cross_params(sd, dtype)
    ph = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items() if k.startswith("classifier.")}
    ties = []
    x = front_forward(p, lat.to(dtype), cfg, True, sd[RM].to(dtype).clone(), sd[RV].to(dtype).clone(), ties=ties)
    loss_fn("bce", head_forward(ph, cross_forward(pc, x, cfg[2]), False), y.to(dtype)).backward()
    return {k: v.grad for k, v in {**p, **pc, **ph}.items()}, sum(ties)


@pytest.mark.parametrize("B,hw", [(3, (9, 20)), (9, (8, 8))])
def test_end_to_end_gradients_through_the_head(B, hw):
    cfg = (1, 1, 8)
    dec, sd = decoder(cfg)
    tr = DecoderTrainer(dec, dropout=(0.0, 0.0, 0.0), attention_dropout=0.0)
    assert tr.cross is not None
    lat, y = latent_input((B, 16, *hw), seed=21 + B), labels(B, 9)
    g64, ties = torch_decoder_grads(sd, cfg, tr.front.shapes, lat, y, torch.float64)
    g32, _ = torch_decoder_grads(sd, cfg, tr.front.shapes, lat, y, torch.float32)
    assert ties == 0, "the inputs must leave no tie in the channel max"
    tr.forward_backward(lat.to(DEV), y.to(DEV))
    print(f"  B={B} {hw}")
    check_gradients({**gradients(tr.front), **gradients(tr.cross), **gradients(tr.head)}, g64, g32)


# ---- 4. accumulation and determinism -----------------------------------------------------------------------------------------------
def test_accumulation_and_determinism():
    dec, _ = decoder((1, 1, 8))
    xs = [F.relu(rand((3, 512), 51)).to(DEV), F.relu(rand((2, 512), 52)).to(DEV)]
    ds = [rand((3, 512), 53).to(DEV), rand((2, 512), 54).to(DEV)]

    def piece(which):
        tr = CrossTrainer(dec)
        for i in which:
            tr.forward(xs[i])
            tr.backward(ds[i])
        return tr

    g1, g2, g12 = gradients(piece([0])), gradients(piece([1])), gradients(piece([0, 1]))
    for k in g12:
        assert torch.equal(g12[k], g1[k] + g2[k]), k
    lats = [latent_input((3, 16, 9, 20), seed=55).to(DEV), latent_input((2, 16, 8, 8), seed=56).to(DEV)]
    ys = [labels(3, 57).to(DEV), labels(2, 58).to(DEV)]

    def full():
        tr = DecoderTrainer(dec, attention_dropout=0.2, seed=3)
        for s in range(2):
            tr.forward_backward(lats[s], ys[s], step=s)
        tr.clip(1.0)
        tr.step(1e-3, 1e-6)
        tr.forward_backward(lats[0], ys[0], step=2)
        return tr

    a, b = full(), full()
    for name in ("head", "front", "cross"):
        assert torch.equal(getattr(a, name).state_bytes(), getattr(b, name).state_bytes()), name


# ---- 5. one clip over three blocks; vt_train_clip over two as before ---------------------------------------------------------------
def scalars(tr):
    raw = tr._read(_lib.HEAD_NORM, None, (16,), torch.uint8).numpy()
    return float(raw[:8].view(np.float64)[0]), float(raw[8:12].view(np.float32)[0]), float(raw[12:16].view(np.float32)[0])


@pytest.mark.parametrize("cross", [True, False], ids=["clip3", "clip"])
def test_train_clip_norm_and_scaling(cross):
    dec, _ = decoder((1, 1, 8), cross=cross)
    tr = DecoderTrainer(dec, seed=2)
    assert (tr.cross is not None) == cross
    blocks = [tr.head, tr.front] + ([tr.cross] if cross else [])
    lat, y = latent_input((5, 16, 9, 20), seed=61).to(DEV), labels(5, 62).to(DEV)
    tr.forward_backward(lat, y)

    def grads():
        return {k: v for b in blocks for k, v in gradients(b).items()}

    g0 = grads()
    want = math.sqrt(sum(float((v.double() ** 2).sum()) for v in g0.values()))
    tr.clip(1e9)
    sq = scalars(blocks[-1])[0]
    print(f"  norm {math.sqrt(sq):.9e} want {want:.9e}")
    assert abs(math.sqrt(sq) - want) <= 1e-12 * want
    assert all(scalars(b) == scalars(tr.head) for b in blocks) and tr.head.grad_norm()[1] == 1.0
    assert all(torch.equal(v, g0[k]) for k, v in grads().items()), "a gradient inside the bound keeps its bits"
    tr.clip(0.25 * want)
    _, norm, coef = scalars(blocks[-1])
    assert all(scalars(b) == scalars(tr.head) for b in blocks)
    assert coef == float(np.float32(np.float32(0.25 * want) / (np.float32(norm) + np.float32(1e-6)))) and coef < 1.0
    for k, v in grads().items():
        assert torch.equal(v, g0[k] * torch.tensor(coef, dtype=torch.float32)), k


# ---- 6. five steps of AdamW + clip, then commit ------------------------------------------------------------------------------------
TRAJ = dict(steps=5, B=6, hw=(9, 20), lr=3e-3, wd=1e-6, max_norm=1.0)


def torch_trajectory(sd, cfg, names, lats, ys, dtype):
    p = front_params(sd, dtype, names)
    p.update(cross_params(sd, dtype))
    p.update({k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items() if k.startswith("classifier.")})
    rm, rv = sd[RM].to(dtype).clone(), sd[RV].to(dtype).clone()
    opt = torch.optim.AdamW(list(p.values()), lr=TRAJ["lr"], weight_decay=TRAJ["wd"])
    losses = []
    for lat, y in zip(lats, ys):
        x = front_forward(p, lat.to(dtype), cfg, True, rm, rv)
        loss = loss_fn("bce", head_forward(p, cross_forward(p, x, cfg[2]), False), y.to(dtype))
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(list(p.values()), TRAJ["max_norm"])
        opt.step()
        losses.append(loss.detach())
    return torch.stack(losses), {k: v.detach() for k, v in p.items()}, rm, rv


def test_five_step_trajectory_follows_torch_and_commit_reaches_the_decoder():
    cfg = (1, 1, 8)
    dec, sd = decoder(cfg, seed=2)                            # (a decoder of its own: commit changes its device tables)
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
    for block in (tr.front, tr.cross):
        for k in block.shapes:
            if k not in ZERO_GRADIENTS:                       # (Adam divides their rounding noise by its own size: +-lr steps of no meaning)
                check(k, block.parameter(k), p64[k], p32[k])
    # commit: the decoder then runs what was trained
    lat = latent_input((4, 16, 9, 20), seed=91).to(DEV)
    before = dec(lat).clone()
    own = tr.forward(lat)
    assert torch.equal(dec(lat), before)                      # nothing reaches the decoder before commit
    tr.commit()
    after = dec(lat)
    torch.cuda.synchronize()
    assert torch.equal(after, own) and not torch.equal(after, before)
    exported = tr.state_dict()
    assert list(exported) == list(dec.state_dict())
    for k in tr.cross.shapes:
        if k not in ZERO_GRADIENTS:
            assert not torch.equal(exported[k], sd[k]), k
