"""train_full on the device, on the small VAE of tests/_vae_train_step_ref.py (block_out (64, 128, 512), one layer per block, B = 2, 16 x 24, 152
tensors of which the encoder's 64 come first) and 11-tag decoders: the attention decoder with and without cross-attention and the plain one.
The joint norm against the two separate clips and the host mirror, bit for bit; vt_posterior_mode_latent against torch's two eager ops; the
encoder-only step against the full one at reconstruction weight 0; FullTrainer.train_step against the same step done by hand through the C ABI; a
resume through files; and learning against a CPU trajectory.

The learning case, chosen on the CPU before any device run.  One fixed batch, the noise of step k keyed on first_image = k B, the simplified loss
(triplet 1 + classification 1, margin 1, cosine), the attention decoder without cross-attention, all dropout rates 0, clip at 1.0, AdamW at a
constant lr with weight decay 1e-6.  The fp32 reference (step_autograd for the triplet term, torch autograd of the restated decoder for the
classification term, clip_grad_norm_ over both, ONE torch.optim.AdamW over the encoder's and the decoder's tensors -- the VAE's image decoder is
not in it -- on the host mirror of the device's eps) gave the trajectories recorded in the learning test's docstring."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vae_tagger_amd import _lib, synth, train_full, vae_backward
from vae_tagger_amd.train import DecoderTrainer

from _vae_train_step_ref import LATENT, MARGIN, SIM, SMALL, _sub, step_autograd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H, W, SEED, N = 2, 16, 24, 77, 11
LR, WD, MAX_NORM = 3e-4, 1e-6, 1.0
SCALING, SHIFT = 0.3611, 0.1159
FULL = {"reconstruction": 1.0, "kl": 1e-2, "triplet": 1.0, "classification": 1.0}
KINDS = ["attention", "cross", "plain"]
vp = ctypes.c_void_p


def stream():
    return vp(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


@pytest.fixture(scope="module")
def case():
    p = synth.synth_state_dict({**synth.encoder_manifest(**SMALL), **synth.image_decoder_manifest(**SMALL)}, seed=5)
    images = synth.synth_images(3 * B, H, W, seed=6)
    g = torch.Generator().manual_seed(8)
    labels = tuple((torch.rand(B, N, generator=g) < 0.5).float() for _ in range(2))
    labels[0][:, 0] = 1.0
    dev = dict(a=images[:B].to(DEV).contiguous(), p=images[B:2 * B].to(DEV).contiguous(), n=images[2 * B:].to(DEV).contiguous(),
               la=labels[0].to(DEV), lp=labels[1].to(DEV))
    return dict(p=p, images=images, labels=labels, dev=dev, decoders={})


def decoder(case, kind):
    """one module per kind, never committed to: every trainer made on it starts from the same tables"""
    if kind not in case["decoders"]:
        from vae_tagger_amd.modules import AttentionClassificationDecoder, ClassificationDecoder
        if kind == "plain":
            d, sd = ClassificationDecoder(16, 16, 16, N), synth.synth_state_dict(synth.plain_decoder_manifest(N), seed=1)
        else:
            cross = kind == "cross"
            d = AttentionClassificationDecoder(16, 16, 16, N, True, True, cross, 8)
            sd = synth.synth_state_dict(synth.attention_decoder_manifest(N, 16, True, True, cross), seed=1)
        d.load_state_dict(sd, strict=False)
        case["decoders"][kind] = (d.to(DEV).eval(), sd)
    return case["decoders"][kind]


def make(case, kind, simplified, **kw):
    kw.setdefault("weights", FULL)
    return train_full.FullTrainer(case["p"], decoder(case, kind)[0], simplified=simplified, margin=MARGIN, similarity_type=SIM, seed=SEED,
                                  scaling_factor=SCALING, shift_factor=SHIFT, **kw)


def batch(case, first):
    d = case["dev"]
    return (d["a"], d["p"], d["n"], d["la"], d["lp"], first)


def arenas(tr):
    torch.cuda.synchronize()
    return [a.clone() for a in tr.vae._arena]


def block_bytes(tr):
    return [b.state_bytes() for b in tr.blocks]


def scalars16(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().tobytes()


def block_scalars(b):
    return b._read(_lib.HEAD_NORM, None, (16,), torch.uint8).numpy().tobytes()


def forward_backwards(ft, case, first=0):
    """both backward passes of one step, no clip and no step -> (grads, latent)"""
    _, grads, moments = ft.vae_forward_backward(*batch(case, first))
    latent = ft.mode_latent(moments, B)
    ft.decoder_forward_backward(latent, case["dev"]["la"], ft.t)
    return grads, latent


def joint(ft, grads, n, max_norm, chunk, scalars):
    """vt_full_optim_norm through the C ABI on the first n gradient tensors"""
    keys = list(grads)[:n]
    ptrs = (vp * n)(*[grads[k].data_ptr() for k in keys])
    numel = (ctypes.c_longlong * n)(*[grads[k].numel() for k in keys])
    need = ft.head.ctx.lib.vt_vae_optim_workspace_bytes(numel, n)
    ws = torch.zeros(need + 256, dtype=torch.uint8, device=DEV)
    ptr = (ws.data_ptr() + 255) // 256 * 256
    ft.head.ctx.call("vt_full_optim_norm", ptrs, numel, n, max_norm, vp(scalars.data_ptr()), vp(ptr), need, chunk, *ft._block_states(), stream())
    return ptrs, numel, ws


# ---- 1. the joint norm, exact ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_joint_norm_is_the_two_separate_sums_added_once(case, kind):
    ft = make(case, kind, simplified=False)
    assert len(ft.blocks) == {"attention": 2, "cross": 3, "plain": 1}[kind] and ft.n == 152 and ft.n_encoder == 64
    grads, _ = forward_backwards(ft, case)
    # the two separate clips at a bound nothing reaches: nothing is scaled, the scalars hold the two squared norms
    ft.vae.clip(grads, 1e30)
    ft.dec.clip(1e30)
    sq_v = np.frombuffer(scalars16(ft.vae._scalars), np.float64)[0]
    sq_d = np.frombuffer(block_scalars(ft.head), np.float64)[0]
    ft.vae._clipped = False
    assert sq_v > 0 and sq_d > 0
    print(f"  {kind}: S_vae = {sq_v!r}, S_blocks = {sq_d!r}")
    scalars = torch.zeros(2, dtype=torch.float64, device=DEV)
    seen = []
    for chunk in (0, 1, 7):
        scalars.zero_()
        joint(ft, grads, 152, 1e30, chunk, scalars)
        got = scalars16(scalars)
        assert np.frombuffer(got, np.float64)[0] == float(sq_v) + float(sq_d)                    # Python's float arithmetic: one fp64 add
        assert got == train_full.joint_clip_host(sq_v, sq_d, 1e30), chunk
        assert all(block_scalars(b) == got for b in ft.blocks), chunk                           # every scalars block holds the same 16 bytes
        seen.append(got)
    assert seen[0] == seen[1] == seen[2]
    # the prefix form: the encoder's tensors alone, on the same list and on a list that holds only them
    enc = {k: g for k, g in grads.items() if k.startswith("encoder.")}
    assert list(enc) == list(grads)[:64]
    ptrs = (vp * 64)(*[g.data_ptr() for g in enc.values()])
    numel = (ctypes.c_longlong * 64)(*[g.numel() for g in enc.values()])
    need = ft.vae.ctx.lib.vt_vae_optim_workspace_bytes(numel, 64)
    ws = torch.zeros(need + 256, dtype=torch.uint8, device=DEV)
    sc_e = torch.zeros(2, dtype=torch.float64, device=DEV)
    ft.vae.ctx.call("vt_vae_optim_norm", ptrs, numel, 64, 1e30, vp(sc_e.data_ptr()), vp((ws.data_ptr() + 255) // 256 * 256), need, 0, stream())
    sq_e = np.frombuffer(scalars16(sc_e), np.float64)[0]
    assert 0 < sq_e < sq_v
    joint(ft, grads, 64, 1e30, 0, scalars)
    prefix = scalars16(scalars)
    joint(ft, enc, 64, 1e30, 5, scalars)
    assert prefix == scalars16(scalars) == train_full.joint_clip_host(sq_e, sq_d, 1e30) != seen[0]
    # a bound below the measured norm: it clips
    norm = float(np.frombuffer(seen[0][8:12], np.float32)[0])
    bound = 0.5 * norm
    before_v = {k: g.clone() for k, g in grads.items()}
    before_d = [{k: b.gradient(k) for k in b.shapes} for b in ft.blocks]
    joint(ft, grads, 152, bound, 0, scalars)
    got = scalars16(scalars)
    assert got == train_full.joint_clip_host(sq_v, sq_d, bound) and all(block_scalars(b) == got for b in ft.blocks)
    coef = np.frombuffer(got[12:], np.float32)[0]
    assert 0.49 < coef < 0.51
    assert all(torch.equal(g, before_v[k]) for k, g in grads.items())                           # the VAE's gradients are not written
    for b, before in zip(ft.blocks, before_d):
        for k, g in before.items():
            assert torch.equal(b.gradient(k), torch.from_numpy(g.numpy() * coef)), k                # g * coef, one fp32 multiply
    # ... and the coefficient is neither separate clip's (what two clips would have applied)
    ft.vae.clip(grads, bound)
    coef_v = np.frombuffer(scalars16(ft.vae._scalars)[12:], np.float32)[0]
    coef_d = np.frombuffer(train_full.joint_clip_host(0.0, sq_d, bound)[12:], np.float32)[0]     # (vt_train_clip's formula on the measured S_blocks)
    print(f"  {kind}: joint coef {coef!r}, the VAE's alone {coef_v!r}, the decoder's alone {coef_d!r}")
    assert coef != coef_v and coef != coef_d and coef < min(coef_v, coef_d)


def test_joint_norm_refusals_name_the_entry(case):
    ft = make(case, "attention", simplified=False)
    grads, _ = forward_backwards(ft, case)
    scalars = torch.zeros(2, dtype=torch.float64, device=DEV)
    ptrs, numel, ws = joint(ft, grads, 152, 1e30, 0, scalars)
    ptr, need = (ws.data_ptr() + 255) // 256 * 256, ws.numel() - 256
    call = lambda *a: ft.head.ctx.call("vt_full_optim_norm", *a)
    head, front = ft.blocks[0]._state(), ft.blocks[1]._state()
    good = [ptrs, numel, 152, 1.0, vp(scalars.data_ptr()), vp(ptr), need, 0, *head, *front, None, 0, stream()]
    bad = {"max_norm": (3, 0.0), "chunk": (7, 65), "n": (2, 0), "workspace": (6, 8), "head": (9, head[1] - 256), "front": (11, 16),
           "scalars": (4, vp(scalars.data_ptr() + 8))}
    scalars.zero_()
    for what, (i, v) in bad.items():
        args = list(good)
        args[i] = v
        with pytest.raises(_lib.VTError, match="vt_full_optim_norm"):
            call(*args)
    with pytest.raises(_lib.VTError, match="vt_full_optim_norm"):                                # a cross-attention block without the front's
        call(*good[:10], None, 0, *front, stream())
    assert scalars16(scalars) == bytes(16)                                                       # a refused call writes nothing
    plain = make(case, "plain", simplified=False)
    with pytest.raises(_lib.VTError, match="vt_full_optim_norm"):                                # the plain decoder has no front to clip
        plain.head.ctx.call("vt_full_optim_norm", *good[:8], *plain.blocks[0]._state(), *front, None, 0, stream())


# ---- 2. the mode latent --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C, h, w", [(16, 2, 3), (16, 5, 7), (3, 5, 7), (16, 40, 40)])      # float4 path; D = 105: one float at a time; 3 chunks
@pytest.mark.parametrize("has_s, has_t", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_mode_latent_is_torch_eager_bit_for_bit(C, h, w, has_s, has_t):
    ctx = vae_backward.context(torch.device(DEV))
    Bm, Bp = 2, 5                                                                              # the anchors of a larger encoder pass
    g = torch.Generator().manual_seed(C * 100 + h)
    moments = (torch.randn(Bp, 2 * C, h, w, generator=g) * 3.0).to(DEV)
    out = torch.full((Bm + 1, C, h, w), 7.0, device=DEV)
    ctx.call("vt_posterior_mode_latent", vp(moments.data_ptr()), Bm, C, h * w, SCALING, has_s, SHIFT, has_t, vp(out.data_ptr()), stream())
    want = moments[:Bm, :C]
    if has_s:
        want = want * SCALING
    if has_t:
        want = want + SHIFT
    torch.cuda.synchronize()
    assert torch.equal(out[:Bm], want) and bool((out[Bm] == 7.0).all())                         # nothing past the B-th image is written


def test_mode_latent_misaligned_and_refusals():
    ctx = vae_backward.context(torch.device(DEV))
    C, h, w = 16, 2, 3
    buf = torch.randn(2 * 2 * C * h * w + 1, device=DEV)
    out = torch.zeros(2 * C * h * w + 1, device=DEV)
    call = lambda *a: ctx.call("vt_posterior_mode_latent", *a)
    call(vp(buf.data_ptr() + 4), 2, C, h * w, SCALING, 1, SHIFT, 1, vp(out.data_ptr() + 4), stream())      # 4-B aligned only: the scalar path
    torch.cuda.synchronize()
    m = buf[1:].view(2, 2 * C, h, w)
    assert torch.equal(out[1:].view(2, C, h, w), m[:, :C] * SCALING + SHIFT) and float(out[0]) == 0.0
    good = [vp(buf.data_ptr()), 2, C, h * w, SCALING, 1, SHIFT, 1, vp(out.data_ptr()), stream()]
    for i, v in ((1, 0), (1, 1 << 20), (2, 0), (3, 0), (0, None), (8, None), (0, vp(buf.data_ptr() + 2)), (4, float("inf")), (6, float("nan"))):
        args = list(good)
        args[i] = v
        with pytest.raises(_lib.VTError, match="vt_posterior_mode_latent"):
            call(*args)
    call(*good[:4], float("inf"), 0, float("nan"), 0, *good[8:])                                 # a factor whose flag is off is not looked at


# ---- 3. the encoder-only step ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w_tri", [1.0, 0.37])
def test_encoder_only_step_is_the_full_step_at_reconstruction_weight_zero(case, w_tri):
    d = case["dev"]
    params = {k: v.to(DEV) for k, v in case["p"].items()}
    saved, moments = {}, []
    losses, grads = vae_backward.vae_triplet_loss_and_grads(params, d["a"], d["p"], d["n"], d["la"], d["lp"], triplet_weight=w_tri, margin=MARGIN,
                                                            similarity_type=SIM, seed=SEED, first_image=3, saved=saved, moments_out=moments)
    moments_full = []
    losses_f, grads_f = vae_backward.vae_loss_and_grads(params, d["a"], d["p"], d["n"], d["la"], d["lp"], margin=MARGIN, similarity_type=SIM,
                                                        weights={"reconstruction": 0.0, "kl": 0.0, "triplet": w_tri}, seed=SEED, first_image=3,
                                                        moments_out=moments_full)
    torch.cuda.synchronize()
    assert "decoder" not in saved and set(saved) == {"encoder", "moments"}                       # no decode was launched
    assert list(grads) == [k for k in params if k.startswith("encoder.")] and len(grads) == 64
    assert torch.equal(losses["triplet"], losses_f["triplet"]) and torch.equal(losses["total"], losses_f["total"]) and float(losses["triplet"]) > 0
    assert torch.equal(losses["kl"], losses_f["kl"]) and float(losses["reconstruction"]) == 0.0
    for k, g in grads.items():
        assert torch.equal(g, grads_f[k]), k
    assert all(not bool(grads_f[k].any()) for k in grads_f if k.startswith("decoder."))          # exact zeros there, not absent
    assert len(moments) == 1 and torch.equal(moments[0], moments_full[0]) and tuple(moments[0].shape) == (3 * B, 2 * LATENT, H >> 2, W >> 2)
    # the default call of vae_loss_and_grads is unchanged by the new keyword
    losses_d, grads_d = vae_backward.vae_loss_and_grads(params, d["a"], d["p"], d["n"], d["la"], d["lp"], margin=MARGIN, similarity_type=SIM,
                                                        weights={"reconstruction": 0.0, "kl": 0.0, "triplet": w_tri}, seed=SEED, first_image=3)
    assert all(torch.equal(grads_d[k], grads_f[k]) for k in grads_f) and all(torch.equal(losses_d[k], losses_f[k]) for k in losses_f)


# ---- 4. the step's composition -----------------------------------------------------------------------------------------------------------------
def by_hand(case, ft, *, joint_clip, max_norm=MAX_NORM, first=0):
    """one step on ft's arenas and blocks through the entry points alone (ft.train_step is not called)"""
    v, d = ft.vae, case["dev"]
    if ft.simplified:
        losses, grads = vae_backward.vae_triplet_loss_and_grads(v.params, d["a"], d["p"], d["n"], d["la"], d["lp"], triplet_weight=1.0, margin=MARGIN,
                                                                similarity_type=SIM, seed=SEED, first_image=first)
        moments = vae_backward.encoder_forward_train({k: p for k, p in v.params.items() if k.startswith("encoder.")}, torch.cat([d["a"], d["p"], d["n"]]))[0]
    else:
        keep = []
        losses, grads = vae_backward.vae_loss_and_grads(v.params, d["a"], d["p"], d["n"], d["la"], d["lp"], margin=MARGIN, similarity_type=SIM, seed=SEED,
                                                        weights={k: FULL[k] for k in ("reconstruction", "kl", "triplet")}, first_image=first, moments_out=keep)
        moments = keep[0]
    latent = torch.empty(B, LATENT, H >> 2, W >> 2, device=DEV)
    v.ctx.call("vt_posterior_mode_latent", vp(moments.data_ptr()), B, LATENT, latent[0, 0].numel(), SCALING, 1, SHIFT, 1, vp(latent.data_ptr()), stream())
    if isinstance(ft.dec, DecoderTrainer):
        ft.dec.forward_backward(latent, d["la"], loss_scale=FULL["classification"], train=True, step=ft.t)
    else:
        ft.dec.forward_backward(ft.dec.features(latent), d["la"], loss_scale=FULL["classification"], train=True, step=ft.t)
    n = len(grads)
    ptrs = (vp * n)(*[g.data_ptr() for g in grads.values()])
    numel = (ctypes.c_longlong * n)(*[g.numel() for g in grads.values()])
    scalars = None
    if max_norm > 0:
        scalars = torch.zeros(2, dtype=torch.float64, device=DEV)
        if joint_clip:
            joint(ft, grads, n, max_norm, 0, scalars)
        else:
            need = v.ctx.lib.vt_vae_optim_workspace_bytes(numel, n)
            ws = torch.zeros(need + 256, dtype=torch.uint8, device=DEV)
            v.ctx.call("vt_vae_optim_norm", ptrs, numel, n, max_norm, vp(scalars.data_ptr()), vp((ws.data_ptr() + 255) // 256 * 256), need, 0, stream())
            ft.dec.clip(max_norm)
    v.ctx.call("vt_vae_optim_step", *(vp(a.data_ptr()) for a in v._arena), v.total, ptrs, numel, n, vp(scalars.data_ptr()) if scalars is not None else None,
               LR, 0.9, 0.999, 1e-8, WD, ft.t + 1, 0, stream())
    ft.dec.step(LR, WD)
    ft.t += 1
    return losses


@pytest.mark.parametrize("simplified", [True, False], ids=["simplified", "full"])
@pytest.mark.parametrize("kind", KINDS)
def test_train_step_is_the_step_by_hand_under_one_clip(case, kind, simplified):
    a, b, c = (make(case, kind, simplified) for _ in range(3))
    start = arenas(a)
    losses = a.train_step(*batch(case, 0), lr=LR, weight_decay=WD, max_grad_norm=MAX_NORM)
    hand = by_hand(case, b, joint_clip=True)
    norm, coef = a.grad_norm()
    print(f"  {kind} {'simplified' if simplified else 'full'}: joint norm {norm:.6g}, coef {coef:.6g}")
    assert coef < 1.0, "the case must clip"
    assert all(torch.equal(x, y) for x, y in zip(arenas(a), arenas(b)))
    assert all(torch.equal(x, y) for x, y in zip(block_bytes(a), block_bytes(b)))
    assert torch.equal(losses["triplet"], hand["triplet"]) and float(losses["classification"]) > 0
    assert float(losses["total"]) == float(hand["total"]) + float(losses["classification"])
    assert a.t == a.vae.t == 1 and all(blk.t == 1 for blk in a.blocks)
    # two separate clips are another optimiser
    by_hand(case, c, joint_clip=False)
    assert not torch.equal(arenas(a)[0], arenas(c)[0]) and not any(torch.equal(x, y) for x, y in zip(block_bytes(a), block_bytes(c)))
    if simplified:
        lo = a.vae.offsets[a.n_encoder]
        assert all(torch.equal(x[lo:], s[lo:]) for x, s in zip(arenas(a), start))                # decoder.*: params, m and v untouched


@pytest.mark.parametrize("kind", ["attention", "plain"])
def test_without_a_bound_the_step_is_the_plain_steps(case, kind):
    a, b, c = (make(case, kind, False) for _ in range(3))
    a.train_step(*batch(case, 0), lr=LR, weight_decay=WD, max_grad_norm=0.0)
    by_hand(case, b, joint_clip=True, max_norm=0.0)
    c.train_step(*batch(case, 0), lr=LR, weight_decay=WD, max_grad_norm=MAX_NORM)
    assert all(torch.equal(x, y) for x, y in zip(arenas(a), arenas(b))) and all(torch.equal(x, y) for x, y in zip(block_bytes(a), block_bytes(b)))
    assert not torch.equal(arenas(a)[0], arenas(c)[0])


@pytest.mark.parametrize("kind", KINDS)
def test_simplified_loss_leaves_the_image_decoder_alone_under_weight_decay(case, kind):
    ft = make(case, kind, True)
    start = arenas(ft)
    start_blocks = [{k: b.parameter(k) for k in b.shapes} for b in ft.blocks]
    for k in range(3):
        ft.train_step(*batch(case, k * B), lr=LR, weight_decay=1e-2, max_grad_norm=MAX_NORM)
    now = arenas(ft)
    lo = ft.vae.offsets[ft.n_encoder]
    assert ft.n == ft.n_encoder == 64 and lo == sum((n + 4095) // 4096 * 4096 for n in ft.vae.numels[:64])
    for x, s in zip(now, start):
        assert torch.equal(x[lo:], s[lo:])                                                      # all three arenas: bit-unchanged
    for i, (k, off, n) in enumerate(zip(ft.vae.params, ft.vae.offsets, ft.vae.numels)):
        if i < 64:
            assert not torch.equal(now[0][off:off + n], start[0][off:off + n]), k                # every encoder.* tensor has moved
    for b, before in zip(ft.blocks, start_blocks):
        for k, v in before.items():
            assert not torch.equal(b.parameter(k), v), k                                        # and every tensor of every decoder-side block


# ---- 5. a resume through files -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, simplified", [("cross", True), ("attention", False), ("plain", True)])
def test_resume_through_files_gives_the_same_bits(case, kind, simplified, tmp_path):
    kw = dict(lr=LR, weight_decay=WD, max_grad_norm=MAX_NORM)
    straight = make(case, kind, simplified)
    losses_a = [straight.train_step(*batch(case, k * B), **kw) for k in range(4)]
    first = make(case, kind, simplified)
    losses_b = [first.train_step(*batch(case, k * B), **kw) for k in range(2)]
    first.save(str(tmp_path / "ckpt"), {"note": "test"})
    del first
    second = make(case, kind, simplified)
    second.load(str(tmp_path / "ckpt"))
    assert second.t == second.vae.t == 2 and all(b.t == 2 for b in second.blocks)
    losses_b += [second.train_step(*batch(case, k * B), **kw) for k in range(2, 4)]
    assert all(torch.equal(x, y) for x, y in zip(arenas(straight), arenas(second)))
    for x, y in zip(straight.blocks, second.blocks):
        for name in x.shapes:
            for kind_, _ in train_full._KINDS:
                assert torch.equal(x._read(kind_, name, x.shapes[name], torch.float32), y._read(kind_, name, y.shapes[name], torch.float32)), name
        for name in getattr(x, "buffers", {}):
            assert torch.equal(x.buffer(name), y.buffer(name)), name
    assert all(torch.equal(la[k], lb[k]) for la, lb in zip(losses_a, losses_b) for k in la)
    assert straight.state_sha256() == second.state_sha256() and straight.t == second.t == 4


# ---- 6. learning ---------------------------------------------------------------------------------------------------------------------------
K_LEARN = 8


def device_eps(ctx, first, draw):
    """the device's own draw: vt_posterior_sample on all-zero moments has std exactly 1, so z is eps"""
    h, w = H >> 2, W >> 2
    zero = torch.zeros(B, 2 * LATENT, h, w, device=DEV)
    z = torch.empty(B, LATENT, h, w, device=DEV)
    ctx.call("vt_posterior_sample", vp(zero.data_ptr()), B, LATENT, h * w, SEED, draw, first, vp(z.data_ptr()), None, None)
    torch.cuda.synchronize()
    return z.cpu()


def test_the_device_learns_at_least_half_of_what_the_reference_learns(case):
    """The CPU reference's total (triplet + classification) before steps 0 .. 8, K = 8 steps, weight decay 1e-6, clip at 1.0 (first joint norm 9.16):
        lr 1e-4: 2.0714 1.9888 1.8275 1.4436 1.3334 0.9200 0.6068 0.3854 0.3627
        lr 3e-4: 2.0714 1.9163 1.7943 1.4318 1.0054 0.3390 0.3146 0.2913 0.2697      (falls by 1.8017 = 87 % of its start; monotone)
        lr 1e-3: 2.0714 1.8624 2.1508 1.6086 2.2019 1.8740 1.6488 1.4491 1.0426      (not monotone: the triplet term follows each step's noise)
    With every gradient element multiplied by 1 + 0.02 N(0, 1) the lr 3e-4 trajectory moved by at most 5e-4 (0.2697 -> 0.2702 at its end) -- far more
    than bf16 operands perturb a gradient, and nothing beside a fall of 1.80.  K = 8 and lr = 3e-4 it is: the triplet term reaches 0 after five steps
    and what is left is the classification term (0.7444 -> 0.2697).  The device has to fall by half as much: the margin of the VAE learning test, for
    the same reason (bf16 MFMA operands in the encoder; the decoder side is fp32).
    First device run, on its own eps: reference 2.0714 1.9163 1.7943 1.4318 1.0054 0.3390 0.3146 0.2913 0.2697,
                                      device    2.0707 1.9167 1.7934 1.4325 1.0054 0.3379 0.3122 0.2880 0.2667 (falls by 1.8040)."""
    from _vae_model_backward_ref import encoder_forward_ref
    from test_train_device import head_forward
    from test_train_front_device import RM, RV, front_forward
    weights = {"triplet": 1.0, "classification": 1.0}
    ft = make(case, "attention", True, weights=weights, dropout=(0.0, 0.0, 0.0), attention_dropout=0.0)
    # the reference trajectory: fp32 autograd on the device's own eps, clip_grad_norm_ over both models, ONE torch.optim.AdamW
    sd = decoder(case, "attention")[1]
    p = {k: v.clone().requires_grad_(True) for k, v in case["p"].items()}
    trainable = [k for k in p if k.startswith("encoder.")]                                      # the image decoder has grad None: not in the optimiser
    pd = {k: v.clone().float().requires_grad_(True) for k, v in sd.items() if k not in (RM, RV) and v.is_floating_point()}
    rm, rv = sd[RM].clone(), sd[RV].clone()
    params = [p[k] for k in trainable] + list(pd.values())
    opt = torch.optim.AdamW(params, lr=LR, weight_decay=WD)
    vae_weights = {"reconstruction": 0.0, "kl": 0.0, "triplet": 1.0}
    ref = []
    for k in range(K_LEARN + 1):
        eps = [device_eps(ft.vae.ctx, k * B, d) for d in range(4)]
        now = {n: v.detach() for n, v in p.items()}
        losses, grads = step_autograd(now, case["images"], eps, case["labels"], vae_weights, MARGIN, SIM)
        with torch.no_grad():
            moments, _ = encoder_forward_ref(_sub(now, "encoder."), case["images"][:B])
            latent = moments[:, :LATENT] * SCALING + SHIFT
        cls = F.binary_cross_entropy_with_logits(head_forward(pd, front_forward(pd, latent, (1, 1, 8), True, rm, rv), False), case["labels"][0])
        ref.append(float(losses["total"]) + float(cls.detach()))
        if k < K_LEARN:
            gd = torch.autograd.grad(cls, list(pd.values()))
            for n in trainable:
                p[n].grad = grads[n]
            for v, g in zip(pd.values(), gd):
                v.grad = g
            torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
            opt.step()
    dev = [ft.train_step(*batch(case, k * B), lr=LR, weight_decay=WD, max_grad_norm=MAX_NORM)["total"] for k in range(K_LEARN)]
    losses, _, moments = ft.vae_forward_backward(*batch(case, K_LEARN * B))
    dev.append(losses["total"] + ft.decoder_forward_backward(ft.mode_latent(moments, B), case["dev"]["la"], ft.t))
    dev = [float(v) for v in torch.stack(dev).cpu()]
    print("  reference total: " + " ".join(f"{v:.4f}" for v in ref))
    print("  device total:    " + " ".join(f"{v:.4f}" for v in dev))
    ref_fall, dev_fall = ref[0] - ref[K_LEARN], dev[0] - dev[K_LEARN]
    assert ref_fall >= 0.10 * ref[0], "the reference itself must fall by at least 10 % of its start"
    assert all(x > y for x, y in zip(ref, ref[1:])), "the reference falls monotonically"
    assert all(math.isfinite(v) for v in dev) and ft.vae.ctx.status() == 0
    assert dev_fall >= 0.5 * ref_fall, f"the device fell by {dev_fall:.4f}, the reference by {ref_fall:.4f}"
