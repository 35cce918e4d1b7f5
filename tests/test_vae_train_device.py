"""VAETrainer on the device, on the small case of tests/_vae_train_step_ref.py (block_out (64, 128, 512), one layer per block, B = 2, 16 x 24, 152
tensors): the parameter views, the composition of a train step from the two entry points, a resume through files, and learning against a CPU
trajectory.

The learning case, chosen on the CPU before any device run.  One fixed batch, the noise of step k keyed on first_image = k B, weights
reconstruction 1 / kl 1e-2 / triplet 1, margin 1, cosine, clip at 1.0, AdamW at a constant lr with weight decay 1e-6.  The fp32 reference
(step_autograd + clip_grad_norm_ + torch.optim.AdamW on the host mirror of the device's eps) gave, for the total before steps 0 .. 8:
    lr 3e-4: 1.7586 1.6919 1.6525 1.2795 0.8381 0.3482 0.3436 0.3403 0.3301      (falls by 1.4285 = 81 % of its start; monotone)
    lr 5e-4: 1.7586 1.7362 1.7864 1.5514 1.2240 0.3511 0.3434 0.3367 0.3350
    lr 1e-3: 1.7586 1.8066 2.0828 1.5770 2.0153 1.6170 1.2661 0.6418 0.9816      (not monotone: the triplet term follows each step's noise)
and the lr 3e-4 trajectory moved by less than 2e-4 when every gradient element was perturbed by a relative 2 % -- far more than bf16 operands do.
K = 8 and lr = 3e-4 it is: the triplet term reaches 0 and what is left is the reconstruction.  The device has to fall by half as much.
(First device run, on its own eps: reference 1.7586 ... 0.3301, device 1.7588 1.6921 1.6525 1.2789 0.8364 0.3471 0.3436 0.3403 0.3299.)"""
import ctypes
import math

import pytest
import torch

from _vae_train_step_ref import LATENT, MARGIN, N_LABELS, SIM, SMALL, WEIGHTS, step_autograd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H, W, SEED = 2, 16, 24, 77
K, LR, WD, MAX_NORM = 8, 3e-4, 1e-6, 1.0


@pytest.fixture(scope="module")
def case():
    from vae_tagger_amd import synth
    p = synth.synth_state_dict({**synth.encoder_manifest(**SMALL), **synth.image_decoder_manifest(**SMALL)}, seed=5)
    images = synth.synth_images(3 * B, H, W, seed=6)
    g = torch.Generator().manual_seed(8)
    labels = tuple((torch.rand(B, N_LABELS, generator=g) < 0.5).float() for _ in range(2))
    labels[0][:, 0] = 1.0
    dev = dict(a=images[:B].to(DEV).contiguous(), p=images[B:2 * B].to(DEV).contiguous(), n=images[2 * B:].to(DEV).contiguous(),
               la=labels[0].to(DEV), lp=labels[1].to(DEV))
    return dict(p=p, images=images, labels=labels, dev=dev)


def make_trainer(case, params=None):
    from vae_tagger_amd import train_vae
    return train_vae.VAETrainer(params if params is not None else case["p"], weights=WEIGHTS, margin=MARGIN, similarity_type=SIM, seed=SEED, device=DEV)


def batch(case, first):
    d = case["dev"]
    return (d["a"], d["p"], d["n"], d["la"], d["lp"], first)


def arenas(tr):
    torch.cuda.synchronize()
    return [a.clone() for a in tr._arena]


def test_params_are_views_and_forward_backward_reads_them(case):
    from vae_tagger_amd import vae_backward
    tr = make_trainer(case)
    assert list(tr.params) == list(case["p"]) and len(tr.params) == 152
    for (k, v), off, n in zip(tr.params.items(), tr.offsets, tr.numels):
        assert v.data_ptr() == tr._arena[0].data_ptr() + 4 * off and v.is_contiguous() and v.dtype == torch.float32
        assert tuple(v.shape) == tuple(case["p"][k].shape) and v.numel() == n and torch.equal(v.cpu(), case["p"][k])
    assert tr._arena[0].data_ptr() % 256 == 0
    losses, grads = tr.forward_backward(*batch(case, 3))
    clones = {k: v.clone() for k, v in tr.params.items()}
    d = case["dev"]
    losses2, grads2 = vae_backward.vae_loss_and_grads(clones, d["a"], d["p"], d["n"], d["la"], d["lp"], weights=WEIGHTS, margin=MARGIN,
                                                      similarity_type=SIM, seed=SEED, first_image=3)
    torch.cuda.synchronize()
    assert list(grads) == list(tr.params)
    assert all(torch.equal(grads[k], grads2[k]) for k in grads) and all(torch.equal(losses[k], losses2[k]) for k in losses)
    assert tr.saved_bytes(d["a"].shape) == vae_backward.vae_train_saved_bytes(SMALL, B, H, W)
    # a write through the view is what the next step reads
    tr.params["decoder.conv_out.bias"].add_(1.0)
    losses3, _ = tr.forward_backward(*batch(case, 3))
    assert float(losses3["reconstruction"]) != float(losses["reconstruction"])


def test_train_step_is_norm_then_step_by_hand(case):
    tr = make_trainer(case)
    _, grads = tr.forward_backward(*batch(case, 0))
    tr.train_step(*batch(case, 0), lr=LR, weight_decay=WD, max_grad_norm=MAX_NORM)
    got = arenas(tr)
    norm, coef = tr.grad_norm()
    norm64 = math.sqrt(sum((g.double() ** 2).sum().item() for g in grads.values()))
    print(f"  grad norm {norm:.6g} (fp64 {norm64:.6g}), coef {coef:.6g}")
    assert abs(norm - norm64) <= 1e-6 * norm64 and coef < 1.0, "the case must clip"
    # by hand, through the C ABI, on a second trainer's arenas
    other = make_trainer(case)
    ctx, n = other.ctx, len(other.numels)
    vp = ctypes.c_void_p
    ptrs = (vp * n)(*[g.data_ptr() for g in grads.values()])
    numel = (ctypes.c_longlong * n)(*other.numels)
    need = ctx.lib.vt_vae_optim_workspace_bytes(numel, n)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    scalars = torch.zeros(2, dtype=torch.float64, device=DEV)
    stream = vp(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    ctx.call("vt_vae_optim_norm", ptrs, numel, n, MAX_NORM, vp(scalars.data_ptr()), vp(ws.data_ptr()), need, 0, stream)
    ctx.call("vt_vae_optim_step", *(vp(a.data_ptr()) for a in other._arena), other.total, ptrs, numel, n, vp(scalars.data_ptr()), LR, 0.9, 0.999, 1e-8,
             WD, 1, 0, stream)
    want = arenas(other)
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    assert torch.equal(scalars.cpu(), tr._scalars.cpu())
    # without a clip the scalars are not read: max_grad_norm = 0 is the plain step
    plain, by_hand = make_trainer(case), make_trainer(case)
    plain.train_step(*batch(case, 0), lr=LR, weight_decay=WD, max_grad_norm=0.0)
    by_hand.step(grads, LR, WD)
    assert all(torch.equal(x, y) for x, y in zip(arenas(plain), arenas(by_hand))) and not torch.equal(arenas(plain)[0], got[0])
    assert plain.t == by_hand.t == 1


def test_resume_through_files_gives_the_same_bits(case, tmp_path):
    from safetensors.torch import load_file, save_file
    from vae_tagger_amd import train_vae
    kw = dict(lr=LR, weight_decay=WD, max_grad_norm=MAX_NORM)
    straight = make_trainer(case)
    losses_a = [straight.train_step(*batch(case, k * B), **kw) for k in range(4)]
    first = make_trainer(case)
    losses_b = [first.train_step(*batch(case, k * B), **kw) for k in range(2)]
    save_file({k: v.cpu().contiguous() for k, v in first.state_dict().items()}, str(tmp_path / "model.safetensors"))
    train_vae.save_optimizer_state(str(tmp_path / "optimizer.safetensors"), first.optimizer_state_dict())
    del first
    second = make_trainer(case, load_file(str(tmp_path / "model.safetensors")))
    second.load_optimizer_state_dict(train_vae.load_optimizer_state(str(tmp_path / "optimizer.safetensors")))
    assert second.t == 2
    losses_b += [second.train_step(*batch(case, k * B), **kw) for k in range(2, 4)]
    assert all(torch.equal(x, y) for x, y in zip(arenas(straight), arenas(second)))
    assert all(torch.equal(la[k], lb[k]) for la, lb in zip(losses_a, losses_b) for k in la)
    assert straight.optimizer_state_sha256().hexdigest() == second.optimizer_state_sha256().hexdigest() and straight.t == second.t == 4


def device_eps(ctx, first, draw):
    """the device's own draw: vt_posterior_sample on all-zero moments has std exactly 1, so z is eps"""
    h, w = H >> 2, W >> 2
    zero = torch.zeros(B, 2 * LATENT, h, w, device=DEV)
    z = torch.empty(B, LATENT, h, w, device=DEV)
    ctx.call("vt_posterior_sample", ctypes.c_void_p(zero.data_ptr()), B, LATENT, h * w, SEED, draw, first, ctypes.c_void_p(z.data_ptr()), None, None)
    torch.cuda.synchronize()
    return z.cpu()


def test_the_device_learns_at_least_half_of_what_the_reference_learns(case):
    tr = make_trainer(case)
    # the reference trajectory: fp32 autograd on the device's own eps, clip_grad_norm_, torch.optim.AdamW
    p = {k: v.clone().requires_grad_(True) for k, v in case["p"].items()}
    params = list(p.values())
    opt = torch.optim.AdamW(params, lr=LR, weight_decay=WD)
    ref = []
    for k in range(K + 1):
        eps = [device_eps(tr.ctx, k * B, d) for d in range(4)]
        losses, grads = step_autograd({n: v.detach() for n, v in p.items()}, case["images"], eps, case["labels"], WEIGHTS, MARGIN, SIM)
        ref.append(float(losses["total"]))
        if k < K:
            for n in p:
                p[n].grad = grads[n]
            torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
            opt.step()
    dev = [tr.train_step(*batch(case, k * B), lr=LR, weight_decay=WD, max_grad_norm=MAX_NORM)["total"] for k in range(K)]
    dev.append(tr.forward_backward(*batch(case, K * B))[0]["total"])
    dev = [float(v) for v in torch.stack(dev).cpu()]
    print("  reference total: " + " ".join(f"{v:.4f}" for v in ref))
    print("  device total:    " + " ".join(f"{v:.4f}" for v in dev))
    ref_fall, dev_fall = ref[0] - ref[K], dev[0] - dev[K]
    assert ref_fall >= 0.10 * ref[0], "the reference itself must fall by at least 10 % of its start"
    assert all(math.isfinite(v) for v in dev) and tr.ctx.status() == 0
    assert dev_fall >= 0.5 * ref_fall, f"the device fell by {dev_fall:.4f}, the reference by {ref_fall:.4f}"
