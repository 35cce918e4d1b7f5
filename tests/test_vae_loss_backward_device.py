"""vt_vae_loss_backward on the device: every output against torch fp64 autograd of the restated loss (tests/_vae_loss_backward_ref.py) fed the
device's own eps and the forward's own z, the exact cases, the bits it shares with vt_vae_loss_update, determinism across runs and across the vector and the scalar
path, and the refusals."""
import ctypes

import numpy as np
import pytest
import torch

import _vae_loss_backward_ref as ref
from vae_tagger_amd import _lib, vae_losses

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (C, h, w): D = 96 (float4 path, one chunk), 15 (scalar path), 4112 (crosses the 4096-element chunk); (H, W): E = 192 and 4107 (crosses a chunk, scalar)
LATENTS = {"D96": (16, 2, 3), "D15": (3, 1, 5), "D4112": (16, 1, 257)}
IMAGES = {"D96": (8, 8), "D15": (37, 37), "D4112": (37, 37)}
FULL = {"reconstruction": 0.01, "kl": 1e-2, "triplet": 1.0}
DRAWS = (1, 2, 3)
SEED, FIRST = 12345, 7


@pytest.fixture(scope="module")
def ctx():
    return _lib.Context(0)


def device_eps(ctx, B, C, h, w, draw, seed=SEED, first=FIRST):
    """the device's own draw: vt_posterior_sample on all-zero moments has std exactly 1, so z is eps"""
    zero = torch.zeros(B, 2 * C, h, w, device=DEV)
    z = torch.empty(B, C, h, w, device=DEV)
    ctx.call("vt_posterior_sample", ctypes.c_void_p(zero.data_ptr()), B, C, h * w, seed, draw, first, ctypes.c_void_p(z.data_ptr()), None, None)
    torch.cuda.synchronize()
    return z.cpu().numpy()


def device_z(ctx, c):
    """the three streams' z as the device's forward forms them: vt_posterior_sample on the moments themselves"""
    out = []
    for m, d in zip(c["moments"], DRAWS):
        B, C2, h, w = m.shape
        t, z = torch.from_numpy(m).to(DEV), torch.empty(B, C2 // 2, h, w, device=DEV)
        ctx.call("vt_posterior_sample", ctypes.c_void_p(t.data_ptr()), B, C2 // 2, h * w, SEED, d, FIRST, ctypes.c_void_p(z.data_ptr()), None, None)
        torch.cuda.synchronize()
        out.append(z.cpu().numpy())
    return out


def dev(x, offset=0):
    """a contiguous device copy of a numpy array, `offset` floats past a 16-byte boundary"""
    if x is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(x))
    if not offset:
        return t.to(DEV)
    buf = torch.empty(t.numel() + offset, dtype=t.dtype, device=DEV)
    buf[offset:].copy_(t.reshape(-1))
    return buf[offset:].view(t.shape)


def run(ctx, c, *, weights=FULL, margin=1.0, sim="cosine", dz=True, offset=0, image=True, labels=True, want=("d_recon", "d_moments", "rows", "loss")):
    """one call -> dict of numpy outputs"""
    B = c["moments"][0].shape[0]
    m = [dev(x, offset) for x in c["moments"]]
    recon, target = (dev(c["recon"], offset), dev(c["target"], offset)) if image and c["recon"] is not None else (None, None)
    out = {"d_recon": dev(np.full(c["recon"].shape, 7.0, np.float32), offset) if recon is not None and "d_recon" in want else None,
           "d_moments": [dev(np.full(x.shape, 7.0, np.float32), offset) for x in c["moments"]] if "d_moments" in want else None,
           "rows": torch.full((B, vae_losses.ROW), 7.0, dtype=torch.float64, device=DEV) if "rows" in want else None,
           "loss": torch.full((4,), 7.0, dtype=torch.float64, device=DEV) if "loss" in want else None}
    vae_losses.loss_backward_device(*zip(m, DRAWS), weights=weights, margin=margin, similarity_type=sim, seed=SEED, first_image=FIRST,
                                    dz_dec=dev(c["dz_dec"], offset) if dz else None, dz_draw=0, recon=recon, target=target,
                                    labels_a=dev(c["labels_a"]) if labels else None, labels_p=dev(c["labels_p"]) if labels else None,
                                    d_recon=out["d_recon"], d_moments=out["d_moments"], rows_out=out["rows"], loss_out=out["loss"], context=ctx)
    torch.cuda.synchronize()
    return {k: ([t.cpu().numpy() for t in v] if isinstance(v, list) else None if v is None else v.cpu().numpy()) for k, v in out.items()}


def within(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err, bound = np.abs(got - want), ref.bound_fp32_store(want)
    worst = np.argmax(err - bound)
    print(f"    {what}: max |d| {err.max():.3e}  max |ref| {np.abs(want).max():.3e}  worst |d| / bound {err.flat[worst] / max(bound.flat[worst], 1e-300):.3f}")
    assert (err <= bound).all(), what


@pytest.mark.parametrize("sim", ["cosine", "euclidean"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", list(LATENTS))
def test_against_fp64_autograd(ctx, shape, B, sim):
    """every element within 2^-23 |ref| + 2^-40 max |ref|: fp64 arithmetic and one rounding to fp32"""
    (C, h, w), (H, W) = LATENTS[shape], IMAGES[shape]
    eps = [device_eps(ctx, B, C, h, w, d) for d in DRAWS + (0,)]
    for labels_dtype, weights, margin in ((np.float32, FULL, 1.0), (np.uint8, dict(FULL, kl=0.0), 0.7)):
        margin *= 1.0 if sim == "cosine" else 4.0
        c = ref.make_case(B, C, h, w, H, W, 9, seed=B + len(shape), labels_dtype=labels_dtype)
        got = run(ctx, c, weights=weights, margin=margin, sim=sim)
        want = ref.autograd(c["moments"], eps[:3], eps_dec=eps[3], weights=weights, margin=margin, similarity_type=sim, dz_dec=c["dz_dec"],
                            recon=c["recon"], target=c["target"], labels_a=c["labels_a"], labels_p=c["labels_p"], z_forward=device_z(ctx, c))
        for s in range(3):
            within(got["d_moments"][s], want["d_moments"][s], f"d_moments[{s}]")
        within(got["d_recon"], want["d_recon"], "d_recon")
        assert np.abs(got["loss"] - want["losses"]).max() <= 1e-12 * np.abs(want["losses"]).max()          # fp64 on both sides
    # without labels, without the decoder's gradient
    got = run(ctx, c, sim=sim, margin=margin, labels=False, dz=False, want=("d_moments",))
    want = ref.autograd(c["moments"], eps[:3], weights=FULL, margin=margin, similarity_type=sim, recon=c["recon"], target=c["target"],
                        z_forward=device_z(ctx, c))
    for s in range(3):
        within(got["d_moments"][s], want["d_moments"][s], f"d_moments[{s}] without labels and dz_dec")


def test_forward_z_is_one_fused_multiply_add(ctx):
    """vt_posterior_sample's z is fma(fp32(std), eps, mean) rounded once -- bit for bit vae_losses.forward_z, the exact model -- and differs from
    the two-rounding form in some elements, so the check tells the two apart"""
    B, (C, h, w) = 3, LATENTS["D4112"]
    c = ref.make_case(B, C, h, w, seed=50)
    eps = device_eps(ctx, B, C, h, w, DRAWS[0])
    m = c["moments"][0]
    std32 = np.exp(0.5 * np.clip(m[:, C:].astype(np.float64), -30.0, 20.0)).astype(np.float32)
    z = device_z(ctx, c)[0]
    differs = z != vae_losses.forward_z(m[:, :C], std32, eps)
    # (std is rounded from this host's exp; where the device's fp64 exp differs in its last bit AND that moves the fp32 rounding, an element may differ)
    assert differs.mean() <= 1e-3, f"{differs.sum()} of {differs.size} elements are not the fused form"
    assert (z != m[:, :C] + std32 * eps).mean() > 0.05


def test_exact_cases(ctx):
    B, (C, h, w) = 3, LATENTS["D96"]
    c = ref.make_case(B, C, h, w, 8, 8, 9, seed=4)
    for s, v in zip(range(3), (-31.0, 21.0, -30.0)):
        c["moments"][s][:, C, 0, 0] = v
    c["moments"][0][:, C + 1, 0, 1] = 20.0
    # a margin that leaves every triplet inactive: positive and negative keep only their KL part, the bits of w_tri = 0
    off = run(ctx, c, margin=-5.0)
    none = run(ctx, c, weights=dict(FULL, triplet=0.0))
    assert not off["rows"][:, 10].any() and off["loss"][2] == 0.0
    for s in (1, 2):
        assert np.array_equal(off["d_moments"][s], none["d_moments"][s])
    assert np.array_equal(off["d_moments"][0], none["d_moments"][0])
    # logvar at -31 and 21: exactly 0; at exactly -30 and 20: the unclamped formula (checked against autograd, and not 0)
    full = run(ctx, c)
    assert not full["d_moments"][0][:, C, 0, 0].any() and not full["d_moments"][1][:, C, 0, 0].any()
    eps = [device_eps(ctx, B, C, h, w, d) for d in DRAWS + (0,)]
    want = ref.autograd(c["moments"], eps[:3], eps_dec=eps[3], weights=FULL, dz_dec=c["dz_dec"], recon=c["recon"], target=c["target"],
                        labels_a=c["labels_a"], labels_p=c["labels_p"], z_forward=device_z(ctx, c))
    for s in range(3):
        within(full["d_moments"][s], want["d_moments"][s], f"d_moments[{s}] with logvar at and past the clamp")
    assert full["d_moments"][2][:, C, 0, 0].all() and full["d_moments"][0][:, C + 1, 0, 1].all()
    # everything off
    zero = run(ctx, c, weights={"reconstruction": 0.0, "kl": 0.0, "triplet": 0.0}, dz=False)
    assert all(not g.any() for g in zero["d_moments"]) and not zero["d_recon"].any()
    # w_rec = 0 alone
    assert not run(ctx, c, weights=dict(FULL, reconstruction=0.0), want=("d_recon",))["d_recon"].any()
    # a one-hot dz_dec with everything else off: d mean one-hot, d logvar = 0.5 std eps there (std the forward's fp32 one)
    hot = dict(c, dz_dec=np.zeros_like(c["dz_dec"]))
    at = [(0, 3, 1, 2), (1, 2, 0, 0), (2, C - 1, h - 1, w - 1)]
    for i in at:
        hot["dz_dec"][i] = 1.0
    got = run(ctx, hot, weights={"reconstruction": 0.0, "kl": 0.0, "triplet": 0.0})
    d_mean, d_lv = got["d_moments"][0][:, :C], got["d_moments"][0][:, C:]
    assert np.array_equal(d_mean, hot["dz_dec"])
    std32 = np.exp(0.5 * np.clip(c["moments"][0][:, C:].astype(np.float64), -30.0, 20.0)).astype(np.float32)
    expect = np.zeros_like(d_lv)
    for i in at:
        expect[i] = np.float32(0.5 * np.float64(std32[i]) * np.float64(eps[3][i]))
    assert np.array_equal(d_lv, expect) and all(expect[i] != 0.0 for i in at)
    assert not got["d_moments"][1].any() and not got["d_moments"][2].any()


@pytest.mark.parametrize("sim", ["cosine", "euclidean"])
@pytest.mark.parametrize("shape,B", [("D96", 3), ("D15", 1), ("D4112", 3)])
def test_rows_and_losses_are_the_forwards_bits(ctx, shape, B, sim):
    (C, h, w), (H, W) = LATENTS[shape], IMAGES[shape]
    c = ref.make_case(B, C, h, w, H, W, 9, seed=21)
    margin = 0.8 if sim == "cosine" else 3.0
    got = run(ctx, c, margin=margin, sim=sim, want=("rows", "loss"))
    acc = vae_losses.DeviceVAELossAccumulator(DEV, margin_triplet=margin, seed=SEED, context=ctx)
    rows = torch.empty(B, vae_losses.ROW, dtype=torch.float64, device=DEV)
    m = [dev(x) for x in c["moments"]]
    acc.update(*[(t, None, d) for t, d in zip(m, DRAWS)], recon=dev(c["recon"]), target=dev(c["target"]), labels_a=dev(c["labels_a"]),
               labels_p=dev(c["labels_p"]), first_image=FIRST, rows_out=rows)
    state = acc.read_state()
    rows = rows.cpu().numpy()
    both = [k for k in range(vae_losses.ROW) if k not in (12, 13)]          # (the contrastive columns are the forward's alone)
    assert np.array_equal(got["rows"][:, both], rows[:, both]) and not got["rows"][:, 12:14].any()
    assert rows[:, 10 if sim == "cosine" else 11].any(), "the case must have an active triplet"
    col = 10 if sim == "cosine" else 11
    in_order = lambda k: float(np.cumsum(got["rows"][:, k])[-1]) / B          # (cumsum adds one image after the other)
    loss = got["loss"]
    assert loss[0] == in_order(0) == state["batch_sums"][0]
    assert loss[1] == state["batch_sums"][2]                                  # log1p of the in-order kl_mean, by the same device function
    assert loss[2] == in_order(col) == state["batch_sums"][3 if sim == "cosine" else 4]
    assert loss[3] == FULL["reconstruction"] * loss[0] + FULL["kl"] * loss[1] + FULL["triplet"] * loss[2]


@pytest.mark.parametrize("sim", ["cosine", "euclidean"])
def test_bit_identical_across_runs_and_paths(ctx, sim):
    B, (C, h, w) = 3, LATENTS["D96"]
    c = ref.make_case(B, C, h, w, 8, 8, 9, seed=30)
    margin = 1.0 if sim == "cosine" else 4.0
    first, second, scalar = run(ctx, c, sim=sim, margin=margin), run(ctx, c, sim=sim, margin=margin), run(ctx, c, sim=sim, margin=margin, offset=1)
    for other in (second, scalar):
        assert all(np.array_equal(x, y) for x, y in zip(first["d_moments"], other["d_moments"]))
        assert np.array_equal(first["d_recon"], other["d_recon"]) and np.array_equal(first["rows"], other["rows"]) and np.array_equal(first["loss"], other["loss"])
    assert first["rows"][:, 10 if sim == "cosine" else 11].any() and all(g.any() for g in first["d_moments"])


def test_refusals(ctx):
    """the error, a message, and nothing written"""
    B, (C, h, w), H, W = 2, LATENTS["D96"], 8, 8
    c = ref.make_case(B, C, h, w, H, W, 9, seed=40)
    m = [dev(x) for x in c["moments"]]
    recon, target, dz = dev(c["recon"]), dev(c["target"]), dev(c["dz_dec"])
    la, lp = dev(c["labels_a"]), dev(c["labels_p"])
    SENT = 7.0
    outs = {"d_recon": torch.full_like(recon, SENT), "dm": torch.full((3,) + tuple(m[0].shape), SENT, device=DEV),
            "rows": torch.full((B, vae_losses.ROW), SENT, dtype=torch.float64, device=DEV), "loss": torch.full((4,), SENT, dtype=torch.float64, device=DEV)}
    need = ctx.lib.vt_vae_loss_backward_workspace_bytes(B, C, h * w, H, W)
    ws = torch.zeros(need + 512, dtype=torch.uint8, device=DEV)
    base = ws.data_ptr() + (-ws.data_ptr() % 256)
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    ins = [_lib.VAELossInput(t.data_ptr(), None, d) for t, d in zip(m, DRAWS)]

    def call(**over):
        a = dict(anchor=ctypes.byref(ins[0]), positive=ctypes.byref(ins[1]), negative=ctypes.byref(ins[2]), dz=vp(dz), dz_draw=0, recon=vp(recon),
                 target=vp(target), H=H, W=W, la=vp(la), lp=vp(lp), dt=_lib.VT_F32, N=la.shape[1], B=B, C=C, hw=h * w, seed=SEED, first=FIRST, w_rec=0.01,
                 w_kl=0.01, w_tri=1.0, margin=1.0, sim=_lib.VAE_COSINE, d_recon=vp(outs["d_recon"]), da=vp(outs["dm"][0]), dp=vp(outs["dm"][1]),
                 dn=vp(outs["dm"][2]), rows=vp(outs["rows"]), loss=vp(outs["loss"]), ws=ctypes.c_void_p(base), ws_bytes=need, stream=None)
        a.update(over)
        ctx.call("vt_vae_loss_backward", *a.values())

    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + n)
    no_moments = _lib.VAELossInput(None, None, 1)
    stored_z = _lib.VAELossInput(m[0].data_ptr(), m[0].data_ptr(), 1)
    odd = _lib.VAELossInput(m[0].data_ptr() + 2, None, 1)
    bad_draw = _lib.VAELossInput(m[0].data_ptr(), None, -1)
    refused = [
        ("required", dict(anchor=None)), ("required", dict(positive=None)), ("negative", dict(negative=None)),
        ("moments", dict(anchor=ctypes.byref(no_moments))), ("stored z", dict(anchor=ctypes.byref(stored_z))),
        ("misaligned", dict(positive=ctypes.byref(odd))), ("draw", dict(negative=ctypes.byref(bad_draw))), ("dz_draw", dict(dz_draw=-1)),
        ("first_image", dict(first=-1)), ("misaligned", dict(dz=off(dz, 2))), ("misaligned", dict(da=off(outs["dm"][0], 2))),
        ("misaligned", dict(recon=off(recon, 1))), ("misaligned", dict(d_recon=off(outs["d_recon"], 2))), ("misaligned", dict(rows=off(outs["rows"], 4))),
        ("misaligned", dict(loss=off(outs["loss"], 4))), ("misaligned", dict(la=off(la, 2))),
        ("together", dict(target=None)), ("needs recon", dict(recon=None, target=None)), ("together", dict(lp=None)),
        ("out of range", dict(B=0)), ("out of range", dict(B=4097)), ("out of range", dict(C=0)), ("out of range", dict(hw=0)),
        ("out of range", dict(H=0)), ("out of range", dict(W=-3)), ("labels", dict(dt=_lib.VT_BF16)), ("labels", dict(N=0)),
        ("finite", dict(w_rec=float("nan"))), ("finite", dict(w_kl=float("inf"))), ("finite", dict(w_tri=float("-inf"))), ("finite", dict(margin=float("nan"))),
        ("similarity", dict(sim=2)), ("workspace", dict(ws=None)), ("256-B aligned", dict(ws=ctypes.c_void_p(base + 8))),
        ("workspace holds", dict(ws_bytes=need - 1)), ("workspace holds", dict(ws_bytes=0)),
    ]
    for match, over in refused:
        with pytest.raises(_lib.VTError, match=match):
            call(**over)
    with pytest.raises(_lib.VTError, match=r"code 5"):
        call(ws_bytes=need - 1)
    torch.cuda.synchronize()
    assert all(bool((t == SENT).all()) for t in outs.values()), "a refused call wrote"
    call()                                                                   # the same arguments, accepted
    torch.cuda.synchronize()
    assert all(not bool((t == SENT).any()) for t in outs.values())
