"""vt_posterior_sample and vt_vae_loss_* on the GPU against the numpy fp64 mirrors: the draw and the fp32 arithmetic of z, the KL, every
scalar of the block and every entry of rows_out, the in-flight path against the given-z path bit for bit, reproducibility, batching
independence of the per-image sums, non-finite inputs, the error codes and the absence of host synchronisation."""
import ctypes
import os

import numpy as np
import pytest
import torch

from _vae_loss_util import measured_fp32_tolerance
from vae_tagger_amd import _lib, improved_losses as il, vae_losses
from vae_tagger_amd.autoencoder_kl import DiagonalGaussianDistribution
from vae_tagger_amd.vae_losses import DeviceVAELossAccumulator, HostVAELossState

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-9
SEQ = (3, 17, 1)
ROWS = sum(SEQ)
# latent (C, h, w) -> image (3, H, W) for the MSE: 1x1 and 2x3 are smaller than a wave, 33x17 is no multiple of anything, 64x64 = 16 chunks
SHAPES = {(16, 1, 1): (3, 8, 8), (16, 2, 3): (3, 16, 24), (16, 33, 17): (3, 264, 136), (16, 64, 64): (3, 264, 136)}
SHAPE_IDS = ["1x1", "2x3", "33x17", "64x64"]
SEED, MARGIN = 1234, 0.75


def _moments(rng, b, shape):
    c, h, w = shape
    m = rng.standard_normal((b, 2 * c, h, w)).astype(np.float32)
    m[:, c:] = m[:, c:] * np.float32(1.5) - np.float32(1.0)
    flat = m[:, c:].reshape(b, -1)
    flat[1::2, 0], flat[:, -1] = 27.5, -41.0                             # logvar outside [-30, 20] on both sides (every other image above:
                                                                         # e^20 would hide the other terms of that image's KL)
    m[:, c:] = flat.reshape(b, c, h, w)
    return m


@pytest.fixture(scope="module")
def ctx():
    return _lib.Context(0)


@pytest.mark.parametrize("shape", list(SHAPES), ids=SHAPE_IDS)
@pytest.mark.parametrize("B", [1, 3, 17])
def test_posterior_sample_matches_the_mirror(B, shape):
    """|z - z_mirror| <= 4 * 2^-24 * (|mean| + |std eps|): three fp32 roundings of half an ulp (std, the product, the sum) and one for a
    libm difference at a rounding boundary of eps; kl within 1e-9 relative."""
    rng = np.random.default_rng(100 * B + shape[1])
    m = _moments(rng, B, shape)
    dist = DiagonalGaussianDistribution(torch.from_numpy(m).cuda())
    z = dist.sample_device(SEED, draw=2, first_image=5).cpu().numpy()
    kl = dist.kl_device().cpu().numpy()
    zm, mean, noise = il.sample_elements(m, SEED, 2, 5)
    assert z.shape == mean.shape and z.dtype == np.float32 and kl.dtype == np.float64
    bound = 4 * 2.0 ** -24 * (np.abs(mean) + np.abs(noise))
    err = np.abs(z.astype(np.float64) - zm)
    klm = il.kl_elements(m)
    rel = float(np.max(np.abs(kl - klm) / klm))
    print(f"B={B} latent={shape}: max |z - mirror| / bound {float(np.max(err / np.maximum(bound, 1e-300))):.3f}, kl max rel {rel:.3e}")
    assert (err <= bound).all()
    assert rel <= REL
    # another draw, another first image: other noise; the same call: the same bits
    assert not np.array_equal(dist.sample_device(SEED, 3, 5).cpu().numpy(), z) and not np.array_equal(dist.sample_device(SEED, 2, 6).cpu().numpy(), z)
    assert np.array_equal(dist.sample_device(SEED, 2, 5).cpu().numpy(), z)
    if B > 1:                                                            # an image's noise follows its global index
        tail = DiagonalGaussianDistribution(torch.from_numpy(m[1:]).cuda()).sample_device(SEED, 2, 6).cpu().numpy()
        assert np.array_equal(tail, z[1:])


def _triplet_inputs(rng, shape, kind):
    """21 rows of latents whose hinge is inactive on every third row (positive next to the anchor, negative opposite), their moments
    (for the KL), images and labels."""
    c, h, w = shape
    d = c * h * w
    za = rng.standard_normal((ROWS, d)).astype(np.float32)
    zp = (za + rng.standard_normal((ROWS, d)) * 0.7).astype(np.float32)
    zn = rng.standard_normal((ROWS, d)).astype(np.float32)
    quiet = np.arange(ROWS) % 3 == 0
    zp[quiet] = za[quiet] + np.float32(0.01) * rng.standard_normal((int(quiet.sum()), d)).astype(np.float32)
    zn[quiet] = np.float32(-2.0) * za[quiet]
    near = np.arange(ROWS) % 3 == 1                                      # a negative nearer than the positive: the hinge is active
    zn[near] = (za[near] + rng.standard_normal((int(near.sum()), d)) * 0.5).astype(np.float32)
    moments = [_moments(rng, ROWS, shape) for _ in range(3)]
    img = SHAPES[shape]
    recon, target = rng.standard_normal((2, ROWS) + img).astype(np.float32)
    n = 70                                                               # more labels than lanes
    if kind == "none":
        la = lp = None
    else:
        la, lp = rng.random((2, ROWS, n)) < 0.3
        la[5], lp[5] = lp[5], lp[5]                                      # identical label rows: a similar pair
        la[7] = False                                                    # an anchor without labels
        if kind == "f32":
            la = (la * rng.choice(np.array([0.25, 0.5, 1.0], dtype=np.float32), size=la.shape)).astype(np.float32)
            lp = lp.astype(np.float32)
        else:
            la, lp = la.astype(np.uint8), lp.astype(np.uint8)
    return za, zp, zn, moments, recon, target, la, lp, quiet


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _close(got, want, what):
    """within 1e-9 relative where the mirror's value is non-zero; exactly zero where it is zero.  Returns the largest relative distance."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.isfinite(want).all(), what
    zero = want == 0
    assert (got[zero] == 0).all(), what
    rel = np.abs(got[~zero] - want[~zero]) / np.abs(want[~zero])
    worst = float(rel.max()) if rel.size else 0.0
    assert worst <= REL, (what, worst)
    return worst


@pytest.mark.parametrize("kind", ["u8", "f32", "none"])
@pytest.mark.parametrize("shape", list(SHAPES), ids=SHAPE_IDS)
def test_accumulator_given_z_matches_the_mirrors(shape, kind, ctx):
    rng = np.random.default_rng(7 + shape[1] * 10 + len(kind))
    za, zp, zn, mom, recon, target, la, lp, quiet = _triplet_inputs(rng, shape, kind)
    for sim in ("cosine", "euclidean"):                                  # about the mirror first: no row sits on the hinge
        x = il.triplet_margin_elements(za, zp, zn, MARGIN, sim)
        assert (np.abs(x) >= 1e-6).all() and (x[quiet] < 0).all() and (x[~quiet] > 0).any()
    host = HostVAELossState(MARGIN, 1.0, seed=SEED)
    acc = DeviceVAELossAccumulator("cuda", MARGIN, 1.0, seed=SEED, context=ctx)
    rows = torch.full((ROWS, vae_losses.ROW), -7.0, dtype=torch.float64, device="cuda")
    dev = [_t(a) for a in (za, zp, zn, *mom, recon, target, la, lp)]
    want_rows, lo = [], 0
    for b in SEQ:
        s = slice(lo, lo + b)
        want_rows.append(host.update((mom[0][s], za[s], 0), (mom[1][s], zp[s], 0), (mom[2][s], zn[s], 0), recon[s], target[s],
                                     None if la is None else la[s], None if lp is None else lp[s], first_image=lo))
        cut = [None if t is None else t[s] for t in dev]
        acc.update((cut[3], cut[0], 0), (cut[4], cut[1], 0), (cut[5], cut[2], 0), cut[6], cut[7], cut[8], cut[9], first_image=lo, rows_out=rows[s])
        lo += b
    want_rows = np.concatenate(want_rows)
    got_rows = rows.cpu().numpy()
    st = acc.read_state()
    worst = 0.0
    for k, name in enumerate(vae_losses.ROW_NAMES):
        worst = max(worst, _close(got_rows[:, k], want_rows[:, k], name))
    assert (got_rows[quiet][:, 10:12] == 0).all()                        # the hinge is inactive: exactly 0, both similarity types
    worst = max(worst, _close(st["batch_sums"], host.state["batch_sums"], "batch sums"), _close(st["image_sums"], host.state["image_sums"], "image sums"))
    for c in vae_losses.COUNTERS:
        assert st[c] == host.state[c], c
    assert (st["updates"], st["images"], st["non_finite"], st["recon_images"], st["negative_images"]) == (3, ROWS, 0, ROWS, ROWS)
    assert (st["margin_triplet"], st["margin_contrastive"], st["jaccard_threshold"], st["seed"]) == (MARGIN, 1.0, 0.3, SEED)
    w = {"reconstruction": 0.01, "kl": 0.01, "triplet": 1.0}
    assert abs(acc.read(w, "cosine")["val_loss"] - host.read(w, "cosine")["val_loss"]) <= REL * abs(host.read(w, "cosine")["val_loss"])
    print(f"latent={shape} labels={kind}: max rel {worst:.3e}")


def test_missing_negative_recon_and_moments_are_left_out(ctx):
    rng = np.random.default_rng(31)
    za, zp, zn, mom, recon, target, la, lp, _ = _triplet_inputs(rng, (16, 2, 3), "f32")
    host = HostVAELossState(MARGIN, 0.9, seed=SEED)
    acc = DeviceVAELossAccumulator("cuda", MARGIN, 0.9, seed=SEED, context=ctx)
    rows = torch.zeros((ROWS, vae_losses.ROW), dtype=torch.float64, device="cuda")
    want = host.update((None, za, 0), (mom[1], zp, 0), None, None, None, la, lp)          # contrastive only; one stream with a KL
    acc.update((None, _t(za), 0), (_t(mom[1]), _t(zp), 0), None, labels_a=_t(la), labels_p=_t(lp), rows_out=rows)
    want2 = host.update((mom[0][:4], za[:4], 0), (mom[1][:4], zp[:4], 0), (mom[2][:4], zn[:4], 0), recon[:4], target[:4], first_image=3)
    rows2 = torch.zeros((4, vae_losses.ROW), dtype=torch.float64, device="cuda")
    acc.update((_t(mom[0][:4]), _t(za[:4]), 0), (_t(mom[1][:4]), _t(zp[:4]), 0), (_t(mom[2][:4]), _t(zn[:4]), 0), _t(recon[:4]), _t(target[:4]),
               first_image=3, rows_out=rows2)
    st = acc.read_state()
    for k, name in enumerate(vae_losses.ROW_NAMES):
        _close(rows.cpu().numpy()[:, k], want[:, k], name)
        _close(rows2.cpu().numpy()[:, k], want2[:, k], name)
    assert (want[:, [0, 1, 3, 7, 9, 10, 11]] == 0).all() and (want[:, 4] == want[:, 2]).all() and (want2[:, 17] == 1).all()
    _close(st["batch_sums"], host.state["batch_sums"], "batch sums")
    _close(st["image_sums"], host.state["image_sums"], "image sums")
    assert [st[c] for c in vae_losses.COUNTERS] == [2, ROWS + 4, 0, 1, 4, 1, 4]
    r = acc.read({"reconstruction": 1.0, "kl": 1.0, "triplet": 1.0})
    assert abs(r["components"]["mse"]["mean_of_batch_means"] - il.mse_elements(recon[:4], target[:4]).mean()) <= REL


def _heads(shape, ctx, in_flight, seq=SEQ, sample=None):
    """The head's bytes and the rows after feeding `seq`: latents sampled in flight (draws 1, 2, 3), or given as what vt_posterior_sample
    writes for the same (seed, draw, first_image)."""
    rng = np.random.default_rng(55 + shape[1])
    mom = [_t(_moments(rng, ROWS, shape)) for _ in range(3)]
    recon, target = (_t(a) for a in rng.standard_normal((2, ROWS) + SHAPES[shape]).astype(np.float32))
    la, lp = (_t(a) for a in (rng.random((2, ROWS, 9)) < 0.4).astype(np.uint8))
    acc = DeviceVAELossAccumulator("cuda", MARGIN, 1.0, seed=SEED, context=ctx)
    rows = torch.zeros((ROWS, vae_losses.ROW), dtype=torch.float64, device="cuda")
    lo = 0
    for b in seq:
        s = slice(lo, lo + b)
        ins = []
        for k in range(3):
            z = None if in_flight else DiagonalGaussianDistribution(mom[k][s], ctx).sample_device(SEED, k + 1, lo)
            ins.append((mom[k][s], z, k + 1))
        acc.update(*ins, recon[s], target[s], la[s], lp[s], first_image=lo, rows_out=rows[s])
        lo += b
    return acc.device_head().cpu().numpy().tobytes(), rows.cpu().numpy().tobytes()


@pytest.mark.parametrize("shape", list(SHAPES), ids=SHAPE_IDS)
def test_in_flight_sampling_equals_the_given_z_path_bit_for_bit(shape, ctx):
    flight, given = _heads(shape, ctx, True), _heads(shape, ctx, False)
    assert flight[0] == given[0] and flight[1] == given[1]
    assert _heads(shape, ctx, True) == flight                            # and the same calls give the same bytes
    st = vae_losses.parse_state(flight[0])
    assert st["images"] == ROWS and st["non_finite"] == 0 and np.isfinite(st["batch_sums"]).all() and (st["batch_sums"][3:5] > 0).all()


def test_per_image_sums_do_not_depend_on_the_batching(ctx):
    shape = (16, 33, 17)
    a, b = _heads(shape, ctx, True, (3, 17, 1)), _heads(shape, ctx, True, (21,))
    sa, sb = vae_losses.parse_state(a[0]), vae_losses.parse_state(b[0])
    assert sa["image_sums"].tobytes() == sb["image_sums"].tobytes() and a[1] == b[1]
    assert sa["batch_sums"].tobytes() != sb["batch_sums"].tobytes() and (sa["updates"], sb["updates"]) == (3, 1)


def test_unaligned_inputs_take_the_scalar_loads_and_give_the_same_bits(ctx):
    """Tensors that start 4 bytes off a 16-byte boundary, and a latent size that is no multiple of 4, go through guarded scalar loads with
    the same element-to-thread mapping: the same sums in the same order."""
    rng = np.random.default_rng(91)
    b, shape, img = 3, (16, 33, 17), (3, 16, 24)
    mom = [_moments(rng, b, shape) for _ in range(3)]
    recon, target = rng.standard_normal((2, b) + img).astype(np.float32)

    def shifted(a):
        buf = torch.zeros(a.size + 1, dtype=torch.float32, device="cuda")
        buf[1:] = torch.from_numpy(a.reshape(-1))
        return buf[1:].view(a.shape)
    out = []
    for move in (_t, shifted):
        acc = DeviceVAELossAccumulator("cuda", MARGIN, seed=SEED, context=ctx)
        m = [move(x) for x in mom]
        assert all(t.data_ptr() % 16 == (0 if move is _t else 4) for t in m)
        z = DiagonalGaussianDistribution(m[0], ctx).sample_device(SEED, 1, 4)
        acc.update((m[0], None, 1), (m[1], None, 2), (m[2], None, 3), move(recon), move(target), first_image=4)
        out.append((acc.device_head().cpu().numpy().tobytes(), z.cpu().numpy().tobytes()))
    assert out[0] == out[1]
    # D = 4099: odd, and one element past a chunk
    za, zp, zn = rng.standard_normal((3, 5, 4099)).astype(np.float32)
    acc, host = DeviceVAELossAccumulator("cuda", MARGIN, context=ctx), HostVAELossState(MARGIN)
    rows = torch.zeros((5, vae_losses.ROW), dtype=torch.float64, device="cuda")
    acc.update((None, _t(za), 0), (None, _t(zp), 0), (None, _t(zn), 0), rows_out=rows)
    want = host.update((None, za, 0), (None, zp, 0), (None, zn, 0))
    for k, name in enumerate(vae_losses.ROW_NAMES):
        _close(rows.cpu().numpy()[:, k], want[:, k], name)
    m = _moments(rng, 2, (3, 5, 7))                                      # 105 elements per image
    d = DiagonalGaussianDistribution(_t(m), ctx)
    zm, mean, noise = il.sample_elements(m, SEED, 0, 0)
    assert (np.abs(d.sample_device(SEED).cpu().numpy() - zm) <= 4 * 2.0 ** -24 * (np.abs(mean) + np.abs(noise))).all()
    assert np.allclose(d.kl_device().cpu().numpy(), il.kl_elements(m), rtol=REL, atol=0)


def test_non_finite_inputs_propagate_and_are_counted(ctx):
    rng = np.random.default_rng(77)
    za, zp, zn, mom, recon, target, la, lp, _ = _triplet_inputs(rng, (16, 33, 17), "u8")
    clean = DeviceVAELossAccumulator("cuda", MARGIN, context=ctx)
    rows_c = torch.zeros((ROWS, vae_losses.ROW), dtype=torch.float64, device="cuda")
    clean.update((_t(mom[0]), _t(za), 0), (_t(mom[1]), _t(zp), 0), (_t(mom[2]), _t(zn), 0), _t(recon), _t(target), _t(la), _t(lp), rows_out=rows_c)
    za[2, 5000], zn[4, 1] = np.nan, np.inf
    mom[1][6, 0, 0, 0] = -np.inf                                         # a mean
    mom[2][8, 20, 3, 3] = np.nan                                         # a logvar: stays NaN through the clamp
    recon[10, 1, 7, 7] = np.inf
    acc = DeviceVAELossAccumulator("cuda", MARGIN, context=ctx)
    rows = torch.zeros((ROWS, vae_losses.ROW), dtype=torch.float64, device="cuda")
    acc.update((_t(mom[0]), _t(za), 0), (_t(mom[1]), _t(zp), 0), (_t(mom[2]), _t(zn), 0), _t(recon), _t(target), _t(la), _t(lp), rows_out=rows)
    st, r, rc = acc.read_state(), rows.cpu().numpy(), rows_c.cpu().numpy()
    assert st["non_finite"] == 5 and st["updates"] == 1
    assert np.isnan(r[2, 6]) and np.isnan(r[2, 10]) and not np.isfinite(r[4, 9]) and r[6, 2] == np.inf and np.isnan(r[8, 3]) and r[10, 0] == np.inf
    hit = np.zeros(ROWS, dtype=bool)
    hit[[2, 4, 6, 8, 10]] = True
    assert r[~hit].tobytes() == rc[~hit].tobytes()                       # the other images: the same bits
    assert not np.isfinite(st["batch_sums"][[0, 1, 3, 4]]).any() and not np.isfinite(st["image_sums"][[0, 1, 3, 4]]).any()
    host = HostVAELossState(MARGIN)
    host.update((mom[0], za, 0), (mom[1], zp, 0), (mom[2], zn, 0), recon, target, la, lp)
    assert host.state["non_finite"] == 5


def _guarded(nbytes, fill=0xA5):
    t = torch.full((nbytes + 768,), fill, dtype=torch.uint8, device="cuda")
    ptr = (t.data_ptr() + 256 + 255) // 256 * 256
    return t, ptr


def test_refusals_return_their_codes_and_write_nothing(ctx):
    L, h, vp = ctx.lib, ctx.handle, ctypes.c_void_p
    OK, INVALID, WORKSPACE = 0, 1, 5
    B, C, hw, H, W, N = 3, 16, 6, 16, 24, 5
    nb = L.vt_vae_loss_state_bytes(B, C, hw, H, W)
    assert nb == vae_losses.state_bytes(B, C, hw, H, W)
    rng = np.random.default_rng(2)
    mom = _t(rng.standard_normal((B, 2 * C, 2, 3)).astype(np.float32))
    z = _t(rng.standard_normal((B + 1, C * hw)).astype(np.float32))
    img = _t(rng.standard_normal((2, B, 3, H, W)).astype(np.float32))
    lab = _t((rng.random((2, B, N)) < 0.5).astype(np.float32))
    state, sp = _guarded(nb)                                             # a poisoned block: never reset, it must stay poisoned
    rows, rp = _guarded(8 * B * vae_losses.ROW, 0x5A)
    zout, zp_ = _guarded(4 * B * C * hw, 0x5A)
    inp = lambda m, zz, draw=0: _lib.VAELossInput(m, zz, draw)
    a, p, n = inp(mom.data_ptr(), None, 1), inp(None, z.data_ptr()), inp(mom.data_ptr(), z.data_ptr(), 3)

    def upd(ptr=sp, nbytes=nb, anchor=a, positive=p, negative=n, recon=img[0].data_ptr(), target=img[1].data_ptr(), la=lab[0].data_ptr(),
            lp=lab[1].data_ptr(), dt=_lib.VT_F32, n_labels=N, b=B, first=0, rows_ptr=rp):
        ref = lambda s: ctypes.byref(s) if s is not None else None
        return L.vt_vae_loss_update(h, vp(ptr), nbytes, ref(anchor), ref(positive), ref(negative), vp(recon), vp(target), H, W, vp(la), vp(lp), dt,
                                    n_labels, b, C, hw, first, vp(rows_ptr), None)
    assert upd(nbytes=nb - 1) == WORKSPACE and b"bytes" in L.vt_last_error(h)      # undersized state
    assert upd(ptr=sp + 8) == INVALID                                    # misaligned state
    assert upd(positive=inp(None, z.data_ptr() + 2)) == INVALID          # misaligned latent
    assert upd(anchor=inp(mom.data_ptr() + 1, None)) == INVALID          # misaligned moments
    assert upd(target=None) == INVALID and upd(recon=None) == INVALID    # recon without target and the other way round
    assert upd(lp=None) == INVALID and upd(dt=_lib.VT_BF16) == INVALID and upd(n_labels=0) == INVALID
    assert upd(b=0) == INVALID and upd(b=4097) == INVALID                # B outside [1, 4096]
    assert upd(anchor=None) == INVALID and upd(positive=inp(None, None)) == INVALID and upd(first=-1) == INVALID
    assert upd(rows_ptr=rp + 4) == INVALID and upd(negative=inp(mom.data_ptr(), None, -1)) == INVALID
    assert L.vt_vae_loss_reset(h, vp(sp), vae_losses.HEAD_BYTES - 1, 1.0, 1.0, 0.3, 0, None) == WORKSPACE
    assert L.vt_vae_loss_reset(h, vp(sp), nb, float("nan"), 1.0, 0.3, 0, None) == INVALID
    assert L.vt_vae_loss_reset(h, vp(sp + 16), nb, 1.0, 1.0, 0.3, 0, None) == INVALID
    out, op = _guarded(vae_losses.HEAD_BYTES, 0x5A)
    assert L.vt_vae_loss_read(h, vp(sp), nb, vp(op), vae_losses.HEAD_BYTES - 1, None) == WORKSPACE
    assert L.vt_vae_loss_read(h, vp(sp), nb, None, vae_losses.HEAD_BYTES, None) == INVALID
    assert L.vt_vae_loss_read(h, vp(sp), nb, vp(sp), vae_losses.HEAD_BYTES, None) == INVALID          # out is the state
    samp = lambda m=mom.data_ptr(), b=B, zo=zp_, draw=0, first=0: L.vt_posterior_sample(h, vp(m), b, C, hw, 1, draw, first, vp(zo), None, None)
    assert samp(m=None) == INVALID and samp(b=0) == INVALID and samp(zo=zp_ + 2) == INVALID and samp(draw=-1) == INVALID and samp(first=-1) == INVALID
    torch.cuda.synchronize()
    assert (state.cpu().numpy() == 0xA5).all()                           # nothing was written: the block is still poisoned
    for t in (rows, zout, out):
        assert (t.cpu().numpy() == 0x5A).all()
    # and the accepted calls stay inside their buffers
    assert L.vt_vae_loss_reset(h, vp(sp), nb, 1.0, 1.0, 0.3, 7, None) == OK and upd() == OK and samp() == OK
    assert L.vt_vae_loss_read(h, vp(sp), nb, vp(op), vae_losses.HEAD_BYTES, None) == OK
    torch.cuda.synchronize()
    for t, ptr, n_in in ((state, sp, nb), (rows, rp, 8 * B * vae_losses.ROW), (zout, zp_, 4 * B * C * hw), (out, op, vae_losses.HEAD_BYTES)):
        raw, off = t.cpu().numpy(), ptr - t.data_ptr()
        fill = raw[0]
        assert (raw[:off] == fill).all() and (raw[off + n_in:] == fill).all()
    s = vae_losses.parse_state(out.cpu().numpy()[op - out.data_ptr():][:vae_losses.HEAD_BYTES])
    assert (s["updates"], s["images"], s["seed"]) == (1, B, 7)


def test_update_sample_and_read_do_not_synchronise_the_host(monkeypatch, ctx):
    rng = np.random.default_rng(12)
    shape = (16, 33, 17)
    mom = [_t(_moments(rng, 8, shape)) for _ in range(3)]
    recon, target = (_t(a) for a in rng.standard_normal((2, 8) + SHAPES[shape]).astype(np.float32))
    lab = _t((rng.random((8, 9)) < 0.4).astype(np.float32))
    rows = torch.zeros((8, vae_losses.ROW), dtype=torch.float64, device="cuda")

    def run(acc):
        for lo in range(0, 8, 4):
            s = slice(lo, lo + 4)
            d = DiagonalGaussianDistribution(mom[0][s], ctx)
            z = d.sample_device(SEED, 0, lo)
            d.kl_device()
            acc.update((mom[0][s], z, 1), (mom[1][s], None, 2), (mom[2][s], None, 3), recon[s], target[s], lab[s], lab[s], first_image=lo, rows_out=rows[s])
        return acc.device_components()
    run(DeviceVAELossAccumulator("cuda", context=ctx))                   # kernels loaded, the block grown once
    torch.cuda.synchronize()
    calls = {"n": 0}

    def counted(fn):
        def wrapper(*a, **k):
            calls["n"] += 1
            return fn(*a, **k)
        return wrapper
    monkeypatch.setattr(torch.cuda, "synchronize", counted(torch.cuda.synchronize))
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", counted(torch.cuda.Stream.synchronize))
    for name in ("cpu", "item", "numpy", "tolist"):
        monkeypatch.setattr(torch.Tensor, name, counted(getattr(torch.Tensor, name)))
    acc = DeviceVAELossAccumulator("cuda", context=ctx)
    done = torch.cuda.Event()
    comps = run(acc)
    done.record()
    queued_before_finished = not done.query()                            # informational: the queue was still busy when the calls returned
    assert calls["n"] == 0
    monkeypatch.undo()
    print(f"work still queued when the calls returned: {queued_before_finished}")
    st = acc.read_state()
    assert st["updates"] == 2 and comps.cpu().numpy().tobytes() == st["batch_sums"].tobytes()


def test_fixture_extremes_against_the_references_recorded_outputs(ctx):
    """The committed fixture (hinge inactive, positive == anchor, an all-zero anchor) through the reference-shaped classes on the device,
    against the reference's fp64 values (1e-9 relative) and its fp32 values (the tolerance measured in the host test)."""
    with np.load(os.path.join(ROOT, "tests", "golden", "vae_loss_reference.npz"), allow_pickle=False) as f:
        fx = {k: f[k].copy() for k in f.files}
    tol = measured_fp32_tolerance(fx)
    za, zp, zn, la, lp = (_t(fx[k]) for k in ("za", "zp", "zn", "labels_a", "labels_p"))
    for sim in ("cosine", "euclidean"):
        trip, con = il.ImprovedTripletLoss(1.0, sim), il.ContrastiveLoss(1.0, sim)
        got = {f"triplet_{sim}_labels": trip(za, zp, zn, la, lp), f"triplet_{sim}_nolabels": trip(za, zp, zn), f"contrastive_{sim}": con(za, zp, la, lp)}
        for name, v in got.items():
            assert v.dim() == 0 and v.dtype == torch.float64 and v.is_cuda
            g, w64, w32 = float(v.cpu()), float(fx[name + "_f64"]), float(fx[name + "_f32"])
            print(f"{name}: device {g!r} reference fp64 {w64!r} rel {abs(g - w64) / abs(w64):.3e}; to reference fp32 {abs(g - w32):.3e} (allowed {tol[name]:.3e})")
            assert abs(g - w64) <= REL * abs(w64) and abs(g - w32) <= tol[name], name
    d = il.SimplifiedCombinedLoss(triplet_weight=0.5, use_focal_loss=False, similarity_type="cosine")
    logits = _t(np.random.default_rng(1).standard_normal((5, 7)).astype(np.float32))
    out = d(za, zp, zn, logits, la, anchor_labels=la, positive_labels=lp)
    want_cls = torch.nn.functional.binary_cross_entropy_with_logits(logits.double(), la.double())
    want = 0.5 * float(fx["triplet_cosine_labels_f64"]) + float(want_cls.cpu())
    assert set(out) == {"triplet_loss", "classification_loss", "total_loss", "weights"}
    assert abs(float(out["total_loss"].cpu()) - want) <= REL * want


def test_combined_loss_returns_the_references_keys_from_one_update(ctx):
    """CombinedLoss.forward with the reference's arguments: posteriors, sampled latents, reconstruction, logits -- against the mirrors."""
    rng = np.random.default_rng(8)
    shape, b = (16, 2, 3), 5
    mom = [_moments(rng, b, shape) for _ in range(3)]
    post = [DiagonalGaussianDistribution(_t(m), ctx) for m in mom]
    z = [p.sample_device(SEED, k + 1, 0) for k, p in enumerate(post)]
    recon, target = rng.standard_normal((2, b, 3, 16, 24)).astype(np.float32)
    logits = rng.standard_normal((b, 9)).astype(np.float32)
    la, lp = (rng.random((2, b, 9)) < 0.4).astype(np.float32)
    fn = il.CombinedLoss(reconstruction_weight=0.3, kl_weight=0.2, triplet_weight=1.5, classification_weight=0.7, use_focal_loss=True,
                         focal_alpha=0.25, focal_gamma=2.0, triplet_margin=MARGIN, similarity_type="euclidean")
    out = fn(_t(recon), _t(target), *post, *z, _t(logits), _t(la), anchor_labels=_t(la), positive_labels=_t(lp))
    assert set(out) == {"total_loss", "reconstruction_loss", "kl_loss", "triplet_loss", "classification_loss", "weights"}
    zs = [t.cpu().numpy() for t in z]
    kl = [il.kl_elements(m) for m in mom]
    from vae_tagger_amd import losses
    want = {"reconstruction_loss": il.mse_elements(recon, target).mean(), "kl_loss": il.kl_log(((kl[0] + kl[1] + kl[2]) / 3).mean()),
            "triplet_loss": il.triplet_elements(zs[0], zs[1], zs[2], la, lp, MARGIN, "euclidean").mean(),
            "classification_loss": losses.focal_loss(logits, la, 0.25, 2.0)}
    for name, w in want.items():
        assert out[name].dim() == 0 and out[name].is_cuda
        assert abs(float(out[name].cpu()) - w) <= REL * abs(w), name
    total = 0.3 * want["reconstruction_loss"] + 0.2 * want["kl_loss"] + 1.5 * want["triplet_loss"] + 0.7 * want["classification_loss"]
    assert abs(float(out["total_loss"].cpu()) - total) <= REL * abs(total) and out["weights"].tolist() == pytest.approx([0.3, 0.2, 1.5, 0.7])
