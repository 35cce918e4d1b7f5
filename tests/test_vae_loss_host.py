"""Host side of the VAE validation loss: the numpy fp64 mirrors of improved_losses.py against the values the reference's own classes
returned (tests/golden/vae_loss_reference.npz, made by tools/make_vae_loss_fixture.py), the counter-based normal generator, the
per-anchor triplet sampling, the host model of the device block and the ABI surface.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from _vae_loss_util import measured_fp32_tolerance
from vae_tagger_amd import _lib, evaluate_vae, improved_losses as il, vae_losses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL_FP64 = 1e-9
SIMS = ("cosine", "euclidean")


@pytest.fixture(scope="module")
def fixture():
    with np.load(os.path.join(ROOT, "tests", "golden", "vae_loss_reference.npz"), allow_pickle=False) as z:
        return {k: z[k].copy() for k in z.files}


def test_mirrors_match_the_reference_classes(fixture):
    fx = fixture
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "vae_loss_reference.npz")) < 64 * 1024
    assert fx["za"].shape == (5, 96) and fx["labels_a"].shape == (5, 7)
    assert np.array_equal(fx["zp"][2], fx["za"][2]) and not fx["za"][3].any()        # positive == anchor; an all-zero anchor
    for sim in SIMS:                                                                  # rows with the hinge inactive
        assert (il.triplet_margin_elements(fx["za"], fx["zp"], fx["zn"], 1.0, sim) < 0).any()
    assert il.distance_elements(fx["za"], fx["zp"], "cosine")[3] == 1.0               # the 1e-12 clamp: 0 / (1e-12 |p|) = 0
    tol = measured_fp32_tolerance(fx)
    for name, t in tol.items():
        kind, sim = name.split("_")[0], name.split("_")[1]
        if kind == "triplet":
            la, lp = (fx["labels_a"], fx["labels_p"]) if name.endswith("_labels") else (None, None)
            got = il.triplet_elements(fx["za"], fx["zp"], fx["zn"], la, lp, float(fx["margin"]), sim).mean()
        else:
            got = il.contrastive_elements(fx["za"], fx["zp"], fx["labels_a"], fx["labels_p"], float(fx["margin"]), sim).mean()
        w64, w32 = float(fx[name + "_f64"]), float(fx[name + "_f32"])
        print(f"{name}: mirror {got!r} reference fp64 {w64!r} (rel {abs(got - w64) / abs(w64):.3e}), reference fp32 {w32!r} "
              f"(|d| {abs(got - w32):.3e}, allowed {t:.3e})")
        assert abs(got - w64) <= REL_FP64 * abs(w64), name
        assert t > 0 and abs(got - w32) <= t, name


def test_kl_and_sample_mirrors_match_torch_in_fp64():
    rng = np.random.default_rng(0)
    m = rng.standard_normal((3, 8, 2, 3)).astype(np.float32)
    m[0, 4, 0, 0], m[1, 5, 1, 2] = 25.0, -40.0                                       # logvar outside [-30, 20] on both sides
    t = torch.from_numpy(m).double()
    mean, lv = t[:, :4], torch.clamp(t[:, 4:], -30.0, 20.0)
    want = 0.5 * torch.sum(mean.pow(2) + lv.exp() - 1.0 - lv, dim=[1, 2, 3])
    assert np.allclose(il.kl_elements(m), want.numpy(), rtol=1e-13, atol=0)
    z, mu, noise = il.sample_elements(m, seed=3, draw=2, first_image=10)
    eps = np.stack([il.normal_draw(3, 2, 10 + i, 24) for i in range(3)]).reshape(3, 4, 2, 3)
    assert np.array_equal(z, mu + noise) and np.allclose(noise, np.exp(0.5 * lv.numpy()) * eps, rtol=1e-15)
    assert noise[0, 0, 0, 0] == np.exp(10.0) * float(eps[0, 0, 0, 0])                 # clamped at 20


def test_generator_uniforms_are_never_zero_and_moments_are_normal():
    n = 1 << 20
    u1, u2 = il.uniform_draws(7, 0, 0, n)
    assert u1.min() > 0.0 and u1.max() <= 1.0 and u2.min() >= 0.0 and u2.max() < 1.0
    # the smallest word gives the smallest u1, 2^-53, not 0: -2 ln u1 stays finite
    assert ((np.uint64(0) >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53 == 2.0 ** -53
    e = il.normal_draw(7, 0, 0, n)
    assert e.dtype == np.float32 and np.isfinite(e).all()
    e = e.astype(np.float64)
    print(f"2^20 draws: mean {e.mean():.3e} var {e.var():.6f}")
    assert abs(e.mean()) <= 5 / np.sqrt(n) and abs(e.var() - 1.0) <= 5 * np.sqrt(2.0 / n)
    base = il.normal_draw(7, 0, 0, 4096)
    for other in (il.normal_draw(7, 1, 0, 4096), il.normal_draw(7, 0, 1, 4096), il.normal_draw(8, 0, 0, 4096)):
        assert (other != base).mean() > 0.99
        assert abs(np.corrcoef(other, base)[0, 1]) < 5 / np.sqrt(4096)


def test_an_images_noise_does_not_depend_on_the_partitioning():
    m = np.random.default_rng(1).standard_normal((6, 8, 3, 5)).astype(np.float32)
    whole = il.sample_elements(m, 11, 1, first_image=100)[0]
    parts = np.concatenate([il.sample_elements(m[lo:hi], 11, 1, first_image=100 + lo)[0] for lo, hi in ((0, 1), (1, 4), (4, 6))])
    assert whole.tobytes() == parts.tobytes()
    assert il.sample_elements(m, 11, 1, first_image=101)[0].tobytes() != whole.tobytes()
    # a prefix of an image's stream does not depend on how many elements are drawn
    assert np.array_equal(il.normal_draw(11, 1, 100, 50), il.normal_draw(11, 1, 100, 500)[:50])


def test_triplet_sampling_is_per_anchor_and_follows_the_fall_backs():
    rng = np.random.default_rng(4)
    labels = (rng.random((40, 6)) < 0.3).astype(np.float32)
    labels[0] = [1, 1, 0, 0, 0, 0]
    a = evaluate_vae.triplet_lists(labels, seed=5)
    assert a == evaluate_vae.triplet_lists(labels, seed=5)                            # deterministic
    assert a[7] == evaluate_vae.sample_triplet(5, 7, labels)                          # an anchor's triplet stands alone: no order, no batch
    assert a != evaluate_vae.triplet_lists(labels, seed=6)
    for i, (p, n) in enumerate(a):
        has_pos = any((labels[j] * labels[i]).sum() > 0 for j in range(40) if j != i)
        has_neg = any(not (labels[j] * labels[i]).sum() > 0 for j in range(40) if j != i)
        assert (p != i and (labels[p] * labels[i]).sum() > 0) if has_pos else p == i   # all 39 others are candidates (39 < 100)
        if has_neg:
            assert n != i and not (labels[n] * labels[i]).sum() > 0
        else:
            assert n != i
    # no positive candidate: the anchor itself; no negative candidate: some other image; a set of one: the anchor twice
    lonely = np.eye(4, dtype=np.float32)
    assert [p for p, _ in evaluate_vae.triplet_lists(lonely, 1)] == [0, 1, 2, 3]
    same = np.ones((5, 3), dtype=np.float32)
    for i, (p, n) in enumerate(evaluate_vae.triplet_lists(same, 1)):
        assert p != i and n != i
    assert evaluate_vae.triplet_lists(np.ones((1, 3), dtype=np.float32), 1) == [(0, 0)]
    # an image without tags overlaps nothing: itself as the positive, another image as the negative
    none = np.zeros((3, 2), dtype=np.float32)
    assert all(p == i and n != i for i, (p, n) in enumerate(evaluate_vae.triplet_lists(none, 2)))
    # at most max_candidates others are looked at
    big = (np.random.default_rng(9).random((300, 4)) < 0.5).astype(np.float32)
    pos, neg = evaluate_vae.mine_candidates(__import__("random").Random(3), 0, big, 100)
    assert len(pos) + len(neg) == 100 and len(set(pos + neg)) == 100 and 0 not in pos + neg


def test_symbols_are_declared_bound_and_exported_and_sizes_are_host_arithmetic():
    header = open(os.path.join(ROOT, "include", "vae_tagger_hip.h")).read()
    lib = _lib.load()
    names = ("vt_posterior_sample", "vt_vae_loss_state_bytes", "vt_vae_loss_reset", "vt_vae_loss_update", "vt_vae_loss_read")
    for name in names:
        m = re.search(r"\b(size_t|int)\s+%s\(([^;]*?)\);" % name, header, re.S)
        assert m, name
        params = [a for a in re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S).split(",") if a.strip()]
        res, args = _lib.PROTOTYPES[name]
        assert res is (ctypes.c_size_t if m.group(1) == "size_t" else ctypes.c_int) and len(args) == len(params), name
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    assert re.search(r"typedef struct \{[^}]*moments;[^}]*z;[^}]*draw;[^}]*\} vt_vae_loss_input;", header)
    assert [f[0] for f in _lib.VAELossInput._fields_] == ["moments", "z", "draw"] and ctypes.sizeof(_lib.VAELossInput) == 24
    assert int(re.search(r"#define VT_VAE_LOSS_ROW (\d+)", header).group(1)) == vae_losses.ROW == _lib.VAE_LOSS_ROW == len(vae_losses.ROW_NAMES)
    assert int(re.search(r"#define VT_VAE_LOSS_HEAD_BYTES (\d+)", header).group(1)) == vae_losses.HEAD_BYTES == _lib.VAE_LOSS_HEAD_BYTES
    for shape in ((1, 16, 1, 0, 0), (3, 16, 6, 16, 24), (17, 16, 33 * 17, 264, 136), (16, 16, 128 * 128, 1024, 1024), (4096, 4, 5, 8, 8)):
        assert lib.vt_vae_loss_state_bytes(*shape) == vae_losses.state_bytes(*shape), shape
    for bad in ((0, 16, 4, 8, 8), (4097, 16, 4, 8, 8), (1, 0, 4, 8, 8), (1, 16, 0, 8, 8), (1, 16, 4, 8, 0), (1, 16, 4, -1, -1)):
        assert lib.vt_vae_loss_state_bytes(*bad) == 0, bad
    assert "eval_vae_loss.hip" in open(os.path.join(ROOT, "vae_tagger_amd", "csrc", "Makefile")).read()


def test_host_state_feeds_reports_and_round_trips():
    rng = np.random.default_rng(6)
    h = vae_losses.HostVAELossState(margin_triplet=0.7, seed=9)
    cuts = ((0, 3), (3, 8), (8, 9))
    m = [rng.standard_normal((9, 8, 2, 2)).astype(np.float32) for _ in range(3)]
    recon, target = rng.standard_normal((2, 9, 3, 4, 4)).astype(np.float32)
    la, lp = (rng.random((2, 9, 5)) < 0.5).astype(np.float32)
    rows = np.concatenate([h.update((m[0][a:b], None, 1), (m[1][a:b], None, 2), (m[2][a:b], None, 3), recon[a:b], target[a:b], la[a:b], lp[a:b],
                                    first_image=a) for a, b in cuts])
    z = [il.sample_elements(m[k], 9, k + 1, 0)[0].astype(np.float32) for k in range(3)]
    kl = [il.kl_elements(x) for x in m]
    assert np.array_equal(rows, vae_losses.rows_from_mirrors(z[0], z[1], z[2], kl, recon, target, la, lp, 0.7))      # sampling by global index
    w = {"reconstruction": 0.01, "kl": 0.01, "triplet": 1.0}
    r = h.read(w, "euclidean", simplified=False)
    trip = il.triplet_elements(z[0], z[1], z[2], la, lp, 0.7, "euclidean")
    mse = il.mse_elements(recon, target)
    klm = (kl[0] + kl[1] + kl[2]) / 3
    want = np.mean([0.01 * mse[a:b].mean() + 0.01 * il.kl_log(klm[a:b].mean()) + trip[a:b].mean() for a, b in cuts])
    assert abs(r["val_loss"] - want) <= 1e-12 * abs(want)
    assert abs(r["components"]["triplet_euclidean"]["per_image"] - trip.mean()) <= 1e-12 * trip.mean()
    assert abs(r["components"]["kl_log"]["per_image"] - il.kl_log(klm).mean()) <= 1e-12
    simple = h.read(w, "euclidean", simplified=True)
    assert abs(simple["val_loss"] - np.mean([0.01 * mse[a:b].mean() + trip[a:b].mean() for a, b in cuts])) <= 1e-12 * want
    assert (r["updates"], r["images"], r["non_finite"], r["recon_images"], r["negative_updates"]) == (3, 9, 0, 9, 3)
    block = h.to_bytes()
    assert len(block) == vae_losses.HEAD_BYTES and vae_losses.pack_state(vae_losses.parse_state(block)) == block
    assert vae_losses.finish_state(vae_losses.parse_state(block), w, "euclidean") == r
    c = vae_losses.HostVAELossState()
    c.update((None, z[0], 0), (None, z[1], 0))                                        # contrastive only: no negative, no KL, no recon
    rc = c.read(w)
    assert rc["components"]["triplet_cosine"]["mean_of_batch_means"] is None and rc["components"]["mse"]["per_image"] is None
    assert abs(rc["components"]["contrastive_cosine"]["per_image"] - il.contrastive_elements(z[0], z[1]).mean()) <= 1e-15
    with pytest.raises(ValueError, match="no data"):
        vae_losses.HostVAELossState().read(w)
    with pytest.raises(NotImplementedError, match="AdaptiveLossWeights"):
        il.CombinedLoss(use_adaptive_weights=True)
