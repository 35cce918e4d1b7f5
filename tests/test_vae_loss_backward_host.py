"""Host side of the training loss's gradient: the fp64 numpy mirror (vae_losses.loss_backward_host) against torch fp64 autograd of the
restated loss (tests/_vae_loss_backward_ref.py), the ABI surface of vt_vae_loss_backward, the saved-bytes formula of the joined step and
the wrappers' refusals that need no device.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _vae_loss_backward_ref as ref
from vae_tagger_amd import _lib, improved_losses as il, synth, vae_backward as vb, vae_losses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL_FP64 = 1e-12                    # both sides are fp64 and differ only in the order of their sums
# (C, h, w) of the latents: D = 96 (vector path, one chunk), 15 (scalar path), 4112 (crosses the 4096-element chunk); (H, W) of the images
LATENTS = [(16, 2, 3), (3, 1, 5), (16, 1, 257)]
IMAGES = [(8, 8), (37, 37), (8, 8)]
FULL = {"reconstruction": 0.01, "kl": 1e-2, "triplet": 1.0}
SIMPLIFIED = {"reconstruction": 0.01, "kl": 0.0, "triplet": 1.0}


def _close(got, want, what):
    want = np.asarray(want, dtype=np.float64)
    scale = np.abs(want).max()
    err = np.abs(np.asarray(got, dtype=np.float64) - want).max()
    print(f"    {what}: max |d| {err:.3e}  scale {scale:.3e}")
    assert err <= REL_FP64 * scale, what


@pytest.mark.parametrize("sim", ["cosine", "euclidean"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", range(len(LATENTS)), ids=["D96", "D15", "D4112"])
def test_mirror_matches_fp64_autograd(shape, B, sim):
    (C, h, w), (H, W) = LATENTS[shape], IMAGES[shape]
    seed, first = 11 + shape, 5
    D = C * h * w
    eps = [np.stack([il.normal_draw(seed, d, first + i, D) for i in range(B)]).reshape(B, C, h, w) for d in (1, 2, 3, 0)]
    active = 0
    for labels, weights, margin in ((0, FULL, 1.0), (7, FULL, 0.6), (7, SIMPLIFIED, 1.0), (0, SIMPLIFIED, 2.5)):
        margin *= 1.0 if sim == "cosine" else 4.0                            # (euclidean distances of these latents differ by a few units)
        c = ref.make_case(B, C, h, w, H, W, labels, seed=100 * shape + 10 * B + labels)
        kw = dict(weights=weights, margin=margin, similarity_type=sim, dz_dec=c["dz_dec"], recon=c["recon"], target=c["target"],
                  labels_a=c["labels_a"], labels_p=c["labels_p"])
        want = ref.autograd(c["moments"], eps[:3], eps_dec=eps[3], **kw)
        got = vae_losses.loss_backward_host(*[(m, d) for m, d in zip(c["moments"], (1, 2, 3))], seed=seed, first_image=first, dz_draw=0, **kw)
        active += want["losses"][2] > 0.0
        for s in range(3):
            _close(got["d_moments"][s], want["d_moments"][s], f"d_moments[{s}] labels={labels} {weights['kl']}")
        _close(got["d_recon"], want["d_recon"], "d_recon")
        _close(got["losses"], want["losses"], "losses")
        # the same numbers with the draws handed in, and without the decoder's gradient
        again = vae_losses.loss_backward_host(*[(m, None, d) for m, d in zip(c["moments"], (1, 2, 3))], eps=eps, **kw)
        assert all(np.array_equal(x, y) for x, y in zip(again["d_moments"], got["d_moments"]))
        kw["dz_dec"] = None
        want = ref.autograd(c["moments"], eps[:3], **kw)
        got = vae_losses.loss_backward_host(*[(m, d) for m, d in zip(c["moments"], (1, 2, 3))], seed=seed, first_image=first, **kw)
        for s in range(3):
            _close(got["d_moments"][s], want["d_moments"][s], f"d_moments[{s}] without dz_dec")
    assert active >= 2, "the cases must have active triplets"


def test_mirror_clamp_hinge_and_rows():
    """logvar outside [-30, 20] has no gradient and the bounds themselves do (torch.clamp's backward); an inactive hinge leaves the KL part
    alone; the rows are the forward mirror's"""
    B, C, h, w = 2, 4, 1, 3
    c = ref.make_case(B, C, h, w, 8, 8, 5, seed=3)
    for s, v in zip(range(3), (-31.0, 21.0, -30.0)):
        c["moments"][s][:, C, 0, 0] = v
    c["moments"][0][:, C + 1, 0, 1] = 20.0
    eps = [np.stack([il.normal_draw(2, d, i, C * h * w) for i in range(B)]).reshape(B, C, h, w) for d in (1, 2, 3, 0)]
    kw = dict(weights=FULL, similarity_type="cosine", dz_dec=c["dz_dec"], recon=c["recon"], target=c["target"], labels_a=c["labels_a"], labels_p=c["labels_p"])
    ins = [(m, d) for m, d in zip(c["moments"], (1, 2, 3))]
    got = vae_losses.loss_backward_host(*ins, seed=2, margin=1.0, **kw)
    want = ref.autograd(c["moments"], eps[:3], eps_dec=eps[3], margin=1.0, **kw)
    for s in range(3):
        _close(got["d_moments"][s], want["d_moments"][s], f"d_moments[{s}]")
    assert not got["d_moments"][0][:, C, 0, 0].any() and not got["d_moments"][1][:, C, 0, 0].any()
    assert got["d_moments"][2][:, C, 0, 0].all() and got["d_moments"][0][:, C + 1, 0, 1].all()
    z = [il.sample_elements(m, 2, d)[0].astype(np.float32) for m, d in zip(c["moments"], (1, 2, 3))]
    rows = vae_losses.rows_from_mirrors(*z, kl=tuple(il.kl_elements(m) for m in c["moments"]), recon=c["recon"], target=c["target"],
                                        labels_a=c["labels_a"], labels_p=c["labels_p"])
    keep = [k for k in range(vae_losses.ROW) if k not in (12, 13)]
    np.testing.assert_allclose(got["rows"][:, keep], rows[:, keep], rtol=1e-6)          # (sample_elements' z is fp64, the gradient's the fp32 one)
    assert not got["rows"][:, 12:14].any()
    off = vae_losses.loss_backward_host(*ins, seed=2, margin=-5.0, **kw)
    none = vae_losses.loss_backward_host(*ins, seed=2, margin=1.0, **dict(kw, weights=dict(FULL, triplet=0.0)))
    assert off["losses"][2] == 0.0
    for s in (1, 2):
        assert np.array_equal(off["d_moments"][s], none["d_moments"][s])


def test_symbols_are_declared_bound_and_exported_and_sizes_are_host_arithmetic():
    header = open(os.path.join(ROOT, "include", "vae_tagger_hip.h")).read()
    lib = _lib.load()
    for name in ("vt_vae_loss_backward_workspace_bytes", "vt_vae_loss_backward"):
        m = re.search(r"\b(size_t|int)\s+%s\(([^;]*?)\);" % name, header, re.S)
        assert m, name
        params = [a for a in re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S).split(",") if a.strip()]
        res, args = _lib.PROTOTYPES[name]
        assert res is (ctypes.c_size_t if m.group(1) == "size_t" else ctypes.c_int) and len(args) == len(params), name
        for a, t in zip(params, args):
            a = a.strip()
            want = (ctypes.c_double if a.startswith("double ") else ctypes.c_ulonglong if a.startswith("unsigned long long") else
                    ctypes.c_longlong if a.startswith("long long") else ctypes.c_size_t if a.startswith("size_t") else
                    ctypes.c_int if a.startswith("int ") else ctypes.POINTER(_lib.VAELossInput) if "vt_vae_loss_input*" in a else ctypes.c_void_p)
            assert t is want, (name, a)
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    assert int(re.search(r"#define VT_VAE_COSINE (\d+)", header).group(1)) == _lib.VAE_COSINE
    assert int(re.search(r"#define VT_VAE_EUCLIDEAN (\d+)", header).group(1)) == _lib.VAE_EUCLIDEAN
    for shape in ((1, 16, 1, 0, 0), (3, 16, 6, 16, 24), (17, 16, 33 * 17, 264, 136), (16, 16, 128 * 128, 1024, 1024), (4096, 4, 5, 8, 8)):
        assert lib.vt_vae_loss_backward_workspace_bytes(*shape) == vae_losses.backward_workspace_bytes(*shape) > 0, shape
    for bad in ((0, 16, 4, 8, 8), (4097, 16, 4, 8, 8), (1, 0, 4, 8, 8), (1, 16, 0, 8, 8), (1, 16, 4, 8, 0), (1, 16, 4, -1, -1)):
        assert lib.vt_vae_loss_backward_workspace_bytes(*bad) == 0, bad
    assert "vae_loss_backward.hip" in open(os.path.join(ROOT, "vae_tagger_amd", "csrc", "Makefile")).read()


def test_saved_bytes_of_the_joined_step_by_hand():
    """FLUX, B = 2, 16 x 24: three levels down, 2 x 3 latents of 16 channels.  Its own tensors: moments [6, 32, 2, 3], z [2, 16, 2, 3], recon [2, 3, 16, 24]"""
    p = {**synth.encoder_manifest(), **synth.image_decoder_manifest()}
    own = (6 * 32 * 6 + 2 * 16 * 6 + 2 * 3 * 16 * 24) * 4
    assert own == 14592
    want = vb.encoder_saved_bytes(synth.encoder_manifest(), 6, 16, 24) + vb.decoder_saved_bytes(synth.image_decoder_manifest(), 2, 2, 3) + own
    assert vb.vae_train_saved_bytes(p, 2, 16, 24) == want == vb.vae_train_saved_bytes(dict(layers_per_block=2), 2, 16, 24)
    small = dict(block_out=(64, 128, 512), layers_per_block=1)           # two levels down: 4 x 6 latents
    own = (3 * 32 * 24 + 16 * 24 + 3 * 16 * 24) * 4
    assert vb.vae_train_saved_bytes(small, 1, 16, 24) == vb.encoder_saved_bytes(small, 3, 16, 24) + vb.decoder_saved_bytes(small, 1, 4, 6) + own


def test_wrappers_refuse_without_a_device():
    c = ref.make_case(1, 4, 1, 3, seed=1)
    ins = [(m, d) for m, d in zip(c["moments"], (1, 2, 3))]
    with pytest.raises(ValueError, match="negative"):
        vae_losses.loss_backward_host(ins[0], ins[1], None, weights=FULL)
    with pytest.raises(ValueError, match="stored z"):
        vae_losses.loss_backward_host((c["moments"][0], c["moments"][0][:, :4], 1), ins[1], ins[2], weights=FULL)
    with pytest.raises(ValueError, match="moments"):
        vae_losses.loss_backward_host((None, 1), ins[1], ins[2], weights=FULL)
    with pytest.raises(ValueError, match="finite"):
        vae_losses.loss_backward_host(*ins, weights=dict(FULL, kl=float("nan")))
    with pytest.raises(ValueError, match="finite"):
        vae_losses.loss_backward_host(*ins, weights=FULL, margin=float("inf"))
    t = [(torch.from_numpy(m), d) for m, d in ins]
    with pytest.raises(ValueError, match="negative"):
        vae_losses.loss_backward_device(t[0], t[1], None, weights=FULL)
    with pytest.raises(ValueError, match="HIP device"):
        vae_losses.loss_backward_device(*t, weights=FULL)
    with pytest.raises(ValueError, match="finite"):
        vae_losses.loss_backward_device(*t, weights=dict(FULL, triplet=float("inf")))
