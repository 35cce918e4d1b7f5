"""vt_loss_* on the GPU: the accumulated state against the numpy fp64 mirrors on the same logits, the extremes of the reference fixture,
non-finite logits, bit-reproducibility of updates and of the merge, the error codes, and the absence of host synchronisation."""
import ctypes
import os

import numpy as np
import pytest
import torch

from vae_tagger_amd import _lib, losses
from vae_tagger_amd.losses import DeviceLossAccumulator, HostLossState

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQ = (16, 16, 5, 64, 1000, 3, 4096)
PAIRS = ((1.0, 2.0), (0.25, 2.0), (1.0, 0.5), (1.0, 0.0))
REL = 1e-9


def _relmax(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.isfinite(want).all() and (np.abs(want) > 0).all()
    return float(np.max(np.abs(got - want) / np.abs(want)))


def _feed(acc, xt, yt, seq=SEQ):
    lo = 0
    for b in seq:
        acc.update(xt[lo:lo + b], yt[lo:lo + b])
        lo += b
    return acc


@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("N", [1, 11, 257, 10000])
def test_update_matches_the_fp64_mirrors(N, kind):
    """All scalars and per-class sums within 1e-9 relative of the mirrors (the bound the project uses for AP: fp64 sums of at most
    4096 x 10000 terms stay orders of magnitude inside it); the largest distance of each case is printed as `max rel`."""
    rng = np.random.default_rng(1000 + N)
    rows = sum(SEQ)
    x = rng.standard_normal((rows, N), dtype=np.float32) * np.float32(3.0)
    y01 = rng.random((rows, N), dtype=np.float32) < 0.3
    if kind == "f32":                                                    # fractional labels, used as their value
        y = (y01 * rng.choice(np.array([0.25, 0.5, 0.75, 1.0], dtype=np.float32), size=(rows, N))).astype(np.float32)
    else:
        y = y01.astype(np.uint8)
    weights = losses.class_balanced_weights(rng.integers(1, 5000, N))
    starts = np.cumsum((0,) + SEQ[:-1])
    sizes = np.array(SEQ, dtype=np.float64) * N
    bce = losses.bce_elements(x, y)
    base = 1.0 - np.exp(-bce)
    bce_b = np.add.reduceat(bce, starts, axis=0)                         # [batches][N] class sums per batch
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    worst = 0.0
    for alpha, gamma in PAIRS:
        focal_b = np.add.reduceat(alpha * np.power(base, gamma) * bce, starts, axis=0)
        for w in (None, weights):
            acc = _feed(DeviceLossAccumulator(N, "cuda", alpha, gamma, w), xt, yt)
            s = acc.read_state()
            assert (s["steps"], s["elements"], s["non_finite"]) == (len(SEQ), rows * N, 0)          # counters: ==
            assert (s["alpha"], s["gamma"], s["has_weights"]) == (alpha, gamma, w is not None)
            w64 = np.ones(N) if w is None else w.astype(np.float64)
            assert s["weights"].tobytes() == w64.tobytes()
            want_scalars = [float((bce_b.sum(1) / sizes).sum()), float((focal_b.sum(1) / sizes).sum()), float(((bce_b * w64).sum(1) / sizes).sum())]
            worst = max(worst, _relmax(s["batch_mean_sums"], want_scalars), _relmax(s["class_sums"][:, 0], bce_b.sum(0)),
                        _relmax(s["class_sums"][:, 1], focal_b.sum(0)))
            if w is None:                                                # weight 1.0 and the same order of summation: the same bits
                assert s["batch_mean_sums"][2] == s["batch_mean_sums"][0]
            r = losses.finish_state(s)
            assert _relmax(r["bce"]["per_element"], bce.mean()) <= REL and _relmax(r["bce"]["mean_of_batch_means"], want_scalars[0] / len(SEQ)) <= REL
            assert (r["class_balanced"] is None) == (w is None)
    print(f"N={N} labels={kind}: max rel {worst:.3e}")
    assert worst <= REL


@pytest.fixture(scope="module")
def fixture():
    with np.load(os.path.join(ROOT, "tests", "golden", "val_loss_reference.npz"), allow_pickle=False) as z:
        return {k: z[k].copy() for k in z.files}


def test_extreme_logits_give_the_mirrors_and_the_references_values(fixture):
    x, samples = fixture["logits"], fixture["samples_per_class"]
    w = losses.class_balanced_weights(samples, float(fixture["beta"]))
    n = x.shape[1]
    for kind in ("float", "u8"):
        y = fixture[f"labels_{kind}"]
        for k, (alpha, gamma) in enumerate(PAIRS):
            acc = DeviceLossAccumulator(n, "cuda", alpha, gamma, w)
            acc.update(torch.from_numpy(x), torch.from_numpy(y))         # host tensors: uploaded without blocking
            s = acc.read_state()
            host = HostLossState(n, alpha, gamma, w)
            host.update(x, y)
            assert np.isfinite(s["class_sums"]).all() and np.isfinite(s["batch_mean_sums"]).all() and s["non_finite"] == 0
            assert _relmax(s["class_sums"], host.state["class_sums"]) <= REL and _relmax(s["batch_mean_sums"], host.state["batch_mean_sums"]) <= REL
            r = acc.read()
            got = [r["bce"]["mean_of_batch_means"], r["focal"]["mean_of_batch_means"], r["class_balanced"]["mean_of_batch_means"]]
            want = [fixture[f"bce_{kind}_f64"], fixture[f"focal_{kind}_f64"][k], fixture[f"class_balanced_{kind}_f64"]]
            d = _relmax(got, want)
            print(f"{kind} alpha={alpha} gamma={gamma}: device against the reference's fp64 values, max rel {d:.3e}")
            assert d <= REL


def test_non_finite_logits_are_counted_and_propagate():
    rng = np.random.default_rng(3)
    n = 70
    x = (rng.standard_normal((20, n)) * 3).astype(np.float32)
    y = (rng.random((20, n)) < 0.3).astype(np.float32)
    clean = DeviceLossAccumulator(n, "cuda")
    clean.update(torch.from_numpy(x), torch.from_numpy(y))
    want = clean.read_state()
    x[0, 1], x[3, 4], x[5, 66] = np.nan, np.inf, -np.inf
    y[3, 4], y[5, 66] = 0.0, 1.0                                         # the label that makes the infinite logit the wrong answer
    acc = DeviceLossAccumulator(n, "cuda")
    acc.update(torch.from_numpy(x), torch.from_numpy(y))
    s = acc.read_state()
    assert s["non_finite"] == 3 and s["steps"] == 1
    hit = np.zeros(n, dtype=bool)
    hit[[1, 4, 66]] = True
    assert not np.isfinite(s["class_sums"][hit]).any() and not np.isfinite(s["batch_mean_sums"]).any()
    assert s["class_sums"][~hit].tobytes() == want["class_sums"][~hit].tobytes()        # the other classes: untouched, the same bits
    ref = torch.nn.functional.binary_cross_entropy_with_logits(torch.from_numpy(x).double(), torch.from_numpy(y).double(), reduction="none").sum(0)
    assert not torch.isfinite(ref[torch.from_numpy(hit)]).any() and torch.isfinite(ref[torch.from_numpy(~hit)]).all()      # as torch does
    host = HostLossState(n)
    host.update(x, y)
    assert host.state["non_finite"] == 3 and not np.isfinite(host.state["class_sums"][hit]).any()
    assert not np.isfinite(acc.read()["bce"]["mean_of_batch_means"])


def _raw(acc):
    return acc.export_state().data.cpu().numpy().tobytes()


def test_the_same_calls_give_the_same_bytes_and_a_merge_is_the_in_order_sum():
    n = 1000
    rng = np.random.default_rng(8)
    w = losses.class_balanced_weights(rng.integers(1, 300, n))
    shards = []
    for k, rows in enumerate((150, 4096 + 37, 64)):
        x = (rng.standard_normal((rows, n)) * (1.0 + 50.0 * k)).astype(np.float32)       # shards of different magnitude: the order matters
        y = (rng.random((rows, n)) < 0.3).astype(np.float32)
        shards.append((torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()))
    seqs = ((16, 16, 5, 64, 49), (4096, 37), (64,))
    runs = []
    for _ in range(2):
        accs = [_feed(DeviceLossAccumulator(n, "cuda", 0.25, 2.0, w), xt, yt, seq) for (xt, yt), seq in zip(shards, seqs)]
        raws = [_raw(a) for a in accs]
        merged = DeviceLossAccumulator(n, "cuda", 0.25, 2.0, w, context=accs[0].ctx)
        merged.merge_from([a.export_state() for a in accs])
        runs.append((raws, _raw(merged), merged.read_state(), [a.read_state() for a in accs]))
    assert runs[0][0] == runs[1][0]                                      # every shard's whole block, byte for byte
    assert runs[0][1] == runs[1][1]                                      # and the merged block
    _, _, m, parts = runs[0]
    want = losses.sum_states(parts)                                      # fp64, in source order, from zero
    assert m["class_sums"].tobytes() == want["class_sums"].tobytes()
    assert m["batch_mean_sums"].tobytes() == want["batch_mean_sums"].tobytes()
    assert (m["steps"], m["elements"], m["non_finite"]) == (want["steps"], want["elements"], 0) == (5 + 2 + 1, n * (150 + 4133 + 64), 0)
    back = losses.sum_states(parts[::-1])
    assert back["class_sums"].tobytes() != want["class_sums"].tobytes()  # another order gives other bits: the order is the contract
    # merging into a state that already holds data adds to it
    first = _feed(DeviceLossAccumulator(n, "cuda", 0.25, 2.0, w), *shards[0], seqs[0])
    first.merge_from([DeviceLossAccumulator.export_state(a) for a in (_feed(DeviceLossAccumulator(n, "cuda", 0.25, 2.0, w), *shards[1], seqs[1]),)])
    got = first.read_state()
    assert got["class_sums"].tobytes() == (parts[0]["class_sums"] + parts[1]["class_sums"]).tobytes() and got["steps"] == 7
    with pytest.raises(_lib.VTError, match="another alpha"):
        first.merge_from([DeviceLossAccumulator(n, "cuda", 1.0, 2.0, w).export_state()])


def _guarded(nbytes):
    t = torch.full((nbytes + 768,), 0xA5, dtype=torch.uint8, device="cuda")
    ptr = (t.data_ptr() + 256 + 255) // 256 * 256
    return t, ptr, ptr - t.data_ptr()


def test_refusals_return_their_codes_and_write_nothing():
    ctx = _lib.Context(0)
    L, h, vp = ctx.lib, ctx.handle, ctypes.c_void_p
    OK, INVALID, WORKSPACE = 0, 1, 5
    N = 37
    nb = L.vt_loss_state_bytes(N)
    rng = np.random.default_rng(4)
    xt = torch.from_numpy((rng.standard_normal((4200, N)) * 2).astype(np.float32)).cuda()
    yt = torch.from_numpy((rng.random((4200, N)) < 0.3).astype(np.uint8)).cuda()
    w = np.ascontiguousarray(losses.class_balanced_weights(np.arange(1, N + 1)).astype(np.float64))
    w2 = w.copy()
    w2[5] *= 2
    wp = lambda a: vp(a.ctypes.data)

    def state(alpha=1.0, gamma=2.0, weights=w, rows=40):
        t, ptr, off = _guarded(nb)
        assert L.vt_loss_reset(h, vp(ptr), nb, N, alpha, gamma, wp(weights) if weights is not None else None, None) == OK
        if rows:
            assert L.vt_loss_update(h, vp(ptr), nb, N, vp(xt.data_ptr()), vp(yt.data_ptr()), _lib.VT_U8, rows, None) == OK
        return t, ptr
    dt, dp = state()
    st, sp = state(rows=25)
    torch.cuda.synchronize()
    before = (dt.cpu().numpy().tobytes(), st.cpu().numpy().tobytes())
    upd = lambda ptr, nbytes, B, dtype=_lib.VT_U8, x=xt: L.vt_loss_update(h, vp(ptr), nbytes, N, vp(x.data_ptr()), vp(yt.data_ptr()), dtype, B, None)
    assert upd(dp, nb - 1, 16) == WORKSPACE                              # undersized state
    assert b"bytes" in L.vt_last_error(h)
    assert upd(dp + 8, nb, 16) == INVALID                                # misaligned state
    assert upd(dp, nb, 4097) == INVALID and upd(dp, nb, 0) == INVALID    # B outside [1, 4096]
    assert upd(dp, nb, 16, _lib.VT_BF16) == INVALID                      # labels neither fp32 nor uint8
    assert L.vt_loss_update(h, vp(dp), nb, N, None, vp(yt.data_ptr()), _lib.VT_U8, 16, None) == INVALID
    assert L.vt_loss_update(h, vp(dp), nb, 0, vp(xt.data_ptr()), vp(yt.data_ptr()), _lib.VT_U8, 16, None) == INVALID
    assert L.vt_loss_reset(h, vp(dp), nb, N, 1.0, -0.5, None, None) == INVALID          # gamma < 0
    assert L.vt_loss_reset(h, vp(dp), nb, N, float("nan"), 2.0, None, None) == INVALID
    assert L.vt_loss_reset(h, vp(dp), nb - 256, N, 1.0, 2.0, None, None) == WORKSPACE
    out = torch.full((nb,), 0x5A, dtype=torch.uint8, device="cuda")
    assert L.vt_loss_read(h, vp(dp), nb, N, vp(out.data_ptr()), nb - 1, None) == WORKSPACE
    assert L.vt_loss_read(h, vp(dp), nb, N, None, nb, None) == INVALID

    def merge(src_ptr, alpha=1.0, gamma=2.0, weights=w, W=1, dst_alpha=1.0, src_bytes=nb):
        src = (_lib.LossSource * 1)(_lib.LossSource(src_ptr, src_bytes, alpha, gamma, weights.ctypes.data if weights is not None else None))
        return L.vt_loss_merge(h, vp(dp), nb, N, dst_alpha, 2.0, wp(w), src, W, None)
    assert merge(sp, alpha=0.25) == INVALID                              # another alpha
    assert b"another alpha" in L.vt_last_error(h)
    assert merge(sp, gamma=1.0) == INVALID                               # another gamma
    assert merge(sp, weights=w2) == INVALID and merge(sp, weights=None) == INVALID      # other weights / none
    assert merge(sp, W=0) == INVALID and merge(sp, W=65) == INVALID
    assert merge(dp) == INVALID                                          # the source is dst
    assert merge(sp + 8) == INVALID and merge(sp, src_bytes=nb - 1) == WORKSPACE
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5A).all()
    assert (dt.cpu().numpy().tobytes(), st.cpu().numpy().tobytes()) == before            # nothing was written, guards included
    # and the accepted calls stay inside the block
    assert merge(sp, weights=w.copy()) == OK                             # equal weights in another array
    assert upd(dp, nb, 4096) == OK
    torch.cuda.synchronize()
    after = dt.cpu().numpy()
    off = dp - dt.data_ptr()
    assert (after[:off] == 0xA5).all() and (after[off + nb:] == 0xA5).all()
    s = losses.parse_state(after[off:off + nb], N)
    assert (s["steps"], s["elements"]) == (1 + 1 + 1, N * (40 + 25 + 4096))


def test_update_export_and_merge_do_not_synchronise_the_host(monkeypatch):
    n = 257
    rng = np.random.default_rng(12)
    xt = torch.from_numpy((rng.standard_normal((300, n)) * 3).astype(np.float32)).cuda()
    yt = torch.from_numpy((rng.random((300, n)) < 0.3).astype(np.float32)).cuda()
    w = losses.class_balanced_weights(rng.integers(1, 100, n))
    warm = DeviceLossAccumulator(n, "cuda", class_weights=w)
    warm.update(xt, yt)
    warm.merge_from([warm.export_state()])                               # kernels loaded
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
    a, b = DeviceLossAccumulator(n, "cuda", class_weights=w, context=warm.ctx), DeviceLossAccumulator(n, "cuda", class_weights=w, context=warm.ctx)
    for lo in range(0, 300, 16):
        a.update(xt[lo:lo + 16], yt[lo:lo + 16])
    b.merge_from([a.export_state()])
    assert calls["n"] == 0
    monkeypatch.undo()
    assert b.read_state()["class_sums"].tobytes() == a.read_state()["class_sums"].tobytes() and b.read()["steps"] == 19
