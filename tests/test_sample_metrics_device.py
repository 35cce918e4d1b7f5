"""vt_sample_* / DeviceSampleEvaluator on the device against sample_metrics_host: the integer tallies are equal, the three fp64 sums lie
within n * 2^-53 * 4 of the host's (the bound of an n-term fp64 sum of values in [0, 1]; n <= 51 here: below 1e-13), the bytes of two
runs are identical; vt_sample_from_keys against vt_sample_update and the host, before and after the rows are ranked and on a merged
state; and the refusals, each of which leaves a sentinel-filled state untouched."""
import ctypes

import numpy as np
import pytest
import torch

from vae_tagger_amd import _lib, sample_metrics as sm
from vae_tagger_amd.evaluation import DeviceMultiLabelEvaluator

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRID32 = np.concatenate([np.round(np.arange(1, 20) * 0.05, 2), [0.3, 0.5, 0.999, 0.0, 1.0, -1.0, 2.0, 0.123, 0.77, 0.5000001, 0.25, 0.625, 0.875]])
INT_KEYS = ("exact_matches", "images_without_prediction", "images_without_true_tag", "nonfinite_probabilities", "total_images")


def _data(n, N, thresholds, seed):
    """fp32 probabilities with the edge cases planted: a row without a positive label, a row without a prediction, one NaN, one +inf and
    one -inf probability, and values exactly on thresholds."""
    g = np.random.default_rng(seed)
    p = g.random((n, N)).astype(np.float32)
    y = (g.random((n, N)) < 0.2).astype(np.uint8)
    extra = g.integers(0, 3, n).astype(np.uint32)
    y[0] = 0; extra[0] = 0                                   # no true tag at all
    if n > 1:
        p[1] = np.float32(-0.5)                              # predicts under none of the positive thresholds
    for k, t in enumerate(thresholds):
        p[(k + 2) % n, (3 * k + 1) % N] = np.float32(t)     # on the threshold when fp32(t) == t, next to it otherwise
    p[n - 1, N - 1] = np.float32(0.5); y[n - 1, N - 1] = 1   # the row's last element (the masked tail's neighbour) sits on 0.5
    p[n // 2, N // 2] = np.nan
    p[n // 2, 0] = np.inf
    p[(n // 2 + 1) % n, N // 3] = -np.inf
    return p, y, extra


def _check(results, host, n):
    assert len(results) == len(host)
    bound = n * 2.0 ** -53 * 4
    for got, want in zip(results, host):
        for k in INT_KEYS:
            assert got[k] == want[k], (k, got[k], want[k])
        for k in ("sum_precision", "sum_recall", "sum_f1"):
            print(f"{k}: device {got[k]!r} host {want[k]!r} |diff| {abs(got[k] - want[k]):.3e} bound {bound:.3e}")
            assert abs(got[k] - want[k]) <= bound, (k, got[k], want[k])
        assert got["exact_match_rate"] == want["exact_match_rate"]
        assert got["samples_recall_sklearn"] == (got["sum_recall"] - got["images_without_true_tag"]) / n


@pytest.mark.parametrize("T", [1, 32])
@pytest.mark.parametrize("B", [1, 3, 17])
@pytest.mark.parametrize("N", [11, 257, 1000, 10000])
def test_update_matches_the_host(N, B, T):
    thresholds = GRID32[:T] if T > 1 else np.asarray([0.5])
    for rule in ("ge", "gt"):
        n = 3 * B                                            # two updates: B rows as uint8 labels, then 2 B rows as float32 (n_seen > 0)
        p, y, extra = _data(n, N, thresholds, seed=N * 100 + B * 3 + T)
        host = sm.sample_metrics_host(p, y, thresholds, rule, extra)
        true_h, rows_h = sm.sample_tallies_host(p, y, thresholds, rule, extra)
        raws = []
        for _ in range(2):                                   # a second evaluator fed the same data
            ev = sm.DeviceSampleEvaluator(thresholds, rule, DEV, capacity=n)
            ev.update(torch.from_numpy(p[:B]).to(DEV), torch.from_numpy(y[:B]).to(DEV), extra[:B])
            ev.update(torch.from_numpy(p[B:]).to(DEV), torch.from_numpy(y[B:].astype(np.float32) * 0.25).to(DEV), extra[B:])
            r1, r2 = ev.finish_raw(), ev.finish_raw()        # finish twice
            torch.cuda.synchronize()
            assert bytes(r1.numpy()) == bytes(r2.numpy())
            raws.append(bytes(r1.numpy()))
        assert raws[0] == raws[1]
        true_d, rows_d = ev.read_rows()
        assert np.array_equal(true_d, true_h) and np.array_equal(rows_d, rows_h)
        _check(ev.finish(), host, n)
        per = ev.per_image()
        P, R, F, exact = sm.per_image_values(rows_h[:, :, 0], rows_h[:, :, 1], true_h[:, None])
        assert np.array_equal(per["precision"], P) and np.array_equal(per["recall"], R) and np.array_equal(per["f1"], F)
        assert np.array_equal(per["exact_match"], exact) and ev.best_threshold() == sm.best_threshold(host)


def test_planted_threshold_values_split_the_two_rules():
    p = np.full((3, 300), 0.25, dtype=np.float32)
    p[0, 299] = p[1, 64] = p[2, 0] = np.float32(0.5)
    y = np.zeros((3, 300), dtype=np.uint8)
    y[0, 299] = y[1, 64] = 1
    ge, gt = sm.DeviceSampleEvaluator([0.5], "ge", DEV, capacity=3), sm.DeviceSampleEvaluator([0.5], "gt", DEV, capacity=3)
    for ev in (ge, gt):
        ev.update(p, y)
    assert ge.read_rows()[1][:, 0].tolist() == [[1, 1], [1, 1], [0, 1]] and gt.read_rows()[1][:, 0].tolist() == [[0, 0]] * 3
    assert ge.finish()[0]["exact_matches"] == 2 and gt.finish()[0]["images_without_prediction"] == 3


def test_capacity_grows_by_doubling_through_a_device_copy():
    thresholds = [0.3, 0.6]
    p, y, extra = _data(40, 33, thresholds, seed=5)
    ev = sm.DeviceSampleEvaluator(thresholds, "ge", DEV)
    ev.capacity, ev._buf, ev._ptr, ev._bytes = (8,) + ev._alloc(8)          # a small first block, reset as the constructor does
    ev.ctx.call("vt_sample_reset", ctypes.c_void_p(ev._ptr), ev._bytes, ev.T, (ctypes.c_double * 2)(*thresholds), 1, 8, ev._stream())
    for lo in range(0, 40, 7):
        ev.update(p[lo:lo + 7], y[lo:lo + 7], extra[lo:lo + 7])
    assert ev.capacity == 64 and ev.n_seen == 40
    true_h, rows_h = sm.sample_tallies_host(p, y, thresholds, "ge", extra)
    true_d, rows_d = ev.read_rows()
    assert np.array_equal(true_d, true_h) and np.array_equal(rows_d, rows_h)
    _check(ev.finish(), sm.sample_metrics_host(p, y, thresholds, "ge", extra), 40)


@pytest.fixture(scope="module")
def keyed():
    """N = 257, 40 samples in three updates: the data, the evaluator with its key store, and one built by vt_eval_merge of two halves."""
    N, n = 257, 40
    p, y, extra = _data(n, N, [0.5, 0.3], seed=77)
    names = [f"t{k}" for k in range(N)]

    def feed(lo, hi, cuts):
        ev = DeviceMultiLabelEvaluator(names, DEV, thresholds=[0.3], threshold=0.5, capacity=n)
        for a, b in zip(cuts[:-1], cuts[1:]):
            ev.update(torch.from_numpy(p[lo + a:lo + b]).to(DEV), torch.from_numpy(y[lo + a:lo + b]).to(DEV))
        return ev
    whole = feed(0, n, [0, 13, 14, 40])
    merged = DeviceMultiLabelEvaluator(names, DEV, thresholds=[0.3], threshold=0.5, capacity=n)
    merged.merge_from([feed(0, 19, [0, 19]).export_state(), feed(19, n, [0, 21]).export_state()])
    torch.cuda.synchronize()
    return {"p": p, "y": y, "extra": extra, "whole": whole, "merged": merged, "N": N, "n": n}


def test_from_keys_equals_update_and_the_host(keyed):
    p, y, extra, n, N = keyed["p"], keyed["y"], keyed["extra"], keyed["n"], keyed["N"]
    g = np.random.default_rng(3)
    random_thr = g.random(N)
    random_thr[:8] = p[5, :8].astype(np.float64)                       # per-class thresholds some probabilities sit on
    for rule in ("ge", "gt"):
        for thr in (0.5, 0.3):
            up = sm.DeviceSampleEvaluator([thr], rule, DEV, capacity=n)
            up.update(p, y, extra)
            fk = sm.DeviceSampleEvaluator.from_evaluator(keyed["whole"], thr, rule, extra)
            (ta, ra), (tb, rb) = up.read_rows(), fk.read_rows()
            assert np.array_equal(ta, tb) and np.array_equal(ra, rb)
            a, b = up.finish(), fk.finish()
            assert a == b
        true_h, rows_h = sm.sample_tallies_host(p, y, random_thr[None, :], rule, extra)
        for source in ("whole", "merged"):
            fk = sm.DeviceSampleEvaluator.from_evaluator(keyed[source], random_thr, rule, extra)
            true_d, rows_d = fk.read_rows()
            assert np.array_equal(true_d, true_h) and np.array_equal(rows_d, rows_h), source
            _check(fk.finish(), sm.finish_host(true_h, rows_h, int((~np.isfinite(p)).sum())), n)
    # unchanged after vt_eval_average_precision has sorted the rows in place
    before = sm.DeviceSampleEvaluator.from_evaluator(keyed["whole"], random_thr, "ge", extra)
    raw_before, rows_before = before.finish_raw(), before.read_rows()
    keyed["whole"].read_state(with_ap=True)
    after = sm.DeviceSampleEvaluator.from_evaluator(keyed["whole"], random_thr, "ge", extra)
    raw_after, rows_after = after.finish_raw(), after.read_rows()
    assert np.array_equal(rows_before[0], rows_after[0]) and np.array_equal(rows_before[1], rows_after[1])
    assert bytes(raw_before.numpy()) == bytes(raw_after.numpy())


def test_refusals_leave_the_state_untouched():
    L = _lib.load()
    ctx = _lib.Context(0)
    h, vp = ctx.handle, ctypes.c_void_p
    OK, INVALID, WORKSPACE = 0, 1, 5
    T, cap, N = 4, 16, 50
    nb = L.vt_sample_state_bytes(T, cap)
    buf = torch.full((nb + 512,), 0xA5, dtype=torch.uint8, device=DEV)
    ptr = (buf.data_ptr() + 255) // 256 * 256
    p = torch.rand(4097, N, device=DEV)
    y = torch.zeros(4097, N, dtype=torch.uint8, device=DEV)
    thr = (ctypes.c_double * 33)(*([0.5] * 33))
    out = torch.empty(L.vt_sample_finish_bytes(T), dtype=torch.uint8, device=DEV)

    def update(state=ptr, nbytes=nb, T_=T, B=2, n_seen=0):
        return L.vt_sample_update(h, vp(state), nbytes, T_, cap, vp(p.data_ptr()), vp(y.data_ptr()), _lib.VT_U8, None, B, N, n_seen, None)
    assert L.vt_sample_reset(h, vp(ptr), nb, 33, thr, 1, cap, None) == INVALID                      # T = 33
    assert L.vt_sample_reset(h, vp(ptr), nb, T, thr, 2, cap, None) == INVALID                       # no such rule
    assert L.vt_sample_reset(h, vp(ptr + 64), nb, T, thr, 1, cap, None) == INVALID                  # misaligned state
    assert L.vt_sample_reset(h, vp(ptr), nb - 256, T, thr, 1, cap, None) == WORKSPACE               # undersized buffer
    assert update(T_=33) == INVALID and update(B=4097) == INVALID and update(B=0) == INVALID
    assert update(B=2, n_seen=15) == INVALID                                                         # n_seen + B > capacity
    assert update(state=ptr + 128) == INVALID and update(nbytes=nb - 256) == WORKSPACE
    assert L.vt_sample_finish(h, vp(ptr), nb, T, cap, 17, vp(out.data_ptr()), out.numel(), None) == INVALID
    assert L.vt_sample_finish(h, vp(ptr), nb, T, cap, 4, vp(out.data_ptr()), out.numel() - 8, None) == WORKSPACE
    assert L.vt_sample_read_rows(h, vp(ptr), nb, T, cap, 4, vp(out.data_ptr()), 8, vp(out.data_ptr()), 8, None) == WORKSPACE
    assert L.vt_sample_from_keys(h, vp(ptr), nb, N, 2, 0, 0, vp(out.data_ptr()), 1, None, vp(ptr), nb, cap, None) == INVALID      # no key store
    assert b"capacity" in L.vt_last_error(h)
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all())
    assert L.vt_sample_reset(h, vp(ptr), nb, T, thr, 1, cap, None) == OK and update(B=16) == OK
    torch.cuda.synchronize()
    assert not bool((buf[ptr - buf.data_ptr():ptr - buf.data_ptr() + nb] == 0xA5).all()) and bool((buf[ptr - buf.data_ptr() + nb:] == 0xA5).all())
