"""vt_eval_recount / DeviceMultiLabelEvaluator.recount / compute_metrics_at on the device: against the state's own counters, against the
host evaluator, before and after the in-place sort, on a merged state, and the error paths.  Integers are compared with ==; average
precision within 1e-9, the bound tests/test_eval_device.py derives (AP does not depend on the threshold)."""
import ctypes

import numpy as np
import pytest
import torch

from vae_tagger_amd import _lib
from vae_tagger_amd.evaluation import THRESHOLD_GRID, DeviceMultiLabelEvaluator, MultiLabelEvaluator

pytestmark = pytest.mark.gpu
AP_TOL = 1e-9
AP_KEYS = ("mAP", "mAP_micro", "mAP_weighted")


def _names(c):
    return [f"tag_{i:05d}" for i in range(c)]


def _data(n, c, seed):
    """fp32 probabilities with heavy ties, exact 0 / 1 and values on / one ulp around grid thresholds; class 0 never positive, class 1 always."""
    rng = np.random.default_rng(seed)
    p = rng.random((n, c), dtype=np.float32)
    kind = rng.random((n, c))
    p = np.where(kind < 0.3, np.round(p * 8) / np.float32(8), p).astype(np.float32)
    p[kind > 0.97] = 0.0
    p[kind > 0.985] = 1.0
    flat = p.reshape(-1)
    special = []
    for k in (1, 4, 8, 13):
        t32 = np.float32(THRESHOLD_GRID[k])
        special += [t32, np.nextafter(t32, np.float32(0)), np.nextafter(t32, np.float32(1))]
    for i, at in enumerate(rng.permutation(flat.size)[:4 * len(special)]):
        flat[at] = special[i % len(special)]
    y = rng.random((n, c)) < 0.3
    y[:, 0] = False
    y[:, 1] = True
    return p, y


def _feed(ev, p, y, sizes=(16, 16, 5, 64, 1000, 3, 700)):
    lo, i = 0, 0
    while lo < len(p):
        b = min(sizes[i % len(sizes)], len(p) - lo)
        ev.update(torch.from_numpy(p[lo:lo + b]).cuda(), torch.from_numpy(y[lo:lo + b]).cuda())
        lo += b; i += 1


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_recount_reproduces_the_states_own_counters_across_a_grow():
    n, c = 2500, 101
    p, y = _data(n, c, 1)
    ev = DeviceMultiLabelEvaluator(_names(c), "cuda", threshold=0.4)      # capacity None: starts at 1024 and grows twice
    _feed(ev, p, y)
    assert ev.capacity == 4096 and ev.n_seen == n
    counts, support, row_stats, _, _ = ev.read_state(with_ap=False)
    for k in range(len(ev.grid)):
        got, _ = ev.recount(ev.grid[k])
        assert np.array_equal(got, counts[:, k, :]), k
    got, got_rows = ev.recount(ev.thr[ev.t_main])
    assert np.array_equal(got, counts[:, ev.t_main, :]) and np.array_equal(got_rows, row_stats)
    assert got.dtype == np.uint32 and got_rows.dtype == np.uint64 and got.shape == (c, 2) and got_rows.shape == (3,)
    # the state was only read
    again = ev.read_state(with_ap=False)
    assert np.array_equal(again[0], counts) and np.array_equal(again[2], row_stats)


@pytest.mark.parametrize("n,c,capacity", [(777, 11, 777), (3000, 257, 3001), (1, 5, 1)])
def test_compute_metrics_at_equals_the_host_evaluator(n, c, capacity):
    """capacity 777 / 3001: odd row pitches, so every second class row starts on a key that is not 16-B aligned."""
    p, y = _data(n, c, 2)
    rng = np.random.default_rng(3)
    vec = rng.choice(THRESHOLD_GRID, size=c)
    vec[: c // 2] = np.round(rng.random(c // 2) * 8) / 8      # values the probabilities hold exactly: equal does not pass
    ev = DeviceMultiLabelEvaluator(_names(c), "cuda", capacity=capacity)
    _feed(ev, p, y)
    for thr, pred in ((vec, p > vec[None, :]), (0.35, p > 0.35)):          # a Python float compares in fp32, as in evaluate_model
        host = MultiLabelEvaluator(_names(c), "cpu")
        host.update(pred.astype(np.float32), y.astype(np.float32), p)
        want, got = host.compute_metrics(), ev.compute_metrics_at(thr)
        assert list(got) == list(want)
        for k in want:
            if k in AP_KEYS:
                assert abs(got[k] - want[k]) <= AP_TOL, (k, got[k], want[k])
            elif k != "per_class":
                assert got[k] == want[k], (k, got[k], want[k])
        for name, w in want["per_class"].items():
            g = got["per_class"][name]
            assert {k: v for k, v in g.items() if k != "ap"} == {k: v for k, v in w.items() if k != "ap"}, name
            assert abs(g["ap"] - w["ap"]) <= AP_TOL, name
    no_ap = ev.compute_metrics_at(vec, with_ap=False)
    assert not any(k in no_ap for k in AP_KEYS)


def test_recount_does_not_depend_on_the_sort_or_on_a_merge():
    n, c = 1800, 67
    p, y = _data(n, c, 4)
    vec = np.random.default_rng(5).choice(THRESHOLD_GRID, size=c)
    one = DeviceMultiLabelEvaluator(_names(c), "cuda", capacity=n + 1)
    _feed(one, p, y)
    before = (one.recount(vec), one.recount(0.5))
    one.read_state(with_ap=True)                             # vt_eval_average_precision sorts every class row in place
    after = (one.recount(vec), one.recount(0.5))
    assert _same(before[0], after[0]) and _same(before[1], after[1])
    assert int(before[0][1][1]) > 0 and int(before[0][1][0]) < n          # the tally is exercised: some rows match, most do not
    cuts = [0, 1, 700, n]                                    # three unequal shards
    shards = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        ev = DeviceMultiLabelEvaluator(_names(c), "cuda", capacity=hi - lo + 3, context=one.ctx)
        _feed(ev, p[lo:hi], y[lo:hi])
        shards.append(ev)
    shards[1].read_state(with_ap=True)                       # one shard arrives sorted
    merged = DeviceMultiLabelEvaluator(_names(c), "cuda", capacity=n, context=one.ctx)
    merged.merge_from([s.export_state() for s in shards])
    assert merged.n_seen == n
    assert _same(merged.recount(vec), before[0]) and _same(merged.recount(0.5), before[1])


def test_recount_error_paths_leave_the_outputs_untouched():
    n, c = 300, 9
    p, y = _data(n, c, 6)
    ev = DeviceMultiLabelEvaluator(_names(c), "cuda", capacity=n)
    _feed(ev, p, y)
    lib, ctx = ev.ctx.lib, ev.ctx
    ws_bytes = lib.vt_eval_recount_workspace_bytes(c, n)
    ws = torch.zeros(ws_bytes + 256, dtype=torch.uint8, device="cuda")
    wp = (ws.data_ptr() + 255) // 256 * 256
    thr = torch.full((c,), 0.5, dtype=torch.float64, device="cuda")
    guard = 64
    counts = torch.full((guard + 2 * c + guard,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    rows = torch.full((guard + 3 + guard,), 0x5a5a5a5a5a5a, dtype=torch.int64, device="cuda")
    cp, rp = counts.data_ptr() + 4 * guard, rows.data_ptr() + 8 * guard
    stream = ev._stream()
    vp = ctypes.c_void_p

    def call(state=ev._ptr, sbytes=ev._bytes, capacity=ev.capacity, n_seen=n, thr_p=thr.data_ptr(), c_p=cp, cb=8 * c, r_p=rp, rb=24, w_p=wp, wb=ws_bytes):
        return lib.vt_eval_recount(ctx.handle, vp(state), sbytes, c, ev.T, capacity, n_seen, vp(thr_p), vp(c_p), cb, vp(r_p), rb, vp(w_p), wb, stream)

    W, I = 5, 1                                               # VT_ERR_WORKSPACE, VT_ERR_INVALID
    assert call(wb=ws_bytes - 1) == W and call(cb=8 * c - 1) == W and call(rb=23) == W and call(sbytes=ev._bytes - 1) == W
    assert call(capacity=0, sbytes=lib.vt_eval_state_bytes(c, ev.T, 0)) == I           # no key store, n_seen > 0
    assert call(n_seen=n + 1) == I and call(n_seen=-1) == I
    assert call(thr_p=0) == I and call(c_p=0) == I and call(r_p=0) == I and call(w_p=0) == I and call(state=0) == I
    assert call(w_p=wp + 8) == I and call(thr_p=thr.data_ptr() + 4) == I and call(r_p=rp + 4) == I and call(state=ev._ptr + 16) == I
    torch.cuda.synchronize()
    assert (counts == 0x5a5a5a5a).all() and (rows == 0x5a5a5a5a5a5a).all()            # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    want_counts, want_rows = ev.recount(0.5)
    assert np.array_equal(counts[guard:guard + 2 * c].cpu().numpy().view(np.uint32).reshape(c, 2), want_counts)
    assert np.array_equal(rows[guard:guard + 3].cpu().numpy().view(np.uint64), want_rows)
    assert (counts[:guard] == 0x5a5a5a5a).all() and (counts[guard + 2 * c:] == 0x5a5a5a5a).all()
    assert (rows[:guard] == 0x5a5a5a5a5a5a).all() and (rows[guard + 3:] == 0x5a5a5a5a5a5a).all()
    # an empty state with a key store is valid: all zero
    empty = DeviceMultiLabelEvaluator(_names(c), "cuda", capacity=8, context=ctx)
    assert call(state=empty._ptr, sbytes=empty._bytes, capacity=8, n_seen=0) == 0
    torch.cuda.synchronize()
    assert int(counts[guard:guard + 2 * c].abs().sum()) == 0 and int(rows[guard:guard + 3].abs().sum()) == 0
    # the Python wrapper refuses a counts-only evaluator before the C call
    bare = DeviceMultiLabelEvaluator(_names(c), "cuda", capacity=0, context=ctx)
    bare.update(torch.from_numpy(p[:8]).cuda(), torch.from_numpy(y[:8]).cuda())
    with pytest.raises(ValueError, match="key store"):
        bare.recount(0.5)
    with pytest.raises(ValueError, match="thresholds"):
        ev.recount(np.zeros(c + 1))
    assert isinstance(_lib.VTError("x"), RuntimeError)
