"""Export and merge of device evaluator states (vt_eval_export / vt_eval_merge, DeviceMultiLabelEvaluator.export_state / merge_from).

The oracle is ONE DeviceMultiLabelEvaluator fed the whole matrix: W evaluators fed contiguous shards of it, exported and merged in
order, must hold the same state byte for byte (thresholds, row_stats, support, counts, key columns [0, n) of every class row) before
any sort -- every quantity is an integer or a copied bit pattern, so there is no tolerance anywhere in this file."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from vae_tagger_amd import _lib, evaluation
from vae_tagger_amd.evaluation import THRESHOLD_GRID, DeviceMultiLabelEvaluator, EvalStateBlock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vae_tagger_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
INVALID, WORKSPACE = 1, 5                                   # VT_ERR_INVALID, VT_ERR_WORKSPACE
WORDS = [a + b for a, b in (("s_st", "ore"), ("s_buffer_st", "ore"), ("s_scratch_st", "ore"), ("s_ato", "mic"), ("s_buffer_ato", "mic"),
                            ("s_dcache_", "wb"), ("s_dcache_", "discard"))]


def _names(c):
    return [f"tag_{i:05d}" for i in range(c)]


def _data(n, c, seed):
    """float32 probabilities with heavy ties, exact 0 / 1 and on-threshold values; class 0 never positive, class 1 always."""
    rng = np.random.default_rng(seed)
    p = rng.random((n, c), dtype=np.float32)
    kind = rng.random((n, c))
    p = np.where(kind < 0.3, np.round(p * 8) / np.float32(8), p).astype(np.float32)
    p[kind > 0.97] = 0.0
    p[kind > 0.985] = 1.0
    p[kind < 0.02] = np.float32(THRESHOLD_GRID[4])
    y = rng.random((n, c)) < 0.3
    y[:, 0] = False
    if c > 1:
        y[:, 1] = True
    return p, y


def _shards(n, W, seed):
    """W contiguous [lo, hi) shards of n samples in order: ragged, and (W >= 2) at least one empty."""
    rng = np.random.default_rng(seed)
    cuts = sorted(int(x) for x in rng.integers(0, n + 1, size=max(0, W - 1)))
    if W >= 2:
        k = int(rng.integers(0, W - 1))
        cuts = sorted(cuts[:k] + [cuts[k - 1] if k else 0] + cuts[k + 1:])          # a repeated cut: an empty shard
    edges = [0] + cuts + [n]
    out = [(edges[i], edges[i + 1]) for i in range(W)]
    assert sum(hi - lo for lo, hi in out) == n and (W < 2 or any(hi == lo for lo, hi in out))
    return out


def _align(x):
    return (x + 255) // 256 * 256


def _layout(N, T, cap):
    """The block layout the header documents (every section 256-B aligned)."""
    thr = 0
    row_stats = thr + _align(8 * 32)
    row_scratch = row_stats + _align(8 * 3)
    support = row_scratch + _align(4 * 4096)
    counts = support + _align(4 * N)
    keys = counts + _align(4 * 2 * N * T)
    return {"thr": (thr, 8 * 32), "row_stats": (row_stats, 24), "row_scratch": (row_scratch, 4 * 4096), "support": (support, 4 * N),
            "counts": (counts, 8 * N * T), "keys": keys, "total": keys + _align(8 * N * cap)}


def _block_bytes(ev):
    off = ev._ptr - ev._buf.data_ptr()
    return ev._buf[off:off + ev._bytes]


def _sections(data, N, T, cap, n):
    """(head sections as byte tensors, keys [N][n] as int64) of a state block given as a uint8 tensor."""
    L = _layout(N, T, cap)
    assert data.numel() == L["total"] == _lib.load().vt_eval_state_bytes(N, T, cap)
    head = {k: data[L[k][0]:L[k][0] + L[k][1]].clone() for k in ("thr", "row_stats", "row_scratch", "support", "counts")}
    keys = None
    if cap:
        keys = data[L["keys"]:L["keys"] + 8 * N * cap].view(torch.int64).view(N, cap)[:, :n].clone()
    return head, keys


def _same_state(a, b):
    (ha, ka), (hb, kb) = a, b
    for k in ha:
        assert torch.equal(ha[k], hb[k]), k
    assert (ka is None) == (kb is None)
    if ka is not None:
        assert ka.shape == kb.shape and torch.equal(ka, kb)


def _feed(ev, pt, yt, lo, hi, step=1000):
    for a in range(lo, hi, step):
        ev.update(pt[a:min(hi, a + step)], yt[a:min(hi, a + step)])
    return ev


def _tensors(p, y, labels):
    return torch.from_numpy(p).cuda(), torch.from_numpy(y.astype(np.float32) if labels == "f32" else y.astype(np.uint8)).cuda()


# ---- CPU --------------------------------------------------------------------------------------------------------------------------
def test_header_and_prototypes_carry_export_and_merge():
    header = open(os.path.join(ROOT, "include", "vae_tagger_hip.h")).read()
    for name in ("vt_eval_export", "vt_eval_merge"):
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.PROTOTYPES, name
    assert re.search(r"typedef struct \{[^}]*state;[^}]*state_bytes;[^}]*capacity;[^}]*n_seen;[^}]*\} vt_eval_source;", header)
    assert [f[0] for f in _lib.EvalSource._fields_] == ["state", "state_bytes", "capacity", "n_seen"]
    assert ctypes.sizeof(_lib.EvalSource) == 32
    assert len(_lib.PROTOTYPES["vt_eval_export"][1]) == 11 and len(_lib.PROTOTYPES["vt_eval_merge"][1]) == 10
    L = _lib.load()
    assert L.vt_eval_export and L.vt_eval_merge


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_merge_kernels_compile_without_scratch_spills_lds_or_atomics(tmp_path):
    out = tmp_path / "eval_metrics.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "-S", "--cuda-device-only",
           "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", str(out), os.path.join(CSRC, "eval_metrics.hip")]
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    asm = out.read_text()
    meta = {}
    for block in asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1))
                      for k in ("private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count", "group_segment_fixed_size")}
    for kernel, variants in (("eval_merge_keys_kernel", 2), ("eval_merge_head_kernel", 1)):
        hit = {k: v for k, v in meta.items() if kernel in k}
        assert len(hit) == variants, (kernel, list(meta))
        for name, v in hit.items():
            assert v == {"private_segment_fixed_size": 0, "sgpr_spill_count": 0, "vgpr_spill_count": 0, "group_segment_fixed_size": 0}, (name, v)
            start = asm.index("\n" + name + ":")
            body = asm[start:asm.index("s_endpgm", start)]
            assert not re.search(r"\b(global|flat|buffer|ds)_atomic|\bds_(read|write)|scratch_", body), name
            assert "global_load" in body and "global_store" in body
    wide = [b for n, b in ((n, asm[asm.index("\n" + n + ":"):]) for n in meta if "eval_merge_keys_kernelILi2" in n)]
    assert wide and "global_store_dwordx4" in wide[0][:wide[0].index("s_endpgm")]
    assert not any(w in asm.lower() for w in WORDS)


def test_forbidden_instruction_words_are_absent_from_the_sources():
    files = [os.path.join(CSRC, f) for f in ("eval_metrics.hip", "vt_eval.h", "capi.hip", "vt_context.h")]
    files += [os.path.join(ROOT, "include", "vae_tagger_hip.h"), os.path.join(ROOT, "tools", "bench_eval.py"), __file__,
              os.path.join(ROOT, "tests", "test_evaluate_sharded.py")]
    files += [os.path.join(ROOT, "vae_tagger_amd", f) for f in ("evaluation.py", "evaluate.py", "_lib.py", "sharding.py", "prefetch.py")]
    for f in files:
        text = open(f, encoding="utf-8").read().lower()
        assert not any(w in text for w in WORDS), f


def _desc(**kw):
    d = {"N": 11, "T": 17, "t_main": 16, "thresholds": np.arange(17, dtype=np.float64).tobytes(), "keys": True, "n_seen": 5, "error": None}
    d.update(kw)
    return d


def test_descriptor_check_is_a_pure_function():
    check = evaluation.check_rank_descriptors
    assert check([_desc(), _desc(n_seen=0), _desc(n_seen=9)]) is None
    other = np.arange(17, dtype=np.float64)
    other[3] = np.nextafter(other[3], 9.0)
    with pytest.raises(ValueError, match="rank 1 .*threshold table"):
        check([_desc(), _desc(thresholds=other.tobytes())])
    with pytest.raises(ValueError, match="rank 2 .*number of classes"):
        check([_desc(), _desc(), _desc(N=12)])
    with pytest.raises(RuntimeError, match=r"rank 1: FloatingPointError: boom"):
        check([_desc(), _desc(error="FloatingPointError: boom"), _desc(N=12)])       # an error wins over a mismatch
    with pytest.raises(ValueError, match="key store"):
        check([_desc(), _desc(keys=False)])
    # the same input gives the same exception text: what lets every rank raise alike
    texts = []
    for _ in range(2):
        with pytest.raises(RuntimeError) as e:
            check([_desc(error="x"), _desc(error="y")])
        texts.append(str(e.value))
    assert texts[0] == texts[1] and "rank 0: x" in texts[0] and "rank 1: y" in texts[0]


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("labels", ["f32", "u8"])
@pytest.mark.parametrize("W", [1, 2, 3, 8])
@pytest.mark.parametrize("n,c", [(1, 11), (37, 11), (48, 10000), (16385, 7)])
def test_merged_shards_equal_the_single_evaluator_byte_for_byte(n, c, W, labels):
    p, y = _data(n, c, seed=n + c + W)
    pt, yt = _tensors(p, y, labels)
    single = _feed(DeviceMultiLabelEvaluator(_names(c), "cuda", threshold=0.5, capacity=n), pt, yt, 0, n)
    shards = _shards(n, W, seed=7 * n + W)
    parts = [_feed(DeviceMultiLabelEvaluator(_names(c), "cuda", threshold=0.5), pt, yt, lo, hi) for lo, hi in shards]     # capacity grows from 1024
    cap = max(e.n_seen for e in parts)
    blocks = [e.export_state(cap) for e in parts]
    assert len({b.data.numel() for b in blocks}) == 1                       # one size: the wire format
    merged = DeviceMultiLabelEvaluator(_names(c), "cuda", threshold=0.5, capacity=n)
    merged.merge_from(blocks)
    assert merged.n_seen == n
    _same_state(_sections(_block_bytes(merged), c, merged.T, n, n), _sections(_block_bytes(single), c, single.T, n, n))
    assert merged.optimal_thresholds() == single.optimal_thresholds()
    got, want = merged.compute_metrics(), single.compute_metrics()
    assert got == want and "mAP_micro" in got


@pytest.mark.gpu
def test_the_8_byte_variant_and_odd_pitches_give_the_same_bytes():
    n, c = 2999, 37                                                         # odd column offsets and odd pitches: every alignment case
    p, y = _data(n, c, seed=3)
    pt, yt = _tensors(p, y, "u8")
    single = _feed(DeviceMultiLabelEvaluator(_names(c), "cuda", capacity=n), pt, yt, 0, n)
    want = _sections(_block_bytes(single), c, single.T, n, n)
    shards = [(0, 701), (701, 701), (701, 1702), (1702, n)]
    parts = [_feed(DeviceMultiLabelEvaluator(_names(c), "cuda"), pt, yt, lo, hi) for lo, hi in shards]
    for flag in (1, 0):
        for cap in (1297, 1298):                                            # odd and even source pitch
            single.ctx.call("vt_set_flag", 21, flag)
            try:
                merged = DeviceMultiLabelEvaluator(_names(c), "cuda", capacity=n, context=single.ctx)
                blocks = []
                for e in parts:
                    e.ctx.call("vt_set_flag", 21, flag)
                    blocks.append(e.export_state(cap))
                    e.ctx.call("vt_set_flag", 21, 1)
                merged.merge_from(blocks)
            finally:
                single.ctx.call("vt_set_flag", 21, 1)
            _same_state(_sections(_block_bytes(merged), c, merged.T, n, n), want)


def _guarded(nbytes, guard=1 << 20, pat=0xA5):
    t = torch.full((nbytes + 256 + 2 * guard,), pat, dtype=torch.uint8, device="cuda")
    p = (t.data_ptr() + guard + 255) // 256 * 256
    return t, p, p - t.data_ptr()


@pytest.mark.gpu
def test_export_compacts_zero_fills_the_padding_and_stays_inside_its_block():
    n, c, out_cap = 1500, 37, 1600
    p, y = _data(n, c, seed=5)
    pt, yt = _tensors(p, y, "u8")
    ev = _feed(DeviceMultiLabelEvaluator(_names(c), "cuda", capacity=2048), pt, yt, 0, n)
    L, h, vp = ev.ctx.lib, ev.ctx.handle, ctypes.c_void_p
    nbytes = L.vt_eval_state_bytes(c, ev.T, out_cap)
    t, ptr, off = _guarded(nbytes)
    assert L.vt_eval_export(h, vp(ev._ptr), ev._bytes, c, ev.T, 2048, n, vp(ptr), nbytes, out_cap, None) == 0
    torch.cuda.synchronize()
    assert bool((t[:off] == 0xA5).all()) and bool((t[off + nbytes:] == 0xA5).all()) and off >= 1 << 20
    out = t[off:off + nbytes]
    head, keys = _sections(out, c, ev.T, out_cap, out_cap)
    src_head, src_keys = _sections(_block_bytes(ev), c, ev.T, 2048, n)
    for k in head:
        assert torch.equal(head[k], src_head[k]), k
    assert not bool(head["row_scratch"].any())
    assert torch.equal(keys[:, :n], src_keys) and not bool(keys[:, n:].any())
    lay = _layout(c, ev.T, out_cap)
    assert not bool(out[lay["keys"] + 8 * c * out_cap:].any())             # the section's alignment tail is zero too
    # the bytes are a function of the data only: the method gives the same block from another allocation
    again = ev.export_state(out_cap)
    assert torch.equal(again.data, out) and again.capacity == out_cap and again.n_seen == n
    assert ev.export_state().capacity == n                                  # default: compact to n_seen


@pytest.mark.gpu
def test_head_only_export_and_merge_at_capacity_0():
    n, c = 300, 11
    p, y = _data(n, c, seed=6)
    pt, yt = _tensors(p, y, "f32")
    single = _feed(DeviceMultiLabelEvaluator(_names(c), "cuda", capacity=0), pt, yt, 0, n)
    a = _feed(DeviceMultiLabelEvaluator(_names(c), "cuda", capacity=0), pt, yt, 0, 120)
    b = _feed(DeviceMultiLabelEvaluator(_names(c), "cuda"), pt, yt, 120, n)            # keeps keys; exported head only
    blocks = [a.export_state(), b.export_state(0)]
    assert [bl.capacity for bl in blocks] == [0, 0]
    assert blocks[0].data.numel() == _lib.load().vt_eval_state_bytes(c, a.T, 0) == _layout(c, a.T, 0)["total"]
    merged = DeviceMultiLabelEvaluator(_names(c), "cuda", capacity=0)
    merged.merge_from(blocks)
    assert merged.n_seen == n
    _same_state(_sections(_block_bytes(merged), c, merged.T, 0, 0), _sections(_block_bytes(single), c, single.T, 0, 0))
    assert merged.optimal_thresholds() == single.optimal_thresholds()
    with pytest.warns(UserWarning, match="capacity=0"):
        got = merged.compute_metrics()
    with pytest.warns(UserWarning, match="capacity=0"):
        assert got == single.compute_metrics()


@pytest.mark.gpu
@pytest.mark.parametrize("fixed", [True, False])
def test_merge_into_a_non_empty_state_then_update(fixed):
    n, c = 5000, 37
    p, y = _data(n, c, seed=8)
    pt, yt = _tensors(p, y, "u8")
    single = _feed(DeviceMultiLabelEvaluator(_names(c), "cuda", capacity=n), pt, yt, 0, n)
    dst = _feed(DeviceMultiLabelEvaluator(_names(c), "cuda", capacity=n if fixed else None), pt, yt, 0, 1001)
    b = _feed(DeviceMultiLabelEvaluator(_names(c), "cuda"), pt, yt, 1001, 2500)
    d = _feed(DeviceMultiLabelEvaluator(_names(c), "cuda"), pt, yt, 2500, 4097)
    dst.merge_from([b.export_state(), d.export_state(1600)])
    assert dst.n_seen == 4097
    _feed(dst, pt, yt, 4097, n)
    cap = dst.capacity
    assert (cap == n) if fixed else (cap >= n)
    _same_state(_sections(_block_bytes(dst), c, dst.T, cap, n), _sections(_block_bytes(single), c, single.T, n, n))
    assert dst.compute_metrics() == single.compute_metrics()


@pytest.mark.gpu
def test_two_runs_are_bit_identical():
    n, c, W = 6000, 101, 8
    p, y = _data(n, c, seed=10)
    pt, yt = _tensors(p, y, "f32")
    shards = _shards(n, W, seed=2)
    runs = []
    for _ in range(2):
        parts = [_feed(DeviceMultiLabelEvaluator(_names(c), "cuda"), pt, yt, lo, hi) for lo, hi in shards]
        cap = max(e.n_seen for e in parts)
        blocks = [e.export_state(cap) for e in parts]
        merged = DeviceMultiLabelEvaluator(_names(c), "cuda", capacity=n)
        merged.merge_from(blocks)
        runs.append(([b.data.clone() for b in blocks], _sections(_block_bytes(merged), c, merged.T, n, n), merged.compute_metrics()))
    for x, z in zip(runs[0][0], runs[1][0]):
        assert torch.equal(x, z)                                            # the exported blocks, padding included
    _same_state(runs[0][1], runs[1][1])
    assert runs[0][2] == runs[1][2]


@pytest.mark.gpu
def test_export_and_merge_do_not_synchronise_the_host(monkeypatch):
    n, c = 900, 37
    p, y = _data(n, c, seed=12)
    pt, yt = _tensors(p, y, "u8")
    parts = [_feed(DeviceMultiLabelEvaluator(_names(c), "cuda"), pt, yt, lo, hi) for lo, hi in ((0, 400), (400, n))]
    merged = DeviceMultiLabelEvaluator(_names(c), "cuda", capacity=n)
    merged.merge_from([e.export_state(500) for e in parts])                  # kernels loaded
    merged = DeviceMultiLabelEvaluator(_names(c), "cuda", capacity=n)
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
    blocks = [e.export_state(500) for e in parts]
    merged.merge_from(blocks)
    assert calls["n"] == 0
    monkeypatch.undo()
    single = _feed(DeviceMultiLabelEvaluator(_names(c), "cuda", capacity=n), pt, yt, 0, n)
    assert merged.compute_metrics() == single.compute_metrics()


@pytest.mark.gpu
def test_refusals_return_their_codes_and_write_nothing():
    ctx = _lib.Context(0)
    L, h, vp = ctx.lib, ctx.handle, ctypes.c_void_p
    N, T, cap, n = 37, 17, 64, 40
    thr = (ctypes.c_double * T)(*([0.5] * T))
    p, y = _data(n, N, seed=4)
    pt, yt = _tensors(p, y, "u8")
    sb = L.vt_eval_state_bytes

    def state(capacity, rows):
        nb = sb(N, T, capacity)
        t, ptr, off = _guarded(nb)
        assert L.vt_eval_reset(h, vp(ptr), nb, N, T, thr, 16, capacity, None) == 0
        for lo in range(0, rows, 16):
            b = min(16, rows - lo)
            assert L.vt_eval_update(h, vp(ptr), nb, N, T, 16, capacity, vp(pt[lo:].data_ptr()), vp(yt[lo:].data_ptr()), _lib.VT_U8, b, lo, None) == 0
        return t, ptr, nb

    dt, dp, db = state(cap, 10)                   # dst: 10 samples of 64
    s1t, s1p, s1b = state(cap, n)                 # 40 samples
    s2t, s2p, s2b = state(cap, 14)                # 14 samples
    s0t, s0p, s0b = state(0, n)                   # counts only, 40 samples
    e0t, e0p, e0b = state(0, 0)                   # counts only, empty
    ot, op, ob = _guarded(sb(N, T, 48))           # an export target, never written
    ob = sb(N, T, 48)
    torch.cuda.synchronize()
    every = (dt, s1t, s0t, e0t, ot, s2t)
    before = [t.clone() for t in every]

    def refused(rc, code):
        assert rc == code, rc
        assert L.vt_last_error(h)
        torch.cuda.synchronize()
        for t, b in zip(every, before):
            assert torch.equal(t, b)

    def src(*items):
        return (_lib.EvalSource * max(1, len(items)))(*[_lib.EvalSource(*it) for it in items])
    one = (s1p, s1b, cap, n)
    merge = lambda *a: L.vt_eval_merge(h, *a)
    refused(merge(vp(dp), db, N, T, cap, 10, src(one), 0, None), INVALID)                               # W < 1
    refused(merge(vp(dp), db, N, T, cap, 10, src(*([(s1p, s1b, cap, 0)] * 65)), 65, None), INVALID)     # W > 64
    refused(merge(vp(dp), db, N, T, cap, 10, None, 1, None), INVALID)                                   # null sources
    refused(merge(vp(dp), db, N, T, cap, 10, src((dp, db, cap, 10)), 1, None), INVALID)                 # a source that is dst
    refused(merge(vp(dp), db, N, T, cap, 10, src((dp + 256, db - 256, 0, 0)), 1, None), INVALID)        # a source inside dst
    refused(merge(vp(dp), db, N, T, cap, 10, src((s0p, s0b, 0, n)), 1, None), INVALID)                  # no keys for its samples, dst keeps keys
    refused(merge(vp(dp), db, N, T, cap, 10, src(one, (s2p, s2b, cap, 14), (s2p, s2b, cap, 1)), 3, None), INVALID)  # 10 + 40 + 14 + 1 > 64
    refused(merge(vp(dp), db, N, T, cap, 10, src((s1p, s1b, cap, cap + 1)), 1, None), INVALID)          # n_seen beyond the source's capacity
    refused(merge(vp(e0p), e0b, N, T, 0, 2 ** 31 - 30, src((s0p, s0b, 0, n)), 1, None), INVALID)        # a total of 2^31 or more
    refused(merge(vp(dp), db - 256, N, T, cap, 10, src(one), 1, None), WORKSPACE)                       # undersized dst
    refused(merge(vp(dp), db, N, T, cap, 10, src((s1p, s1b - 256, cap, n)), 1, None), WORKSPACE)        # undersized source
    refused(merge(vp(dp + 8), db, N, T, cap, 10, src(one), 1, None), INVALID)                           # misaligned dst
    refused(merge(vp(dp), db, N, T, cap, 10, src((s1p + 8, s1b, cap, n)), 1, None), INVALID)            # misaligned source
    refused(merge(vp(dp), db, N, T, cap, 10, src((0, s1b, cap, n)), 1, None), INVALID)                  # null source
    refused(merge(vp(dp), db, N, 33, cap, 10, src(one), 1, None), INVALID)                              # T = 33
    export = lambda *a: L.vt_eval_export(h, *a)
    refused(export(vp(s1p), s1b, N, T, cap, n, vp(op), ob, 39, None), INVALID)                          # 0 < out_capacity < n_seen
    refused(export(vp(s1p), s1b, N, T, cap, cap + 1, vp(op), ob, 0, None), INVALID)                     # n_seen beyond the capacity
    refused(export(vp(s0p), s0b, N, T, 0, n, vp(op), ob, 48, None), INVALID)                            # keys asked of a state without
    refused(export(vp(s1p), s1b, N, T, cap, n, vp(op), ob - 256, 48, None), WORKSPACE)                  # undersized output
    refused(export(vp(s1p), s1b - 256, N, T, cap, n, vp(op), ob, 48, None), WORKSPACE)                  # undersized state
    refused(export(vp(s1p), s1b, N, T, cap, n, vp(op + 8), ob, 48, None), INVALID)                      # misaligned output
    refused(export(vp(s1p), s1b, N, T, cap, n, vp(0), ob, 48, None), INVALID)                           # null output
    refused(export(vp(s1p), s1b, N, T, cap, n, vp(s1p), s1b, cap, None), INVALID)                       # out_state is the state
    # and the accepted calls stay inside their blocks: merge to exactly full, export at exactly n_seen
    assert merge(vp(dp), db, N, T, cap, 10, src(one, (s2p, s2b, cap, 14)), 2, None) == 0
    nb40 = sb(N, T, n)
    xt, xp, xo = _guarded(nb40)
    assert export(vp(s1p), s1b, N, T, cap, n, vp(xp), nb40, n, None) == 0
    torch.cuda.synchronize()
    for t, ptr, nb in ((dt, dp, db), (xt, xp, nb40)):
        off = ptr - t.data_ptr()
        assert bool((t[:off] == 0xA5).all()) and bool((t[off + nb:] == 0xA5).all())
    for t, b in zip(every[1:], before[1:]):
        assert torch.equal(t, b)                                            # sources are read only
    ev = DeviceMultiLabelEvaluator(_names(N), "cuda", thresholds=[0.5] * 16, threshold=0.5, capacity=cap, context=ctx)
    order = np.concatenate([np.arange(10), np.arange(n), np.arange(14)])
    idx = torch.from_numpy(order).cuda()
    _feed(ev, pt[idx], yt[idx], 0, cap)
    off = dp - dt.data_ptr()
    _same_state(_sections(dt[off:off + db], N, T, cap, cap), _sections(_block_bytes(ev), N, T, cap, cap))


@pytest.mark.gpu
def test_merge_from_checks_thresholds_and_capacity():
    c = 11
    p, y = _data(64, c, seed=1)
    pt, yt = _tensors(p, y, "u8")
    a = _feed(DeviceMultiLabelEvaluator(_names(c), "cuda", threshold=0.5), pt, yt, 0, 64)
    other = DeviceMultiLabelEvaluator(_names(c), "cuda", threshold=0.4, capacity=64)
    with pytest.raises(ValueError, match="thresholds"):
        other.merge_from([a.export_state()])
    small = DeviceMultiLabelEvaluator(_names(c), "cuda", threshold=0.5, capacity=32)
    with pytest.raises(ValueError, match="capacity 32"):
        small.merge_from([a.export_state()])
    blk = a.export_state()
    assert isinstance(blk, EvalStateBlock) and blk.t_main == a.t_main and blk.data.data_ptr() % 256 == 0
    assert evaluation.merge_across_ranks(a) is a                             # no process group: the evaluator itself
