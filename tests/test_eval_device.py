"""Device-side evaluator (vt_eval_* / DeviceMultiLabelEvaluator): integer counts, threshold search and average precision against the
host evaluator of vae_tagger_amd/evaluation.py, which is the oracle here and is not touched.

Bounds: everything derived from the integer counts is compared with `==` (same integers in, same fp64 formulas).  Average precision is
compared within 1e-9: both sides sum at most n non-negative fp64 terms each <= 1 (difference <= about n * 2^-53 = 2e-12 at n = 20000),
while one misplaced element of a tie group moves AP by at least about 1 / n^2 = 2.5e-9."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from vae_tagger_amd import _lib, evaluation
from vae_tagger_amd.evaluation import (THRESHOLD_GRID, MultiLabelEvaluator, _average_precision, evaluate_model, find_optimal_threshold,
                                       finish_from_counts)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vae_tagger_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
AP_TOL = 1e-9
ON_GRID = [1, 4, 8, 13]                # grid indices whose values are planted exactly, one ulp below and one ulp above
AP_KEYS = ("mAP", "mAP_micro", "mAP_weighted")


def _names(c):
    return [f"tag_{i:05d}" for i in range(c)]


def _data(n, c, seed):
    """float32 probabilities [n][c] mixing uniform values, values quantised to 1/8 (heavy ties), exact 0.0 / 1.0 and the on-threshold
    values; boolean labels with class 0 never positive and class 1 always positive."""
    rng = np.random.default_rng(seed)
    p = rng.random((n, c), dtype=np.float32)
    kind = rng.random((n, c))
    q = np.round(p * 8) / np.float32(8)
    p = np.where(kind < 0.3, q, p).astype(np.float32)
    p[kind > 0.97] = 0.0
    p[kind > 0.985] = 1.0
    special = []
    for k in ON_GRID:
        t32 = np.float32(THRESHOLD_GRID[k])
        special += [t32, np.nextafter(t32, np.float32(0)), np.nextafter(t32, np.float32(1))]
    flat = p.reshape(-1)
    pos = rng.permutation(flat.size)[:max(len(special), min(flat.size, 4 * len(special)))]
    for i, at in enumerate(pos):
        flat[at] = special[i % len(special)]
    y = rng.random((n, c)) < 0.3
    y[:, 0] = False
    if c > 1:
        y[:, 1] = True
    return p, y


def _splits(n):
    sizes, out, lo, i = (16, 16, 5, 64, 1000, 3, 4096), [], 0, 0
    while lo < n:
        b = min(sizes[i % len(sizes)], n - lo)
        out.append((lo, lo + b)); lo += b; i += 1
    return out


def _numpy_state(p, y, threshold):
    """The evaluator's integers, computed in numpy: thresholds = the grid (fp64 comparison) + float32(threshold)."""
    thr = np.concatenate([THRESHOLD_GRID, [np.float64(np.float32(threshold))]])
    n, c = p.shape
    counts = np.zeros((c, len(thr), 2), np.uint32)
    for k, t in enumerate(thr):
        pred = p > t                                         # float32 array > float64 scalar: compared in fp64
        counts[:, k, 0] = (pred & y).sum(0)
        counts[:, k, 1] = (pred & ~y).sum(0)
    pred = p > thr[-1]
    row_stats = np.array([(pred == y).all(1).sum(), (pred != y).sum(), (~np.isfinite(p)).sum()], np.uint64)
    return counts, y.sum(0).astype(np.uint32), row_stats


class _Dummy:
    def eval(self):
        return self


def _host_oracle(p, y, threshold, monkeypatch, tmp_path=None):
    """evaluate_model + find_optimal_threshold as they stand (device_metrics=False), fed (p, y) in place of a model's probabilities."""
    monkeypatch.setattr(evaluation, "_probabilities", lambda *a, **k: (p, y.astype(np.float32)))
    names = _names(p.shape[1])
    out = str(tmp_path) if tmp_path is not None else None
    m = evaluate_model(_Dummy(), _Dummy(), None, names, device="cpu", threshold=threshold, output_dir=out)
    o = find_optimal_threshold(_Dummy(), _Dummy(), None, names, device="cpu", output_dir=out)
    return m, o


def _search():
    return [(t, k) for k, t in enumerate(THRESHOLD_GRID)]


# ---- CPU --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold", [0.5, float(THRESHOLD_GRID[4]), 0.3])
def test_finish_from_counts_equals_host_evaluator_exactly(threshold, monkeypatch, capsys):
    n, c = 96, 11
    p, y = _data(n, c, seed=1)
    sup = y.sum(0)
    assert sup[0] == 0 and sup[1] == n                       # both special classes of per_class
    for k in ON_GRID:
        t32 = np.float32(THRESHOLD_GRID[k])
        assert (p == t32).any() and (p == np.nextafter(t32, np.float32(0))).any() and (p == np.nextafter(t32, np.float32(1))).any()
    # the rule under test: fp32(t) > t in fp64 for some grid values, never in fp32
    assert any(np.float64(np.float32(THRESHOLD_GRID[k])) > THRESHOLD_GRID[k] for k in ON_GRID)
    want_m, want_o = _host_oracle(p, y, threshold, monkeypatch)
    counts, support, row_stats = _numpy_state(p, y, threshold)
    ap = _average_precision(y, p)
    micro = _average_precision(y.reshape(-1, 1), p.reshape(-1, 1))[0]
    got_m, got_o = finish_from_counts(counts, support, row_stats, n, ap, micro, len(THRESHOLD_GRID), _names(c), _search())
    assert got_m == want_m
    assert got_o == want_o
    assert list(got_m) == list(want_m) and list(got_m["per_class"]["tag_00002"]) == list(want_m["per_class"]["tag_00002"])
    # without a ranking the AP keys are left out, nothing else changes
    no_ap = finish_from_counts(counts, support, row_stats, n, None, None, len(THRESHOLD_GRID), _names(c))[0]
    assert not any(k in no_ap for k in AP_KEYS) and "ap" not in no_ap["per_class"]["tag_00002"]
    assert {k: v for k, v in no_ap.items() if k != "per_class"} == {k: v for k, v in want_m.items() if k not in AP_KEYS + ("per_class",)}
    row_stats[2] = 1
    with pytest.raises(FloatingPointError):
        finish_from_counts(counts, support, row_stats, n, ap, micro, len(THRESHOLD_GRID), _names(c))


def test_header_and_prototypes_carry_the_evaluator():
    header = open(os.path.join(ROOT, "include", "vae_tagger_hip.h")).read()
    for name in ("vt_eval_state_bytes", "vt_eval_reset", "vt_eval_update", "vt_eval_grow", "vt_eval_ap_workspace_bytes",
                 "vt_eval_average_precision", "vt_eval_read_counts"):
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.PROTOTYPES, name
    assert re.search(r"VT_U8\s*=\s*3", header) and _lib.VT_U8 == 3 and (_lib.VT_F32, _lib.VT_BF16, _lib.VT_F16) == (0, 1, 2)


def test_state_and_workspace_sizes_are_host_arithmetic():
    L = _lib.load()
    sb, wb = L.vt_eval_state_bytes, L.vt_eval_ap_workspace_bytes
    base = sb(100, 17, 64)
    assert base > 0 and base % 256 == 0
    assert sb(101, 17, 64) >= base and sb(100, 18, 64) >= base and sb(100, 17, 65) >= base
    assert sb(10000, 17, 2048) > sb(10000, 17, 0) >= 10000 * 17 * 8 and sb(10000, 17, 2048) - sb(10000, 17, 0) >= 10000 * 2048 * 8
    assert sb(100, 33, 64) == 0 and sb(0, 17, 64) == 0 and sb(100, 17, -1) == 0
    w = wb(100, 64)
    assert w >= 100 * 64 * 8 and w % 256 == 0 and wb(101, 64) >= w and wb(100, 65) >= w
    assert wb(10000, 214748) > 0 and wb(10000, 214749) == 0          # micro AP on the device while n * N < 2^31


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_eval_kernels_compile_without_scratch_and_without_scalar_stores(tmp_path):
    out = tmp_path / "eval_metrics.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "-S", "--cuda-device-only",
           "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", str(out), os.path.join(CSRC, "eval_metrics.hip")]
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    asm = out.read_text()
    meta = {}
    for block in asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1))
                      for k in ("private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count")}
    for kernel in ("eval_accumulate_kernel", "eval_sort_local_kernel", "eval_ap_kernel"):
        hit = {k: v for k, v in meta.items() if kernel in k}
        assert hit, (kernel, list(meta))
        for name, v in hit.items():
            assert v == {"private_segment_fixed_size": 0, "sgpr_spill_count": 0, "vgpr_spill_count": 0}, (name, v)
    words = [a + b for a, b in (("s_st", "ore"), ("s_buffer_st", "ore"), ("s_scratch_st", "ore"), ("s_ato", "mic"), ("s_buffer_ato", "mic"),
                                ("s_dcache_", "wb"), ("s_dcache_", "discard"))]
    for f in ("eval_metrics.hip", "vt_eval.h", "vt_sort_network.h"):
        text = open(os.path.join(CSRC, f)).read().lower()
        assert not any(w in text for w in words), f
    assert not any(w in asm.lower() for w in words)


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
def _feed(ev, p, y, labels, splits=None):
    pt = torch.from_numpy(p).cuda()
    yt = torch.from_numpy(y.astype(np.float32) if labels == "f32" else y.astype(np.uint8)).cuda()
    for lo, hi in (splits or _splits(len(p))):
        ev.update(pt[lo:hi], yt[lo:hi])
    return ev


def _strip_ap(m):
    out = {k: v for k, v in m.items() if k not in AP_KEYS + ("per_class",)}
    out["per_class"] = {n: {k: v for k, v in d.items() if k != "ap"} for n, d in m["per_class"].items()}
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("labels", ["f32", "u8"])
@pytest.mark.parametrize("n,c", [(1, 11), (37, 11), (48, 10000), (16385, 7)])
def test_counts_are_exact(n, c, labels, monkeypatch, capsys):
    p, y = _data(n, c, seed=n + c)
    threshold = float(THRESHOLD_GRID[4])                     # an on-threshold operating point: fp32 comparison there, fp64 on the grid
    ev = _feed(evaluation.DeviceMultiLabelEvaluator(_names(c), "cuda", threshold=threshold, capacity=0), p, y, labels)
    counts, support, row_stats, ap, micro = ev.read_state()
    assert ap is None and micro is None
    want = _numpy_state(p, y, threshold)
    assert np.array_equal(counts, want[0]) and np.array_equal(support, want[1]) and np.array_equal(row_stats, want[2])
    want_m, want_o = _host_oracle(p, y, threshold, monkeypatch)
    with pytest.warns(UserWarning, match="capacity=0"):
        got_m = ev.compute_metrics()
    assert got_m == _strip_ap(want_m)
    assert ev.optimal_thresholds() == want_o


@pytest.mark.gpu
@pytest.mark.parametrize("n,c", [(1, 11), (37, 11), (48, 10000), (16384, 7), (16385, 7), (20000, 7)])
def test_average_precision(n, c, monkeypatch, capsys):
    p, y = _data(n, c, seed=3 * n + c)
    ev = _feed(evaluation.DeviceMultiLabelEvaluator(_names(c), "cuda", threshold=0.5), p, y, "u8")       # capacity grows from 1024
    got = ev.compute_metrics()
    want, _ = _host_oracle(p, y, 0.5, monkeypatch)
    _, _, _, ap, micro = ev.read_state()                     # a second finish on the already sorted store: same values
    ref = _average_precision(y, p)
    assert np.array_equal(np.isnan(ap), np.isnan(ref)) and np.isnan(ref[0])
    worst = float(np.nanmax(np.abs(ap - ref))) if n > 1 or c > 1 else 0.0
    ref_micro = float(_average_precision(y.reshape(-1, 1), p.reshape(-1, 1))[0])
    print(f"AP n={n} c={c}: max |d ap| = {worst:.3e}, |d micro| = {abs(micro - ref_micro):.3e}")
    assert worst <= AP_TOL and abs(micro - ref_micro) <= AP_TOL
    for k in AP_KEYS:
        assert abs(got[k] - want[k]) <= AP_TOL, k
    for name, d in want["per_class"].items():
        assert abs(got["per_class"][name]["ap"] - d["ap"]) <= AP_TOL, name
    assert _strip_ap(got) == _strip_ap(want)
    if c <= 11:
        try:
            from sklearn.metrics import average_precision_score
        except ImportError:
            return
        for j in range(c):
            if 0 < y[:, j].sum():
                assert abs(ap[j] - average_precision_score(y[:, j], p[:, j])) <= AP_TOL, j


def _keys_of(ev):
    head = ev.ctx.lib.vt_eval_state_bytes(ev.N, ev.T, 0)
    off = ev._ptr - ev._buf.data_ptr() + head
    return ev._buf[off:off + ev.N * ev.capacity * 8].view(torch.int64).view(ev.N, ev.capacity)[:, :ev.n_seen].clone()


@pytest.mark.gpu
def test_two_runs_are_bit_identical_and_the_batch_split_does_not_matter():
    n, c = 5000, 37
    p, y = _data(n, c, seed=9)
    runs = []
    for splits in (None, None, [(0, 7), (7, 4103), (4103, 4104), (4104, n)]):
        ev = _feed(evaluation.DeviceMultiLabelEvaluator(_names(c), "cuda", capacity=n), p, y, "f32", splits)
        keys = _keys_of(ev)
        state = ev.read_state()
        runs.append((keys, _keys_of(ev)) + state)
    a, b, s = runs
    for x, z in zip(a, b):                                   # unsorted keys, sorted keys, counts, support, row_stats, ap, micro
        assert (torch.equal(x, z) if isinstance(x, torch.Tensor) else np.array_equal(np.asarray(x), np.asarray(z), equal_nan=True))
    for i in (2, 3, 4):
        assert np.array_equal(a[i], s[i])
    assert np.nanmax(np.abs(a[5] - s[5])) <= AP_TOL and abs(a[6] - s[6]) <= AP_TOL
    assert torch.equal(a[0], s[0])                           # a key depends on the sample's position in the stream, not on its batch


@pytest.fixture(scope="module")
def vae():
    from vae_tagger_amd import synth
    from vae_tagger_amd.diffusers_vae_loader import DiffusersVAEWrapper, get_diffusers_vae_config, load_diffusers_vae_from_config
    m = load_diffusers_vae_from_config(get_diffusers_vae_config())
    missing, unexpected = m.load_state_dict(synth.synth_state_dict(synth.encoder_manifest(), seed=0), strict=False)
    assert not missing and not unexpected
    return DiffusersVAEWrapper(m).to("cuda").eval()


def _decoder(n):
    from vae_tagger_amd import synth
    from vae_tagger_amd.modules import create_attention_decoder
    d = create_attention_decoder(16, 16, 16, n, {"use_spatial_attention": True, "use_self_attention": True, "use_cross_attention": False,
                                                 "attention_heads": 8})
    missing, unexpected = d.load_state_dict(synth.synth_state_dict(synth.attention_decoder_manifest(n, 16, True, True, False), seed=1), strict=False)
    assert not missing and not unexpected
    return d.to("cuda").eval()


def _loader(n_tags, on_device=False):
    from vae_tagger_amd import synth
    g = torch.Generator().manual_seed(5)
    batches = []
    for i in range(3):
        x = synth.synth_images(2, 64, 64, seed=40 + i)
        lab = (torch.rand(2, n_tags, generator=g) < 0.4).float()
        batches.append({"pixel_values": x.cuda() if on_device else x, "labels": lab.cuda() if on_device else lab})
    return batches


def _same_files(host_dir, dev_dir):
    """The written files, field by field: every count-derived field is the same text; an AP field (summed in another order on the device:
    numpy adds a[0] to the sum of the rest, the kernel adds left to right) is the same number within AP_TOL."""
    jh, jd = (json.load(open(d / "evaluation_results_overall.json")) for d in (host_dir, dev_dir))
    assert list(jh) == list(jd)
    for k in jh:
        assert abs(jh[k] - jd[k]) <= AP_TOL if k in AP_KEYS else jh[k] == jd[k], k
    rh, rd = ((d / "evaluation_results.csv").read_text().splitlines() for d in (host_dir, dev_dir))
    assert len(rh) == len(rd) and rh[0] == rd[0] == "class_name,precision,recall,f1,ap,support"
    for a, b in zip(rh[1:], rd[1:]):
        fa, fb = a.split(","), b.split(",")
        assert fa[:4] == fb[:4] and fa[5] == fb[5] and abs(float(fa[4]) - float(fb[4])) <= AP_TOL, (a, b)


@pytest.mark.gpu
def test_end_to_end_device_metrics_equal_the_host_path(vae, tmp_path, capsys):
    n_tags = 11
    dec, names, batches = _decoder(n_tags), _names(n_tags), _loader(n_tags)
    host_dir, dev_dir = tmp_path / "host", tmp_path / "device"
    for thr in (0.5, 0.47):
        mh = evaluate_model(vae, dec, batches, names, device="cuda", threshold=thr, output_dir=str(host_dir))
        md = evaluate_model(vae, dec, batches, names, device="cuda", threshold=thr, output_dir=str(dev_dir), device_metrics=True)
        assert list(md) == list(mh)
        assert _strip_ap(md) == _strip_ap(mh)
        for k in AP_KEYS:
            assert abs(md[k] - mh[k]) <= AP_TOL, k
        for name in names:
            assert abs(md["per_class"][name]["ap"] - mh["per_class"][name]["ap"]) <= AP_TOL
        _same_files(host_dir, dev_dir)
    oh = find_optimal_threshold(vae, dec, batches, names, device="cuda", output_dir=str(host_dir))
    od = find_optimal_threshold(vae, dec, batches, names, device="cuda", output_dir=str(dev_dir), device_metrics=True)
    assert od == oh
    assert (host_dir / "optimal_thresholds.json").read_text() == (dev_dir / "optimal_thresholds.json").read_text()
    assert json.load(open(dev_dir / "optimal_thresholds.json")) == od


@pytest.mark.gpu
def test_no_host_synchronisation_between_updates(vae, monkeypatch, capsys):
    n_tags = 11
    dec, names, batches = _decoder(n_tags), _names(n_tags), _loader(n_tags, on_device=True)
    evaluate_model(vae, dec, batches, names, device="cuda", device_metrics=True)          # weights uploaded, kernels loaded
    calls = {"n": 0}
    marks = []

    def counted(fn):
        def wrapper(*a, **k):
            calls["n"] += 1
            return fn(*a, **k)
        return wrapper
    monkeypatch.setattr(torch.cuda, "synchronize", counted(torch.cuda.synchronize))
    for name in ("cpu", "item", "numpy"):
        monkeypatch.setattr(torch.Tensor, name, counted(getattr(torch.Tensor, name)))
    real_update = evaluation.DeviceMultiLabelEvaluator.update

    def update(self, *a, **k):
        marks.append(calls["n"])
        out = real_update(self, *a, **k)
        marks.append(calls["n"])
        return out
    monkeypatch.setattr(evaluation.DeviceMultiLabelEvaluator, "update", update)
    evaluate_model(vae, dec, batches, names, device="cuda", device_metrics=True)
    find_optimal_threshold(vae, dec, batches, names, device="cuda", device_metrics=True)
    assert len(marks) == 4 * len(batches)
    for leg in (marks[:2 * len(batches)], marks[2 * len(batches):]):
        assert leg[-1] - leg[0] == 0, marks


def _aligned(nbytes, guard=4096, pat=0xA5):
    t = torch.full((nbytes + 256 + 2 * guard,), pat, dtype=torch.uint8, device="cuda")
    p = (t.data_ptr() + guard + 255) // 256 * 256
    return t, p, p - t.data_ptr()


@pytest.mark.gpu
def test_error_paths_are_refused_on_the_host_and_writes_stay_inside_the_buffers():
    ctx = _lib.Context(0)
    L, h, vp = ctx.lib, ctx.handle, ctypes.c_void_p
    N, T, cap, B = 37, 17, 64, 16
    thr = (ctypes.c_double * 33)(*([0.5] * 33))
    nbytes = L.vt_eval_state_bytes(N, T, cap)
    st, sp, so = _aligned(nbytes)
    p, y = _data(3 * B, N, seed=4)
    pt, yt = torch.from_numpy(p).cuda(), torch.from_numpy(y.astype(np.uint8)).cuda()
    assert L.vt_eval_reset(h, vp(sp), nbytes, N, T, thr, 16, cap, None) == 0
    for i in range(3):
        assert L.vt_eval_update(h, vp(sp), nbytes, N, T, 16, cap, vp(pt[i * B:].data_ptr()), vp(yt[i * B:].data_ptr()), _lib.VT_U8, B, i * B, None) == 0
    torch.cuda.synchronize()
    before = st.clone()

    def refused(rc, code):
        assert rc == code, rc
        assert L.vt_last_error(h)
        torch.cuda.synchronize()
        assert torch.equal(st, before)
    ap = torch.zeros(N + 1, dtype=torch.float64, device="cuda")
    wbytes = L.vt_eval_ap_workspace_bytes(N, 3 * B)
    wt, wp, wo = _aligned(wbytes)
    upd = (vp(pt.data_ptr()), vp(yt.data_ptr()), _lib.VT_U8)
    refused(L.vt_eval_update(h, vp(sp), nbytes - 256, N, T, 16, cap, *upd, B, 0, None), 5)                 # undersized state: VT_ERR_WORKSPACE
    refused(L.vt_eval_update(h, vp(sp), nbytes, N, T, 16, cap, *upd, B, cap - B + 1, None), 1)             # n_seen + B > capacity
    refused(L.vt_eval_reset(h, vp(sp), 1 << 30, N, 33, thr, 16, cap, None), 1)                             # T = 33
    refused(L.vt_eval_reset(h, vp(sp), nbytes, N, T, thr, T, cap, None), 1)                                # t_main outside [0, T)
    refused(L.vt_eval_update(h, vp(sp), nbytes, N, T, -1, cap, *upd, B, 0, None), 1)
    refused(L.vt_eval_average_precision(h, vp(sp), nbytes, N, T, cap, 3 * B, vp(ap.data_ptr()), N * 8, vp(ap.data_ptr() + 8 * N), vp(wp + 8),
                                        wbytes, None), 1)                                                  # misaligned workspace
    refused(L.vt_eval_average_precision(h, vp(sp), nbytes, N, T, cap, 3 * B, vp(ap.data_ptr()), N * 8, vp(ap.data_ptr() + 8 * N), vp(wp),
                                        wbytes - 256, None), 5)                                            # undersized workspace
    refused(L.vt_eval_update(h, vp(sp + 8), nbytes, N, T, 16, cap, *upd, B, 0, None), 1)                   # misaligned state
    assert bool((ap == 0).all()) and bool((wt == 0xA5).all())
    # guard bands: the state holds exactly n_seen = capacity samples; update + AP leave both sides of both buffers alone
    assert L.vt_eval_update(h, vp(sp), nbytes, N, T, 16, cap, vp(pt[2 * B:].data_ptr()), vp(yt[2 * B:].data_ptr()), _lib.VT_U8, B, 3 * B, None) == 0
    wbytes = L.vt_eval_ap_workspace_bytes(N, cap)
    wt, wp, wo = _aligned(wbytes)
    assert L.vt_eval_average_precision(h, vp(sp), nbytes, N, T, cap, cap, vp(ap.data_ptr()), N * 8, vp(ap.data_ptr() + 8 * N), vp(wp), wbytes, None) == 0
    torch.cuda.synchronize()
    for t, off, nb in ((st, so, nbytes), (wt, wo, wbytes)):
        assert bool((t[:off] == 0xA5).all()) and bool((t[off + nb:] == 0xA5).all())
    p4 = np.concatenate([p, p[2 * B:]]); y4 = np.concatenate([y, y[2 * B:]])
    ref = _average_precision(y4, p4)
    got = ap.cpu().numpy()
    assert np.nanmax(np.abs(got[:N] - ref)) <= AP_TOL
    assert abs(got[N] - _average_precision(y4.reshape(-1, 1), p4.reshape(-1, 1))[0]) <= AP_TOL
