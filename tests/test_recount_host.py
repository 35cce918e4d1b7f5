"""Host side of the recount / per-class-threshold feature: a numpy model of vt_eval_recount against the host evaluator, the one-pass
search + evaluation on the host matrix against the two existing functions (byte for byte), the CLI refusals, the thresholds-file
loader, the host reference of the per-class summary, and the ABI surface of the built library.  All comparisons are of integers or of
floats computed from the same integers by the same formulas: exact."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from vae_tagger_amd import _lib, evaluate, evaluation, infer_full
from vae_tagger_amd.evaluation import (THRESHOLD_GRID, MultiLabelEvaluator, _average_precision, evaluate_and_search, evaluate_model,
                                       find_optimal_threshold, finish_from_counts, threshold_vector)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _names(c):
    return [f"tag_{i:05d}" for i in range(c)]


def encode_keys(p, y):
    """The key store as include/vae_tagger_hip.h documents it, class-major [c][n]: high word = the monotone unsigned map of the fp32
    bits (NaN -> 1, -0 -> +0), low word = (~sample << 1) | label."""
    n, c = p.shape
    u = np.ascontiguousarray(p.T, dtype=np.float32).view(np.uint32).copy()
    u[u == np.uint32(0x80000000)] = 0
    hi = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    hi[np.isnan(p.T)] = 1
    sample = np.arange(n, dtype=np.uint32)[None, :]
    lo = ((~sample) << np.uint32(1)) | (y.T > 0).astype(np.uint32)
    return (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)


def recount_model(keys, thr):
    """vt_eval_recount in numpy: decode, decide with > in fp64, tally per class and per SAMPLE (taken from the key, not the column)."""
    c, n = keys.shape
    hi = (keys >> np.uint64(32)).astype(np.uint32)
    lo = (keys & np.uint64(0xffffffff)).astype(np.uint32)
    bits = np.where(hi & np.uint32(0x80000000), hi & np.uint32(0x7fffffff), ~hi).astype(np.uint32)
    p = bits.view(np.float32).copy()
    p[hi == 1] = np.nan
    y = (lo & np.uint32(1)).astype(bool)
    sample = ((~lo) >> np.uint32(1)).astype(np.int64)
    thr = np.broadcast_to(np.asarray(thr, dtype=np.float64), (c,))
    pred = p.astype(np.float64) > thr[:, None]
    counts = np.stack([(pred & y).sum(1), (pred & ~y).sum(1)], axis=1).astype(np.uint32)
    tally = np.zeros(n, np.int64)
    np.add.at(tally, sample[pred != y], 1)
    return counts, np.array([(tally == 0).sum(), tally.sum(), (~np.isfinite(p)).sum()], np.uint64)


def _data(n, c, seed, thr_vec=None):
    rng = np.random.default_rng(seed)
    p = rng.random((n, c), dtype=np.float32)
    p[rng.random((n, c)) < 0.3] = np.float32(0.5)                        # heavy ties
    y = rng.random((n, c)) < 0.3
    y[:, 0] = False                                                      # a class without a positive
    y[:, 1] = True                                                       # a class with every sample positive
    if thr_vec is not None:                                              # probabilities EQUAL to their class threshold: strict, do not pass
        for j in range(c):
            t32 = np.float32(thr_vec[j])
            if np.float64(t32) == thr_vec[j]:
                p[rng.integers(0, n, 3), j] = t32
    return p, y


@pytest.mark.parametrize("per_class", [False, True])
def test_numpy_recount_model_equals_the_host_evaluator(per_class):
    n, c = 150, 13
    rng = np.random.default_rng(7)
    vec = np.round(rng.random(c) * 16) / 16 if per_class else np.full(c, 0.5)      # multiples of 1/16: exact in fp32
    if per_class:
        vec[2] = float(THRESHOLD_GRID[3])                                # and one grid value that fp32 does not hold
    p, y = _data(n, c, 3, vec)
    assert any((p[:, j] == np.float32(vec[j])).any() for j in range(c))
    keys = encode_keys(p, y)
    for order in ("as stored", "rows shuffled"):
        if order == "rows shuffled":                                     # what the in-place sort does to the columns: any permutation per row
            keys = np.stack([row[np.random.default_rng(j).permutation(n)] for j, row in enumerate(keys)])
        counts, row_stats = recount_model(keys, vec if per_class else 0.5)
        pred = p > vec[None, :]                                          # float32 matrix > float64 row: compared in fp64
        assert np.array_equal(counts[:, 0], (pred & y).sum(0)) and np.array_equal(counts[:, 1], (pred & ~y).sum(0))
        for j in range(c):                                               # equal to the threshold: strict, does not pass
            if np.float64(np.float32(vec[j])) == vec[j]:
                assert not pred[p[:, j] == np.float32(vec[j]), j].any()
        assert row_stats.tolist() == [(pred == y).all(1).sum(), (pred != y).sum(), 0]
        host = MultiLabelEvaluator(_names(c), "cpu")
        host.update(pred.astype(np.float32), y.astype(np.float32), p)
        want = host.compute_metrics()
        ap = _average_precision(y, p)
        micro = _average_precision(y.reshape(-1, 1), p.reshape(-1, 1))[0]
        got = finish_from_counts(counts.reshape(c, 1, 2), y.sum(0), row_stats, n, ap, micro, 0, _names(c))[0]
        assert got == want
        assert want["per_class"]["tag_00000"]["support"] == 0 and want["per_class"]["tag_00001"]["support"] == n


def test_recount_model_counts_non_finite_and_negative_zero():
    p = np.array([[np.nan, -0.0, np.inf], [0.25, 0.0, -1.0]], dtype=np.float32)
    y = np.array([[1, 0, 1], [0, 1, 0]], dtype=bool)
    counts, row_stats = recount_model(encode_keys(p, y), [0.1, -0.5, 0.0])
    assert counts.tolist() == [[0, 1], [1, 1], [1, 0]]                   # NaN never passes; -0 reads as +0 > -0.5
    assert int(row_stats[2]) == 2


class _Dummy:
    def eval(self):
        return self


@pytest.mark.parametrize("per_class", [False, True])
def test_one_pass_on_the_host_matrix_writes_the_two_pass_files(per_class, monkeypatch, tmp_path, capsys):
    n, c = 120, 11
    p, y = _data(n, c, 5)
    calls = []
    monkeypatch.setattr(evaluation, "_probabilities", lambda *a, **k: (calls.append(1), (p, y.astype(np.float32)))[1])
    names = _names(c)
    two, one = tmp_path / "two", tmp_path / "one"
    opt2 = find_optimal_threshold(_Dummy(), _Dummy(), None, names, device="cpu", output_dir=str(two))
    m2 = evaluate_model(_Dummy(), _Dummy(), None, names, device="cpu", threshold=opt2["global_threshold"], output_dir=str(two))
    out2 = capsys.readouterr().out
    assert len(calls) == 2
    opt1, m1, pc1 = evaluate_and_search(_Dummy(), _Dummy(), None, names, device="cpu", output_dir=str(one), device_metrics=False,
                                        per_class=per_class)
    out1 = capsys.readouterr().out
    assert len(calls) == 3                                               # ONE pass
    assert opt1 == opt2 and m1 == m2
    for f in ("optimal_thresholds.json", "evaluation_results.csv", "evaluation_results_overall.json"):
        assert (one / f).read_bytes() == (two / f).read_bytes(), f
    assert sorted(os.listdir(two)) == ["evaluation_results.csv", "evaluation_results_overall.json", "optimal_thresholds.json"]
    extra = ["evaluation_results_per_class_thresholds.csv", "evaluation_results_per_class_thresholds_overall.json"]
    assert sorted(os.listdir(one)) == sorted(os.listdir(two) + (extra if per_class else []))
    if not per_class:
        assert pc1 is None and out1 == out2
        return
    assert out1.startswith(out2)
    vec = threshold_vector(opt1, names, 0.5)
    assert len(set(vec.tolist())) > 1                                    # the search did find different thresholds
    host = MultiLabelEvaluator(names, "cpu")
    host.update((p > vec[None, :]).astype(np.float32), y.astype(np.float32), p)
    assert pc1 == host.compute_metrics()
    assert json.loads((one / extra[1]).read_text()) == {k: v for k, v in pc1.items() if k != "per_class"}
    # the two-pass functions report the same per-class metrics from the evaluation pass (keyword, additive)
    m3, pc3 = evaluate_model(_Dummy(), _Dummy(), None, names, device="cpu", threshold=opt2["global_threshold"], per_class_thresholds=opt2)
    assert m3 == m2 and pc3 == pc1


def test_threshold_vector_forms():
    names = ["a", "b", "c"]
    opt = {"global_threshold": 0.3, "per_class_thresholds": {"a": {"threshold": 0.25, "f1_score": 1.0}, "c": {"threshold": 0.75, "f1_score": 0.5}}}
    assert threshold_vector(opt, names, 0.5).tolist() == [0.25, 0.5, 0.75]
    assert threshold_vector({"b": 0.125}, names, 0.5).tolist() == [0.5, 0.125, 0.5]
    assert threshold_vector(np.array([0.1, 0.2, 0.3]), names, 0.5).dtype == np.float64
    with pytest.raises(ValueError):
        threshold_vector(np.zeros(2), names, 0.5)


BASE = ["--vae_checkpoint", "v", "--decoder_checkpoint", "d", "--json_path", "j", "--tags_csv_path", "t"]


def test_single_pass_with_threshold_is_refused_before_any_gpu_work(monkeypatch):
    def never(*a, **k):
        raise AssertionError("reached GPU / process-group work")
    monkeypatch.setattr(infer_full, "_dist_setup", never)
    monkeypatch.setattr(infer_full, "load_models", never)
    monkeypatch.setattr(torch.cuda, "is_available", never)
    monkeypatch.setenv("WORLD_SIZE", "1")
    parser = evaluate.build_parser(distributed=True, recount=True)
    a = parser.parse_args(BASE)
    assert (a.single_pass, a.per_class_thresholds, a.threshold) == (False, False, None)
    with pytest.raises(RuntimeError, match="single_pass.*--threshold"):
        evaluate.evaluate(parser.parse_args(BASE + ["--single_pass", "--threshold", "0.4"]))
    with pytest.raises(RuntimeError, match="per_class_thresholds.*--threshold"):
        evaluate.evaluate(parser.parse_args(BASE + ["--per_class_thresholds", "--threshold", "0.4"]))
    evaluate.check_mode(parser.parse_args(BASE + ["--single_pass", "--per_class_thresholds"]), 1)
    # the flag sets earlier tests pin are unchanged; `main` parses with the extended ones
    flags = lambda p: {o for a in p._actions for o in a.option_strings}
    assert flags(parser) - flags(evaluate.build_parser(distributed=True)) == {"--single_pass", "--per_class_thresholds"}
    assert flags(infer_full.build_parser(per_class=True)) - flags(infer_full.build_parser()) == {"--thresholds_json"}


def test_thresholds_json_loading_falls_back_for_a_missing_tag(tmp_path):
    tags = ["t0", "t1", "t2", "t3"]
    f = tmp_path / "optimal_thresholds.json"
    f.write_text(json.dumps({"global_threshold": 0.35, "global_f1": 0.5,
                             "per_class_thresholds": {"t0": {"threshold": 0.15, "f1_score": 0.9}, "t2": {"threshold": 0.8, "f1_score": 0.1},
                                                      "unknown": {"threshold": 0.9, "f1_score": 0.0}}}))
    v = infer_full.load_class_thresholds(str(f), tags, 0.6)
    assert v.dtype == np.float32 and v.tolist() == [np.float32(0.15), np.float32(0.6), np.float32(0.8), np.float32(0.6)]
    (tmp_path / "bad.json").write_text(json.dumps({"global_threshold": 0.35}))
    with pytest.raises(ValueError, match="per_class_thresholds"):
        infer_full.load_class_thresholds(str(tmp_path / "bad.json"), tags, 0.5)
    a = infer_full.build_parser(per_class=True).parse_args(["--vae_checkpoint", "v", "--decoder_checkpoint", "d", "--image_path", "i",
                                                            "--tags_csv_path", "t", "--thresholds_json", str(f)])
    assert a.thresholds_json == str(f)


def test_per_class_summary_reference_lower_rank_passes_higher_does_not():
    conf = [0.9, 0.7, 0.6, 0.3, float("nan")]
    idx = [2, 0, 3, 1, 4]
    tags = [f"t{i}" for i in range(5)]
    thr = [0.8, 0.25, 0.5, 0.6, 0.0]                                     # t0 (0.7) fails its 0.8; t1 (0.3), ranked below it, passes its 0.25
    r = infer_full.summarize_per_class(conf, idx, tags, thr)
    assert r["predicted_tags"] == [{"tag": "t2", "confidence": 0.9}, {"tag": "t3", "confidence": 0.6}, {"tag": "t1", "confidence": 0.3}]
    assert r["total_tags_above_threshold"] == 3 and r["max_confidence"] == 0.9          # the NaN never passes, whatever its threshold
    assert list(r) == list(infer_full.summarize(conf[:4], idx[:4], tags, 0.5))
    # equal thresholds: the scalar summary
    assert infer_full.summarize_per_class(conf[:4], idx[:4], tags, [0.6] * 5) == infer_full.summarize(conf[:4], idx[:4], tags, 0.6)


def _header_params(header, name):
    m = re.search(r"\b(size_t|int)\s+%s\(([^;]*?)\);" % name, header, re.S)
    assert m, name
    body = re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S)
    return m.group(1), [a.strip() for a in body.split(",")]


def test_new_symbols_are_in_the_built_library_with_the_declared_signatures():
    header = open(os.path.join(ROOT, "include", "vae_tagger_hip.h")).read()
    lib = _lib.load()
    want = {"vt_eval_recount_workspace_bytes": ("size_t", ["int", "long long"]),
            "vt_eval_recount": ("int", ["vt_context*", "const void*", "size_t", "int", "int", "long long", "long long", "const double*",
                                        "uint32_t*", "size_t", "uint64_t*", "size_t", "void*", "size_t", "void*"]),
            "vt_summarize_confidence_per_class": ("int", ["vt_context*", "const float*", "const int64_t*", "int", "int", "const float*", "int",
                                                          "float*", "int32_t*", "float*", "void*"])}
    ctype = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t}
    for name, (res, params) in want.items():
        assert hasattr(lib, name), f"{name} is not exported by the built library"
        got_res, got = _header_params(header, name)
        assert got_res == res
        assert [re.sub(r"\s*\w+$", "", g).replace(" *", "*") for g in got] == params, name        # declared types, parameter names dropped
        pres, pargs = _lib.PROTOTYPES[name]
        assert pres is ctype[res] and len(pargs) == len(params)
        for t, a in zip(params, pargs):
            assert a is (ctype[t] if t in ctype else ctypes.c_void_p), (name, t)
    assert lib.vt_eval_recount_workspace_bytes(0, 10) == 0 and lib.vt_eval_recount_workspace_bytes(5, -1) == 0
    ws = lib.vt_eval_recount_workspace_bytes(10000, 8192)
    assert ws % 256 == 0 and ws >= 4 * 8192 + 8 * 10000 + 24
    assert "uses >" in header or "strict >" in header                    # the header says which comparison evaluation uses
