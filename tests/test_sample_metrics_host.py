"""Host side of the per-image metrics: sample_metrics_host against what the reference's calculate_metrics made of the committed inputs
(tests/golden/batch_test_reference.json, written by tools/make_batch_test_fixture.py), both rules on a confidence equal to the
threshold, the true_extra effect, the CLI's ground-truth handling, and the header against the bindings.  No GPU."""
import json
import os
import re

import numpy as np

from vae_tagger_amd import _lib, batch_inference_test as bit, sample_metrics as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fixture():
    with open(os.path.join(ROOT, "tests", "golden", "batch_test_reference.json"), encoding="utf-8") as fh:
        d = json.load(fh)
    tags = d["tags"]
    index = {t: k for k, t in enumerate(tags)}
    probs = np.asarray([im["confidences"] for im in d["images"]], dtype=np.float32)
    labels = np.zeros(probs.shape, dtype=np.uint8)
    extra = np.zeros(len(d["images"]), dtype=np.uint32)
    for i, im in enumerate(d["images"]):
        labels[i], extra[i] = bit.label_row(im["true_tags"], index)
    return d, probs, labels, extra


def test_fixture_covers_the_edge_cases():
    d, probs, labels, extra = _fixture()
    assert probs.shape == (40, 11) and np.array_equal(probs.astype(np.float64), np.asarray([im["confidences"] for im in d["images"]]))
    ref = d["reference"]["detailed_results"]
    assert any(not r["true_tags"] for r in ref) and any(not r["pred_tags"] for r in ref) and extra.any()
    assert any(len(r["true_tags"]) != len(set(r["true_tags"])) for r in ref) and any(r["exact_match"] for r in ref)
    assert (probs == np.float32(d["threshold"])).any()


def test_host_reproduces_every_field_of_the_reference():
    d, probs, labels, extra = _fixture()
    ref = d["reference"]
    got = sm.sample_metrics_host(probs, labels, [d["threshold"]], d["rule"], extra)[0]
    # the averages are the reference's own sequence of operations: an in-order sum divided by the count
    for k in ("avg_precision", "avg_recall", "avg_f1", "exact_match_rate", "total_images"):
        assert got[k] == ref[k], (k, got[k], ref[k])
    true, rows = sm.sample_tallies_host(probs, labels, [d["threshold"]], d["rule"], extra)
    P, R, F, exact = sm.per_image_values(rows[:, 0, 0], rows[:, 0, 1], true)
    order = np.argsort(-probs, axis=1, kind="stable")
    for i, r in enumerate(ref["detailed_results"]):
        assert r["image"] == d["images"][i]["image"]
        assert (P[i], R[i], F[i], int(exact[i])) == (r["precision"], r["recall"], r["f1"], r["exact_match"]), (i, r)
        assert [d["tags"][k] for k in order[i, :rows[i, 0, 1]]] == r["pred_tags"]
        assert true[i] == len(set(r["true_tags"])) and rows[i, 0, 1] == len(r["pred_tags"])
        assert rows[i, 0, 0] == len(set(r["true_tags"]) & set(r["pred_tags"]))
    assert got["samples_recall_sklearn"] == (got["sum_recall"] - got["images_without_true_tag"]) / 40
    assert got["images_without_true_tag"] == sum(1 for r in ref["detailed_results"] if not r["true_tags"])


def test_both_rules_on_a_confidence_equal_to_the_threshold():
    p = np.asarray([[0.5, 0.25, 0.75], [0.5, 0.5, np.nan]], dtype=np.float32)
    y = np.asarray([[1, 0, 1], [0, 1, 1]], dtype=np.uint8)
    t_gt, r_gt = sm.sample_tallies_host(p, y, [0.5], "gt")
    t_ge, r_ge = sm.sample_tallies_host(p, y, [0.5], "ge")
    assert t_gt.tolist() == t_ge.tolist() == [2, 2]
    assert r_gt[:, 0].tolist() == [[1, 1], [0, 0]] and r_ge[:, 0].tolist() == [[2, 2], [1, 2]]      # NaN predicts under neither
    ge = sm.sample_metrics_host(p, y, [0.5], "ge")[0]
    assert ge["avg_precision"] == (1.0 + 0.5) / 2 and ge["avg_recall"] == (1.0 + 0.5) / 2 and ge["exact_match_rate"] == 0.5
    assert ge["nonfinite_probabilities"] == 1
    gt = sm.sample_metrics_host(p, y, [0.5], "gt")[0]
    assert gt["images_without_prediction"] == 1 and gt["avg_precision"] == 0.5 and gt["avg_f1"] == (2 * 1.0 * 0.5 / 1.5) / 2
    # the threshold is compared in fp64: fp32(0.7) < 0.7 does not pass at 0.7 under either rule
    assert sm.sample_tallies_host(np.asarray([[0.7]], dtype=np.float32), [[1]], [0.7], "ge")[1][0, 0, 1] == 0


def test_true_extra_lowers_recall_and_rules_out_an_exact_match():
    p = np.asarray([[0.9, 0.1], [0.1, 0.1]], dtype=np.float32)
    y = np.asarray([[1, 0], [0, 0]], dtype=np.uint8)
    a = sm.sample_metrics_host(p, y, [0.5], "ge")[0]
    assert (a["avg_recall"], a["exact_match_rate"], a["images_without_true_tag"]) == (1.0, 1.0, 1)      # (no prediction, no true tag: a match)
    b = sm.sample_metrics_host(p, y, [0.5], "ge", true_extra=[1, 2])[0]
    assert (b["avg_recall"], b["exact_match_rate"], b["images_without_true_tag"]) == (0.25, 0.0, 0) and b["avg_precision"] == 0.5
    res = sm.sample_metrics_host(p, y, [0.05, 0.5, 0.95], "gt")
    assert sm.best_threshold(res) == 1 and sm.best_threshold([{"avg_f1": 0.5}, {"avg_f1": 0.5}]) == 0


def test_ground_truth_matching_set_semantics_and_unknown_tags(tmp_path):
    data = {"a/b/img1.jpg": "cat:0.5, dog, cat:1.0, zebra:0.0", "other/img1.jpg": "dog", "c\\img2.jpg": "bird:2", "x/img3.jpg": "unknown_only"}
    (tmp_path / "data.json").write_text(json.dumps(data))
    gt = bit.load_ground_truth(str(tmp_path / "data.json"))
    assert gt["a/b/img1.jpg"] == ["cat", "dog", "cat", "zebra"]
    assert bit.match_ground_truth("/elsewhere/img1.jpg", gt) == ["cat", "dog", "cat", "zebra"]          # the FIRST entry of that basename
    assert bit.match_ground_truth("img9.jpg", gt) is None
    index = {"cat": 0, "dog": 1, "bird": 2}
    row, extra = bit.label_row(gt["a/b/img1.jpg"], index)
    assert row.dtype == np.uint8 and row.tolist() == [1, 1, 0] and extra == 1          # weights ignored (zebra:0.0 counts), the duplicate once
    assert bit.label_row(["unknown_only"], index)[1] == 1 and bit.label_row([], index)[0].tolist() == [0, 0, 0]
    for k, name in enumerate(("b.jpg", "a.jpg", "c.JPG", "d.png", "0.jpg")):
        (tmp_path / name).write_bytes(b"x")
    assert [os.path.basename(p) for p in bit.list_images(str(tmp_path), 2)] == ["0.jpg", "a.jpg"]


def test_header_declares_every_sample_symbol_the_bindings_name():
    with open(os.path.join(ROOT, "include", "vae_tagger_hip.h"), encoding="utf-8") as fh:
        header = fh.read()
    names = [n for n in _lib.PROTOTYPES if n.startswith("vt_sample_")]
    assert sorted(names) == ["vt_sample_finish", "vt_sample_finish_bytes", "vt_sample_from_keys", "vt_sample_read_rows", "vt_sample_reset",
                             "vt_sample_state_bytes", "vt_sample_update"]
    for n in names:
        m = re.search(r"\b(int|size_t)\s+" + n + r"\s*\(([^;]*)\)\s*;", header)
        assert m, n
        args = [a for a in re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S).split(",") if a.strip()]
        assert len(args) == len(_lib.PROTOTYPES[n][1]), (n, len(args), len(_lib.PROTOTYPES[n][1]))
    assert "VT_SAMPLE_GT = 0" in header and "VT_SAMPLE_GE = 1" in header and (_lib.VT_SAMPLE_GT, _lib.VT_SAMPLE_GE) == (0, 1)
    lib = _lib.load()
    for T, cap in ((1, 1), (32, 51), (19, 8192)):
        assert lib.vt_sample_state_bytes(T, cap) == sm.sample_layout(T, cap)["total"]
    assert lib.vt_sample_state_bytes(33, 8) == 0 and lib.vt_sample_state_bytes(1, 0) == 0 and lib.vt_sample_state_bytes(1, 1 << 31) == 0
    assert lib.vt_sample_finish_bytes(19) == 19 * 40 + 16 and lib.vt_sample_finish_bytes(33) == 0
