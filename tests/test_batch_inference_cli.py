"""`python -m vae_tagger_amd.batch_inference_test` end to end on synthetic weights: the reference's JSON shape, pred_tags against what
infer_full writes for the same images and threshold, the device route against --host_metrics byte for byte, --thresholds_json with all
thresholds equal against the global-threshold run, and --search.  (The ground-truth matching, the set semantics and unknown tags are
tested on the host in test_sample_metrics_host.py.)"""
import json

import numpy as np
import pytest
import torch

from vae_tagger_amd import batch_inference_test as bit, infer_full, sample_metrics as sm, synth

pytestmark = pytest.mark.gpu
N_TAGS, RES, THR = 11, 64, 0.5
SIZES = [(80, 64), (64, 64), (50, 90), (120, 70), (64, 100), (77, 77)]


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from PIL import Image
    from safetensors.torch import save_file
    root = tmp_path_factory.mktemp("batch_test")
    g = torch.Generator().manual_seed(23)
    imgs = root / "imgs"
    imgs.mkdir()
    tags = [f"tag_{i:02d}" for i in range(N_TAGS)]
    data = {}
    for i, (w, h) in enumerate(SIZES):
        arr = (torch.rand(h, w, 3, generator=g) * 255).to(torch.uint8).numpy()
        arr[: h // 2, : w // 3] = 30 * i
        name = f"img{5 - i}.jpg"                              # written in reverse: the run sorts by name
        Image.fromarray(arr).save(imgs / name, quality=95)
        picks = [tags[k] for k in torch.randperm(N_TAGS, generator=g)[: i % 4].tolist()]
        if i == 2:
            picks += ["not_in_the_list", picks[0]]           # an unknown tag and a duplicate
        data[f"somewhere/else/{name}"] = ", ".join(f"{t}:{0.5 * (k % 3)}" if k % 2 else t for k, t in enumerate(picks))
    Image.fromarray(np.zeros((64, 64, 3), dtype=np.uint8)).save(imgs / "img9_no_truth.jpg")
    (root / "data.json").write_text(json.dumps(data))
    (root / "tags.csv").write_text("name\n" + "\n".join(tags) + "\n")
    save_file(synth.synth_state_dict(synth.encoder_manifest(), seed=0), str(root / "vae.safetensors"))
    torch.save(synth.synth_state_dict(synth.attention_decoder_manifest(N_TAGS), seed=1), root / "dec.pth")
    models = ["--vae_checkpoint", str(root / "vae.safetensors"), "--decoder_checkpoint", str(root / "dec.pth"),
              "--tags_csv_path", str(root / "tags.csv"), "--resolution", str(RES), "--confidence_threshold", str(THR), "--batch_size", "1"]
    argv = models + ["--image_dir", str(imgs), "--data_json_path", str(root / "data.json"), "--max_images", "10"]
    base = bit.main(argv + ["--output_dir", str(root / "base")])
    return {"root": root, "tags": tags, "data": data, "imgs": imgs, "models": models, "argv": argv, "base": base}


def test_json_shape_and_pred_tags_of_infer_full(dataset, capsys):
    root, base = dataset["root"], dataset["base"]["metrics"]
    written = json.loads((root / "base" / "batch_test_results.json").read_text())
    assert written == base
    assert list(written) == ["avg_precision", "avg_recall", "avg_f1", "exact_match_rate", "total_images", "detailed_results"]
    assert written["total_images"] == 6 and [r["image"] for r in written["detailed_results"]] == [f"img{i}.jpg" for i in range(6)]
    for r in written["detailed_results"]:
        assert list(r) == ["image", "true_tags", "pred_tags", "precision", "recall", "f1", "exact_match"]
    full = infer_full.main(dataset["models"] + ["--image_path", str(dataset["imgs"]), "--output_dir", str(root / "full")])
    by_name = {p.replace("\\", "/").rsplit("/", 1)[-1]: e for p, e in full.items()}
    truth = bit.load_ground_truth(str(root / "data.json"))
    index = {t: k for k, t in enumerate(dataset["tags"])}
    for r in written["detailed_results"]:
        assert r["pred_tags"] == [e["tag"] for e in by_name[r["image"]]["predicted_tags"]], r["image"]
        # the reference's arithmetic on the two tag lists
        true_set, pred_set = set(r["true_tags"]), set(r["pred_tags"])
        assert r["true_tags"] == bit.match_ground_truth(r["image"], truth)
        inter = len(true_set & pred_set)
        precision = inter / len(pred_set) if pred_set else 0
        recall = inter / len(true_set) if true_set else 1
        f1 = 2 * precision * recall / (precision + recall) if precision + recall > 0 else 0
        assert (r["precision"], r["recall"], r["f1"], r["exact_match"]) == (precision, recall, f1, 1 if true_set == pred_set else 0)
        assert bit.label_row(r["true_tags"], index)[1] == len(true_set - set(dataset["tags"]))
    n = 6
    assert written["avg_precision"] == sum(r["precision"] for r in written["detailed_results"]) / n
    assert written["avg_f1"] == sum(r["f1"] for r in written["detailed_results"]) / n
    assert any("not_in_the_list" in r["true_tags"] for r in written["detailed_results"])


def test_device_and_host_files_are_identical_and_equal_thresholds_json_gives_the_global_file(dataset):
    root = dataset["root"]
    want = (root / "base" / "batch_test_results.json").read_bytes()
    bit.main(dataset["argv"] + ["--output_dir", str(root / "host"), "--host_metrics"])
    assert (root / "host" / "batch_test_results.json").read_bytes() == want
    (root / "thr.json").write_text(json.dumps({"global_threshold": THR, "per_class_thresholds": {t: THR for t in dataset["tags"][:7]}}))
    bit.main(dataset["argv"] + ["--output_dir", str(root / "pc"), "--thresholds_json", str(root / "thr.json")])
    assert (root / "pc" / "batch_test_results.json").read_bytes() == want
    bit.main(dataset["argv"] + ["--output_dir", str(root / "pc_host"), "--thresholds_json", str(root / "thr.json"), "--host_metrics"])
    assert (root / "pc_host" / "batch_test_results.json").read_bytes() == want


def test_search_reports_the_best_threshold_of_the_same_pass(dataset, capsys):
    root = dataset["root"]
    out = bit.main(dataset["argv"] + ["--output_dir", str(root / "search"), "--search"])
    printed = capsys.readouterr().out
    assert "img9_no_truth.jpg 的真实标签" in printed and "平均F1分数" in printed
    assert (root / "search" / "batch_test_results.json").read_bytes() == (root / "base" / "batch_test_results.json").read_bytes()
    search = json.loads((root / "search" / "threshold_search.json").read_text())
    assert search == out["search"] and [t["threshold"] for t in search["thresholds"]] == [float(t) for t in sm.SEARCH_GRID]
    f1 = [t["avg_f1"] for t in search["thresholds"]]
    assert search["best_index"] == f1.index(max(f1)) and search["best_threshold"] == search["thresholds"][search["best_index"]]["threshold"]
    at_half = search["thresholds"][9]
    assert at_half["threshold"] == 0.5 and at_half["avg_f1"] == dataset["base"]["metrics"]["avg_f1"]
    host = bit.main(dataset["argv"] + ["--output_dir", str(root / "search_host"), "--search", "--host_metrics"])
    assert host["search"] == out["search"]
