"""`evaluate --single_pass` and `--per_class_thresholds` end to end: the one-pass run against the two-pass run of the same list (byte for
byte, at a fixed resolution: the feeder keeps list order there, so every pass sees batches of the same composition), the per-class
metrics against the host evaluator on the probabilities of the same run, and the sharded one-pass run (two ranks on one GPU, gloo)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from vae_tagger_amd import evaluate, evaluation, synth
from vae_tagger_amd.evaluation import MultiLabelEvaluator, threshold_vector

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_TAGS = 40
SIZES = [(200, 150), (128, 128), (90, 160), (300, 300), (256, 128), (130, 250), (640, 480), (100, 100), (192, 256), (333, 222),
         (150, 200), (257, 255), (512, 256), (64, 128), (240, 180), (180, 240), (129, 127), (300, 150), (210, 140)]
FILES = ("optimal_thresholds.json", "evaluation_results.csv", "evaluation_results_overall.json")
PC_FILES = ("evaluation_results_per_class_thresholds.csv", "evaluation_results_per_class_thresholds_overall.json")


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from PIL import Image
    from safetensors.torch import save_file
    root = tmp_path_factory.mktemp("single_pass")
    g = torch.Generator().manual_seed(11)
    imgs = root / "imgs"
    imgs.mkdir()
    tags = [f"tag_{i:05d}" for i in range(N_TAGS)]
    data = {}
    for i, (w, h) in enumerate(SIZES):
        arr = (torch.rand(h, w, 3, generator=g) * 255).to(torch.uint8).numpy()
        arr[: h // 2, : w // 3] = 200
        Image.fromarray(arr).save(imgs / f"img{i:02d}.png")
        picks = torch.randperm(N_TAGS, generator=g)[: 3 + i % 9].tolist()
        data[str(imgs / f"img{i:02d}.png")] = ", ".join(f"{tags[k]}:{0.5 + 0.5 * ((k + i) % 2)}" if k % 3 else tags[k] for k in picks)
        if i == 5:
            (imgs / "broken.png").write_bytes(b"not a png")
            data[str(imgs / "broken.png")] = f"{tags[0]}:1.0"
    (root / "data.json").write_text(json.dumps(data))
    (root / "tags.csv").write_text("name\n" + "\n".join(tags) + "\n")
    save_file(synth.synth_state_dict(synth.encoder_manifest(), seed=0), str(root / "vae.safetensors"))
    torch.save(synth.synth_state_dict(synth.attention_decoder_manifest(N_TAGS), seed=1), root / "dec.pth")
    return {"root": root, "tags": tags,
            "argv": ["--vae_checkpoint", str(root / "vae.safetensors"), "--decoder_checkpoint", str(root / "dec.pth"), "--json_path",
                     str(root / "data.json"), "--tags_csv_path", str(root / "tags.csv"), "--resolution", "128", "--batch_size", "4"]}


def _identical(a, b, files=FILES):
    for f in files:
        assert (a / f).read_bytes() == (b / f).read_bytes(), f


def test_single_pass_writes_the_two_pass_files_and_per_class_metrics_match_the_host(dataset, monkeypatch):
    root = dataset["root"]
    two = evaluate.main(dataset["argv"] + ["--output_dir", str(root / "two")])
    assert evaluate.LAST_RUN_STATS["passes"] == 2 and two["skipped"] == 1
    batches_two = list(evaluate.LAST_RUN_STATS["batches"])
    # record what the evaluator is fed during the one-pass run: the probabilities "dumped from the same run"
    fed = []
    real_update = evaluation.DeviceMultiLabelEvaluator.update

    def recording_update(self, probabilities, targets):
        fed.append((probabilities.detach().float().cpu().numpy().copy(), MultiLabelEvaluator._np(targets).copy()))
        return real_update(self, probabilities, targets)
    monkeypatch.setattr(evaluation.DeviceMultiLabelEvaluator, "update", recording_update)
    one = evaluate.main(dataset["argv"] + ["--output_dir", str(root / "one"), "--single_pass", "--per_class_thresholds"])
    monkeypatch.undo()
    assert evaluate.LAST_RUN_STATS["passes"] == 1 and evaluate.LAST_RUN_STATS["images"] == len(SIZES)
    # batch composition: the second pass of the two-pass run and the one pass saw the same batches (fixed resolution: list order)
    assert [n for n, _ in evaluate.LAST_RUN_STATS["batches"]] == [n for n, _ in batches_two]
    _identical(root / "one", root / "two")
    assert one["threshold"] == two["threshold"] and one["optimal_thresholds"] == two["optimal_thresholds"] and one["metrics"] == two["metrics"]
    assert "per_class_metrics" not in two and sorted(os.listdir(root / "two")) == sorted(FILES)
    assert sorted(os.listdir(root / "one")) == sorted(FILES + PC_FILES)
    # the per-class metrics against the host evaluator on the recorded probabilities
    p, y = np.vstack([a for a, _ in fed]), np.vstack([b for _, b in fed])
    assert p.shape == (len(SIZES), N_TAGS) and p.dtype == np.float32
    vec = threshold_vector(one["optimal_thresholds"], dataset["tags"], one["threshold"])
    host = MultiLabelEvaluator(dataset["tags"], "cpu")
    host.update((p > vec[None, :]).astype(np.float32), y, p)
    want, got = host.compute_metrics(), one["per_class_metrics"]
    for k, v in want.items():
        if k in ("mAP", "mAP_micro", "mAP_weighted"):
            assert abs(got[k] - v) <= 1e-9, k
        elif k != "per_class":
            assert got[k] == v, (k, got[k], v)
    for name, w in want["per_class"].items():
        g = got["per_class"][name]
        assert (g["precision"], g["recall"], g["f1"], g["support"]) == (w["precision"], w["recall"], w["f1"], w["support"]), name
        assert abs(g["ap"] - w["ap"]) <= 1e-9, name
    assert json.loads((root / "one" / PC_FILES[1]).read_text()) == {k: v for k, v in got.items() if k != "per_class"}
    # without --single_pass the per-class metrics come from the second pass's key store: the same files
    both = evaluate.main(dataset["argv"] + ["--output_dir", str(root / "two_pc"), "--per_class_thresholds"])
    assert evaluate.LAST_RUN_STATS["passes"] == 2
    _identical(root / "two_pc", root / "one", FILES + PC_FILES)
    assert both["per_class_metrics"] == got
    # the host evaluator's route writes the same count-derived files in one pass too
    host_one = evaluate.main(dataset["argv"] + ["--output_dir", str(root / "host_one"), "--single_pass", "--per_class_thresholds", "--host_metrics"])
    assert evaluate.LAST_RUN_STATS["passes"] == 1 and host_one["optimal_thresholds"] == one["optimal_thresholds"]
    assert (root / "host_one" / "optimal_thresholds.json").read_bytes() == (root / "one" / "optimal_thresholds.json").read_bytes()
    for k in ("accuracy", "hamming_loss", "f1_micro", "f1_macro", "precision_weighted", "recall_micro"):
        assert host_one["metrics"][k] == one["metrics"][k] and host_one["per_class_metrics"][k] == got[k], k


def test_sharded_single_pass_two_ranks_write_the_one_process_files(dataset):
    """Two ranks share GPU 0 (gloo), as the existing sharded tests rehearse: the keys travel in the merge and rank 0 recounts.  The
    ranks' batches differ from the one-process run's: count-derived fields are compared exactly on the strength of the batch-composition
    invariance those tests rest on, AP fields within 1e-9."""
    root = dataset["root"]
    one = evaluate.main(dataset["argv"] + ["--output_dir", str(root / "one_sp"), "--single_pass", "--per_class_thresholds"])
    env = dict(os.environ, VT_CLI_GLOO="1", PYTHONDONTWRITEBYTECODE="1", HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
           str(29500 + os.getpid() % 200), "-m", "vae_tagger_amd.evaluate"] + dataset["argv"] + \
          ["--output_dir", str(root / "two_sp"), "--single_pass", "--per_class_thresholds", "--sharded"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=420)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    out = r.stdout.decode()
    assert out.count("评估完成") == 1 and f"图像: {len(SIZES)}, 跳过: 1," in out
    assert sorted(os.listdir(root / "two_sp")) == sorted(os.listdir(root / "one_sp"))
    assert (root / "two_sp" / FILES[0]).read_bytes() == (root / "one_sp" / FILES[0]).read_bytes()
    assert json.loads((root / "two_sp" / FILES[0]).read_text())["global_threshold"] == one["threshold"]
    for overall in (FILES[2], PC_FILES[1]):
        g, w = json.loads((root / "two_sp" / overall).read_text()), json.loads((root / "one_sp" / overall).read_text())
        assert list(g) == list(w)
        for k in w:
            assert (abs(g[k] - w[k]) <= 1e-9) if k.startswith("mAP") else (g[k] == w[k]), (overall, k, g[k], w[k])
    for csv in (FILES[1], PC_FILES[0]):
        gl, wl = (root / "two_sp" / csv).read_text().strip().split("\n"), (root / "one_sp" / csv).read_text().strip().split("\n")
        assert len(gl) == len(wl) == N_TAGS + 1 and gl[0] == wl[0]
        for a, b in zip(gl[1:], wl[1:]):
            a, b = a.split(","), b.split(",")
            assert a[:4] == b[:4] and a[5] == b[5] and abs(float(a[4]) - float(b[4])) <= 1e-9, (csv, a, b)
