"""`evaluate --decoder_checkpoints A B C` end to end: three seeded synthetic decoders scored in ONE pass against three separate
`--single_pass` runs (every file byte for byte, at a fixed resolution and with --use_bucketing), validation_loss.json against the numpy
mirrors on the logits of the separate runs, checkpoint_sweep.json's ranking, one encode per batch, and the unchanged files of a run
without the new flags."""
import json
import os

import numpy as np
import pytest
import torch

from vae_tagger_amd import diffusers_vae_loader, evaluate, evaluation, losses, modules, synth
from vae_tagger_amd.evaluation import MultiLabelEvaluator

pytestmark = pytest.mark.gpu
N_TAGS = 40
SIZES = [(200, 150), (128, 128), (90, 160), (300, 300), (256, 128), (130, 250), (640, 480), (100, 100), (192, 256), (333, 222),
         (150, 200), (257, 255), (512, 256), (64, 128), (240, 180), (180, 240), (129, 127), (300, 150), (210, 140)]
FILES = ("optimal_thresholds.json", "evaluation_results.csv", "evaluation_results_overall.json")
PC_FILES = ("evaluation_results_per_class_thresholds.csv", "evaluation_results_per_class_thresholds_overall.json")
SEEDS = (1, 2, 3)
REL = 1e-9


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from PIL import Image
    from safetensors.torch import save_file
    root = tmp_path_factory.mktemp("sweep")
    g = torch.Generator().manual_seed(11)
    imgs = root / "imgs"
    imgs.mkdir()
    tags = [f"tag_{i:05d}" for i in range(N_TAGS)]
    data = {}
    for i, (w, h) in enumerate(SIZES):
        arr = (torch.rand(h, w, 3, generator=g) * 255).to(torch.uint8).numpy()
        arr[: h // 2, : w // 3] = 200
        Image.fromarray(arr).save(imgs / f"img{i:02d}.png")
        picks = [(3 * i + k) % N_TAGS for k in range(6 + i % 4)]        # every tag has a sample: finite class-balanced weights
        data[str(imgs / f"img{i:02d}.png")] = ", ".join(f"{tags[k]}:{0.5 + 0.5 * ((k + i) % 2)}" if k % 3 else tags[k] for k in picks)
        if i == 5:
            (imgs / "broken.png").write_bytes(b"not a png")
            data[str(imgs / "broken.png")] = f"{tags[0]}:1.0"
    (root / "data.json").write_text(json.dumps(data))
    (root / "tags.csv").write_text("name\n" + "\n".join(tags) + "\n")
    save_file(synth.synth_state_dict(synth.encoder_manifest(), seed=0), str(root / "vae.safetensors"))
    ckpts = []
    for s in SEEDS:
        ckpts.append(str(root / f"epoch_{s:02d}.pth"))
        torch.save(synth.synth_state_dict(synth.attention_decoder_manifest(N_TAGS), seed=s), ckpts[-1])
    common = ["--vae_checkpoint", str(root / "vae.safetensors"), "--json_path", str(root / "data.json"), "--tags_csv_path", str(root / "tags.csv"),
              "--resolution", "128", "--batch_size", "4"]
    all_labels = evaluate.TaggedImageList(str(root / "data.json"), str(root / "tags.csv"), check_files=False).labels
    assert len(all_labels) == len(SIZES) + 1
    weights = losses.class_balanced_weights(losses.class_distribution(all_labels))       # from the WHOLE JSON, the broken file's entry too
    assert np.isfinite(weights).all()
    return {"root": root, "tags": tags, "ckpts": ckpts, "common": common, "weights": weights}


def _separate_run(dataset, i, out, extra, monkeypatch):
    """One --single_pass run of checkpoint i, recording the logits its decoder returned and the labels its evaluator was fed."""
    fed_logits, fed_labels = [], []
    real_forward, real_update = modules._HipDecoder.forward, evaluation.DeviceMultiLabelEvaluator.update

    def forward(self, latent):
        out_ = real_forward(self, latent)
        fed_logits.append(out_.detach().float().cpu().numpy().copy())
        return out_

    def update(self, probabilities, targets):
        fed_labels.append(MultiLabelEvaluator._np(targets).copy())
        return real_update(self, probabilities, targets)
    monkeypatch.setattr(modules._HipDecoder, "forward", forward)
    monkeypatch.setattr(evaluation.DeviceMultiLabelEvaluator, "update", update)
    r = evaluate.main(dataset["common"] + ["--decoder_checkpoint", dataset["ckpts"][i], "--output_dir", str(out), "--single_pass"] + extra)
    monkeypatch.undo()
    assert len(fed_logits) == len(fed_labels)
    return r, fed_logits, fed_labels, [list(n) for n, _ in evaluate.LAST_RUN_STATS["batches"]]


def _mirror(dataset, logits, labels, alpha=1.0, gamma=2.0):
    h = losses.HostLossState(N_TAGS, alpha, gamma, dataset["weights"])
    for x, y in zip(logits, labels):
        h.update(x, y)
    return h.read()


def _close(got, want):
    if not np.isfinite(want):
        return got == want or (np.isnan(got) and np.isnan(want))
    return abs(got - want) <= REL * abs(want)


def _sweep(dataset, out, extra, monkeypatch):
    """The sweep over the three checkpoints with the encoder's calls counted."""
    calls = {"encode": 0}
    real_encode = diffusers_vae_loader.DiffusersVAEWrapper.encode

    def encode(self, *a, **k):
        calls["encode"] += 1
        return real_encode(self, *a, **k)
    monkeypatch.setattr(diffusers_vae_loader.DiffusersVAEWrapper, "encode", encode)
    r = evaluate.main(dataset["common"] + ["--decoder_checkpoint", dataset["ckpts"][0], "--decoder_checkpoints"] + dataset["ckpts"]
                      + ["--output_dir", str(out)] + extra)
    monkeypatch.undo()
    return r, calls["encode"]


@pytest.mark.parametrize("bucketing", [False, True], ids=["fixed", "bucketed"])
def test_sweep_equals_three_single_pass_runs_and_encodes_once(dataset, monkeypatch, bucketing):
    root = dataset["root"]
    tag = "b" if bucketing else "f"
    shape = ["--use_bucketing", "--base_resolution", "128", "--max_resolution", "256", "--bucket_step", "64"] if bucketing else []
    extra = shape + ["--per_class_thresholds"]
    singles = [_separate_run(dataset, i, root / f"single_{tag}_{i}", extra, monkeypatch) for i in range(3)]
    sweep, encodes = _sweep(dataset, root / f"sweep_{tag}", extra + ["--use_focal_loss", "--focal_alpha", "0.25"], monkeypatch)
    stats = dict(evaluate.LAST_RUN_STATS)
    assert stats["passes"] == 1 and stats["images"] == len(SIZES) and sweep["skipped"] == 1
    assert encodes == len(stats["batches"])                              # ONE encode per batch, not one per checkpoint
    assert len(singles[0][1]) == len(stats["batches"])
    out = root / f"sweep_{tag}"
    dirs = [f"ckpt_{i}_epoch_{s:02d}" for i, s in enumerate(SEEDS)]
    assert sorted(os.listdir(out)) == sorted(dirs + ["checkpoint_sweep.json"])
    summary = json.loads((out / "checkpoint_sweep.json").read_text())
    assert summary == json.loads(json.dumps(sweep["sweep"])) and summary["selected_loss"] == "focal"
    mirrors = []
    sweep_batches = [list(n) for n, _ in stats["batches"]]
    if not bucketing:                                                    # fixed resolution: the feeder keeps list order, every run sees the same batches
        assert all(b == sweep_batches for _, _, _, b in singles)
    for i, (single, logits, labels, batches) in enumerate(singles):
        d = out / dirs[i]
        assert sorted(os.listdir(d)) == sorted(FILES + PC_FILES + ("validation_loss.json",))
        for f in FILES + PC_FILES:                                       # exactly the files of the separate run
            assert (d / f).read_bytes() == (root / f"single_{tag}_{i}" / f).read_bytes(), (i, f)
        got = json.loads((d / "validation_loss.json").read_text())
        want = _mirror(dataset, logits, labels, 0.25, 2.0)
        mirrors.append(want)
        for name in losses.LOSS_NAMES:
            # (the mean of batch means is a function of the batching: compared when the separate run formed the sweep's batches)
            for key in ("mean_of_batch_means", "per_element") if batches == sweep_batches else ("per_element",):
                print(f"ckpt {i} {name} {key}: device {got[name][key]!r} mirror {want[name][key]!r}")
                assert _close(got[name][key], want[name][key]), (i, name, key)
        assert got["selected_loss"] == "focal" and got["val_loss"] == got["focal"]["mean_of_batch_means"]
        assert (got["steps"], got["elements"], got["non_finite"]) == (len(stats["batches"]), len(SIZES) * N_TAGS, 0)       # clean status
        assert (got["alpha"], got["gamma"]) == (0.25, 2.0) and "per_class" not in got
        row = summary["checkpoints"][i]
        assert row["path"] == dataset["ckpts"][i] and row["non_finite"] == 0 and row["val_loss"] == got["val_loss"]
        assert (row["global_threshold"], row["global_f1"]) == (single["optimal_thresholds"]["global_threshold"], single["optimal_thresholds"]["global_f1"])
        assert (row["f1_macro"], row["f1_micro"], row["mAP"]) == (single["metrics"]["f1_macro"], single["metrics"]["f1_micro"], single["metrics"]["mAP"])
        assert all(row[name] == got[name] for name in losses.LOSS_NAMES)
    focal = [m["focal"]["mean_of_batch_means"] for m in mirrors]
    assert len(set(focal)) == 3 and summary["best_by_val_loss"]["index"] == int(np.argmin(focal))
    f1 = [s[0]["metrics"]["f1_macro"] for s in singles]
    assert summary["best_by_macro_f1"]["index"] == f1.index(max(f1))
    assert summary["best_by_val_loss"]["path"] == dataset["ckpts"][summary["best_by_val_loss"]["index"]]


def test_val_loss_alone_adds_one_file_and_changes_no_other(dataset, monkeypatch):
    """Without the new flags the CLI writes its three files as before; --val_loss (two passes, one pass, fixed threshold) adds
    validation_loss.json and leaves the others byte for byte; a one-checkpoint --val_loss run reports the sweep's numbers."""
    root = dataset["root"]
    base = dataset["common"] + ["--decoder_checkpoint", dataset["ckpts"][0], "--use_bucketing", "--base_resolution", "128", "--max_resolution", "256",
                                "--bucket_step", "64"]
    plain = evaluate.main(base + ["--output_dir", str(root / "plain")])
    assert sorted(os.listdir(root / "plain")) == sorted(FILES) and evaluate.LAST_RUN_STATS["passes"] == 2
    assert "validation_loss" not in plain and "sweep" not in plain
    with_loss = evaluate.main(base + ["--output_dir", str(root / "plain_loss"), "--val_loss", "--use_class_balanced"])
    assert evaluate.LAST_RUN_STATS["passes"] == 2
    assert sorted(os.listdir(root / "plain_loss")) == sorted(FILES + ("validation_loss.json",))
    for f in FILES:
        assert (root / "plain_loss" / f).read_bytes() == (root / "plain" / f).read_bytes(), f
    assert with_loss["metrics"] == plain["metrics"] and with_loss["threshold"] == plain["threshold"]
    report = json.loads((root / "plain_loss" / "validation_loss.json").read_text())
    assert report["selected_loss"] == "class_balanced" and report["val_loss"] == report["class_balanced"]["mean_of_batch_means"] > 0
    # fixed threshold: evaluate_model's two files
    thr = evaluate.main(base + ["--output_dir", str(root / "thr"), "--threshold", "0.35"])
    thr_loss = evaluate.main(base + ["--output_dir", str(root / "thr_loss"), "--threshold", "0.35", "--val_loss"])
    assert sorted(os.listdir(root / "thr_loss")) == sorted(FILES[1:] + ("validation_loss.json",)) and thr_loss["metrics"] == thr["metrics"]
    for f in FILES[1:]:
        assert (root / "thr_loss" / f).read_bytes() == (root / "thr" / f).read_bytes(), f
    # one pass, fixed resolution: the loss of a lone --val_loss run is the loss the sweep reports for that checkpoint
    fixed = dataset["common"] + ["--decoder_checkpoint", dataset["ckpts"][1]]
    lone = evaluate.main(fixed + ["--output_dir", str(root / "lone"), "--single_pass", "--val_loss", "--use_focal_loss"])
    sweep, _ = _sweep(dataset, root / "sweep_lone", ["--use_focal_loss"], monkeypatch)
    assert (root / "lone" / "validation_loss.json").read_bytes() == (root / "sweep_lone" / "ckpt_1_epoch_02" / "validation_loss.json").read_bytes()
    assert lone["validation_loss"]["focal"] == sweep["checkpoints"][1]["loss"]["focal"]
    for f in FILES:
        assert (root / "lone" / f).read_bytes() == (root / "sweep_lone" / "ckpt_1_epoch_02" / f).read_bytes(), f
