"""`python -m vae_tagger_amd.train_decoder` end to end on a small synthetic set: the files the reference writes, the feature cache
(no encoder batch after epoch 1), the recorded best validation loss against `evaluate --val_loss` on the saved checkpoint, and an
attention decoder trained with --freeze_front (only classifier.* moves)."""
import json
import os

import pytest
import torch

from vae_tagger_amd import evaluate, synth, train_decoder
from vae_tagger_amd.train import split_indices

pytestmark = pytest.mark.gpu
N_TAGS = 20
SIZES = [(96, 64), (64, 64), (80, 120), (128, 128), (100, 70), (64, 96), (90, 90), (120, 80), (70, 100), (64, 80), (110, 110), (72, 64)]
EVAL_FILES = ("optimal_thresholds.json", "evaluation_results.csv", "evaluation_results_overall.json")


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from PIL import Image
    from safetensors.torch import save_file
    root = tmp_path_factory.mktemp("train_cli")
    g = torch.Generator().manual_seed(5)
    (root / "imgs").mkdir()
    tags = [f"tag_{i:03d}" for i in range(N_TAGS)]
    data = {}
    for i, (w, h) in enumerate(SIZES):
        arr = (torch.rand(h, w, 3, generator=g) * 255).to(torch.uint8).numpy()
        arr[: h // 2, : w // 3] = 40 + 15 * i
        path = str(root / "imgs" / f"img{i:02d}.png")
        Image.fromarray(arr).save(path)
        picks = [(3 * i + k) % N_TAGS for k in range(4 + i % 3)]
        data[path] = ", ".join(f"{tags[k]}:{0.5 + 0.5 * ((k + i) % 2)}" if k % 3 else tags[k] for k in picks)
    (root / "data.json").write_text(json.dumps(data))
    (root / "tags.csv").write_text("name\n" + "\n".join(tags) + "\n")
    save_file(synth.synth_state_dict(synth.encoder_manifest(), seed=0), str(root / "vae.safetensors"))
    common = ["--vae_checkpoint", str(root / "vae.safetensors"), "--tags_csv_path", str(root / "tags.csv"), "--resolution", "64"]
    return {"root": root, "data": data, "common": common, "json": str(root / "data.json")}


def test_plain_decoder_trains_from_the_cache_and_its_best_checkpoint_reproduces_its_val_loss(dataset):
    root, out = dataset["root"], dataset["root"] / "plain"
    r = train_decoder.main(dataset["common"] + ["--json_path", dataset["json"], "--output_dir", str(out), "--no_attention", "--num_epochs", "2",
                                                "--train_batch_size", "4", "--save_steps", "1", "--lr_warmup_steps", "2", "--mixed_precision", "fp16"])
    for f in ("best_pytorch_model.bin", "pytorch_model.bin", "training_history.json", "train_report.json") + EVAL_FILES:
        assert os.path.isfile(out / f), f
    history = json.loads((out / "training_history.json").read_text())
    assert sorted(history) == ["learning_rates", "train_loss", "val_loss"] and all(len(v) == 2 for v in history.values())
    report = json.loads((out / "train_report.json").read_text())
    assert [e["encoder_batches"] for e in report["epochs"]] == [4, 0] and report["epochs"][1]["steps"] == 3
    assert report["feature_cache_bytes"] == len(SIZES) * (256 + N_TAGS) * 4
    # the best checkpoint, scored by the existing evaluate --val_loss path over the validation images (same batching: one batch)
    from vae_tagger_amd.modules import ClassificationDecoder
    best = torch.load(out / "best_pytorch_model.bin", map_location="cpu")
    dec = ClassificationDecoder(16, 8, 8, N_TAGS)
    assert set(best) == set(dec.state_dict())
    dec.load_state_dict(best)
    paths = list(dataset["data"])
    _, val_idx = split_indices(len(paths), 42)
    (root / "val.json").write_text(json.dumps({paths[i]: dataset["data"][paths[i]] for i in val_idx}))
    evaluate.main(dataset["common"] + ["--json_path", str(root / "val.json"), "--decoder_checkpoint", str(out / "best_pytorch_model.bin"),
                                       "--no_attention", "--batch_size", "4", "--output_dir", str(root / "val_eval"), "--single_pass", "--val_loss"])
    scored = json.loads((root / "val_eval" / "validation_loss.json").read_text())["val_loss"]
    print(f"recorded best val_loss {min(history['val_loss'])!r}, evaluate --val_loss {scored!r}")
    assert scored == min(history["val_loss"]) == r["best_val_loss"]          # exact: the same single batch


def test_attention_decoder_needs_freeze_front_and_keeps_its_front(dataset):
    root, out = dataset["root"], dataset["root"] / "attn"
    start = synth.synth_state_dict(synth.attention_decoder_manifest(N_TAGS), seed=3)
    torch.save(start, root / "start.pth")
    args = dataset["common"] + ["--json_path", dataset["json"], "--output_dir", str(out), "--decoder_checkpoint", str(root / "start.pth"),
                                "--num_epochs", "1", "--train_batch_size", "4", "--save_steps", "1", "--lr_warmup_steps", "0"]
    with pytest.raises(SystemExit, match="not implemented"):
        train_decoder.main(args)
    assert not os.path.exists(out)
    train_decoder.main(args + ["--freeze_front"])
    saved = torch.load(out / "pytorch_model.bin", map_location="cpu")
    assert set(saved) == set(start)
    for k, v in start.items():
        if not k.startswith("classifier."):
            assert torch.equal(saved[k], v), k
    assert not torch.equal(saved["classifier.12.weight"], start["classifier.12.weight"])
