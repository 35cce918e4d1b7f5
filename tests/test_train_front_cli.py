"""`python -m vae_tagger_amd.train_decoder --train_front` end to end on the synthetic set of test_train_cli.py: the attention decoder
trained in full (front tensors, running statistics and num_batches_tracked move), the latent cache (no encoder batch in epoch 2 when it
fits, re-encoding under --latent_cache_gb 0), and `evaluate --val_loss` on the saved best checkpoint against the recorded best loss."""
import json
import os

import pytest
import torch

from vae_tagger_amd import evaluate, synth, train_decoder
from vae_tagger_amd.train import FRONT_PREFIXES, split_indices

from test_train_cli import EVAL_FILES, N_TAGS, SIZES, dataset      # noqa: F401  (the module-scoped fixture builds the set once per module)

pytestmark = pytest.mark.gpu
NBT = "feature_compress.1.num_batches_tracked"


def run(dataset, out, *extra):
    start = dataset["root"] / "front_start.pth"
    if not os.path.exists(start):
        torch.save(synth.synth_state_dict(synth.attention_decoder_manifest(N_TAGS), seed=3), start)
    args = dataset["common"] + ["--json_path", dataset["json"], "--output_dir", str(out), "--decoder_checkpoint", str(start), "--num_epochs", "2",
                                "--train_batch_size", "4", "--save_steps", "1", "--lr_warmup_steps", "0", "--train_front"]
    return train_decoder.main(args + list(extra)), torch.load(start, map_location="cpu")


def test_train_front_trains_the_whole_decoder_from_the_latent_cache(dataset):
    root, out = dataset["root"], dataset["root"] / "full"
    r, start = run(dataset, out)
    for f in ("best_pytorch_model.bin", "pytorch_model.bin", "training_history.json", "train_report.json") + EVAL_FILES:
        assert os.path.isfile(out / f), f
    report = json.loads((out / "train_report.json").read_text())
    epochs = report["epochs"]
    n_train = len(SIZES) - 1                                  # 12 images: 1 for validation
    assert [e["encoder_batches"] for e in epochs] == [4, 0] and report["feature_cache_bytes"] == 0
    cache = report["latent_cache"]
    assert cache["cached"] and cache["bytes_used"] == len(SIZES) * (16 * 8 * 8 + N_TAGS) * 4 <= cache["bytes_needed"] <= cache["budget_bytes"]
    saved = torch.load(out / "pytorch_model.bin", map_location="cpu")
    assert set(saved) == set(start)
    for k, v in start.items():
        if k.startswith(FRONT_PREFIXES) and k != "self_attention_post.k_proj.bias":      # (its gradient is zero: softmax ignores it)
            assert not torch.equal(saved[k], v), k
    assert not torch.equal(saved["classifier.12.weight"], start["classifier.12.weight"])
    assert int(saved[NBT]) == int(start[NBT]) + sum(e["steps"] for e in epochs) and epochs[0]["steps"] == (n_train + 3) // 4
    assert saved[NBT].dtype == torch.int64 and all(torch.isfinite(v.float()).all() for v in saved.values())
    # the best checkpoint, scored by evaluate --val_loss over the validation image.  The checkpoint is loaded by a fresh decoder, which
    # folds the running statistics on the host in fp32 as the trainer does on the device (same formula, correctly rounded operations).
    history = json.loads((out / "training_history.json").read_text())
    paths = list(dataset["data"])
    _, val_idx = split_indices(len(paths), 42)
    (root / "val_front.json").write_text(json.dumps({paths[i]: dataset["data"][paths[i]] for i in val_idx}))
    evaluate.main(dataset["common"] + ["--json_path", str(root / "val_front.json"), "--decoder_checkpoint", str(out / "best_pytorch_model.bin"),
                                       "--batch_size", "4", "--output_dir", str(root / "val_front_eval"), "--single_pass", "--val_loss"])
    scored = json.loads((root / "val_front_eval" / "validation_loss.json").read_text())["val_loss"]
    print(f"recorded best val_loss {min(history['val_loss'])!r}, evaluate --val_loss {scored!r}")
    assert min(history["val_loss"]) == r["best_val_loss"]
    assert scored == r["best_val_loss"]


def test_latent_cache_gb_zero_re_encodes_every_epoch(dataset):
    out = dataset["root"] / "full_nocache"
    run(dataset, out, "--latent_cache_gb", "0")
    report = json.loads((out / "train_report.json").read_text())
    assert [e["encoder_batches"] for e in report["epochs"]] == [4, 4]
    assert report["latent_cache"] == {"cached": False, "budget_bytes": 0, "bytes_needed": report["latent_cache"]["bytes_needed"], "bytes_used": 0}
