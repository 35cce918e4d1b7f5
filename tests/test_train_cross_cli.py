"""`python -m vae_tagger_amd.train_decoder --train_front --use_cross_attention --train_cross_attention` end to end on the synthetic set of
test_train_cli.py: the attention decoder with cross-attention trained in full (cross, front and head tensors move), epoch 2 from the
latent cache, and `evaluate --val_loss --use_cross_attention` on the saved best checkpoint against the recorded best loss."""
import json
import os

import pytest
import torch

from vae_tagger_amd import evaluate, synth, train_decoder
from vae_tagger_amd.train import CROSS_PREFIXES, FRONT_PREFIXES, split_indices

from test_train_cli import EVAL_FILES, N_TAGS, SIZES, dataset      # noqa: F401  (the module-scoped fixture builds the set once per module)

pytestmark = pytest.mark.gpu
NBT = "feature_compress.1.num_batches_tracked"
# zero in exact arithmetic (softmax ignores a shift of every score): nothing but the weight decay moves these
ZERO = ("self_attention_post.k_proj.bias", "cross_attention.k_proj.bias")


def test_train_cross_attention_trains_the_whole_decoder_from_the_latent_cache(dataset):
    root, out = dataset["root"], dataset["root"] / "cross"
    start_path = root / "cross_start.pth"
    torch.save(synth.synth_state_dict(synth.attention_decoder_manifest(N_TAGS, 16, True, True, True), seed=3), start_path)
    r = train_decoder.main(dataset["common"] + ["--json_path", dataset["json"], "--output_dir", str(out), "--decoder_checkpoint", str(start_path),
                                                "--num_epochs", "2", "--train_batch_size", "4", "--save_steps", "1", "--lr_warmup_steps", "0",
                                                "--train_front", "--use_cross_attention", "--train_cross_attention"])
    start = torch.load(start_path, map_location="cpu")
    for f in ("best_pytorch_model.bin", "pytorch_model.bin", "training_history.json", "train_report.json") + EVAL_FILES:
        assert os.path.isfile(out / f), f
    report = json.loads((out / "train_report.json").read_text())
    epochs = report["epochs"]
    assert [e["encoder_batches"] for e in epochs] == [4, 0], "epoch 2 takes no encoder batch"
    assert report["latent_cache"]["cached"] and report["feature_cache_bytes"] == 0
    saved = torch.load(out / "pytorch_model.bin", map_location="cpu")
    assert list(saved) == list(start) and any(k.startswith(CROSS_PREFIXES) for k in saved)
    for k, v in start.items():
        if k.startswith(CROSS_PREFIXES + FRONT_PREFIXES) and k not in ZERO:
            assert not torch.equal(saved[k], v), k
    assert not torch.equal(saved["classifier.12.weight"], start["classifier.12.weight"])
    assert int(saved[NBT]) == int(start[NBT]) + sum(e["steps"] for e in epochs)
    assert all(torch.isfinite(v.float()).all() for v in saved.values())
    # the best checkpoint, scored by evaluate --val_loss over the validation image
    history = json.loads((out / "training_history.json").read_text())
    paths = list(dataset["data"])
    _, val_idx = split_indices(len(paths), 42)
    (root / "val_cross.json").write_text(json.dumps({paths[i]: dataset["data"][paths[i]] for i in val_idx}))
    evaluate.main(dataset["common"] + ["--json_path", str(root / "val_cross.json"), "--decoder_checkpoint", str(out / "best_pytorch_model.bin"),
                                       "--batch_size", "4", "--output_dir", str(root / "val_cross_eval"), "--single_pass", "--val_loss",
                                       "--use_cross_attention"])
    scored = json.loads((root / "val_cross_eval" / "validation_loss.json").read_text())["val_loss"]
    print(f"recorded best val_loss {min(history['val_loss'])!r}, evaluate --val_loss {scored!r}")
    assert min(history["val_loss"]) == r["best_val_loss"]
    assert scored == r["best_val_loss"]
