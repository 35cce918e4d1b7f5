"""python -m vae_tagger_amd.train_vae on the device: 12 generated pictures, the small configuration (block_out (64, 128, 512), one layer per block)
from a --vae_config_path, resolution 32, batch 2, 2 epochs of 6 steps, --save_steps 1, 2 warm-up steps.  The files the reference writes, best_vae
through the loader, val_loss against evaluate_vae.run_checkpoint on the saved model, byte-identical files from two runs and from a run that was
stopped after one epoch and resumed, the logged learning rates, and --max_grad_norm 0."""
import json

import numpy as np
import pytest
import torch

from vae_tagger_amd import train_vae
from vae_tagger_amd.train import lr_schedule, split_indices

pytestmark = pytest.mark.gpu
TAGS = ["cat", "dog", "tree", "sky", "car"]
PROMPTS = ["cat, dog", "dog:0.5, tree", "sky", "cat, sky, car", "tree, car:0.25", "dog", "cat", "tree, sky", "car, dog", "sky, dog", "cat, tree", "car"]
CONFIG = {"_class_name": "AutoencoderKL", "act_fn": "silu", "block_out_channels": [64, 128, 512], "down_block_types": ["DownEncoderBlock2D"] * 3,
          "up_block_types": ["UpDecoderBlock2D"] * 3, "in_channels": 3, "out_channels": 3, "latent_channels": 16, "layers_per_block": 1,
          "norm_num_groups": 32, "sample_size": 32, "scaling_factor": 0.3611, "shift_factor": 0.1159, "use_quant_conv": False,
          "use_post_quant_conv": False, "force_upcast": True, "mid_block_add_attention": True}
SEED, LR, EPOCHS, WARMUP, BATCH = 7, 2e-4, 2, 2, 2
MODEL_DIRS = ["best_vae", "best_checkpoint", "checkpoint-0", "checkpoint-1", "vae_checkpoint_epoch_0", "vae_checkpoint_epoch_1"]


def _dataset(tmp):
    from PIL import Image
    rng = np.random.default_rng(17)
    paths = []
    for i in range(12):
        yy, xx = np.mgrid[0:64, 0:64]
        img = np.stack([(xx * (i + 1) * 4) % 256, (yy * (12 - i) * 3) % 256, rng.integers(0, 256, (64, 64))], axis=2).astype(np.uint8)
        paths.append(str(tmp / f"img_{i}.png"))
        Image.fromarray(img).save(paths[-1])
    (tmp / "tags.csv").write_text("name\n" + "\n".join(TAGS) + "\n")
    (tmp / "data.json").write_text(json.dumps(dict(zip(paths, PROMPTS))))
    (tmp / "vae_config.json").write_text(json.dumps(CONFIG))
    return paths


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("train_vae")
    paths = _dataset(tmp)
    common = ["--json_path", str(tmp / "data.json"), "--tags_csv_path", str(tmp / "tags.csv"), "--vae_config_path", str(tmp / "vae_config.json"),
              "--resolution", "32", "--train_batch_size", str(BATCH), "--num_epochs", str(EPOCHS), "--save_steps", "1", "--lr_warmup_steps", str(WARMUP),
              "--learning_rate", str(LR), "--seed", str(SEED), "--reconstruction_weight", "1.0", "--logging_steps", "4"]
    train_vae.main(common + ["--output_dir", str(tmp / "a")])
    train_vae.main(common + ["--output_dir", str(tmp / "b")])
    train_vae.main(common + ["--output_dir", str(tmp / "c"), "--stop_after_epochs", "1"])
    assert not (tmp / "c" / "checkpoint-1").exists() and (tmp / "c" / "checkpoint-0" / "state.json").exists()
    train_vae.main(common + ["--output_dir", str(tmp / "c"), "--resume_from", str(tmp / "c" / "checkpoint-0")])
    train_vae.main(common + ["--output_dir", str(tmp / "d"), "--max_grad_norm", "0", "--stop_after_epochs", "1", "--mixed_precision", "bf16"])
    return {"tmp": tmp, "paths": paths, "common": common}


def test_every_file_is_written_and_best_vae_loads(runs):
    from vae_tagger_amd.diffusers_vae_loader import load_diffusers_vae_from_pretrained
    out = runs["tmp"] / "a"
    for d in MODEL_DIRS:
        assert (out / d / "config.json").exists() and (out / d / train_vae.MODEL_FILE).exists(), d
    for d in ("best_checkpoint", "checkpoint-0", "checkpoint-1"):
        assert (out / d / train_vae.OPTIMIZER_FILE).exists() and (out / d / train_vae.STATE_FILE).exists(), d
    history = json.load(open(out / "training_history.json"))
    report = json.load(open(out / "train_report.json"))
    assert set(history) == {"train_loss", "val_loss", "learning_rates"} and all(len(v) == EPOCHS for v in history.values())
    state = json.load(open(out / "checkpoint-1" / "state.json"))
    assert (state["step"], state["epoch"], state["images"]) == (12, 2, 22) and state["best_val_loss"] == min(history["val_loss"])
    assert len(report["epochs"]) == EPOCHS and report["steps_per_epoch"] == 6 and report["clip"] is True
    for e in report["epochs"]:
        assert e["steps"] == 6 and e["images"] == 11 and e["seconds"] > 0 and e["images_per_second"] > 0 and e["saved_bytes_per_step"] > 0
        assert e["grad_norm"]["norm"] > 0 and 0 < e["grad_norm"]["coef"] <= 1.0 and len(e["optimizer_state_sha256"]) == 64
    assert report["epochs"][0]["optimizer_state_sha256"] != report["epochs"][1]["optimizer_state_sha256"]
    vae = load_diffusers_vae_from_pretrained(str(out / "best_vae"))
    assert vae is not None and list(vae.config.block_out_channels) == [64, 128, 512]
    from safetensors.torch import load_file
    saved = load_file(str(out / "best_vae" / train_vae.MODEL_FILE))
    assert len(saved) == 152 and all(torch.equal(vae.state_dict()[k], saved[k]) for k in vae.state_dict())
    assert all(torch.equal(v, saved[k]) for k, v in vae.image_decoder().state_dict().items())


def test_val_loss_is_run_checkpoint_on_the_saved_model(runs):
    from types import SimpleNamespace
    from vae_tagger_amd import evaluate_vae
    from vae_tagger_amd.diffusers_vae_loader import DiffusersVAEWrapper, load_diffusers_vae_from_pretrained
    from vae_tagger_amd.evaluate import TaggedImageList
    tmp, out = runs["tmp"], runs["tmp"] / "a"
    history = json.load(open(out / "training_history.json"))
    args = train_vae.build_parser().parse_args(runs["common"])
    data = TaggedImageList(args.json_path, args.tags_csv_path)
    _, val_idx = split_indices(len(data.image_paths), SEED)
    val_paths = [data.image_paths[i] for i in val_idx]
    labels = np.stack([data.labels[p] for p in val_paths]).astype(np.float32)
    triplets = evaluate_vae.triplet_lists(labels, SEED)
    batches = evaluate_vae.plan_batches(val_paths, BATCH)
    for epoch in range(EPOCHS):
        model = DiffusersVAEWrapper(load_diffusers_vae_from_pretrained(str(out / f"vae_checkpoint_epoch_{epoch}"))).to("cuda:0").eval()
        model.check_finite = False
        state, _, _ = evaluate_vae.run_checkpoint(args, model, SimpleNamespace(image_paths=val_paths), labels, triplets, batches, device="cuda:0")
        assert evaluate_vae.build_report(state, args)["val_loss"] == history["val_loss"][epoch], epoch
    best = int(np.argmin(history["val_loss"]))
    assert (out / "best_vae" / train_vae.MODEL_FILE).read_bytes() == (out / f"vae_checkpoint_epoch_{best}" / train_vae.MODEL_FILE).read_bytes()
    assert history["train_loss"][1] != history["train_loss"][0] and all(np.isfinite(history["train_loss"]))


def _same_files(x, y):
    for d in MODEL_DIRS:
        assert (x / d / train_vae.MODEL_FILE).read_bytes() == (y / d / train_vae.MODEL_FILE).read_bytes(), d
        assert (x / d / "config.json").read_bytes() == (y / d / "config.json").read_bytes(), d
    for d in ("best_checkpoint", "checkpoint-0", "checkpoint-1"):
        assert (x / d / train_vae.OPTIMIZER_FILE).read_bytes() == (y / d / train_vae.OPTIMIZER_FILE).read_bytes(), d
        assert (x / d / train_vae.STATE_FILE).read_bytes() == (y / d / train_vae.STATE_FILE).read_bytes(), d
    assert json.load(open(x / "training_history.json")) == json.load(open(y / "training_history.json"))
    sha = lambda p: [e["optimizer_state_sha256"] for e in json.load(open(p / "train_report.json"))["epochs"]]
    assert sha(x) == sha(y) and len(sha(x)) == EPOCHS


def test_two_runs_write_the_same_bytes(runs):
    _same_files(runs["tmp"] / "a", runs["tmp"] / "b")


def test_a_resumed_run_equals_the_straight_one(runs):
    _same_files(runs["tmp"] / "a", runs["tmp"] / "c")


def test_logged_lr_follows_the_schedule_and_no_clip_is_reported(runs):
    report = json.load(open(runs["tmp"] / "a" / "train_report.json"))
    total = EPOCHS * 6
    for e in report["epochs"]:
        want = [LR * lr_schedule("cosine", e["epoch"] * 6 + k, WARMUP, total) for k in range(6)]
        assert e["learning_rates"] == want, e["epoch"]
    assert report["epochs"][0]["learning_rates"][:3] == [0.0, LR / 2, LR]
    history = json.load(open(runs["tmp"] / "a" / "training_history.json"))
    assert history["learning_rates"] == [LR * lr_schedule("cosine", 6 * (e + 1), WARMUP, total) for e in range(EPOCHS)]
    plain = json.load(open(runs["tmp"] / "d" / "train_report.json"))
    assert plain["clip"] is False and plain["max_grad_norm"] == 0 and plain["epochs"][0]["grad_norm"] is None and len(plain["epochs"]) == 1
    assert plain["ignored_arguments"] == ["mixed_precision"] and report["ignored_arguments"] == []
    assert plain["epochs"][0]["optimizer_state_sha256"] != report["epochs"][0]["optimizer_state_sha256"]
