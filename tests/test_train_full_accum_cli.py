"""python -m vae_tagger_amd.train_full --accumulate_gradients --gradient_accumulation_steps 3 on the device: the dataset and the arguments of
tests/test_train_full_cli.py (eight generated 64 x 64 pictures, the small VAE, batch 2, 2 epochs of 4 steps, --save_steps 1).  By the reference's
rule -- the optimiser steps when (step + 1) % 3 == 0 with `step` counted inside the epoch -- the run takes optimiser steps at micro-steps 3
(three micro-gradients) and 7 (four: the tail of epoch 0 and three of epoch 1), and each epoch ends with one micro-step pending.  Two runs
write the same bytes; a run stopped after epoch 0, with its pending micro-step in pending_gradients.safetensors, and resumed equals the
straight one; the counters in state.json; and A = 1 under the flag writes what a run without the flag writes."""
import json

import numpy as np
import pytest
import torch

from vae_tagger_amd import synth, train_full
from vae_tagger_amd.train import lr_schedule
from vae_tagger_amd.train_vae import MODEL_FILE, OPTIMIZER_FILE, STATE_FILE

pytestmark = pytest.mark.gpu
TAGS = ["cat", "dog", "tree", "sky", "car"]
PROMPTS = ["cat, dog", "dog:0.5, tree", "sky", "cat, sky, car", "tree, car:0.25", "dog", "cat", "tree, sky"]
SMALL = dict(block_out=(64, 128, 512), layers_per_block=1)
CONFIG = {"_class_name": "AutoencoderKL", "act_fn": "silu", "block_out_channels": [64, 128, 512], "down_block_types": ["DownEncoderBlock2D"] * 3,
          "up_block_types": ["UpDecoderBlock2D"] * 3, "in_channels": 3, "out_channels": 3, "latent_channels": 16, "layers_per_block": 1,
          "norm_num_groups": 32, "sample_size": 64, "scaling_factor": 0.3611, "shift_factor": 0.1159, "use_quant_conv": False,
          "use_post_quant_conv": False, "force_upcast": True, "mid_block_add_attention": True}
SEED, LR, EPOCHS, BATCH, STEPS, A, WARMUP = 7, 2e-4, 2, 2, 4, 3, 2
CHECKPOINTS = ["best_checkpoint", "checkpoint-0", "checkpoint-1"]
VAE_DIRS, DECODER_DIRS = ["best_vae", "vae"] + CHECKPOINTS, ["best_decoder", "decoder"] + CHECKPOINTS


def _dataset(tmp):
    from PIL import Image
    from safetensors.torch import save_file
    rng = np.random.default_rng(17)
    paths = []
    for i in range(8):
        yy, xx = np.mgrid[0:64, 0:64]
        img = np.stack([(xx * (i + 1) * 4) % 256, (yy * (12 - i) * 3) % 256, rng.integers(0, 256, (64, 64))], axis=2).astype(np.uint8)
        paths.append(str(tmp / f"img_{i}.png"))
        Image.fromarray(img).save(paths[-1])
    (tmp / "tags.csv").write_text("name\n" + "\n".join(TAGS) + "\n")
    (tmp / "data.json").write_text(json.dumps(dict(zip(paths, PROMPTS))))
    (tmp / "vae_config.json").write_text(json.dumps(CONFIG))
    sd = synth.synth_state_dict({**synth.encoder_manifest(**SMALL), **synth.image_decoder_manifest(**SMALL)}, seed=3)
    save_file(sd, str(tmp / "vae_in.safetensors"))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("train_full_accum")
    _dataset(tmp)
    common = ["--json_path", str(tmp / "data.json"), "--tags_csv_path", str(tmp / "tags.csv"), "--vae_config_path", str(tmp / "vae_config.json"),
              "--vae_checkpoint", str(tmp / "vae_in.safetensors"), "--resolution", "64", "--train_batch_size", str(BATCH), "--num_epochs", str(EPOCHS),
              "--save_steps", "1", "--lr_warmup_steps", str(WARMUP), "--learning_rate", str(LR), "--seed", str(SEED), "--logging_steps", "2",
              "--weight_decay", "1e-2"]
    accum = common + ["--accumulate_gradients", "--gradient_accumulation_steps", str(A)]

    def run(name, flags, *more):
        torch.manual_seed(11)                                                                   # (a decoder trained from scratch is initialised from torch's generator)
        train_full.main(flags + ["--output_dir", str(tmp / name)] + list(more))
    run("a", accum)
    run("b", accum)
    run("c", accum, "--stop_after_epochs", "1")
    assert not (tmp / "c" / "checkpoint-1").exists() and (tmp / "c" / "checkpoint-0" / STATE_FILE).exists()
    train_full.main(accum + ["--output_dir", str(tmp / "c"), "--resume_from", str(tmp / "c" / "checkpoint-0")])
    run("one", common + ["--accumulate_gradients", "--gradient_accumulation_steps", "1"])
    run("plain", common)
    return tmp


def _same_files(x, y):
    for d in VAE_DIRS:
        assert (x / d / MODEL_FILE).read_bytes() == (y / d / MODEL_FILE).read_bytes(), d
        assert (x / d / "config.json").read_bytes() == (y / d / "config.json").read_bytes(), d
    for d in DECODER_DIRS:
        a, b = (torch.load(str(p / d / train_full.DECODER_FILE), map_location="cpu", weights_only=True) for p in (x, y))
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a), d
    for d in CHECKPOINTS:
        for name in (OPTIMIZER_FILE, train_full.DECODER_OPTIMIZER_FILE, STATE_FILE, train_full.PENDING_FILE):
            assert (x / d / name).exists() == (y / d / name).exists(), (d, name)
            if (x / d / name).exists():
                assert (x / d / name).read_bytes() == (y / d / name).read_bytes(), (d, name)
    assert json.load(open(x / "training_history.json")) == json.load(open(y / "training_history.json"))
    sha = lambda p: [e["state_sha256"] for e in json.load(open(p / "train_report.json"))["epochs"]]
    assert sha(x) == sha(y) and len(sha(x)) == EPOCHS
    for name in ("optimal_thresholds.json", "evaluation_results_overall.json"):
        assert (x / name).read_bytes() == (y / name).read_bytes(), name


def test_two_runs_write_the_same_bytes(runs):
    _same_files(runs / "a", runs / "b")


def test_a_run_resumed_with_a_micro_step_pending_equals_the_straight_one(runs):
    state = json.load(open(runs / "c" / "checkpoint-0" / STATE_FILE))
    assert state["pending_micro_steps"] == 1 and state["micro_steps"] == 4 and state["optimizer_steps"] == 1     # epoch 0 ends with one pending
    assert (runs / "c" / "checkpoint-0" / train_full.PENDING_FILE).exists()
    _same_files(runs / "a", runs / "c")


def test_counters_and_learning_rates(runs):
    """pending_micro_steps after the second epoch follows from the rule the plan implements, (step + 1) % 3 == 0 with `step` counted inside the
    epoch: epoch 1 steps at its third micro-step on four micro-gradients and its fourth stays pending -- one, where counting (step + 1) % 3
    over the whole run would leave two: 8 micro-steps are 3 + 4 stepped and 1 pending (tests/test_train_full_accum_host.py pins
    accumulation_plan's [[0, 1, 2], [3, 4, 5, 6]] and [[3], [7]] against a literal simulation of the reference's counters)."""
    state = json.load(open(runs / "a" / "checkpoint-1" / STATE_FILE))
    assert state["micro_steps"] == 8 and state["optimizer_steps"] == 2 and state["pending_micro_steps"] == 1
    assert (state["step"], state["epoch"], state["images"]) == (EPOCHS * STEPS, 2, 14)
    assert (runs / "a" / "checkpoint-1" / train_full.PENDING_FILE).exists()
    history = json.load(open(runs / "a" / "training_history.json"))
    total = EPOCHS * STEPS                                                                      # the schedule's length stays num_epochs * steps_per_epoch
    assert history["learning_rates"] == [LR * lr_schedule("cosine", k, WARMUP, total) for k in (1, 2)]
    report = json.load(open(runs / "a" / "train_report.json"))
    assert [e["accumulation_steps"] for e in report["epochs"]] == [A, A] and [e["optimizer_steps"] for e in report["epochs"]] == [1, 1]
    assert [e["steps"] for e in report["epochs"]] == [STEPS, STEPS]
    lrs = [LR * lr_schedule("cosine", k, WARMUP, total) for k in (0, 0, 0, 1, 1, 1, 1, 2)]      # the rate in force at every micro-step
    assert [lr for e in report["epochs"] for lr in e["learning_rates"]] == lrs
    assert all(np.isfinite(history["train_loss"])) and all(np.isfinite(history["val_loss"]))
    # accumulation is another optimiser than the plain run
    assert (runs / "a" / "checkpoint-1" / MODEL_FILE).read_bytes() != (runs / "plain" / "checkpoint-1" / MODEL_FILE).read_bytes()


def test_one_step_of_accumulation_under_the_flag_is_the_run_without_it(runs):
    _same_files(runs / "one", runs / "plain")
    assert not any((runs / "one" / d / train_full.PENDING_FILE).exists() for d in CHECKPOINTS)
    state = json.load(open(runs / "one" / "checkpoint-1" / STATE_FILE))
    assert state["micro_steps"] == state["optimizer_steps"] == state["step"] == 8 and state["pending_micro_steps"] == 0
