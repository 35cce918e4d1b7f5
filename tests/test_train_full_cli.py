"""python -m vae_tagger_amd.train_full on the device: eight generated 64 x 64 pictures, the small VAE (block_out (64, 128, 512), one layer per block) from
a --vae_config_path and an input checkpoint, resolution 64, batch 2, 2 epochs of 4 steps, --save_steps 1.  The files the reference writes, best_vae and
best_decoder through the loaders, byte-identical files from two runs and from a run that was stopped after one epoch and resumed, and which VAE tensors
each loss trains."""
import json

import numpy as np
import pytest
import torch

from vae_tagger_amd import synth, train_full
from vae_tagger_amd.train_vae import MODEL_FILE, OPTIMIZER_FILE, STATE_FILE

pytestmark = pytest.mark.gpu
TAGS = ["cat", "dog", "tree", "sky", "car"]
PROMPTS = ["cat, dog", "dog:0.5, tree", "sky", "cat, sky, car", "tree, car:0.25", "dog", "cat", "tree, sky"]
SMALL = dict(block_out=(64, 128, 512), layers_per_block=1)
CONFIG = {"_class_name": "AutoencoderKL", "act_fn": "silu", "block_out_channels": [64, 128, 512], "down_block_types": ["DownEncoderBlock2D"] * 3,
          "up_block_types": ["UpDecoderBlock2D"] * 3, "in_channels": 3, "out_channels": 3, "latent_channels": 16, "layers_per_block": 1,
          "norm_num_groups": 32, "sample_size": 64, "scaling_factor": 0.3611, "shift_factor": 0.1159, "use_quant_conv": False,
          "use_post_quant_conv": False, "force_upcast": True, "mid_block_add_attention": True}
SEED, LR, EPOCHS, BATCH, STEPS = 7, 2e-4, 2, 2, 4
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
    return sd


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("train_full")
    start = _dataset(tmp)
    common = ["--json_path", str(tmp / "data.json"), "--tags_csv_path", str(tmp / "tags.csv"), "--vae_config_path", str(tmp / "vae_config.json"),
              "--vae_checkpoint", str(tmp / "vae_in.safetensors"), "--resolution", "64", "--train_batch_size", str(BATCH), "--num_epochs", str(EPOCHS),
              "--save_steps", "1", "--lr_warmup_steps", "2", "--learning_rate", str(LR), "--seed", str(SEED), "--logging_steps", "2", "--weight_decay", "1e-2"]
    torch.manual_seed(11)                                                                      # (a decoder trained from scratch is initialised from torch's generator)
    train_full.main(common + ["--output_dir", str(tmp / "a")])
    torch.manual_seed(11)
    train_full.main(common + ["--output_dir", str(tmp / "b")])
    torch.manual_seed(11)
    train_full.main(common + ["--output_dir", str(tmp / "c"), "--stop_after_epochs", "1"])
    assert not (tmp / "c" / "checkpoint-1").exists() and (tmp / "c" / "checkpoint-0" / STATE_FILE).exists()
    train_full.main(common + ["--output_dir", str(tmp / "c"), "--resume_from", str(tmp / "c" / "checkpoint-0")])
    torch.manual_seed(11)
    train_full.main(common + ["--output_dir", str(tmp / "d"), "--full_loss", "--stop_after_epochs", "1", "--reconstruction_weight", "1.0"])
    return {"tmp": tmp, "common": common, "start": start}


def test_every_file_is_written_and_the_models_load(runs):
    from safetensors.torch import load_file
    from vae_tagger_amd.diffusers_vae_loader import load_diffusers_vae_from_pretrained
    from vae_tagger_amd.infer_full import load_state_dict_file
    from vae_tagger_amd.modules import create_attention_decoder
    out = runs["tmp"] / "a"
    for d in VAE_DIRS:
        assert (out / d / "config.json").exists() and (out / d / MODEL_FILE).exists(), d
    for d in DECODER_DIRS:
        assert (out / d / train_full.DECODER_FILE).exists(), d
    for d in CHECKPOINTS:
        assert (out / d / OPTIMIZER_FILE).exists() and (out / d / train_full.DECODER_OPTIMIZER_FILE).exists() and (out / d / STATE_FILE).exists(), d
    for name in ("training_history.json", "train_report.json", "optimal_thresholds.json", "evaluation_results.csv", "evaluation_results_overall.json"):
        assert (out / name).exists(), name
    history = json.load(open(out / "training_history.json"))
    report = json.load(open(out / "train_report.json"))
    assert set(history) == {"train_loss", "val_loss", "learning_rates"} and all(len(v) == EPOCHS for v in history.values())
    assert all(np.isfinite(history["train_loss"])) and all(np.isfinite(history["val_loss"])) and history["train_loss"][0] != history["train_loss"][1]
    state = json.load(open(out / "checkpoint-1" / STATE_FILE))
    assert (state["step"], state["epoch"], state["images"]) == (EPOCHS * STEPS, 2, 14) and state["best_val_loss"] == min(history["val_loss"])
    assert len(report["epochs"]) == EPOCHS and report["steps_per_epoch"] == STEPS and report["clip"] is True and report["simplified"] is True
    assert report["vae_tensors_trained"] == 64 and report["decoder_blocks"] == 2 and report["selected_loss"] == "bce"
    for e in report["epochs"]:
        assert e["steps"] == STEPS and e["images"] == 7 and e["seconds"] > 0 and e["images_per_second"] > 0 and e["saved_bytes_per_step"] > 0
        assert e["grad_norm"]["norm"] > 0 and 0 < e["grad_norm"]["coef"] <= 1.0
        assert set(e["state_sha256"]) == {"vae", "decoder"} and all(len(v) == 64 for v in e["state_sha256"].values())
    assert report["epochs"][0]["state_sha256"]["vae"] != report["epochs"][1]["state_sha256"]["vae"]
    assert report["epochs"][0]["state_sha256"]["decoder"] != report["epochs"][1]["state_sha256"]["decoder"]
    print(f"  images/s per epoch on the tiny set: {[round(e['images_per_second'], 2) for e in report['epochs']]}")
    # best_vae through the loader --vae_checkpoint uses, best_decoder through infer_full's
    vae = load_diffusers_vae_from_pretrained(str(out / "best_vae"))
    assert vae is not None and list(vae.config.block_out_channels) == [64, 128, 512]
    saved = load_file(str(out / "best_vae" / MODEL_FILE))
    assert len(saved) == 152 and all(torch.equal(vae.state_dict()[k], saved[k]) for k in vae.state_dict())
    sd = load_state_dict_file(str(out / "best_decoder" / train_full.DECODER_FILE))
    dec = create_attention_decoder(16, 8, 8, len(TAGS), {})                                     # (the CLI's default: spatial and self attention)
    missing, unexpected = dec.load_state_dict(sd, strict=False)
    assert not missing and not unexpected and set(sd) == set(dec.state_dict())
    best = int(np.argmin(history["val_loss"]))
    assert (out / "best_checkpoint" / MODEL_FILE).read_bytes() == (out / f"checkpoint-{best}" / MODEL_FILE).read_bytes()
    assert (out / "best_decoder" / train_full.DECODER_FILE).read_bytes() == (out / f"checkpoint-{best}" / train_full.DECODER_FILE).read_bytes()


def _same_files(x, y):
    for d in VAE_DIRS:
        assert (x / d / MODEL_FILE).read_bytes() == (y / d / MODEL_FILE).read_bytes(), d
        assert (x / d / "config.json").read_bytes() == (y / d / "config.json").read_bytes(), d
    for d in DECODER_DIRS:
        a, b = (torch.load(str(p / d / train_full.DECODER_FILE), map_location="cpu", weights_only=True) for p in (x, y))
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a), d
    for d in CHECKPOINTS:
        for name in (OPTIMIZER_FILE, train_full.DECODER_OPTIMIZER_FILE, STATE_FILE):
            assert (x / d / name).read_bytes() == (y / d / name).read_bytes(), (d, name)
    assert json.load(open(x / "training_history.json")) == json.load(open(y / "training_history.json"))
    sha = lambda p: [e["state_sha256"] for e in json.load(open(p / "train_report.json"))["epochs"]]
    assert sha(x) == sha(y) and len(sha(x)) == EPOCHS
    for name in ("optimal_thresholds.json", "evaluation_results_overall.json"):
        assert (x / name).read_bytes() == (y / name).read_bytes(), name


def test_two_runs_write_the_same_bytes(runs):
    _same_files(runs["tmp"] / "a", runs["tmp"] / "b")


def test_a_resumed_run_equals_the_straight_one(runs):
    _same_files(runs["tmp"] / "a", runs["tmp"] / "c")


def test_which_vae_tensors_each_loss_trains(runs):
    from safetensors.torch import load_file
    start = runs["start"]
    simplified = load_file(str(runs["tmp"] / "a" / "checkpoint-1" / MODEL_FILE))
    full = load_file(str(runs["tmp"] / "d" / "checkpoint-0" / MODEL_FILE))
    assert set(simplified) == set(full) == set(start)
    for k, v in start.items():
        if k.startswith("decoder."):
            assert torch.equal(simplified[k], v), k                                             # weight decay 1e-2 included: not a bit
            assert not torch.equal(full[k], v), k
        else:
            assert not torch.equal(simplified[k], v) and not torch.equal(full[k], v), k
    # the moments of the image decoder were never written either
    opt = load_file(str(runs["tmp"] / "a" / "checkpoint-1" / OPTIMIZER_FILE))
    assert all(not bool(v.any()) for k, v in opt.items() if k.startswith(("exp_avg.decoder.", "exp_avg_sq.decoder.")))
    assert all(bool(v.any()) for k, v in opt.items() if k.startswith("exp_avg.encoder."))
    report = json.load(open(runs["tmp"] / "d" / "train_report.json"))
    assert report["simplified"] is False and report["vae_tensors_trained"] == 152 and len(report["epochs"]) == 1
