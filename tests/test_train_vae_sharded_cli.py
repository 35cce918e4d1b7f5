"""`python -m vae_tagger_amd.train_vae ... --sharded` end to end (GPU), on the data set and configuration of tests/test_train_vae_cli.py (12 generated
pictures, block_out (64, 128, 512), resolution 32, 2 epochs): a one-rank RCCL rehearsal (VT_CLI_ONE_RANK_GROUP=1) whose forced exchange -- export,
all_to_all_single, merge of K = 1 at weight 1, all_gather_into_tensor -- must leave every byte of the plain run; and two ranks that share GPU 0 over
gloo (VT_CLI_GLOO=1; RCCL needs one GPU per rank) at batch 1 against the plain run at batch 2: the same batches, so the same step counts, learning
rates and image counts, and a different summation order.  11 training images at a global batch of 2: rank 1's slice of each epoch's last batch is
empty and that step is taken at weights (1, 0).  None of this yields a scaling figure."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from vae_tagger_amd import train_vae

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ["cat", "dog", "tree", "sky", "car"]
PROMPTS = ["cat, dog", "dog:0.5, tree", "sky", "cat, sky, car", "tree, car:0.25", "dog", "cat", "tree, sky", "car, dog", "sky, dog", "cat, tree", "car"]
CONFIG = {"_class_name": "AutoencoderKL", "act_fn": "silu", "block_out_channels": [64, 128, 512], "down_block_types": ["DownEncoderBlock2D"] * 3,
          "up_block_types": ["UpDecoderBlock2D"] * 3, "in_channels": 3, "out_channels": 3, "latent_channels": 16, "layers_per_block": 1,
          "norm_num_groups": 32, "sample_size": 32, "scaling_factor": 0.3611, "shift_factor": 0.1159, "use_quant_conv": False,
          "use_post_quant_conv": False, "force_upcast": True, "mid_block_add_attention": True}
SEED, LR, EPOCHS, WARMUP, STEPS = 7, 2e-4, 2, 2, 6
MODEL_DIRS = ["best_vae", "best_checkpoint", "checkpoint-0", "checkpoint-1", "vae_checkpoint_epoch_0", "vae_checkpoint_epoch_1"]
CHECKPOINTS = ("best_checkpoint", "checkpoint-0", "checkpoint-1")


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from PIL import Image
    tmp = tmp_path_factory.mktemp("train_vae_sharded")
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
    common = ["--json_path", str(tmp / "data.json"), "--tags_csv_path", str(tmp / "tags.csv"), "--vae_config_path", str(tmp / "vae_config.json"),
              "--resolution", "32", "--num_epochs", str(EPOCHS), "--save_steps", "1", "--lr_warmup_steps", str(WARMUP), "--learning_rate", str(LR),
              "--seed", str(SEED), "--reconstruction_weight", "1.0", "--logging_steps", "4"]
    train_vae.main(common + ["--train_batch_size", "2", "--output_dir", str(tmp / "plain")])
    return {"tmp": tmp, "common": common}


def env(**extra):
    return dict(os.environ, PYTHONDONTWRITEBYTECODE="1", HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT, **extra)


def run_one_rank(dataset, out):
    cmd = [sys.executable, "-m", "vae_tagger_amd.train_vae"] + dataset["common"] + ["--train_batch_size", "2", "--output_dir", str(out), "--sharded"]
    r = subprocess.run(cmd, env=env(VT_CLI_ONE_RANK_GROUP="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29800 + os.getpid() % 40)), cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return r.stdout.decode()


def run_two_ranks(dataset, out, salt, *more):
    port = str(29500 + (os.getpid() + 11 * salt + 100) % 200)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", port,
           "-m", "vae_tagger_amd.train_vae"] + dataset["common"] + ["--train_batch_size", "1", "--output_dir", str(out), "--sharded", *more]
    r = subprocess.run(cmd, env=env(VT_CLI_GLOO="1"), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=420)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return r.stdout.decode()


def load(out, *parts):
    return json.load(open(os.path.join(str(out), *parts)))


def same_files(x, y):
    for d in MODEL_DIRS:
        assert (x / d / train_vae.MODEL_FILE).read_bytes() == (y / d / train_vae.MODEL_FILE).read_bytes(), d
        assert (x / d / "config.json").read_bytes() == (y / d / "config.json").read_bytes(), d
    for d in CHECKPOINTS:
        assert (x / d / train_vae.OPTIMIZER_FILE).read_bytes() == (y / d / train_vae.OPTIMIZER_FILE).read_bytes(), d
        assert (x / d / train_vae.STATE_FILE).read_bytes() == (y / d / train_vae.STATE_FILE).read_bytes(), d
    assert (x / "training_history.json").read_bytes() == (y / "training_history.json").read_bytes()
    sha = lambda p: [e["optimizer_state_sha256"] for e in load(p, "train_report.json")["epochs"]]
    assert sha(x) == sha(y) and len(sha(x)) == EPOCHS


def test_one_rank_rccl_rehearsal_writes_the_plain_runs_bytes(dataset):
    tmp = dataset["tmp"]
    text = run_one_rank(dataset, tmp / "rehearsal")
    same_files(tmp / "plain", tmp / "rehearsal")
    report = load(tmp / "rehearsal", "train_report.json")
    sh = report["sharded"]
    assert sh["world"] == 1 and sh["backend"] == "nccl" and sh["per_rank_batch"] == 2 and sh["exchange_calls"] == EPOCHS * STEPS
    assert sh["bytes_sent_per_step"] == sh["bytes_received_per_step"] == 0 and len(sh["state_sha256"]) == 1
    assert sh["state_sha256"][0] == report["epochs"][-1]["optimizer_state_sha256"]
    assert "sharded" not in load(tmp / "plain", "train_report.json") and text.count("VAE训练完成") == 1


def test_two_ranks_over_gloo_see_the_plain_runs_batches(dataset):
    tmp = dataset["tmp"]
    text = run_two_ranks(dataset, tmp / "two_a", 0)
    run_two_ranks(dataset, tmp / "two_b", 1)
    assert sorted(os.listdir(tmp / "two_a")) == sorted(MODEL_DIRS + ["training_history.json", "train_report.json"])      # every file once, nothing else
    assert text.count("VAE训练完成") == 1 and text.count("Epoch 0 completed") == 1                                          # rank 0 alone prints
    plain, two = load(tmp / "plain", "train_report.json"), load(tmp / "two_a", "train_report.json")
    sh = two["sharded"]
    assert sh["world"] == 2 and sh["backend"] == "gloo" and sh["per_rank_batch"] == 1 and sh["exchange_calls"] == EPOCHS * STEPS
    assert sh["state_sha256"][0] == sh["state_sha256"][1] == two["epochs"][-1]["optimizer_state_sha256"] and len(sh["state_sha256"][0]) == 64
    assert sh["bytes_sent_per_step"] == sh["bytes_received_per_step"] > 0
    assert two["steps_per_epoch"] == plain["steps_per_epoch"] == STEPS and two["total_steps"] == plain["total_steps"]
    for a, b in zip(plain["epochs"], two["epochs"]):
        assert a["learning_rates"] == b["learning_rates"] and a["steps"] == b["steps"] == STEPS and a["images"] == b["images"] == 11
    for d in CHECKPOINTS[1:]:
        a, b = load(tmp / "plain", d, "state.json"), load(tmp / "two_a", d, "state.json")
        assert (a["step"], a["epoch"], a["images"]) == (b["step"], b["epoch"], b["images"]), d
    assert load(tmp / "two_a", "checkpoint-1", "state.json")["images"] == 22      # 11 a epoch: the last global batch holds one image, rank 1 none
    assert train_vae.shard_weights(11 % 2, 2, 1) == [1.0, 0.0]
    h_plain, h_two = load(tmp / "plain", "training_history.json"), load(tmp / "two_a", "training_history.json")
    assert h_plain["learning_rates"] == h_two["learning_rates"] and all(np.isfinite(h_two["train_loss"])) and all(np.isfinite(h_two["val_loss"]))
    print(f"train_loss: plain at batch 2 {h_plain['train_loss']!r}, two ranks at batch 1 {h_two['train_loss']!r}")
    same_files(tmp / "two_a", tmp / "two_b")                                      # a second two-rank run writes the same bytes


def test_a_resumed_two_rank_run_equals_the_straight_one(dataset):
    tmp = dataset["tmp"]
    if not (tmp / "two_a").exists():
        run_two_ranks(dataset, tmp / "two_a", 0)
    run_two_ranks(dataset, tmp / "two_c", 2, "--stop_after_epochs", "1")
    assert not (tmp / "two_c" / "checkpoint-1").exists() and (tmp / "two_c" / "checkpoint-0" / "state.json").exists()
    run_two_ranks(dataset, tmp / "two_c", 3, "--resume_from", str(tmp / "two_c" / "checkpoint-0"))
    same_files(tmp / "two_a", tmp / "two_c")
