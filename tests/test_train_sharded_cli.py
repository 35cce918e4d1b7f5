"""`torchrun -m vae_tagger_amd.train_decoder ... --sharded` end to end (GPU): two ranks that share GPU 0 over gloo (VT_CLI_GLOO=1; RCCL
needs one GPU per rank) against the one-process run, for the plain decoder and for the whole attention decoder with bucketing; and a
one-rank RCCL rehearsal (VT_CLI_ONE_RANK_GROUP=1) whose forced exchange runs export, all_gather_into_tensor and merge on the real
backend.  None of this yields a scaling figure.

The data set: 20 small PNG files and one broken file.  (13 files give ONE validation image -- max(1, int(0.1 n)) -- and a second rank
without a validation image is refused by --sharded itself; 21 entries are the fewest whose split leaves each of two ranks one.)  The
broken file sits in rank 1's training share, so rank 1 has one batch fewer than rank 0 and joins the last step of an epoch at weight 0."""
import contextlib
import io
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from vae_tagger_amd import synth, train_decoder
from vae_tagger_amd.train import batch_count, owned, split_indices

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_TAGS, SEED, EPOCHS, BS = 40, 42, 2, 2
SIZES = [(96, 64), (64, 64), (80, 120), (128, 128), (100, 70), (64, 96), (90, 90), (120, 80), (70, 100), (64, 80), (110, 110), (72, 64),
         (160, 96), (96, 160), (150, 150), (64, 128), (128, 64), (88, 132), (132, 88), (77, 77)]
FILES = {"best_pytorch_model.bin", "pytorch_model.bin", "training_history.json", "train_report.json", "optimal_thresholds.json",
         "evaluation_results.csv", "evaluation_results_overall.json"}
PLAIN = ["--no_attention"]
FULL = ["--train_front", "--use_cross_attention", "--train_cross_attention", "--use_bucketing", "--base_resolution", "64", "--max_resolution",
        "128", "--bucket_step", "64"]


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from PIL import Image
    from safetensors.torch import save_file
    root = tmp_path_factory.mktemp("train_sharded")
    g = torch.Generator().manual_seed(9)
    (root / "imgs").mkdir()
    tags = [f"tag_{i:03d}" for i in range(N_TAGS)]
    n = len(SIZES) + 1
    train_idx, val_idx = split_indices(n, SEED)
    broken = owned(train_idx, 1, 2)[1]                               # an entry of rank 1's training share
    data, sizes = {}, iter(SIZES)
    for i in range(n):
        path = str(root / "imgs" / ("broken.png" if i == broken else f"img{i:02d}.png"))
        if i == broken:
            open(path, "wb").write(b"not a png")
        else:
            w, h = next(sizes)
            arr = (torch.rand(h, w, 3, generator=g) * 255).to(torch.uint8).numpy()
            arr[: h // 2, : w // 3] = 40 + 9 * i
            Image.fromarray(arr).save(path)
        picks = [(3 * i + k) % N_TAGS for k in range(4 + i % 3)]
        data[path] = ", ".join(f"{tags[k]}:{0.5 + 0.5 * ((k + i) % 2)}" if k % 3 else tags[k] for k in picks)
    (root / "data.json").write_text(json.dumps(data))
    (root / "tags.csv").write_text("name\n" + "\n".join(tags) + "\n")
    save_file(synth.synth_state_dict(synth.encoder_manifest(), seed=0), str(root / "vae.safetensors"))
    torch.save(synth.synth_state_dict(synth.plain_decoder_manifest(N_TAGS), seed=3), root / "plain_start.pth")
    torch.save(synth.synth_state_dict(synth.attention_decoder_manifest(N_TAGS, 16, True, True, True), seed=3), root / "full_start.pth")
    common = ["--vae_checkpoint", str(root / "vae.safetensors"), "--tags_csv_path", str(root / "tags.csv"), "--json_path", str(root / "data.json"),
              "--resolution", "64", "--save_steps", "1", "--lr_warmup_steps", "2", "--logging_steps", "1", "--seed", str(SEED)]
    return {"root": root, "common": common, "train": len(train_idx), "val": len(val_idx)}


def argv(dataset, mode, out, epochs=EPOCHS, bs=BS):
    start = dataset["root"] / ("plain_start.pth" if mode is PLAIN else "full_start.pth")
    return dataset["common"] + mode + ["--decoder_checkpoint", str(start), "--output_dir", str(out), "--num_epochs", str(epochs),
                                       "--train_batch_size", str(bs)]


def run_plain(dataset, mode, out, **kw):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        train_decoder.main(argv(dataset, mode, out, **kw))
    return buf.getvalue(), json.loads((out / "train_report.json").read_text())


def env(**extra):
    return dict(os.environ, PYTHONDONTWRITEBYTECODE="1", HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT, **extra)


def run_two_ranks(dataset, mode, out, salt):
    port = str(29500 + (os.getpid() + 11 * salt) % 200)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", port,
           "-m", "vae_tagger_amd.train_decoder"] + argv(dataset, mode, out) + ["--sharded"]
    r = subprocess.run(cmd, env=env(VT_CLI_GLOO="1"), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=420)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return r.stdout.decode(), json.loads((out / "train_report.json").read_text())


def check_two_ranks(dataset, text, report, one_report, out, full):
    assert {f for f in os.listdir(out)} == FILES                     # every file once, nothing else
    assert text.count("训练完成") == 1 and text.count("训练和评估完成") == 1
    assert sum(1 for ln in text.splitlines() if ln.startswith("跳过图像")) == 1 and "broken.png" in text
    sh = report["sharded"]
    assert sh["world"] == 2 and sh["backend"] == "gloo"
    assert sh["state_sha256"][0] == sh["state_sha256"][1] and len(sh["state_sha256"][0]) == 64
    assert sh["train_images"] == [math.ceil(dataset["train"] / 2), dataset["train"] // 2] and sum(sh["train_images"]) == dataset["train"]
    assert report["train_images"] == one_report["train_images"] == dataset["train"] and report["val_images"] == dataset["val"]
    one_bytes = one_report["latent_cache"]["bytes_used"] if full else one_report["feature_cache_bytes"]
    print(f"cache bytes: one process {one_bytes}, ranks {sh['cache_bytes']}")
    assert all(0 < b < one_bytes for b in sh["cache_bytes"])
    steps = sh["steps_per_epoch"]
    assert len(steps) == EPOCHS and report["epochs"][-1]["optimizer_steps"] == sum(steps)
    assert [e["steps"] for e in report["epochs"]] == steps and [e["encoder_batches"] > 0 for e in report["epochs"]] == [True, False]
    readable = [sh["train_images"][0], sh["train_images"][1] - 1]    # the broken file is rank 1's
    if full:
        assert all(s >= batch_count(max(readable), BS) for s in steps)           # (batches of one latent shape: at least these)
    else:
        assert steps == [max(batch_count(n, BS) for n in readable)] * EPOCHS
        assert batch_count(readable[1], BS) < steps[0]               # rank 1 joined the last step of each epoch at weight 0
    history = json.loads((out / "training_history.json").read_text())
    assert sorted(history) == ["learning_rates", "train_loss", "val_loss"]
    assert all(len(v) == EPOCHS and all(math.isfinite(x) for x in v) for v in history.values())
    saved = torch.load(out / "pytorch_model.bin", map_location="cpu")
    assert all(torch.isfinite(v.float()).all() for v in saved.values())


def test_two_ranks_train_the_plain_decoder(dataset):
    root = dataset["root"]
    _, one_report = run_plain(dataset, PLAIN, root / "plain_one")
    text, report = run_two_ranks(dataset, PLAIN, root / "plain_two", 0)
    check_two_ranks(dataset, text, report, one_report, root / "plain_two", full=False)
    start = torch.load(root / "plain_start.pth", map_location="cpu")
    saved = torch.load(root / "plain_two" / "pytorch_model.bin", map_location="cpu")
    assert set(saved) == set(start) and not torch.equal(saved["classifier.8.weight"], start["classifier.8.weight"])


def test_two_ranks_train_the_whole_attention_decoder_with_bucketing(dataset):
    root = dataset["root"]
    _, one_report = run_plain(dataset, FULL, root / "full_one")
    text, report = run_two_ranks(dataset, FULL, root / "full_two", 1)
    check_two_ranks(dataset, text, report, one_report, root / "full_two", full=True)
    start = torch.load(root / "full_start.pth", map_location="cpu")
    saved = torch.load(root / "full_two" / "pytorch_model.bin", map_location="cpu")
    assert list(saved) == list(start)
    for k in ("classifier.12.weight", "feature_compress.0.weight", "cross_attention.q_proj.weight", "feature_compress.1.running_mean"):
        assert not torch.equal(saved[k], start[k]), k
    # rank 0's BatchNorm buffers are the ones saved: one training-mode forward per step it had a batch for
    tracked = int(saved["feature_compress.1.num_batches_tracked"]) - int(start["feature_compress.1.num_batches_tracked"])
    assert 0 < tracked <= sum(report["sharded"]["steps_per_epoch"])


def test_one_rank_rccl_rehearsal_starts_where_the_plain_run_starts(dataset):
    """One epoch of ONE step (the batch holds the whole training set), so training_history.json's train_loss IS the first step's loss,
    at full precision: the forced exchange (export, all_gather_into_tensor on RCCL, merge of K = 1 at weight 1) leaves the gradients'
    bits, and the loss of the first step is taken before any of it.  The plain run, started twice, gives the same checkpoints."""
    root = dataset["root"]
    big = dataset["train"] + 5
    run_plain(dataset, PLAIN, root / "one_a", epochs=1, bs=big)
    run_plain(dataset, PLAIN, root / "one_b", epochs=1, bs=big)
    for f in ("best_pytorch_model.bin", "pytorch_model.bin"):
        a, b = (torch.load(root / d / f, map_location="cpu") for d in ("one_a", "one_b"))
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a), f
    assert (root / "one_a" / "training_history.json").read_text() == (root / "one_b" / "training_history.json").read_text()
    out = root / "rehearsal"
    cmd = [sys.executable, "-m", "vae_tagger_amd.train_decoder"] + argv(dataset, PLAIN, out, epochs=1, bs=big) + ["--sharded"]
    r = subprocess.run(cmd, env=env(VT_CLI_ONE_RANK_GROUP="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29750 + os.getpid() % 40)), cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    report = json.loads((out / "train_report.json").read_text())
    assert report["sharded"]["world"] == 1 and report["sharded"]["backend"] == "nccl" and report["sharded"]["steps_per_epoch"] == [1]
    plain, rehearsal = (json.loads((root / d / "training_history.json").read_text()) for d in ("one_a", "rehearsal"))
    print(f"first step loss: plain {plain['train_loss'][0]!r}, one-rank sharded {rehearsal['train_loss'][0]!r}")
    assert rehearsal["train_loss"][0] == plain["train_loss"][0]
    assert {f for f in os.listdir(out)} == FILES and r.stdout.decode().count("训练完成") == 1
