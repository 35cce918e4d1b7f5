"""Sharded data-set evaluation: `--sharded` of the evaluate CLI and evaluation.merge_across_ranks.  CPU: the flag, the refusals and the
shard assignment.  GPU: two ranks (sharing GPU 0, gloo) against the one-process run, file by file, and the merge's collectives on a
one-rank RCCL group -- that one shows the calls execute on RCCL; no scaling figure follows from it."""
import json
import os
import subprocess
import sys

import pytest
import torch

from vae_tagger_amd import evaluate, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--vae_checkpoint", "v", "--decoder_checkpoint", "d", "--json_path", "j", "--tags_csv_path", "t"]


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
def test_cli_parser_has_sharded():
    flags = {o for a in evaluate.build_parser(distributed=True)._actions for o in a.option_strings}
    assert "--sharded" in flags
    assert flags - {"--sharded"} == {o for a in evaluate.build_parser()._actions for o in a.option_strings}
    a = evaluate.build_parser(distributed=True).parse_args(BASE)
    assert a.sharded is False
    assert evaluate.build_parser(distributed=True).parse_args(BASE + ["--sharded"]).sharded is True


def test_sharded_with_host_metrics_is_refused_before_any_gpu_or_group_work(monkeypatch):
    import torch.distributed as dist
    from vae_tagger_amd import infer_full

    def never(*a, **k):
        raise AssertionError("reached GPU / process-group work")
    monkeypatch.setattr(infer_full, "_dist_setup", never)
    monkeypatch.setattr(infer_full, "load_models", never)
    monkeypatch.setattr(dist, "init_process_group", never)
    monkeypatch.setattr(torch.cuda, "is_available", never)
    for world in ("1", "2"):
        monkeypatch.setenv("WORLD_SIZE", world)
        args = evaluate.build_parser(distributed=True).parse_args(BASE + ["--sharded", "--host_metrics"])
        with pytest.raises(RuntimeError, match="host_metrics"):
            evaluate.evaluate(args)
    # without --sharded more than one rank is still refused, and the message names the flag
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="single process.*--sharded"):
        evaluate.evaluate(evaluate.build_parser(distributed=True).parse_args(BASE))


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [0, 1, 5, 25])
def test_shard_paths_partition_the_list(world, n):
    paths = [f"img{i}.png" for i in range(n)]
    shares = [evaluate.shard_paths(paths, r, world) for r in range(world)]
    assert all(s == paths[r::world] for r, s in enumerate(shares))
    assert sorted(p for s in shares for p in s) == sorted(paths) and sum(len(s) for s in shares) == n
    assert max(len(s) for s in shares) - min(len(s) for s in shares) <= 1
    if n < world:
        assert sum(1 for s in shares if not s) == world - n


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
N_TAGS = 40
SIZES = [(200, 150), (128, 128), (90, 160), (300, 300), (256, 128), (130, 250), (640, 480), (100, 100), (192, 256), (333, 222),
         (150, 200), (257, 255), (512, 256), (64, 128), (240, 180), (180, 240), (1000, 700), (129, 127), (300, 150), (210, 140),
         (140, 210), (97, 193), (256, 256), (400, 300)]
COUNT_KEYS = ("accuracy", "hamming_loss", "precision_micro", "precision_macro", "precision_weighted", "recall_micro", "recall_macro",
              "recall_weighted", "f1_micro", "f1_macro", "f1_weighted")
AP_KEYS = ("mAP", "mAP_micro", "mAP_weighted")
AP_TOL = 1e-9


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """24 PNG files of assorted sizes + one broken file, the training JSON, a tag CSV and synthetic checkpoints."""
    from PIL import Image
    from safetensors.torch import save_file
    root = tmp_path_factory.mktemp("sharded")
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
    return {"root": root,
            "argv": ["--vae_checkpoint", str(root / "vae.safetensors"), "--decoder_checkpoint", str(root / "dec.pth"), "--json_path",
                     str(root / "data.json"), "--tags_csv_path", str(root / "tags.csv"), "--resolution", "128", "--use_bucketing",
                     "--base_resolution", "128", "--max_resolution", "256", "--bucket_step", "64", "--batch_size", "4"]}


def _read_outputs(d, with_thresholds):
    rows = [line.split(",") for line in (d / "evaluation_results.csv").read_text().strip().split("\n")]
    assert rows[0] == ["class_name", "precision", "recall", "f1", "ap", "support"]
    per_class = {r[0]: {"precision": float(r[1]), "recall": float(r[2]), "f1": float(r[3]), "ap": float(r[4]), "support": int(r[5])} for r in rows[1:]}
    overall = json.loads((d / "evaluation_results_overall.json").read_text())
    thr = json.loads((d / "optimal_thresholds.json").read_text()) if with_thresholds else None
    return thr, overall, per_class


def _same_files(got_dir, want_dir, with_thresholds):
    """Field for field: the thresholds and every count-derived field exactly, the AP fields within 1e-9."""
    (gt, go, gp), (wt, wo, wp) = _read_outputs(got_dir, with_thresholds), _read_outputs(want_dir, with_thresholds)
    assert gt == wt
    assert list(go) == list(wo) and set(go) == set(COUNT_KEYS + AP_KEYS)
    for k in COUNT_KEYS:
        assert go[k] == wo[k], (k, go[k], wo[k])
    for k in AP_KEYS:
        print(f"{k}: sharded {go[k]!r} one process {wo[k]!r}")
        assert abs(go[k] - wo[k]) <= AP_TOL, (k, go[k], wo[k])
    assert list(gp) == list(wp)
    for name, w in wp.items():
        g = gp[name]
        assert (g["precision"], g["recall"], g["f1"], g["support"]) == (w["precision"], w["recall"], w["f1"], w["support"]), name
        assert abs(g["ap"] - w["ap"]) <= AP_TOL, name


@pytest.mark.gpu
def test_sharded_cli_two_ranks_equal_the_one_process_run(dataset):
    """`torchrun --nproc-per-node 2 -m vae_tagger_amd.evaluate ... --sharded`: both ranks share GPU 0 here, so the exchanges run on gloo
    (VT_CLI_GLOO=1; RCCL needs one GPU per rank).  Once with the threshold search (two passes, two merges), once with --threshold.
    The batches of a rank differ from the one-process run's: exact equality of the counts rests on the batch-composition invariance
    of the encode + tag path, as the one-process end-to-end test does for this fixture."""
    root = dataset["root"]
    one = evaluate.main(dataset["argv"] + ["--output_dir", str(root / "one")])
    assert one["skipped"] == 1
    one_thr = evaluate.main(dataset["argv"] + ["--output_dir", str(root / "one_thr"), "--threshold", "0.35"])
    assert one_thr["optimal_thresholds"] is None
    env = dict(os.environ, VT_CLI_GLOO="1", PYTHONDONTWRITEBYTECODE="1", HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT)
    for k, (extra, want_dir, search) in enumerate(((["--output_dir", str(root / "two")], root / "one", True),
                                                   (["--output_dir", str(root / "two_thr"), "--threshold", "0.35"], root / "one_thr", False))):
        port = str(29300 + (os.getpid() + 7 * k) % 200)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
               "--master-port", port, "-m", "vae_tagger_amd.evaluate"] + dataset["argv"] + extra + ["--sharded"]
        r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=420)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        out = r.stdout.decode()
        got_dir = root / ("two" if search else "two_thr")
        assert (got_dir / "optimal_thresholds.json").exists() == search
        _same_files(got_dir, want_dir, search)
        assert out.count("评估完成") == 1 and f"图像: {len(SIZES)}, 跳过: 1," in out          # rank 0 alone closes; the broken file once
        assert sum(1 for ln in out.splitlines() if ln.startswith("跳过图像")) == 1 and "broken.png" in out
        if search:
            thr = json.loads((got_dir / "optimal_thresholds.json").read_text())["global_threshold"]
            assert thr == one["threshold"] and f"阈值: {thr:.3f}" in out


@pytest.mark.gpu
def test_merge_across_ranks_runs_on_a_one_rank_rccl_group(tmp_path):
    """A child process creates a ONE-rank "nccl" (= RCCL) group on cuda:0 before any other GPU call and runs
    merge_across_ranks(..., force_collective=True): the descriptor all_gather_object and the block all_gather_into_tensor execute on
    RCCL, and the merged evaluator's metrics equal the un-merged one's.  It proves the collectives run; it says NOTHING about scaling."""
    script = tmp_path / "merge_one_rank.py"
    script.write_text(
        "import os, sys\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "import torch, torch.distributed as dist\n"
        "dev = torch.device('cuda', 0)\n"
        "dist.init_process_group('nccl', world_size=1, rank=0, device_id=dev)\n"
        "torch.cuda.set_device(dev)\n"
        "from vae_tagger_amd import evaluation\n"
        "assert dist.get_backend() == 'nccl'\n"
        "g = torch.Generator().manual_seed(3)\n"
        "n, c = 1500, 101\n"
        "p = (torch.rand(n, c, generator=g) * 16).round() / 16\n"
        "y = (torch.rand(n, c, generator=g) < 0.3).float()\n"
        "names = [f'tag_{i:05d}' for i in range(c)]\n"
        "ev = evaluation.DeviceMultiLabelEvaluator(names, dev, threshold=0.4)\n"
        "for lo in range(0, n, 256):\n"
        "    ev.update(p[lo:lo + 256].cuda(), y[lo:lo + 256].cuda())\n"
        "merged = evaluation.merge_across_ranks(ev, dist.group.WORLD, force_collective=True)\n"
        "assert merged is not None and merged is not ev and merged.n_seen == n and merged.capacity == n\n"
        "try:\n"
        "    evaluation.merge_across_ranks(ev, dist.group.WORLD, force_collective=True, error='FloatingPointError: planted')\n"
        "    raise SystemExit('an error on a rank did not raise')\n"
        "except RuntimeError as e:\n"
        "    assert 'rank 0: FloatingPointError: planted' in str(e)\n"
        "a, b = merged.compute_metrics(), ev.compute_metrics()\n"
        "assert a == b and a['mAP'] > 0, 'merged metrics differ'\n"
        "assert merged.optimal_thresholds() == ev.optimal_thresholds()\n"
        "dist.barrier()\n"
        "torch.cuda.synchronize()\n"
        "print('MERGE_RCCL_OK', torch.cuda.nccl.version(), a['mAP'])\n"
        "dist.destroy_process_group()\n")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29900 + os.getpid() % 40), PYTHONDONTWRITEBYTECODE="1",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, str(script)], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0 and b"MERGE_RCCL_OK" in r.stdout, (r.stdout.decode()[-500:], r.stderr.decode()[-2000:])
    print(r.stdout.decode().strip())
