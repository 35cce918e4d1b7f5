"""Sharded decoder training, the parts that need no GPU: the host definition of the gradient merge, static ownership and the agreed step
count, the --sharded flag and its refusals (raised before any GPU or process-group work), and the new entries of the C ABI."""
import json
import os
import re

import numpy as np
import pytest
import torch

from vae_tagger_amd import _lib, train_decoder
from vae_tagger_amd.train import (agreed_steps, batch_count, epoch_order, exchange_weights, merge_gradients_host, owned)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--vae_checkpoint", "v", "--json_path", "j", "--tags_csv_path", "t", "--no_attention"]
NEW_SYMBOLS = tuple(f"vt_{block}_grads_{what}" for block in ("head", "front", "cross") for what in ("floats", "export", "merge"))


# ---- the merge's arithmetic ----------------------------------------------------------------------------------------------------------
def plain_loop(blocks, weights):
    """Python floats are fp64: acc = acc + w * x rounds the product, then the sum; one cast at the end."""
    out = np.empty(len(blocks[0]), dtype=np.float32)
    for e in range(len(blocks[0])):
        acc = 0.0
        for r in range(len(blocks)):
            prod = float(weights[r]) * float(blocks[r][e])
            acc = acc + prod
        out[e] = np.float32(acc)
    return out


@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_merge_gradients_host_is_the_plain_loop(K):
    g = np.random.default_rng(K)
    blocks = (g.standard_normal((K, 257)) * 10.0 ** g.integers(-6, 7, (K, 257))).astype(np.float32)
    blocks[:, ::19] = 0.0
    blocks[0, 5], blocks[K - 1, 5] = 1e30, -1e30                      # a cancellation: the order of the sum shows
    counts = [7] if K == 1 else ([3, 0, 4, 1, 5, 2, 6, 8][:K])
    w = exchange_weights(counts)
    got = merge_gradients_host(blocks, w)
    assert got.dtype == np.float32 and got.shape == (257,)
    assert np.array_equal(got.view(np.uint32), plain_loop(blocks, w).view(np.uint32))
    assert np.array_equal(merge_gradients_host(list(blocks), w).view(np.uint32), got.view(np.uint32))


def test_one_rank_at_weight_one_returns_the_inputs_bits():
    g = np.random.default_rng(0)
    x = g.standard_normal(300).astype(np.float32)
    x[:4] = [0.0, -0.0, np.float32(1e-45), np.float32(3.4e38)]
    got = merge_gradients_host(x[None], [1.0])
    want = x.copy()
    want[1] = 0.0                                                     # 0.0 + 1.0 * -0.0 is +0.0, on the device as here
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert exchange_weights([5]) == [1.0] and exchange_weights([3, 0, 1]) == [0.75, 0.0, 0.25]
    with pytest.raises(ValueError):
        exchange_weights([0, 0])
    with pytest.raises(ValueError):
        merge_gradients_host(x[None], [0.5, 0.5])


def test_weights_make_the_merge_the_concatenated_batchs_mean():
    """Per-rank batch means weighted by n_r / sum n are the mean over the concatenated batch, ragged last batches included."""
    g = np.random.default_rng(4)
    rows = g.standard_normal((9, 33))
    counts = [4, 2, 0, 3]
    means, lo = [], 0
    for n in counts:
        means.append(rows[lo:lo + n].mean(axis=0) if n else np.zeros(33))
        lo += n
    got = merge_gradients_host(np.asarray(means, dtype=np.float32), exchange_weights(counts))
    assert np.allclose(got, rows.mean(axis=0), rtol=2e-6, atol=2e-7)


# ---- ownership and the agreed step count ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [4, 5, 25])
def test_ownership_partitions_the_list(world, n):
    paths = [f"img{i}.png" for i in range(n)]
    shares = [owned(paths, r, world) for r in range(world)]
    assert all(s == paths[r::world] for r, s in enumerate(shares))
    assert sorted(p for s in shares for p in s) == sorted(paths) and sum(len(s) for s in shares) == n
    assert max(len(s) for s in shares) - min(len(s) for s in shares) <= 1
    assert min(len(s) for s in shares) == n // world == len(shares[-1])          # what check_shares looks at
    for r, s in enumerate(shares):                                               # a rank's epoch order is a permutation of ITS share
        assert sorted(epoch_order(len(s), 42, 1)) == list(range(len(s)))


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [4, 5, 25])
@pytest.mark.parametrize("bs", [1, 2, 4])
def test_agreed_steps_is_the_largest_local_batch_count(world, n, bs):
    local = [batch_count(len(owned(range(n), r, world)), bs) for r in range(world)]
    assert agreed_steps(local) == max(local) == batch_count(-(-n // world), bs)
    assert all(c == len(range(0, len(owned(range(n), r, world)), bs)) for r, c in enumerate(local))


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------------
def test_sharded_exists_only_in_the_distributed_parser():
    plain = {o for a in train_decoder.build_parser()._actions for o in a.option_strings}
    dist_flags = {o for a in train_decoder.build_parser(distributed=True)._actions for o in a.option_strings}
    assert "--sharded" not in plain and dist_flags - {"--sharded"} == plain
    assert train_decoder.build_parser(distributed=True).parse_args(BASE).sharded is False
    assert train_decoder.build_parser(distributed=True).parse_args(BASE + ["--sharded"]).sharded is True
    with pytest.raises(SystemExit):
        train_decoder.build_parser().parse_args(BASE + ["--sharded"])
    # a namespace of the single-process parser passes check_args as before
    assert train_decoder.check_args(train_decoder.build_parser().parse_args(BASE)).use_attention is False


@pytest.fixture()
def no_gpu_or_group_work(monkeypatch):
    import torch.distributed as dist
    from vae_tagger_amd import infer_full

    def never(*a, **k):
        raise AssertionError("reached GPU / process-group work")
    monkeypatch.setattr(infer_full, "_dist_setup", never)
    monkeypatch.setattr(dist, "init_process_group", never)
    monkeypatch.setattr(torch.cuda, "is_available", never)
    monkeypatch.setattr(train_decoder, "_load_models", never)


def test_sharded_with_gradient_accumulation_is_refused_first(no_gpu_or_group_work, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match=r"--sharded.*--gradient_accumulation_steps"):
        train_decoder.main(BASE + ["--sharded", "--gradient_accumulation_steps", "2"])
    with pytest.raises(SystemExit, match=r"--sharded.*--no_feature_cache"):
        train_decoder.main(BASE + ["--sharded", "--no_feature_cache"])


def _listing(tmp_path, n):
    imgs = []
    for i in range(n):
        p = tmp_path / f"img{i:02d}.png"
        p.write_bytes(b"x")                                          # (only its existence is looked at before the refusal)
        imgs.append(str(p))
    (tmp_path / "data.json").write_text(json.dumps({p: "tag_a" for p in imgs}))
    (tmp_path / "tags.csv").write_text("name\ntag_a\ntag_b\n")
    return ["--vae_checkpoint", "v", "--json_path", str(tmp_path / "data.json"), "--tags_csv_path", str(tmp_path / "tags.csv"), "--no_attention",
            "--sharded"]


@pytest.mark.parametrize("n,world,what", [(13, 2, "0 validation"), (25, 8, "0 validation"), (21, 8, "0 validation"), (4, 2, "1 training")])
def test_sharded_shares_too_small_are_refused_before_any_gpu_or_group_work(no_gpu_or_group_work, monkeypatch, tmp_path, n, world, what):
    monkeypatch.setenv("WORLD_SIZE", str(world))
    with pytest.raises(RuntimeError, match=rf"--sharded over {world} ranks.*{what}"):
        train_decoder.main(_listing(tmp_path, n))


def test_check_shares():
    train_decoder.check_shares(19, 2, 2)
    train_decoder.check_shares(2, 1, 1)
    for bad in ((19, 2, 3), (3, 2, 2), (100, 7, 8)):
        with pytest.raises(RuntimeError, match="--sharded"):
            train_decoder.check_shares(*bad)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "vae_tagger_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.PROTOTYPES, name
    for block in ("head", "front", "cross"):
        assert _lib.PROTOTYPES[f"vt_{block}_grads_floats"][0] is _lib._sz
        assert len(_lib.PROTOTYPES[f"vt_{block}_grads_export"][1]) == 6 and len(_lib.PROTOTYPES[f"vt_{block}_grads_merge"][1]) == 8
        assert _lib.PROTOTYPES[f"vt_{block}_grads_merge"] == _lib.PROTOTYPES["vt_head_grads_merge"]
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in NEW_SYMBOLS)
    # the partition of P behind the squared-norm partials is written once, in vt_train.h
    common = open(os.path.join(ROOT, "vae_tagger_amd", "csrc", "vt_train.h")).read()
    assert common.count("inline long long vt_train_merge_chunk4(") == 1
