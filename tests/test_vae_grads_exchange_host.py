"""train_vae --sharded on the host: the batch's shards and their weights, the owners' ranges, the numpy mirror of the merge, the flag and its
refusal, the two new entries of the C ABI (header, _lib.PROTOTYPES, the built library), and the objective a sharded step optimises --
sum_r w_r L_r is the concatenated batch's loss with kl = 0 and is NOT under the KL term, in fp64 autograd on the CPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from vae_tagger_amd import _lib, train_vae
from vae_tagger_amd.train import merge_gradients_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = train_vae.TILE
REQUIRED = ["--json_path", "j", "--tags_csv_path", "t"]


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("B", [1, 2, 3])
def test_shards_cover_every_position_once_and_weights_sum_to_one(world, B):
    order = list(range(100, 100 + 5 * B * world + 1))                           # five full global batches and the ragged ones below
    empty_seen = False
    for n_last in range(1, B * world + 1):                                      # every length of a ragged last batch
        for _, batch in train_vae.plan_train_batches(order[:4 * B * world + n_last], B * world):
            shards = [train_vae.shard_of_batch(batch, r, world, B) for r in range(world)]
            assert [i for s in shards for i in s] == batch                      # contiguous, in rank order, each position exactly once
            assert all(len(s) <= B for s in shards)
            w = train_vae.shard_weights(len(batch), world, B)
            assert w == [len(s) / len(batch) for s in shards] and abs(sum(w) - 1.0) <= 1e-15 and w[0] > 0
            empty_seen |= any(not s for s in shards)
    assert empty_seen == (world > 1)                                            # ranks with an empty slice were among the cases
    with pytest.raises(ValueError):
        train_vae.shard_weights(B * world + 1, world, B)
    with pytest.raises(ValueError):
        train_vae.shard_of_batch([1, 2], world, world, B)


@pytest.mark.parametrize("tiles, world", [(1, 1), (7, 2), (7, 3), (20505, 8), (5, 8), (64, 64)])
def test_owner_ranges_tile_the_padded_row(tiles, world):
    S, row = train_vae.owner_split(tiles * TILE, world)
    assert S == -(-tiles // world) and row == world * S * TILE and row >= tiles * TILE and row - tiles * TILE < world * TILE
    ranges = [(r * S, (r + 1) * S) for r in range(world)]
    assert ranges[0][0] == 0 and ranges[-1][1] == world * S and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    with pytest.raises(ValueError):
        train_vae.owner_split(tiles * TILE, 65)
    with pytest.raises(ValueError):
        train_vae.owner_split(tiles * TILE + 4, world)


def test_merge_rows_host_is_the_identity_at_one_rank_and_the_decoders_merge_otherwise():
    x = np.array([-0.0, 0.0, 1e-45, -1e-45, 1.1754942e-38, -5.877e-39, 1.0, -3.5, 3.4028235e38, 1e-30], dtype=np.float32)
    assert np.signbit(x[0]) and x[2] != 0 and abs(x[4]) < np.finfo(np.float32).tiny
    out = train_vae.merge_rows_host([x], [1.0])
    assert out.dtype == np.float32 and out.tobytes() == x.tobytes()
    assert merge_gradients_host([x], [1.0]).tobytes() != x.tobytes()            # (0.0 + -0.0 is +0.0: why the first term is not added to 0.0)
    rng = np.random.default_rng(3)
    rows = [(rng.standard_normal(1000) * 10.0 ** rng.integers(-6, 6)).astype(np.float32) for _ in range(5)]
    w = [1 / 6, 2 / 6, 0.0, 3 / 6, 0.0]
    got = train_vae.merge_rows_host(rows, w)
    assert got.tobytes() == merge_gradients_host(rows, w).tobytes()             # on numbers other than -0.0 the two agree bit for bit
    acc = np.float64(w[0]) * rows[0].astype(np.float64)
    for r in range(1, 5):
        acc = acc + np.float64(w[r]) * rows[r].astype(np.float64)
    assert got.tobytes() == acc.astype(np.float32).tobytes()
    with pytest.raises(ValueError):
        train_vae.merge_rows_host(rows, w[:4])


def test_the_flag_and_its_refusals(monkeypatch):
    assert train_vae.build_parser().parse_args(REQUIRED).sharded is False
    args = train_vae.build_parser().parse_args(REQUIRED + ["--sharded"])
    assert args.sharded is True
    for k in ("WORLD_SIZE", "VT_CLI_ONE_RANK_GROUP"):
        monkeypatch.delenv(k, raising=False)
    with pytest.raises(SystemExit, match=re.escape("--sharded")):                # no process group: refused before any device work
        train_vae.main(REQUIRED + ["--sharded"])
    with pytest.raises(SystemExit, match=re.escape("--sharded")):
        train_vae.check_sharded(args, {"WORLD_SIZE": "65"})
    train_vae.check_sharded(args, {"WORLD_SIZE": "64"})
    train_vae.check_sharded(args, {"VT_CLI_ONE_RANK_GROUP": "1"})
    train_vae.check_sharded(train_vae.build_parser().parse_args(REQUIRED), {})


def _header_argument_count(header, name):
    m = re.search(r"\b" + name + r"\s*\(", header)
    assert m, f"{name} is not declared in the header"
    depth, i = 1, m.end()
    while depth:
        depth += {"(": 1, ")": -1}.get(header[i], 0)
        i += 1
    body = re.sub(r"/\*.*?\*/", "", header[m.end():i - 1], flags=re.S)
    return len([a for a in body.split(",") if a.strip()])


def test_the_two_new_entries_in_header_prototypes_and_library():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "vae_tagger_hip.h")).read()
    for name, count in (("vt_vae_grads_export", 8), ("vt_vae_grads_merge", 9)):
        res, args = _lib.PROTOTYPES[name]
        declared = [m.start() for m in re.finditer(r"\bint " + name + r"\(", header)]          # (the comment above names the entry without a type)
        assert len(declared) == 1, name
        assert _header_argument_count(header[declared[0]:], name) == len(args) == count, name
        fn = getattr(lib, name)
        assert fn.restype == res == ctypes.c_int and list(fn.argtypes) == list(args), name
    one = (ctypes.c_longlong * 1)(4)
    assert lib.vt_vae_grads_export(None, None, one, 1, None, TILE, 0, None) == 1                 # no context
    assert lib.vt_vae_grads_merge(None, None, TILE, 1, (ctypes.c_double * 1)(1.0), 0, TILE, None, None) == 1


def test_the_objective_is_the_concatenated_batch_only_without_the_kl_term():
    """fp64 autograd of the plain step (tests/_vae_train_step_ref.step_autograd) on the small 2 x 16 x 24 case; the eps rows of the two images are
    what the device draws for the global indices FIRST and FIRST + 1 whichever rank holds the image, here any fixed draw.  Two ranks at batch 1
    have weights (1/2, 1/2): with kl = 0 the merged gradient is the batch-2 gradient (MSE and the triplet term are batch means), with kl = 1e-2
    it is not, because log(1 + mean KL / 10000) is taken per rank."""
    from _vae_model_backward_ref import rel
    from _vae_train_step_ref import CASES, LATENT, MARGIN, N_LABELS, SIM, step_autograd
    from vae_tagger_amd import synth
    cfg, B, H, W = CASES["small-2x16x24"]
    assert B == 2
    p = {k: v.double() for k, v in synth.synth_state_dict({**synth.encoder_manifest(**cfg), **synth.image_decoder_manifest(**cfg)}, seed=5).items()}
    images = synth.synth_images(3 * B, H, W, seed=6).double()
    g = torch.Generator().manual_seed(8)
    labels = tuple((torch.rand(B, N_LABELS, generator=g) < 0.5).double() for _ in range(2))
    labels[0][:, 0] = 1.0
    nb = len(cfg["block_out"]) - 1
    eps = [torch.randn(B, LATENT, H >> nb, W >> nb, generator=g, dtype=torch.float64) for _ in range(4)]
    one = lambda i: (images[[i, B + i, 2 * B + i]], [e[i:i + 1] for e in eps], tuple(y[i:i + 1] for y in labels))
    different = {}
    for kl in (0.0, 1e-2):
        weights = {"reconstruction": 1.0, "kl": kl, "triplet": 1.0}
        losses, both = step_autograd(p, images, eps, labels, weights, MARGIN, SIM)
        parts = [step_autograd(p, *one(i), weights, MARGIN, SIM) for i in range(B)]
        assert float(losses["triplet"]) > 0.0, "the case must have an active triplet"
        worst = {}
        for k in p:
            merged = 0.5 * parts[0][1][k] + 0.5 * parts[1][1][k]
            worst[k] = rel(merged, both, k)                                      # (to_k.bias, whose exact gradient is zero, on to_q.bias's scale)
        different[kl] = [k for k, d in worst.items() if d > 1e-10]
        print(f"kl = {kl}: largest relative distance {max(worst.values()):.3e}, {len(different[kl])} of {len(p)} tensors beyond 1e-10")
    assert different[0.0] == []
    assert any(k.startswith("encoder.") for k in different[1e-2])
