"""No GPU: the --train_front surface of train_decoder (parsing, refusals), train.LatentCache on CPU tensors (indexing, grouping by
latent shape, the memory rule), the exported key set, and the C ABI's new entries in the header and the ctypes table."""
import os
import re

import pytest
import torch

from vae_tagger_amd import _lib, synth, train, train_decoder

BASE = ["--vae_checkpoint", "ae.safetensors", "--json_path", "data.json", "--tags_csv_path", "tags.csv"]
NEW_SYMBOLS = ("vt_front_state_bytes", "vt_front_workspace_bytes", "vt_front_init", "vt_front_forward", "vt_front_backward", "vt_front_step",
               "vt_front_commit", "vt_front_read", "vt_front_write", "vt_head_forward_backward_dx", "vt_train_clip")


def parse(*extra):
    return train_decoder.check_args(train_decoder.build_parser().parse_args(BASE + list(extra)))


def test_train_front_parses_and_passes_the_checks():
    args = parse("--train_front", "--attention_dropout", "0.2", "--latent_cache_gb", "0.5", "--attention_heads", "2")
    assert args.train_front and not args.freeze_front and args.use_attention
    assert args.attention_dropout == 0.2 and args.latent_cache_gb == 0.5
    assert train_decoder.build_parser().parse_args(BASE).latent_cache_gb == 16.0
    assert not parse("--freeze_front").train_front and not parse("--no_attention").train_front


def test_attention_decoder_with_neither_flag_is_still_refused():
    for extra in ([], ["--use_cross_attention"], ["--latent_cache_gb", "4"]):
        with pytest.raises(RuntimeError, match="front.*not implemented"):
            parse(*extra)
    assert "--train_front" in train_decoder.FRONT_MESSAGE


@pytest.mark.parametrize("extra,match", [(["--use_cross_attention"], "cross-attention is not implemented"), (["--no_attention"], "no_attention"),
                                         (["--freeze_front"], "exclude"), (["--attention_heads", "3"], "attention_heads"),
                                         (["--attention_dropout", "1.0"], "attention_dropout"), (["--latent_cache_gb", "-1"], "latent_cache_gb")])
def test_train_front_refusals(extra, match):
    with pytest.raises(RuntimeError, match=match):
        parse("--train_front", *extra)
    with pytest.raises(SystemExit, match=match):                    # and main() refuses before it touches a file
        train_decoder.main(BASE + ["--train_front", "--output_dir", os.path.join(os.sep, "nonexistent", "out")] + extra)


def test_cross_attention_is_allowed_with_freeze_front_only():
    assert parse("--freeze_front", "--use_cross_attention").use_cross_attention


# ---- LatentCache -----------------------------------------------------------------------------------------------------------------------
def filled_cache():
    g = torch.Generator().manual_seed(0)
    cache = train.LatentCache(7, 16 * 4 * 5, 3, "cpu")
    lat = {"a": torch.randn(2, 16, 2, 3, generator=g), "b": torch.randn(3, 16, 4, 5, generator=g), "c": torch.randn(1, 16, 2, 3, generator=g)}
    lab = {k: torch.rand(v.shape[0], 3, generator=g) for k, v in lat.items()}
    cache.put(["a0", "a1"], lat["a"], lab["a"])
    cache.put(["b0", "b1", "b2"], lat["b"], lab["b"])
    cache.put(["c0"], lat["c"], lab["c"])
    return cache, lat, lab


def test_latent_cache_indexing():
    cache, lat, lab = filled_cache()
    assert len(cache) == 6 and "b1" in cache and "zz" not in cache
    assert cache.shape("a1") == (2, 3) and cache.shape("b0") == (4, 5)
    got, y = cache.gather(["c0", "a1", "a0"])
    assert torch.equal(got, torch.cat([lat["c"], lat["a"].flip(0)])) and torch.equal(y, torch.cat([lab["c"], lab["a"].flip(0)]))
    got, y = cache.gather(["b2", "b0"])
    assert torch.equal(got, lat["b"][[2, 0]]) and torch.equal(y, lab["b"][[2, 0]])
    assert cache.used == 3 * 96 + 3 * 320 and cache.nbytes == cache.used * 4 + 6 * 3 * 4
    with pytest.raises(ValueError, match="one latent shape"):
        cache.gather(["a0", "b0"])
    # a second put of a key overwrites in place; another shape under the same key is an error
    cache.put(["a0"], lat["a"][1:], lab["a"][1:])
    assert torch.equal(cache.gather(["a0"])[0], lat["a"][1:]) and cache.used == 3 * 96 + 3 * 320
    with pytest.raises(ValueError, match="was stored as"):
        cache.put(["a0"], lat["b"][:1], lab["b"][:1])
    cache.put(["d0"], lat["c"], lab["c"])
    with pytest.raises(IndexError):
        cache.put(["e0"], lat["c"], lab["c"])
    with pytest.raises(ValueError, match="exceeds"):
        train.LatentCache(2, 10, 3, "cpu").put(["x"], lat["c"], lab["c"])


def test_latent_cache_groups_an_epoch_order_by_latent_shape():
    cache, _, _ = filled_cache()
    order = ["b1", "a0", "missing", "b0", "c0", "a1", "b2"]
    batches = cache.batches(order, 2)
    assert batches == [["b1", "b0"], ["a0", "c0"], ["a1"], ["b2"]]          # full groups leave at once; the rest oldest first
    assert all(len({cache.shape(k) for k in b}) == 1 and len(b) <= 2 for b in batches)
    assert sorted(k for b in batches for k in b) == sorted(k for k in order if k in cache)
    assert cache.batches(order, 8) == [["b1", "b0", "b2"], ["a0", "c0", "a1"]]


def test_latent_cache_memory_rule():
    per_image = 16 * 128 * 128 * 4                                          # a 1024 x 1024 image: 1 MiB of latent
    assert per_image == 1 << 20
    n, N = 1000, 10000
    need = train.LatentCache.bytes_needed(n, 16 * 128 * 128, N)
    assert need == n * (per_image + N * 4)
    assert train.LatentCache.fits(n, 16 * 128 * 128, N, need) and not train.LatentCache.fits(n, 16 * 128 * 128, N, need - 1)
    assert not train.LatentCache.fits(1, 16, 1, 0)                          # --latent_cache_gb 0: nothing is cached


# ---- exported keys and the ABI ---------------------------------------------------------------------------------------------------------
def test_front_tensor_names_cover_the_attention_manifest():
    manifest = synth.attention_decoder_manifest(11)
    front = [k for k in manifest if k.startswith(train.FRONT_PREFIXES)]
    header = open(os.path.join(os.path.dirname(train.__file__), "csrc", "vt_train.h")).read()
    table = set(re.findall(r'\{"([a-z_0-9.]+)", \d+, \d+, \d\}', header))
    assert table | set(train.FRONT_BUFFERS) == set(front)
    assert set(manifest) == set(front) | {k for k in manifest if k.startswith("classifier.")}
    # sizes and offsets of the table: every tensor inside its 64-float slots, in order, nothing overlapping
    rows = [(k, int(o), int(n)) for k, o, n in re.findall(r'\{"([a-z_0-9.]+)", (\d+), (\d+), \d\}', header)]
    for (k, off, n), nxt in zip(rows, rows[1:] + [(None, 2240, 0)]):
        shape = manifest[k]
        assert n == int(torch.tensor(shape).prod()) and off % 64 == 0 and off + n <= nxt[1], k


def test_new_symbols_are_in_the_header_and_in_the_ctypes_table():
    header = open(os.path.join(os.path.dirname(train.__file__), "..", "include", "vae_tagger_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.PROTOTYPES, name
        assert re.search(r"\b" + name + r"\(", header), name
    assert (_lib.FRONT_BN_MEAN, _lib.FRONT_BN_VAR, _lib.FRONT_BN_TRACKED) == (6, 7, 8)
    assert re.search(r"VT_FRONT_BN_MEAN = 6, VT_FRONT_BN_VAR = 7, VT_FRONT_BN_TRACKED = 8", header)
