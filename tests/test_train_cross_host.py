"""No GPU: the --train_cross_attention surface of train_decoder (parsing, refusals), the exported key order with the cross-attention
tensors, and the C ABI's new entries in the header, the ctypes table and the layout table of csrc/vt_train.h."""
import os
import re

import pytest
import torch

from vae_tagger_amd import _lib, synth, train, train_decoder

BASE = ["--vae_checkpoint", "ae.safetensors", "--json_path", "data.json", "--tags_csv_path", "tags.csv"]
FULL = ["--train_front", "--use_cross_attention", "--train_cross_attention"]
NEW_SYMBOLS = ("vt_cross_state_bytes", "vt_cross_workspace_bytes", "vt_cross_init", "vt_cross_forward", "vt_cross_backward", "vt_cross_step",
               "vt_cross_commit", "vt_cross_read", "vt_cross_write", "vt_train_clip3")


def parse(*extra):
    return train_decoder.check_args(train_decoder.build_parser().parse_args(BASE + list(extra)))


def test_train_cross_attention_parses_and_passes_the_checks():
    args = parse(*FULL, "--attention_heads", "2")
    assert args.train_front and args.use_cross_attention and args.train_cross_attention and not args.freeze_front
    assert not train_decoder.build_parser().parse_args(BASE).train_cross_attention
    assert not parse("--train_front").train_cross_attention and not parse("--freeze_front", "--use_cross_attention").train_cross_attention


@pytest.mark.parametrize("extra,match", [(["--train_cross_attention", "--use_cross_attention", "--no_attention"], "--train_front"),
                                         (["--train_cross_attention", "--use_cross_attention"], "--train_front"),
                                         (["--train_cross_attention", "--use_cross_attention", "--freeze_front"], "freeze_front"),
                                         (["--train_cross_attention", "--use_cross_attention", "--freeze_front", "--train_front"], "freeze_front"),
                                         (["--train_cross_attention", "--train_front"], "--use_cross_attention"),
                                         (["--train_front", "--use_cross_attention"], "cross-attention is not implemented")])
def test_refusals(extra, match):
    with pytest.raises(RuntimeError, match=match):
        parse(*extra)
    with pytest.raises(SystemExit, match=match):                    # and main() refuses before it touches a file
        train_decoder.main(BASE + ["--output_dir", os.path.join(os.sep, "nonexistent", "out")] + extra)


def test_the_pinned_refusal_names_the_new_flag():
    with pytest.raises(RuntimeError, match="cross-attention is not implemented") as e:
        parse("--train_front", "--use_cross_attention")
    assert "--train_cross_attention" in str(e.value)
    assert re.search("front.*not implemented", train_decoder.FRONT_MESSAGE) and "--train_cross_attention" in train_decoder.FRONT_MESSAGE
    assert "--train_cross_attention" in train_decoder.build_parser().format_help()


def test_new_symbols_are_in_the_header_and_in_the_ctypes_table():
    header = open(os.path.join(os.path.dirname(train.__file__), "..", "include", "vae_tagger_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.PROTOTYPES, name
        assert re.search(r"\b" + name + r"\(", header), name
    assert len(_lib.PROTOTYPES["vt_train_clip3"][1]) == len(_lib.PROTOTYPES["vt_train_clip"][1]) + 2


def test_cross_tensor_table_covers_the_manifest():
    manifest = synth.attention_decoder_manifest(11, 16, True, True, True)
    cross = [k for k in manifest if k.startswith(train.CROSS_PREFIXES)]
    assert train.CROSS_PREFIXES == ("query_generator.", "cross_attention.") and len(cross) == 10
    header = open(os.path.join(os.path.dirname(train.__file__), "csrc", "vt_train.h")).read()
    rows = [(k, int(o), int(n)) for k, o, n in re.findall(r'\{"([a-z_0-9.]+)", (\d+), (\d+)\}', header)]
    assert {k for k, _, _ in rows} == set(cross)
    end = 0
    for k, off, n in rows:                                          # in order, nothing overlapping, every size a multiple of 64
        assert n == int(torch.tensor(manifest[k]).prod()) and n % 64 == 0 and off == end, k
        end = off + n
    assert end == 530176 == sum(int(torch.tensor(manifest[k]).prod()) for k in cross)
    assert re.search(r"VT_CROSS_P = 530176;", header)
    assert set(manifest) == set(cross) | {k for k in manifest if k.startswith(train.FRONT_PREFIXES + ("classifier.",))}


def test_front_trainable_with_and_without_cross_attention():
    from vae_tagger_amd.modules import AttentionClassificationDecoder, ClassificationDecoder
    assert train.front_trainable(AttentionClassificationDecoder(16, 8, 8, 7, use_cross_attention=True))
    assert train.front_trainable(AttentionClassificationDecoder(16, 8, 8, 7))
    assert not train.front_trainable(ClassificationDecoder(16, 8, 8, 7))


def test_export_state_dict_over_head_front_and_cross_names_keeps_order_and_dtypes():
    from vae_tagger_amd.modules import AttentionClassificationDecoder
    dec = AttentionClassificationDecoder(16, 8, 8, 7, use_cross_attention=True)
    sd = dec.state_dict()
    names = [k for k in sd if k.startswith(train.CROSS_PREFIXES + train.FRONT_PREFIXES + ("classifier.",))]
    assert set(names) == set(sd)
    seen = []

    def read(k):
        seen.append(k)
        fill = 3 if sd[k].dtype == torch.int64 else 0.5
        return torch.full(tuple(sd[k].shape), fill, dtype=torch.float64 if sd[k].dtype != torch.int64 else torch.int64)

    out = train.export_state_dict(dec, read, names)
    assert list(out) == list(sd) and sorted(seen) == sorted(names)
    assert all(out[k].dtype == v.dtype and out[k].shape == v.shape for k, v in sd.items())
    assert all(bool((out[k] == (3 if v.dtype == torch.int64 else 0.5)).all()) for k, v in sd.items())
    cross_only = train.export_state_dict(dec, read, [k for k in sd if k.startswith(train.CROSS_PREFIXES)])
    assert torch.equal(cross_only["classifier.0.weight"], sd["classifier.0.weight"].cpu())
    assert bool((cross_only["query_generator.bias"] == 0.5).all())
