"""CPU: the host side of decoder training -- schedules, split, feature cache indexing, the CLI's arguments and the exported keys."""
import math

import pytest
import torch

from vae_tagger_amd import synth, train, train_decoder


@pytest.mark.parametrize("kind", train.SCHEDULES)
def test_lr_schedule_closed_forms(kind):
    warmup, T = 10, 100
    for step in (0, warmup - 1, warmup, 55, T):
        warm = step / max(1, warmup)
        p = (step - warmup) / max(1, T - warmup)
        want = {"constant": 1.0,
                "constant_with_warmup": warm if step < warmup else 1.0,
                "linear": warm if step < warmup else max(0.0, (T - step) / max(1, T - warmup)),
                "cosine": warm if step < warmup else max(0.0, 0.5 * (1.0 + math.cos(math.pi * p)))}[kind]
        assert train.lr_schedule(kind, step, warmup, T) == pytest.approx(want, abs=1e-15), (kind, step)
    assert train.lr_schedule(kind, 0, 0, T) == 1.0                      # no warm-up: the full rate at once
    if kind in ("linear", "cosine"):
        assert train.lr_schedule(kind, T, warmup, T) == pytest.approx(0.0, abs=1e-15)
    with pytest.raises(ValueError):
        train.lr_schedule("polynomial", 0, 1, 2)


def test_split_and_epoch_orders_come_from_the_seed():
    tr, va = train.split_indices(57, 42)
    assert (tr, va) == train.split_indices(57, 42) and (tr, va) != train.split_indices(57, 43)
    assert len(va) == 5 and not set(tr) & set(va) and sorted(tr + va) == list(range(57))
    assert len(train.split_indices(3, 0)[1]) == 1                       # max(1, int(0.1 n))
    o0, o1 = train.epoch_order(52, 42, 0), train.epoch_order(52, 42, 1)
    assert o0 == train.epoch_order(52, 42, 0) and o0 != o1 and sorted(o0) == sorted(o1) == list(range(52))
    with pytest.raises(ValueError):
        train.split_indices(1, 0)


def test_feature_cache_indexing_on_host_tensors():
    c = train.FeatureCache(5, 4, 3, device="cpu")
    f = torch.arange(20.0).view(5, 4)
    y = torch.arange(15.0).view(5, 3)
    c.put(["a", "b"], f[:2], y[:2])
    c.put(["c", "a"], f[2:4], y[2:4])                                   # "a" is overwritten in its slot
    assert len(c) == 3 and "c" in c and "d" not in c and c.nbytes == 5 * 7 * 4
    gf, gy = c.gather(["c", "a", "b", "c"])
    assert torch.equal(gf, f[[2, 3, 1, 2]]) and torch.equal(gy, y[[2, 3, 1, 2]])
    c.put(["d", "e"], f[3:5], y[3:5])
    with pytest.raises(IndexError):
        c.put(["f"], f[:1], y[:1])
    with pytest.raises(ValueError):
        c.put(["a"], f[:2], y[:2])
    with pytest.raises(KeyError):
        c.gather(["zz"])


REFERENCE_ARGV = [
    "--vae_checkpoint", "ae.safetensors", "--vae_config_path", "cfg.json", "--decoder_checkpoint", "d.bin", "--json_path", "d.json",
    "--tags_csv_path", "t.csv", "--output_dir", "o", "--resolution", "512", "--train_batch_size", "8", "--num_epochs", "3",
    "--learning_rate", "5e-4", "--weight_decay", "1e-5", "--mixed_precision", "bf16", "--use_attention", "--no_attention",
    "--use_spatial_attention", "--use_self_attention", "--use_cross_attention", "--attention_heads", "4", "--attention_dropout", "0.2",
    "--use_simplified_decoder_loss", "--use_focal_loss", "--use_class_balanced", "--focal_alpha", "0.25", "--focal_gamma", "1.5",
    "--lr_scheduler_type", "linear", "--lr_warmup_steps", "7", "--max_grad_norm", "0.5", "--logging_steps", "10", "--save_steps", "2",
    "--use_quant_conv", "--use_post_quant_conv", "--use_safetensors", "--use_bucketing", "--base_resolution", "256", "--max_resolution", "512",
    "--bucket_step", "32", "--num_workers", "8", "--prefetch_factor", "4", "--gradient_accumulation_steps", "2", "--seed", "7",
    "--cudnn_benchmark", "--cudnn_deterministic"]


def test_parser_accepts_the_references_arguments_and_reports_the_ignored_ones():
    args = train_decoder.build_parser().parse_args(REFERENCE_ARGV)
    assert args.train_batch_size == 8 and args.lr_scheduler_type == "linear" and args.gradient_accumulation_steps == 2 and args.seed == 7
    assert sorted(train_decoder.ignored_arguments(args)) == sorted(train_decoder.IGNORED_ARGUMENTS)
    train_decoder.check_args(args)
    assert args.use_attention is False
    defaults = train_decoder.build_parser().parse_args(REFERENCE_ARGV[:2] + ["--json_path", "d.json", "--tags_csv_path", "t.csv"])
    assert train_decoder.ignored_arguments(defaults) == []
    assert (defaults.learning_rate, defaults.weight_decay, defaults.lr_warmup_steps, defaults.max_grad_norm, defaults.save_steps) == (1e-3, 1e-6, 500, 1.0, 5)
    assert "NOT" in train_decoder.build_parser().format_help() and "random_split" in train_decoder.build_parser().format_help()


def test_attention_decoder_without_freeze_front_is_refused():
    base = ["--vae_checkpoint", "ae.safetensors", "--json_path", "d.json", "--tags_csv_path", "t.csv"]
    with pytest.raises(RuntimeError, match="front.*not implemented"):
        train_decoder.check_args(train_decoder.build_parser().parse_args(base))
    with pytest.raises(SystemExit, match="not implemented"):
        train_decoder.main(base)                                        # before any file or GPU is touched
    train_decoder.check_args(train_decoder.build_parser().parse_args(base + ["--freeze_front"]))
    train_decoder.check_args(train_decoder.build_parser().parse_args(base + ["--no_attention"]))
    with pytest.raises(RuntimeError, match="lr_scheduler_type"):
        train_decoder.check_args(train_decoder.build_parser().parse_args(base + ["--no_attention", "--lr_scheduler_type", "polynomial"]))


@pytest.mark.parametrize("plain", [True, False])
def test_exported_checkpoint_has_the_decoders_keys(plain):
    from vae_tagger_amd.modules import AttentionClassificationDecoder, ClassificationDecoder
    dec = ClassificationDecoder(16, 8, 8, 7) if plain else AttentionClassificationDecoder(16, 8, 8, 7, use_cross_attention=True)
    asked = []

    def read(name):                                                     # the stubbed head reader
        asked.append(name)
        return torch.full(dec.state_dict()[name].shape, 2.5)
    out = train.export_state_dict(dec, read)
    assert list(out) == list(dec.state_dict()) and sorted(asked) == sorted(train.head_parameter_names(dec))
    for k, v in dec.state_dict().items():
        assert out[k].shape == v.shape and out[k].dtype == v.dtype
        assert bool((out[k] == 2.5).all()) if k.startswith("classifier.") else torch.equal(out[k], v)
    assert train.head_dropout_rates(dec) == ((0.3, 0.2) if plain else (0.3, 0.2, 0.1))
    with pytest.raises(ValueError):
        train.export_state_dict(dec, lambda name: torch.zeros(1))
