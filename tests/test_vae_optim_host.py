"""The VAE optimiser and train_vae on the host: the arena layout (Python mirror against hand-worked offsets and against vt_vae_optim_layout), the
new symbols of the C ABI, the optimiser state through safetensors, the CLI's flags against the reference's names and defaults (a settings-only
fixture), the learning rate at the schedule's corners, and every refusal that needs no device."""
import ctypes
import json
import math
import os

import pytest
import torch

from vae_tagger_amd import _lib, synth, train_vae
from vae_tagger_amd.train import lr_schedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(block_out=(64, 128, 512), layers_per_block=1)
WEIGHTS = {"reconstruction": 1.0, "kl": 0.0, "triplet": 1.0}


def _numels(cfg):
    m = {**synth.encoder_manifest(**cfg), **synth.image_decoder_manifest(**cfg)}
    return [math.prod(s) for s in m.values()]


def _c_layout(numels):
    lib = _lib.load()
    n = len(numels)
    arr, off, total = (ctypes.c_longlong * max(n, 1))(*numels), (ctypes.c_longlong * max(n, 1))(), ctypes.c_longlong(-1)
    rc = lib.vt_vae_optim_layout(arr, n, off, ctypes.byref(total))
    return rc, list(off)[:n], total.value


def test_layout_mirror_against_offsets_worked_out_by_hand():
    # 3 -> one tile [0, 4096); 1 -> one tile [4096, 8192); 4096 -> exactly one tile [8192, 12288); 4097 -> two tiles [12288, 20480)
    assert train_vae.TILE == 4096
    assert train_vae.optim_layout([3, 1, 4096, 4097]) == ([0, 4096, 8192, 12288], 20480)
    assert train_vae.optim_layout([4097]) == ([0], 8192)
    offsets, _ = train_vae.optim_layout([5, 8191, 8193, 7])
    assert offsets == [0, 4096, 12288, 24576] and all(o % 4 == 0 for o in offsets)          # every slot 16-B aligned


def test_c_layout_agrees_with_the_mirror_on_the_flux_and_the_small_manifests():
    for cfg, count in (({}, 244), (SMALL, 152)):
        numels = _numels(cfg)
        assert len(numels) == count
        rc, off, total = _c_layout(numels)
        assert rc == 0 and (off, total) == train_vae.optim_layout(numels)
        assert _lib.load().vt_vae_optim_workspace_bytes((ctypes.c_longlong * count)(*numels), count) == (8 * (total // 4096) + 255) // 256 * 256
    flux = _numels({})
    assert sum(flux) == 83819683 and min(flux) == 3 and [n for n in flux if n % 4] == [3]
    assert train_vae.optim_layout(flux)[1] - sum(flux) < 1 << 20                             # the padding stays below 1 M floats


def test_new_symbols_and_their_argtypes():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "vae_tagger_hip.h")).read()
    c = ctypes
    ll, vp = c.c_longlong, c.c_void_p
    want = {
        "vt_vae_optim_layout": (c.c_int, [c.POINTER(ll), c.c_int, c.POINTER(ll), c.POINTER(ll)]),
        "vt_vae_optim_workspace_bytes": (c.c_size_t, [c.POINTER(ll), c.c_int]),
        "vt_vae_optim_norm": (c.c_int, [vp, c.POINTER(vp), c.POINTER(ll), c.c_int, c.c_float, vp, vp, c.c_size_t, c.c_int, vp]),
        "vt_vae_optim_step": (c.c_int, [vp, vp, vp, vp, c.c_size_t, c.POINTER(vp), c.POINTER(ll), c.c_int, vp] + [c.c_double] * 5 + [ll, c.c_int, vp]),
    }
    for name, (res, args) in want.items():
        fn = getattr(lib, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
        assert name + "(" in header, name
    assert "#define VT_VAE_OPTIM_TILE 4096" in header and f"#define VT_VAE_OPTIM_CHUNK {_lib.VAE_OPTIM_CHUNK}" in header
    assert (_lib.VAE_OPTIM_TILE, train_vae.CHUNK) == (4096, _lib.VAE_OPTIM_CHUNK)
    # the per-element arithmetic has one source, in the header both units include
    csrc = os.path.join(ROOT, "vae_tagger_amd", "csrc")
    assert "void adamw_one(" in open(os.path.join(csrc, "vt_train.h")).read()
    for unit in ("train_common.hip", "vae_optim.hip"):
        text = open(os.path.join(csrc, unit)).read()
        assert "adamw_one(" in text and "void adamw_one(" not in text, unit


def _cpu_trainer(seed=1):
    sd = synth.synth_state_dict({**synth.encoder_manifest(**SMALL), **synth.image_decoder_manifest(**SMALL)}, seed=seed)
    return sd, train_vae.VAETrainer(sd, weights=WEIGHTS, device="cpu")


def test_optimizer_state_round_trip_through_safetensors(tmp_path):
    sd, tr = _cpu_trainer()
    assert list(tr.params) == list(sd) and len(tr.params) == 152
    by_name = train_vae.VAETrainer(dict(sorted(sd.items())), weights=WEIGHTS, device="cpu")      # as a file read back from disk: sorted by name
    assert list(by_name.params) == list(sd) and by_name.offsets == tr.offsets                    # the layout is the manifests', whatever the order given
    flux = {k: torch.empty(tuple(s), device="meta") for k, s in sorted({**synth.encoder_manifest(), **synth.image_decoder_manifest()}.items())}
    assert train_vae.manifest_order(flux, list(flux)) == list({**synth.encoder_manifest(), **synth.image_decoder_manifest()})
    odd = {"encoder.a": torch.zeros(3), "decoder.b": torch.zeros(5)}                             # not such a model: the order given stands
    assert list(train_vae.VAETrainer(odd, weights=WEIGHTS, device="cpu").params) == ["encoder.a", "decoder.b"]
    g = torch.Generator().manual_seed(3)
    for views in (tr.exp_avg, tr.exp_avg_sq):
        for v in views.values():
            v.copy_(torch.randn(v.shape, generator=g))
    tr.t = 7
    state = tr.optimizer_state_dict()
    assert state["step"] == 7 and len(state) == 1 + 2 * 152
    path = str(tmp_path / "optimizer.safetensors")
    train_vae.save_optimizer_state(path, state)
    back = train_vae.load_optimizer_state(path)
    assert back["step"] == 7 and set(back) == set(state)
    assert all(torch.equal(back[k], state[k]) for k in state if k != "step")
    _, other = _cpu_trainer(seed=2)
    before = other.optimizer_state_sha256().hexdigest()
    other.load_optimizer_state_dict(back)
    other.load_state_dict(tr.state_dict())
    assert other.t == 7 and other.optimizer_state_sha256().hexdigest() == tr.optimizer_state_sha256().hexdigest() != before
    # the views alias the arenas, and the padding of all three is zero
    for arena, views in zip(tr._arena, (tr.params, tr.exp_avg, tr.exp_avg_sq)):
        real = torch.zeros(tr.total, dtype=torch.bool)
        for (k, v), off, n in zip(views.items(), tr.offsets, tr.numels):
            assert v.data_ptr() == arena.data_ptr() + 4 * off and v.is_contiguous() and v.numel() == n
            real[off:off + n] = True
        assert not arena[~real].any()


def test_parser_has_every_flag_of_the_reference_with_its_default():
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "train_vae_flags.json")))
    args = train_vae.build_parser().parse_args(["--json_path", "j", "--tags_csv_path", "t"])
    assert len(want) == 30
    for name, default in want.items():
        assert hasattr(args, name), name
        assert getattr(args, name) == default and type(getattr(args, name)) is type(default), name
    with pytest.raises(SystemExit):
        train_vae.build_parser().parse_args([])                                               # --json_path and --tags_csv_path are required
    assert train_vae.ignored_arguments(args) == []
    args = train_vae.build_parser().parse_args(["--json_path", "j", "--tags_csv_path", "t", "--mixed_precision", "bf16", "--cudnn_benchmark",
                                                "--num_workers", "8", "--enable_xformers_memory_efficient_attention"])
    assert train_vae.ignored_arguments(args) == ["mixed_precision", "cudnn_benchmark", "num_workers", "enable_xformers_memory_efficient_attention"]


def test_lr_at_the_corners_of_the_four_schedules():
    base, warmup, total = 1e-4, 4, 20
    lr = lambda kind, k: base * lr_schedule(kind, k, warmup, total)
    last = total - 1
    assert [lr("constant", k) for k in (0, warmup - 1, warmup, last)] == [base] * 4
    assert [lr("constant_with_warmup", k) for k in (0, warmup - 1, warmup, last)] == [0.0, base * 3 / 4, base, base]
    assert [lr("linear", k) for k in (0, warmup - 1, warmup, last)] == [0.0, base * 3 / 4, base, base * (1 / 16)]
    cos = [lr("cosine", k) for k in (0, warmup - 1, warmup, last)]
    assert cos[:3] == [0.0, base * 3 / 4, base] and cos[3] == base * 0.5 * (1.0 + math.cos(math.pi * 15 / 16))
    with pytest.raises(ValueError):
        lr_schedule("polynomial", 0, warmup, total)
    # the batches of an epoch: one bucket each, the same count every epoch
    buckets = [(512, 512), (768, 512), (512, 512), (512, 512), (768, 512)]
    plan = train_vae.plan_train_batches([4, 0, 2, 1, 3], 2, buckets)
    assert plan == [((512, 512), [0, 2]), ((768, 512), [4, 1]), ((512, 512), [3])]
    assert len(plan) == train_vae.steps_per_epoch(5, 2, buckets) == 3 and train_vae.steps_per_epoch(5, 2) == 3
    assert train_vae.plan_train_batches([4, 0, 2, 1, 3], 2) == [(None, [4, 0]), (None, [2, 1]), (None, [3])]


def test_refusals_that_need_no_device():
    for bad in ([], [0], [4, -1], [1 << 41]):
        rc, _, total = _c_layout(bad)
        assert rc == 1 and total == -1, bad                                                   # VT_ERR_INVALID, nothing written
        n = len(bad)
        assert _lib.load().vt_vae_optim_workspace_bytes((ctypes.c_longlong * max(n, 1))(*bad), n) == 0
    assert _lib.load().vt_vae_optim_layout(None, 3, None, None) == 1
    for bad in ([], [0], [4, -1]):
        with pytest.raises(ValueError):
            train_vae.optim_layout(bad)
    lib = _lib.load()
    one = (ctypes.c_longlong * 1)(4)
    assert lib.vt_vae_optim_norm(None, None, one, 1, 1.0, None, None, 0, 0, None) == 1       # no context
    assert lib.vt_vae_optim_step(None, None, None, None, 0, None, one, 1, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0, None) == 1
    sd, tr = _cpu_trainer()
    with pytest.raises(ValueError):
        train_vae.VAETrainer({**sd, "quant_conv.weight": torch.zeros(1)}, weights=WEIGHTS, device="cpu")
    with pytest.raises(ValueError):
        train_vae.VAETrainer({k: v for k, v in sd.items() if k.startswith("encoder.")}, weights=WEIGHTS, device="cpu")
    with pytest.raises(ValueError):
        train_vae.VAETrainer(sd, weights=WEIGHTS, similarity_type="manhattan", device="cpu")
    with pytest.raises(TypeError):
        train_vae.VAETrainer([1, 2], weights=WEIGHTS, device="cpu")
    with pytest.raises(_lib.VTError):
        tr.ctx                                                                                # no CPU fallback
    state = tr.optimizer_state_dict()
    with pytest.raises(ValueError):
        tr.load_optimizer_state_dict({k: v for k, v in state.items() if k != "exp_avg.encoder.conv_in.bias"})
    with pytest.raises(ValueError):
        tr.load_optimizer_state_dict({**state, "step": -1})
    with pytest.raises(ValueError):
        tr.load_state_dict({k: v for k, v in sd.items() if k != "decoder.conv_out.bias"})
    grads = {k: torch.zeros_like(v) for k, v in tr.params.items()}
    with pytest.raises(ValueError):
        tr._grad_pointers(dict(reversed(list(grads.items()))))                                # keyed and ORDERED like params
    with pytest.raises(ValueError):
        tr._grad_pointers({**grads, "decoder.conv_out.bias": torch.zeros(3, dtype=torch.float64)})
    # a configuration with quant convs is refused, as the backward refuses it
    from types import SimpleNamespace
    fake = SimpleNamespace(config=SimpleNamespace(use_quant_conv=False, use_post_quant_conv=True), image_decoder=lambda: None, state_dict=dict)
    with pytest.raises(ValueError, match="use_quant_conv"):
        train_vae.VAETrainer(fake, weights=WEIGHTS, device="cpu")
