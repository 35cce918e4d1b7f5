"""Host side of the validation loss and the checkpoint sweep: the numpy fp64 mirrors against the values the reference's own loss classes
returned (tests/golden/val_loss_reference.npz, made by tools/make_val_loss_fixture.py), the class-balanced weights bit for bit, the host
model of the device state block, the ABI surface, the CLI refusals and defaults, the sweep's naming and ranking, the ISA lint of
eval_loss.hip and a two-rank gloo rehearsal of the loss-block exchange.  No GPU."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from vae_tagger_amd import _lib, evaluate, infer_full, losses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vae_tagger_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
BASE = ["--vae_checkpoint", "v", "--decoder_checkpoint", "d", "--json_path", "j", "--tags_csv_path", "t"]
REL_FP64 = 1e-9          # the bound the project uses for AP; fp64 sums of 288 terms stay orders of magnitude inside it
REL_FP32 = 1e-5          # the reference's own fp32 run against its fp64 run: information, asserted no tighter than this


@pytest.fixture(scope="module")
def fixture():
    with np.load(os.path.join(ROOT, "tests", "golden", "val_loss_reference.npz"), allow_pickle=False) as z:
        return {k: z[k].copy() for k in z.files}


def _rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def test_numpy_mirrors_match_the_reference_losses(fixture):
    """Observed on the committed fixture: largest relative distance of a mirror to the reference's fp64 value 2.7e-16 (class-balanced,
    fractional labels; BCE and most focal values are bit-equal); the reference's fp32 values lie up to 8.3e-8 from its fp64 ones."""
    x, s = fixture["logits"], fixture["samples_per_class"]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "val_loss_reference.npz")) < 64 * 1024
    for v in (0.0, 30.0, 88.0, 1e4, 1e-40, 1.4e-45):                     # the extremes are in the logits, with both signs
        v32 = np.float32(v)
        assert (x == v32).any() and ((x == -v32) & (np.signbit(x))).any(), v
    assert [tuple(p) for p in fixture["focal_params"]] == [(1.0, 2.0), (0.25, 2.0), (1.0, 0.5), (1.0, 0.0)]
    assert (s > 0).all()
    worst64 = worst32 = 0.0
    for kind in ("float", "u8"):
        y = fixture[f"labels_{kind}"]
        if kind == "float":
            assert ((y > 0) & (y < 1)).any()                             # fractional labels are used as their value
        else:
            assert set(np.unique(y).tolist()) == {0, 1}
        got = {"bce": [losses.bce_loss(x, y)], "focal": [losses.focal_loss(x, y, a, g) for a, g in fixture["focal_params"]],
               "class_balanced": [losses.class_balanced_loss(x, y, s, float(fixture["beta"]))]}
        for name, values in got.items():
            want64 = np.atleast_1d(fixture[f"{name}_{kind}_f64"])
            want32 = np.atleast_1d(fixture[f"{name}_{kind}_f32"])
            for g, w64, w32 in zip(values, want64, want32):
                assert np.isfinite(g) and np.isfinite(w64)
                d64, d32 = _rel(g, w64), _rel(w32, w64)
                print(f"{kind:5s} {name:14s} mirror {g!r} reference fp64 {float(w64)!r} rel {d64:.3e}; reference fp32 rel {d32:.3e}")
                worst64, worst32 = max(worst64, d64), max(worst32, d32)
                assert d64 <= REL_FP64, (kind, name, g, w64)
                assert d32 <= REL_FP32, (kind, name, w32, w64)
        # per element: the reference's form (1 - y) x - logsigmoid(x) cancels at magnitude |x|, ours at |x y|: a few ulp of max(1, |x|)
        tol = 8 * np.finfo(np.float64).eps * np.maximum(1.0, np.abs(x.astype(np.float64)))
        assert (np.abs(losses.bce_elements(x, y) - fixture[f"bce_elements_{kind}_f64"]) <= tol).all()
        assert (np.abs(losses.focal_elements(x, y, 1.0, 2.0) - fixture[f"focal_elements_{kind}_f64"]) <= tol).all()
    print(f"largest relative distance: mirrors to fp64 {worst64:.3e}, reference fp32 to fp64 {worst32:.3e}")


def test_class_balanced_weights_equal_the_reference_tensor_bit_for_bit(fixture):
    w = losses.class_balanced_weights(fixture["samples_per_class"], float(fixture["beta"]))
    assert w.dtype == np.float32 and np.array_equal(w.view(np.uint32), fixture["class_balanced_weights_f32"].view(np.uint32))
    assert abs(float(w.astype(np.float64).sum()) - len(w)) < 1e-4
    z = losses.class_balanced_weights([3, 0, 10])
    assert np.isposinf(z[1]) and z[0] == 0 and z[2] == 0               # a class without a sample: an infinite weight, an infinite loss
    x, y = np.array([[0.5, -1.0, 2.0]], dtype=np.float32), np.array([[1, 0, 1]], dtype=np.float32)
    h = losses.HostLossState(3, class_weights=z)
    h.update(x, y)
    assert h.read()["class_balanced"]["mean_of_batch_means"] == np.inf and np.isfinite(h.read()["bce"]["per_element"])


def test_class_distribution_counts_positive_labels_over_every_row():
    rows = {"a": np.array([0.5, 0.0, 1.0], np.float32), "b": np.array([0.0, 0.0, 0.25], np.float32), "c": np.array([1.0, -1.0, 0.0], np.float32)}
    d = losses.class_distribution(rows)
    assert d.dtype == np.float64 and d.tolist() == [2.0, 0.0, 2.0]
    assert losses.class_distribution([], 4).tolist() == [0.0] * 4
    assert [losses.select_loss(cb, f) for cb, f in ((False, False), (False, True), (True, False), (True, True))] == \
        ["bce", "focal", "class_balanced", "class_balanced"]


def test_host_state_reports_both_means_and_round_trips_through_the_block_layout():
    rng = np.random.default_rng(2)
    n = 70                                                               # two workgroups of 64 classes: two partial slots in the layout
    x = (rng.standard_normal((45, n)) * 3).astype(np.float32)
    y = ((rng.random((45, n)) < 0.3) * rng.choice([0.5, 1.0], size=(45, n))).astype(np.float32)
    w = losses.class_balanced_weights(rng.integers(1, 100, n))
    h = losses.HostLossState(n, 0.25, 2.0, w)
    cuts = [(0, 16), (16, 32), (32, 37), (37, 45)]
    for lo, hi in cuts:
        h.update(x[lo:hi], y[lo:hi])
    r = h.read()
    batch_means = {"bce": [losses.bce_loss(x[a:b], y[a:b]) for a, b in cuts],
                   "focal": [losses.focal_loss(x[a:b], y[a:b], 0.25, 2.0) for a, b in cuts],
                   "class_balanced": [float((losses.bce_elements(x[a:b], y[a:b]) * w.astype(np.float64)).mean()) for a, b in cuts]}
    whole = {"bce": losses.bce_loss(x, y), "focal": losses.focal_loss(x, y, 0.25, 2.0),
             "class_balanced": float((losses.bce_elements(x, y) * w.astype(np.float64)).mean())}
    for name in losses.LOSS_NAMES:
        assert _rel(r[name]["mean_of_batch_means"], np.mean(batch_means[name])) <= 1e-12, name     # the reference's val_loss / val_steps
        assert _rel(r[name]["per_element"], whole[name]) <= 1e-12, name
        assert r[name]["mean_of_batch_means"] != r[name]["per_element"]                             # uneven batches: the two differ
    assert (r["steps"], r["elements"], r["non_finite"]) == (4, 45 * n, 0)
    assert _rel(r["per_class"]["Class_3"]["bce"], losses.bce_elements(x, y)[:, 3].mean()) <= 1e-12
    block = h.to_bytes()
    lay = losses.state_layout(n)
    assert len(block) == lay["total"] and all(v % 256 == 0 for v in lay.values())
    assert lay["total"] - lay["partials"] == 256 and losses.state_layout(10000)["total"] == 512 + 80128 + 160000 + 5120
    s = losses.parse_state(block, n)
    assert losses.pack_state(s) == block and losses.finish_state(s) == r
    with pytest.raises(ValueError):
        losses.parse_state(block, n + 1)
    no_w = losses.HostLossState(n)
    no_w.update(x, y)
    assert no_w.read()["class_balanced"] is None
    with pytest.raises(ValueError, match="no data"):
        losses.HostLossState(n).read()


def test_sum_states_adds_in_the_order_given_and_refuses_other_parameters():
    rng = np.random.default_rng(5)
    n = 9
    parts = []
    for k in range(3):
        h = losses.HostLossState(n, 1.0, 2.0)
        h.update((rng.standard_normal((7 + k, n)) * 10 ** k).astype(np.float32), (rng.random((7 + k, n)) < 0.5).astype(np.float32))
        parts.append(h.state)
    m = losses.sum_states(parts)
    want = ((np.zeros((n, 2)) + parts[0]["class_sums"]) + parts[1]["class_sums"]) + parts[2]["class_sums"]
    assert m["class_sums"].tobytes() == want.tobytes() and m["steps"] == 3 and m["elements"] == n * (7 + 8 + 9)
    other = losses.sum_states(parts[::-1])                               # fp64 addition is not associative: the order is part of the result
    assert np.allclose(other["class_sums"], m["class_sums"], rtol=1e-12)
    for kw in ({"alpha": 0.25}, {"gamma": 1.0}, {"class_weights": np.full(n, 2.0)}):
        h = losses.HostLossState(n, **{"alpha": 1.0, "gamma": 2.0, **kw})
        with pytest.raises(ValueError, match="different alpha"):
            losses.sum_states([parts[0], h.state])


# ---- ABI surface ----------------------------------------------------------------------------------------------------------------------
def _header_params(header, name):
    m = re.search(r"\b(size_t|int)\s+%s\(([^;]*?)\);" % name, header, re.S)
    assert m, name
    body = re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S)
    return m.group(1), [a.strip() for a in body.split(",")]


def test_loss_symbols_are_in_the_header_the_bindings_and_the_built_library():
    header = open(os.path.join(ROOT, "include", "vae_tagger_hip.h")).read()
    lib = _lib.load()
    want = {"vt_loss_state_bytes": ("size_t", ["int"]),
            "vt_loss_reset": ("int", ["vt_context*", "void*", "size_t", "int", "double", "double", "const double*", "void*"]),
            "vt_loss_update": ("int", ["vt_context*", "void*", "size_t", "int", "const float*", "const void*", "int", "int", "void*"]),
            "vt_loss_read": ("int", ["vt_context*", "const void*", "size_t", "int", "void*", "size_t", "void*"]),
            "vt_loss_merge": ("int", ["vt_context*", "void*", "size_t", "int", "double", "double", "const double*", "const vt_loss_source*", "int",
                                      "void*"])}
    ctype = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "double": ctypes.c_double, "const vt_loss_source*": ctypes.POINTER(_lib.LossSource)}
    for name, (res, params) in want.items():
        assert hasattr(lib, name), f"{name} is not exported by the built library"
        got_res, got = _header_params(header, name)
        assert got_res == res
        assert [re.sub(r"\s*\w+$", "", g).replace(" *", "*") for g in got] == params, name
        pres, pargs = _lib.PROTOTYPES[name]
        assert pres is ctype[res] and len(pargs) == len(params)
        for t, a in zip(params, pargs):
            assert a is (ctype[t] if t in ctype else ctypes.c_void_p), (name, t)
    assert re.search(r"typedef struct \{[^}]*state;[^}]*state_bytes;[^}]*alpha;[^}]*gamma;[^}]*class_weights[^}]*\} vt_loss_source;", header)
    assert [f[0] for f in _lib.LossSource._fields_] == ["state", "state_bytes", "alpha", "gamma", "class_weights"]
    assert ctypes.sizeof(_lib.LossSource) == 40
    assert "train_decoder.py:218-241" in header and all(n in header for n in ("BCEWithLogitsLoss", "FocalLoss", "ClassBalancedLoss"))
    assert lib.vt_loss_state_bytes(0) == 0 and lib.vt_loss_state_bytes(-3) == 0
    for n in (1, 11, 64, 65, 257, 10000):                                # the Python layout is the library's
        assert lib.vt_loss_state_bytes(n) == losses.state_layout(n)["total"], n
    assert "eval_loss.hip" in open(os.path.join(CSRC, "Makefile")).read()
    assert "vt_loss_update" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_eval_loss_compiles_without_a_floating_point_atomic(tmp_path):
    """The -S route needs only hipcc: no skip.  Determinism is part of the contract: no atomic instruction of any kind is expected in
    the unit, and a floating-point one (global / flat / buffer / ds *_atomic_*add_f32 / f64, pk_add, fmin, fmax) never."""
    assert os.path.exists(HIPCC), "hipcc is needed to lint the generated code"
    out = tmp_path / "eval_loss.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "-S", "--cuda-device-only",
           "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", str(out), os.path.join(CSRC, "eval_loss.hip")]
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    asm = out.read_text()
    kernels = re.findall(r"^(_Z\w*loss_\w+):", asm, re.M)
    assert len([k for k in kernels if "loss_accumulate_kernel" in k]) == 2 and any("loss_fold_kernel" in k for k in kernels) \
        and any("loss_merge_kernel" in k for k in kernels), kernels
    code = [l.strip() for l in asm.split("\n") if l.strip() and not l.strip().startswith((";", ".", "//"))]
    fp_atomic = re.compile(r"atomic\w*(_f16|_f32|_f64|_bf16|fadd|fmin|fmax|pk_add)|atomic_(add|min|max)_(f|x2_f)", re.I)
    assert not [l for l in code if fp_atomic.search(l)]
    assert not [l for l in code if re.match(r"(\w+_)?atomic|\w+_atomic", l)]   # no atomic instruction at all, vector or scalar
    acc = asm[asm.index("\n" + [k for k in kernels if "loss_accumulate_kernel" in k][0] + ":"):]
    acc = acc[:acc.index("s_endpgm")]
    assert "v_fma_f64" in acc or "v_mul_f64" in acc                      # the loss is evaluated in fp64
    for block in asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if "loss_" in name:
            assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1)) == 0, name
            assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)) == 0, name


# ---- CLI ------------------------------------------------------------------------------------------------------------------------------
def test_parser_takes_the_loss_flags_with_the_reference_defaults():
    p = evaluate.build_parser(distributed=True, recount=True, val_loss=True)
    a = p.parse_args(BASE)
    assert (a.val_loss, a.use_focal_loss, a.use_class_balanced, a.focal_alpha, a.focal_gamma, a.decoder_checkpoints) == \
        (False, False, False, 1.0, 2.0, None)
    a = p.parse_args(BASE + ["--decoder_checkpoints", "a.pth", "b.pth", "c.pth", "--use_focal_loss", "--focal_alpha", "0.25"])
    assert a.decoder_checkpoints == ["a.pth", "b.pth", "c.pth"] and a.use_focal_loss and a.focal_alpha == 0.25
    flags = lambda q: {o for act in q._actions for o in act.option_strings}
    assert flags(p) - flags(evaluate.build_parser(distributed=True, recount=True)) == \
        {"--val_loss", "--use_focal_loss", "--use_class_balanced", "--focal_alpha", "--focal_gamma", "--decoder_checkpoints"}
    text = p.format_help()
    assert "655 MB" in text and "6.6 GB" in text                         # the memory of the sweep is stated in the help


def test_refused_flag_combinations_stop_before_any_gpu_work(monkeypatch, tmp_path):
    def never(*a, **k):
        raise AssertionError("reached GPU / process-group work")
    monkeypatch.setattr(infer_full, "_dist_setup", never)
    monkeypatch.setattr(infer_full, "load_models", never)
    monkeypatch.setattr(torch.cuda, "is_available", never)
    monkeypatch.setenv("WORLD_SIZE", "1")
    parser = evaluate.build_parser(distributed=True, recount=True, val_loss=True)
    sd = lambda n: {"classifier.8.weight": torch.zeros(256, 512), "classifier.12.weight": torch.zeros(n, 256), "classifier.12.bias": torch.zeros(n),
                    "query_generator.weight": torch.zeros(512, 64)}
    paths = []
    for k, n in enumerate((11, 11, 12)):
        paths.append(str(tmp_path / f"epoch_{k}.pth"))
        torch.save(sd(n), paths[-1])
    assert evaluate.checkpoint_tag_count(paths[0]) == 11 and evaluate.checkpoint_tag_count(paths[2]) == 12

    def run(extra):
        args = parser.parse_args(BASE + extra)
        if args.decoder_checkpoints:
            args.single_pass = args.val_loss = True
        evaluate.evaluate(args)
    with pytest.raises(RuntimeError, match="host_metrics"):
        run(["--val_loss", "--host_metrics"])
    with pytest.raises(RuntimeError, match="host_metrics"):
        run(["--decoder_checkpoints"] + paths[:2] + ["--host_metrics"])
    with pytest.raises(RuntimeError, match="decoder_checkpoints.*--threshold"):
        run(["--decoder_checkpoints"] + paths[:2] + ["--threshold", "0.4"])
    with pytest.raises(RuntimeError, match="different numbers of tags.*epoch_2.pth: 12"):
        run(["--decoder_checkpoints"] + paths)
    with pytest.raises(RuntimeError, match="不存在"):
        run(["--decoder_checkpoints", paths[0], str(tmp_path / "missing.pth")])
    args = parser.parse_args(BASE + ["--decoder_checkpoints"] + paths[:2])
    args.single_pass = args.val_loss = True
    evaluate.check_mode(args, 1)                                         # equal tag counts pass
    evaluate.check_mode(parser.parse_args(BASE + ["--val_loss", "--threshold", "0.4"]), 1)


# ---- sweep: names, ranking, tie rule (pure Python) ------------------------------------------------------------------------------------
def _row(path, bce, focal, f1, cb=None, non_finite=0):
    pair = lambda v: None if v is None else {"mean_of_batch_means": v, "per_element": v * 0.99}
    return {"path": path, "loss": {"bce": pair(bce), "focal": pair(focal), "class_balanced": pair(cb), "steps": 5, "elements": 50,
                                   "non_finite": non_finite, "alpha": 1.0, "gamma": 2.0, "per_class": {}},
            "optimal": {"global_threshold": 0.35, "global_f1": f1 + 0.01, "per_class_thresholds": {}},
            "metrics": {"f1_macro": f1, "f1_micro": f1 / 2, "mAP": 0.5, "per_class": {}}}


def test_sweep_names_ranking_and_tie_rule():
    assert losses.sweep_dir_name(0, "/runs/a/epoch_03.pth") == "ckpt_0_epoch_03"
    assert losses.sweep_dir_name(12, "best_pytorch_model.bin") == "ckpt_12_best_pytorch_model"
    assert losses.sweep_dir_name(1, "dir.v2/model.safetensors") == "ckpt_1_model"
    rows = [_row("a.pth", 0.50, 0.20, 0.30), _row("b.pth", 0.40, 0.25, 0.45), _row("c.pth", 0.40, 0.10, 0.45), _row("d.pth", 0.60, 0.30, 0.10)]
    s = losses.sweep_summary(rows, "bce")
    assert s["best_by_val_loss"] == {"index": 1, "path": "b.pth"}       # 0.40 twice: the earlier checkpoint
    assert s["best_by_macro_f1"] == {"index": 1, "path": "b.pth"}       # 0.45 twice: the earlier checkpoint
    assert [c["index"] for c in s["checkpoints"]] == [0, 1, 2, 3] and s["selected_loss"] == "bce"
    c = s["checkpoints"][2]
    assert c["val_loss"] == 0.40 and c["bce"]["mean_of_batch_means"] == 0.40 and c["focal"]["per_element"] == 0.10 * 0.99
    assert (c["global_threshold"], c["global_f1"], c["f1_macro"], c["f1_micro"], c["mAP"], c["non_finite"], c["path"]) == \
        (0.35, 0.46, 0.45, 0.225, 0.5, 0, "c.pth")
    assert losses.sweep_summary(rows, "focal")["best_by_val_loss"] == {"index": 2, "path": "c.pth"}    # ranked by the SELECTED loss
    json.dumps(s)
    with pytest.raises(ValueError, match="class_balanced"):
        losses.sweep_summary(rows, "class_balanced")                     # selected but not accumulated
    nan_rows = [_row("a.pth", float("nan"), 0.2, 0.3, non_finite=4), _row("b.pth", 0.7, 0.2, 0.3)]
    s = losses.sweep_summary(nan_rows, "bce")
    assert s["best_by_val_loss"] == {"index": 1, "path": "b.pth"} and s["checkpoints"][0]["non_finite"] == 4    # a NaN never wins
    report = losses.loss_report(rows[0]["loss"], "focal")
    assert report["selected_loss"] == "focal" and report["val_loss"] == 0.20 and "per_class" not in report and report["bce"]["mean_of_batch_means"] == 0.5


# ---- two ranks over gloo: the loss-block exchange -------------------------------------------------------------------------------------
_RANK_SCRIPT = """
import os, sys
sys.path.insert(0, {root!r})
import numpy as np, torch, torch.distributed as dist
from vae_tagger_amd import losses
rank = int(sys.argv[1])
dist.init_process_group("gloo", init_method="file://" + sys.argv[2], world_size=2, rank=rank)
n = 70
rng = np.random.default_rng(100 + rank)
w = losses.class_balanced_weights(np.arange(1, n + 1))
h = losses.HostLossState(n, 0.25, 2.0, w)
for b in range(2 + rank):                                   # rank 0 feeds two batches, rank 1 three
    h.update((rng.standard_normal((5 + b, n)) * (1.0 + 1e6 * rank)).astype(np.float32), (rng.random((5 + b, n)) < 0.4).astype(np.float32))
mine = h.to_bytes()
parts = losses.exchange_loss_blocks(torch.frombuffer(bytearray(mine), dtype=torch.uint8), dist.group.WORLD)
assert len(parts) == 2 and parts[rank].numpy().tobytes() == mine
states = [losses.parse_state(p.numpy(), n) for p in parts]
assert [s["steps"] for s in states] == [2, 3]              # the list is in RANK order on every rank
merged = losses.sum_states(states)
want = (np.zeros((n, 2)) + states[0]["class_sums"]) + states[1]["class_sums"]
assert merged["class_sums"].tobytes() == want.tobytes()
assert merged["batch_mean_sums"].tobytes() == ((np.zeros(3) + states[0]["batch_mean_sums"]) + states[1]["batch_mean_sums"]).tobytes()
assert (merged["steps"], merged["elements"]) == (5, n * (5 + 6 + 5 + 6 + 7))
np.save(sys.argv[3], np.frombuffer(losses.pack_state(merged), dtype=np.uint8))
dist.barrier()
dist.destroy_process_group()
print("EXCHANGE_OK", rank)
"""


def test_two_rank_gloo_rehearsal_of_the_loss_block_exchange(tmp_path):
    script = tmp_path / "rank.py"
    script.write_text(_RANK_SCRIPT.format(root=ROOT))
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", GLOO_SOCKET_IFNAME="lo")
    procs = [subprocess.Popen([sys.executable, str(script), str(r), str(tmp_path / "store"), str(tmp_path / f"merged_{r}.npy")], env=env, cwd=ROOT,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE) for r in range(2)]
    outs = [p.communicate(timeout=240) for p in procs]
    for r, (p, (so, se)) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"EXCHANGE_OK {r}".encode() in so, se.decode()[-3000:]
    a, b = np.load(tmp_path / "merged_0.npy"), np.load(tmp_path / "merged_1.npy")
    assert a.tobytes() == b.tobytes()                                    # every rank computes the same merged block
    m = losses.finish_state(losses.parse_state(a, 70))
    assert m["steps"] == 5 and np.isfinite(m["class_balanced"]["mean_of_batch_means"])
