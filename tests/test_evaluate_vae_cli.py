"""python -m vae_tagger_amd.evaluate_vae: parser, batch plan and report arithmetic on the host; on the GPU the CLI's files against a loop
written here from forward_device, sample_device and the numpy mirrors, the ordering of per_image.json, a two-checkpoint sweep and
byte-identical files from two runs."""
import argparse
import json
import math
import os

import numpy as np
import pytest
import torch

from vae_tagger_amd import evaluate_vae, improved_losses as il, synth, vae_losses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-9
TAGS = ["cat", "dog", "tree", "sky", "car"]
PROMPTS = ["cat, dog", "dog:0.5, tree", "sky", "cat, sky, car", "tree, car:0.25", "dog"]


# ---- host -----------------------------------------------------------------------------------------------------------------------------
def test_parser_has_train_vaes_loss_arguments_with_its_defaults():
    p = evaluate_vae.build_parser()
    a = p.parse_args(["--json_path", "j", "--tags_csv_path", "t"])
    assert (a.reconstruction_weight, a.kl_weight, a.triplet_weight, a.triplet_margin, a.similarity_type) == (0.01, 1e-2, 1.0, 1.0, "cosine")
    assert (a.resolution, a.batch_size, a.base_resolution, a.max_resolution, a.bucket_step, a.seed) == (1024, 4, 512, 1024, 64, 42)
    assert not a.use_simplified_vae_loss and not a.use_bucketing and a.vae_checkpoints is None and a.decoder_checkpoint is None
    assert a.classification_weight == 1.0 and not a.fp16_operands and not a.bf16_operands
    a = p.parse_args(["--json_path", "j", "--tags_csv_path", "t", "--vae_checkpoints", "a.safetensors", "b.safetensors", "--similarity_type", "euclidean"])
    assert a.vae_checkpoints == ["a.safetensors", "b.safetensors"] and a.similarity_type == "euclidean"
    with pytest.raises(SystemExit):
        evaluate_vae.main(["--json_path", "j", "--tags_csv_path", "t"])                   # no model at all
    assert "NOT the reference's stream" in evaluate_vae.__doc__ and "ANCHOR's bucket" in evaluate_vae.__doc__


def test_batch_plan_keeps_an_images_position_whatever_the_batch_size():
    paths = [f"{i}.png" for i in range(7)]
    assert evaluate_vae.plan_batches(paths, 3) == [(None, [0, 1, 2]), (None, [3, 4, 5]), (None, [6])]
    buckets = [(512, 512), (768, 512), (512, 512), (768, 512), (512, 512), (512, 768), (512, 512)]
    plan = evaluate_vae.plan_batches(paths, 2, buckets)
    assert plan == [((512, 512), [0, 2]), ((512, 512), [4, 6]), ((512, 768), [5]), ((768, 512), [1, 3])]
    order = lambda pl: [i for _, b in pl for i in b]
    assert order(plan) == order(evaluate_vae.plan_batches(paths, 5, buckets)) == [0, 2, 4, 6, 5, 1, 3]
    assert all(len({buckets[i] for i in b}) == 1 for _, b in plan)


def _args(**kw):
    base = dict(reconstruction_weight=0.01, kl_weight=0.01, triplet_weight=1.0, similarity_type="cosine", use_simplified_vae_loss=False,
                classification_weight=2.0)
    base.update(kw)
    return argparse.Namespace(**base)


def test_report_arithmetic_on_a_host_state():
    rng = np.random.default_rng(3)
    h = vae_losses.HostVAELossState(1.0, seed=5)
    m = [rng.standard_normal((6, 8, 2, 2)).astype(np.float32) for _ in range(3)]
    recon, target = rng.standard_normal((2, 6, 3, 4, 4)).astype(np.float32)
    rows = np.concatenate([h.update((m[0][s], None, 1), (m[1][s], None, 2), (m[2][s], None, 3), recon[s], target[s], first_image=s.start)
                           for s in (slice(0, 4), slice(4, 6))])
    c = vae_losses.finish_state(h.state, {"reconstruction": 1, "kl": 1, "triplet": 1})["components"]
    comp = lambda name: c[name]["mean_of_batch_means"]
    full = evaluate_vae.build_report(h.state, _args())
    assert full["val_loss"] == full["val_loss_train_vae"] == 0.01 * comp("mse") + 1.0 * comp("triplet_cosine") + 0.01 * comp("kl_log")
    simple = evaluate_vae.build_report(h.state, _args(use_simplified_vae_loss=True, similarity_type="euclidean"))
    assert simple["val_loss"] == 0.01 * comp("mse") + 1.0 * comp("triplet_euclidean")
    cls = ({"bce": {"mean_of_batch_means": 0.7}, "focal": {"mean_of_batch_means": 0.2}, "class_balanced": None}, "focal")
    tf = evaluate_vae.build_report(h.state, _args(), cls)
    assert abs(tf["val_loss_train_full"] - (full["val_loss"] + 2.0 * 0.2)) <= 1e-15 and tf["val_loss"] == tf["val_loss_train_full"]
    tfs = evaluate_vae.build_report(h.state, _args(use_simplified_vae_loss=True), cls)     # SimplifiedCombinedLoss: triplet + classification
    assert abs(tfs["val_loss"] - (comp("triplet_cosine") + 0.4)) <= 1e-15
    json.dumps(full)
    # per_image.json: sorted by mse, worst first; PSNR of [-1, 1] images
    paths = [f"{i}.png" for i in range(6)]
    order = [3, 1, 5, 0, 2, 4]
    trip = [(i, (i + 1) % 6) for i in range(6)]
    table = evaluate_vae.per_image_table(rows, paths, order, trip, "cosine")
    assert [e["mse"] for e in table] == sorted(rows[:, 0], reverse=True)
    top = table[0]
    k = int(np.argmax(rows[:, 0]))
    assert top["path"] == paths[order[k]] and top["positive"] == paths[order[k]] and top["negative"] == paths[(order[k] + 1) % 6] and top["position"] == k
    assert abs(top["psnr"] - (20 * math.log10(2.0) - 10 * math.log10(top["mse"]))) <= 1e-12 and top["kl"] == rows[k, 1] and top["triplet"] == rows[k, 10]
    assert evaluate_vae.psnr(0.0) == float("inf") and abs(evaluate_vae.psnr(4.0)) <= 1e-12
    # the sweep: ranked by the selected total, a tie to the earlier checkpoint, a NaN never wins
    rep = lambda v: {"val_loss": v, "val_loss_per_image": v, "components": {}, "non_finite": 0}
    s = evaluate_vae.sweep_summary([{"path": "a", "report": rep(0.5)}, {"path": "b", "report": rep(float("nan"))}, {"path": "c", "report": rep(0.3)},
                                    {"path": "d", "report": rep(0.3)}])
    assert s["ranking"] == [2, 3, 0] and s["best_by_val_loss"] == {"index": 2, "path": "c"} and [c["index"] for c in s["checkpoints"]] == [0, 1, 2, 3]


# ---- device ---------------------------------------------------------------------------------------------------------------------------
def _dataset(tmp):
    from PIL import Image
    rng = np.random.default_rng(17)
    paths = []
    for i in range(6):
        yy, xx = np.mgrid[0:64, 0:64]
        img = np.stack([(xx * (i + 1) * 4) % 256, (yy * (6 - i) * 3) % 256, rng.integers(0, 256, (64, 64))], axis=2).astype(np.uint8)
        paths.append(str(tmp / f"img_{i}.png"))
        Image.fromarray(img).save(paths[-1])
    (tmp / "tags.csv").write_text("name\n" + "\n".join(TAGS) + "\n")
    (tmp / "val.json").write_text(json.dumps(dict(zip(paths, PROMPTS))))
    return paths


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """One data set, two checkpoints (the second with conv_out's bias moved by 10: its reconstruction is worse by construction), the CLI
    once alone, once as a sweep (which runs the first checkpoint again) and once with a decoder for train_full's total."""
    from safetensors.torch import save_file
    tmp = tmp_path_factory.mktemp("evaluate_vae")
    paths = _dataset(tmp)
    sd = synth.synth_state_dict(synth.encoder_manifest(), seed=0)
    sd.update(synth.synth_state_dict(synth.image_decoder_manifest(), seed=3))
    good, bad = str(tmp / "good.safetensors"), str(tmp / "bad.safetensors")
    save_file({k: v.contiguous() for k, v in sd.items()}, good)
    sd["decoder.conv_out.bias"] = sd["decoder.conv_out.bias"] + 10.0
    save_file({k: v.contiguous() for k, v in sd.items()}, bad)
    common = ["--json_path", str(tmp / "val.json"), "--tags_csv_path", str(tmp / "tags.csv"), "--resolution", "64", "--batch_size", "4", "--seed", "7",
              "--reconstruction_weight", "1.0", "--triplet_margin", "0.5"]
    evaluate_vae.main(["--vae_checkpoint", good, "--output_dir", str(tmp / "one")] + common)
    evaluate_vae.main(["--vae_checkpoints", good, bad, "--output_dir", str(tmp / "sweep")] + common)
    dec = str(tmp / "decoder.pth")
    torch.save(synth.synth_state_dict(synth.attention_decoder_manifest(len(TAGS)), seed=1), dec)
    evaluate_vae.main(["--vae_checkpoint", good, "--output_dir", str(tmp / "full"), "--decoder_checkpoint", dec, "--use_simplified_vae_loss",
                       "--use_focal_loss", "--classification_weight", "0.5", "--triplet_weight", "2.0"] + common)
    return {"tmp": tmp, "paths": paths, "good": good, "bad": bad}


@pytest.mark.gpu
def test_cli_report_equals_a_loop_over_forward_device_and_the_mirrors(runs):
    from PIL import Image
    from vae_tagger_amd.diffusers_vae_loader import DiffusersVAEWrapper, get_diffusers_vae_config, load_diffusers_vae_from_config
    from vae_tagger_amd.evaluate import TaggedImageList
    from vae_tagger_amd.modules import get_image_transform
    tmp, paths = runs["tmp"], runs["paths"]
    report = json.load(open(tmp / "one" / "vae_validation_loss.json"))
    data = TaggedImageList(str(tmp / "val.json"), str(tmp / "tags.csv"))
    labels = np.stack([data.labels[p] for p in paths])
    assert labels[1, 1] == 0.5 and labels[4, 4] == 0.25
    triplets = evaluate_vae.triplet_lists(labels, 7)
    model = DiffusersVAEWrapper(load_diffusers_vae_from_config(get_diffusers_vae_config(), runs["good"])).to("cuda:0").eval()
    tf = get_image_transform(64)
    load = lambda idx: torch.stack([tf(Image.open(paths[i]).convert("RGB")) for i in idx]).cuda()
    rows, batch = [], {k: [] for k in ("mse", "kl_log", "triplet_cosine", "triplet_euclidean")}
    for lo, idx in ((0, [0, 1, 2, 3]), (4, [4, 5])):
        xa = load(idx)
        recon, pa = model.forward_device(xa, 7, lo)
        pp = model.vae.encode(load([triplets[i][0] for i in idx])).latent_dist
        pn = model.vae.encode(load([triplets[i][1] for i in idx])).latent_dist
        z = [p.sample_device(7, k + 1, lo).cpu().numpy() for k, p in enumerate((pa, pp, pn))]
        kl = [il.kl_elements(p.parameters.cpu().numpy()) for p in (pa, pp, pn)]
        assert np.allclose(pa.kl_device().cpu().numpy(), kl[0], rtol=REL, atol=0)
        la, lp = labels[idx], labels[[triplets[i][0] for i in idx]]
        r = vae_losses.rows_from_mirrors(z[0], z[1], z[2], kl, recon.cpu().numpy(), xa.cpu().numpy(), la, lp, 0.5)
        rows.append(r)
        batch["mse"].append(r[:, 0].mean())
        batch["kl_log"].append(il.kl_log(r[:, 4].mean()))
        batch["triplet_cosine"].append(r[:, 10].mean())
        batch["triplet_euclidean"].append(r[:, 11].mean())
    rows = np.concatenate(rows)

    def rel(got, want):
        if want == 0:
            assert got == 0
            return 0.0
        return abs(got - want) / abs(want)
    worst = 0.0
    for name, values in batch.items():
        worst = max(worst, rel(report["components"][name]["mean_of_batch_means"], float(np.mean(values))))
    for name, col in (("mse", 0), ("kl_mean", 4), ("kl_log", 5), ("triplet_cosine", 10), ("triplet_euclidean", 11), ("contrastive_cosine", 12)):
        worst = max(worst, rel(report["components"][name]["per_image"], float(rows[:, col].mean())))
    want_total = 1.0 * np.mean(batch["mse"]) + 0.01 * np.mean(batch["kl_log"]) + 1.0 * np.mean(batch["triplet_cosine"])
    worst = max(worst, rel(report["val_loss"], want_total))
    print(f"CLI against the loop: max rel {worst:.3e}")
    assert worst <= REL
    assert (report["updates"], report["images"], report["non_finite"], report["recon_images"], report["negative_images"]) == (2, 6, 0, 6, 6)
    assert report["settings"]["seed"] == 7 and report["margin_triplet"] == 0.5 and report["similarity_type"] == "cosine"
    table = json.load(open(tmp / "one" / "per_image.json"))
    assert [e["mse"] for e in table] == sorted((e["mse"] for e in table), reverse=True) and len(table) == 6
    by_path = {e["path"]: e for e in table}
    for k, p in enumerate(paths):
        e = by_path[p]
        assert abs(e["mse"] - rows[k, 0]) <= REL * rows[k, 0] and abs(e["psnr"] - evaluate_vae.psnr(rows[k, 0])) <= 1e-6
        assert (e["positive"], e["negative"]) == (paths[triplets[k][0]], paths[triplets[k][1]])


@pytest.mark.gpu
def test_two_runs_write_identical_bytes_and_the_sweep_ranks_the_perturbed_checkpoint_second(runs):
    tmp = runs["tmp"]
    for name in ("vae_validation_loss.json", "per_image.json"):          # the same checkpoint, data and settings, run again inside the sweep
        assert (tmp / "one" / name).read_bytes() == (tmp / "sweep" / "ckpt_0_good" / name).read_bytes(), name
    sweep = json.load(open(tmp / "sweep" / "checkpoint_sweep.json"))
    assert sweep["ranking"] == [0, 1] and sweep["best_by_val_loss"] == {"index": 0, "path": runs["good"]}
    first, second = sweep["checkpoints"]
    assert second["val_loss"] > first["val_loss"] and second["components"]["mse"]["per_image"] > first["components"]["mse"]["per_image"] + 10.0
    # the encoder is the same: everything but the reconstruction agrees bit for bit
    for name in ("kl_mean", "triplet_cosine", "triplet_euclidean", "contrastive_cosine"):
        assert first["components"][name] == second["components"][name], name
    assert (tmp / "sweep" / "ckpt_1_bad" / "per_image.json").exists()


@pytest.mark.gpu
def test_train_fulls_simplified_total_adds_the_classification_loss_and_decodes_nothing(runs):
    tmp = runs["tmp"]
    one = json.load(open(tmp / "one" / "vae_validation_loss.json"))
    full = json.load(open(tmp / "full" / "vae_validation_loss.json"))
    assert (full["recon_updates"], full["recon_images"]) == (0, 0) and full["components"]["mse"]["mean_of_batch_means"] is None      # no decode
    for name in ("kl_mean", "triplet_cosine", "triplet_euclidean", "contrastive_cosine"):     # the same encoder, seed and margin: the same bits
        assert full["components"][name] == one["components"][name], name
    cls = full["classification"]
    assert cls["selected_loss"] == "focal" and cls["weight"] == 0.5 and cls["class_balanced"] is not None
    focal, bce = cls["focal"]["mean_of_batch_means"], cls["bce"]["mean_of_batch_means"]
    assert 0 < focal < bce and math.isfinite(bce)                        # (1 - pt)^2 < 1 on every element
    want = 2.0 * full["components"]["triplet_cosine"]["mean_of_batch_means"] + 0.5 * focal
    assert abs(full["val_loss"] - want) <= 1e-12 * want and full["val_loss_train_full"] == full["val_loss"]
    table = json.load(open(tmp / "full" / "per_image.json"))
    assert all(e["mse"] is None and e["psnr"] is None for e in table) and [e["position"] for e in table] == list(range(6))      # no reconstruction: the evaluation order stands
