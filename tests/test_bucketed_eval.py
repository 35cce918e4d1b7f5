"""Bucketed data-set evaluation: the bucket feeder's grouping policy, the training-JSON reader and the evaluate CLI's flags (CPU);
feeder equivalence with the reference's CPU transforms and the CLI end to end against host metrics and the CPU oracle (GPU)."""
import inspect
import json

import numpy as np
import pytest
import torch

from vae_tagger_amd import evaluate, infer_full, synth
from vae_tagger_amd.modules import AspectRatioBucketing
from vae_tagger_amd.prefetch import BatchFeeder, BucketGrouper

SMALL = dict(base_resolution=128, max_resolution=256, bucket_step=64)     # nine buckets of 128..256: the CPU oracle stays affordable


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
def test_grouping_policy_full_buckets_cap_and_flush():
    """batch_size 3, at most 4 images waiting.  Arrival order (image number: bucket):
         1:A 2:B 3:A 4:C 5:D   -> five wait: the fullest bucket, A, leaves short           [1, 3]
         6:B 7:B               -> B is full                                                [2, 6, 7]
         8:E 9:A 10:F          -> five wait, every bucket holds one: the oldest, C, leaves [4]
         11:D                  -> five wait: D holds two                                   [5, 11]
         end                   -> flush, oldest first                                      [8] [9] [10]"""
    bk = AspectRatioBucketing()
    size = {"A": [(800, 800), (640, 640), (1000, 1000)], "B": [(1024, 512), (2048, 1024), (1500, 750)], "C": [(512, 1024)],
            "D": [(768, 576), (1024, 768)], "E": [(576, 768)], "F": [(960, 640)]}
    order = "ABACDBBEAFD"
    seen = {k: 0 for k in size}
    arrivals = []
    for n, letter in enumerate(order, start=1):
        w, h = size[letter][seen[letter]]
        seen[letter] += 1
        arrivals.append((f"img{n}.png", (w, h)))
    bucket_of = {p: bk.bucket_for_ratio(w / h) for p, (w, h) in arrivals}
    letters = {letter: {bucket_of[f"img{n}.png"] for n, l in enumerate(order, start=1) if l == letter} for letter in size}
    assert all(len(v) == 1 for v in letters.values())                       # every size of a letter lands in ONE bucket ...
    assert len({next(iter(v)) for v in letters.values()}) == len(size)      # ... and the letters in different ones
    assert bucket_of["img1.png"] == (512, 512) and bucket_of["img2.png"] == (1024, 512) and bucket_of["img5.png"] == (768, 576)

    def run():
        g = BucketGrouper(batch_size=3, max_pending=4)
        out, held = [], []
        for p, (w, h) in arrivals:
            for bucket, group in g.add(p, bk.bucket_for_ratio(w / h), (w, h)):
                out.append((bucket, [k for k, _ in group]))
            held.append(g.count)
        out += [(bucket, [k for k, _ in group]) for bucket, group in g.flush()]
        return out, held, g

    out, held, g = run()
    names = lambda *ns: [f"img{n}.png" for n in ns]
    b = lambda letter: next(iter(letters[letter]))
    assert out == [(b("A"), names(1, 3)), (b("B"), names(2, 6, 7)), (b("C"), names(4)), (b("D"), names(5, 11)), (b("E"), names(8)),
                   (b("A"), names(9)), (b("F"), names(10))]
    assert sorted(k for _, group in out for k in group) == sorted(p for p, _ in arrivals)       # every image once
    assert all(len({bucket_of[k] for k in group}) == 1 and bucket_of[group[0]] == bucket for bucket, group in out)   # single-shape batches
    assert max(held) <= 4 and g.high_water <= 4 and g.count == 0
    assert run()[0] == out                                                                      # a pure function of the arrivals
    # the cap is never below one batch, and the feeder takes the new arguments
    params = inspect.signature(BatchFeeder.__init__).parameters
    assert {"bucketing", "labels", "max_pending"} <= set(params)
    assert all(params[k].default is None for k in ("bucketing", "labels", "max_pending"))


def test_grouping_without_cap_pressure_is_first_come_per_bucket():
    g = BucketGrouper(batch_size=2, max_pending=100)
    out = []
    for n, bucket in enumerate("xyxzzy"):
        out += [(bk, [k for k, _ in grp]) for bk, grp in g.add(n, bucket, None)]
    assert out == [("x", [0, 2]), ("z", [3, 4]), ("y", [1, 5])] and g.flush() == []


def test_dataset_reader(tmp_path):
    from PIL import Image
    for name in ("a.png", "b.png", "c.png", "d.png"):
        Image.new("RGB", (8, 8)).save(tmp_path / name)
    (tmp_path / "tags.csv").write_text("tag_id,name,category\n0,cat,0\n1,dog,0\n2,long hair,0\n3,1girl,4\n")
    data = {str(tmp_path / "a.png"): "cat:1.0, dog:0.25, unicorn:0.9",              # an unknown tag is ignored
            str(tmp_path / "b.png"): "long hair, 1girl:0.5,cat:oops",               # no weight -> 1.0; a weight that does not parse -> 1.0
            str(tmp_path / "c.png"): "dog:0.75",                                    # single entry with a weight
            str(tmp_path / "d.png"): "1girl",                                       # single entry without
            str(tmp_path / "gone.png"): "cat:1.0"}                                  # the file does not exist
    (tmp_path / "data.json").write_text(json.dumps(data))
    ds = evaluate.TaggedImageList(str(tmp_path / "data.json"), str(tmp_path / "tags.csv"))
    assert ds.tags == ["cat", "dog", "long hair", "1girl"]
    assert ds.image_paths == [str(tmp_path / n) for n in ("a.png", "b.png", "c.png", "d.png")] and len(ds) == 4
    assert ds.missing == [str(tmp_path / "gone.png")]
    rows = np.stack([ds.labels[p] for p in ds.image_paths])
    assert rows.dtype == np.float32
    assert np.array_equal(rows, np.array([[1.0, 0.25, 0, 0], [1.0, 0, 1.0, 0.5], [0, 0.75, 0, 0], [0, 0, 0, 1.0]], dtype=np.float32))
    every = evaluate.TaggedImageList(str(tmp_path / "data.json"), str(tmp_path / "tags.csv"), check_files=False)
    assert len(every) == 5 and every.missing == []


def test_evaluate_parser_has_the_reference_flags_and_defaults():
    flags = {o for a in evaluate.build_parser()._actions for o in a.option_strings if o.startswith("--") and o != "--help"}
    ref = {"--vae_checkpoint", "--vae_config_path", "--decoder_checkpoint", "--json_path", "--tags_csv_path", "--output_dir", "--resolution",
           "--use_bucketing", "--base_resolution", "--max_resolution", "--bucket_step", "--use_attention", "--no_attention",
           "--use_spatial_attention", "--use_self_attention", "--use_cross_attention", "--attention_heads", "--attention_dropout"}
    own = {"--batch_size", "--workers", "--host_resize", "--fp16_operands", "--fp8", "--host_metrics", "--threshold", "--max_pending"}
    assert flags == ref | own
    a = evaluate.build_parser().parse_args(["--vae_checkpoint", "v", "--decoder_checkpoint", "d", "--json_path", "j", "--tags_csv_path", "t"])
    # train_decoder.py:290-333
    assert (a.output_dir, a.resolution, a.use_bucketing, a.base_resolution, a.max_resolution, a.bucket_step) == ("decoder_output", 1024, False, 512, 1024, 64)
    assert (a.use_attention, a.no_attention, a.use_spatial_attention, a.use_self_attention, a.use_cross_attention, a.attention_heads,
            a.attention_dropout, a.vae_config_path) == (True, False, True, True, False, 8, 0.1, None)
    assert (a.host_metrics, a.host_resize, a.fp8, a.fp16_operands, a.threshold) == (False, False, False, False, None)
    assert "two" in evaluate.build_parser().format_help().lower()            # the help says that search + metrics are two passes
    # the inference CLIs keep their parsers (tests/test_cli.py pins them): no bucketing flags arrived there
    assert not any("bucket" in o for p in (infer_full.build_parser(),) for a in p._actions for o in a.option_strings)


def test_evaluate_refuses_more_than_one_rank(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    args = evaluate.build_parser().parse_args(["--vae_checkpoint", "v", "--decoder_checkpoint", "d", "--json_path", "j", "--tags_csv_path", "t"])
    with pytest.raises(RuntimeError, match="single process"):
        evaluate.evaluate(args)


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
N_TAGS = 40
SIZES = [(200, 150), (128, 128), (90, 160), (300, 300), (256, 128), (130, 250), (640, 480), (100, 100), (192, 256), (333, 222),
         (150, 200), (257, 255), (512, 256), (64, 128), (240, 180), (180, 240), (1000, 700), (129, 127), (300, 150), (210, 140),
         (140, 210), (97, 193), (256, 256), (400, 300)]


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """24 PNG files of assorted sizes + one broken file, the training JSON, a tag CSV and synthetic checkpoints."""
    from PIL import Image
    from safetensors.torch import save_file
    root = tmp_path_factory.mktemp("bucketed")
    g = torch.Generator().manual_seed(11)
    imgs = root / "imgs"
    imgs.mkdir()
    tags = [f"tag_{i:05d}" for i in range(N_TAGS)]
    data = {}
    for i, (w, h) in enumerate(SIZES):
        arr = (torch.rand(h, w, 3, generator=g) * 255).to(torch.uint8).numpy()
        arr[: h // 2, : w // 3] = 200                                       # some structure: crops and resamples must land on the same pixels
        Image.fromarray(arr).save(imgs / f"img{i:02d}.png")
        picks = torch.randperm(N_TAGS, generator=g)[: 3 + i % 9].tolist()
        data[str(imgs / f"img{i:02d}.png")] = ", ".join(f"{tags[k]}:{0.5 + 0.5 * ((k + i) % 2)}" if k % 3 else tags[k] for k in picks)
        if i == 5:
            (imgs / "broken.png").write_bytes(b"not a png")                 # skip-and-count, in the middle of the list
            data[str(imgs / "broken.png")] = f"{tags[0]}:1.0"
    (root / "data.json").write_text(json.dumps(data))
    (root / "tags.csv").write_text("name\n" + "\n".join(tags) + "\n")
    sd_e = synth.synth_state_dict(synth.encoder_manifest(), seed=0)
    save_file(sd_e, str(root / "vae.safetensors"))
    sd_d = synth.synth_state_dict(synth.attention_decoder_manifest(N_TAGS), seed=1)
    torch.save(sd_d, root / "dec.pth")
    return {"root": root, "paths": list(data), "tags": tags, "sd_e": sd_e, "sd_d": sd_d,
            "argv": ["--vae_checkpoint", str(root / "vae.safetensors"), "--decoder_checkpoint", str(root / "dec.pth"), "--json_path",
                     str(root / "data.json"), "--tags_csv_path", str(root / "tags.csv"), "--resolution", "128", "--use_bucketing",
                     "--base_resolution", "128", "--max_resolution", "256", "--bucket_step", "64", "--batch_size", "4"]}


@pytest.fixture(scope="module")
def models(dataset):
    args = evaluate.build_parser().parse_args(dataset["argv"])
    return infer_full.load_models(args, torch.device("cuda", 0))


@pytest.mark.gpu
def test_bucket_feeder_matches_host_resize_and_per_image_route(dataset, models):
    """BatchFeeder(bucketing=...) on the device route and on the reference's CPU route yield the same names and bit-identical batches,
    each staged by ONE load_batch call; pipe.load_image(img, bucket=...) gives the same pixels; the broken file costs itself only."""
    from PIL import Image
    from vae_tagger_amd.pipeline import EncodeTagPipeline
    pipe = EncodeTagPipeline.input_side(models[0])
    calls = []
    real = pipe.load_batch
    pipe.load_batch = lambda raws, **kw: (calls.append((len(raws), kw.get("bucket"))), real(raws, **kw))[1]
    bk = AspectRatioBucketing(**SMALL)
    labels = {p: np.full(N_TAGS, i, dtype=np.float32) for i, p in enumerate(dataset["paths"])}

    def collect(**kw):
        out, failed = [], []
        for names, x, ready, bad, y in BatchFeeder(pipe, dataset["paths"], 4, 128, workers=3, bucketing=bk, labels=labels, max_pending=8, **kw):
            failed += [p for p, _ in bad]
            if names:
                ready.synchronize()
                out.append((list(names), x.clone(), y.clone()))
        return out, failed

    dev, dev_failed = collect()
    n_dev_calls = len(calls)
    host, host_failed = collect(host_resize=True)
    assert len(calls) == n_dev_calls == len(dev)                     # one load_batch per device-route batch, none on the host route
    assert dev_failed == host_failed == [p for p in dataset["paths"] if p.endswith("broken.png")]
    assert [n for n, _, _ in dev] == [n for n, _, _ in host]
    assert sorted(p for n, _, _ in dev for p in n) == sorted(p for p in dataset["paths"] if not p.endswith("broken.png"))
    buckets = set()
    for (names, x, y), (_, xh, yh), (b, bucket) in zip(dev, host, calls):
        assert x.shape == (len(names), 3, bucket[1], bucket[0]) and b == len(names) <= 4
        assert torch.equal(x, xh.to(x.device)) and torch.equal(y, yh)
        assert torch.equal(y.cpu(), torch.stack([torch.from_numpy(labels[p]) for p in names]))
        for k, p in enumerate(names):
            img = Image.open(p).convert("RGB")
            assert bk.bucket_for_ratio(img.size[0] / img.size[1]) == bucket
            assert torch.equal(pipe.load_image(img, bucket=bucket), x[k]), p
        buckets.add(bucket)
    assert len(buckets) >= 3
    # the same arrivals through the policy alone give the same batches
    g = BucketGrouper(4, 8)
    want = []
    for p in dataset["paths"]:
        if p.endswith("broken.png"):
            continue
        w, h = Image.open(p).size
        want += [[k for k, _ in grp] for _, grp in g.add(p, bk.bucket_for_ratio(w / h), None)]
    want += [[k for k, _ in grp] for _, grp in g.flush()]
    assert [n for n, _, _ in dev] == want


COUNT_KEYS = ("accuracy", "hamming_loss", "precision_micro", "precision_macro", "precision_weighted", "recall_micro", "recall_macro",
              "recall_weighted", "f1_micro", "f1_macro", "f1_weighted")
AP_KEYS = ("mAP", "mAP_micro", "mAP_weighted")


def _same_metrics(got, want):
    for k in COUNT_KEYS:
        assert got[k] == want[k], (k, got[k], want[k])
    for k in AP_KEYS:
        assert abs(got[k] - want[k]) <= 1e-9, (k, got[k], want[k])
    assert list(got["per_class"]) == list(want["per_class"])
    for name, w in want["per_class"].items():
        g = got["per_class"][name]
        assert (g["precision"], g["recall"], g["f1"], g["support"]) == (w["precision"], w["recall"], w["f1"], w["support"]), name
        assert abs(g["ap"] - w["ap"]) <= 1e-9, name


def _read_outputs(d):
    rows = [line.split(",") for line in (d / "evaluation_results.csv").read_text().strip().split("\n")]
    per_class = {r[0]: {"precision": float(r[1]), "recall": float(r[2]), "f1": float(r[3]), "ap": float(r[4]), "support": int(r[5])} for r in rows[1:]}
    overall = json.loads((d / "evaluation_results_overall.json").read_text())
    return json.loads((d / "optimal_thresholds.json").read_text()), dict(overall, per_class=per_class)


@pytest.mark.gpu
def test_evaluate_cli_end_to_end_bucketed(dataset, models):
    from PIL import Image
    from oracle import decoder_ref, encoder_ref
    from vae_tagger_amd.evaluation import evaluate_model, find_optimal_threshold
    from vae_tagger_amd.modules import get_image_transform
    from vae_tagger_amd.pipeline import EncodeTagPipeline
    root = dataset["root"]
    res = evaluate.main(dataset["argv"] + ["--output_dir", str(root / "out")])
    batches = list(evaluate.LAST_RUN_STATS["batches"])
    assert res["skipped"] == 1 and evaluate.LAST_RUN_STATS["passes"] == 2
    assert sum(len(n) for n, _ in batches) == len(SIZES) and len({s[2:] for _, s in batches}) >= 3
    thr_file, metrics_file = _read_outputs(root / "out")
    assert thr_file == res["optimal_thresholds"] and thr_file["global_threshold"] == res["threshold"]
    _same_metrics(metrics_file, res["metrics"])

    # (a) host metrics over the SAME batches, built image by image through load_image by a plain loop
    vae_model, decoder, tags = models
    pipe = EncodeTagPipeline.input_side(vae_model)
    ds = evaluate.TaggedImageList(str(root / "data.json"), str(root / "tags.csv"))
    loop = []
    for names, shape in batches:
        bucket = (shape[3], shape[2])
        x = torch.stack([pipe.load_image(Image.open(p).convert("RGB"), bucket=bucket) for p in names])
        loop.append({"pixel_values": x, "labels": torch.from_numpy(np.stack([ds.labels[p] for p in names]))})
    host_thr = find_optimal_threshold(vae_model, decoder, loop, tags, "cuda:0", None, device_metrics=False)
    assert host_thr == res["optimal_thresholds"]
    host_metrics = evaluate_model(vae_model, decoder, loop, tags, "cuda:0", host_thr["global_threshold"], None, device_metrics=False)
    _same_metrics(res["metrics"], host_metrics)

    # (b) one image of every bucket used: logits within 1e-2 of the CPU oracle on the reference's own transform of that image
    seen = {}
    for names, shape in batches:
        seen.setdefault((shape[3], shape[2]), names[0])
    assert len(seen) >= 3
    for bucket, p in seen.items():
        img = Image.open(p).convert("RGB")
        x_ref = get_image_transform(128, True, bucket)(img)[None]
        ref_logits = decoder_ref.attention_decoder_forward(dataset["sd_d"], encoder_ref.vae_wrapper_encode(dataset["sd_e"], x_ref))
        x = pipe.load_batch([torch.from_numpy(np.asarray(img).copy()).cuda()], bucket=bucket)
        assert torch.equal(x.cpu(), x_ref)
        logits = decoder(vae_model.encode(x)).cpu()
        d = (logits - ref_logits).abs().max().item()
        print(f"bucket {bucket}: max |dlogit| = {d:.3e}")
        assert d <= 1e-2, (bucket, p, d)

    # (c) --host_metrics, the reference's CPU input route, and --threshold (one pass) write the same files
    for extra in (["--host_metrics"], ["--host_resize"], ["--host_metrics", "--host_resize", "--workers", "2"]):
        alt = evaluate.main(dataset["argv"] + ["--output_dir", str(root / "out_alt")] + extra)
        assert evaluate.LAST_RUN_STATS["batches"] == batches, extra
        thr_alt, metrics_alt = _read_outputs(root / "out_alt")
        assert thr_alt == thr_file == alt["optimal_thresholds"], extra
        _same_metrics(metrics_alt, metrics_file)
    one = evaluate.main(dataset["argv"] + ["--output_dir", str(root / "out_one"), "--threshold", str(res["threshold"])])
    assert evaluate.LAST_RUN_STATS["passes"] == 1 and one["optimal_thresholds"] is None
    assert not (root / "out_one" / "optimal_thresholds.json").exists()
    _same_metrics(_read_outputs_no_thr(root / "out_one"), metrics_file)


def _read_outputs_no_thr(d):
    (d / "optimal_thresholds.json").write_text("{}")
    return _read_outputs(d)[1]


@pytest.mark.gpu
def test_evaluate_cli_square_route(dataset, models):
    """Without --use_bucketing the CLI squashes to --resolution squared (the inference CLIs' route): same files with --host_resize."""
    root = dataset["root"]
    argv = [a for a in dataset["argv"] if a != "--use_bucketing"]
    res = evaluate.main(argv + ["--output_dir", str(root / "sq")])
    shapes = [s for _, s in evaluate.LAST_RUN_STATS["batches"]]
    assert all(s[1:] == (3, 128, 128) for s in shapes) and sum(s[0] for s in shapes) == len(SIZES) and res["skipped"] == 1
    alt = evaluate.main(argv + ["--output_dir", str(root / "sq_alt"), "--host_resize"])
    assert alt["optimal_thresholds"] == res["optimal_thresholds"]
    _same_metrics(_read_outputs(root / "sq_alt")[1], _read_outputs(root / "sq")[1])
