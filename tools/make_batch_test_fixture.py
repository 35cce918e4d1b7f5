#!/usr/bin/env python3
"""Writes tests/golden/batch_test_reference.json: seeded synthetic predictions and ground truth (40 images, 11 tags) and what the
REFERENCE's calculate_metrics (batch_inference_test.py:63-137) makes of them.  Runs on the CPU; the reference tree is imported at
generation time only -- the fixture holds data, no program text:

    python tools/make_batch_test_fixture.py --reference_dir /path/to/vae-tagger

The inputs cover: images with no true tag, images with no prediction, ground-truth tags that are not in the tag list, a duplicated
ground-truth tag, and confidences exactly on the threshold (predicted under the reference's `>=`)."""
import argparse
import contextlib
import importlib.util
import io
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_IMAGES, N_TAGS, THRESHOLD = 40, 11, 0.5


def build_inputs(seed=20240917):
    rng = np.random.default_rng(seed)
    tags = [f"tag_{k:02d}" for k in range(N_TAGS)]
    images = []
    for i in range(N_IMAGES):
        conf = rng.random(N_TAGS).astype(np.float32)
        picks = [tags[k] for k in np.flatnonzero(rng.random(N_TAGS) < 0.3)]
        if i % 7 == 3:
            picks = []                                      # no true tag: recall 1
        if i % 9 == 4:
            conf = (conf * np.float32(0.25)).astype(np.float32)          # nothing reaches the threshold: precision 0
        if i % 5 == 1:
            picks += [f"unknown_{i}", "unknown_shared"][: 1 + i % 2]     # ground truth outside the tag list
        if i % 8 == 2 and picks:
            picks.append(picks[0])                          # a duplicate: the reference counts the SET
        if i % 6 == 0:
            conf[i % N_TAGS] = np.float32(THRESHOLD)        # exactly on the threshold: predicted under >=, not under >
        if i % 10 == 5:
            conf[(i + 3) % N_TAGS] = np.nextafter(np.float32(THRESHOLD), np.float32(1))   # the smallest fp32 above the threshold ...
            conf[(i + 4) % N_TAGS] = np.nextafter(np.float32(THRESHOLD), np.float32(0))   # ... and the largest below
        if i == 12:
            picks = [tags[k] for k in np.flatnonzero(conf.astype(np.float64) >= THRESHOLD)]   # an exact match
        images.append({"image": f"img_{i:03d}.jpg", "confidences": [float(c) for c in conf], "true_tags": picks})
    return {"tags": tags, "threshold": THRESHOLD, "rule": "ge", "images": images}


def reference_metrics(reference_dir, inputs):
    spec = importlib.util.spec_from_file_location("reference_batch_inference_test", os.path.join(reference_dir, "batch_inference_test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    tags, thr = inputs["tags"], inputs["threshold"]
    predictions, ground_truth = {}, {}
    for im in inputs["images"]:
        conf = np.asarray(im["confidences"], dtype=np.float32)
        order = np.argsort(-conf, kind="stable")
        # infer_full.py: conf_value = sorted_conf[j].item(); if conf_value >= args.confidence_threshold
        predicted = [{"tag": tags[k], "confidence": float(f"{float(conf[k]):.4f}")} for k in order if float(conf[k]) >= thr]
        predictions[f"some/dir/{im['image']}"] = {"predicted_tags": predicted}
        ground_truth[f"dataset/images/{im['image']}"] = list(im["true_tags"])
    with contextlib.redirect_stdout(io.StringIO()):
        return mod.calculate_metrics(predictions, ground_truth)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference_dir", required=True, help="a checkout of the reference project (read at generation time only)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "batch_test_reference.json"))
    args = ap.parse_args()
    inputs = build_inputs()
    inputs["reference"] = reference_metrics(args.reference_dir, inputs)
    with open(args.out, "w", encoding="utf-8") as fh:
        json.dump(inputs, fh, indent=1)
        fh.write("\n")
    print(f"{args.out}: {os.path.getsize(args.out)} bytes, {len(inputs['images'])} images")


if __name__ == "__main__":
    main()
