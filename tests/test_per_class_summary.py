"""vt_summarize_confidence_per_class against its host reference (infer_full.summarize_per_class), and `infer_full --thresholds_json` end to
end on the serial and the pipelined loop.  Confidences and indices are copied, not computed, by the summary: exact comparisons."""
import json

import numpy as np
import pytest
import torch

from vae_tagger_amd import infer_full, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pipe():
    from vae_tagger_amd.diffusers_vae_loader import DiffusersVAEWrapper, get_diffusers_vae_config, load_diffusers_vae_from_config
    from vae_tagger_amd.modules import create_attention_decoder
    from vae_tagger_amd.pipeline import EncodeTagPipeline
    vae = load_diffusers_vae_from_config(get_diffusers_vae_config())
    vae.load_state_dict(synth.synth_state_dict(synth.encoder_manifest(), seed=0), strict=False)
    dec = create_attention_decoder(16, 16, 16, 11, {"use_spatial_attention": True, "use_self_attention": True})
    dec.load_state_dict(synth.synth_state_dict(synth.attention_decoder_manifest(11), seed=1), strict=False)
    return EncodeTagPipeline(DiffusersVAEWrapper(vae).to("cuda").eval(), dec.to("cuda").eval())


def _reference(conf, idx, thr, K):
    """Host model of the entry point: first K passing pairs in sorted order (0 / -1 behind them), stats as documented."""
    B, N = conf.shape
    tc, ti, st = np.zeros((B, K), np.float32), np.full((B, K), -1, np.int32), np.zeros((B, 4), np.float32)
    for b in range(B):
        keep = conf[b] >= thr[idx[b]]                         # NaN fails
        cs, ix = conf[b][keep], idx[b][keep]
        m = min(K, len(cs))
        tc[b, :m], ti[b, :m] = cs[:m], ix[:m]
        s5 = np.float32(0)
        for v in conf[b, :5]:
            s5 = np.float32(s5 + v)
        st[b] = (len(cs), conf[b, 0], s5 / np.float32(5), (~np.isfinite(conf[b])).sum())
    return tc, ti, st


@pytest.mark.parametrize("N", [11, 10000, 70001])
@pytest.mark.parametrize("B", [1, 16])
def test_per_class_summary_equals_the_host_reference(pipe, N, B):
    g = torch.Generator().manual_seed(N + B)
    logits = torch.randn(B, N, generator=g) * 2
    logits = (logits * 4).round() / 4                         # heavy ties
    if B > 1:
        logits[1, :: 3] = float("nan")                        # a row with NaN confidences: they sort last and never pass
    conf, idx = pipe.confidence(logits.cuda())
    rng = np.random.default_rng(N)
    c_host, i_host = conf.cpu().numpy(), idx.cpu().numpy()
    finite = c_host[0][np.isfinite(c_host[0])]
    vectors = {"random": rng.random(N).astype(np.float32),
               "on the values": rng.choice(finite, size=N).astype(np.float32),         # confidence == threshold passes (>=)
               "few pass": np.full(N, 2.0, np.float32), "all equal": np.full(N, np.float32(0.5))}
    vectors["few pass"][i_host[0][[0, min(7, N - 1), N - 1]]] = 0.0                   # the best, a middle and the LAST-ranked tag pass
    for name, vec in vectors.items():
        thr = torch.from_numpy(vec).cuda()
        for K in (5, 64, min(N, 300)):
            tc, ti, st = pipe.summarize(conf, idx, thr, K)
            K = tc.shape[1]
            wc, wi, ws = _reference(c_host, i_host, vec, K)
            assert np.array_equal(st[:, 0], ws[:, 0]) and np.array_equal(st[:, 3], ws[:, 3]), (name, K)
            assert np.array_equal(st[:, 1:3], ws[:, 1:3], equal_nan=True), (name, K)
            assert np.array_equal(ti, wi) and np.array_equal(tc, wc), (name, K)
            if name == "few pass":
                assert st[0, 0] == 3 and ti[0, 2] == i_host[0, N - 1]
            if name == "all equal":                            # the scalar entry point at that threshold: same stats, same passing pairs
                sc, si, ss = pipe.summarize(conf, idx, 0.5, K)
                assert np.array_equal(ss, st, equal_nan=True)
                for b in range(B):
                    m = min(int(st[b, 0]), K)
                    assert np.array_equal(sc[b, :m], tc[b, :m]) and np.array_equal(si[b, :m], ti[b, :m])
        # the JSON entries, through the path the CLI takes (a row with more than K passing tags is fetched whole and filtered on the host)
        rows = [b for b in range(B) if np.isfinite(c_host[b]).all()]
        tags = [f"t{i}" for i in range(N)]
        entries = infer_full._entries_from_summary(pipe.summarize(conf[rows], idx[rows], thr, 8), conf[rows], idx[rows], tags, class_thresholds=vec)
        assert entries == [infer_full.summarize_per_class(c_host[b], i_host[b], tags, vec) for b in rows], name
    with pytest.raises(ValueError):
        pipe.summarize(conf, idx, torch.zeros(N + 1, device="cuda"), 8)


def test_infer_full_with_thresholds_json_serial_and_pipelined(tmp_path):
    from PIL import Image
    from safetensors.torch import save_file
    n_tags, res = 40, 128
    g = torch.Generator().manual_seed(5)
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    for i, size in enumerate([(200, 150), (128, 128), (90, 160), (160, 90), (256, 256)]):
        Image.fromarray((torch.rand(size[1], size[0], 3, generator=g) * 255).to(torch.uint8).numpy()).save(imgs / f"img{i}.png")
    save_file(synth.synth_state_dict(synth.encoder_manifest(), seed=0), str(tmp_path / "vae.safetensors"))
    torch.save(synth.synth_state_dict(synth.attention_decoder_manifest(n_tags), seed=1), tmp_path / "dec.pth")
    tags = [f"tag_{i:05d}" for i in range(n_tags)]
    (tmp_path / "tags.csv").write_text("name\n" + "\n".join(tags) + "\n")
    rng = np.random.default_rng(1)
    per_class = {t: {"threshold": float(rng.choice([0.2, 0.45, 0.5, 0.55, 0.8])), "f1_score": 0.0} for t in tags[:30]}    # ten tags fall back
    (tmp_path / "thr.json").write_text(json.dumps({"global_threshold": 0.5, "global_f1": 0.0, "per_class_thresholds": per_class}))
    common = ["--vae_checkpoint", str(tmp_path / "vae.safetensors"), "--decoder_checkpoint", str(tmp_path / "dec.pth"), "--image_path", str(imgs),
              "--tags_csv_path", str(tmp_path / "tags.csv"), "--resolution", str(res), "--confidence_threshold", "0.52", "--batch_size", "2"]
    # the confidences of the same run: every tag listed (threshold 0)
    every = infer_full.main(common[:-4] + ["--confidence_threshold", "0.0", "--batch_size", "2", "--output_dir", str(tmp_path / "all")])
    vec = infer_full.load_class_thresholds(str(tmp_path / "thr.json"), tags, 0.52)
    assert (vec[30:] == np.float32(0.52)).all()
    runs = {}
    for name, extra in (("pipelined", []), ("serial", ["--serial"])):
        runs[name] = infer_full.main(common + ["--thresholds_json", str(tmp_path / "thr.json"), "--output_dir", str(tmp_path / name)] + extra)
        assert json.loads((tmp_path / name / "classification_results.json").read_text()) == runs[name]
    assert runs["serial"] == runs["pipelined"] and len(runs["serial"]) == 5
    scalar = infer_full.main(common + ["--output_dir", str(tmp_path / "scalar")])
    assert scalar != runs["serial"]
    for path, entry in runs["serial"].items():
        full = every[path]
        assert full["total_tags_above_threshold"] == n_tags
        assert entry["max_confidence"] == full["max_confidence"] and entry["avg_confidence_top5"] == full["avg_confidence_top5"]
        assert entry["total_tags_above_threshold"] == len(entry["predicted_tags"])
        order = [t["tag"] for t in full["predicted_tags"]]
        got = [t["tag"] for t in entry["predicted_tags"]]
        assert got == [t for t in order if t in set(got)]                  # sorted order is kept
        for t in full["predicted_tags"]:
            thr = float(vec[tags.index(t["tag"])])
            if abs(t["confidence"] - thr) > 1e-4:                          # (4-digit rounding of the listed confidence: away from the edge the decision is known)
                assert (t["tag"] in set(got)) == (t["confidence"] >= thr), (path, t, thr)
        assert all(t in full["predicted_tags"] for t in entry["predicted_tags"])
