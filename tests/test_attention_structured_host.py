"""The constructions of _attention_cases.py, checked without a GPU: the operands are exact in bf16 and e4m3, fp64 softmax attention of
them IS the closed form, mode 0's norm-bound gap falls on the side of 120 each family is built for, and every kernel mistake a family
is meant to catch moves the fp64 reference by more than 4 x the tolerance the device test allows (so the device test cannot pass
with that mistake in a kernel)."""
import pytest
import torch

import _attention_cases as ac

CASES = [(f, B, S) for f in ac.FAMILIES for (B, S) in ac.SHAPES_ALL]


@pytest.fixture(scope="module")
def refs():
    """fp64 reference per case, computed once and shared"""
    cache = {}

    def get(family, B, S):
        if (family, B, S) not in cache:
            cache[(family, B, S)] = ac.reference(ac.make_case(family, B, S))
        return cache[(family, B, S)]
    return get


def test_weights_replace_only_the_attention_tensors():
    from vae_tagger_amd import synth
    sd = synth.synth_state_dict(synth.encoder_manifest(), seed=0)
    new = ac.attention_weights(sd)
    changed = {k for k in sd if not torch.equal(sd[k], new[k])}
    assert set(new) == set(sd)
    assert changed == {ac.A + n + s for n in ("to_q", "to_k", "to_v", "to_out.0") for s in (".weight", ".bias")}
    for n in ("to_q", "to_k", "to_v", "to_out.0"):
        assert not new[ac.A + n + ".bias"].any() and ac.exactly_representable(new[ac.A + n + ".weight"])
    assert int((new[ac.A + "to_q.weight"] != 0).sum()) == 128 and int((new[ac.A + "to_v.weight"] != 0).sum()) == 256


@pytest.mark.parametrize("family,B,S", CASES)
def test_operands_are_exact_in_bf16_and_e4m3(family, B, S):
    c = ac.make_case(family, B, S)
    q, k, v = ac.operands(c, torch.float32)
    for name, t in (("x", c.x), ("q", q), ("k", k), ("v", v)):
        assert ac.exactly_representable(t), name
    amp = ac.AMPLITUDE[family]
    if amp is not None:                       # q = 8 qcode, k = 8 kcode, v = payload: independent per token
        assert set(q.unique().tolist()) == {0.0, 8 * amp} and set(k.unique().tolist()) == {0.0, 8 * amp}
        assert torch.equal((q != 0).sum(-1), torch.full((B, S), 2)) and torch.equal((k != 0).sum(-1), torch.full((B, S), 2))
    assert torch.equal(v[:, :, :ac.PAYLOAD], c.payload) and not v[:, :, ac.PAYLOAD:].any()
    assert c.payload.abs().max().item() <= ac.PAYLOAD_MAX and torch.equal(c.payload * 2, (c.payload * 2).round())
    b = torch.arange(B).float()
    assert torch.equal(c.payload[:, 0, ac.TAG[0]] * 20 + c.payload[:, 0, ac.TAG[1]] * 2, b + 11)     # the tag names the image
    if family == "allneg":
        assert c.payload.min().item() >= 0.5


@pytest.mark.parametrize("family,B,S", CASES)
def test_fp64_attention_is_the_closed_form(refs, family, B, S):
    c = ac.make_case(family, B, S)
    ref = refs(family, B, S)
    err = (ref - c.expected).abs().max().item()
    print(f"{family} B={B} S={S}: max|fp64 softmax attention - closed form| = {err:.3e}")
    assert err <= 1e-12
    if family == "select" and S > 128:        # the keys either side of the tile boundaries are selected, the ends crosswise
        assert c.sel[0, 0] == S - 1 and c.sel[0, S - 1] == 0 and c.sel[0, 1:7].tolist() == [31, 32, 63, 64, 127, 128]
    if family == "avg4":
        want = [p for p in (0, 63, 64, S - 1) if p < S]
        assert all(set(want) <= set(g[0].tolist()) for g in c.groups)
        if S >= 1024:
            assert all(sorted(int(p) * 4 // S for p in g[1]) == [0, 1, 2, 3] for g in c.groups)


@pytest.mark.parametrize("family,B,S", CASES)
def test_norm_bound_gap_is_on_the_side_the_family_is_built_for(family, B, S):
    gap = ac.shift_gap(ac.make_case(family, B, S))
    if family == "select_loose":
        assert (gap.max(dim=1).values > ac.MAX_GAP).all()        # every image raises its group's flag
    else:
        assert gap.max().item() <= ac.MAX_GAP
    if family == "allneg":
        assert abs(gap.max().item() - 45.26) < 0.01


@pytest.mark.parametrize("family,B,S", CASES)
def test_each_kernel_mistake_moves_the_reference_past_the_device_tolerance(refs, family, B, S):
    c = ac.make_case(family, B, S)
    ref, tol = refs(family, B, S), ac.tolerance(c)
    muts = ac.mutations_of(c)
    assert muts
    for m in muts:
        d = (ac.reference(c, m) - ref).abs().max().item()
        print(f"{family} B={B} S={S} {m}: max|d| = {d:.3f} = {d / tol:.0f} x the device tolerance {tol:.4f}")
        assert d > 4 * tol, m
    if family in ("select", "select_loose"):
        # documented blind spot: a selection of one key keeps weight 1 when its tile is counted twice in BOTH sums -- avg4's job
        assert (ac.reference(c, "tile0_twice") - ref).abs().max().item() <= 1e-12
