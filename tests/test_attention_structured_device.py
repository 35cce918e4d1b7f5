"""vt_op_attention on inputs whose softmax is known by construction (_attention_cases.py): every query's row is a selection of one key,
an equal-weight average of four, or the plain mean of all S, so a wrong, dropped, duplicated, leaked or foreign key moves the output
by O(1) of the value scale -- against a bound of a few bf16 ulps that is derived, not observed (_attention_cases.tolerance).  The
dense random cases of test_gpu_e2e.py hold the arithmetic; these hold the indexing: key <-> value maps, fragment order, tile and
segment boundaries, the ragged tail mask, cross-image reads, on every route of run_attention (dedicated kernels, generic GEMMs,
softmax pass, e4m3), then on a workspace full of NaN between guard bands, and last which kernel each route launches.
test_attention_structured_host.py shows, without a GPU, that each mistake a family is built for is > 4 x the bound away."""
import ctypes

import pytest
import torch

import _attention_cases as ac
from _util import Guarded, vp

pytestmark = pytest.mark.gpu

DEFAULT_FLAGS = {7: 0, 9: 1, 11: 0, 12: 1, 14: 1, 15: 1, 17: 1}
BF16_ROUTES = [({9: qk, 12: pv, 7: mode}, f"bf16 {name} mode {mode}")
               for (qk, pv, name) in ((1, 1, "qk+pv kernels"), (1, 0, "qk kernel + gemm pv"), (0, 0, "gemm")) for mode in (0, 1, 2)]
BF16_ROUTES.insert(1, ({17: 0}, "bf16 qk+pv kernels mode 0, gemm projections"))
FP8_ROUTES = [({11: 1, 15: f15, 14: 1, 7: mode}, f"fp8 {'e4m3' if f15 else 'bf16'} projections mode {mode}") for f15 in (1, 0) for mode in (0, 1)]


@pytest.fixture(scope="module")
def attn():
    """one context per module: the FLUX configuration (C = 512), the synthetic state dict with the mid-block attention replaced"""
    from vae_tagger_amd import synth
    from vae_tagger_amd.diffusers_vae_loader import get_diffusers_vae_config, load_diffusers_vae_from_config
    m = load_diffusers_vae_from_config(get_diffusers_vae_config())
    missing, unexpected = m.load_state_dict(ac.attention_weights(synth.synth_state_dict(synth.encoder_manifest(), seed=0)), strict=False)
    assert not missing and not unexpected
    m = m.to("cuda").eval()
    return m, m._context()


@pytest.fixture(scope="module")
def refs():
    """fp64 softmax attention of each case's operands on the CPU: computed once, shared by the tests, never modified"""
    cache = {}

    def get(case):
        key = (case.family, case.B, case.S)
        if key not in cache:
            ref = ac.reference(case)
            assert (ref - case.expected).abs().max().item() <= 1e-12
            cache[key] = ref
        return cache[key]
    return get


class flags:
    """set the given vt_set_flag values, put every attention flag back on the way out"""

    def __init__(self, ctx, values):
        self.ctx, self.values = ctx, values

    def __enter__(self):
        for f, v in self.values.items():
            self.ctx.call("vt_set_flag", f, v)

    def __exit__(self, *exc):
        for f, v in DEFAULT_FLAGS.items():
            self.ctx.call("vt_set_flag", f, v)


def run(ctx, case, ws_ptr):
    """one vt_op_attention call on a NaN-prefilled output -> the output on the CPU"""
    B, S = case.B, case.S
    xd, rd = case.x.bfloat16().cuda(), case.res.cuda()
    out = torch.full((B, S, ac.C), float("nan"), device="cuda")
    ctx.call("vt_op_attention", vp(xd), vp(rd), vp(out), B, S, ac.C, ws_ptr, ctypes.c_void_p(0))
    torch.cuda.synchronize()
    return out.cpu()


def check_routes(ctx, case, ref, routes):
    """run the case on every route, print one line per route, -> {label: output}; fails after the last line if any route missed"""
    ws = torch.empty(ctx.lib.vt_op_attention_workspace_bytes(case.B, case.S, ac.C), dtype=torch.uint8, device="cuda")
    tol, outs, bad = ac.tolerance(case), {}, []
    for values, label in routes:
        with flags(ctx, values):
            out = run(ctx, case, vp(ws))
            st = ctx.status()
        outs[label] = out
        finite = bool(torch.isfinite(out).all())
        d = (out.double() - ref).abs()
        err = d.max().item() if finite else float("nan")
        print(f"{case.family} B={case.B} S={case.S} {label}: max|out - fp64 ref| = {err:.3e} = {err / tol:.3f} x the bound {tol:.4e}; status {st}")
        if st != 0 or not finite or not err <= tol:
            rows = (d.amax(dim=-1) > tol).nonzero()
            bad.append((label, st, finite, err, f"{len(rows)} rows off, first (image, query): {rows[:8].tolist()}"))
        elif case.family != "allneg":
            # the tag channels come back as the row's own image, exactly (a multiple of 0.5 plus a multiple of 0.25: bf16 holds it, fp32 adds it)
            tag = out[:, :, list(ac.TAG)] - case.res[:, :, list(ac.TAG)]
            if not torch.equal(tag, case.payload[:, :, list(ac.TAG)]):
                bad.append((label, "tag channels name another image"))
    assert not bad, bad
    return outs


@pytest.mark.parametrize("B,S", ac.SHAPES_BF16)
@pytest.mark.parametrize("family", ac.FAMILIES)
def test_structured_attention_bf16(attn, refs, family, B, S):
    """(flag 9, flag 12) in {(1, 1), (1, 0), (0, 0)} x flag 7 in {0, 1, 2}, and flag 17 = 0 once on the default route.  select_loose:
    u - l > 120 raises the group flag, so mode 0 takes the exact maximum and is bit-identical to mode 1 on each route."""
    _, ctx = attn
    case = ac.make_case(family, B, S)
    outs = check_routes(ctx, case, refs(case), BF16_ROUTES)
    if family == "select_loose":           # (the exact families give no "differs when not flagged" check: both shifts round to the same exact output)
        for name in ("qk+pv kernels", "qk kernel + gemm pv", "gemm"):
            assert torch.equal(outs[f"bf16 {name} mode 0"], outs[f"bf16 {name} mode 1"]), name


@pytest.mark.parametrize("B,S", ac.SHAPES_FP8)
@pytest.mark.parametrize("family", ac.FAMILIES)
def test_structured_attention_fp8(attn, refs, family, B, S):
    """flag 11 with flag 15 in {1, 0} x flag 7 in {0, 1}.  The operands are exact in e4m3 and the numerators all equal or single, so the
    e4m3 kernels owe the same result as the bf16 ones.  Below 16 key tiles (S < 1921) mode 0's first sweep takes every tile: bit-identical
    to mode 1; from 16 tiles it samples every 4th and redoes a group whose numerators passed 448 (select: the sampled tiles miss most
    selected keys by 45 or 90 nats)."""
    _, ctx = attn
    case = ac.make_case(family, B, S)
    outs = check_routes(ctx, case, refs(case), FP8_ROUTES)
    if S < 1921:
        for p in ("e4m3", "bf16"):
            assert torch.equal(outs[f"fp8 {p} projections mode 0"], outs[f"fp8 {p} projections mode 1"]), p


WS_ROUTES = [BF16_ROUTES[0], ({9: 1, 12: 0}, "bf16 qk kernel + gemm pv mode 0"), ({9: 0, 12: 0}, "bf16 gemm mode 0"), FP8_ROUTES[0], FP8_ROUTES[2]]


@pytest.mark.parametrize("B,S", ac.RAGGED)
@pytest.mark.parametrize("family", ["select", "allneg"])
def test_attention_does_not_depend_on_what_its_workspace_held(attn, refs, family, B, S):
    """The ragged shapes on a workspace between guard bands with every byte 0xFF (a NaN in fp32, fp16, bf16 and e4m3), then on a zeroed one
    of the same size: the same bits, finite everywhere, the bands intact.  A pad row or column that a kernel multiplies without having
    written it shows as NaN (0 x NaN) or as a difference.  (Nothing in the workspace is an index, flag or address before the call writes
    it: the group flags are cleared by the call in the modes that gate on them and the gates are null otherwise -- run_attention.)"""
    _, ctx = attn
    case = ac.make_case(family, B, S)
    ref, tol = refs(case), ac.tolerance(case)
    n = ctx.lib.vt_op_attention_workspace_bytes(B, S, ac.C)
    for values, label in WS_ROUTES:
        got = []
        for fill in (0xFF, 0x00):
            ws = Guarded(n, torch.device("cuda"))
            if fill == 0:
                ws.body().zero_()
            with flags(ctx, values):
                got.append(run(ctx, case, ws.ptr))
                st = ctx.status()
            assert st == 0 and ws.guards_intact(), (label, hex(fill), st)
            assert torch.isfinite(got[-1]).all(), (label, hex(fill))
        assert torch.equal(got[0], got[1]), label
        assert (got[0].double() - ref).abs().max().item() <= tol, label


def test_routes_launch_the_kernels_their_labels_name(attn):
    """Which kernel took the launches of one call, from the library's profiler slots selected by the kernel names vt_profile_end returns:
    the route labels printed above are only worth their names if flags 9 / 12 / 17 / 11 / 15 move the launches the way run_attention says."""
    _, ctx = attn
    case = ac.make_case("select", 3, 130)
    n = ctx.lib.vt_profile_num_configs()
    ws = torch.empty(ctx.lib.vt_op_attention_workspace_bytes(case.B, case.S, ac.C), dtype=torch.uint8, device="cuda")

    def launches(values):
        la, ms, fl, nm = (ctypes.c_longlong * n)(), (ctypes.c_double * n)(), (ctypes.c_double * n)(), (ctypes.c_char_p * n)()
        with flags(ctx, values):
            ctx.call("vt_profile_begin")
            try:
                run(ctx, case, vp(ws))
            finally:
                ctx.call("vt_profile_end", n, la, ms, fl, nm)
        got = {}
        for i in range(n):
            if la[i]:
                name = nm[i].decode()
                name = "gemm" if name.startswith("conv_gemm_kernel<") else name
                got[name] = got.get(name, 0) + la[i]
        return got

    QK, PV, PROJ = "attn_qk_kernel", "attn_pv_kernel", "attn_qk_kernel<4> (projections)"
    # default: q | k, v^T and the output projection on the skeleton, one Q.K^T numerator sweep (the row-maximum sweep is gated, not counted), one P.V
    assert launches({}) == {PROJ: 3, QK: 1, PV: 1}
    assert launches({7: 1}) == {PROJ: 3, QK: 1, PV: 1}
    assert launches({17: 0}) == {"gemm": 3, QK: 1, PV: 1}
    assert launches({12: 0}) == {PROJ: 3, QK: 1, "gemm": 1}
    got = launches({9: 0, 12: 0})                 # nothing on attn_qk.hip / attn_pv.hip: projections, numerators, P.V, output projection
    assert set(got) == {"gemm"} and got["gemm"] >= 5, got
    got = launches({7: 2})                        # the softmax-pass route: scores and P.V on the generic GEMM, projections on the skeleton
    assert got == {PROJ: 3, "gemm": 2}, got
    assert launches({11: 1}) == {"proj_fp8_kernel": 2, "attn_qk_fp8_kernel": 1, "attn_pv_fp8_kernel": 1, PROJ: 1}
    assert launches({11: 1, 15: 0}) == {PROJ: 3, "attn_qk_fp8_kernel": 1, "attn_pv_fp8_kernel": 1}
    assert launches({11: 1, 14: 0}) == {PROJ: 3, QK: 1, PV: 1}
