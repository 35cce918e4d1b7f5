"""GPU: the resnet-block forms of the 3x3 conv kernels, one operator at a time, through vt_op_conv3x3_block -- the schedules' own dispatcher
(run_conv) and weight packers: fused shortcut, fp16 residual stream, 16-bit operand copy (bf16 / fp16 bits, NHWC / chunk-planar), GroupNorm
partials, on every tile of vt_launch_conv3x3_halo's switch that takes plain input, the stride-2 phase-plane kernel and the generic GEMM.
Reference: tests/_conv_block_ref.py (fp64, checked on the CPU by test_conv_block_host.py) on the same pre-rounded operands, so the parity rule
is test_conv2d_matches_torch's (accumulation-order noise: rtol 1e-4, atol 2e-4) and the GroupNorm rule test_conv_epilogue_groupnorm_statistics'
(rtol 1e-3, atol 1e-3 on the normalised tensor, large common offset); every 16-bit store is asserted bit for bit as a function of the fp32
result.  Ops.conv3x3_block keeps every output and the workspace between guard bands and NaN-filled: each launch here also
checks that nothing outside was stored to and that every element inside was."""
import contextlib
import functools

import pytest
import torch

from _conv_block_ref import conv_sum, group_norm, planar_pack, planar_unpack
from _util import Ops

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-4               # test_conv2d_matches_torch
GN_RTOL, GN_ATOL = 1e-3, 1e-3         # test_conv_epilogue_groupnorm_statistics

# name: B, H, W, Cin, Cout, scCin -- more than one tile both ways for the 16- and 32-row tiles, ragged on both edges, batch 2
S1_CASES = {
    "c128_sc64_33x17": (2, 33, 17, 128, 128, 64),        # 128-cout tiles; shortcut narrower than the conv: two shortcut K-steps
    "c256_sc128_33x17": (2, 33, 17, 256, 256, 128),      # `big` tiles (16 x 16 px x 256 couts); two cout halves of 128
    "c512_sc256_9x13": (1, 9, 13, 512, 512, 256),        # image smaller than a tile; 16 chunks; 8 shortcut K-steps; 2-4 cout tiles
    "c128_40x50": (2, 40, 50, 128, 128, 0),              # HV_4204_4 (flag 3 = 1, no shortcut); several 32 x 16 tiles
}
# stride 2: even and odd sizes (the padding row / column is read or not), Ho = H / 2, ragged 16 x 16 output tiles, one and two cout tiles
S2_CASES = {"s2_c128_34x21": (2, 34, 21, 128, 128), "s2_c256_34x21": (2, 34, 21, 256, 256),
            "s2_c128_70x39": (1, 70, 39, 128, 128), "s2_c256_70x39": (1, 70, 39, 256, 256)}
# flag 3 = 0..4 on the halo kernel; "gemm": flag 0 = 0, the generic implicit GEMM
MODES = ["tile0", "tile1", "tile2", "tile3", "tile4", "gemm"]
HALO_MODES = MODES[:5]
DEFAULTS = {0: 1, 3: 3, 13: 1, 18: 0}


@pytest.fixture(scope="module")
def ops():
    return Ops()


@contextlib.contextmanager
def flags(ops, **kw):
    """vt_set_flag for the block, the defaults back afterwards: flags(ops, f3=1, f18=1)"""
    ids = [int(k[1:]) for k in kw]
    try:
        for i, v in zip(ids, kw.values()):
            ops.ctx.call("vt_set_flag", i, int(v))
        yield
    finally:
        for i in ids:
            ops.ctx.call("vt_set_flag", i, DEFAULTS[i])


def mode_flags(mode):
    return {"f0": 0} if mode == "gemm" else {"f0": 1, "f3": int(mode[-1])}


def f16_kernel(mode, Cout):
    """conv_f16(): the fp16-operand form exists on the default tile HV_2208_4 -- flag 3 = 3, or flag 3 = 2 on a 128-cout layer"""
    return mode == "tile3" or (mode == "tile2" and Cout % 256 != 0)


def _rand(shape, seed, scale=1.0):
    return scale * torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def bits(t):
    return t.contiguous().view(torch.int16)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def s1_data(case, f16):
    """operands pre-rounded to the operand type, residual to fp16; the fp64 references of the two forms (computed once per case and type)"""
    B, H, W, Cin, Cout, sc = S1_CASES[case]
    t16 = torch.float16 if f16 else torch.bfloat16
    seed = 1000 * sorted(S1_CASES).index(case)
    K = 9 * Cin + sc
    d = {"x": _rand((B, H, W, Cin), seed + 1).to(t16).float(), "w": _rand((Cout, Cin, 3, 3), seed + 2, K ** -0.5).to(t16).float(),
         "b": _rand((Cout,), seed + 3, 0.1), "r16": _rand((B, H, W, Cout), seed + 4).half()}
    conv = conv_sum(d["x"], d["w"], d["b"])
    d["v_res"] = conv + d["r16"].double()
    if sc:
        d["sx"], d["sw"] = _rand((B, H, W, sc), seed + 5).to(t16).float(), _rand((Cout, sc), seed + 6, K ** -0.5).to(t16).float()
        d["v_sc"] = conv + d["sx"].double() @ d["sw"].double().t()
    # the GroupNorm launches: a large common offset in the bias (mean >> std inside the groups)
    d["b_gn"] = d["b"] + 3.0
    d["gamma"], d["beta"] = 1 + 0.1 * _rand((Cout,), seed + 7), 0.1 * _rand((Cout,), seed + 8)
    return d


def forms_of(case, mode):
    """"sc": fused shortcut, no residual (what a block whose channel count changes launches); "res": residual, no shortcut"""
    return (["sc"] if S1_CASES[case][5] and mode != "gemm" else []) + ["res"]


_RESULTS = {}


def s1_results(ops, case, mode):
    """Every launch of one (case, tile mode), once: per (form, operand type) the fp32 result (launch 1: fp32 residual holding the
    fp16-representable values, fp32 output) and, per operand-copy form, the fp16 output and the copy (launch 2: the same values as an fp16
    residual).  The halo kernel writes all four copy forms; the generic GEMM only bf16 NHWC."""
    if (case, mode) in _RESULTS:
        return _RESULTS[(case, mode)]
    Cout = S1_CASES[case][4]
    copies = [("bf16", False)] + ([("f16", True), ("bf16", True), ("f16", False)] if mode != "gemm" else [])
    out = {}
    with flags(ops, **mode_flags(mode)):
        for f16 in (False, True):
            if f16 and not f16_kernel(mode, Cout):
                continue
            d = s1_data(case, f16)
            with flags(ops, f18=f16):
                for form in forms_of(case, mode):
                    kw = dict(sc_x=d["sx"], sc_w=d["sw"]) if form == "sc" else {}
                    r32, r16 = (d["r16"].float(), d["r16"]) if form == "res" else (None, None)
                    o = {"out32": ops.conv3x3_block(d["x"], d["w"], d["b"], residual=r32, out="f32", f16_operands=f16, **kw)["out"]}
                    for ctype, planar in copies:
                        z = ops.conv3x3_block(d["x"], d["w"], d["b"], residual=r16, out="f16", copy=ctype, copy_planar=planar, f16_operands=f16, **kw)
                        o[("out16", ctype, planar)], o[("copy", ctype, planar)] = z["out"], z["copy"]
                    out[(form, "f16" if f16 else "bf16")] = o
    _RESULTS[(case, mode)] = out
    return out


def check_parity(tag, got32, v):
    """rule (a): |got - ref| <= ATOL + RTOL |ref| against the fp64 reference; prints the largest error and the largest fraction of the bound used"""
    err = (got32.double() - v).abs()
    frac = (err / (ATOL + RTOL * v.abs())).max().item()
    print(f"conv_block parity {tag}: max|err| {err.max().item():.3e}, {frac:.3f} of the bound (rtol {RTOL:g}, atol {ATOL:g})")
    assert got32.shape == v.shape and frac <= 1.0, (tag, err.max().item(), frac)


def check_stores(tag, o):
    """rule (b): the fp16 output is fp16(out_f32) and the operand copy bf16(out_f32) / fp16(out_f32), bit for bit; planar == NHWC after unpacking"""
    o32 = o["out32"]
    n = 0
    for key, t in o.items():
        if key == "out32":
            continue
        kind, ctype, planar = key
        if kind == "out16":
            assert same_bits(t, o32.half()), (tag, key, "out_f16 != fp16(out_f32)")
        else:
            want = o32.half() if ctype == "f16" else o32.bfloat16()
            got = planar_unpack(t) if planar else t
            assert same_bits(got, want), (tag, key, "operand copy != 16-bit rounding of out_f32")
            if planar:
                assert same_bits(t, planar_pack(want)) and same_bits(got, o[("copy", ctype, False)]), (tag, key)
        n += 1
    print(f"conv_block stores {tag}: {n} 16-bit tensors equal the rounding of out_f32 bit for bit (bound: 0 ulp)")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(S1_CASES))
def test_block_forms_match_fp64_and_16bit_stores_are_exact(ops, case, mode):
    """(a) + (b) + (g) for every form of one case on one tile: random data against the fp64 reference under the plain conv's rule, then
    out_f16 == fp16(out_f32) and copy == bf16 / fp16(out_f32) bit for bit (launch 2 adds the exactly widened fp16 residual to the same
    accumulators in one fp32 add, on both res_f16 read paths and on the generic GEMM), the planar copy equal to the NHWC one after unpacking."""
    res = s1_results(ops, case, mode)
    assert ("res", "bf16") in res and (("sc", "bf16") in res) == (bool(S1_CASES[case][5]) and mode != "gemm")
    assert (("res", "f16") in res) == f16_kernel(mode, S1_CASES[case][4])
    for (form, optype), o in res.items():
        tag = f"{case} {mode} {form} {optype}"
        check_parity(tag, o["out32"], s1_data(case, optype == "f16")["v_" + form])
        check_stores(tag, o)
    if mode in ("tile0", "tile1", "tile2"):               # nothing promises these are the default tile's bits: reported, not asserted
        base = s1_results(ops, case, "tile3")
        eq = all(same_bits(t, base[k][kk]) for k, o in res.items() for kk, t in o.items())
        print(f"conv_block {case} {mode}: outputs {'equal' if eq else 'differ from'} the default tile's bit for bit (not asserted)")


@pytest.mark.parametrize("case", list(S1_CASES))
def test_tile_mode_4_is_bit_identical_to_the_default_tile(ops, case):
    """(f) flag 3 = 4 (one wave per SIMD, 32 x 16 px x 128 couts) is documented as the default tile's result bit for bit (header):
    every output of every form -- fused shortcut, fp16 residual, fp16 output, all four operand copies."""
    base, got = s1_results(ops, case, "tile3"), s1_results(ops, case, "tile4")
    assert set(got) == {k for k in base if k[1] == "bf16"}          # (the fp16-operand kernel exists for the default tile only)
    for k, o in got.items():
        for kk, t in o.items():
            assert same_bits(t, base[k][kk]), (case, k, kk)


def _ramp(shape):
    n = 1
    for s in shape:
        n *= s
    return (torch.arange(n, dtype=torch.float32).reshape(shape) % 251) - 125.0


@pytest.mark.parametrize("mode", HALO_MODES)
@pytest.mark.parametrize("case", [c for c, v in S1_CASES.items() if v[5]])
def test_one_hot_shortcut_and_one_hot_taps_are_exact(ops, case, mode):
    """(c) zero 3x3 weights and sc_w[co][co % scCin] = 1 on the asymmetric integer ramp: out == sc_x[..., co % scCin] + bias[co] exactly (the
    interleaved cout-row order of scW, the centre-tap address, the buffer reuse after the last chunk); then one-hot 3x3 taps, one at a time,
    with a random-integer shortcut: the exact integer sum.  Integers up to 125 are exact in bf16 and fp16, the sums stay below 2^24."""
    B, H, W, Cin, Cout, sc = S1_CASES[case]
    sx, x = _ramp((B, H, W, sc)), _ramp((B, H, W, Cin)).flip(3)
    bias = torch.randint(-9, 10, (Cout,), generator=torch.Generator().manual_seed(5)).float()
    co = torch.arange(Cout)
    sw1 = torch.zeros(Cout, sc)
    sw1[co, co % sc] = 1.0
    want1 = sx[..., co % sc] + bias
    swr = torch.randint(-3, 4, (Cout, sc), generator=torch.Generator().manual_seed(6)).float()
    sc_part = sx.double() @ swr.double().t() + bias.double()
    xp = torch.zeros(B, H + 2, W + 2, Cin)
    xp[:, 1:H + 1, 1:W + 1] = x
    with flags(ops, **mode_flags(mode)):
        for f16 in ((False, True) if f16_kernel(mode, Cout) else (False,)):
            with flags(ops, f18=f16):
                got = ops.conv3x3_block(x, torch.zeros(Cout, Cin, 3, 3), bias, sc_x=sx, sc_w=sw1, out="f32", f16_operands=f16)["out"]
                assert torch.equal(got, want1), (case, mode, f16, "one-hot shortcut")
        for tap in range(9):
            w = torch.zeros(Cout, Cin, 3, 3)
            w[co, co % Cin, tap // 3, tap % 3] = 1.0
            want = xp[:, tap // 3:tap // 3 + H, tap % 3:tap % 3 + W][..., co % Cin].double() + sc_part
            got = ops.conv3x3_block(x, w, bias, sc_x=sx, sc_w=swr, out="f32")["out"]
            assert torch.equal(got.double(), want), (case, mode, f"tap {tap}")
    print(f"conv_block one-hot {case} {mode}: shortcut and 9 taps exact (bound: 0)")


def check_gn(tag, out32, ss, v, d, groups=32):
    """rule (d): out * scale + shift against the fp64 GroupNorm of the reference sum"""
    assert torch.isfinite(ss).all(), (tag, "non-finite (scale, shift): stale partials were read")
    B, Cout = ss.shape[:2]
    got = out32.double() * ss[:, :, 0].double().view(B, 1, 1, Cout) + ss[:, :, 1].double().view(B, 1, 1, Cout)
    want = group_norm(v, groups, d["gamma"], d["beta"], 1e-6)
    err = (got - want).abs()
    frac = (err / (GN_ATOL + GN_RTOL * want.abs())).max().item()
    print(f"conv_block groupnorm {tag}: max|err| {err.max().item():.3e}, {frac:.3f} of the bound (rtol {GN_RTOL:g}, atol {GN_ATOL:g})")
    assert frac <= 1.0, (tag, err.max().item(), frac)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(S1_CASES))
def test_groupnorm_partials_with_everything_fused(ops, case, mode):
    """(d) (scale, shift) from the epilogue partials of the sum (conv + shortcut, conv + fp16 residual) on every tile, with and without the
    shortcut: vt_conv3x3_halo_tiles(..., has_sc) must agree with the launch -- the workspace is NaN before each launch, so a count that is too
    large reads NaN, one that is too small misses pixels.  The fp16-stream launch must produce the same table (same accumulators)."""
    d = s1_data(case, False)
    gn = (d["gamma"], d["beta"], 32, 1e-6)
    with flags(ops, **mode_flags(mode)):
        for form in forms_of(case, mode):
            kw = dict(sc_x=d["sx"], sc_w=d["sw"]) if form == "sc" else {}
            r32, r16 = (d["r16"].float(), d["r16"]) if form == "res" else (None, None)
            v = d["v_" + form] - d["b"].double() + d["b_gn"].double()
            a = ops.conv3x3_block(d["x"], d["w"], d["b_gn"], residual=r32, out="f32", gn=gn, **kw)
            check_parity(f"{case} {mode} {form} bf16 (+3 bias)", a["out"], v)
            check_gn(f"{case} {mode} {form}", a["out"], a["ss"], v, d)
            z = ops.conv3x3_block(d["x"], d["w"], d["b_gn"], residual=r16, out="f16", copy="bf16", copy_planar=mode != "gemm", gn=gn, **kw)
            check_gn(f"{case} {mode} {form} fp16 stream", a["out"], z["ss"], v, d)
            print(f"conv_block groupnorm {case} {mode} {form}: fp16-stream table {'equals' if torch.equal(a['ss'], z['ss']) else 'differs from'} the fp32-stream one")


@functools.lru_cache(maxsize=None)
def s2_data(case, f16):
    B, H, W, Cin, Cout = S2_CASES[case]
    t16 = torch.float16 if f16 else torch.bfloat16
    seed = 7000 + 100 * sorted(S2_CASES).index(case)
    d = {"x": _rand((B, H, W, Cin), seed + 1).to(t16).float(), "w": _rand((Cout, Cin, 3, 3), seed + 2, (9 * Cin) ** -0.5).to(t16).float(),
         "b": _rand((Cout,), seed + 3, 0.1)}
    d["v"] = conv_sum(d["x"], d["w"], d["b"], stride=2)
    d["b_gn"] = d["b"] + 3.0
    d["gamma"], d["beta"] = 1 + 0.1 * _rand((Cout,), seed + 7), 0.1 * _rand((Cout,), seed + 8)
    return d


@pytest.mark.parametrize("kernel", ["phase_plane", "gemm"])
@pytest.mark.parametrize("case", list(S2_CASES))
def test_stride2_forms(ops, case, kernel):
    """(e) Downsample2D's conv as the schedules launch it (no residual): parity on bf16 and -- phase-plane kernel -- fp16 operands, chunk-planar
    against NHWC input bit for bit, out_f16 and both operand-copy types exact functions of out_f32, GroupNorm partials."""
    B, H, W, Cin, Cout = S2_CASES[case]
    pp = kernel == "phase_plane"
    with flags(ops, f13=int(pp)):
        for f16 in ((False, True) if pp else (False,)):
            d = s2_data(case, f16)
            tag = f"{case} {kernel} {'f16' if f16 else 'bf16'}"
            with flags(ops, f18=f16):
                o = {"out32": ops.conv3x3_block(d["x"], d["w"], d["b"], stride=2, out="f32", f16_operands=f16)["out"]}
                assert o["out32"].shape == (B, H // 2, W // 2, Cout)
                check_parity(tag, o["out32"], d["v"])
                for ctype in (("bf16", "f16") if pp else ("bf16",)):
                    z = ops.conv3x3_block(d["x"], d["w"], d["b"], stride=2, out="f16", copy=ctype, f16_operands=f16)
                    o[("out16", ctype, False)], o[("copy", ctype, False)] = z["out"], z["copy"]
                check_stores(tag, o)
                if pp:
                    p = ops.conv3x3_block(d["x"], d["w"], d["b"], stride=2, out="f32", copy="bf16", x_planar=True, f16_operands=f16)
                    assert same_bits(p["out"], o["out32"]) and same_bits(p["copy"], o[("copy", "bf16", False)]), (tag, "planar input != NHWC input")
                a = ops.conv3x3_block(d["x"], d["w"], d["b_gn"], stride=2, out="f32", f16_operands=f16, gn=(d["gamma"], d["beta"], 32, 1e-6))
                check_gn(tag, a["out"], a["ss"], d["v"] - d["b"].double() + d["b_gn"].double(), d)


@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "f16"])
def test_planar_copy_feeds_the_stride2_kernel(ops, f16):
    """(e) the producer / consumer pair of a down block: the chunk-planar operand copy a stride-1 launch wrote goes straight into a stride-2
    launch as x_planar; the NHWC route (NHWC copy, NHWC input) must give the same bits.  With flag 18 the copy carries fp16 bits."""
    B, H, W, Cin, Cout = S2_CASES["s2_c128_34x21"]
    t16 = torch.float16 if f16 else torch.bfloat16
    x = _rand((B, H, W, Cin), 31).to(t16).float()
    w1, w2 = (_rand((Cout, Cin, 3, 3), s, (9 * Cin) ** -0.5).to(t16).float() for s in (32, 33))
    b1, b2, r16 = _rand((Cout,), 34, 0.1), _rand((Cout,), 35, 0.1), _rand((B, H, W, Cout), 36).half()
    ctype = "f16" if f16 else "bf16"
    with flags(ops, f18=f16):
        outs = []
        for planar in (True, False):
            a = ops.conv3x3_block(x, w1, b1, residual=r16, out="f16", copy=ctype, copy_planar=planar, f16_operands=f16)
            z = ops.conv3x3_block(a["copy_dev"], w2, b2, stride=2, out="f32", copy="bf16", x_planar=planar, f16_operands=f16, shape=(B, H, W, Cout))
            outs.append((a, z))
    (ap, zp), (an, zn) = outs
    assert same_bits(planar_unpack(ap["copy"]), an["copy"]) and same_bits(ap["out"], an["out"])
    assert same_bits(zp["out"], zn["out"]) and same_bits(zp["copy"], zn["copy"])
    v = conv_sum(an["copy"].float(), w2, b2, stride=2)              # ... and the consumer computed the conv of what the producer stored
    check_parity(f"s2_c128_34x21 planar chain {ctype}", zp["out"], v)


def test_dispatch_reaches_every_kernel_the_suite_claims(ops):
    """Which kernel took a launch, read from the library's profiler slots (vt_profile_begin / _end: 0-2 and 9 generic GEMM tiles, 3 HV_2208_4 --
    bf16 and fp16 operands --, 4 HV_4204_4, 5 HV_4208_6 and HV_2216_6, 6 HV_2408_6, 14 the stride-2 phase-plane kernel): the tile modes
    above are only worth their names if flag 3, the cout count and the shortcut select what halo_variant() says."""
    import ctypes
    n = ops.ctx.lib.vt_profile_num_configs()
    GEMM = (0, 1, 2, 9)

    def slots_of(**kw):
        C = kw.pop("C")
        sc = kw.pop("sc", False)
        x, w, b = _rand((1, 4, 6, C), 61), _rand((C, C, 3, 3), 62, 0.02), _rand((C,), 63)
        if sc:
            kw.update(sc_x=_rand((1, 4, 6, 64), 64), sc_w=_rand((C, 64), 65, 0.05))
        la, ms, fl = (ctypes.c_longlong * n)(), (ctypes.c_double * n)(), (ctypes.c_double * n)()
        ops.ctx.call("vt_profile_begin")
        try:
            ops.conv3x3_block(x, w, b, out="f32", **kw)
        finally:
            ops.ctx.call("vt_profile_end", n, la, ms, fl, None)
        return {i: la[i] for i in range(n) if la[i]}

    want = {("tile0", 128, False): 5, ("tile0", 128, True): 5, ("tile0", 256, False): 6, ("tile0", 256, True): 6,
            ("tile1", 128, False): 4, ("tile1", 128, True): 5, ("tile1", 256, False): 6, ("tile1", 256, True): 6,
            ("tile2", 128, False): 3, ("tile2", 128, True): 3, ("tile2", 256, False): 6, ("tile2", 256, True): 6,
            ("tile3", 128, False): 3, ("tile3", 128, True): 3, ("tile3", 256, False): 3, ("tile3", 256, True): 3,
            ("tile4", 128, False): 5, ("tile4", 128, True): 5, ("tile4", 256, False): 5, ("tile4", 256, True): 5}
    for (mode, C, sc), slot in want.items():
        with flags(ops, **mode_flags(mode)):
            assert slots_of(C=C, sc=sc) == {slot: 1}, (mode, C, sc)
    with flags(ops, f18=1):
        assert slots_of(C=256, sc=True, f16_operands=True) == {3: 1}
    with flags(ops, f0=0):
        got = slots_of(C=128)
        assert sum(got.values()) == 1 and set(got) <= set(GEMM), got
    assert slots_of(C=128, stride=2) == {14: 1} and slots_of(C=128, stride=2, x_planar=True) == {14: 1}
    with flags(ops, f13=0):
        got = slots_of(C=128, stride=2)
        assert sum(got.values()) == 1 and set(got) <= set(GEMM), got


def test_refused_combinations_return_an_error_and_write_nothing(ops):
    """(h) whatever run_conv or a launcher would reject is an error code with a message before anything is launched; Ops.conv3x3_block
    asserts that no byte of the (pattern-filled) outputs and workspace changed, then raises the library's message."""
    from vae_tagger_amd._lib import VTError
    B, H, W, C = 1, 4, 6, 128
    x, w, b = _rand((B, H, W, C), 41), _rand((C, C, 3, 3), 42, 0.03), _rand((C,), 43)
    sx, sw = _rand((B, H, W, 64), 44), _rand((C, 64), 45, 0.1)
    r32, r16 = _rand((B, H, W, C), 46), _rand((B, H, W, C), 46).half()
    gn = (torch.ones(C), torch.zeros(C), 32, 1e-6)

    def refused(match, *a, **kw):
        with pytest.raises(VTError, match=match):
            ops.conv3x3_block(*a, **kw)

    refused("stride-2 kernel has no fused shortcut", x, w, b, stride=2, sc_x=sx, sc_w=sw)
    refused("replaces the residual", x, w, b, sc_x=sx, sc_w=sw, residual=r32)
    refused("sc_cin", x, w, b, sc_x=_rand((B, H, W, 48), 47), sc_w=_rand((C, 48), 48))
    refused("one type", x, w, b, residual=r16, out="f32")                       # res_f16 with an fp32 output
    refused("one type", x, w, b, residual=r32, out="f16")
    refused("NHWC input only", x, w, b, x_planar=True)                          # planar input at stride 1
    refused("no chunk-planar copy", x, w, b, stride=2, out="f16", copy="bf16", copy_planar=True)
    refused("Cin % 32", _rand((B, H, W, 48), 49), _rand((C, 48, 3, 3), 50), b)   # channel counts the halo kernels refuse
    refused("Cout % 128", x, _rand((64, C, 3, 3), 51), _rand((64,), 52))
    refused("channels per group", x, w, b, gn=(torch.ones(C), torch.zeros(C), 2, 1e-6))
    with flags(ops, f0=0):                                                      # a conv the generic GEMM takes
        refused("halo kernel cannot run", x, w, b, sc_x=sx, sc_w=sw)
        refused("generic GEMM", x, w, b, out="f16", copy="bf16", copy_planar=True)
        refused("generic GEMM", x, w, b, out="f16", copy="f16")
        with flags(ops, f18=1):
            refused("no fp16-operand kernel", x, w, b, f16_operands=True)
    with flags(ops, f13=0):
        refused("generic GEMM", x, w, b, stride=2, x_planar=True)
        with flags(ops, f18=1):
            refused("no fp16-operand kernel", x, w, b, stride=2, f16_operands=True)
    with flags(ops, f3=0, f18=1):                                               # fp16 operands on a tile that has no fp16 form
        refused("no fp16-operand kernel", x, w, b, f16_operands=True)
    with flags(ops, f3=1, f18=1):
        refused("no fp16-operand kernel", x, w, b, sc_x=sx, sc_w=sw, f16_operands=True)
    # a shortcut under flag 3 = 1 on a 128-cout layer is NOT a refusal: the 128-VGPR tile has no registers for it, so halo_variant() gives
    # the launch (and vt_conv3x3_halo_tiles the partial count) the 256-VGPR 32-row tile -- and the result is right
    with flags(ops, f3=1):
        a = ops.conv3x3_block(x.bfloat16().float(), w.bfloat16().float(), b, sc_x=sx.bfloat16().float(), sc_w=sw.bfloat16().float(), out="f32", gn=gn)
        v = conv_sum(x.bfloat16().float(), w.bfloat16().float(), b, sc_x=sx.bfloat16().float(), sc_w=sw.bfloat16().float())
        check_parity("refusals: shortcut under flag 3 = 1", a["out"], v)
        assert torch.isfinite(a["ss"]).all()
    # the defaults are back: the plain call still works
    ops.conv3x3_block(x, w, b, out="f32")
