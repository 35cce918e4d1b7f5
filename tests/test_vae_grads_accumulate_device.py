"""vt_vae_grads_accumulate on the device, synthetic and bit-exact: against vt_vae_grads_export (first, scale 1), against the numpy mirror
train_vae.accumulate_rows_host (every other case) and against vt_vae_grads_merge (two micro-steps at scale 0.5).

Tensors: the sizes around a float4 and around the tile (1, 3, 4095, 4096, 4097, 8193, 5), then 130 tensors of 1 to 9 floats: 137 tensors, three
launch tables at the default chunk.  Every other gradient is held one float past a 16-B boundary (the scalar loads), four NaN floats lie
behind every gradient (a load past numel would show in the row), the row has two tiles of padding behind the layout's total, and a NaN
sentinel lies behind the row.  The values spread over 2^-20 .. 2^20 and hold -0.0, zeros and denormals."""
import ctypes
import struct

import numpy as np
import pytest
import torch

from vae_tagger_amd import _lib, train_vae

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = train_vae.TILE
NUMELS = [1, 3, 4095, 4096, 4097, 8193, 5] + [1 + (5 * i) % 9 for i in range(130)]
PAD_TILES = 2
VP = ctypes.c_void_p


def _ctx():
    from vae_tagger_amd import vae_backward
    return vae_backward.context(DEV)


def _stream():
    return VP(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _aligned(floats, fill=float("nan"), guard=TILE):
    """a 256-B aligned fp32 tensor of `floats` with `guard` floats of NaN behind it -> (tensor, guard)"""
    buf = torch.full((floats + guard + 64,), float("nan"), dtype=torch.float32, device=DEV)
    skip = (-buf.data_ptr() % 256) // 4
    row = buf[skip:skip + floats]
    row.fill_(fill)
    return row, buf[skip + floats:skip + floats + guard]


def _gradients(seed, denormals=True):
    rng = np.random.default_rng(seed)
    host = [(rng.standard_normal(n) * 2.0 ** rng.integers(-20, 21, n)).astype(np.float32) for n in NUMELS]
    host[2][::7] = 0.0
    host[2][3::11] = -0.0
    host[1][0] = -0.0
    if denormals:
        host[4][5::13] = np.float32(3e-41)
        host[6][:2] = [np.float32(1e-45), np.float32(-2e-39)]
    dev = []
    for i, h in enumerate(host):
        buf = torch.full((h.size + 12,), float("nan"), dtype=torch.float32, device=DEV)
        first = (-buf.data_ptr() % 16) // 4 + (i % 2)                          # every other gradient one float past a 16-B boundary
        t = buf[first:first + h.size]
        t.copy_(torch.from_numpy(h))
        assert t.data_ptr() % 16 == 4 * (i % 2)
        dev.append(t)
    return host, dev


@pytest.fixture(scope="module")
def case():
    offsets, total = train_vae.optim_layout(NUMELS)
    assert len(NUMELS) == 137 > 2 * _lib.VAE_OPTIM_CHUNK and set(NUMELS[7:]) == set(range(1, 10))
    sets = [_gradients(31 + k) for k in range(4)]
    return dict(offsets=offsets, total=total, row_floats=total + PAD_TILES * TILE, numel=(ctypes.c_longlong * len(NUMELS))(*NUMELS), sets=sets,
                ptrs=[(VP * len(NUMELS))(*[t.data_ptr() for t in dev]) for _, dev in sets])


def scalars_with(coef):
    """a device TrainScalars { fp64 norm^2, fp32 norm, fp32 coef } that holds `coef` at byte 12"""
    raw = np.frombuffer(struct.pack("<dff", 4.0, 2.0, coef), dtype=np.uint8).copy()
    t = torch.from_numpy(raw).to(DEV)
    assert t.data_ptr() % 16 == 0
    return t


def accumulate(case, k, row, scale, first, scalars=None, chunk=0, **kw):
    a = dict(grads=case["ptrs"][k], numel=case["numel"], n=len(NUMELS), dst=VP(row.data_ptr()), floats=row.numel(), scale=scale,
             scalars=None if scalars is None else VP(scalars.data_ptr()), first=int(first), chunk=chunk)
    a.update(kw)
    ctx = _ctx()
    return ctx.lib.vt_vae_grads_accumulate(ctx.handle, a["grads"], a["numel"], a["n"], a["dst"], a["floats"], a["scale"], a["scalars"], a["first"],
                                           a["chunk"], _stream())


def export(case, k, row):
    ctx = _ctx()
    return ctx.lib.vt_vae_grads_export(ctx.handle, case["ptrs"][k], case["numel"], len(NUMELS), VP(row.data_ptr()), row.numel(), 0, _stream())


def bits(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().tobytes()


def host_step(case, row, k, scale, coef, first):
    return train_vae.accumulate_rows_host(row, case["sets"][k][0], case["offsets"], NUMELS, scale, coef, first)


def padding_mask(case):
    mask = np.ones(case["row_floats"], dtype=bool)
    for o, n in zip(case["offsets"], NUMELS):
        mask[o:o + n] = False
    return mask


def test_first_at_scale_one_is_the_export_byte_for_byte(case):
    row, guard = _aligned(case["row_floats"])                                   # pre-filled with NaN: every float must be written
    want, _ = _aligned(case["row_floats"])
    keep = [t.clone() for t in case["sets"][0][1]]
    assert accumulate(case, 0, row, 1.0, True) == 0 and export(case, 0, want) == 0
    assert bits(row) == bits(want) == host_step(case, np.zeros(case["row_floats"], np.float32), 0, 1.0, None, True).tobytes()
    assert torch.isnan(guard).all()
    assert all(torch.equal(a, b) for a, b in zip(case["sets"][0][1], keep))     # the gradients are only read
    # a pending coefficient means nothing to a first call
    again, _ = _aligned(case["row_floats"])
    assert accumulate(case, 0, again, 1.0, True, scalars_with(0.37)) == 0
    assert bits(again) == bits(row)


@pytest.mark.parametrize("scale", [1.0 / 3.0, -0.25])
def test_a_sum_of_four_micro_steps_is_the_host_mirror_byte_for_byte(case, scale):
    """first at `scale`, then first = 0 with coef 0.37, with NULL scalars, with coef exactly 1.0 and with a NaN coef: after every call the whole
    row equals accumulate_rows_host's, so the padding stays +0.0 (under a negative scale too) and nothing behind the row is written"""
    row, guard = _aligned(case["row_floats"])
    mask = padding_mask(case)
    assert accumulate(case, 0, row, scale, True) == 0
    want = host_step(case, np.full(case["row_floats"], np.nan, np.float32), 0, scale, None, True)
    assert bits(row) == want.tobytes()
    assert not want[mask].any() and not np.signbit(want[mask]).any()
    for k, coef in ((1, 0.37), (2, None), (3, 1.0), (1, float("nan"))):
        scalars = None if coef is None else scalars_with(coef)
        assert accumulate(case, k, row, scale, False, scalars) == 0
        want = host_step(case, want, k, scale, coef, False)
        got = bits(row)
        differ = np.flatnonzero(np.frombuffer(got, np.uint32) != want.view(np.uint32))
        print(f"  scale {scale:.4f}, coef {coef}: {differ.size} of {want.size} floats differ from the host mirror")
        assert got == want.tobytes(), (k, coef)
        assert not np.frombuffer(got, np.float32)[mask].any()
    assert torch.isnan(guard).all()
    assert np.isfinite(want[~mask]).all() and np.count_nonzero(want) > 0.9 * sum(NUMELS)


def test_the_bytes_do_not_depend_on_chunk_or_on_the_run(case):
    seen = []
    for chunk in (0, 1, 7, 64, 0):
        row, guard = _aligned(case["row_floats"])
        assert accumulate(case, 0, row, 1.0 / 3.0, True, chunk=chunk) == 0
        assert accumulate(case, 1, row, 1.0 / 3.0, False, scalars_with(0.37), chunk=chunk) == 0
        seen.append(bits(row))
        assert torch.isnan(guard).all()
    assert all(s == seen[0] for s in seen)


def test_two_halves_are_the_merge_of_the_two_exported_rows(case):
    """0.5 g is exact without subnormals, and rounding the fp64 sum of two fp32 numbers to fp32 is rounding their exact sum (53 >= 2 * 24 + 2):
    first then first = 0, both at scale 0.5 with no coefficient, is vt_vae_grads_merge at weights (0.5, 0.5)"""
    sets = [_gradients(71 + k, denormals=False) for k in range(2)]
    local = dict(case, sets=sets, ptrs=[(VP * len(NUMELS))(*[t.data_ptr() for t in dev]) for _, dev in sets])
    assert all(np.all((np.abs(h) >= 1e-30) | (h == 0)) for host, _ in sets for h in host)
    F = case["row_floats"]
    rows, _ = _aligned(2 * F)
    assert export(local, 0, rows[:F]) == 0 and export(local, 1, rows[F:]) == 0
    merged, _ = _aligned(F)
    ctx = _ctx()
    w = (ctypes.c_double * 2)(0.5, 0.5)
    assert ctx.lib.vt_vae_grads_merge(ctx.handle, VP(rows.data_ptr()), F, 2, w, 0, F, VP(merged.data_ptr()), _stream()) == 0
    row, _ = _aligned(F)
    assert accumulate(local, 0, row, 0.5, True) == 0 and accumulate(local, 1, row, 0.5, False) == 0
    assert bits(row) == bits(merged)


def test_refusals_write_nothing(case):
    row, _ = _aligned(case["row_floats"])
    ctx = _ctx()
    bad_numel = (ctypes.c_longlong * len(NUMELS))(*([NUMELS[0], 0] + NUMELS[2:]))
    cases = {"n < 1": dict(n=0), "null grads": dict(grads=None), "null numel": dict(numel=None), "a null row": dict(dst=None),
             "a numel <= 0": dict(numel=bad_numel), "a misaligned row": dict(dst=VP(row.data_ptr() + 16)),
             "a short row": dict(floats=case["total"] - TILE), "a row that is no multiple of the tile": dict(floats=case["total"] + 4),
             "a NaN scale": dict(scale=float("nan")), "an infinite scale": dict(scale=float("inf")),
             "chunk too large": dict(chunk=_lib.VAE_OPTIM_CHUNK + 1), "a negative chunk": dict(chunk=-1),
             "scalars that are not 16-B aligned": dict(scalars=torch.zeros(32, dtype=torch.uint8, device=DEV)[4:20])}
    for first in (True, False):
        for what, kw in cases.items():
            kw = dict(kw)
            assert accumulate(case, 0, row, kw.pop("scale", 0.5), first, **kw) == 1, what
            assert b"vt_vae_grads_accumulate" in ctx.lib.vt_last_error(ctx.handle), what
    torch.cuda.synchronize()
    assert torch.isnan(row).all()


def test_trainer_accumulate_passes_the_scalars_exactly_when_a_clip_is_pending():
    """VAETrainer.accumulate on a prefix of a small trainer: the row is allocated on first use, `accumulated` returns views into it, and the
    coefficient of a clip() is applied by the next accumulate and by no other"""
    g = torch.Generator().manual_seed(3)
    sd = {"encoder.a": torch.randn(5, 3, generator=g), "encoder.b": torch.randn(4100, generator=g), "decoder.c": torch.randn(7, generator=g)}
    tr = train_vae.VAETrainer(sd, weights={"triplet": 1.0}, device=DEV)
    assert tr._row is None and tr.row_bytes() == 0
    grads = [{k: (torch.randn(v.shape, generator=g) * 3).to(DEV) for k, v in list(sd.items())[:2]} for _ in range(3)]
    host = [[x.cpu().numpy().reshape(-1) for x in gs.values()] for gs in grads]
    offs, nums = tr.offsets[:2], tr.numels[:2]
    tr.accumulate(grads[0], scale=0.5, first=True, n=2)
    assert tr.row_bytes() == 4 * tr.total and tr._row.data_ptr() % 256 == 0
    views = tr.accumulated(2)
    assert list(views) == list(sd)[:2] and all(v.data_ptr() == tr._row.data_ptr() + 4 * o for v, o in zip(views.values(), offs))
    want = train_vae.accumulate_rows_host(np.zeros(tr.total, np.float32), host[0], offs, nums, 0.5, None, True)
    assert bits(tr._row) == want.tobytes()
    tr.clip({**views, "decoder.c": tr.accumulated()["decoder.c"]}, 0.25)        # the existing norm on views into the row
    norm, coef = tr.grad_norm()
    assert coef < 1.0 and tr._clipped
    tr.accumulate(grads[1], scale=0.5, first=False, n=2)
    want = train_vae.accumulate_rows_host(want, host[1], offs, nums, 0.5, coef, False)
    assert bits(tr._row) == want.tobytes() and not tr._clipped
    tr.accumulate(grads[2], scale=0.5, first=False, n=2)                        # no clip since: the stale coefficient is not applied again
    want = train_vae.accumulate_rows_host(want, host[2], offs, nums, 0.5, None, False)
    assert bits(tr._row) == want.tobytes()
    with pytest.raises(ValueError):
        tr.accumulate(grads[0], scale=0.5, first=True, n=3)
