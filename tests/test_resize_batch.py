"""vt_resize_normalize_batch: the batched, fused resize + normalise of the C ABI (csrc/resize_batch.hip) against Pillow itself,
its argument checks, and the surface around it (header, exported symbols, ctypes binding)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from vae_tagger_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BILINEAR, LANCZOS = 0, 1
BUCKETS = [(512, 512), (1024, 512), (576, 768), (960, 1024)]          # (width, height)


def _items(entries):
    arr = (_lib.ResizeItem * len(entries))()
    for k, e in enumerate(entries):
        arr[k] = _lib.ResizeItem(*e)
    return arr


# ---- CPU: ABI surface ----------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_declared_and_bound():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "vae_tagger_hip.h")).read()
    for name in ("vt_resize_batch_workspace_bytes", "vt_resize_normalize_batch"):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert "vt_resize_item" in header
    assert ctypes.sizeof(_lib.ResizeItem) == 32                     # pointer + six ints, as the header's struct


def test_workspace_bytes_is_zero_for_invalid_arguments():
    lib = _lib.load()
    ok = [(0, 100, 200, 10, 5, 150, 90), (0, 64, 64, 0, 0, 64, 64)]
    assert lib.vt_resize_batch_workspace_bytes(_items(ok), 2, 64, 64, LANCZOS) > 0
    assert lib.vt_resize_batch_workspace_bytes(_items(ok), 2, 64, 64, BILINEAR) > 0
    for bad in ((0, 100, 200, 60, 0, 150, 90),        # crop box leaves the source on the right
                (0, 100, 200, 0, 20, 150, 90),        # ... at the bottom
                (0, 100, 200, -1, 0, 150, 90), (0, 100, 200, 0, 0, 0, 90), (0, 0, 200, 0, 0, 1, 1)):
        assert lib.vt_resize_batch_workspace_bytes(_items([ok[0], bad]), 2, 64, 64, LANCZOS) == 0, bad
    assert lib.vt_resize_batch_workspace_bytes(None, 2, 64, 64, LANCZOS) == 0
    assert lib.vt_resize_batch_workspace_bytes(_items(ok), 0, 64, 64, LANCZOS) == 0
    assert lib.vt_resize_batch_workspace_bytes(_items(ok), 2, 0, 64, LANCZOS) == 0
    assert lib.vt_resize_batch_workspace_bytes(_items(ok), 2, 64, 64, 2) == 0
    # images of one size share their tables: the block does not grow with them
    one = lib.vt_resize_batch_workspace_bytes(_items([ok[0]]), 1, 64, 64, LANCZOS)
    two = lib.vt_resize_batch_workspace_bytes(_items([ok[0], ok[0]]), 2, 64, 64, LANCZOS)
    assert two - one == (90 * 64 * 3 + 255) // 256 * 256


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    return _lib.Context(0)


def _rand_image(rng, h, w):
    # smooth ramps + noise: resampling a pure-noise picture exercises the clipping less than edges do
    a = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    a[: h // 3, : w // 2] = 255
    a[h // 2:, w // 3: w // 3 + 7] = 0
    return a


def _run(ctx, arrays, boxes, tw, th, filt, want_u8=True, want_f32=True):
    """One vt_resize_normalize_batch call -> (fp32 [B,3,th,tw] or None, uint8 [B,th,tw,3] or None) on the device."""
    dev = torch.device("cuda:0")
    srcs = [torch.from_numpy(a).to(dev) for a in arrays]
    items = _items([(s.data_ptr(), a.shape[0], a.shape[1]) + tuple(b) for s, a, b in zip(srcs, arrays, boxes)])
    B = len(arrays)
    need = ctx.lib.vt_resize_batch_workspace_bytes(items, B, th, tw, filt)
    assert need > 0
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    f32 = torch.full((B, 3, th, tw), float("nan"), dtype=torch.float32, device=dev) if want_f32 else None
    u8 = torch.zeros(B, th, tw, 3, dtype=torch.uint8, device=dev) if want_u8 else None
    vp = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
    ctx.call("vt_resize_normalize_batch", items, B, th, tw, filt, vp(f32), f32.numel() * 4 if want_f32 else 0, vp(u8),
             u8.numel() if want_u8 else 0, ctypes.c_void_p((ws.data_ptr() + 255) // 256 * 256), need, None)
    torch.cuda.synchronize()
    return f32, u8


def _pil_resize(a, box, tw, th, filt):
    """SmartResize's order: crop, then resize the cropped image (Image.resize(box=...) would let the filter read past the box)."""
    from PIL import Image
    left, top, cw, ch = box
    img = Image.fromarray(a)
    if (left, top, cw, ch) != (0, 0) + img.size:
        img = img.crop((left, top, left + cw, top + ch))
    return np.asarray(img.resize((tw, th), Image.LANCZOS if filt == LANCZOS else Image.BILINEAR))


def _geometry_cases(tw, th):
    """(name, source (h, w), crop box (left, top, w, h)) -- mixed source sizes in one batch."""
    return [
        ("both axes shrink", (th * 3 // 2 + 11, tw * 3 // 2 + 5), (0, 0, tw * 3 // 2 + 5, th * 3 // 2 + 11)),
        ("both axes grow", (th * 5 // 8, tw * 3 // 5), (0, 0, tw * 3 // 5, th * 5 // 8)),
        ("horizontal only", (th, tw * 2 + 3), (0, 0, tw * 2 + 3, th)),
        ("horizontal only, growing", (th + 9, tw // 2 + 40), (20, 9, tw // 2, th)),
        ("vertical only", (th * 2 - 7, tw), (0, 0, tw, th * 2 - 7)),
        ("vertical only, growing, inside a wider source", (th // 2 + 3, tw + 33), (33, 2, tw, th // 2)),
        ("identity", (th, tw), (0, 0, tw, th)),
        ("identity crop copy out of a larger source", (th + 40, tw + 25), (13, 31, tw, th)),
        ("off-centre crop box", (th + 300, tw + 411), (5, 170, tw + 300, th + 101)),
        ("crop box ending at the source's last pixel", (th + 77, tw + 90), (1, 3, tw + 89, th + 74)),
        (">4x LANCZOS downscale", (th * 9 // 2 + 3, tw * 17 // 4 + 1), (0, 0, tw * 17 // 4 + 1, th * 9 // 2 + 3)),
        ("shrink one axis, grow the other", (th // 2 + 1, tw * 2 + 1), (0, 0, tw * 2 + 1, th // 2 + 1)),
        ("odd widths (unaligned rows)", (th + 1, tw + 1), (0, 0, tw + 1, th + 1)),
        ("single column crop", (th + 5, 37), (18, 0, 1, th + 5)),
        ("tiny source", (3, 5), (0, 0, 5, 3)),
        ("both axes shrink, off-centre", (th * 2, tw * 3), (tw // 2 + 1, 7, tw * 2 + 3, th * 2 - 9)),
    ]


@pytest.mark.gpu
@pytest.mark.parametrize("filt", [LANCZOS, BILINEAR])
@pytest.mark.parametrize("bucket", BUCKETS)
def test_batch_matches_pillow_byte_for_byte(ctx, bucket, filt):
    """One batch of 16 per (bucket, filter): every geometry case against Pillow's crop + Image.resize, and the fp32 output against
    vt_preprocess_u8 of the uint8 output, bit for bit; then the first image alone (B = 1) and fp32-only / uint8-only calls."""
    from vae_tagger_amd._runtime import vp
    tw, th = bucket
    rng = np.random.default_rng(tw * 7 + th + filt)
    cases = _geometry_cases(tw, th)
    assert len(cases) == 16
    arrays = [_rand_image(rng, h, w) for _, (h, w), _ in cases]
    boxes = [b for _, _, b in cases]
    f32, u8 = _run(ctx, arrays, boxes, tw, th, filt)
    ref32 = torch.empty_like(f32)
    ctx.call("vt_preprocess_u8", vp(u8), len(cases), th, tw, vp(ref32), None)
    torch.cuda.synchronize()
    got = u8.cpu().numpy()
    for k, (name, _, box) in enumerate(cases):
        want = _pil_resize(arrays[k], box, tw, th, filt)
        diff = int((got[k].astype(np.int16) - want.astype(np.int16)).__abs__().max())
        print(f"{tw}x{th} filter {filt} {name}: max |d| = {diff}")
        assert np.array_equal(got[k], want), (bucket, filt, name, diff)
    assert torch.equal(f32, ref32)
    f1, u1 = _run(ctx, arrays[:1], boxes[:1], tw, th, filt)
    assert torch.equal(u1[0], u8[0]) and torch.equal(f1[0], f32[0])
    f_only, none = _run(ctx, arrays[8:11], boxes[8:11], tw, th, filt, want_u8=False)
    assert none is None and torch.equal(f_only, f32[8:11])
    none, u_only = _run(ctx, arrays[8:11], boxes[8:11], tw, th, filt, want_f32=False)
    assert none is None and torch.equal(u_only, u8[8:11])


@pytest.fixture(scope="module")
def pipe():
    from vae_tagger_amd import synth
    from vae_tagger_amd.diffusers_vae_loader import DiffusersVAEWrapper, get_diffusers_vae_config, load_diffusers_vae_from_config
    from vae_tagger_amd.modules import create_attention_decoder
    from vae_tagger_amd.pipeline import EncodeTagPipeline
    vae = DiffusersVAEWrapper(load_diffusers_vae_from_config(get_diffusers_vae_config())).to("cuda:0").eval()
    dec = create_attention_decoder(16, 16, 16, 11, {"use_spatial_attention": True, "use_self_attention": True}).to("cuda:0").eval()
    return EncodeTagPipeline(vae, dec)


@pytest.mark.gpu
@pytest.mark.parametrize("bucket", BUCKETS)
def test_load_batch_equals_smart_resize_and_load_image(pipe, bucket):
    """pipe.load_batch(bucket=...) == SmartResize(bucket)(img) byte for byte (uint8) and == get_image_transform(.., True, bucket)(img) /
    pipe.load_image(img, bucket=...) bit for bit (fp32), for a batch of 16 sources of assorted aspect ratios."""
    from PIL import Image
    from vae_tagger_amd.modules import SmartResize, get_image_transform
    tw, th = bucket
    rng = np.random.default_rng(tw + th)
    sizes = [(tw, th), (tw * 2, th * 2), (tw + 130, th), (tw, th + 97), (tw // 2, th // 2), (tw * 3 + 1, th + 3), (tw // 3, th * 2),
             (1200, 800), (800, 1200), (333, 517), (2048, 1024), (640, 640), (tw * 5, th * 5 - 20), (97, 89), (tw - 1, th + 1), (1500, 1499)]
    arrays = [_rand_image(rng, h, w) for (w, h) in sizes]
    raws = [torch.from_numpy(a).cuda() for a in arrays]
    x, u8 = pipe.load_batch(raws, bucket=bucket, return_u8=True)
    torch.cuda.synchronize()
    tf = get_image_transform(1024, True, bucket)
    for k, a in enumerate(arrays):
        img = Image.fromarray(a)
        assert np.array_equal(u8[k].cpu().numpy(), np.asarray(SmartResize(tw, th)(img))), (bucket, sizes[k])
        assert torch.equal(x[k].cpu(), tf(img)), (bucket, sizes[k])
    for k in (1, 5, 9):
        assert torch.equal(pipe.load_image(Image.fromarray(arrays[k]), bucket=bucket), x[k])
    assert torch.equal(pipe.load_batch(raws[3:4], bucket=bucket), x[3:4])


@pytest.mark.gpu
@pytest.mark.parametrize("res", [512, 1024, 128])
def test_load_batch_square_route_equals_bilinear_resize(pipe, res):
    from PIL import Image
    from vae_tagger_amd.modules import get_image_transform
    rng = np.random.default_rng(res)
    sizes = [(res, res), (res * 2, res // 2), (res // 2 + 1, res * 3), (777, 333), (res, res + 1), (res - 1, res), (3000, 2000), (40, 30)]
    arrays = [_rand_image(rng, h, w) for (w, h) in sizes]
    x, u8 = pipe.load_batch([torch.from_numpy(a).cuda() for a in arrays], resolution=res, return_u8=True)
    torch.cuda.synchronize()
    tf = get_image_transform(res)
    for k, a in enumerate(arrays):
        img = Image.fromarray(a)
        assert np.array_equal(u8[k].cpu().numpy(), np.asarray(img.resize((res, res), Image.BILINEAR))), (res, sizes[k])
        assert torch.equal(x[k].cpu(), tf(img)), (res, sizes[k])


@pytest.mark.gpu
def test_bad_arguments_are_rejected_before_anything_is_written(ctx):
    """Undersized outputs / workspace -> VT_ERR_WORKSPACE; a crop box outside its source, NULL items, a NULL source, no output ->
    VT_ERR_INVALID; in every case the outputs, the workspace and 1 MB guard bands around them keep their byte pattern.  Then a valid
    call into the same exactly-sized buffers leaves the guard bands intact."""
    dev = torch.device("cuda:0")
    GUARD, PAT = 1 << 20, 0xA5
    tw, th, B = 192, 128, 3
    rng = np.random.default_rng(3)
    arrays = [_rand_image(rng, h, w) for (h, w) in ((200, 300), (128, 192), (90, 500))]
    srcs = [torch.from_numpy(a).to(dev) for a in arrays]
    good = [(s.data_ptr(), a.shape[0], a.shape[1], 0, 0, a.shape[1], a.shape[0]) for s, a in zip(srcs, arrays)]
    L = ctx.lib
    need = L.vt_resize_batch_workspace_bytes(_items(good), B, th, tw, LANCZOS)
    n32, n8 = B * 3 * th * tw * 4, B * th * tw * 3

    def guarded(nbytes):
        t = torch.full((GUARD + nbytes + 256 + GUARD,), PAT, dtype=torch.uint8, device=dev)
        p = (t.data_ptr() + GUARD + 255) // 256 * 256
        return t, p

    bufs = {"f32": guarded(n32), "u8": guarded(n8), "ws": guarded(need)}

    def call(items, b=B, f32_bytes=n32, u8_bytes=n8, ws_bytes=need, f32=True, u8=True, ws=True):
        return L.vt_resize_normalize_batch(ctx.handle, items, b, th, tw, LANCZOS, ctypes.c_void_p(bufs["f32"][1] if f32 else 0), f32_bytes,
                                           ctypes.c_void_p(bufs["u8"][1] if u8 else 0), u8_bytes, ctypes.c_void_p(bufs["ws"][1] if ws else 0),
                                           ws_bytes, None)

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == PAT).all()) for t, _ in bufs.values())

    INVALID, WORKSPACE = 1, 5
    outside = list(good)
    outside[1] = good[1][:3] + (1, 0, 192, 128)                      # one column past the right edge
    null_src = list(good)
    null_src[2] = (0,) + good[2][1:]
    for what, rc, want in (("undersized fp32 output", call(_items(good), f32_bytes=n32 - 1), WORKSPACE),
                           ("undersized uint8 output", call(_items(good), u8_bytes=n8 - 1), WORKSPACE),
                           ("undersized workspace", call(_items(good), ws_bytes=need - 257), WORKSPACE),
                           ("crop outside the source", call(_items(outside)), INVALID),
                           ("NULL items", call(None), INVALID),
                           ("NULL source", call(_items(null_src)), INVALID),
                           ("no output", call(_items(good), f32=False, u8=False), INVALID),
                           ("NULL workspace", call(_items(good), ws=False), INVALID),
                           ("B = 0", call(_items(good), b=0), INVALID)):
        assert rc == want, (what, rc, L.vt_last_error(ctx.handle))
        assert untouched(), what
    assert call(_items(good)) == 0, L.vt_last_error(ctx.handle)
    torch.cuda.synchronize()
    for name, nbytes in (("f32", n32), ("u8", n8), ("ws", need)):
        t, p = bufs[name]
        off = p - t.data_ptr()
        assert bool((t[:off] == PAT).all()), (name, "bytes in front of the buffer")
        assert bool((t[off + nbytes:] == PAT).all()), (name, "bytes behind the buffer")
    t, p = bufs["u8"]
    got = t[p - t.data_ptr(): p - t.data_ptr() + n8].view(B, th, tw, 3).cpu().numpy()
    for k in range(B):
        assert np.array_equal(got[k], _pil_resize(arrays[k], good[k][3:], tw, th, LANCZOS))
