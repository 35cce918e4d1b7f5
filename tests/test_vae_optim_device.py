"""vt_vae_optim_norm and vt_vae_optim_step on the device, driven through the C ABI: the norm and the clip coefficient against fp64, run-to-run and
chunking-independent bits, AdamW against torch.optim.AdamW in fp64 and fp32 (the rule and the constants of tests/test_train_device.py), the folded
scale against a separate fp32 multiply, the exact cases (gradients never written, zero padding, a zero gradient, the float4 path against the scalar
one) and every refusal against guard copies.

Tensors: the sizes around the tile (4095, 4096, 4097, 8191, 3 * 4096), below a float4 (1, 3), not a multiple of 4 (5, 70 000 is; 4097 is not), a
larger one (70 000: 18 tiles), and 120 tensors of 7 floats so that the list (132 tensors) crosses two boundaries of the 64-tensor launch table."""
import ctypes
import math

import pytest
import torch

from vae_tagger_amd import _lib, train_vae

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR, FACTOR = 1e-7, 4.0                       # tests/test_train_device.py's
NUMELS = [3, 1, 5, 4, 32, 128, 4095, 4096, 4097, 8191, 3 * 4096, 70000] + [7] * 120
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8
VP = ctypes.c_void_p


def rel(a, ref):
    ref = ref.double()
    return ((a.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def check(name, dev, r64, r32):
    e32 = max(rel(r32, r64), FLOOR)
    ratio = rel(dev, r64) / e32
    assert ratio <= FACTOR, f"{name}: device error is {ratio:.2f} x the fp32 yardstick {e32:.2e}"
    return ratio


def make_grads(seed, scale=1.0, offset_floats=0):
    """randn gradients scaled differently per tensor (CPU master copies and device tensors; offset_floats = 1 holds every tensor 4 B past a
    16-B boundary: the same data on the scalar path)"""
    g = torch.Generator().manual_seed(seed)
    host = [torch.randn(n, generator=g) * (scale * (0.05 + 0.37 * (i % 11))) for i, n in enumerate(NUMELS)]
    dev = []
    for h in host:
        buf = torch.empty(h.numel() + 4, dtype=torch.float32, device=DEV)
        t = buf[offset_floats:offset_floats + h.numel()]
        t.copy_(h)
        assert t.data_ptr() % 16 == 4 * offset_floats
        dev.append(t)
    return host, dev


class Optim:
    """three arenas, the scalars and the workspace, and the two entry points with every argument replaceable"""

    def __init__(self, seed=0):
        from vae_tagger_amd import vae_backward
        self.ctx = vae_backward.context(DEV)
        self.offsets, self.total = train_vae.optim_layout(NUMELS)
        g = torch.Generator().manual_seed(seed)
        self.p0 = [torch.randn(n, generator=g) for n in NUMELS]
        self.arenas = [torch.zeros(self.total, dtype=torch.float32, device=DEV) for _ in range(3)]
        assert all(a.data_ptr() % 256 == 0 for a in self.arenas)
        for p, o in zip(self.p0, self.offsets):
            self.arenas[0][o:o + p.numel()].copy_(p)
        self.scalars = torch.zeros(2, dtype=torch.float64, device=DEV)
        self.numel = (ctypes.c_longlong * len(NUMELS))(*NUMELS)
        self.ws_bytes = self.ctx.lib.vt_vae_optim_workspace_bytes(self.numel, len(NUMELS))
        assert self.ws_bytes == (8 * (self.total // 4096) + 255) // 256 * 256
        self.ws = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=DEV)

    def stream(self):
        return VP(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)

    def ptrs(self, grads):
        return (VP * len(grads))(*[g.data_ptr() if g is not None else 0 for g in grads])

    def norm(self, dev, bound, **kw):
        a = dict(grads=self.ptrs(dev), numel=self.numel, n=len(NUMELS), max_norm=float(bound), scalars=VP(self.scalars.data_ptr()),
                 ws=VP(self.ws.data_ptr()), ws_bytes=self.ws_bytes, chunk=0)
        a.update(kw)
        return self.ctx.lib.vt_vae_optim_norm(self.ctx.handle, a["grads"], a["numel"], a["n"], a["max_norm"], a["scalars"], a["ws"], a["ws_bytes"],
                                              a["chunk"], self.stream())

    def step(self, dev, use_scalars=False, **kw):
        a = dict(p=VP(self.arenas[0].data_ptr()), m=VP(self.arenas[1].data_ptr()), v=VP(self.arenas[2].data_ptr()), floats=self.total,
                 grads=self.ptrs(dev), numel=self.numel, n=len(NUMELS), scalars=VP(self.scalars.data_ptr()) if use_scalars else None, lr=LR,
                 beta1=BETAS[0], beta2=BETAS[1], eps=EPS, wd=0.0, t=None, chunk=0)
        a.update(kw)
        return self.ctx.lib.vt_vae_optim_step(self.ctx.handle, a["p"], a["m"], a["v"], a["floats"], a["grads"], a["numel"], a["n"], a["scalars"],
                                              a["lr"], a["beta1"], a["beta2"], a["eps"], float(a["wd"]), a["t"], a["chunk"], self.stream())

    def tensor(self, which, i):
        return self.arenas[which][self.offsets[i]:self.offsets[i] + NUMELS[i]]

    def read_scalars(self):
        raw = self.scalars.cpu()
        f = raw.view(torch.float32)
        return raw[0].item(), f[2].item(), f[3].item(), raw.view(torch.uint8).clone()

    def guard(self):
        torch.cuda.synchronize()
        return [a.clone() for a in self.arenas] + [self.scalars.clone(), self.ws.clone()]

    def unchanged(self, guard):
        torch.cuda.synchronize()
        return all(torch.equal(a, b) for a, b in zip(self.arenas + [self.scalars, self.ws], guard))


def test_norm_and_clip_coefficient():
    o = Optim()
    host, dev = make_grads(1)
    keep = [g.clone() for g in dev]
    norm64 = math.sqrt(sum((h.double() ** 2).sum().item() for h in host))
    assert o.norm(dev, 10.0 * norm64) == 0
    sq, norm, coef, bits = o.read_scalars()
    print(f"  norm {norm:.9g} vs fp64 {norm64:.9g}, coef {coef}")
    assert abs(norm - norm64) <= 1e-6 * norm64 and coef == 1.0 and abs(math.sqrt(sq) - norm64) <= 1e-12 * norm64
    max_norm = 0.25 * norm64
    assert o.norm(dev, max_norm) == 0
    _, norm, coef, bits = o.read_scalars()
    assert abs(norm - norm64) <= 1e-6 * norm64 and coef < 1.0
    f32 = torch.tensor
    want = (f32(max_norm, dtype=torch.float32) / (f32(norm, dtype=torch.float32) + f32(1e-6, dtype=torch.float32))).item()
    assert coef == want                                        # train_clip_kernel's formula, in fp32
    assert o.norm(dev, max_norm) == 0                          # a second call: the same bits
    assert torch.equal(o.read_scalars()[3], bits)
    for chunk in (1, 5, 63, 64):                               # the same tensors in other launch tables: the same bits
        o.scalars.zero_()
        o.ws.zero_()
        assert o.norm(dev, max_norm, chunk=chunk) == 0
        assert torch.equal(o.read_scalars()[3], bits), chunk
    _, dev1 = make_grads(1, offset_floats=1)                   # the scalar path loads the same elements into the same places
    assert o.norm(dev1, max_norm) == 0
    assert torch.equal(o.read_scalars()[3], bits)
    assert all(torch.equal(a, b) for a, b in zip(dev, keep))   # the gradients are not written


@pytest.mark.parametrize("wd", [0.0, 1e-6, 1e-2])
def test_adamw_matches_torch(wd):
    o = Optim(seed=3)
    refs = {}
    for dtype in (torch.float64, torch.float32):
        ps = [p.to(dtype).clone().requires_grad_(True) for p in o.p0]
        refs[dtype] = (ps, torch.optim.AdamW(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd))
    for t in range(1, 6):
        host, dev = make_grads(100 + t, scale=0.1 + t)
        keep = [g.clone() for g in dev]
        assert o.step(dev, t=t, wd=wd) == 0
        for dtype, (ps, opt) in refs.items():
            for p, h in zip(ps, host):
                p.grad = h.to(dtype)
            opt.step()
        assert all(torch.equal(a, b) for a, b in zip(dev, keep))                   # never written, never zeroed
    worst = 0.0
    for i in range(len(NUMELS)):
        worst = max(worst, check(f"tensor {i} ({NUMELS[i]})", o.tensor(0, i).cpu(), refs[torch.float64][0][i].detach(), refs[torch.float32][0][i].detach()))
    print(f"adamw wd={wd}: worst device/e32 = {worst:.3f}")
    real = torch.zeros(o.total, dtype=torch.bool, device=DEV)
    for off, n in zip(o.offsets, NUMELS):
        real[off:off + n] = True
    for a in o.arenas:                                                              # the padding of all three arenas is still zero
        assert not a[~real].any()
    assert all(o.tensor(w, i).abs().sum() > 0 for w in (1, 2) for i in range(len(NUMELS)))


def test_folded_scale_is_one_fp32_multiply():
    host, dev = make_grads(7)
    norm64 = math.sqrt(sum((h.double() ** 2).sum().item() for h in host))
    a, b = Optim(seed=5), Optim(seed=5)
    for t in (1, 2):
        assert a.norm(dev, 0.25 * norm64) == 0
        assert a.step(dev, True, t=t, wd=1e-2) == 0
        coef = a.scalars.view(torch.float32)[3]                                     # stays on the device
        scaled = [g * coef for g in dev]                                            # one fp32 multiply, one rounding
        assert b.step(scaled, t=t, wd=1e-2) == 0
    assert a.read_scalars()[2] < 1.0
    for x, y in zip(a.arenas, b.arenas):
        assert torch.equal(x, y)
    # inside the bound the coefficient is 1 and the scalars change nothing
    c, d = Optim(seed=5), Optim(seed=5)
    assert c.norm(dev, 10.0 * norm64) == 0 and c.step(dev, True, t=1, wd=1e-2) == 0 and d.step(dev, t=1, wd=1e-2) == 0
    assert all(torch.equal(x, y) for x, y in zip(c.arenas, d.arenas))


def test_exact_cases():
    # a zero gradient with wd = 0 at t = 1 leaves p's bits (and the moments zero)
    o = Optim(seed=9)
    before = o.arenas[0].clone()
    zeros = [torch.zeros(n, device=DEV) for n in NUMELS]
    assert o.step(zeros, t=1, wd=0.0) == 0
    assert torch.equal(o.arenas[0].view(torch.int32), before.view(torch.int32)) and not o.arenas[1].any() and not o.arenas[2].any()
    # float4 path against scalar path: the same data held 4 bytes past a 16-B boundary, and another chunking, give the same bits
    a, b, c = Optim(seed=11), Optim(seed=11), Optim(seed=11)
    for t in (1, 2, 3):
        _, g0 = make_grads(40 + t)
        _, g1 = make_grads(40 + t, offset_floats=1)
        assert a.step(g0, t=t, wd=1e-2) == 0 and b.step(g1, t=t, wd=1e-2) == 0 and c.step(g0, t=t, wd=1e-2, chunk=3) == 0
    for x, y, z in zip(a.arenas, b.arenas, c.arenas):
        assert torch.equal(x, y) and torch.equal(x, z)


def test_refusals_leave_everything_untouched():
    o = Optim(seed=13)
    _, dev = make_grads(21)
    assert o.norm(dev, 1.0) == 0 and o.step(dev, t=1) == 0                             # a state worth guarding
    guard = o.guard()
    numel0 = (ctypes.c_longlong * len(NUMELS))(*([3, 0] + NUMELS[2:]))
    null_grad = list(dev)
    null_grad[77] = None
    odd = (VP * len(dev))(*[g.data_ptr() + (2 if i == 5 else 0) for i, g in enumerate(dev)])
    INVALID, WORKSPACE = 1, 5
    norm_cases = {"n < 1": dict(n=0), "a numel <= 0": dict(numel=numel0), "a null gradient": dict(grads=o.ptrs(null_grad)), "a misaligned gradient": dict(grads=odd),
                  "max_norm = 0": dict(max_norm=0.0), "max_norm < 0": dict(max_norm=-1.0), "max_norm nan": dict(max_norm=float("nan")),
                  "null scalars": dict(scalars=None), "misaligned scalars": dict(scalars=VP(o.scalars.data_ptr() + 8)), "null workspace": dict(ws=None),
                  "misaligned workspace": dict(ws=VP(o.ws.data_ptr() + 16)), "chunk too large": dict(chunk=_lib.VAE_OPTIM_CHUNK + 1),
                  "negative chunk": dict(chunk=-1), "null numel": dict(numel=None), "null grads": dict(grads=None)}
    for what, kw in norm_cases.items():
        assert o.norm(dev, 1.0, **kw) == INVALID, what
        assert o.unchanged(guard), what
    assert o.norm(dev, 1.0, ws_bytes=o.ws_bytes - 1) == WORKSPACE and o.unchanged(guard)
    assert b"vt_vae_optim_norm" in o.ctx.lib.vt_last_error(o.ctx.handle)
    step_cases = {"null params": dict(p=None), "null m": dict(m=None), "null v": dict(v=None), "misaligned params": dict(p=VP(o.arenas[0].data_ptr() + 16)),
                  "misaligned v": dict(v=VP(o.arenas[2].data_ptr() + 128)), "small arenas": dict(floats=o.total - 1), "n < 1": dict(n=0),
                  "a numel <= 0": dict(numel=numel0), "a null gradient": dict(grads=o.ptrs(null_grad)), "a misaligned gradient": dict(grads=odd),
                  "misaligned scalars": dict(scalars=VP(o.scalars.data_ptr() + 8)), "t = 0": dict(t=0), "beta1 = 1": dict(beta1=1.0),
                  "beta2 < 0": dict(beta2=-0.1), "eps < 0": dict(eps=-1e-8), "lr inf": dict(lr=float("inf")), "wd nan": dict(wd=float("nan")),
                  "chunk too large": dict(chunk=_lib.VAE_OPTIM_CHUNK + 1)}
    for what, kw in step_cases.items():
        assert o.step(dev, **{"t": 2, **kw}) == INVALID, what
        assert o.unchanged(guard), what
    assert b"vt_vae_optim_step" in o.ctx.lib.vt_last_error(o.ctx.handle)
    assert o.step(dev, t=2) == 0 and not o.unchanged(guard)                            # and the call they guarded still works
