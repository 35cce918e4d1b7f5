"""vt_vae_grads_export and vt_vae_grads_merge on the device, and VAEGradientExchange over K ranks emulated in one process.  Every kernel case is
bit-exact: the exported row against the host packing, the merge against train_vae.merge_rows_host.

Tensors: the sizes around a float4 and around the tile (1, 3, 4, 5, 4095, 4096, 4097, 8192, 8195), one of 64 tiles less 3 floats that straddles
the owners' boundary at K = 2 (tile 74 of 147) and at K = 3 (tile 49), and 70 tensors of 7 floats, so that the list (80 tensors) needs two
launch tables; gradient 6 is held one float past a 16-B boundary (the scalar loads).  Behind every gradient lie four NaN floats: a load past
numel would show in the row.  At K = 8 the row has 5 tiles of padding behind the layout's total."""
import ctypes

import numpy as np
import pytest
import torch

from vae_tagger_amd import _lib, train_vae

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = train_vae.TILE
BIG = 64 * TILE - 3
NUMELS = [1, 3, 4, 5, 4095, 4096, 4097, 8192, 8195, BIG] + [7] * 70
UNALIGNED = 6
VP = ctypes.c_void_p
COUNTS = {1: [[1]], 2: [[1, 2], [2, 0]], 3: [[1, 2, 3], [2, 1, 0]], 8: [[1, 2, 3, 0, 1, 2, 3, 1]]}      # images per rank: w = n_r / sum n


def _ctx():
    from vae_tagger_amd import vae_backward
    return vae_backward.context(DEV)


def _stream():
    return VP(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _aligned(floats, fill=float("nan"), guard=TILE):
    """a 256-B aligned fp32 tensor of `floats` with `guard` floats of NaN behind it -> (tensor, guard)"""
    buf = torch.full((floats + guard + 64,), fill, dtype=torch.float32, device=DEV)
    skip = (-buf.data_ptr() % 256) // 4
    return buf[skip:skip + floats], buf[skip + floats:skip + floats + guard]


@pytest.fixture(scope="module")
def layout():
    offsets, total = train_vae.optim_layout(NUMELS)
    tiles = total // TILE
    assert len(NUMELS) > _lib.VAE_OPTIM_CHUNK and tiles == 147
    lo, hi = offsets[9] // TILE, (offsets[9] + BIG - 1) // TILE                # the big tensor's first and last tile
    for K in (2, 3):
        S, _ = train_vae.owner_split(total, K)
        assert lo < S <= hi, K                                                 # a boundary between two owners lies inside it
    g = torch.Generator().manual_seed(4)
    host = [torch.randn(n, generator=g) * (0.05 + 0.37 * (i % 11)) for i, n in enumerate(NUMELS)]
    host[3][:3] = torch.tensor([-0.0, 1e-45, -3e-39])                          # -0.0 and denormals travel as they are
    dev = []
    for i, h in enumerate(host):
        buf = torch.full((h.numel() + 8,), float("nan"), dtype=torch.float32, device=DEV)
        off = 1 if i == UNALIGNED else 0
        t = buf[off:off + h.numel()]
        t.copy_(h)
        assert t.data_ptr() % 16 == 4 * off
        dev.append(t)
    return dict(offsets=offsets, total=total, host=host, dev=dev, numel=(ctypes.c_longlong * len(NUMELS))(*NUMELS),
                ptrs=(VP * len(NUMELS))(*[t.data_ptr() for t in dev]))


def pack_host(host, offsets, row_floats):
    row = np.zeros(row_floats, dtype=np.float32)
    for h, o in zip(host, offsets):
        row[o:o + h.numel()] = h.numpy()
    return row


def export(layout, row, chunk=0, **kw):
    a = dict(grads=layout["ptrs"], numel=layout["numel"], n=len(NUMELS), dst=VP(row.data_ptr()), floats=row.numel(), chunk=chunk)
    a.update(kw)
    ctx = _ctx()
    return ctx.lib.vt_vae_grads_export(ctx.handle, a["grads"], a["numel"], a["n"], a["dst"], a["floats"], a["chunk"], _stream())


def merge(rows, stride, weights, first, floats, out, K=None):
    ctx = _ctx()
    K = len(weights) if K is None else K
    w = (ctypes.c_double * max(1, len(weights)))(*weights)
    return ctx.lib.vt_vae_grads_merge(ctx.handle, VP(rows.data_ptr()), stride, K, w, first, floats, VP(out.data_ptr()), _stream())


def bits(t):
    return t.detach().cpu().numpy().tobytes()


@pytest.mark.parametrize("chunk", [0, 1, 64])
@pytest.mark.parametrize("K", [1, 8])
def test_export_writes_every_float_of_the_row(layout, chunk, K):
    _, row_floats = train_vae.owner_split(layout["total"], K)
    assert (row_floats > layout["total"]) == (K == 8)
    row, guard = _aligned(row_floats)                                           # pre-filled with NaN: every float must be written
    keep = [t.clone() for t in layout["dev"]]
    assert export(layout, row, chunk) == 0
    torch.cuda.synchronize()
    assert bits(row) == pack_host(layout["host"], layout["offsets"], row_floats).tobytes()
    assert torch.isnan(guard).all()                                             # and nothing behind it
    assert all(torch.equal(a, b) for a, b in zip(layout["dev"], keep))          # the gradients are only read


def test_export_refusals_write_nothing(layout):
    row, _ = _aligned(layout["total"])
    ctx = _ctx()
    cases = {"a short row": dict(floats=layout["total"] - TILE), "a row that is no multiple of the tile": dict(floats=layout["total"] + 4),
             "a null row": dict(dst=None), "a misaligned row": dict(dst=VP(row.data_ptr() + 16)), "chunk too large": dict(chunk=_lib.VAE_OPTIM_CHUNK + 1),
             "n < 1": dict(n=0), "null grads": dict(grads=None)}
    for what, kw in cases.items():
        assert export(layout, row, **kw) == 1, what
        assert b"vt_vae_grads_export" in ctx.lib.vt_last_error(ctx.handle)
    torch.cuda.synchronize()
    assert torch.isnan(row).all()


@pytest.fixture(scope="module")
def rank_rows(layout):
    """eight ranks' rows [8][row of K = 8] with every kind of float a gradient row can hold, on the host and on the device"""
    _, row_floats = train_vae.owner_split(layout["total"], 8)
    rng = np.random.default_rng(12)
    rows = (rng.standard_normal((8, row_floats)) * 10.0 ** rng.integers(-8, 4, (8, row_floats))).astype(np.float32)
    rows[:, ::97] = 0.0
    rows[:, 5::389] = -0.0
    rows[:, 11::1013] = np.float32(1e-41)                                       # denormals
    rows[3, layout["total"]:] = 0.0
    dev, _ = _aligned(8 * row_floats)
    dev.copy_(torch.from_numpy(rows.reshape(-1)))
    return rows, dev, row_floats


@pytest.mark.parametrize("K, counts", [(K, c) for K, cs in COUNTS.items() for c in cs])
def test_merge_is_merge_rows_host_byte_for_byte(rank_rows, K, counts):
    rows, dev, row_floats = rank_rows
    w = [c / sum(counts) for c in counts]
    assert len(w) == K
    want = train_vae.merge_rows_host(rows[:K], w)
    out, guard = _aligned(row_floats)
    assert merge(dev, row_floats, w, 0, row_floats, out) == 0                   # the whole row in one call
    torch.cuda.synchronize()
    assert bits(out) == want.tobytes() and torch.isnan(guard).all()
    if K == 1:
        assert bits(out) == rows[0].tobytes()                                   # weight 1 at one rank: the identity, -0.0 and denormals included
    first = bits(out)
    out.fill_(float("nan"))
    assert merge(dev, row_floats, w, 0, row_floats, out) == 0                   # a second run: the same bytes
    assert bits(out) == first
    # a range in one call equals its two halves in two calls; and every owner's range of a K-rank row, merged into a slice of its own
    half = row_floats // TILE // 2 * TILE
    two, _ = _aligned(row_floats)
    assert merge(dev, row_floats, w, 0, half, two) == 0 and merge(dev, row_floats, w, half, row_floats - half, two[half:]) == 0
    assert bits(two) == first
    S, padded = train_vae.owner_split(TILE * 147, K)
    for r in range(K):
        piece, g = _aligned(S * TILE)
        assert merge(dev, row_floats, w, r * S * TILE, S * TILE, piece) == 0
        assert bits(piece) == want[r * S * TILE:(r + 1) * S * TILE].tobytes() and torch.isnan(g).all(), r


def test_merge_refusals_write_nothing(rank_rows):
    rows, dev, row_floats = rank_rows
    out, _ = _aligned(row_floats)
    ctx = _ctx()
    assert merge(dev, row_floats, [1 / 65] * 65, 0, row_floats, out) == 1       # K = 65
    assert b"vt_vae_grads_merge" in ctx.lib.vt_last_error(ctx.handle) and b"65" in ctx.lib.vt_last_error(ctx.handle)
    assert merge(dev, row_floats, [1.0], 0, row_floats, out, K=0) == 1
    assert merge(dev, row_floats, [0.5, -0.5], 0, row_floats, out) == 1
    assert merge(dev, row_floats, [0.5, float("nan")], 0, row_floats, out) == 1
    assert merge(dev, row_floats, [1.0], 4, TILE, out) == 1                     # first_float is no multiple of the tile
    assert merge(dev, row_floats, [1.0], 0, TILE + 4, out) == 1
    assert merge(dev, row_floats, [1.0], 0, 0, out) == 1
    assert merge(dev, row_floats, [1.0], TILE, row_floats, out) == 1            # the range leaves the row
    assert merge(dev, row_floats, [1.0], 0, TILE, out[1:]) == 1                 # a misaligned out
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


def test_norm_on_views_into_a_row_is_the_norm_on_separate_tensors(layout):
    row, _ = _aligned(layout["total"])
    assert export(layout, row) == 0
    views = [row[o:o + n] for o, n in zip(layout["offsets"], NUMELS)]
    copies = [v.clone() for v in views]
    ctx = _ctx()
    need = ctx.lib.vt_vae_optim_workspace_bytes(layout["numel"], len(NUMELS))
    ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    ws_ptr = (ws.data_ptr() + 255) // 256 * 256
    got = []
    for tensors in (views, copies):
        scalars = torch.zeros(2, dtype=torch.float64, device=DEV)
        ptrs = (VP * len(NUMELS))(*[t.data_ptr() for t in tensors])
        ctx.call("vt_vae_optim_norm", ptrs, layout["numel"], len(NUMELS), 1.0, VP(scalars.data_ptr()), VP(ws_ptr), need, 0, _stream())
        got.append(bits(scalars))
    assert got[0] == got[1] and len(got[0]) == 16 and np.frombuffer(got[0][8:12], np.float32)[0] > 0


# ---- the trainer level: two ranks emulated in one process, on the small case of tests/_vae_train_step_ref.py with kl = 0 -------------------
def test_two_emulated_ranks_merge_their_gradients_and_stay_bit_identical():
    from _vae_model_backward_ref import rel, scale_of
    from _vae_train_step_ref import CASES, FIRST, MARGIN, N_LABELS, SEED, SIM, step_refs
    from vae_tagger_amd import synth
    cfg, B, H, W = CASES["small-2x16x24"]
    weights = {"reconstruction": 1.0, "kl": 0.0, "triplet": 1.0}
    p = synth.synth_state_dict({**synth.encoder_manifest(**cfg), **synth.image_decoder_manifest(**cfg)}, seed=5)
    images = synth.synth_images(3 * B, H, W, seed=6)
    g = torch.Generator().manual_seed(8)
    labels = tuple((torch.rand(B, N_LABELS, generator=g) < 0.5).float() for _ in range(2))
    labels[0][:, 0] = 1.0
    a, pos, neg = (images[i * B:(i + 1) * B].to(DEV).contiguous() for i in range(3))
    la, lp = (y.to(DEV) for y in labels)
    trainers = [train_vae.VAETrainer(p, weights=weights, margin=MARGIN, similarity_type=SIM, seed=SEED, device=DEV) for _ in range(2)]
    ranks = train_vae.InProcessRanks(2)
    exchanges = [train_vae.VAEGradientExchange(t, emulated=(ranks, r)) for r, t in enumerate(trainers)]
    assert all(e.active and e.world == 2 and e.bytes_sent_per_step == e.bytes_received_per_step == 4 * e.slice_floats * 2 for e in exchanges)
    # rank r holds image r of the global batch: batch 1, the noise of the global index FIRST + r
    own = [trainers[r].forward_backward(a[r:r + 1], pos[r:r + 1], neg[r:r + 1], la[r:r + 1], lp[r:r + 1], FIRST + r)[1] for r in range(2)]
    w = train_vae.shard_weights(2, 2, 1)
    assert w == [0.5, 0.5]
    for e, grads in zip(exchanges, own):
        e.export(grads)
    for e in exchanges:
        e.merge(w)
    merged = [e.gather() for e in exchanges]
    torch.cuda.synchronize()
    assert exchanges[0].calls == exchanges[1].calls == 1 and list(merged[0]) == list(trainers[0].params)
    for k in trainers[0].params:
        want = train_vae.merge_rows_host([own[0][k].cpu().numpy(), own[1][k].cpu().numpy()], w)
        assert bits(merged[0][k]) == bits(merged[1][k]) == want.tobytes(), k
        assert merged[0][k].shape == trainers[0].params[k].shape
    assert bits(exchanges[0].merged) == bits(exchanges[1].merged)                # the padding too
    digests = []
    for t, m in zip(trainers, merged):
        t.clip(m, 1.0)
        t.step(m, 3e-4, 1e-6)
        digests.append(t.optimizer_state_sha256().hexdigest())
    fresh = train_vae.VAETrainer(p, weights=weights, margin=MARGIN, similarity_type=SIM, seed=SEED, device=DEV)
    assert digests[0] == digests[1] != fresh.optimizer_state_sha256().hexdigest()
    # recorded, not asserted: the merged gradient against the device's own batch-2 gradient (summation order only), beside the restatement's
    # d_emu for the tensor (both relative to the tensor's largest exact value)
    _, both = fresh.forward_backward(a, pos, neg, la, lp, FIRST)
    ctx = _ctx()

    def device_eps(draw):
        h, wd = H >> (len(cfg["block_out"]) - 1), W >> (len(cfg["block_out"]) - 1)
        zero, z = torch.zeros(B, 32, h, wd, device=DEV), torch.empty(B, 16, h, wd, device=DEV)
        ctx.call("vt_posterior_sample", VP(zero.data_ptr()), B, 16, h * wd, SEED, draw, FIRST, VP(z.data_ptr()), None, None)
        return z.cpu()

    refs = step_refs(p, images, [device_eps(d) for d in range(4)], labels, weights, MARGIN, SIM)
    worst = (0.0, None)
    for k in trainers[0].params:
        d_order = ((merged[0][k].double() - both[k].double()).abs().max().cpu() / scale_of(refs["exact"], k)).item()
        d_emu, d_hip = rel(refs["emu"][k], refs["exact"], k), rel(both[k].cpu(), refs["exact"], k)
        print(f"    {k}: merged vs batch-2 {d_order:.3e}  d_emu {d_emu:.3e}  d_hip(batch-2) {d_hip:.3e}")
        if d_emu > 0 and d_order / d_emu > worst[0]:
            worst = (d_order / d_emu, k)
    print(f"    largest (merged vs batch-2) / d_emu {worst[0]:.3e} ({worst[1]})")


def test_an_exchange_without_a_group_returns_what_it_was_given():
    from vae_tagger_amd import synth
    cfg = dict(block_out=(64, 512), layers_per_block=1)
    p = synth.synth_state_dict({**synth.encoder_manifest(**cfg), **synth.image_decoder_manifest(**cfg)}, seed=1)
    t = train_vae.VAETrainer(p, weights={"reconstruction": 1.0}, device=DEV)
    e = train_vae.VAEGradientExchange(t)
    grads = {"x": None}
    assert not e.active and e.exchange(grads, [1.0]) is grads and e.calls == 0 and e.bytes_sent_per_step == 0
    with pytest.raises(_lib.VTError, match="vt_vae_grads_merge"):
        row = t._aligned(t.total)
        t.merge_gradients(row, t.total, [1 / 65] * 65, 0, t.total, t._aligned(t.total))
