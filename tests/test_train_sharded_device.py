"""GPU: the gradient exchange of sharded training (vt_*_grads_export / vt_*_grads_merge, csrc/train_common.hip; train.GradientExchange's
device side).  The merge is compared BIT FOR BIT with train.merge_gradients_host (fp64, rank order, separate multiply and add, one final
cast) on every trainer block; the squared-norm partials it rewrites are checked through clip(); two emulated ranks in one process end
with the same state and a merged gradient that is the whole batch's by the rule of test_train_device.py."""
import math

import numpy as np
import pytest
import torch

from vae_tagger_amd import _lib, synth
from vae_tagger_amd.train import DecoderTrainer, HeadTrainer, exchange_weights, merge_gradients_host

from test_train_device import FACTOR, FLOOR, all_gradients, batch, check, decoder, torch_grads  # noqa: F401  (FACTOR / FLOOR: check's rule)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COUNTS = {1: [7], 2: [5, 0], 3: [3, 0, 4], 8: [4, 2, 0, 4, 1, 4, 3, 4]}       # images per rank: unequal weights, one of them 0
_CROSS = {}


def cross_decoder(N=11):
    if N not in _CROSS:
        from vae_tagger_amd.modules import AttentionClassificationDecoder
        d = AttentionClassificationDecoder(16, 16, 16, N, True, True, True, 8)
        d.load_state_dict(synth.synth_state_dict(synth.attention_decoder_manifest(N, 16, True, True, True), seed=1), strict=False)
        _CROSS[N] = d.to(DEV).eval()
    return _CROSS[N]


def block_trainer(which):
    """(the block, the trainer whose clip() covers it).  head11 / head70: ragged last rows and chunks; front: P = 2240 over 16 partials;
    cross: 530 176 floats over 274 partials.  The front and the cross block have no clip of their own: DecoderTrainer's one clip runs
    over all blocks, and the blocks that are not merged into hold zero gradients and zero partials, so its norm is the merged block's."""
    if which == "head11":
        tr = HeadTrainer(decoder(False, 11)[0])
        return tr, tr
    if which == "head70":
        tr = HeadTrainer(decoder(False, 70)[0])
        return tr, tr
    whole = DecoderTrainer(cross_decoder() if which == "cross" else decoder(False, 11)[0])
    return (whole.cross if which == "cross" else whole.front), whole


def sources(K, stride, seed):
    """[K][stride] fp32 of mixed magnitude: normal values times 10^(-6 .. 6), a few exact zeros."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(K, stride, generator=g) * 10.0 ** torch.randint(-6, 7, (K, stride), generator=g).float()
    x[torch.rand(K, stride, generator=g) < 0.01] = 0.0
    return x.contiguous()


def exported(tr):
    out = torch.empty(tr.grads_floats(), dtype=torch.float32, device=DEV)
    tr.export_gradients(out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def one_ulp(x):
    return float(np.spacing(np.float32(x)))


# ---- 1. bit for bit against the host reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("which", ["head11", "head70", "front", "cross"])
def test_merge_equals_the_host_reference_bit_for_bit(which, K):
    tr, whole = block_trainer(which)
    P = tr.grads_floats()
    assert P > 0 and P % 64 == 0
    if which == "front":
        assert P == 2240
    if which == "cross":
        assert P == 530176
    host = sources(K, P, seed=17 * K + len(which))
    w = [1.0] if K == 1 else exchange_weights(COUNTS[K])
    assert K == 1 or (0.0 in w and len(set(w)) >= min(K, 3))
    src = host.to(DEV)
    before = src.clone()
    want = merge_gradients_host(host.numpy(), w)
    tr.merge_gradients(src, P, w)
    got = exported(tr)
    assert same_bits(got, want), f"{which} K={K}: {(got.view(np.uint32) != want.view(np.uint32)).sum()} of {P} floats differ"
    if K == 1:
        assert same_bits(got, host.numpy()[0])                       # one rank at weight 1: the input's bits
    assert torch.equal(src, before)                                  # the sources are not changed
    # the squared-norm partials the same launch rewrote, through clip: sqrt of the fp64 sum of squares of the merged values, to 1 fp32 ulp
    # (the fp64 summation order is the only difference)
    whole.clip(1e30)
    norm = math.sqrt(float((want.astype(np.float64) ** 2).sum()))
    got_norm, coef = tr.grad_norm()
    assert whole.grad_norm() == (got_norm, coef)
    print(f"{which} K={K}: norm device {got_norm!r} host {np.float32(norm)!r}")
    assert abs(got_norm - float(np.float32(norm))) <= one_ulp(norm) and coef == 1.0
    first = tr.state_bytes()
    tr.merge_gradients(src, P, w)                                    # a second run: identical state bytes
    whole.clip(1e30)
    assert torch.equal(tr.state_bytes(), first)
    assert same_bits(exported(tr), want)                             # (a clip inside the bound keeps the gradients' bits)


@pytest.mark.parametrize("cross", [False, True], ids=["front+head", "front+cross+head"])
def test_packed_blocks_merge_at_a_stride_larger_than_P(cross):
    """DecoderTrainer's blocks side by side in one row [P_front (+ P_cross) + P_head], K rows at stride P_total (and at the exchange's
    row, P_total + 4): every block merges its own range."""
    tr = DecoderTrainer(cross_decoder() if cross else decoder(False, 11)[0])
    parts = [b.grads_floats() for b in tr.blocks()]
    total = tr.grads_floats()
    assert total == sum(parts) and len(parts) == (3 if cross else 2) and all(p < total for p in parts)
    K = 3
    w = exchange_weights(COUNTS[K])
    for stride in (total, total + 4):
        host = sources(K, stride, seed=5 + stride % 7)
        src = host.to(DEV)
        tr.merge_gradients(src, stride, w)
        out = torch.empty(total, dtype=torch.float32, device=DEV)
        tr.export_gradients(out)
        torch.cuda.synchronize()
        want = merge_gradients_host(host.numpy()[:, :total], w)
        assert same_bits(out.cpu().numpy(), want)
        assert torch.equal(src.cpu(), host)
        tr.clip(1e30)                                                # ONE norm over all blocks, from the rewritten partials
        norm = math.sqrt(float((want.astype(np.float64) ** 2).sum()))
        assert abs(tr.grad_norm()[0] - float(np.float32(norm))) <= one_ulp(norm)


# ---- 2. two emulated ranks in one process -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [(3, 3), (4, 2)], ids=["3+3", "4+2"])
def test_two_emulated_ranks_end_with_one_state_and_the_whole_batch_gradient(split):
    N, B, plain = 70, 6, False
    dec, sd = decoder(plain, N)
    x, y = batch(plain, N, B, seed=61, labels="f32")
    ranks = [HeadTrainer(dec, dropout=(0.0, 0.0, 0.0), seed=s) for s in (0, 1000003)]
    whole = HeadTrainer(dec, dropout=(0.0, 0.0, 0.0))
    assert torch.equal(ranks[0].state_bytes(), ranks[1].state_bytes())
    P = whole.grads_floats()
    rows = torch.zeros(2, P, dtype=torch.float32, device=DEV)
    lo = 0
    for r, n in enumerate(split):
        ranks[r].forward_backward(x[lo:lo + n], y[lo:lo + n], train=True, step=0)
        ranks[r].export_gradients(rows[r])
        lo += n
    w = exchange_weights(split)
    for tr in ranks:
        tr.merge_gradients(rows, P, w)
    whole.forward_backward(x, y, train=True, step=0)
    _, g64 = torch_grads(sd, plain, torch.float64, x, y, "bce", {})
    _, g32 = torch_grads(sd, plain, torch.float32, x, y, "bce", {})
    merged, one = all_gradients(ranks[0]), all_gradients(whole)
    worst = [0.0, 0.0]
    for k in merged:
        assert torch.equal(merged[k], ranks[1].gradient(k))
        worst[0] = max(worst[0], check("merged " + k, merged[k], g64[k], g32[k]))
        worst[1] = max(worst[1], check("whole  " + k, one[k], g64[k], g32[k]))
    print(f"two ranks {split}: worst device/e32 merged = {worst[0]:.3f}, one trainer on the whole batch = {worst[1]:.3f}")
    for tr in ranks:
        tr.clip(1.0)
        tr.step(1e-3, 1e-6)
    assert ranks[0].grad_norm() == ranks[1].grad_norm()
    for k in ranks[0].shapes:
        for kind in (_lib.HEAD_PARAM, _lib.HEAD_GRAD, _lib.HEAD_ADAM_M, _lib.HEAD_ADAM_V):
            a, b = (t._read(kind, k, t.shapes[k], torch.float32) for t in ranks)
            assert torch.equal(a, b), (k, kind)
    # the whole blocks: the ranks saw different images, so the ONE fp64 slot of the loss ring that step 0 wrote differs; nothing else may
    a, b = (t.state_bytes().numpy() for t in ranks)
    diff = np.flatnonzero(a != b)
    la, lb = float(ranks[0].losses()[0]), float(ranks[1].losses()[0])
    assert la != lb and diff.size and diff[-1] // 8 == diff[0] // 8, f"{diff.size} bytes differ outside one loss slot"
    assert not torch.equal(ranks[0].parameter("classifier.12.weight"), sd["classifier.12.weight"])


# ---- 3. bad input ---------------------------------------------------------------------------------------------------------------------------
def test_bad_input_fails_and_leaves_the_state_alone():
    tr = HeadTrainer(decoder(False, 11)[0])
    P = tr.grads_floats()
    src = sources(2, P + 4, seed=3).to(DEV)
    tr.merge_gradients(src, P + 4, [0.5, 0.5])
    before = tr.state_bytes()
    for what, call in (("K = 0", lambda: tr.merge_gradients(src, P + 4, [])),
                       ("K = 65", lambda: tr.merge_gradients(src, P + 4, [1.0 / 65] * 65)),
                       ("a NaN weight", lambda: tr.merge_gradients(src, P + 4, [0.5, float("nan")])),
                       ("a negative weight", lambda: tr.merge_gradients(src, P + 4, [1.5, -0.5])),
                       ("a misaligned source", lambda: tr.merge_gradients(src.view(-1)[1:], P + 4, [1.0])),
                       ("a stride below P", lambda: tr.merge_gradients(src, P - 4, [0.5, 0.5]))):
        with pytest.raises(_lib.VTError, match="vt_head_grads_merge"):
            call()
        assert torch.equal(tr.state_bytes(), before), what
    small = torch.empty(P - 4, dtype=torch.float32, device=DEV)
    with pytest.raises(_lib.VTError, match="vt_head_grads_export"):
        tr.export_gradients(small)
