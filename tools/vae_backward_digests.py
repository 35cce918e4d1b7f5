"""SHA-256 digests of what the training operators compute through vae_tagger_amd.vae_backward: every backward operator at two shapes (and, where
flags 0, 22 or 23 choose the route, under each of them), the attention block's training forward and backward, and one whole vae_loss_and_grads
step per case of tests/_vae_train_step_ref.CASES -- what a change to the host layer between the tests and the kernels (ops_backward.hip,
attention_backward.hip, vae_backward.py) must leave bit for bit.  One `name sha256` line per output tensor.

    cd <root of the tree to be measured> && python <this file> > digests.txt

The package and tests/ are imported from the current directory and only public vae_backward names are used, so the same file measures a built
checkout of another commit when it is run from that checkout's root; two trees agree when their outputs are identical (`cmp`)."""
import hashlib
import os
import sys
import zlib

sys.path[:0] = [os.getcwd(), os.path.join(os.getcwd(), "tests")]
import torch
import _vae_train_step_ref as step_ref
from vae_tagger_amd import synth
from vae_tagger_amd import vae_backward as vb

DEV = "cuda:0"
BIG, ODD = (2, 8, 8), (1, 5, 7)               # B, H, W: whole tiles on the halo route's channel counts / an odd size that ends inside a tile
ROUTES = [{}, {0: 0}, {22: 1}, {23: 1}]        # the settings under which a data gradient takes its other route (defaults: flag 0 on, 22 and 23 off)
DEFAULTS = {0: 1, 22: 0, 23: 0}
BF = torch.bfloat16


def dig(name, t):
    print(name, "none" if t is None else hashlib.sha256(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest(), flush=True)


def rnd(name, *shape, dtype=torch.float32, scale=1.0):
    """a seeded CPU draw, keyed by the case's name and the tensor's shape, on the device"""
    g = torch.Generator().manual_seed(zlib.crc32(f"{name}{shape}".encode()))
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(DEV).contiguous()


def routed(name, fn):
    ctx = vb.context(DEV)
    for flags in ROUTES:
        try:
            for f, v in flags.items():
                ctx.call("vt_set_flag", f, v)
            dig(name + "".join(f"/flag{f}={v}" for f, v in flags.items()), fn())
        finally:
            for f, v in DEFAULTS.items():
                ctx.call("vt_set_flag", f, v)


def operators(tag, B, H, W, c_any, c_pair8, c_pair64, c_gn, groups, c_up8, c_wide, c_thin):
    """c_any: cast_bias_grad's C; c_pair8 / c_pair64: the (Cin, Cout) pairs of the data / weight gradients; c_gn, groups: GroupNorm; c_up8: Upsample2D's
    data gradient; c_wide: the thin weight gradient's wide side and Upsample2D's weight gradient; c_thin: conv_thin_forward's C"""
    n = f"{tag}/cast_bias_grad"
    for out, t in zip(("dy16", "dbias"), vb.cast_bias_grad(rnd(n, B, H, W, c_any))):
        dig(f"{n}/{out}", t)
    for ci, co in c_pair8:
        for k in (1, 3):
            n = f"{tag}/conv_backward_data/k{k}/{ci}-{co}"
            dy16, w, add = rnd(n, B, H, W, co, dtype=BF), rnd(n, co, ci, k, k, scale=0.05), rnd(n, B, H, W, ci)
            routed(n, lambda: vb.conv_backward_data(dy16, w, dx_add=add))
        n = f"{tag}/downsample_backward_data/{ci}-{co}"
        dy16, w, add = rnd(n, B, H // 2, W // 2, co, dtype=BF), rnd(n, co, ci, 3, 3, scale=0.05), rnd(n, B, H, W, ci)
        routed(n, lambda: vb.downsample_backward_data(dy16, w, H, W, dx_add=add))
    n = f"{tag}/upsample_backward_data/{c_up8}"
    dy16, w, add = rnd(n, B, 2 * H, 2 * W, c_up8, dtype=BF), rnd(n, c_up8, c_up8, 3, 3, scale=0.05), rnd(n, B, H, W, c_up8)
    routed(n, lambda: vb.upsample_backward_data(dy16, w, dx_add=add))
    for ci, co in c_pair64:
        for k in (1, 3):
            n = f"{tag}/conv_backward_weight/k{k}/{ci}-{co}"
            dig(n, vb.conv_backward_weight(rnd(n, B, H, W, co, dtype=BF), rnd(n, B, H, W, ci, dtype=BF), k))
        n = f"{tag}/downsample_backward_weight/{ci}-{co}"
        dig(n, vb.downsample_backward_weight(rnd(n, B, H // 2, W // 2, co, dtype=BF), rnd(n, B, H, W, ci, dtype=BF)))
    n = f"{tag}/upsample_backward_weight/{c_wide}"
    dig(n, vb.upsample_backward_weight(rnd(n, B, 2 * H, 2 * W, c_wide, dtype=BF), rnd(n, B, H, W, c_wide, dtype=BF)))
    n = f"{tag}/groupnorm/{c_gn}"
    x, gamma, beta, d, add = rnd(n, B, H, W, c_gn), rnd(n + "g", c_gn), rnd(n + "b", c_gn), rnd(n + "d", B, H, W, c_gn), rnd(n + "a", B, H, W, c_gn)
    stats = vb.groupnorm_stats(x, groups=groups)
    dig(f"{n}/stats", stats)
    for fn in (vb.groupnorm_silu_backward, vb.groupnorm_backward):
        for out, t in zip(("dx", "dx16", "dgamma", "dbeta"), fn(x, stats, gamma, beta, d, dx_add=add, want_dx16=True)):
            dig(f"{n}/{fn.__name__}/{out}", t)
    for thin_is_input in (True, False):
        n = f"{tag}/conv_thin_backward_weight/{c_wide}/thin_is_input={int(thin_is_input)}"
        for out, t in zip(("dw", "sums"), vb.conv_thin_backward_weight(rnd(n, B, 3, H, W), rnd(n, B, H, W, c_wide, dtype=BF), thin_is_input, want_sums=True)):
            dig(f"{n}/{out}", t)
    for tr in (False, True):
        n = f"{tag}/conv_thin_forward/{c_thin}/transpose_rotate={int(tr)}"
        w = rnd(n, *((3, c_thin, 3, 3) if tr else (c_thin, 3, 3, 3)), scale=0.2)
        for out, t in zip(("o32", "o16"), vb.conv_thin_forward(rnd(n, B, 3, H, W), w, None if tr else rnd(n, c_thin), transpose_rotate=tr, want_bf16=True)):
            dig(f"{n}/{out}", t)


def attention(B, H, W):
    n, C = f"attention/{B}x{H}x{W}", vb.ATTN_C
    p = {k: rnd(n + k, *((C, C) if k.endswith("weight") and not k.startswith("group_norm") else (C,)), scale=0.04) for k in vb.ATTN_PARAMS}
    y, saved = vb.attention_block_forward_train(p, rnd(n, B, H, W, C))
    dig(f"{n}/y", y)
    for k in vb.ATTN_SAVED[1:]:
        dig(f"{n}/saved/{k}", saved[k][..., :H * W] if k == "vT16" else saved[k])         # (the pitch's padding columns are never written)
    dx, g = vb.attention_block_backward(p, saved, rnd(n + "dy", B, H, W, C))
    dig(f"{n}/dx", dx)
    for k, v in g.items():
        dig(f"{n}/grad/{k}", v)


def step(name):
    cfg, B, H, W = step_ref.CASES[name]
    p = {k: v.to(DEV).contiguous() for k, v in synth.synth_state_dict({**synth.encoder_manifest(**cfg), **synth.image_decoder_manifest(**cfg)}, seed=5).items()}
    a, pos, neg = (t.to(DEV).contiguous() for t in synth.synth_images(3 * B, H, W, seed=6).split(B))
    g = torch.Generator().manual_seed(8)
    la, lp = ((torch.rand(B, step_ref.N_LABELS, generator=g) < 0.5).float().to(DEV) for _ in range(2))
    losses, grads = vb.vae_loss_and_grads(p, a, pos, neg, la, lp, weights=step_ref.WEIGHTS, margin=step_ref.MARGIN, similarity_type=step_ref.SIM,
                                          seed=step_ref.SEED, first_image=step_ref.FIRST)
    for k, v in losses.items():
        dig(f"step/{name}/loss/{k}", v)
    for k, v in grads.items():
        dig(f"step/{name}/grad/{k}", v)


operators("big", *BIG, 128, [(64, 128), (128, 64)], [(64, 128)], 128, 32, 128, 128, 128)
operators("odd", *ODD, 4, [(8, 8)], [(64, 64)], 16, 8, 8, 64, 8)
attention(2, 4, 4)
attention(1, 3, 5)
for case in step_ref.CASES:
    step(case)
torch.cuda.synchronize()
