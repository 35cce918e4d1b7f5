"""Gradient accumulation of train_full on the host: the flag surface, accumulation_plan against a literal simulation of the reference's counters
(train_full.py:201-255: `step` from enumerate inside the epoch, a gradient that is zeroed only where the optimiser steps), the numpy mirror of
vt_vae_grads_accumulate against torch's separately rounded CPU ops, and the new entry of the C ABI (header, _lib.PROTOTYPES, the built library)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from vae_tagger_amd import _lib, train_full, train_vae

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = train_vae.TILE
REQUIRED = ["--json_path", "j", "--tags_csv_path", "t"]


def test_flag_surface():
    parse = lambda *flags: train_full.build_parser().parse_args(REQUIRED + list(flags))
    assert parse().accumulate_gradients is False                                                # off by default
    args = train_full.check_args(parse("--accumulate_gradients", "--gradient_accumulation_steps", "3"))
    assert args.accumulate_gradients is True and args.gradient_accumulation_steps == 3
    train_full.check_args(parse("--accumulate_gradients"))                                      # A = 1 with the flag
    train_full.check_args(parse("--accumulate_gradients", "--gradient_accumulation_steps", "1"))
    with pytest.raises(RuntimeError) as e:                                                      # A = 3 without the flag: both flags named
        train_full.check_args(parse("--gradient_accumulation_steps", "3"))
    assert "--gradient_accumulation_steps" in str(e.value) and "--accumulate_gradients" in str(e.value)
    with pytest.raises(SystemExit, match=re.escape("--accumulate_gradients")):
        train_full.main(REQUIRED + ["--gradient_accumulation_steps", "3"])
    for bad in ("0", "-2"):
        with pytest.raises(RuntimeError, match=re.escape("--accumulate_gradients")):
            train_full.check_args(parse("--accumulate_gradients", "--gradient_accumulation_steps", bad))
    with pytest.raises(RuntimeError, match=re.escape("--sharded")):                             # --sharded stays refused
        train_full.check_args(parse("--accumulate_gradients", "--gradient_accumulation_steps", "2", "--sharded"))


def _reference_counters(spe, epochs, A):
    """The reference's loop with the model taken out: the gradient is a bag of micro-step ids that backward() adds to and zero_grad() empties."""
    bag, micro, steps, pending_at_epoch_end, flags = [], 0, [], [], []
    for epoch in range(epochs):
        for step in range(spe):                                                 # for step, batch in enumerate(train_dataloader)
            first = not bag
            bag.append(micro)                                                   # accelerator.backward(total_loss / A)
            now = (step + 1) % A == 0                                           # if (step + 1) % args.gradient_accumulation_steps == 0
            if now:
                steps.append(list(bag))                                         # optimizer.step(); lr_scheduler.step()
                bag = []                                                        # optimizer.zero_grad()
            flags.append((epoch, step, first, now))
            micro += 1
        pending_at_epoch_end.append(list(bag))
    return steps, pending_at_epoch_end, flags


@pytest.mark.parametrize("spe, epochs, A", [(4, 2, 3), (4, 2, 2), (5, 3, 4), (1, 3, 2), (4, 2, 1)])
def test_accumulation_plan_is_the_references_counters(spe, epochs, A):
    want_steps, want_pending, want_flags = _reference_counters(spe, epochs, A)
    plan = list(train_full.accumulation_plan(spe, epochs, A))
    assert plan == want_flags and len(plan) == spe * epochs
    bag, steps, pending = [], [], []
    for micro, (epoch, step, first, now) in enumerate(plan):
        assert first == (not bag)
        bag.append(micro)
        if now:
            steps.append(bag)
            bag = []
        if step == spe - 1:
            pending.append(list(bag))
    assert steps == want_steps and pending == want_pending
    assert len(steps) == epochs * (spe // A)                                    # the optimiser-step count
    if (spe, epochs, A) == (4, 2, 3):
        assert steps == [[0, 1, 2], [3, 4, 5, 6]] and pending == [[3], [7]]     # the tail of epoch 0 rides into epoch 1's first optimiser step
    if (spe, epochs, A) == (1, 3, 2):
        assert steps == [] and pending == [[0], [0, 1], [0, 1, 2]]              # (1 + 0) % 2 is never 0: the reference never steps
    if A == 1:
        assert all(first and now for _, _, first, now in plan)
    with pytest.raises(ValueError):
        list(train_full.accumulation_plan(spe, epochs, 0))


def _spread(rng, n):
    return (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 21, n)).astype(np.float32)


@pytest.mark.parametrize("s", [1.0, 1.0 / 3.0])
@pytest.mark.parametrize("c", [0.37, 1.0, float("nan")])
def test_accumulate_rows_host_is_torchs_separately_rounded_ops(c, s):
    rng = np.random.default_rng(21)
    numels = [1, 3, 4097, 5, 2 * TILE]
    offsets, total = train_vae.optim_layout(numels)
    grads = [_spread(rng, n) for n in numels]
    row = _spread(rng, total)
    grads[1][0], row[offsets[1] + 1] = -0.0, -0.0
    s32, c32 = np.float32(s), np.float32(c)
    got = train_vae.accumulate_rows_host(row, grads, offsets, numels, s, c, first=False)
    assert got.dtype == np.float32 and got is not row
    want = torch.from_numpy(row.copy())
    fused_differs = 0
    for g, o, n in zip(grads, offsets, numels):
        view = want[o:o + n]
        if c < 1.0:                                                             # NaN and >= 1: no multiply
            view.mul_(float(c32))
        view.add_(float(s32) * torch.from_numpy(g))
        a64 = row[o:o + n].astype(np.float64) * (np.float64(c32) if c < 1.0 else 1.0)       # exact: 24 + 24 bits
        t64 = g.astype(np.float64) * np.float64(s32)
        for fused in ((a64 + (g * s32).astype(np.float64)).astype(np.float32),               # fma(c, a, t)
                      ((row[o:o + n] * (c32 if c < 1.0 else np.float32(1))).astype(np.float64) + t64).astype(np.float32)):      # fma(s, g, a)
            fused_differs += int((fused.view(np.uint32) != got[o:o + n].view(np.uint32)).sum())
    assert torch.equal(torch.from_numpy(got), want) and got.tobytes() == want.numpy().tobytes()
    if c < 1.0 or s != 1.0:
        assert fused_differs > 0, "the data must hold elements on which a fused multiply-add of the same operands has other bits"
    # outside the tensors' elements the row keeps its bytes; the input row is not changed
    mask = np.ones(total, dtype=bool)
    for o, n in zip(offsets, numels):
        mask[o:o + n] = False
    assert got[mask].tobytes() == row[mask].tobytes()
    # first: t at the slots, zero everywhere else, whatever the row held and whatever the coefficient
    first = train_vae.accumulate_rows_host(row, grads, offsets, numels, s, c, first=True)
    assert not first[mask].any() and not np.signbit(first[mask]).any()
    for g, o, n in zip(grads, offsets, numels):
        assert first[o:o + n].tobytes() == (g if s == 1.0 else g * s32).tobytes()
    assert np.signbit(first[offsets[1]])                                        # -0.0 travels at scale 1 and under a positive scale
    assert train_vae.accumulate_rows_host(row, grads, offsets, numels, s, None, first=False).tobytes() == \
        train_vae.accumulate_rows_host(row, grads, offsets, numels, s, 1.0, first=False).tobytes()


def _header_argument_count(header, name):
    m = re.search(r"\b" + name + r"\s*\(", header)
    assert m, f"{name} is not declared in the header"
    depth, i = 1, m.end()
    while depth:
        depth += {"(": 1, ")": -1}.get(header[i], 0)
        i += 1
    body = re.sub(r"/\*.*?\*/", "", header[m.end():i - 1], flags=re.S)
    return len([a for a in body.split(",") if a.strip()])


def test_the_new_entry_in_header_prototypes_and_library():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "vae_tagger_hip.h")).read()
    name = "vt_vae_grads_accumulate"
    res, args = _lib.PROTOTYPES[name]
    declared = [m.start() for m in re.finditer(r"\bint " + name + r"\(", header)]
    assert len(declared) == 1
    assert _header_argument_count(header[declared[0]:], name) == len(args) == 11
    fn = getattr(lib, name)
    assert fn.restype == res == ctypes.c_int and list(fn.argtypes) == list(args)
    # the export's arguments, then scale, scalars and first before chunk and stream
    export = _lib.PROTOTYPES["vt_vae_grads_export"][1]
    assert list(args[:6]) == list(export[:6]) and list(args[6:]) == [ctypes.c_float, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    one = (ctypes.c_longlong * 1)(4)
    assert lib.vt_vae_grads_accumulate(None, None, one, 1, None, TILE, 1.0, None, 1, 0, None) == 1          # no context
