"""Mid-block attention inputs whose softmax is known by construction (pure torch, CPU): every query's row is a selection of one key
position, an equal-weight average of four, or the plain mean of all S -- so the expected output is a closed form of the value rows,
and a wrong, dropped, duplicated, leaked or foreign key moves it by O(1) of the value scale.

Weights (attention_weights): to_q reads token channels 0..127 (x 8), to_k channels 128..255 (x 8), to_v channels 256..511 (x 1, into
value channels 0..255), to_out is the identity, all biases zero.  A token x = [qcode | kcode | payload] therefore sets q = 8 qcode,
k = 8 kcode, v = payload independently; the S x S products still run dense on whatever kernel takes them.

Codes are two-hot in the 128 code dimensions, e[c % 64] + e[64 + c // 64] (4096 codes).  At amplitude 4 (q, k entries 32) a full
match scores 2 * 32^2 / sqrt(512) = 90.5, a half match 45.25, no match 0: every weight off the selection is below e^-45 < 1e-19.
All of x, q, k, v and 8 x them are exact in bf16 and in float8_e4m3fn, so the bf16 and the fp8 kernels multiply the same numbers.

Families:
  select        key position j of image b holds code perm_b[j]; query i selects position j_b(i): out = payload[b, j_b(i)] + residual
  select_loose  the same at amplitude 6 (full match 203.6): the operand-norm bound of mode 0 is too loose, the exact-maximum path must run
  avg4          codes shared by groups of exactly four positions: out = mean of the four payloads (weights exactly 0.25) + residual
  allneg        qcode = -2, kcode = +4 on one channel for every token: all S^2 scores are -22.63, out = mean of all S payloads + residual;
                a pad key counted with score 0 outweighs every real key by e^22.6
"""
import functools
import math
from types import SimpleNamespace

import torch

C = 512
NCODE = 128                       # code dimensions: 64 + 64, two-hot
PAYLOAD = 256                     # value channels
TAG = (PAYLOAD - 2, PAYLOAD - 1)  # payload channels that carry the image index
A = "encoder.mid_block.attentions.0."
FAMILIES = ("select", "select_loose", "avg4", "allneg")
AMPLITUDE = {"select": 4.0, "select_loose": 6.0, "avg4": 4.0, "allneg": None}
PAYLOAD_MAX = 7.0
MAX_GAP = 120.0                   # run_attention's threshold on u - l

# (B, S): the smallest sizes that reach each unit of the kernels (256-query workgroups of 32-query slabs; 64-key tiles in bf16, 128-key
# tiles in fp8; v^T pitch S rounded to 8 / 16 with the +2112 pad at 2-KB multiples; key sweeps split in 2 at S = 1024 and 4 at 2048; the fp8
# sampled maximum from 16 key tiles; the 256-channel P.V forms from 96 query blocks)
SHAPES_COMMON = ((3, 64), (3, 130), (2, 333), (2, 1024), (2, 1021), (1, 2048), (1, 2044))
SHAPES_BF16 = SHAPES_COMMON + ((96, 40),)
SHAPES_FP8 = SHAPES_COMMON + ((48, 300),)
SHAPES_ALL = SHAPES_COMMON + ((96, 40), (48, 300))
RAGGED = ((3, 130), (2, 333), (2, 1021), (1, 2044))


def attention_weights(sd):
    """-> a copy of the state dict `sd` with the mid-block attention's tensors replaced by the construction's."""
    sd = dict(sd)
    wq, wk, wv = torch.zeros(C, C), torch.zeros(C, C), torch.zeros(C, C)
    i = torch.arange(NCODE)
    wq[i, i] = 8.0
    wk[i, NCODE + i] = 8.0
    j = torch.arange(PAYLOAD)
    wv[j, 2 * NCODE + j] = 1.0
    for name, w in (("to_q", wq), ("to_k", wk), ("to_v", wv), ("to_out.0", torch.eye(C))):
        assert sd[A + name + ".weight"].shape == w.shape
        sd[A + name + ".weight"] = w
        sd[A + name + ".bias"] = torch.zeros(C)
    return sd


def code_vectors(codes, amp):
    """codes [...] int64 in [0, 4096) -> [..., 128] two-hot rows of height amp"""
    out = torch.zeros(codes.shape + (NCODE,))
    out.scatter_(-1, (codes % 64).unsqueeze(-1), amp)
    out.scatter_(-1, (64 + codes // 64).unsqueeze(-1), amp)
    return out


def _payload(B, S, g, lo):
    """multiples of 0.5 in [lo / 2, 7]; the two tag channels hold the decimal digits of the image index (+ 1) x 0.5"""
    p = torch.randint(lo, 15, (B, S, PAYLOAD), generator=g).float() * 0.5
    b = torch.arange(B)
    p[:, :, TAG[0]] = ((b // 10 + 1) * 0.5).view(B, 1)
    p[:, :, TAG[1]] = ((b % 10 + 1) * 0.5).view(B, 1)
    return p


def _select_positions(S, g):
    """j(i): query 0 -> the last key, query S - 1 -> key 0, queries 1.. -> the keys either side of the 32 / 64 / 128 boundaries, the rest random"""
    j = torch.randint(0, S, (S,), generator=g)
    j[0], j[S - 1] = S - 1, 0
    for t, pos in enumerate((31, 32, 63, 64, 127, 128)):
        if pos < S and 1 + t < S - 1:
            j[1 + t] = pos
    return j


def _avg4_groups(S, g):
    """-> (groups [S // 4, 4] of key positions, leftover positions): group 0 is {0, 63, 64, S - 1} as far as those exist (filled up with
    other positions, never position 1), group 1 at S >= 1024 has one key in each quarter of the key range, the rest is a random partition"""
    first = []
    for p in (0, 63, 64, S - 1):
        if p < S and p not in first:
            first.append(p)
    fixed = [first]
    if S >= 1024:
        q = S // 4                                                # (100 keys off the quarter boundaries: clear of group 0 and of any tile edge)
        fixed.append([s * q + 100 + int(torch.randint(0, q - 200, (1,), generator=g)) for s in range(4)])
    used = {p for grp in fixed for p in grp}
    rest = [int(p) for p in torch.randperm(S, generator=g) if int(p) not in used and int(p) != 1]
    while len(fixed[0]) < 4:
        fixed[0].append(rest.pop())
    rest.append(1)
    n = S // 4
    groups = fixed + [rest[4 * t:4 * t + 4] for t in range(n - len(fixed))]
    left = rest[4 * (n - len(fixed)):]
    assert len(groups) == n and all(len(grp) == 4 for grp in groups) and len(left) == S % 4
    assert len({p for grp in groups for p in grp} | set(left)) == S
    return torch.tensor(groups), left


@functools.lru_cache(maxsize=None)
def make_case(family, B, S):
    """-> namespace: x [B, S, 512] tokens, res [B, S, 512] residual (multiples of 0.25), payload [B, S, 256], expected [B, S, 512] fp64 (the
    closed form, residual included), and what the mutations need (swap_at, segment).  Deterministic in (family, B, S)."""
    g = torch.Generator().manual_seed(FAMILIES.index(family) * 1000003 + B * 4099 + S)
    amp = AMPLITUDE[family]
    x = torch.zeros(B, S, C)
    payload = _payload(B, S, g, 1 if family == "allneg" else -14)
    x[:, :, 2 * NCODE:] = payload
    res = torch.randint(-16, 17, (B, S, C), generator=g).float() * 0.25
    attn = torch.zeros(B, S, C, dtype=torch.float64)
    c = SimpleNamespace(family=family, B=B, S=S, payload=payload, res=res, swap_at=None, segment=None)
    if family in ("select", "select_loose"):
        sel = torch.empty(B, S, dtype=torch.int64)
        for b in range(B):
            perm = torch.randperm(4096, generator=g)[:S]          # a different permutation per image
            sel[b] = _select_positions(S, g)
            x[b, :, NCODE:2 * NCODE] = code_vectors(perm, amp)
            x[b, :, :NCODE] = code_vectors(perm[sel[b]], amp)
            attn[b, :, :PAYLOAD] = payload[b, sel[b]].double()
        c.sel, c.swap_at = sel, 31                                # query 1 selects key 31: its value swapped with key 32's
    elif family == "avg4":
        c.groups = []
        for b in range(B):
            groups, left = _avg4_groups(S, g)
            n = groups.shape[0]
            codes = torch.randperm(4096, generator=g)[:n + len(left)]
            kc = torch.empty(S, dtype=torch.int64)
            kc[groups.reshape(-1)] = codes[:n].repeat_interleave(4)
            if left:
                kc[torch.tensor(left)] = codes[n:]                 # unique codes that no query selects
            pick = torch.randint(0, n, (S,), generator=g)
            pick[0], pick[S - 1] = 0, 0
            if S >= 1024:
                pick[1] = 1
                c.segment = 2                                     # the quarter whose row sum the mutation drops: it holds groups[1][2]
            x[b, :, NCODE:2 * NCODE] = code_vectors(kc, amp)
            x[b, :, :NCODE] = code_vectors(codes[pick], amp)
            attn[b, :, :PAYLOAD] = payload[b].double()[groups[pick]].mean(dim=1)
            c.groups.append(groups)
        c.swap_at = 0                                             # key 0 is in group 0, key 1 in another group (or in none)
    else:
        x[:, :, 0] = -2.0
        x[:, :, NCODE] = 4.0
        attn[:, :, :PAYLOAD] = payload.double().mean(dim=1, keepdim=True)
    c.x = x
    c.attn = attn
    c.expected = attn + res.double()
    return c


def operands(case, dtype=torch.float64):
    """q, k, v [B, S, 512] of the case through the construction's weight matrices"""
    w = attention_weights({A + n + s: torch.zeros(C, C) if s == ".weight" else torch.zeros(C) for n in ("to_q", "to_k", "to_v", "to_out.0")
                           for s in (".weight", ".bias")})
    x = case.x.to(dtype)
    return tuple(x @ w[A + n + ".weight"].to(dtype).t() for n in ("to_q", "to_k", "to_v"))


MUTATIONS = ("swap_pv", "drop_last", "tile0_twice_pv", "tile0_twice", "other_image", "drop_segment_sum", "pad_key")


def reference(case, mutation=None):
    """fp64 softmax attention of the case's operands + residual, [B, S, 512]; `mutation`: one typical kernel mistake applied to it --
       swap_pv           the values of two neighbouring keys (swap_at, swap_at + 1) exchanged while P keeps its order
       drop_last         the last key never scored
       tile0_twice_pv    the first 64-key tile accumulated twice in P.V (the row sums, taken in Q.K^T, count it once)
       tile0_twice       ... twice in P.V and in the row sums (a selection of ONE key cannot see this: its weight stays 1)
       other_image       keys and values of the next image of the batch
       drop_segment_sum  the row sum of one quarter of the key range (case.segment) left out of the denominator
       pad_key           one zero key (k = 0, v = 0) counted in every row"""
    q, k, v = operands(case)
    S = case.S
    if mutation == "other_image":
        k, v = k.roll(1, 0), v.roll(1, 0)
    if mutation == "pad_key":
        z = torch.zeros(case.B, 1, C, dtype=torch.float64)
        k, v = torch.cat([k, z], 1), torch.cat([v, z], 1)
    if mutation == "swap_pv":
        j = case.swap_at
        v = v.clone()
        v[:, [j, j + 1]] = v[:, [j + 1, j]]
    s = q @ k.transpose(1, 2) / math.sqrt(C)
    if mutation == "drop_last":
        s[:, :, S - 1] = -math.inf
    p = torch.exp(s - s.max(dim=-1, keepdim=True).values)
    num, den = p, p
    if mutation in ("tile0_twice_pv", "tile0_twice"):
        num = p.clone()
        num[:, :, :64] *= 2
        den = num if mutation == "tile0_twice" else p
    if mutation == "drop_segment_sum":
        den = p.clone()
        den[:, :, case.segment * S // 4:(case.segment + 1) * S // 4] = 0
    o = (num @ v) / den.sum(dim=-1, keepdim=True)
    return o + case.res.double()                                   # (to_out is the identity, its bias zero)


def mutations_of(case):
    """the mistakes the family is meant to catch at this shape"""
    if case.family == "allneg":
        return ("pad_key",)
    m = ["swap_pv", "drop_last", "tile0_twice_pv"]
    if case.family == "avg4":
        if case.S > 64:                      # (up to 64 keys the first tile is the whole row: counting it twice in both sums is no change)
            m.append("tile0_twice")
        if case.S >= 1024:
            m.append("drop_segment_sum")
    if case.B > 1:
        m.append("other_image")
    return tuple(m)


def tolerance(case):
    """the device bound: 2^-7 max|payload| (select, select_loose, avg4: exact in exact arithmetic; one bf16 rounding of P, one of o, a
    reciprocal and one fp32 add -- 4 x one bf16 half-ulp) or 2^-7 of the largest attention term (allneg: the mean is not bf16-exact).
    The rounding of P does not cancel against the row sum: attn_qk.hip and the generic GEMM's row_mode 2 both sum the fp32 numerators, P.V
    multiplies their bf16 roundings -- at most 2^-8 of the value when the numerator sits at the bottom of a binade -- and o rounds once more, half
    an ulp of its own binade: for |o| in [4, 8) that is |o| 2^-8 + 2^-6 <= 2^-7 max whenever max >= 4, and likewise below (every case here
    has max|payload| = 7 and a largest mean above 3.5).  Mode 2 rounds the normalised P, which does not cancel either: the same two terms."""
    if case.family == "allneg":
        return 2.0 ** -7 * case.attn.abs().max().item()
    return 2.0 ** -7 * case.payload.abs().max().item()


def shift_gap(case):
    """u - l per row [B, S] by attn_shift_kernel's formula: u = |q_i| max_j|k_j| alpha 1.0001, l = q_i . k_i alpha"""
    q, k, _ = operands(case)
    alpha = 1.0 / math.sqrt(C)
    u = q.norm(dim=-1) * k.norm(dim=-1).max(dim=-1, keepdim=True).values * alpha * 1.0001
    return u - (q * k).sum(-1) * alpha


def exactly_representable(t):
    """t and 8 t survive a round trip through bf16 and through float8_e4m3fn, and |8 t| <= 448"""
    for s in (1.0, 8.0):
        y = (t * s).float()
        if y.abs().max().item() > 448.0:
            return False
        for dt in (torch.bfloat16, torch.float8_e4m3fn):
            if not torch.equal(y.to(dt).float(), y):
                return False
    return True
