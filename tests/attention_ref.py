"""A plain attention reference with a stated contract, and the case tables of the attention edge tests.

Nothing here needs a GPU: ``tests/test_attention_cases_cpu.py`` checks the reference and the tables on any machine,
``tests/test_attention_edges_gpu.py`` runs the tables on the kernels of ``csrc/attention.hip``.

The contract (also in the header comment of ``cer_attention_fwd`` / ``cer_attention_bwd``, include/cer_hip.h):

  out = softmax(q k^T * scale + key mask) v,  lse = log sum_k exp(score) over the visible keys;
  a query with NO visible key (its batch row's mask is all zero) has out = 0, lse = +inf and dq = 0, and contributes
  nothing to dk or dv.  torch's softmax returns NaN for such a row; the kernel's ``l_run > 0 ? ... : INFINITY`` /
  ``inv = 0`` exit and the backward's ``exp(score - inf) = 0`` return the values above.

The gradients are written out as the kernel computes them (P from the saved statistics, Delta = rowsum(dO * O),
dS = P (dP - Delta) scale), so that the SAME function evaluated in float32 is an independent fp32 realisation of the
same formula: the yardstick of the extreme-score tests.
"""
import math
import re

import torch

# ---------------------------------------------------------------------------------------------- the reference


def attention_ref(q, k, v, mask=None, scale=None, dout=None, dtype=torch.float64):
    """q [B, Sq, H, d], k / v [B, Sk, H, d] (any strides), mask [B, Sk] (nonzero = attend) or None.
    Returns {"out" [B, Sq, H, d], "lse" [B, H, Sq]} and, with ``dout`` [B, Sq, H, d], also "dq", "dk", "dv"."""
    q, k, v = q.detach().to(dtype), k.detach().to(dtype), v.detach().to(dtype)
    d = q.shape[-1]
    scale = 1.0 / math.sqrt(d) if scale is None else scale
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * scale
    vis = torch.ones(s.shape, dtype=torch.bool)
    if mask is not None:
        vis = (mask != 0)[:, None, None, :].expand_as(s)
    s = s.masked_fill(~vis, float("-inf"))
    dead = ~vis.any(-1, keepdim=True)                       # rows with no visible key
    m = torch.where(dead, torch.zeros((), dtype=dtype), s.amax(-1, keepdim=True))
    e = torch.exp(s - m)                                    # masked entries: exp(-inf) = 0
    l = torch.where(dead, torch.ones((), dtype=dtype), e.sum(-1, keepdim=True))
    p = e / l                                               # dead rows: 0 / 1
    res = {"out": torch.einsum("bhqk,bkhd->bqhd", p, v),
           "lse": torch.where(dead, torch.full((), float("inf"), dtype=dtype), m + torch.log(l)).squeeze(-1)}
    if dout is not None:
        do = dout.detach().to(dtype)
        delta = (do * res["out"]).sum(-1).permute(0, 2, 1)[..., None]       # [B, H, Sq, 1]
        dp = torch.einsum("bqhd,bkhd->bhqk", do, v)
        ds = p * (dp - delta) * scale
        res["dv"] = torch.einsum("bhqk,bqhd->bkhd", p, do)
        res["dq"] = torch.einsum("bhqk,bkhd->bqhd", ds, k)
        res["dk"] = torch.einsum("bhqk,bqhd->bkhd", ds, q)
    return res


# ---------------------------------------------------------------------------------------------- launch variants
SPLIT_MAX_BLOCKS, SPLIT_MIN_STREAM, OWNER_ROWS_PER_BLOCK = 128, 128, 128


def use_split(owner_rows, streamed_rows, heads, batch):
    """attn_use_split (csrc/attention.hip) restated: the four waves of a block share 32 owner rows and split the streamed
    range when the plain grid would be short of blocks and there are enough streamed rows to split."""
    blocks = -(-owner_rows // OWNER_ROWS_PER_BLOCK) * heads * batch
    return blocks < SPLIT_MAX_BLOCKS and streamed_rows >= SPLIT_MIN_STREAM


def split_constants_in_source(text):
    """(block limit, streamed-row limit, owner rows per plain block) as attn_use_split's source text states them."""
    body = text[text.index("static bool attn_use_split"):]
    body = body[:body.index("\n}")]
    rows = re.search(r"\(owner_rows \+ (\d+)\) / (\d+)\) \* H \* B", body)
    lim = re.search(r"return blocks < (\d+) && streamed_rows >= (\d+);", body)
    assert rows and lim and int(rows.group(1)) + 1 == int(rows.group(2)), "attn_use_split no longer reads as restated"
    return int(lim.group(1)), int(lim.group(2)), int(rows.group(2))


def variants(b, h, sq, sk, d):
    """The kernels one forward + backward call reaches: {(pass, "split" | "plain", d)}.  Forward and dQ own queries and
    stream keys; dK/dV owns keys and streams queries."""
    qs = "split" if use_split(sq, sk, h, b) else "plain"
    ks = "split" if use_split(sk, sq, h, b) else "plain"
    return {("fwd", qs, d), ("dq", qs, d), ("dkv", ks, d)}


ALL_VARIANTS = {(p, s, d) for p in ("fwd", "dq", "dkv") for s in ("plain", "split") for d in (32, 64, 128)}

# ---------------------------------------------------------------------------------------------- structured masks
TILE = 32          # keys per tile
WAVES = 4          # split mode: tile t belongs to wave t % 4
TRAILING_LENGTHS = (1, 31, 32, 33, 64, None)      # None = Sk (no padding)


def tiles_all_masked(mask_row, sk):
    """[ceil(Sk / 32)] bool: tile t has no visible key."""
    n = -(-sk // TILE)
    return [not bool(mask_row[t * TILE:min((t + 1) * TILE, sk)].any()) for t in range(n)]


def mask_trailing(b, sk):
    """BERT key padding: batch row i attends its first TRAILING_LENGTHS[i % 6] keys."""
    m = torch.zeros(b, sk, dtype=torch.int32)
    for i in range(b):
        n = TRAILING_LENGTHS[i % len(TRAILING_LENGTHS)]
        m[i, :sk if n is None else min(n, sk)] = 1
    return m


def mask_leading(b, sk, n):
    """The first ``n`` keys masked: whole leading tiles see nothing (the forward's m_new == -inf branches)."""
    m = torch.ones(b, sk, dtype=torch.int32)
    m[:, :n] = 0
    return m


def mask_wave(b, sk, w):
    """Split mode: every key of the tiles t % 4 == w masked, so wave w ends with m = -inf, l = 0 (the merge's mw == -inf)."""
    m = torch.ones(b, sk, dtype=torch.int32)
    for t in range(-(-sk // TILE)):
        if t % WAVES == w:
            m[:, t * TILE:(t + 1) * TILE] = 0
    return m


def mask_random(b, sk, seed, keep=0.7):
    m = (torch.rand(b, sk, generator=torch.Generator().manual_seed(seed)) < keep).to(torch.int32)
    m[:, 0] = 1
    return m


def mask_dead_row(b, sk, row, seed):
    """Batch row ``row`` fully masked, its neighbours randomly masked."""
    m = mask_random(b, sk, seed)
    m[row] = 0
    return m


# ---------------------------------------------------------------------------------------------- case tables
# Geometries (b, h, sq, sk) of the structured-mask cases:
#   plain: Sk = 96 < 128 streamed keys, Sq = 70 < 128 streamed queries -> forward, dQ and dK/dV all plain
#   split: 6 / 12 owner blocks < 128, Sk = 200 >= 128 and Sq = 130 >= 128      -> all split; 200 keys = 7 tiles (6.25)
GEO = {"plain": (6, 1, 70, 96), "split": (6, 1, 130, 200)}
DS = (32, 64, 128)


def _mask_cases():
    out = []
    for d in DS:
        for var, (b, h, sq, sk) in GEO.items():
            out.append((f"trailing-{var}-d{d}", b, h, sq, sk, d, ("trailing",)))
            out.append((f"lead32-{var}-d{d}", b, h, sq, sk, d, ("leading", 32)))
            out.append((f"lead64-{var}-d{d}", b, h, sq, sk, d, ("leading", 64)))
            out.append((f"deadrow-{var}-d{d}", b, h, sq, sk, d, ("dead_row", 2)))
        b, h, sq, sk = GEO["split"]
        for w in range(WAVES):
            out.append((f"wave{w}-split-d{d}", b, h, sq, sk, d, ("wave", w)))
    return out


MASK_CASES = _mask_cases()


def build_mask(spec, b, sk, seed=0):
    if spec is None:
        return None
    kind = spec[0]
    if kind == "trailing":
        return mask_trailing(b, sk)
    if kind == "leading":
        return mask_leading(b, sk, spec[1])
    if kind == "wave":
        return mask_wave(b, sk, spec[1])
    if kind == "dead_row":
        return mask_dead_row(b, sk, spec[1], seed)
    if kind == "random":
        return mask_random(b, sk, seed)
    raise ValueError(spec)


# Shape edges: (name, b, h, sq, sk, d, mask spec).  The two asymmetric geometries run at every d, masked and unmasked:
# together they reach every kernel instantiation both ways (checked in test_attention_cases_cpu.py).
def _shape_cases():
    out = []
    for d in DS:
        for mk, spec in (("nomask", None), ("masked", ("random",))):
            out.append((f"qsplit-kplain-d{d}-{mk}", 1, 1, 37, 160, d, spec))     # forward / dQ split, dK/dV plain
            out.append((f"qplain-ksplit-d{d}-{mk}", 1, 1, 160, 37, d, spec))     # forward / dQ plain, dK/dV split
    out += [
        ("sq1", 2, 2, 1, 40, 64, ("random",)),
        ("sq1-split", 1, 1, 1, 130, 128, None),
        ("sk1", 2, 2, 40, 1, 32, None),
        ("sk1-ksplit", 1, 1, 130, 1, 64, None),
        ("sk33", 1, 3, 50, 33, 128, ("random",)),
        ("sq129", 1, 2, 129, 70, 64, ("random",)),                 # one past a multiple of 128 (plain: a second block)
        ("sq129-split", 1, 2, 129, 140, 32, None),
        ("sq33", 2, 1, 33, 160, 32, ("random",)),                  # one past a multiple of 32 (split: a second block)
        ("sq33-plain", 2, 1, 33, 60, 128, None),
        ("sk128", 1, 1, 40, 128, 64, ("random",)),                 # the split threshold exactly ...
        ("sk127", 1, 1, 40, 127, 64, ("random",)),                 # ... and one below it
        ("sk128-d128", 2, 1, 40, 128, 128, None),
        ("sk127-d32", 2, 1, 40, 127, 32, None),
        ("both-split", 2, 2, 130, 200, 64, ("random",)),
        ("both-plain", 2, 3, 40, 40, 64, None),
        ("plain-long-stream", 4, 32, 16, 256, 32, ("random",)),    # 128 blocks: plain although Sk >= 128
        ("split-1024", 1, 1, 64, 1024, 64, ("trailing",)),
        ("split-517", 1, 1, 300, 517, 128, ("random",)),
    ]
    return out


SHAPE_CASES = _shape_cases()

# Extreme scores: (name, b, h, sq, sk, d, kind, scale or None = 1/sqrt(d), mask spec)
#   "big"    Q and K times 5, so |score| reaches about 100 at scale 1/sqrt(d): exp() without the max shift overflows fp32
#   "scale"  standard-normal Q, K with a scale that is not 1/sqrt(d)
#   "offset" one key's scores carry a common offset of +60: its probability is 1 in fp32, the others ~ e^-60


def _extreme_cases():
    out = []
    for d in DS:
        for var, (b, h, sq, sk) in (("plain", (2, 2, 70, 96)), ("split", (2, 1, 130, 200))):
            out.append((f"big-{var}-d{d}", b, h, sq, sk, d, "big", None, ("random",)))
            out.append((f"offset-{var}-d{d}", b, h, sq, sk, d, "offset", None, None))
            out.append((f"scale-{var}-d{d}", b, h, sq, sk, d, "scale", 1.0 if d == 32 else 0.37, ("random",)))
    out.append(("big-split-1024", 1, 1, 64, 1024, 64, "big", None, None))
    out.append(("big-lead64-split", 2, 1, 130, 200, 64, "big", None, ("leading", 64)))
    return out


EXTREME_CASES = _extreme_cases()


def make_inputs(name, b, h, sq, sk, d, kind="randn"):
    """Deterministic fp32 q, k, v, dout [B, S, H, d] of one case (seeded by its name)."""
    g = torch.Generator().manual_seed(sum(ord(c) * (i + 1) for i, c in enumerate(name)) % (2 ** 31))
    q = torch.randn(b, sq, h, d, generator=g)
    k = torch.randn(b, sk, h, d, generator=g)
    v = torch.randn(b, sk, h, d, generator=g)
    dout = torch.randn(b, sq, h, d, generator=g)
    if kind == "big":
        q, k = q * 5.0, k * 5.0
    elif kind == "offset":
        # channel 0 carries the offset alone: q[..., 0] = 8, k[..., 0] = 0 except the chosen key, whose product with
        # 8 * scale is 60
        key = sk // 2 + 3
        q[..., 0] = 8.0
        k[..., 0] = 0.0
        k[:, key, :, 0] = 60.0 * math.sqrt(d) / 8.0
    elif kind not in ("randn", "scale"):
        raise ValueError(kind)
    return q, k, v, dout


def all_cases():
    """Every (name, b, h, sq, sk, d, kind, scale, mask spec) of the GPU tables, in one list."""
    out = [(n, b, h, sq, sk, d, "randn", None, spec) for n, b, h, sq, sk, d, spec in MASK_CASES + SHAPE_CASES]
    return out + list(EXTREME_CASES)


def case_seed(name):
    return sum(ord(c) for c in name)
