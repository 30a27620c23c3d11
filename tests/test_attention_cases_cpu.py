"""The float64 attention reference and the case tables of test_attention_edges_gpu.py, checked without a GPU:
the reference against torch's own softmax / autograd, its degenerate-row contract, the restated launch chooser against
the kernel's source text, the kernels the tables reach, and what each structured mask is meant to mask."""
import math
import os

import pytest
import torch

import attention_ref as ar

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "feature_vs_text_compound_emotion_amd", "csrc",
                   "attention.hip")


@pytest.mark.parametrize("b,h,sq,sk,d,scale,masked", [(2, 3, 40, 70, 32, None, True), (1, 2, 33, 130, 64, 0.37, False),
                                                      (3, 1, 7, 5, 128, 1.0, True)])
def test_reference_matches_torch_softmax_and_autograd_in_float64(b, h, sq, sk, d, scale, masked):
    g = torch.Generator().manual_seed(sq * 10 + sk)
    q, k, v = (torch.randn(b, s, h, d, generator=g, dtype=torch.float64, requires_grad=True) for s in (sq, sk, sk))
    dout = torch.randn(b, sq, h, d, generator=g, dtype=torch.float64)
    mask = ar.mask_random(b, sk, seed=3) if masked else None
    sc = 1.0 / math.sqrt(d) if scale is None else scale
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * sc
    if masked:
        s = s + torch.zeros(b, 1, 1, sk, dtype=torch.float64).masked_fill(mask[:, None, None, :] == 0, float("-inf"))
    want = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v)
    want.backward(dout)
    # strided inputs: the helper takes whatever view it is given
    wide = torch.zeros(b, sq, h, 2 * d, dtype=torch.float64)
    wide[..., d:] = q.detach()
    got = ar.attention_ref(wide[..., d:], k, v, mask, scale, dout)
    assert (got["out"] - want.detach()).abs().max().item() < 1e-13
    assert (got["lse"] - torch.logsumexp(s.detach(), -1)).abs().max().item() < 1e-13
    for name, t in (("dq", q), ("dk", k), ("dv", v)):
        assert (got[name] - t.grad).abs().max().item() < 1e-12, name


def test_reference_contract_on_rows_without_a_visible_key():
    b, h, sq, sk, d = 3, 2, 9, 40, 32
    q, k, v, dout = ar.make_inputs("contract", b, h, sq, sk, d)
    mask = ar.mask_dead_row(b, sk, 1, seed=5)
    r = ar.attention_ref(q, k, v, mask, None, dout)
    assert all(torch.isfinite(r[n]).all() for n in ("out", "dq", "dk", "dv"))
    assert (r["out"][1] == 0).all() and (r["dq"][1] == 0).all() and (r["dk"][1] == 0).all() and (r["dv"][1] == 0).all()
    assert (r["lse"][1] == float("inf")).all() and torch.isfinite(r["lse"][[0, 2]]).all()
    # the neighbours are what they are without the dead row
    keep = [0, 2]
    alone = ar.attention_ref(q[keep], k[keep], v[keep], mask[keep], None, dout[keep])
    for n in ("out", "dq", "dk", "dv", "lse"):
        assert torch.equal(r[n][keep], alone[n]), n
    # masked keys of a live row get no gradient
    assert (r["dk"][0][mask[0] == 0] == 0).all() and (r["dv"][0][mask[0] == 0] == 0).all()


def test_reference_is_finite_on_every_case_of_the_gpu_tables():
    cases = ar.all_cases()
    assert len({c[0] for c in cases}) == len(cases), "case names must be unique (they seed the inputs)"
    for name, b, h, sq, sk, d, kind, scale, spec in cases:
        q, k, v, dout = ar.make_inputs(name, b, h, sq, sk, d, kind)
        mask = ar.build_mask(spec, b, sk, ar.case_seed(name))
        r = ar.attention_ref(q, k, v, mask, scale, dout)
        for n in ("out", "dq", "dk", "dv"):
            assert torch.isfinite(r[n]).all(), (name, n)
        dead = torch.zeros(b, dtype=torch.bool) if mask is None else ~(mask != 0).any(-1)
        assert torch.isfinite(r["lse"][~dead]).all() and (r["lse"][dead] == float("inf")).all(), name
        for t in (q, k, v):     # the kernel reads float4s: the tables only hold fp32 inputs
            assert t.dtype == torch.float32


def test_extreme_cases_are_extreme():
    """|score| reaches about 100 in the "big" cases (an unshifted expf overflows at 88.7), one probability is 1 to fp32
    in the "offset" cases, and no "scale" case uses 1 / sqrt(d)."""
    kinds = set()
    for name, b, h, sq, sk, d, kind, scale, spec in ar.EXTREME_CASES:
        q, k, v, _ = ar.make_inputs(name, b, h, sq, sk, d, kind)
        sc = 1.0 / math.sqrt(d) if scale is None else scale
        s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) * sc
        kinds.add((kind, d))
        if kind == "big":
            assert 90.0 < s.abs().max().item() < 200.0, (name, s.abs().max().item())
        elif kind == "offset":
            p = torch.softmax(s, -1).amax(-1)
            assert (1.0 - p).max().item() < 2.0 ** -30, name
        else:
            assert abs(sc - 1.0 / math.sqrt(d)) > 0.05, name
    assert kinds == {(kd, d) for kd in ("big", "offset", "scale") for d in ar.DS}
    assert any(c[6] == "scale" and c[5] == 32 and c[7] == 1.0 for c in ar.EXTREME_CASES)


def test_split_chooser_restated_matches_the_source_text():
    with open(SRC) as fh:
        text = fh.read()
    assert ar.split_constants_in_source(text) == (ar.SPLIT_MAX_BLOCKS, ar.SPLIT_MIN_STREAM, ar.OWNER_ROWS_PER_BLOCK)
    # the forward and dQ choose by (Sq, Sk), dK/dV by (Sk, Sq)
    assert "attn_use_split(Sq, Sk, H, B)" in text
    assert "attn_use_split(a.Sq, a.Sk, a.H, a.B) ? launch_attn_bwd_one<D, false, true>" in text
    assert "attn_use_split(a.Sk, a.Sq, a.H, a.B) ? launch_attn_bwd_one<D, true, true>" in text
    assert ar.use_split(40, 128, 1, 1) and not ar.use_split(40, 127, 1, 1)
    assert ar.use_split(127 * 128, 128, 1, 1) and not ar.use_split(127 * 128 + 1, 128, 1, 1)
    assert not ar.use_split(16, 256, 32, 4)                      # 128 blocks already
    assert ar.use_split(1024, 1024, 1, 6)                        # the JMT / MT final stage the variants were built for


def test_tables_reach_every_kernel_masked_and_unmasked():
    """{forward, dQ, dK/dV} x {plain, split} x d in {32, 64, 128}: eighteen instantiations (six of attention_fwd_kernel,
    twelve of attention_bwd_kernel), each reached with and without a key mask."""
    reached = {True: set(), False: set()}
    for name, b, h, sq, sk, d, kind, scale, spec in ar.all_cases():
        reached[spec is not None] |= ar.variants(b, h, sq, sk, d)
    assert len(ar.ALL_VARIANTS) == 3 * 2 * 3
    assert reached[True] == ar.ALL_VARIANTS, sorted(ar.ALL_VARIANTS - reached[True])
    assert reached[False] == ar.ALL_VARIANTS, sorted(ar.ALL_VARIANTS - reached[False])
    # the structured masks alone run plain and split at every d, and the names say which
    for name, b, h, sq, sk, d, spec in ar.MASK_CASES:
        want = "split" if "-split-" in name else "plain"
        assert ar.variants(b, h, sq, sk, d) == {("fwd", want, d), ("dq", want, d), ("dkv", want, d)}, name
    for name, b, h, sq, sk, d, kind, scale, spec in ar.EXTREME_CASES:
        if "-split" in name:
            assert ("fwd", "split", d) in ar.variants(b, h, sq, sk, d), name
        else:
            assert ar.variants(b, h, sq, sk, d) == {("fwd", "plain", d), ("dq", "plain", d), ("dkv", "plain", d)}, name
    by_name = {c[0]: c for c in ar.SHAPE_CASES}
    for d in ar.DS:
        assert ar.variants(*by_name[f"qsplit-kplain-d{d}-nomask"][1:6]) == {("fwd", "split", d), ("dq", "split", d),
                                                                          ("dkv", "plain", d)}
        assert ar.variants(*by_name[f"qplain-ksplit-d{d}-nomask"][1:6]) == {("fwd", "plain", d), ("dq", "plain", d),
                                                                          ("dkv", "split", d)}


def test_structured_masks_mask_what_they_are_meant_to():
    for name, b, h, sq, sk, d, spec in ar.MASK_CASES:
        mask = ar.build_mask(spec, b, sk, ar.case_seed(name))
        assert tuple(mask.shape) == (b, sk) and mask.dtype == torch.int32
        split = "-split-" in name
        n_tiles = -(-sk // ar.TILE)
        assert not split or n_tiles > ar.WAVES, "every wave needs a tile of its own"
        for row in range(b):
            dead = ar.tiles_all_masked(mask[row], sk)
            if spec[0] == "trailing":
                n = ar.TRAILING_LENGTHS[row % 6]
                n = sk if n is None else n
                assert int(mask[row].sum()) == n and bool(mask[row, :n].all())
                # the last k tiles are all masked, the ones before them are not
                k_dead = n_tiles - (-(-n // ar.TILE))
                assert dead == [False] * (n_tiles - k_dead) + [True] * k_dead, (name, row)
                if split and n <= 64:      # waves 2 and 3 see nothing at all
                    assert all(dead[t] for t in range(n_tiles) if t % ar.WAVES >= 2)
            elif spec[0] == "leading":
                k_dead = spec[1] // ar.TILE
                assert dead == [True] * k_dead + [False] * (n_tiles - k_dead), (name, row)
            elif spec[0] == "wave":
                assert split
                assert [dead[t] for t in range(n_tiles)] == [t % ar.WAVES == spec[1] for t in range(n_tiles)], (name, row)
                assert any(t % ar.WAVES == spec[1] for t in range(n_tiles))
            elif spec[0] == "dead_row":
                assert all(dead) == (row == spec[1]), (name, row)
                if row != spec[1]:
                    assert bool(mask[row].any()) and not bool(mask[row].all())
    assert {row % 6 for row in range(ar.GEO["plain"][0])} == set(range(6)), "every trailing length needs a batch row"
    assert ar.TRAILING_LENGTHS == (1, 31, 32, 33, 64, None)
    names = {c[0] for c in ar.MASK_CASES}
    for d in ar.DS:
        assert {f"wave{w}-split-d{d}" for w in range(4)} <= names
        for var in ("plain", "split"):
            assert {f"{m}-{var}-d{d}" for m in ("trailing", "lead32", "lead64", "deadrow")} <= names
