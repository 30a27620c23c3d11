"""The float64 conv reference and the case tables of the fp32 implicit-GEMM edge tests, checked without a GPU.

* ``conv_ref`` (F.pad + F.conv2d) against ``conv_loops``, the gather written out tap by tap;
* every exact case meets its precondition (``exact_margin`` < 2^24, which includes A < 2^24; the statistics condition where
  statistics are taken; the data-gradient cases on the gradient's own products), so a bit-for-bit comparison is owed;
* torch's own fp32 CPU conv -- a correct fp32 contraction that is not the code under test -- reproduces every exact reference
  bit for bit and stays inside every rounding bound.
"""
import functools
import itertools

import pytest
import torch

import conv_ref as cr

LIMIT = 2.0 ** 24


def _ids(table):
    return [c.name for c in table]


TINY = [
    # asymmetric pad, stride 2, affine, PReLU, mask
    cr.C("tiny_asym_pad", 2, 4, 5, 3, 4, 3, 2, stride=2, pad=(2, 0), affine=True, bias=True, act1="prelu", mask=True),
    # dilation whose taps pass the bottom edge (pad_t = 1 taken as symmetric by the output size, nothing padded below)
    cr.C("tiny_dil_bottom", 1, 5, 3, 2, 3, 3, 1, dil=(2, 1), pad=(1, 0), bias=True, act1="leaky", act2="leaky"),
    # strided residual from an odd-sized tensor, aux
    cr.C("tiny_res_stride2", 2, 3, 4, 2, 5, 1, 3, pad=(0, 1), res="stride2", aux=True, act1="relu", act2="leaky"),
    # a forced output grid on a causal geometry
    cr.causal_case("tiny_causal", 2, 3, 2, 3, 3, 2, bias=True, res="same", act1="gelu"),
]


@pytest.mark.parametrize("case", TINY, ids=_ids(TINY))
@pytest.mark.parametrize("exact", [True, False])
def test_conv_ref_equals_the_gather_loop(case, exact):
    if exact and case.act1 == "gelu":
        exact = False
    d = cr.make(case, exact=exact)
    got = cr.reference(case, d)
    want = cr.conv_loops(d["x"], d["w"], **cr.ref_kwargs(case, d))
    for g, w, name in zip(got, want, ("y", "aux", "raw")):
        assert g.dtype == torch.float64 and g.shape == w.shape, name
        if exact:
            assert torch.equal(g, w), name
        else:
            assert (g - w).abs().max().item() <= 1e-13 * (1.0 + w.abs().max().item()), name


def test_padding_contributes_zero_not_the_shift():
    x = torch.zeros(1, 2, 2, 1)
    w = torch.ones(1, 1, 3, 3)
    _, _, raw = cr.conv_ref(x, w, pad_t=1, pad_l=1, in_scale=torch.ones(1), in_shift=torch.ones(1))
    assert torch.equal(raw, torch.full((1, 2, 2, 1), 4.0, dtype=torch.float64))    # 4 in-bounds taps of 9, each = the shift
    assert torch.equal(cr.conv_mag(x, w, pad_t=1, pad_l=1, in_scale=torch.ones(1), in_shift=torch.ones(1)), raw)


def test_names_are_unique_and_the_epilogue_rows_cover_every_pair():
    names = [c.name for c in cr.EXACT + cr.ROUNDING]
    assert len(names) == len(set(names))
    assert 20 <= len(cr.EPILOGUE) <= 30
    rows = cr.EPILOGUE[:cr.N_PAIRWISE]
    values = {f: sorted({getattr(c, f) for c in cr.EPILOGUE}, key=str) for f in cr.EPI_FACTORS}
    assert values["act1"] == ["leaky", "none", "prelu", "relu"] and values["res"] == ["none", "same", "stride2"]
    assert values["y_extra"] == [0, 3, 4] and values["cout"] == [37, 64] and values["split_k"] == [1, 3]
    for f, h in itertools.combinations(cr.EPI_FACTORS, 2):
        seen = {(getattr(c, f), getattr(c, h)) for c in rows}
        assert seen == set(itertools.product(values[f], values[h])), (f, h)
    tcn = cr.EPILOGUE[0]
    assert (tcn.bias, tcn.act1, tcn.mask, tcn.res, tcn.act2, tcn.aux) == (True, "leaky", True, "same", "leaky", True)


@pytest.mark.parametrize("case", cr.EXACT, ids=_ids(cr.EXACT))
def test_exact_case_meets_its_precondition_and_torch_fp32_is_bit_exact(case):
    d = cr.make(case)
    for t in (d["x"], d["w"], d["bias"], d["residual"], d["in_shift"]):
        assert t is None or torch.equal(t, t.round())
    margin, a = cr.exact_margin(case, d)
    assert a < LIMIT and margin < LIMIT, (a, margin)
    y, aux, raw = cr.reference(case, d)
    if case.stats:
        assert cr.stats_margin(raw) < LIMIT
        assert raw.abs().sum((0, 1, 2)).max().item() < LIMIT          # the column sums themselves
    # torch's fp32 CPU conv: the same function in float32
    y32, aux32, raw32 = cr.reference(case, d, dtype=torch.float32)
    assert y32.dtype == torch.float32
    assert torch.equal(y32.double(), y) and torch.equal(aux32.double(), aux) and torch.equal(raw32.double(), raw)
    assert y.abs().max().item() > 0


@pytest.mark.parametrize("case", cr.CAUSAL, ids=_ids(cr.CAUSAL))
def test_data_gradient_case_meets_its_precondition(case):
    d = cr.make(case)
    ho, wo = cr.out_hw_of(case)
    dz = cr.dgrad_draw(case)
    assert tuple(dz.shape) == (case.n, ho, wo, case.cout)
    dx, mag = cr.dgrad_reference(case, d, dz)
    res = cr.dgrad_residual(case)
    assert (mag + (res.double().abs() if res is not None else 0.0)).max().item() < LIMIT
    assert torch.equal(dx, dx.round())
    # the anti-causal form: dX[t] = sum_j W[:, :, j]^T dZ[t + (k - 1 - j) dil], zero past the end of the sequence
    w = d["w"].double()[:, :, :, 0]
    want = torch.zeros_like(dx)
    for t in range(case.h):
        for j in range(case.kh):
            s = t + (case.kh - 1 - j) * case.dil[0]
            if s < case.h:
                want[:, t, 0] += dz.double()[:, s, 0] @ w[:, :, j]
    assert torch.equal(dx, want)


@pytest.mark.parametrize("case", cr.ROUNDING, ids=_ids(cr.ROUNDING))
def test_torch_fp32_meets_the_rounding_bound(case):
    d = cr.make(case, exact=False)
    y, _, raw = cr.reference(case, d)
    y32, _, _ = cr.reference(case, d, dtype=torch.float32)
    erf_err = None
    if case.act1 == "gelu":
        erf_err = cr.erf_error(raw + d["bias"].double())
    bound = cr.rounding_bound(case, d, erf_err)
    assert bound.shape == y.shape and bound.min().item() > 0
    ratio = ((y32.double() - y).abs() / bound).max().item()
    print(f"{case.name}: torch fp32 worst error / bound = {ratio:.3f}" + (f", erf error {erf_err:.3e}" if erf_err is not None else ""))
    assert ratio < 1.0


# ====================================================================================================================
# The backward convs (tests/test_conv_backward_edges_gpu.py): the weight-gradient reference against a gather written out product
# by product, the precondition of every exact case, torch's fp32 CPU GEMM as a correct contraction that is not the code under
# test, and the SENSITIVITY of the comparison: contractions with one deliberate mistake each, of the kind a kernel could make,
# are rejected by the assertion helper the GPU tests use.
W2D = [w.case for w in cr.WGRAD_2D]
W1D = [w.case for w in cr.WGRAD_1D]

TINY_W = [
    cr.C("tinyw_3x2_s2_pad2x0", 2, 4, 5, 3, 4, 3, 2, stride=2, pad=(2, 0)),
    cr.C("tinyw_1x3_pad0x2", 2, 3, 4, 2, 5, 1, 3, pad=(0, 2)),
    cr.C("tinyw_3x1_s2_pad1x0", 2, 5, 4, 2, 3, 3, 1, stride=2, pad=(1, 0)),
    cr.causal_case("tinyw_causal_d2", 2, 5, 2, 3, 3, 2),
    cr.causal_case("tinyw_causal_d4_past_L", 2, 3, 2, 3, 3, 4),
]


@functools.lru_cache(maxsize=None)
def _wdata(case, cls):
    return cr.wgrad_make(case, cls)


@functools.lru_cache(maxsize=None)
def _wref(case, cls):
    return cr.wgrad_reference(case, *_wdata(case, cls))


@pytest.mark.parametrize("cls", cr.OPERAND_CLASSES)
@pytest.mark.parametrize("case", TINY_W, ids=_ids(TINY_W))
def test_wgrad_reference_equals_the_gather_loop(case, cls):
    d, dz = cr.wgrad_make(case, cls)
    dw, mag = cr.wgrad_reference(case, d, dz)
    assert dw.dtype == torch.float64 and tuple(dw.shape) == (case.cout, case.cin, case.kh, case.kw)
    assert torch.equal(dw, cr.wgrad_loops(case, d, dz))
    assert torch.equal(mag, cr.wgrad_loops(case, {"x": d["x"].abs()}, dz.abs()))
    assert torch.equal(cr.wgrad_rows(case, d, dz, dtype=torch.float64), dw)
    assert dw.abs().max().item() > 0


def _is_class(cls, z, x):
    """The structure the exactness argument rests on: multiples of 2^-8, and one operand of every product without a lo plane."""
    for t in (z, x):
        assert torch.equal(t * 256, (t * 256).round()) and t.abs().max().item() <= 8.0
    if cls == "ints":
        assert torch.equal(z, z.round()) and torch.equal(x, x.round())
    z_lo, x_lo = z - cr.bf16_hi(z), x - cr.bf16_hi(x)
    assert torch.equal(cr.bf16_hi(z_lo), z_lo) and torch.equal(cr.bf16_hi(x_lo), x_lo)        # hi + lo is the value
    assert not (z_lo != 0).any() or not (x_lo != 0).any()
    if cls != "ints":
        frac = ((x_lo if cls == "x_lo" else z_lo) != 0).float().mean().item()
        assert 0.5 < frac < 0.8, frac                                                          # the lo plane is exercised


def _three_products(case, d, dz):
    """float32 emulation of the bf16x3 kernels: hi hi + hi lo + lo hi, each a float32 GEMM, the lo lo product dropped."""
    zh, xh = cr.bf16_hi(dz), cr.bf16_hi(d["x"])
    zl, xl = dz - zh, d["x"] - xh
    return cr.wgrad_rows(case, {"x": xh}, zl) + cr.wgrad_rows(case, {"x": xl}, zh) + cr.wgrad_rows(case, {"x": xh}, zh)


@pytest.mark.parametrize("cls", cr.OPERAND_CLASSES)
@pytest.mark.parametrize("case", W2D + W1D, ids=_ids(W2D + W1D))
def test_wgrad_case_meets_its_precondition_and_torch_fp32_is_bit_exact(case, cls):
    d, dz = _wdata(case, cls)
    ho, wo = cr.out_hw_of(case)
    assert tuple(dz.shape) == (case.n, ho, wo, case.cout) and tuple(d["x"].shape) == (case.n, case.h, case.w, case.cin)
    assert case.n * ho * wo <= 2000 and max(case.cin, case.cout) <= 512
    _is_class(cls, dz, d["x"])
    assert cr.wgrad_exact_margin(case, d, dz) < cr.WGRAD_LIMIT
    dw, _ = _wref(case, cls)
    got = cr.wgrad_rows(case, d, dz)
    assert got.dtype == torch.float32
    cr.assert_exact(got, dw, case.name)
    cr.assert_exact(_three_products(case, d, dz), dw, case.name + " (three products)")
    assert dw.abs().max().item() > 0
    if case.w == 1 and case.kw == 1:                  # causal: a tap whose shift reaches the sequence length sees no data at all
        for j in range(case.kh):
            if (case.kh - 1 - j) * case.dil[0] >= case.h:
                assert not dw[:, :, j].any()


def test_the_backward_tables_contain_what_they_are_for():
    names = [c.name for c in W2D + W1D + cr.DGRAD_2D + [w.case for w in cr.WGRAD_ROUNDING] + [cr.WGRAD_ROUNDING_1D.case]]
    assert len(names) == len(set(names))
    geo = {(c.kh, c.kw, c.stride, c.pad) for c in W2D}
    assert {(3, 2), (1, 3), (3, 1), (1, 1), (3, 3)} <= {(kh, kw) for kh, kw, _, _ in geo}
    assert any(p == (0, 2) and kw == 3 for _, kw, _, p in geo) and any(p == (2, 0) and kh == 3 for kh, _, _, p in geo)
    assert any(c.stride == 2 and (c.h + c.w) % 2 == 1 for c in W2D) and any(c.stride == 2 and c.kh == c.kw == 1 for c in W2D)
    outs = [cr.out_hw_of(c) for c in W2D]
    assert any(ho * wo < 32 and c.n >= 50 for c, (ho, wo) in zip(W2D, outs))
    assert any(wo > 64 and ho == 2 for ho, wo in outs) and any(wo == 1 for _, wo in outs)
    assert any(cr.wgrad_rows_of(c) % 32 for c in W2D)
    chans = {(c.cin, c.cout) for c in W2D}
    assert {(4, 64), (200, 40), (72, 132), (72, 200), (128, 256), (256, 512)} <= chans
    assert any(ci == 3 for ci, _ in chans) and any(co == 7 for _, co in chans)
    b3 = [w for w in cr.WGRAD_2D if w.split_b3 is not None]
    assert all((w.split_b3 is None) == bool(w.case.cin % 4 or w.case.cout % 4) for w in cr.WGRAD_2D)
    assert sum(w.split_b3 for w in b3) >= 3 and sum(w.split_f32 for w in cr.WGRAD_2D) >= 2
    for path in ("t64", "t128_", "t128dma", "wide"):       # every kernel has a split and a single-pass case
        mine = [w for w in b3 if path in w.case.name + "_"]
        assert any(w.split_b3 for w in mine) and not all(w.split_b3 for w in mine), path
    assert not all(w.split_f32 for w in cr.WGRAD_2D) and not all(w.split_f32 for w in cr.WGRAD_1D)
    one = cr.WGRAD_1D
    assert {w.case.dil[0] for w in one if w.case.kh == 5} == {1, 2, 4, 8} and any(w.case.kh == 1 for w in one)
    assert {7, 36, 64, 96, 200} <= {w.case.cin for w in one} | {w.case.cout for w in one}
    wides = [s for w in one for s in (w.x_wide, w.dz_wide) if s is not None]
    assert {4, 64} <= {off for pitch, off in wides if pitch % 4 == 0}
    assert any(pitch % 4 for pitch, _ in wides) and any(pitch % 4 == 0 and off == 1 for pitch, off in wides)


# ---------------------------------------------------------------------------------------------- sensitivity
def _rejected(case, cls, mutant):
    d, dz = _wdata(case, cls)
    try:
        cr.assert_exact(cr.wgrad_rows(case, d, dz, mutant=mutant), _wref(case, cls)[0], f"{case.name} [{mutant}]")
    except AssertionError:
        return True
    return False


# mutant -> (operand class, the table cases that have to catch it)
_CATCHERS = {
    "hw_swap": ("ints", ["rect10x25_3x3_4to64_t64stem", "row2x70_3x3_128to256_t128dma_full", "tiny3x5_n50_s2_3x3_72to132_t128"]),
    "pad_swap": ("ints", ["rect10x25_3x2_pad1x0_72to132_t128", "rect7x12_1x3_pad0x2_72to200_t128dma_partial",
                          "rect6x11_3x3_pad2x0_128to256_t128dma_full"]),
    "tap_div_kh": ("ints", ["rect10x25_3x2_pad1x0_72to132_t128", "rect7x12_1x3_pad0x2_72to200_t128dma_partial",
                            "s2_9x8_3x1_pad1x0_128to256_t128dma_full"]),
    "drop_last_step": ("ints", ["rect10x25_3x3_4to64_t64stem", "rect7x12_1x3_pad0x2_72to200_t128dma_partial",
                                "w1_k5_d1_36to64"]),
    "drop_lo": ("x_lo", ["rect10x25_3x2_pad1x0_72to132_t128", "s2_7x10_1x1_256to512_wide", "tiny3x5_n50_s2_3x3_4to64_t64stem"]),
    "tile_neighbour": ("ints", ["rect7x12_1x3_pad0x2_72to200_t128dma_partial", "rect10x25_3x2_pad1x0_72to132_t128",
                                "s2_7x10_1x1_256to512_wide"]),
}


@pytest.mark.parametrize("mutant", cr.WGRAD_MUTANTS)
def test_a_wrong_contraction_is_rejected_by_the_comparison_the_gpu_tests_use(mutant):
    cls, names = _CATCHERS[mutant]
    table = cr.by_name(W2D + W1D)
    for name in names:
        assert _rejected(table[name], cls, mutant), f"{mutant} passes on {name}"
        assert not _rejected(table[name], cls, None)
    caught = [c.name for c in W2D if _rejected(c, cls, mutant)]
    print(f"{mutant}: rejected on {len(caught)} of {len(W2D)} WGRAD_2D cases")


def test_the_lo_plane_of_dz_is_needed_in_the_mirror_class():
    case = cr.by_name(W2D)["rect10x25_3x2_pad1x0_72to132_t128"]
    d, dz = _wdata(case, "z_lo")
    with pytest.raises(AssertionError, match="values differ"):
        cr.assert_exact(cr.wgrad_rows(case, d, cr.bf16_hi(dz)), _wref(case, "z_lo")[0], case.name)


# ---------------------------------------------------------------------------------------------- data gradient
@pytest.mark.parametrize("cls", cr.DGRAD_CLASSES)
@pytest.mark.parametrize("case", cr.DGRAD_2D, ids=_ids(cr.DGRAD_2D))
def test_dgrad_2d_case_meets_its_precondition_and_torch_fp32_is_bit_exact(case, cls):
    d, dy = cr.dgrad_make(case, cls)
    _is_class(cls, dy, d["w"])
    dx, mag = cr.dgrad_reference(case, d, dy)
    assert tuple(dx.shape) == (case.n, case.h, case.w, case.cin)
    assert 2.0 ** 9 * mag.max().item() < cr.WGRAD_LIMIT
    x = torch.zeros(case.n, case.h, case.w, case.cin, requires_grad=True)
    raw = cr._contract(x.permute(0, 3, 1, 2), d["w"], case.stride, case.dil, case.pad[0], case.pad[1], None)
    assert raw.dtype == torch.float32 and tuple(raw.shape) == tuple(dy.shape)
    cr.assert_exact(torch.autograd.grad(raw, x, dy)[0], dx, case.name)
    assert dx.abs().max().item() > 0


# ---------------------------------------------------------------------------------------------- rounding cases
@pytest.mark.parametrize("w", cr.WGRAD_ROUNDING + [cr.WGRAD_ROUNDING_1D], ids=lambda w: w.case.name)
def test_torch_fp32_meets_the_weight_gradient_bounds(w):
    case = w.case
    d, dz = cr.wgrad_make(case, "normal")
    dw, mag = cr.wgrad_reference(case, d, dz)
    err = (cr.wgrad_rows(case, d, dz).double() - dw).abs()
    r32, rb3 = (err / cr.wgrad_bound_f32(case, mag, 1)).max().item(), (err / cr.wgrad_bound_b3(case, mag)).max().item()
    print(f"{case.name}: torch fp32 worst error / fp32 bound = {r32:.3f}, / bf16x3 bound = {rb3:.3f}")
    assert r32 < 1.0 and rb3 < 1.0
