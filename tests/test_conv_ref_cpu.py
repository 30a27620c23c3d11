"""The float64 conv reference and the case tables of the fp32 implicit-GEMM edge tests, checked without a GPU.

* ``conv_ref`` (F.pad + F.conv2d) against ``conv_loops``, the gather written out tap by tap;
* every exact case meets its precondition (``exact_margin`` < 2^24, which includes A < 2^24; the statistics condition where
  statistics are taken; the data-gradient cases on the gradient's own products), so a bit-for-bit comparison is owed;
* torch's own fp32 CPU conv -- a correct fp32 contraction that is not the code under test -- reproduces every exact reference
  bit for bit and stays inside every rounding bound.
"""
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
