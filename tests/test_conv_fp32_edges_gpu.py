"""The fp32 implicit-GEMM conv (csrc/conv_igemm.hip), its general epilogue (csrc/conv_common.h) and ``ops.linear`` against the
float64 reference of ``tests/conv_ref.py``.

The exact cases carry integer-valued data for which every product and every partial sum, in any order, is a float32 number
(``conv_ref``'s docstring; the precondition of every case is asserted by ``tests/test_conv_ref_cpu.py``): the kernel has to
return the float64 reference bit for bit whatever the tile, the split-K factor or the order of its reduction, so these
comparisons are ``torch.equal`` and carry no tolerance.  The rounding cases keep a check on fp32 accumulation of normal data
against the derived bound ``conv_ref.rounding_bound`` and print their worst error / bound.
"""
import ctypes
import functools

import pytest
import torch

import conv_ref as cr

pytestmark = pytest.mark.gpu

NAN = float("nan")
TILES = [0, 1, 2, 4, 5]


def _ops():
    from feature_vs_text_compound_emotion_amd import ops
    return ops


def _ids(table):
    return [c.name for c in table]


@functools.lru_cache(maxsize=None)
def _data(case, exact=True):
    return cr.make(case, exact=exact)


@functools.lru_cache(maxsize=None)
def _ref(case, exact=True):
    return cr.reference(case, _data(case, exact))


def _cuda(t):
    return None if t is None else t.cuda()


def _launch(case, d, tile=0, split_k=None, want_stats=False):
    """One ``ops.conv2d`` call of a case.  Returns (y [N,Ho,Wo,Cout], aux or None, stats or None) as float64 CPU tensors after
    checking that the columns of ``out`` beyond Cout (the pitch ``y_ld``) are still NaN."""
    ops = _ops()
    n, h, w, cin, cout = case.n, case.h, case.w, case.cin, case.cout
    ho, wo = cr.out_hw_of(case)
    kw = {}
    if case.nchw:
        x = d["x"].permute(0, 3, 1, 2).contiguous().cuda()
        kw["x_nchw"] = True
    elif case.x_wide is not None:
        width, off = case.x_wide
        buf = torch.full((n * h * w, width), NAN)
        buf[:, off:off + cin] = d["x"].reshape(-1, cin)
        x = buf.cuda()[:, off:off + cin]
        kw.update(x_ld=width, x_shape=(n, h, w, cin))
    else:
        x = d["x"].contiguous().cuda()
    y_ld = cout + case.y_extra if case.y_extra else 0
    out = torch.full((n * ho * wo, y_ld or cout), NAN, device="cuda")
    aux = torch.full((n, ho, wo, cout), NAN, device="cuda") if case.aux else None
    r = ops.conv2d(x, ops.pack_conv_weight(d["w"].cuda()), case.kh, case.kw, stride=case.stride, dil=case.dil, pad=case.pad,
                   out_hw=case.out_hw, in_scale=_cuda(d["in_scale"]), in_shift=_cuda(d["in_shift"]), bias=_cuda(d["bias"]),
                   alpha=_cuda(d["alpha"]), residual=_cuda(d["residual"]), res_stride=d["res_stride"], mask=_cuda(d["mask"]),
                   act1=cr.ACTS[case.act1], act2=cr.ACTS[case.act2], slope=cr.SLOPE,
                   split_k=case.split_k if split_k is None else split_k, tile=tile, out=out, aux=aux, y_ld=y_ld,
                   want_stats=want_stats, **kw)
    stats = r[1].cpu().double() if want_stats else None
    torch.cuda.synchronize()
    host = out.cpu()
    assert torch.isnan(host[:, cout:]).all(), "columns beyond Cout were written"
    y = host[:, :cout].double().reshape(n, ho, wo, cout)
    return y, (aux.cpu().double() if aux is not None else None), stats


def _check(case, tile=0, split_k=None):
    y_ref, aux_ref, _ = _ref(case)
    y, aux, _ = _launch(case, _data(case), tile=tile, split_k=split_k)
    assert torch.equal(y, y_ref), f"{case.name}: {(y != y_ref).sum().item()} of {y.numel()} outputs differ"
    if case.aux:
        assert torch.equal(aux, aux_ref), f"{case.name}: aux differs"
    return y


# ---------------------------------------------------------------------------------------------- geometry, exact
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("case", cr.GEOMETRY, ids=_ids(cr.GEOMETRY))
def test_geometry_exact(case, tile):
    _check(case, tile=tile)


# ---------------------------------------------------------------------------------------------- input paths, exact
@pytest.mark.parametrize("case", cr.INPUTS, ids=_ids(cr.INPUTS))
def test_input_paths_exact(case):
    _check(case)


# ---------------------------------------------------------------------------------------------- epilogue, exact
@pytest.mark.parametrize("case", cr.EPILOGUE, ids=_ids(cr.EPILOGUE))
def test_epilogue_exact(case):
    _check(case)


# ---------------------------------------------------------------------------------------------- split-K, exact
@pytest.mark.parametrize("case,factors", cr.SPLIT_K, ids=[c.name for c, _ in cr.SPLIT_K])
def test_split_k_exact_and_identical_to_one_slab(case, factors):
    one = _check(case, split_k=1)
    for s in factors:
        assert torch.equal(_check(case, split_k=s), one), f"split_k = {s}"


# ---------------------------------------------------------------------------------------------- causal 1-D and its data gradient
def _rows(t):
    return t.reshape(-1, t.shape[-1]).contiguous().cuda()


@pytest.mark.parametrize("case", cr.CAUSAL, ids=_ids(cr.CAUSAL))
def test_causal_conv_rows_exact(case):
    from feature_vs_text_compound_emotion_amd.temporal_convnet import _conv_rows
    d = _data(case)
    y = _conv_rows(_rows(d["x"]), d["w"][:, :, :, 0].contiguous().cuda(), case.n, case.h, case.kh, case.dil[0], bias=d["bias"].cuda())
    assert torch.equal(y.cpu().double().view(case.n, case.h, 1, case.cout), _ref(case)[0])


def test_causal_conv_rows_with_the_tcn_second_conv_epilogue():
    from feature_vs_text_compound_emotion_amd.temporal_convnet import _conv_rows
    ops, case = _ops(), cr.CAUSAL_TCN
    d = _data(case)
    aux = torch.full((case.n * case.h, case.cout), NAN, device="cuda")
    y = _conv_rows(_rows(d["x"]), d["w"][:, :, :, 0].contiguous().cuda(), case.n, case.h, case.kh, case.dil[0], bias=d["bias"].cuda(),
                   act1=ops.ACT_LEAKY, mask=_rows(d["mask"]), residual=d["residual"].cuda(), act2=ops.ACT_LEAKY, aux=aux,
                   slope=cr.SLOPE)
    y_ref, aux_ref, _ = _ref(case)
    assert torch.equal(y.cpu().double().view(y_ref.shape), y_ref)
    assert torch.equal(aux.cpu().double().view(aux_ref.shape), aux_ref)


@pytest.mark.parametrize("case", cr.CAUSAL, ids=_ids(cr.CAUSAL))
def test_anticausal_dgrad_rows_exact(case):
    """dX of the causal conv (pad = 0, flipped and transposed filter, taps past the END of the sequence are zero) against the
    float64 autograd gradient of the same conv."""
    from feature_vs_text_compound_emotion_amd.temporal_convnet import _dgrad_rows
    d = _data(case)
    dz, res = cr.dgrad_draw(case), cr.dgrad_residual(case)
    want = cr.dgrad_reference(case, d, dz)[0]
    if res is not None:
        want = want + res.double()
    dx = _dgrad_rows(_rows(dz), d["w"][:, :, :, 0].contiguous().cuda(), case.n, case.h, case.kh, case.dil[0],
                     residual=None if res is None else _rows(res))
    assert torch.equal(dx.cpu().double().view(want.shape), want)


# ---------------------------------------------------------------------------------------------- statistics, exact
def _desc(case, tile):
    from feature_vs_text_compound_emotion_amd._lib import ConvDesc
    ho, wo = cr.out_hw_of(case)
    d = ConvDesc()
    d.N, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout = case.n, case.h, case.w, case.cin, ho, wo, case.cout
    d.KH, d.KW, d.stride, d.dil_h, d.dil_w, d.pad_t, d.pad_l = case.kh, case.kw, case.stride, case.dil[0], case.dil[1], *case.pad
    d.res_stride, d.act1, d.act2, d.slope, d.split_k, d.tile = 1, cr.ACTS[case.act1], cr.ACTS[case.act2], cr.SLOPE, 1, tile
    return d


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("case", cr.STATS, ids=_ids(cr.STATS))
def test_statistics_are_exact_sums_of_the_raw_accumulators(case, tile):
    from feature_vs_text_compound_emotion_amd import _lib
    ops = _ops()
    d = _data(case)
    y_ref, _, raw = _ref(case)
    assert cr.stats_margin(raw) < 2.0 ** 24                              # the precondition of an exact comparison
    y, _, stats = _launch(case, d, tile=tile, want_stats=True)
    assert torch.equal(y, y_ref)                                          # bias + PReLU went into y ...
    tiles = _lib.load().cer_conv2d_stats_tiles(ctypes.byref(_desc(case, tile)), 0)
    m = raw.numel() // case.cout
    bm = cr.TILE_ROWS[tile] if tile else {-(-m // 128): 128, -(-m // 64): 64}[tiles]
    assert tiles == -(-m // bm) and tuple(stats.shape) == (tiles, 2, case.cout)
    assert torch.equal(stats, cr.tile_rows(raw, bm))                      # ... and not into the statistics; last tile: rows < M
    # the partials through bn_finalize against the float64 batch-norm formula (bars of tests/test_sync_bn_gpu.py: 2 U on a
    # value rounded once -- gamma is a power of two --, 8 U on the sums of two fp32 terms)
    g = torch.Generator().manual_seed(case.cout)
    gamma = cr.pick(g,(case.cout,), [0.5, 1.0, 2.0])
    beta, rm0, rv0 = torch.randn(case.cout, generator=g), torch.randn(case.cout, generator=g), torch.rand(case.cout, generator=g) + 0.5
    rm, rv = rm0.cuda(), rv0.cuda()
    eps, mom = 1e-5, 0.1
    scale, shift = ops.bn_finalize(stats.float().cuda(), float(m), gamma.cuda(), beta.cuda(), rm, rv, momentum=mom, eps=eps)
    r2 = raw.reshape(m, case.cout)
    mean = r2.sum(0) / m
    var = (r2 * r2).sum(0) / m - mean * mean
    s_ref = gamma.double() / torch.sqrt(var + eps)
    t_ref = beta.double() - mean * s_ref
    assert ((scale.cpu().double() - s_ref).abs() <= 2 * cr.U * s_ref.abs()).all()
    assert ((shift.cpu().double() - t_ref).abs() <= 8 * cr.U * (beta.double().abs() + (mean * s_ref).abs())).all()
    unbiased = var * m / (m - 1)
    assert ((rm.cpu().double() - ((1 - mom) * rm0.double() + mom * mean)).abs() <= 8 * cr.U * (rm0.double().abs() + mean.abs())).all()
    assert ((rv.cpu().double() - ((1 - mom) * rv0.double() + mom * unbiased)).abs() <= 8 * cr.U * (rv0.double().abs() + unbiased.abs())).all()


# ---------------------------------------------------------------------------------------------- ops.linear, exact
@pytest.mark.parametrize("case", cr.LINEAR, ids=_ids(cr.LINEAR))
def test_linear_on_column_slices_exact(case):
    ops = _ops()
    d = _data(case)
    m, k, cout = case.n, case.cin, case.cout
    width, off = case.x_wide
    xb = torch.full((m, width), NAN)
    xb[:, off:off + k] = d["x"].view(m, k)
    ob = torch.full((m, cout + case.y_extra), NAN, device="cuda")
    out = ob[:, 8:8 + cout]
    res = d["residual"].view(m, cout).cuda() if d["residual"] is not None else None
    y = ops.linear(xb.cuda()[:, off:off + k], ops.pack_conv_weight(d["w"].cuda()), bias=d["bias"].cuda(), residual=res, out=out)
    assert y.data_ptr() == out.data_ptr()
    host = ob.cpu()
    assert torch.equal(host[:, 8:8 + cout].double().view(m, 1, 1, cout), _ref(case)[0])
    assert torch.isnan(host[:, :8]).all() and torch.isnan(host[:, 8 + cout:]).all()


@pytest.mark.parametrize("case", cr.LINEAR_T, ids=_ids(cr.LINEAR_T))
def test_linear_with_the_transposed_pack_gives_dy_times_w(case):
    """``lfan._linear_T``: W [out = 7, in = 32] packed with ``transpose=True``, dX = dY @ W."""
    ops = _ops()
    d = _data(case)
    m, n_cls, feat = case.n, case.cin, case.cout
    w = d["w"].view(feat, n_cls).t().contiguous()                      # the Linear's weight [out, in]
    wt = ops.pack_conv_weight(w.view(n_cls, feat, 1, 1).cuda(), transpose=True)
    assert tuple(wt.shape) == (feat, 32)
    dx = ops.linear(d["x"].view(m, n_cls).cuda(), wt)
    assert torch.equal(dx.cpu().double(), d["x"].view(m, n_cls).double() @ w.double())
    assert torch.equal(dx.cpu().double().view(m, 1, 1, feat), _ref(case)[0])


# ---------------------------------------------------------------------------------------------- refusals
def _refusal_operands(cin=64, hw=4, cout=64, kh=3, kw=3):
    ops = _ops()
    x = torch.zeros(1, hw, hw, cin, device="cuda")
    w = torch.zeros(cout, ops.conv_kpad(kh, kw, cin), device="cuda")
    out = torch.full((1, hw, hw, cout), NAN, device="cuda")
    return ops, x, w, out


def _untouched(out):
    torch.cuda.synchronize()
    return bool(torch.isnan(out).all())


def test_statistics_with_split_k_are_refused():
    ops, x, w, out = _refusal_operands()
    with pytest.raises(RuntimeError, match="not available with split-K"):
        ops.conv2d(x, w, 3, 3, pad=(1, 1), split_k=2, want_stats=True, out=out)
    assert _untouched(out)


def test_more_than_32_taps_on_the_vector_path_are_refused():
    ops = _ops()
    x = torch.zeros(1, 4, 12, 32, device="cuda")
    w = torch.zeros(64, ops.conv_kpad(3, 11, 32), device="cuda")
    out = torch.full((1, 4, 12, 64), NAN, device="cuda")
    with pytest.raises(RuntimeError, match="32 filter taps"):
        ops.conv2d(x, w, 3, 11, pad=(1, 5), out=out)
    assert _untouched(out)


def test_nchw_input_with_cin_32_is_refused():
    ops, _, w, out = _refusal_operands(cin=32)
    with pytest.raises(RuntimeError, match="NCHW"):
        ops.conv2d(torch.zeros(1, 32, 4, 4, device="cuda"), w, 3, 3, pad=(1, 1), x_nchw=True, out=out)
    assert _untouched(out)


def test_unaligned_x_ld_on_the_vector_path_is_refused():
    ops, _, w, out = _refusal_operands(cin=32)
    buf = torch.zeros(16, 34, device="cuda")
    with pytest.raises(RuntimeError, match="x_ld"):
        ops.conv2d(buf[:, :32], w, 3, 3, pad=(1, 1), x_ld=34, x_shape=(1, 4, 4, 32), out=out)
    assert _untouched(out)


def test_y_ld_below_cout_is_refused():
    ops, x, w, _ = _refusal_operands()
    out = torch.full((16, 60), NAN, device="cuda")
    with pytest.raises(RuntimeError, match="y_ld"):
        ops.conv2d(x, w, 3, 3, pad=(1, 1), y_ld=60, out=out)
    assert _untouched(out)


def test_residual_geometry_out_of_range_is_refused():
    ops, x, w, out = _refusal_operands()
    with pytest.raises(RuntimeError, match="residual geometry"):
        ops.conv2d(x, w, 3, 3, pad=(1, 1), residual=torch.zeros(1, 4, 4, 64, device="cuda"), res_stride=2, out=out)
    assert _untouched(out)


def test_unknown_tile_id_is_refused():
    ops, x, w, out = _refusal_operands()
    with pytest.raises(RuntimeError, match="unknown tile id"):
        ops.conv2d(x, w, 3, 3, pad=(1, 1), tile=3, out=out)
    assert _untouched(out)


def test_mask_with_the_wrong_element_count_is_refused_by_the_wrapper():
    ops, x, w, out = _refusal_operands()
    with pytest.raises(ValueError, match="mask"):
        ops.conv2d(x, w, 3, 3, pad=(1, 1), mask=torch.ones(1, 4, 4, 32, device="cuda"), out=out)
    assert _untouched(out)


# ---------------------------------------------------------------------------------------------- rounding cases
@pytest.mark.parametrize("case", cr.ROUNDING, ids=_ids(cr.ROUNDING))
def test_rounding_stays_inside_the_derived_bound(case):
    """|y - y64| <= 1.01 u (K + S + 8) (A + |bias| + |residual|) per output (``conv_ref.rounding_bound``).  GELU: x 1.13 plus
    four times the error of torch's fp32 erf on this device over the same pre-activations plus 4 u.
    Measured on an MI355X, worst error / bound: see DESIGN.md section 2."""
    d = _data(case, False)
    y_ref, _, raw = _ref(case, False)
    erf_err = cr.erf_error(raw + d["bias"].double(), device="cuda") if case.act1 == "gelu" else None
    bound = cr.rounding_bound(case, d, erf_err)
    y, _, _ = _launch(case, d)
    ratio = ((y - y_ref).abs() / bound).max().item()
    extra = ""
    if erf_err is not None:
        extra = f", device erf error {erf_err:.3e}, allowance {4 * erf_err + 4 * cr.U:.3e}"
    print(f"{case.name}: worst error / bound = {ratio:.4f}, worst error {(y - y_ref).abs().max().item():.3e}{extra}")
    assert ratio < 1.0
