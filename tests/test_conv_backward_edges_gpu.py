"""The backward convs against the float64 references of ``tests/conv_ref.py``: the fp32-MFMA weight gradient (csrc/wgrad.hip:
``ops.conv1d_wgrad``, ``ops.conv1d_wgrad_weight_norm_bwd``, ``ops.conv2d_wgrad``), the bf16x3 weight gradient
(csrc/wgrad_b3.hip: ``ops.conv2d_wgrad(..., b3=True)`` on fp32 and on ``Split`` operands) and ``visual_backbone._conv_dgrad``.

The exact cases carry operands of three classes (``conv_ref.OPERAND_CLASSES``: small integers, or one ternary operand against one
of twelve significant bits) for which every product -- also as the two or three bf16 products of the bf16x3 kernels -- and every
partial sum in any order is a float32 number; the precondition of every case is asserted by ``tests/test_conv_ref_cpu.py``, which
also shows that the comparison used here rejects contractions with a swapped H / W, swapped paddings, ``tap // KH``, a dropped
last step, a dropped lo plane and a misrouted tile.  So every kernel owes the float64 gradient bit for bit: the comparisons are
``conv_ref.assert_exact`` and carry no tolerance.  The rounding cases keep a check on normal data against the project's bounds and
print their worst error / bound.
"""
import functools

import pytest
import torch

import conv_ref as cr

pytestmark = pytest.mark.gpu

NAN = float("nan")
KERNELS = ("f32", "b3", "b3s")          # wgrad.hip; wgrad_b3.hip on fp32 operands; wgrad_b3.hip on Split operands


def _ops():
    from feature_vs_text_compound_emotion_amd import ops
    return ops


def _lib():
    from feature_vs_text_compound_emotion_amd import _lib as lib
    return lib.load()


@functools.lru_cache(maxsize=None)
def _wdata(case, cls):
    return cr.wgrad_make(case, cls)


@functools.lru_cache(maxsize=None)
def _wref(case, cls):
    return cr.wgrad_reference(case, *_wdata(case, cls))


def _workspace(case, kernel):
    """The bytes the library asks for: nonzero exactly when the launch splits its rows over blocks."""
    ho, wo = cr.out_hw_of(case)
    if kernel == "f32":
        return _lib().cer_conv_wgrad_workspace_bytes(case.n * ho * wo, case.cout, case.cin, case.kh * case.kw)
    return _lib().cer_conv2d_wgrad_b3_workspace_bytes(case.n, ho, wo, case.cout, case.cin, case.kh, case.kw)


def _wgrad_2d(case, d, dz, kernel):
    ops = _ops()
    z, x = dz.cuda(), d["x"].cuda()
    if kernel == "b3s":
        z, x = ops.split_bf16(z), ops.split_bf16(x)
    dw = ops.conv2d_wgrad(z, x, case.kh, case.kw, stride=case.stride, pad=case.pad, b3=kernel != "f32")
    torch.cuda.synchronize()
    return dw


def _kernels_of(w):
    return KERNELS if w.split_b3 is not None else KERNELS[:1]


W2D_RUNS = [(w, k) for w in cr.WGRAD_2D for k in _kernels_of(w)]


# ---------------------------------------------------------------------------------------------- weight gradient, 2-D, exact
@pytest.mark.parametrize("cls", cr.OPERAND_CLASSES)
@pytest.mark.parametrize("w,kernel", W2D_RUNS, ids=[f"{w.case.name}-{k}" for w, k in W2D_RUNS])
def test_wgrad_2d_exact(w, kernel, cls):
    case = w.case
    assert (_workspace(case, kernel) > 0) == (w.split_f32 if kernel == "f32" else w.split_b3), "row-split / single-pass mode"
    d, dz = _wdata(case, cls)
    cr.assert_exact(_wgrad_2d(case, d, dz, kernel), _wref(case, cls)[0], f"{case.name} [{kernel}, {cls}]")


# (channel counts that are both multiples of 256 go to the wide kernel with Split operands: another tile, another order)
SAME_TILE = [w for w in cr.WGRAD_2D if w.split_b3 is not None and (w.case.cin % 256 or w.case.cout % 256)]


@pytest.mark.parametrize("w", SAME_TILE, ids=[w.case.name for w in SAME_TILE])
def test_wgrad_b3_split_operands_equal_fp32_operands_on_the_same_tile(w):
    """Normal data: the loader's own hi / lo split and ``ops.split_bf16`` are the same arithmetic, so where both launches take the
    same tile the results are identical."""
    d, dz = cr.wgrad_make(w.case, "normal")
    assert torch.equal(_wgrad_2d(w.case, d, dz, "b3"), _wgrad_2d(w.case, d, dz, "b3s"))


# ---------------------------------------------------------------------------------------------- weight gradient, causal 1-D, exact
def _wide(t2d, wide):
    """[R, C] on the GPU, dense or as columns offset .. of a NaN-filled pitch-wide buffer."""
    if wide is None:
        return t2d.contiguous().cuda()
    pitch, off = wide
    buf = torch.full((t2d.shape[0], pitch), NAN)
    buf[:, off:off + t2d.shape[1]] = t2d
    return buf.cuda()[:, off:off + t2d.shape[1]]


def _operands_1d(w, cls):
    case = w.case
    d, dz = _wdata(case, cls)
    return _wide(dz.reshape(-1, case.cout), w.dz_wide), _wide(d["x"].reshape(-1, case.cin), w.x_wide)


@pytest.mark.parametrize("cls", cr.OPERAND_CLASSES)
@pytest.mark.parametrize("w", cr.WGRAD_1D, ids=[w.case.name for w in cr.WGRAD_1D])
def test_wgrad_1d_exact(w, cls):
    case = w.case
    assert (_workspace(case, "f32") > 0) == w.split_f32, "row-split / single-pass mode"
    z, x = _operands_1d(w, cls)
    if w.x_wide is not None and w.x_wide[1] % 4:
        assert x.data_ptr() % 16 and x.stride(0) % 4 == 0          # rows that start off a 16-byte boundary under a pitch % 4 == 0
    dw = _ops().conv1d_wgrad(z, x, case.h, case.kh, case.dil[0])
    torch.cuda.synchronize()
    cr.assert_exact(dw.view(case.cout, case.cin, case.kh, 1), _wref(case, cls)[0], f"{case.name} [{cls}]")


@pytest.mark.parametrize("w", cr.WGRAD_1D, ids=[w.case.name for w in cr.WGRAD_1D])
def test_wgrad_into_weight_norm_backward(w):
    """``conv1d_wgrad_weight_norm_bwd`` with g = ||v|| (the backward is not the identity): bit-identical to the three launches,
    and (dv, dg) inside ``conv_ref.weight_norm_bwd_bound`` of float64 autograd through ``oracle.tcn.weight_norm_weight`` fed
    the exact float64 weight gradient."""
    from oracle.tcn import weight_norm_weight
    ops, case = _ops(), w.case
    z, x = _operands_1d(w, "ints")
    gen = torch.Generator().manual_seed(cr._seed(case) + 3)
    v = torch.randn(case.cout, case.cin, case.kh, generator=gen)
    g = v.double().reshape(case.cout, -1).norm(dim=1).float().view(case.cout, 1, 1)
    vc, gc = v.cuda(), g.cuda()
    _, norm = ops.weight_norm_fwd(vc, gc)
    dv, dg = ops.conv1d_wgrad_weight_norm_bwd(z, x, case.h, case.kh, case.dil[0], vc, gc, norm)
    dv0, dg0 = ops.weight_norm_bwd(ops.conv1d_wgrad(z, x, case.h, case.kh, case.dil[0]), vc, gc, norm)
    torch.cuda.synchronize()
    assert torch.equal(dv, dv0) and torch.equal(dg, dg0)
    dw = _wref(case, "ints")[0][:, :, :, 0]
    v64, g64 = v.double().requires_grad_(True), g.double().requires_grad_(True)
    (weight_norm_weight(g64, v64) * dw).sum().backward()
    bv, bg = cr.weight_norm_bwd_bound(dw, v, g)
    rv = ((dv.cpu().double() - v64.grad).abs() / (bv + 1e-30)).max().item()
    rg = ((dg.cpu().double() - g64.grad).abs() / (bg + 1e-30)).max().item()
    print(f"{case.name}: weight-norm backward worst error / bound: dv {rv:.4f}, dg {rg:.4f}")
    assert rv < 1.0 and rg < 1.0
    assert not torch.equal(dv.cpu().double(), dw)                    # the backward did something


# ---------------------------------------------------------------------------------------------- weight gradient, rounding
@pytest.mark.parametrize("w", cr.WGRAD_ROUNDING, ids=[w.case.name for w in cr.WGRAD_ROUNDING])
def test_wgrad_2d_rounding_stays_inside_the_bounds(w):
    """bf16x3: mag (2^-15 + R 2^-24) + 1e-6; fp32-MFMA: 1.01 u (R + splits + 8) mag (``conv_ref.wgrad_bound_*``).
    Measured worst error / bound on an MI355X: DESIGN.md section 2."""
    case = w.case
    d, dz = cr.wgrad_make(case, "normal")
    dw, mag = cr.wgrad_reference(case, d, dz)
    splits = max(1, _workspace(case, "f32") // (4 * dw.numel()))
    bounds = {"f32": cr.wgrad_bound_f32(case, mag, splits), "b3": cr.wgrad_bound_b3(case, mag), "b3s": cr.wgrad_bound_b3(case, mag)}
    ratios = {}
    for kernel in KERNELS:
        err = (_wgrad_2d(case, d, dz, kernel).double().cpu() - dw).abs()
        ratios[kernel] = (err / bounds[kernel]).max().item()
    print(f"{case.name}: worst error / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in ratios.items()) + f" ({splits} fp32 splits)")
    assert max(ratios.values()) < 1.0, ratios


def test_wgrad_1d_rounding_stays_inside_the_bound():
    w = cr.WGRAD_ROUNDING_1D
    case = w.case
    d, dz = cr.wgrad_make(case, "normal")
    dw, mag = cr.wgrad_reference(case, d, dz)
    splits = max(1, _workspace(case, "f32") // (4 * dw.numel()))
    got = _ops().conv1d_wgrad(_wide(dz.reshape(-1, case.cout), None), _wide(d["x"].reshape(-1, case.cin), None), case.h, case.kh,
                              case.dil[0])
    ratio = ((got.double().cpu().view(dw.shape) - dw).abs() / cr.wgrad_bound_f32(case, mag, splits)).max().item()
    print(f"{case.name}: worst error / bound: f32 {ratio:.4f} ({splits} fp32 splits)")
    assert ratio < 1.0


# ---------------------------------------------------------------------------------------------- data gradient, exact
DGRAD_RUNS = [("fp32", "ints"), ("fp32", "x_lo"), ("bf16x3", "ints"), ("bf16x3", "x_lo"), ("fp16", "ints"), ("bf16", "ints")]


@functools.lru_cache(maxsize=None)
def _dref(case, cls):
    d, dy = cr.dgrad_make(case, cls)
    return d, dy, cr.dgrad_reference(case, d, dy)[0]


@pytest.mark.parametrize("prec,cls", DGRAD_RUNS, ids=[f"{p}-{c}" for p, c in DGRAD_RUNS])
@pytest.mark.parametrize("case", cr.DGRAD_2D, ids=[c.name for c in cr.DGRAD_2D])
def test_conv_dgrad_exact(case, prec, cls):
    """Rectangular inputs: height and width of different parity under the four-parity stride-2 decomposition, H = 1 and W = 1
    (a whole parity without pixels), the window-resident kernels at stride 1.  Integers are exact in all four precisions;
    ternary dy against 12-bit weights needs both bf16 planes of the filter."""
    from feature_vs_text_compound_emotion_amd.visual_backbone import _conv_dgrad
    d, dy, dx_ref = _dref(case, cls)
    if case.name.endswith("_window"):                  # the case exists to reach the window-resident kernels (tile ids 53 .. 59 / 71 .. 79)
        ops, launch = _ops(), (case.n, case.h, case.w, case.cout, case.cin, 3, 3, 1, (1, 1))
        assert prec == "fp32" or (ops.conv2d_b3_tile(*launch) in (53, 56, 58, 59) if prec == "bf16x3" else
                                  ops.conv2d_n16_tile(*launch) in (71, 72, 73, 76, 77, 78, 79))
    dx = _conv_dgrad(dy.cuda(), d["w"].cuda(), case.stride, case.pad[0], (case.h, case.w), prec)
    torch.cuda.synchronize()
    cr.assert_exact(dx, dx_ref, f"{case.name} [{prec}, {cls}]")
