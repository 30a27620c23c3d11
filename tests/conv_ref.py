"""A float64 reference of ``ops.conv2d`` / ``ops.linear`` on the fp32 implicit-GEMM kernel, and the case tables of its edge tests.

Nothing here needs a GPU: ``tests/test_conv_ref_cpu.py`` checks the reference and every table on any machine,
``tests/test_conv_fp32_edges_gpu.py`` runs the tables on ``csrc/conv_igemm.hip`` and the epilogue of ``csrc/conv_common.h``.
The second half of the file is the same for the backward convs (weight and data gradients; ``tests/test_conv_backward_edges_gpu.py``).

The contract is the docstring of ``ops.conv2d``:

  y = act2(mask * act1(conv(affine(x), w) + bias) + residual),   aux = mask * act1(conv(affine(x), w) + bias)

with the affine ``x * in_scale[c] + in_shift[c]`` applied to in-bounds pixels only (padding stays zero), only the top and left
padding given (whatever the taps reach beyond the image is zero) and ``out_hw`` cropping or fixing the output grid.

Two kinds of cases:

* EXACT.  x, w, bias, residual and in_shift are small integers, in_scale and the PReLU slopes powers of two, the leaky slope
  0.25, masks in {0, 2}.  Let ``unit`` be the product of the smallest |in_scale| (if below 1), the smallest PReLU slope and 0.25
  per leaky activation: every value that can occur anywhere in the launch -- a product, a partial sum of products in ANY order,
  the sum with the bias, an activation, the masked value, the sum with the residual -- is an integer multiple of ``unit``.  With
  B = 2 (A + |bias|) + |residual| (A = the sum of |products| of one output, 2 = the largest mask value) bounding all of their
  magnitudes, B / unit < 2^24 makes every one of them a float32 number and every operation on them exact.  So the kernel has
  to return the float64 reference BIT FOR BIT, whatever its tile, its split-K factor or the permutation of its reduction, and
  any dropped, duplicated or mis-addressed term shows as a difference of at least ``unit``.  ``exact_margin`` returns
  max B / unit; the CPU test asserts it below 2^24 for every exact case (which includes A < 2^24).
  For the batch statistics the same holds when every per-tile column sum of raw^2 stays below 2^24 (``stats_margin``).

* ROUNDING.  Standard-normal data, one case per path, against a derived bound with u = 2^-24:

      |y - y64| <= 1.01 u (K + S + 8) (A + |bias| + |residual|)

  K products and K - 1 additions of one output in any order lose at most ~K u A (the fp32 matrix cores' fused multiply-adds
  lose less), S split-K slabs add S - 1 more additions, and 8 covers the affine (two roundings per input value), the bias, the
  activation, the mask, the residual and ``act2`` (one each).  GELU multiplies the pre-activation bound by its Lipschitz constant
  1.13 and adds an allowance for ``erff``: four times the error of ``torch.erf`` in fp32 on the SAME device over the same
  pre-activations, plus 4 u (``rounding_bound(..., erf_err=...)``).
"""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

ACT_NONE, ACT_PRELU, ACT_LEAKY, ACT_RELU, ACT_GELU = 0, 1, 2, 3, 4      # cer_hip.h / _lib.py
ACTS = {"none": ACT_NONE, "prelu": ACT_PRELU, "leaky": ACT_LEAKY, "relu": ACT_RELU, "gelu": ACT_GELU}
U = 2.0 ** -24
SLOPE = 0.25
GELU_LIPSCHITZ = 1.13


# ---------------------------------------------------------------------------------------------- the reference
def _act(v, act, alpha, slope):
    if act == ACT_PRELU:
        return torch.where(v >= 0, v, v * alpha)
    if act == ACT_LEAKY:
        return torch.where(v >= 0, v, v * slope)
    if act == ACT_RELU:
        return torch.where(v <= 0, torch.zeros_like(v), v)        # NaN passes, as torch.relu (non-finite values)
    if act == ACT_GELU:
        return 0.5 * v * (1.0 + torch.erf(v * 0.70710678118654752440))
    return v


def out_size(h, w, kh, kw, stride, dil, pad):
    """The natural output grid of ``ops.conv2d`` (it takes the given padding as symmetric)."""
    return ((h + 2 * pad[0] - dil[0] * (kh - 1) - 1) // stride + 1, (w + 2 * pad[1] - dil[1] * (kw - 1) - 1) // stride + 1)


def _contract(x_nchw, w, stride, dil, pad_t, pad_l, out_hw):
    h, wd = x_nchw.shape[2:]
    kh, kw = w.shape[2:]
    ho, wo = out_hw if out_hw is not None else out_size(h, wd, kh, kw, stride, dil, (pad_t, pad_l))
    pad_b = max(0, (ho - 1) * stride + dil[0] * (kh - 1) + 1 - (h + pad_t))       # whatever the last taps reach: zeros
    pad_r = max(0, (wo - 1) * stride + dil[1] * (kw - 1) + 1 - (wd + pad_l))
    y = F.conv2d(F.pad(x_nchw, (pad_l, pad_r, pad_t, pad_b)), w, None, stride, 0, dil)
    return y[:, :, :ho, :wo].permute(0, 2, 3, 1)


def conv_ref(x_nhwc, w_oihw, *, stride=1, dil=(1, 1), pad_t=0, pad_l=0, out_hw=None, in_scale=None, in_shift=None, bias=None,
             act1=ACT_NONE, alpha=None, slope=0.01, mask=None, residual=None, res_stride=1, act2=ACT_NONE, dtype=torch.float64):
    """(y, aux, raw), NHWC, in ``dtype`` (float64; float32 makes the same function torch's own fp32 CPU realisation).
    ``raw`` is the contraction before the bias, ``aux`` the value before the residual add."""
    cv = (lambda t: None if t is None else t.detach().to(dtype))
    x, w, in_scale, in_shift, bias, alpha, mask, residual = (cv(t) for t in (x_nhwc, w_oihw, in_scale, in_shift, bias, alpha,
                                                                               mask, residual))
    if in_scale is not None:
        x = x * in_scale + in_shift                       # before F.pad: the padding stays zero
    raw = _contract(x.permute(0, 3, 1, 2), w, stride, dil, pad_t, pad_l, out_hw)
    v = raw if bias is None else raw + bias
    v = _act(v, act1, alpha, slope)
    if mask is not None:
        v = v * mask.reshape(v.shape)
    aux = v
    if residual is not None:
        ho, wo = v.shape[1:3]
        v = v + residual[:, ::res_stride, ::res_stride][:, :ho, :wo]
    return _act(v, act2, None, slope), aux, raw


def conv_mag(x_nhwc, w_oihw, *, stride=1, dil=(1, 1), pad_t=0, pad_l=0, out_hw=None, in_scale=None, in_shift=None):
    """The magnitude twin: the same contraction on |x| |in_scale| + |in_shift| and |w| -- A, the sum of |products| per output."""
    x = x_nhwc.detach().double().abs()
    if in_scale is not None:
        x = x * in_scale.double().abs() + in_shift.double().abs()
    return _contract(x.permute(0, 3, 1, 2), w_oihw.detach().double().abs(), stride, dil, pad_t, pad_l, out_hw)


def conv_loops(x_nhwc, w_oihw, *, stride=1, dil=(1, 1), pad_t=0, pad_l=0, out_hw=None, in_scale=None, in_shift=None, bias=None,
               act1=ACT_NONE, alpha=None, slope=0.01, mask=None, residual=None, res_stride=1, act2=ACT_NONE):
    """``conv_ref`` restated as the kernel's gather: one output at a time, tap by tap, bounds tested per tap (tiny shapes)."""
    x, w = x_nhwc.double(), w_oihw.double()
    n, h, wd, cin = x.shape
    cout, _, kh, kw = w.shape
    ho, wo = out_hw if out_hw is not None else out_size(h, wd, kh, kw, stride, dil, (pad_t, pad_l))
    y, aux, raw = (torch.zeros(n, ho, wo, cout, dtype=torch.float64) for _ in range(3))
    scalar_act = (lambda v, act, a: float(_act(torch.tensor(v, dtype=torch.float64), act,
                                                None if a is None else torch.tensor(a, dtype=torch.float64), slope)))
    for b in range(n):
        for i in range(ho):
            for j in range(wo):
                for co in range(cout):
                    s = 0.0
                    for r in range(kh):
                        for q in range(kw):
                            hi, wi = i * stride - pad_t + r * dil[0], j * stride - pad_l + q * dil[1]
                            if not (0 <= hi < h and 0 <= wi < wd):
                                continue
                            for c in range(cin):
                                v = float(x[b, hi, wi, c])
                                if in_scale is not None:
                                    v = v * float(in_scale[c]) + float(in_shift[c])
                                s += v * float(w[co, c, r, q])
                    raw[b, i, j, co] = s
                    t = s + (float(bias[co]) if bias is not None else 0.0)
                    t = scalar_act(t, act1, float(alpha[co]) if alpha is not None else None)
                    if mask is not None:
                        t *= float(mask.reshape(n, ho, wo, cout)[b, i, j, co])
                    aux[b, i, j, co] = t
                    if residual is not None:
                        t += float(residual[b, i * res_stride, j * res_stride, co])
                    y[b, i, j, co] = scalar_act(t, act2, None)
    return y, aux, raw


# ---------------------------------------------------------------------------------------------- cases
# n h w cin cout kh kw stride dil pad: the geometry (pad = (top, left)); out_hw None = natural.  nchw: x is handed over NCHW.
# x_wide (width, offset): x is columns offset .. offset + cin of a width-wide NaN-filled buffer.  affine / bias: given or not.
# act1 / act2: names of ACTS.  mask / aux: given or not.  res: "none" | "same" | "stride2" (an odd-sized (2 Ho - 1) x (2 Wo - 1)
# tensor read with res_stride = 2).  y_extra: out is a NaN-filled buffer of row pitch cout + y_extra.  split_k as passed.
# stats: the launch takes batch statistics.  lim_x / lim_w: integer ranges of the exact draws.
_FIELDS = ("name n h w cin cout kh kw stride dil pad out_hw nchw x_wide affine bias act1 mask aux res act2 y_extra split_k stats "
           "lim_x lim_w")
_DEFAULTS = dict(stride=1, dil=(1, 1), pad=(0, 0), out_hw=None, nchw=False, x_wide=None, affine=False, bias=False, act1="none",
                 mask=False, aux=False, res="none", act2="none", y_extra=0, split_k=1, stats=False, lim_x=4, lim_w=4)
Case = namedtuple("Case", _FIELDS)


def C(name, n, h, w, cin, cout, kh, kw, **kw_):
    d = dict(_DEFAULTS)
    d.update(kw_)
    return Case(name=name, n=n, h=h, w=w, cin=cin, cout=cout, kh=kh, kw=kw, **d)


def linear_case(name, m, k, cout, **kw_):
    """[M, K] @ W[Cout, K]^T as ``ops.linear`` runs it: a 1x1 conv on an [M, 1, 1, K] image."""
    return C(name, m, 1, 1, k, cout, 1, 1, **kw_)


def causal_case(name, bsz, length, cin, cout, k, dil, **kw_):
    """``temporal_convnet._conv_rows``: [B, L, 1, Cin] image, k x 1 filter, dilation d, (k - 1) d rows of left padding."""
    return C(name, bsz, length, 1, cin, cout, k, 1, dil=(dil, 1), pad=((k - 1) * dil, 0), out_hw=(length, 1), **kw_)


# geometry (each runs on tile 0 = the picker, 1 = 128x128, 2 = 128x64, 4 = 64x128, 5 = 64x64)
GEOMETRY = [
    # (a) M = 147: a 128-row tile spans three 49-pixel images and leaves a 19-row tail; Cout = 37: scalar epilogue
    C("a_cout36", 3, 7, 7, 32, 36, 3, 3, pad=(1, 1)),
    C("a_cout37", 3, 7, 7, 32, 37, 3, 3, pad=(1, 1)),
    # (b) stride 2 on odd and even sizes, H != W
    C("b_3x3_7x10", 2, 7, 10, 32, 64, 3, 3, stride=2, pad=(1, 1)),
    C("b_3x3_8x5", 2, 8, 5, 32, 64, 3, 3, stride=2, pad=(1, 1)),
    C("b_1x1_7x10", 2, 7, 10, 32, 64, 1, 1, stride=2),
    C("b_1x1_8x5", 2, 8, 5, 32, 64, 1, 1, stride=2),
    # (c) 1x3 and 5x1 filters, dilations (1,3) and (2,1), pad_t != pad_l, natural output size; the 5x1 taps pass the bottom edge
    C("c_1x3_d13", 2, 6, 9, 32, 64, 1, 3, dil=(1, 3), pad=(0, 2)),
    C("c_1x3_d21", 2, 6, 9, 32, 64, 1, 3, dil=(2, 1), pad=(0, 1)),
    C("c_5x1_d13", 2, 9, 6, 32, 64, 5, 1, dil=(1, 3), pad=(1, 0)),
    C("c_5x1_d21", 2, 9, 6, 32, 64, 5, 1, dil=(2, 1), pad=(3, 0)),
    # (d) ragged against both 64 and 128 in Cout, three K chunks per tap
    C("d_96_100", 2, 5, 5, 96, 100, 3, 3, pad=(1, 1)),
]

# input paths: the element-wise gather (Cin % 32 != 0), NCHW, the in-affine under padding, column slices
INPUTS = [
    C("gather_cin1", 2, 6, 5, 1, 64, 3, 3, pad=(1, 1)),
    C("gather_cin3", 2, 6, 5, 3, 64, 3, 3, pad=(1, 1)),
    C("gather_cin7_1x1", 2, 6, 5, 7, 36, 1, 1),
    C("gather_cin40", 2, 6, 5, 40, 64, 3, 3, pad=(1, 1)),                # K = 360, Kpad = 384: a K tail inside the last step
    C("nchw_cin1", 2, 6, 5, 1, 64, 3, 3, pad=(1, 1), nchw=True),
    C("nchw_cin3", 2, 6, 5, 3, 37, 3, 3, pad=(1, 1), nchw=True),
    C("affine_vector", 2, 6, 5, 32, 64, 3, 3, pad=(1, 1), affine=True),   # padded taps must add zero, not the shift
    C("affine_gather40", 2, 6, 5, 40, 64, 3, 3, pad=(1, 1), affine=True),
    C("affine_gather7_splitk", 2, 6, 5, 7, 37, 3, 3, pad=(1, 1), affine=True, split_k=2),
    C("slice_cin32", 2, 6, 5, 32, 64, 3, 3, pad=(1, 1), x_wide=(40, 4)),
    C("slice_cin7", 2, 6, 5, 7, 64, 3, 3, pad=(1, 1), x_wide=(12, 4)),
    C("slice_cin7_affine_splitk", 2, 6, 5, 7, 36, 3, 3, pad=(1, 1), x_wide=(12, 4), affine=True, split_k=2),
    C("gather_cin40_splitk", 2, 6, 5, 40, 37, 3, 3, pad=(1, 1), split_k=5),
]

# epilogue: (bias, act1, mask, aux, res, act2, cout, y_extra, split_k).  The first sixteen rows cover every PAIR of option values
# (asserted by the CPU test); the first is the TCN block's second conv verbatim.  The rest are the launches of the fast epilogue
# (epi_store4_direct) and the split-K reducer's scalar path with a residual.
_EPI_ROWS = [
    (1, "leaky", 1, 1, "same", "leaky", 64, 0, 1),
    (0, "none", 0, 0, "none", "none", 37, 4, 1),
    (0, "prelu", 0, 1, "stride2", "none", 64, 3, 3),
    (1, "relu", 0, 0, "same", "leaky", 37, 3, 3),
    (0, "relu", 1, 1, "none", "leaky", 64, 4, 3),
    (1, "prelu", 1, 0, "stride2", "leaky", 37, 0, 1),
    (0, "leaky", 0, 0, "none", "none", 37, 0, 3),
    (1, "none", 1, 1, "none", "none", 64, 3, 1),
    (0, "relu", 1, 1, "same", "none", 37, 0, 1),
    (1, "none", 0, 0, "same", "leaky", 37, 4, 3),
    (0, "leaky", 0, 0, "stride2", "leaky", 64, 4, 3),
    (0, "prelu", 1, 0, "same", "none", 37, 4, 1),
    (0, "none", 1, 1, "stride2", "none", 64, 0, 1),
    (1, "prelu", 0, 1, "none", "none", 37, 4, 3),
    (0, "relu", 0, 1, "stride2", "leaky", 64, 4, 1),
    (1, "leaky", 1, 0, "same", "leaky", 64, 3, 1),
    (1, "prelu", 0, 0, "same", "none", 64, 0, 1),
    (1, "relu", 0, 0, "stride2", "none", 64, 4, 1),
    (1, "none", 0, 0, "none", "none", 64, 0, 3),
    (1, "prelu", 0, 0, "stride2", "none", 64, 0, 3),
    (1, "relu", 0, 0, "stride2", "none", 37, 0, 3),
    (1, "leaky", 1, 1, "same", "leaky", 37, 3, 3),
    (1, "leaky", 1, 1, "same", "leaky", 64, 4, 3),
    (0, "none", 0, 0, "same", "none", 37, 3, 1),
]
EPI_FACTORS = ("bias", "act1", "mask", "aux", "res", "act2", "cout", "y_extra", "split_k")
N_PAIRWISE = 16
# N = 3 images of 5x5: M = 75, two 64-row tiles; 3x3 on Cin = 32: nine K steps for split_k = 3
EPILOGUE = [C("epi%02d_%s" % (i, "_".join(str(v) for v in r)), 3, 5, 5, 32, r[6], 3, 3, pad=(1, 1), bias=bool(r[0]), act1=r[1],
              mask=bool(r[2]), aux=bool(r[3]), res=r[4], act2=r[5], y_extra=r[7], split_k=r[8]) for i, r in enumerate(_EPI_ROWS)]

# split-K: each case runs at split_k = 1 and at every factor of its list; all results are bit-identical and equal the reference
SPLIT_K = [
    # 5x1, dilation 2, Cin = 64: ten K steps.  3 -> slabs of 4, 4, 2 (a shorter last slab); 4 -> 3, 3, 3, 1; 16 -> clamped to 10
    (C("splitk_5x1_dil2", 2, 9, 3, 64, 64, 5, 1, dil=(2, 1), pad=(4, 0), out_hw=(9, 3)), (3, 4, 16)),
    # K = 1280 linear (40 steps), M = 70, residual + ReLU.  7 -> six slabs of 6 and one of 4; Cout = 37: the reducer's scalar path
    (linear_case("splitk_linear_cout64", 70, 1280, 64, bias=True, act1="relu", res="same", lim_x=3, lim_w=3), (2, 7)),
    (linear_case("splitk_linear_cout37", 70, 1280, 37, bias=True, act1="relu", res="same", lim_x=3, lim_w=3), (2, 7)),
]

# batch statistics of the raw accumulators, under a bias and a PReLU in the same launch (each on tiles 0, 1, 2, 4, 5)
STATS = [C("stats_cout%d" % co, 3, 7, 7, 32, co, 3, 3, pad=(1, 1), bias=True, act1="prelu", stats=True, lim_x=2, lim_w=1)
         for co in (64, 100, 37)]
TILE_ROWS = {1: 128, 2: 128, 4: 64, 5: 64}

# causal 1-D (temporal_convnet._conv_rows) and its anti-causal data gradient (_dgrad_rows): B = 3, k = 5; L = 1 and
# (k - 1) dil >= L (only the last taps see data) included
CAUSAL = [causal_case("causal_L%d_d%d_%dto%d" % (length, dil, ci, co), 3, length, ci, co, 5, dil, bias=True)
          for length in (1, 5, 16) for dil in (1, 4, 8) for ci, co in ((32, 64), (64, 32))]
# the TCN block's second conv on its own geometry: bias, leaky, mask, residual, leaky, aux
CAUSAL_TCN = causal_case("causal_tcn_conv2", 3, 5, 64, 64, 5, 4, bias=True, act1="leaky", mask=True, aux=True, res="same",
                         act2="leaky")
# data-gradient cases that also add the ``residual`` argument (the downsample branch's gradient)
DGRAD_WITH_RESIDUAL = ("causal_L5_d4_32to64", "causal_L16_d1_64to32")

# ops.linear with x2d and out as column slices of wider buffers (offsets 4 and 8 floats): M x K x residual
LINEAR = [linear_case("linear_M%d_K%d_%s" % (m, k, "res" if r else "plain"), m, k, 36, bias=True, res="same" if r else "none",
                      x_wide=(k + 8, 4), y_extra=12)
          for m in (1, 129) for k in (7, 200, 64) for r in (False, True)]
# lfan._linear_T: dX = dY @ W through pack_conv_weight(transpose=True); Cin of the launch = the 7 classes
LINEAR_T = [linear_case("linear_T_M%d" % m, m, 7, 32) for m in (1, 129)]

EXACT = GEOMETRY + INPUTS + EPILOGUE + [c for c, _ in SPLIT_K] + STATS + CAUSAL + [CAUSAL_TCN] + LINEAR + LINEAR_T

# rounding cases: standard-normal data, w / sqrt(K)
ROUNDING = [
    C("round_vector_cin96_affine", 2, 7, 7, 96, 64, 3, 3, pad=(1, 1), affine=True, bias=True),
    C("round_gather_cin40", 2, 7, 7, 40, 64, 3, 3, pad=(1, 1), bias=True),
    linear_case("round_linear_cin7", 129, 7, 32, bias=True),
    linear_case("round_linear_k1280_split5", 70, 1280, 64, bias=True, res="same", split_k=5),
    linear_case("round_gelu_linear", 70, 96, 100, bias=True, act1="gelu"),
]


def by_name(table):
    return {c.name: c for c in table}


# ---------------------------------------------------------------------------------------------- data
def _seed(case):
    return sum((i + 1) * b for i, b in enumerate(case.name.encode())) % (2 ** 31)


def _ints(g, shape, lim):
    return torch.randint(-lim, lim + 1, shape, generator=g).float()


def pick(g, shape, values):
    return torch.tensor(values, dtype=torch.float32)[torch.randint(0, len(values), shape, generator=g)]


def out_hw_of(case):
    return case.out_hw if case.out_hw is not None else out_size(case.h, case.w, case.kh, case.kw, case.stride, case.dil, case.pad)


def make(case, exact=True):
    """The operands of a case as float32 CPU tensors (None where the case has none): x NHWC, w OIHW, in_scale, in_shift, bias,
    alpha, mask, residual NHWC, res_stride.  Deterministic in the case's name."""
    g = torch.Generator().manual_seed(_seed(case))
    ho, wo = out_hw_of(case)
    k = case.kh * case.kw * case.cin
    d = dict.fromkeys(("in_scale", "in_shift", "bias", "alpha", "mask", "residual"))
    if exact:
        d["x"] = _ints(g, (case.n, case.h, case.w, case.cin), case.lim_x)
        d["w"] = _ints(g, (case.cout, case.cin, case.kh, case.kw), case.lim_w)
    else:
        d["x"] = torch.randn(case.n, case.h, case.w, case.cin, generator=g)
        d["w"] = torch.randn(case.cout, case.cin, case.kh, case.kw, generator=g) / math.sqrt(k)
    if case.affine:
        d["in_scale"] = pick(g, (case.cin,), [0.5, 1.0, 2.0, -1.0]) if exact else torch.rand(case.cin, generator=g) + 0.5
        d["in_shift"] = _ints(g, (case.cin,), 2) if exact else torch.randn(case.cin, generator=g) * 0.3
        if exact:
            d["in_shift"][0] = 2.0                       # never all zero
    if case.bias:
        d["bias"] = _ints(g, (case.cout,), 8) if exact else torch.randn(case.cout, generator=g)
    if case.act1 == "prelu":
        d["alpha"] = pick(g, (case.cout,), [0.5, 0.25, 0.125]) if exact else torch.rand(case.cout, generator=g) * 0.3 + 0.1
    if case.mask:
        d["mask"] = pick(g, (case.n, ho, wo, case.cout), [0.0, 2.0, 2.0])
    shape = {"none": None, "same": (case.n, ho, wo, case.cout), "stride2": (case.n, 2 * ho - 1, 2 * wo - 1, case.cout)}[case.res]
    if shape is not None:
        d["residual"] = _ints(g, shape, 8) if exact else torch.randn(shape, generator=g)
    d["res_stride"] = 2 if case.res == "stride2" else 1
    return d


def ref_kwargs(case, d):
    """What ``conv_ref`` / ``conv_loops`` take for a case."""
    return dict(stride=case.stride, dil=case.dil, pad_t=case.pad[0], pad_l=case.pad[1], out_hw=case.out_hw, in_scale=d["in_scale"],
                in_shift=d["in_shift"], bias=d["bias"], act1=ACTS[case.act1], alpha=d["alpha"], slope=SLOPE, mask=d["mask"],
                residual=d["residual"], res_stride=d["res_stride"], act2=ACTS[case.act2])


def mag_kwargs(case, d):
    kw = ref_kwargs(case, d)
    return {k: kw[k] for k in ("stride", "dil", "pad_t", "pad_l", "out_hw", "in_scale", "in_shift")}


def reference(case, d, dtype=torch.float64):
    return conv_ref(d["x"], d["w"], dtype=dtype, **ref_kwargs(case, d))


def _cropped_residual(case, d):
    if d["residual"] is None:
        return None
    ho, wo = out_hw_of(case)
    return d["residual"].double()[:, ::d["res_stride"], ::d["res_stride"]][:, :ho, :wo]


def exact_margin(case, d):
    """max B / unit of the module docstring (must stay below 2^24), and max A."""
    a = conv_mag(d["x"], d["w"], **mag_kwargs(case, d))
    b = a + (d["bias"].double().abs() if d["bias"] is not None else 0.0)
    b = 2.0 * b
    res = _cropped_residual(case, d)
    if res is not None:
        b = b + res.abs()
    unit = 1.0
    if d["in_scale"] is not None:
        unit *= min(1.0, d["in_scale"].abs().min().item())
    if d["alpha"] is not None:
        unit *= d["alpha"].abs().min().item()
    unit *= SLOPE ** ((case.act1 == "leaky") + (case.act2 == "leaky"))
    assert math.log2(unit) == round(math.log2(unit))
    return b.max().item() / unit, a.max().item()


def tile_rows(raw, bm):
    """raw [N, Ho, Wo, C] -> the per-tile (sum, sum of squares) [tiles, 2, C] over blocks of ``bm`` pixel rows."""
    r = raw.reshape(-1, raw.shape[-1])
    return torch.stack([torch.stack([blk.sum(0), (blk * blk).sum(0)]) for blk in r.split(bm)])


def stats_margin(raw):
    """The largest per-tile column sum of raw^2 over the tile heights in use (must stay below 2^24 for exact statistics; the
    128-row tiles bound the 64-row ones)."""
    return max(tile_rows(raw, bm)[:, 1].max().item() for bm in (64, 128))


def dgrad_draw(case):
    """The output gradient dz [N, Ho, Wo, Cout] of a data-gradient case: small integers."""
    ho, wo = out_hw_of(case)
    return _ints(torch.Generator().manual_seed(_seed(case) + 1), (case.n, ho, wo, case.cout), 4)


def dgrad_residual(case):
    """The tensor ``_dgrad_rows`` adds to the gradient ([N, H, W, Cin]), for the cases that pass one."""
    if case.name not in DGRAD_WITH_RESIDUAL:
        return None
    return _ints(torch.Generator().manual_seed(_seed(case) + 2), (case.n, case.h, case.w, case.cin), 8)


def dgrad_reference(case, d, dz):
    """float64 autograd gradient of the causal conv with respect to x for the output gradient dz [N, Ho, Wo, Cout], and the
    magnitude twin (the same gradient on |dz|, |w|): both NHWC."""
    out = []
    for f in (lambda t: t.double(), lambda t: t.double().abs()):
        x = torch.zeros(case.n, case.h, case.w, case.cin, dtype=torch.float64, requires_grad=True)
        raw = _contract(x.permute(0, 3, 1, 2), f(d["w"]), case.stride, case.dil, case.pad[0], case.pad[1], case.out_hw)
        out.append(torch.autograd.grad(raw, x, f(dz))[0])
    return out


def rounding_bound(case, d, erf_err=None):
    """The per-output bound of the module docstring for a rounding case; GELU needs ``erf_err``, the measured fp32 erf error."""
    a = conv_mag(d["x"], d["w"], **mag_kwargs(case, d))
    t = a + (d["bias"].double().abs() if d["bias"] is not None else 0.0)
    res = _cropped_residual(case, d)
    if res is not None:
        t = t + res.abs()
    k = case.kh * case.kw * case.cin
    bound = 1.01 * U * (k + case.split_k + 8) * t
    if case.act1 == "gelu":
        bound = GELU_LIPSCHITZ * bound + 4.0 * erf_err + 4.0 * U
    return bound


def erf_error(pre64, device="cpu"):
    """The error of ``torch.erf`` in fp32 on ``device`` against float64 over the arguments GELU hands it."""
    arg = (pre64 * 0.70710678118654752440).float()
    return (torch.erf(arg.to(device)).cpu().double() - torch.erf(arg.double())).abs().max().item()


# ====================================================================================================================
# The backward convs: the weight gradient (csrc/wgrad.hip, csrc/wgrad_b3.hip) and ``visual_backbone._conv_dgrad``.
#
#   dW[co][ci][kh][kw] = sum over output pixels r = (n, ho, wo) of dZ[r][co] X[n, ho s - pad_t + kh dil_h, wo s - pad_l + kw dil_w][ci]
#
# Three operand classes, all values multiples of 2^-8 and deterministic in the case name:
#
#   ints   dz and x integers in [-4, 4]
#   x_lo   dz in {-1, 0, 1}, x = m / 256 with |m| <= 2047: twelve significant bits, so bf16(x) drops up to four and the ``lo``
#          plane of x is nonzero for about two thirds of the values, while dz has lo == 0
#   z_lo   the mirror image: dz twelve bits, x ternary
#
# In every class one operand of each product has lo == 0, so dz x = dz_hi x_hi + dz_hi x_lo (or + dz_lo x_hi) holds exactly and the
# lo lo product the bf16x3 kernels drop is zero; hi and lo themselves are multiples of 2^-8 with |hi| + |lo| <= 2 |value|.  Every
# product and every partial sum, in any order and over any subset of rows, taps, splits and planes, is therefore a multiple of 2^-8
# of magnitude at most 2 mag (mag = sum |dz| |x|, the magnitude twin), and with 2^9 max(mag) < 2^24 (``wgrad_exact_margin``: a
# condition, asserted on the CPU for every case) all of them are float32 numbers and every addition is exact.  The bf16x3 kernels
# then owe the float64 gradient BIT FOR BIT like the fp32-MFMA kernel, whatever their tile, split or summation order, and a dropped,
# doubled or misrouted row, tap, split, plane or tile shows as a nonzero difference.  The same holds for the data gradient with
# (dy, w) in the place of (dz, x).
OPERAND_CLASSES = ("ints", "x_lo", "z_lo")
WGRAD_LIMIT = 2.0 ** 24


def _lo12(g, shape):
    return torch.randint(-2047, 2048, shape, generator=g).float() / 256.0


def _ternary(g, shape):
    return torch.randint(-1, 2, shape, generator=g).float()


def _pair(g, cls, shape_z, shape_x):
    """(z, x) of an operand class; z is drawn first."""
    if cls == "ints":
        return _ints(g, shape_z, 4), _ints(g, shape_x, 4)
    if cls == "x_lo":
        return _ternary(g, shape_z), _lo12(g, shape_x)
    if cls == "z_lo":
        return _lo12(g, shape_z), _ternary(g, shape_x)
    if cls == "normal":
        return torch.randn(shape_z, generator=g), torch.randn(shape_x, generator=g)
    raise ValueError(cls)


def wgrad_make(case, cls="ints"):
    """(d, dz) of a weight-gradient case: d["x"] [N, H, W, Cin] and the output gradient dz [N, Ho, Wo, Cout], float32 on the CPU."""
    g = torch.Generator().manual_seed(_seed(case) + 7 * (1 + (OPERAND_CLASSES + ("normal",)).index(cls)))
    ho, wo = out_hw_of(case)
    dz, x = _pair(g, cls, (case.n, ho, wo, case.cout), (case.n, case.h, case.w, case.cin))
    return {"x": x}, dz


def wgrad_reference(case, d, dz):
    """float64 autograd gradient of the conv with respect to its WEIGHT for the output gradient dz, [Cout, Cin, KH, KW], and the
    magnitude twin sum |dz| |x|."""
    out = []
    for f in (lambda t: t.double(), lambda t: t.double().abs()):
        w = torch.zeros(case.cout, case.cin, case.kh, case.kw, dtype=torch.float64, requires_grad=True)
        raw = _contract(f(d["x"]).permute(0, 3, 1, 2), w, case.stride, case.dil, case.pad[0], case.pad[1], case.out_hw)
        out.append(torch.autograd.grad(raw, w, f(dz))[0])
    return out


def wgrad_exact_margin(case, d, dz):
    """2^9 max(mag): 2^8 for the unit 2^-8 of the operand classes, 2 for |hi| + |lo| >= |value|.  Must stay below 2^24."""
    return 2.0 ** 9 * wgrad_reference(case, d, dz)[1].max().item()


def wgrad_loops(case, d, dz):
    """The weight gradient as the kernels gather it, written out one product at a time (tiny shapes)."""
    x, z = d["x"].double(), dz.double()
    ho, wo = out_hw_of(case)
    dw = torch.zeros(case.cout, case.cin, case.kh, case.kw, dtype=torch.float64)
    for b in range(case.n):
        for i in range(ho):
            for j in range(wo):
                for r in range(case.kh):
                    for q in range(case.kw):
                        hi, wi = i * case.stride - case.pad[0] + r * case.dil[0], j * case.stride - case.pad[1] + q * case.dil[1]
                        if 0 <= hi < case.h and 0 <= wi < case.w:
                            dw[:, :, r, q] += torch.outer(z[b, i, j], x[b, hi, wi])
    return dw


def bf16_hi(t):
    """The hi plane of ``ops.split_bf16``: the value rounded to bfloat16."""
    return t.to(torch.bfloat16).float()


WGRAD_MUTANTS = ("hw_swap", "pad_swap", "tap_div_kh", "drop_last_step", "drop_lo", "tile_neighbour")


def wgrad_rows(case, d, dz, dtype=torch.float32, mutant=None):
    """The weight gradient as a float32 CPU GEMM per filter tap over the pixel rows r = (n, ho, wo): a correct contraction that is
    not the code under test (``mutant`` None), or one with a deliberate mistake of the kind a kernel could make:

      hw_swap         Ho written for Wo in the decomposition of r      pad_swap        pad_t and pad_l exchanged
      tap_div_kh      kh = tap // KH instead of tap // KW              drop_last_step  the last partial 32-row step left out
      drop_lo         the lo plane of x left out (x rounded to bf16)   tile_neighbour  the dz columns past a 128-wide tile edge
                                                                                       taken from the tile before
    """
    assert mutant is None or mutant in WGRAD_MUTANTS
    ho, wo = out_hw_of(case)
    rows = case.n * ho * wo
    x = d["x"].reshape(-1, case.cin).to(dtype)
    z = dz.reshape(rows, case.cout).to(dtype)
    if mutant == "drop_lo":
        x = bf16_hi(x).to(dtype)
    if mutant == "tile_neighbour" and case.cout > 128:
        z = torch.cat([z[:, :128], z[:, :case.cout - 128]], 1)
    if mutant == "drop_last_step":
        rows = rows // 32 * 32
    pad_t, pad_l = case.pad[::-1] if mutant == "pad_swap" else case.pad
    r = torch.arange(rows)
    n, q = r // (ho * wo), r % (ho * wo)
    i, j = (q // ho, q % ho) if mutant == "hw_swap" else (q // wo, q % wo)
    dw = torch.zeros(case.cout, case.cin, case.kh, case.kw, dtype=dtype)
    for tap in range(case.kh * case.kw):
        a = tap // (case.kh if mutant == "tap_div_kh" else case.kw)
        b = tap - a * case.kw
        hi, wi = i * case.stride - pad_t + a * case.dil[0], j * case.stride - pad_l + b * case.dil[1]
        ok = (hi >= 0) & (hi < case.h) & (wi >= 0) & (wi < case.w)
        src = ((n * case.h + hi) * case.w + wi).clamp(0, x.shape[0] - 1)
        xg = torch.where(ok[:, None], x[src], torch.zeros((), dtype=dtype))
        dw[:, :, tap // case.kw, tap % case.kw] = z[:rows].t() @ xg
    return dw


def assert_exact(got, ref, what):
    """THE comparison of the exact backward tests: ``got`` (any float dtype, any device) equals the float64 ``ref`` bit for bit."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)}, expected {tuple(ref.shape)}"
    if not torch.equal(got, ref):
        bad = got != ref
        first = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {ref.numel()} values differ, first at {first}: "
                             f"{got[first].item()!r} for {ref[first].item()!r}")


# ---- weight gradient, 2-D.  The name carries the geometry and the path ``wgrad_b3_tile`` / the dispatch of ``wgrad_b3_run`` send
# the channel set to: t64 = the 64-wide tile (<64, *>), t128 = <128, false> with fp32 operands and the NON-DMA <128, true> with Split
# operands (a channel count that is no multiple of 8), t128dma = <128, true, DMA> with Split operands, wide = the 256 x 256 kernel
# with Split operands (<128, false> with fp32 operands); f32only = a channel count that is no multiple of 4 (csrc/wgrad.hip only).
# split_b3 / split_f32: the launch is expected to take the row-split path of wgrad_b3.hip / wgrad.hip (the GPU test asserts it
# through the workspace the library asks for); R = N Ho Wo in the comment.
WCase = namedtuple("WCase", "case split_b3 split_f32")


def _w(name, n, h, w, cin, cout, kh, kw, split_b3, split_f32, **kw_):
    return WCase(C(name, n, h, w, cin, cout, kh, kw, **kw_), split_b3, split_f32)


WGRAD_2D = [
    # H != W under 3x3; R = 1500 = 5 x 256 + 220: six splits, the last one partial and ending in a 28-row step
    _w("rect10x25_3x3_4to64_t64stem", 6, 10, 25, 4, 64, 3, 3, True, True, pad=(1, 1)),
    _w("rect10x25_3x3_3to64_f32only_cin3", 6, 10, 25, 3, 64, 3, 3, None, True, pad=(1, 1)),
    _w("rect10x25_3x3_40to7_f32only_cout7", 6, 10, 25, 40, 7, 3, 3, None, True, pad=(1, 1)),
    _w("rect10x25_3x3_1to64_f32only_cin1", 6, 10, 25, 1, 64, 3, 3, None, True, pad=(1, 1)),          # the first VGGish conv's channels
    # KH != KW, pad_t != pad_l with a pad of 0; R = 1440: six splits of 256 rows, 160 in the last
    _w("rect10x25_3x2_pad1x0_72to132_t128", 6, 10, 25, 72, 132, 3, 2, True, True, pad=(1, 0)),
    _w("rect10x25_3x2_pad1x0_200to40_t64ragged", 6, 10, 25, 200, 40, 3, 2, True, True, pad=(1, 0)),
    # 1x3 with a pad of 2 under three taps and no padding above; R = 392 = 12 x 32 + 8
    _w("rect7x12_1x3_pad0x2_72to200_t128dma_partial", 4, 7, 12, 72, 200, 1, 3, False, True, pad=(0, 2)),
    # 3x3 with pad (2, 0): the output is taller than the input; R = 288
    _w("rect6x11_3x3_pad2x0_128to256_t128dma_full", 4, 6, 11, 128, 256, 3, 3, False, True, pad=(2, 0)),
    # 3x1, stride 2, (H, W) = (9, 8) of mixed parity; R = 600: two splits of 320 rows
    _w("s2_9x8_3x1_pad1x0_128to256_t128dma_full", 30, 9, 8, 128, 256, 3, 1, True, True, stride=2, pad=(1, 0)),
    # 3x3, stride 2, (7, 10) -> (4, 5); R = 200
    _w("s2_7x10_3x3_200to40_t64ragged", 10, 7, 10, 200, 40, 3, 3, False, True, stride=2, pad=(1, 1)),
    # 1x1, stride 2, pad 0; R = 600
    _w("s2_7x10_1x1_256to512_wide", 30, 7, 10, 256, 512, 1, 1, True, True, stride=2),
    # Ho Wo = 6 < 32: five images and more in one 32-row step; R = 300
    _w("tiny3x5_n50_s2_3x3_72to132_t128", 50, 3, 5, 72, 132, 3, 3, False, True, stride=2, pad=(1, 1)),
    _w("tiny3x5_n50_s2_3x3_72to200_t128dma_partial", 50, 3, 5, 72, 200, 3, 3, False, True, stride=2, pad=(1, 1)),
    _w("tiny3x5_n50_s2_3x3_4to64_t64stem", 50, 3, 5, 4, 64, 3, 3, False, True, stride=2, pad=(1, 1)),
    _w("tiny3x5_n50_s2_1x3_256to512_wide", 50, 3, 5, 256, 512, 1, 3, False, True, stride=2, pad=(0, 1)),
    # Wo = 70 > 64 with Ho = 2: a step is less than one image row; R = 420
    _w("row2x70_3x3_4to64_t64stem", 3, 2, 70, 4, 64, 3, 3, False, True, pad=(1, 1)),
    _w("row2x70_3x3_128to256_t128dma_full", 3, 2, 70, 128, 256, 3, 3, False, True, pad=(1, 1)),
    _w("row2x70_3x3_72to132_t128", 3, 2, 70, 72, 132, 3, 3, False, True, pad=(1, 1)),
    _w("row2x70_1x3_pad0x1_256to512_wide", 3, 2, 70, 256, 512, 1, 3, False, True, pad=(0, 1)),
    # Wo == 1; R = 63: one pass in every kernel
    _w("col9x3_wo1_3x3_pad1x0_200to40_t64ragged", 7, 9, 3, 200, 40, 3, 3, False, False, pad=(1, 0)),
    _w("col9x3_wo1_3x3_pad1x0_72to132_t128", 7, 9, 3, 72, 132, 3, 3, False, False, pad=(1, 0)),
    _w("col9x3_wo1_3x3_pad1x0_72to200_t128dma_partial", 7, 9, 3, 72, 200, 3, 3, False, False, pad=(1, 0)),
    _w("col9x3_wo1_3x3_pad1x0_256to512_wide", 7, 9, 3, 256, 512, 3, 3, False, False, pad=(1, 0)),
]

# ---- weight gradient, causal 1-D (ops.conv1d_wgrad and, through it, conv1d_wgrad_weight_norm_bwd): the ``causal_case`` geometry.
# x_wide / dz_wide = (pitch, offset): the operand is columns offset .. of a pitch-wide NaN-filled buffer.
W1Case = namedtuple("W1Case", "case x_wide dz_wide split_f32")


def _w1(name, bsz, length, cin, cout, k, dil, x_wide=None, dz_wide=None, split=True):
    return W1Case(causal_case(name, bsz, length, cin, cout, k, dil), x_wide, dz_wide, split)


# R = 300 = 15 sequences of 20: three splits of 128, 128 and 44 rows, sequence boundaries inside steps and inside splits
WGRAD_1D = [
    _w1("w1_k5_d1_36to64", 15, 20, 36, 64, 5, 1),
    _w1("w1_k5_d2_64to36", 15, 20, 64, 36, 5, 2),
    _w1("w1_k5_d4_96to200", 15, 20, 96, 200, 5, 4),
    _w1("w1_k5_d8_200to96_zero_taps", 15, 20, 200, 96, 5, 8),          # taps 0 and 1 shift by 32 and 24 >= L: zero slabs
    _w1("w1_k5_d8_7to7", 15, 20, 7, 7, 5, 8),
    _w1("w1_k1_200to7", 15, 20, 200, 7, 1, 1),
    _w1("w1_k1_7to200", 15, 20, 7, 200, 1, 1),
    _w1("w1_k5_d2_96to64_one_pass", 3, 20, 96, 64, 5, 2, split=False),           # R = 60
    _w1("w1_k5_d2_96to64_slices_off4_off64", 15, 20, 96, 64, 5, 2, x_wide=(104, 4), dz_wide=(132, 64)),
    _w1("w1_k1_200to36_slices_off64_off4", 15, 20, 200, 36, 1, 1, x_wide=(264, 64), dz_wide=(44, 4)),
    _w1("w1_k5_d1_36to64_pitch_not_x4", 15, 20, 36, 64, 5, 1, x_wide=(39, 0), dz_wide=(67, 2)),
    _w1("w1_k5_d1_36to64_slices_off1_pitch_x4", 15, 20, 36, 64, 5, 1, x_wide=(40, 1), dz_wide=(68, 1)),
    _w1("w1_k1_96to7_slice_off1_pitch_x4", 15, 20, 96, 7, 1, 1, x_wide=(100, 1)),
]

# ---- data gradient (visual_backbone._conv_dgrad): 3x3 / pad 1 or 1x1 / pad 0, stride 1 or 2; (dy, w) classes "ints" and "x_lo"
# (ternary dy, 12-bit weights)
def _dg(name, n, h, w, cin, cout, k, stride):
    return C(name, n, h, w, cin, cout, k, k, stride=stride, pad=(k // 2, k // 2))


DGRAD_2D = [
    _dg("dg_s1_3x3_5x12", 3, 5, 12, 32, 64, 3, 1),
    _dg("dg_s1_1x1_5x12", 3, 5, 12, 64, 128, 1, 1),
    _dg("dg_s1_3x3_16x32_n32_window", 32, 16, 32, 32, 64, 3, 1),        # 64 blocks of 256 pixels: the window-resident kernels
    _dg("dg_s2_3x3_5x8", 3, 5, 8, 32, 64, 3, 2),
    _dg("dg_s2_3x3_8x5", 3, 8, 5, 32, 64, 3, 2),
    _dg("dg_s2_3x3_7x9", 3, 7, 9, 64, 128, 3, 2),
    _dg("dg_s2_3x3_6x10", 3, 6, 10, 32, 64, 3, 2),
    _dg("dg_s2_3x3_1x4", 3, 1, 4, 32, 64, 3, 2),                        # H = 1: the odd-row parities have no pixel
    _dg("dg_s2_3x3_2x1", 3, 2, 1, 32, 64, 3, 2),
    _dg("dg_s2_1x1_5x8", 3, 5, 8, 32, 64, 1, 2),
    _dg("dg_s2_1x1_4x7", 3, 4, 7, 64, 128, 1, 2),
]
DGRAD_CLASSES = ("ints", "x_lo")


def dgrad_make(case, cls="ints"):
    """(d, dy) of a data-gradient case: d["w"] [Cout, Cin, KH, KW] and dy [N, Ho, Wo, Cout]."""
    g = torch.Generator().manual_seed(_seed(case) + 11 * (1 + OPERAND_CLASSES.index(cls)))
    ho, wo = out_hw_of(case)
    dy, w = _pair(g, cls, (case.n, ho, wo, case.cout), (case.cout, case.cin, case.kh, case.kw))
    return {"w": w}, dy


# ---- rounding: standard-normal operands on rectangular, asymmetric geometry, one case per kernel family (the names say which)
WGRAD_ROUNDING = [
    _w("round_rect10x25_3x2_pad1x0_72to132_f32_and_t128", 6, 10, 25, 72, 132, 3, 2, True, True, pad=(1, 0)),
    _w("round_s2_9x8_3x1_pad1x0_128to256_t128dma", 30, 9, 8, 128, 256, 3, 1, True, True, stride=2, pad=(1, 0)),
    _w("round_rect10x25_3x2_pad1x0_200to40_t64", 6, 10, 25, 200, 40, 3, 2, True, True, pad=(1, 0)),
    _w("round_s2_7x10_1x3_pad0x2_256to512_wide", 30, 7, 10, 256, 512, 1, 3, True, True, stride=2, pad=(0, 2)),
]
WGRAD_ROUNDING_1D = _w1("round_w1_k5_d2_96to200", 15, 20, 96, 200, 5, 2)


def wgrad_rows_of(case):
    ho, wo = out_hw_of(case)
    return case.n * ho * wo


def wgrad_bound_b3(case, mag):
    """The project's bf16x3 bound (tests/test_head_release_gpu.py): every product drops lo lo and rounds both lo parts,
    <= 2^-15 relative, plus fp32 accumulation over the R rows."""
    return mag * (2.0 ** -15 + wgrad_rows_of(case) * 2.0 ** -24) + 1e-6


def wgrad_bound_f32(case, mag, splits):
    """The analogue of ``rounding_bound`` with the reduction length R: 1.01 u (R + splits + 8) mag."""
    return 1.01 * U * (wgrad_rows_of(case) + splits + 8) * mag


def weight_norm_bwd_bound(dw, v, g):
    """Bounds (dv, dg) on the fp32 error of the weight-norm backward of w = g v / n, n = ||v|| per output channel over E elements:

        dg = sum dw v / n,      dv = (g / n) (dw - v dg / n)

    derived like ``rounding_bound``: E products and additions lose <= E u A with A = sum |dw| |v| / n, 8 covers the divisions and
    the roundings outside the sum, and the fp32 norm the kernel is handed carries a relative error <= E u of its own, which
    enters dg once (another E u A), the first term of dv once and the second twice."""
    dw, v, g = dw.double(), v.double(), g.double().reshape(-1, 1, 1)
    e = v[0].numel()
    n = v.reshape(v.shape[0], -1).norm(dim=1).reshape(-1, 1, 1)
    a = (dw.abs() * v.abs()).sum((1, 2), keepdim=True) / n
    scale = (g / n).abs()
    dg = 1.01 * U * (2 * e + 8) * a
    dv = 1.01 * U * ((e + 8) * scale * dw.abs() + (4 * e + 16) * scale * v.abs() / n * a)
    return dv, dg
