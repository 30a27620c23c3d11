"""The non-finite contract of DESIGN.md ("Non-finite values") as torch-CPU float64 restatements, and the case tables of its tests.

Nothing here needs a GPU: ``tests/test_nonfinite_ref_cpu.py`` checks every table and restatement against torch on any machine,
``tests/test_nonfinite_gpu.py`` runs them on the kernels.

Two kinds of checks use this module:

* POISON.  One input element of a conv launch is NaN or +Inf.  The outputs whose receptive field holds that element are the
  reference's non-finite outputs (``poison_reference``: the mask once from the geometry, once read from ``F.conv2d`` in float64
  on the poisoned input); every other output has to be BIT-IDENTICAL to the same launch on the clean input, which needs no
  tolerance.  A border that a kernel handles by multiplying with a zero instead of selecting the tap away passes every
  finite test (0 * x == 0) and fails this one (0 * inf is NaN, in the neighbouring image).
  With one +Inf per receptive field and every weight non-zero the reference value is +-inf by the sign of the tap's weight,
  never NaN (``make_conv`` draws until every weight survives rounding to bf16 and to fp16; the CPU test asserts it).

* TABLES.  The elementwise rules (activations, their backward masks, max-pool, the roundings) written out with ``torch.where``
  on ``special_values()``; the CPU test pins each to torch's own operator, the GPU test pins each kernel to the table.
"""
import functools
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

NAN, INF = float("nan"), float("inf")
FLT_MAX = 3.4028234663852886e38
DENORM_MIN = 2.0 ** -149


# ---------------------------------------------------------------------------------------------- values and comparison
def special_values():
    """nan, +-inf, +-0, the smallest denormal, +-FLT_MAX, +-1 as float32."""
    return torch.tensor([NAN, INF, -INF, 0.0, -0.0, DENORM_MIN, FLT_MAX, -FLT_MAX, 1.0, -1.0], dtype=torch.float32)


def tiled_specials(n):
    """``special_values()`` repeated to length n."""
    s = special_values()
    return s.repeat((n + s.numel() - 1) // s.numel())[:n].clone()


def nan_equal(got, want, ignore_zero_sign=False):
    """Do two tensors hold NaN at the same positions and the same values elsewhere?  The sign of a zero counts unless
    ``ignore_zero_sign``.  Compared in float64 (exact for every narrower type)."""
    g, w = got.detach().cpu().double(), want.detach().cpu().double()
    if g.shape != w.shape or not torch.equal(torch.isnan(g), torch.isnan(w)):
        return False
    g, w = torch.nan_to_num(g, nan=0.0, posinf=INF, neginf=-INF), torch.nan_to_num(w, nan=0.0, posinf=INF, neginf=-INF)
    if not torch.equal(g, w):
        return False
    return ignore_zero_sign or torch.equal(torch.signbit(g), torch.signbit(w))


def describe_mismatch(got, want, limit=5):
    """The first few positions where ``nan_equal`` fails, for assertion messages."""
    g, w = got.detach().cpu().double(), want.detach().cpu().double()
    if g.shape != w.shape:
        return f"shapes {tuple(g.shape)} vs {tuple(w.shape)}"
    bad = ~((g == w) | (torch.isnan(g) & torch.isnan(w))) | (torch.signbit(g) != torch.signbit(w)) & ~torch.isnan(g)
    idx = bad.nonzero()[:limit].tolist()
    return "; ".join(f"{tuple(i)}: got {g[tuple(i)].item()} want {w[tuple(i)].item()}" for i in idx) + f" ({int(bad.sum())} differ)"


# ---------------------------------------------------------------------------------------------- elementwise tables
# Each function is the contract's rule spelled with comparisons and selects; test_nonfinite_ref_cpu.py pins it to torch.
def relu(v):
    """relu(nan) = nan, relu(-inf) = 0, relu(-0.0) = 0 of either sign (torch.relu keeps -0.0: the accepted divergence)."""
    return torch.where(v <= 0, torch.zeros_like(v), v)


def leaky(v, slope):
    return torch.where(v > 0, v, v * slope)


def prelu(v, alpha):
    return torch.where(v > 0, v, v * alpha)


def gelu(v):
    """The kernels' formula; at +inf it gives +inf where torch-CPU gives nan (accepted: only non-finiteness is pinned there)."""
    return 0.5 * v * (1.0 + torch.erf(v * 0.70710678118654752440))


def relu_bwd(a, g):
    """ReLU backward from the SAVED OUTPUT a (torch's threshold_backward): a zero activation stops any gradient, a NaN
    activation lets it through."""
    return torch.where(a <= 0, torch.zeros_like(g), g)


def leaky_bwd(a, g, slope):
    """torch's leaky_relu_backward; slope == 0 is the ReLU rule above (a select, not a product with zero)."""
    if slope == 0:
        return relu_bwd(a, g)
    return torch.where(a > 0, g, g * slope)


def prelu_bwd(x, g, alpha):
    """(dx, the per-element terms whose column sums are dalpha) of torch's PReLU backward."""
    return torch.where(x > 0, g, alpha * g), torch.where(x > 0, torch.zeros_like(g), x * g)


def maxpool2x2(x_nhwc):
    """2x2 / stride 2 max over NHWC that returns NaN when any of the four inputs is NaN."""
    n, h, w, c = x_nhwc.shape
    t = x_nhwc[:, :h // 2 * 2, :w // 2 * 2].reshape(n, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, c, 4)
    clean = torch.nan_to_num(t, nan=-INF, posinf=INF, neginf=-INF).amax(-1)
    return torch.where(torch.isnan(t).any(-1), torch.full_like(clean, NAN), clean)


def round_bf16(v):
    """float32 -> bfloat16 values (as float32), round-to-nearest-even on the bit pattern; NaN stays NaN."""
    bits = v.float().contiguous().view(torch.int32).to(torch.int64) & 0xffffffff
    rounded = ((bits + 0x7fff + ((bits >> 16) & 1)) & 0xffff0000)
    out = torch.where(rounded >= 2 ** 31, rounded - 2 ** 32, rounded).to(torch.int32).view(torch.float32)
    return torch.where(torch.isnan(v), torch.full_like(out, NAN), out)


def round_f16(v):
    """float32 -> IEEE half values (as float32) through numpy's conversion (round-to-nearest-even, overflow to inf)."""
    with np.errstate(over="ignore"):
        return torch.from_numpy(v.float().numpy().astype(np.float16).astype(np.float32))


def round_to(v, dtype):
    return round_bf16(v) if dtype == torch.bfloat16 else round_f16(v)


def split_bf16(v):
    """(hi, lo) of the bf16x3 split: hi = bf16(v), lo = bf16(v - hi).  split(inf) = (inf, nan): why bf16x3 turns Inf into NaN."""
    hi = round_bf16(v)
    return hi, round_bf16(v.float() - hi)


def ties(dtype):
    """Values exactly halfway between two neighbours of ``dtype`` (both parities of the kept bit, both signs, several
    exponents), the case a random draw never hits; plus the halfway points next to the overflow threshold."""
    half = 2.0 ** (-8 if dtype == torch.bfloat16 else -11)
    m = torch.tensor([1.0 + (2 * k + 1) * half for k in range(8)], dtype=torch.float64)
    e = torch.tensor([2.0 ** p for p in (-14, -3, 0, 5, 14)], dtype=torch.float64)
    v = (m[:, None] * e[None, :]).reshape(-1)
    top = 2.0 ** 127 if dtype == torch.bfloat16 else 2.0 ** 15
    v = torch.cat([v, torch.tensor([top * (2.0 - half), top * (2.0 - 3 * half)], dtype=torch.float64)])
    v = torch.cat([v, -v]).float()
    return v[: v.numel() // 4 * 4]


# ---------------------------------------------------------------------------------------------- conv cases
# path: "fp32" (ops.conv2d), "stem" (ops.stem_conv), "b3" (ops.conv2d_b3), "n16" (ops.conv2d_n16, run in bf16 and fp16).
# tile as passed (0 = the picker).  The conv is k x k, pad k // 2, on [n, h, w, cin]; s2d: the kernel reads the input
# space-to-depth (a 3x3 / stride 2 conv).
ConvCase = namedtuple("ConvCase", "name path tile n cin cout h w k stride s2d")


def conv_case(path, tile, n, cin, cout, h, w, k=3, stride=1, s2d=False):
    name = f"{path}_t{tile}_n{n}_{cin}to{cout}_{h}x{w}_k{k}s{stride}" + ("_s2d" if s2d else "")
    return ConvCase(name, path, tile, n, cin, cout, h, w, k, stride, s2d)


FP32_TILES = [0, 1, 2, 4, 5]
_FP32_GEO = [(3, 8, 12, 5, 7, 3, 1), (3, 8, 12, 5, 7, 3, 2), (3, 8, 12, 5, 7, 1, 2),     # element-wise gather (Cin % 32 != 0)
             (3, 32, 36, 7, 7, 3, 1)]                                                    # vector loads; M = 147 spans three images
FP32 = [conv_case("fp32", t, *g) for g in _FP32_GEO for t in FP32_TILES]
STEM = [conv_case("stem", 0, 3, 3, 64, 7, 13)]

_FLAT = (3, 64, 96, 7, 7)
_WINDOW = [(7, 64, 64, 5, 5), (50, 64, 64, 2, 2), (5, 128, 200, 14, 14), (3, 64, 128, 13, 21)]
_PATCH = [(3, 64, 64, 32, 32), (3, 128, 128, 16, 16), (3, 64, 100, 32, 32)]

B3 = ([conv_case("b3", t, *_FLAT) for t in (0, 41, 42, 45)] +
      [conv_case("b3", t, 3, 64, 128, 7, 7) for t in (44,)] + [conv_case("b3", 48, 3, 64, 64, 7, 7)] +
      [conv_case("b3", t, 5, 64, 128, 9, 9, 3, 2) for t in (41, 44)] + [conv_case("b3", t, 4, 64, 128, 9, 9, 1, 2) for t in (41, 44)] +
      [conv_case("b3", 48, 5, 64, 64, 9, 9, 3, 2), conv_case("b3", 48, 4, 64, 64, 9, 9, 1, 2)] +
      [conv_case("b3", t, *g) for t in (53, 56) for g in _WINDOW] +
      [conv_case("b3", t, *g) for t in (59, 58) for g in _PATCH] +
      [conv_case("b3", t, *g, 3, 2, True) for t in (51, 52) for g in ((9, 64, 64, 2, 2), (5, 128, 256, 6, 2), (3, 64, 64, 16, 16))])

N16 = ([conv_case("n16", t, *_FLAT) for t in (0, 63, 64, 65, 66, 67, 91, 94)] +
       [conv_case("n16", t, 5, 64, 128, 9, 9, 3, 2) for t in (64, 67, 91, 94)] +
       [conv_case("n16", t, 4, 64, 128, 9, 9, 1, 2) for t in (64, 67, 91, 94)] +
       [conv_case("n16", t, 5, 64, 64, 9, 9, 3, 2) for t in (63, 65, 66)] + [conv_case("n16", t, 4, 64, 64, 9, 9, 1, 2) for t in (63, 65, 66)] +
       [conv_case("n16", t, *g) for t in (73, 76, 77) for g in _WINDOW if not (t == 77 and g[1] != 64)] +      # 77: Cin == 64
       [conv_case("n16", t, *g) for t in (71, 72, 78) for g in _PATCH if not (t == 71 and g[1] != 64)] +       # 71: Cin == 64
       [conv_case("n16", 79, 3, 64, 64, 48, 48), conv_case("n16", 79, 7, 64, 64, 16, 16)] +
       [conv_case("n16", t, *g, 3, 2, True) for t in (81, 82) for g in ((9, 128, 64, 2, 2), (5, 128, 256, 6, 2), (3, 128, 64, 16, 16))])

CONV_CASES = FP32 + STEM + B3 + N16
POISON_VALUES = (("nan", NAN), ("inf", INF))
CHUNK = {"fp32": 0, "stem": 0, "b3": 32, "n16": 64}     # channels per K step: poison (c) sits on a chunk boundary


def out_hw(case):
    p = case.k // 2
    return (case.h + 2 * p - case.k) // case.stride + 1, (case.w + 2 * p - case.k) // case.stride + 1


def poisons(case):
    """[(label, (image, row, column, channel))]: (a) the last pixel of image 0 on the last channel, (b) pixel (0, 0) of image 1
    on channel 0, (c) a centre pixel of the last image on a chunk boundary (its last channel for odd tiles, the next chunk's
    first for even ones, where Cin has a next chunk)."""
    chunk = CHUNK[case.path]
    ch = min(case.cin - 1, chunk - 1 + (1 - case.tile % 2)) if chunk else case.cin // 2
    cy, cx = case.h // 2 // case.stride * case.stride, case.w // 2 // case.stride * case.stride   # a pixel a strided 1x1 reads
    return [("a", (0, case.h - 1, case.w - 1, case.cin - 1)), ("b", (1, 0, 0, 0)), ("c", (case.n - 1, cy, cx, ch))]


def _seed(name):
    return sum((i + 1) * b for i, b in enumerate(name.encode())) % (2 ** 31)


def weights_survive_rounding(w):
    return bool((w.bfloat16() != 0).all() and (w.half() != 0).all())


@functools.lru_cache(maxsize=None)
def _make(n, cin, cout, h, w, k):
    seed = _seed(f"{n}_{cin}_{cout}_{h}_{w}_{k}")
    for attempt in range(64):                     # the first seed whose weights are all non-zero in bf16 and in fp16
        g = torch.Generator().manual_seed(seed + attempt)
        x = torch.randn(n, h, w, cin, generator=g)
        wt = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
        if weights_survive_rounding(wt):
            return x, wt
    raise AssertionError("no seed with non-zero rounded weights")


def make_conv(case, dtype=None):
    """(x NHWC, w OIHW) of a case as float32 CPU tensors, standard-normal x and w / sqrt(K), rounded to ``dtype`` for the narrow
    path (so the kernel and the reference see the same operands).  Shared by every case of the same geometry; do not modify."""
    x, w = _make(case.n, case.cin, case.cout, case.h, case.w, case.k)
    if dtype is not None:
        x, w = round_to(x, dtype), round_to(w, dtype)
    return x, w


def poisoned(x, where, value):
    x = x.clone()
    x[where] = value
    return x


def geometric_mask(case, where):
    """[n, ho, wo] bool: the outputs whose receptive field contains input pixel ``where`` = (image, row, column, channel)."""
    b, y, xx, _ = where
    ho, wo = out_hw(case)
    p = case.k // 2
    i = torch.arange(ho)[:, None] * case.stride - p
    j = torch.arange(wo)[None, :] * case.stride - p
    m = torch.zeros(case.n, ho, wo, dtype=torch.bool)
    m[b] = (i <= y) & (y < i + case.k) & (j <= xx) & (xx < j + case.k)
    return m


def geometric_value(case, w, where, value):
    """[n, ho, wo, cout] float64: NaN for a NaN poison, +-inf by the sign of the weight of the tap that reaches ``where`` for
    an Inf poison, 0 outside the mask."""
    b, y, xx, ch = where
    ho, wo = out_hw(case)
    p = case.k // 2
    out = torch.zeros(case.n, ho, wo, case.cout, dtype=torch.float64)
    for i in range(ho):
        for j in range(wo):
            r, q = y - (i * case.stride - p), xx - (j * case.stride - p)
            if 0 <= r < case.k and 0 <= q < case.k:
                out[b, i, j] = NAN if math.isnan(value) else torch.sign(w[:, ch, r, q].double()) * value
    return out


def conv_f64(case, x, w):
    """The float64 ``F.conv2d`` of a case, NHWC."""
    return F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), None, case.stride, case.k // 2).permute(0, 2, 3, 1).contiguous()


Poisoned = namedtuple("Poisoned", "x geo_mask ref ref_mask geo_value")


@functools.lru_cache(maxsize=None)
def _poison_reference(case_geo, dtype, where, value_name):
    case = ConvCase("", "", 0, *case_geo)
    value = dict(POISON_VALUES)[value_name]
    x, w = make_conv(case, dtype)
    xp = poisoned(x, where, value)
    ref = conv_f64(case, xp, w)
    bad = ~torch.isfinite(ref)
    return Poisoned(xp, geometric_mask(case, where), ref, bad, geometric_value(case, w, where, value))


def poison_reference(case, where, value_name, dtype=None):
    """For one poison of a case: the poisoned input, the mask [n, ho, wo] from the geometry, the float64 conv of the poisoned
    input [n, ho, wo, cout] with its non-finite mask, and the geometric statement of the non-finite values.  Cached per
    geometry; do not modify what it returns."""
    return _poison_reference(tuple(case[3:]), dtype, tuple(where), value_name)


@functools.lru_cache(maxsize=None)
def _clean_reference(case_geo, dtype):
    case = ConvCase("", "", 0, *case_geo)
    return conv_f64(case, *make_conv(case, dtype))


def clean_reference(case, dtype=None):
    return _clean_reference(tuple(case[3:]), dtype)


def check_poisoned(got, clean, mask, expected, value_name, exact, tag):
    """The assertions of one poisoned launch.  ``got`` / ``clean``: {name: CPU tensor [n, ho, wo, cout]} of the poisoned and the
    clean launch; ``mask`` / ``expected``: the reference's non-finite mask and values.  Every output tensor: its non-finite set
    is the mask; a NaN poison gives NaN; the outputs named in ``exact`` carry the reference's non-finite values; everything
    outside the mask is bit-identical to the clean launch."""
    for name, t in got.items():
        bad = ~torch.isfinite(t)
        assert torch.equal(bad, mask), (f"{tag} [{name}]: {int((bad & ~mask).sum())} outputs outside the receptive field are "
                                        f"non-finite, {int((mask & ~bad).sum())} inside it are finite")
        if value_name == "nan":
            assert torch.isnan(t[mask]).all(), f"{tag} [{name}]: a NaN input must give NaN"
        elif name in exact:
            assert nan_equal(t[mask], expected[mask], ignore_zero_sign=True), \
                f"{tag} [{name}] value: {describe_mismatch(t[mask], expected[mask])}"
        assert torch.equal(t[~mask], clean[name][~mask]), \
            f"{tag} [{name}] outside the receptive field vs the clean launch: {describe_mismatch(t[~mask], clean[name][~mask])}"


def flat_conv(case, x, w, border):
    """A 3x3 / stride 1 / pad 1 conv written as the window kernels walk it: over the flat [n h w, cin] pixel array, tap by tap,
    where a tap outside the image lands on a pixel of the neighbouring row or IMAGE.  ``border`` = "select": that value is
    selected away (correct); "zero_factor": it is multiplied by 0 -- equal on finite data, and the kind of kernel the poison
    test exists to catch.  float64, NHWC."""
    assert case.k == 3 and case.stride == 1 and border in ("select", "zero_factor")
    n, h, wd, cin = x.shape
    xf = x.double().reshape(n * h * wd, cin)
    pix = torch.arange(n * h * wd)
    row, col = (pix // wd) % h, pix % wd
    out = torch.zeros(n * h * wd, case.cout, dtype=torch.float64)
    for r in range(3):
        for q in range(3):
            inside = (row + r - 1 >= 0) & (row + r - 1 < h) & (col + q - 1 >= 0) & (col + q - 1 < wd)
            src = (pix + (r - 1) * wd + (q - 1)).clamp(0, n * h * wd - 1)
            tap = xf[src]
            if border == "select":
                tap = torch.where(inside[:, None], tap, torch.zeros_like(tap))
            else:
                tap = tap * inside[:, None].double()
            out += tap @ w[:, :, r, q].double().t()
    return out.reshape(n, h, wd, case.cout)
