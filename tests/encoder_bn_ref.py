"""A float64 restatement of ``csrc/encoder_bn.hip`` (the train-mode BatchNorm passes of the IR-50) and the data of its edge tests.

Nothing here needs a GPU or the package: ``tests/test_encoder_bn_ref_cpu.py`` proves the restatement against torch on any machine,
``tests/test_encoder_bn_edges_gpu.py`` holds the kernels to it.

  bn_apply      out = mask * prelu(y * scale + shift) + (res[:, ::s, ::s][:, :Ho, :Wo] * rs + rt), NHWC, per-channel vectors;
                stats[tile] = (sum, sum of squares) of ``out`` over the tile's pixel rows (``rows_per_block`` / ``tiles``)
  bn_finalize   [tiles, 2, C] fp32 partial sums over ``count`` elements -> scale = gamma / sqrt(var + eps), shift = beta - mean scale
                and torch's running-buffer update (biased variance clamped at 0; unbiased for the buffer where count > 1)
  fold_bn_3x3   w' = w * s[cin]; bias9[3 ry + rx][o] = sum of w . t over the taps a 3x3 / pad 1 conv has INSIDE the image at an
                output pixel on the first / an inner / the last row (ry = 0 / 1 / 2) and column (rx)

Two kinds of data:

* EXACT (``exact_inputs``).  y and res are integers in [-3, 3], scale and rs in {0.5, 1, 2}, shift and rt multiples of 0.5 in
  [-1, 1], alpha in {0.25, 0.5}, mask in {0, 2}.  Every value that occurs in the kernel -- y scale, + shift, the PReLU product,
  the mask product, res rs, + rt, the sum -- is a multiple of GRANULE = 1/8 of magnitude at most 2 (3 * 2 + 1) + (3 * 2 + 1) = 21,
  so each is a float32 number however the compiler contracts the multiply-adds, and, being m / 8 with |m| <= 168 < 2^8, also a
  bfloat16 and a float16 number (the ``lo`` plane of a split is zero).  The per-tile statistics are sums of multiples of 1/8 and
  of 1/64: they are exact in float32, in ANY order of summation, when sum |out| / GRANULE and sum out^2 / GRANULE^2 over the tile
  stay below 2^24.  ``exact_margin`` returns the larger of the two for a given tile height; it is a condition on the drawn data
  (the worst case 21^2 * 64 * 2048 would not meet it), asserted by every test that compares with ``torch.equal`` and checked on
  the CPU for a full 2048-row tile.  The kernel then owes the float64 reference BIT FOR BIT.

* RANDOM.  Standard-normal data against ``apply_ref``'s bound: the kernel makes seven roundings, each at most U = 2^-24 of a
  magnitude that |mask| (|y| |scale| + |shift|) + |res| |rs| + |rt| bounds; 8 of them, plus the smallest denormal.
"""
import torch

import nonfinite_ref as nf
from conv_ref import pick, tile_rows

U = 2.0 ** -24
GRANULE = 0.125
EXACT_LIMIT = 2.0 ** 24

Y_VALUES = [-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0]
SCALE_VALUES = [0.5, 1.0, 2.0]
SHIFT_VALUES = [-1.0, -0.5, 0.0, 0.5, 1.0]
ALPHA_VALUES = [0.25, 0.5]
MASK_VALUES = [0.0, 2.0, 2.0]
MAX_EXACT = 2.0 * (3.0 * 2.0 + 1.0) + (3.0 * 2.0 + 1.0)


# ---------------------------------------------------------------------------------------------- bn_apply
def bn_apply_ref(y, res, scale, shift, alpha, rs, rt, mask):
    """(the float64 restatement rounded once to float32, the float32 error bound of its finite values): the kernel makes seven
    roundings (y * scale + shift, the PReLU product, the mask product, res * rs + rt, the sum), each at most 2^-24 of a
    magnitude that |mask| (|y| |scale| + |shift|) + |res| |rs| + |rt| bounds; 8 of them, plus the smallest denormal."""
    v = y.double() * scale.double() + shift.double()
    v = nf.prelu(v, alpha.double()) * mask.double()
    mag = mask.double().abs() * (y.double().abs() * scale.double() + shift.double().abs()) + res.double().abs() * rs.double() + rt.double().abs()
    return (v + (res.double() * rs.double() + rt.double())).float(), 8 * 2.0 ** -24 * mag + 2.0 ** -149


def crop_residual(res, stride, ho, wo):
    """The residual pixels ``bn_apply`` adds: every ``stride``-th row and column, cut to the output grid."""
    return res[:, ::stride, ::stride][:, :ho, :wo]


def apply_ref(y, scale, shift, alpha=None, mask=None, res=None, res_stride=1, res_scale=None, res_shift=None):
    """(out, bound) in float64: the contract of ``ops.bn_apply_nhwc`` with every optional part left out when None, and the
    magnitude and bound of ``bn_apply_ref`` (8 roundings x 2^-24 x magnitude, + 2^-149) for the same parts."""
    d = (lambda t: None if t is None else t.detach().double())
    y, scale, shift, alpha, mask, res, res_scale, res_shift = (d(t) for t in (y, scale, shift, alpha, mask, res, res_scale, res_shift))
    v = y * scale + shift
    mag = y.abs() * scale.abs() + shift.abs()
    if alpha is not None:
        v = torch.where(v > 0, v, v * alpha)
    if mask is not None:
        v = v * mask.reshape(v.shape)
        mag = mag * mask.reshape(v.shape).abs()
    if res is not None:
        r = crop_residual(res, res_stride, y.shape[1], y.shape[2])
        assert r.shape == y.shape, f"residual {tuple(res.shape)} at stride {res_stride} does not cover {tuple(y.shape)}"
        if res_scale is not None:
            v, mag = v + (r * res_scale + res_shift), mag + r.abs() * res_scale.abs() + res_shift.abs()
        else:
            v, mag = v + r, mag + r.abs()
    return v, 8 * U * mag + 2.0 ** -149


def rows_per_block(p):
    """Pixel rows per statistics tile of ``bn_apply``: about 2048 blocks, 128 .. 2048 rows each, in multiples of 128."""
    r = (p // 2048 + 127) // 128 * 128
    return min(max(r, 128), 2048)


def tiles(p):
    return 0 if p <= 0 else -(-p // rows_per_block(p))


def rows_per_pass(c, per_thread):
    """Rows one 256-thread block covers per pass: ``per_thread`` = 4 channels (fp32, bf16x3 kernels) or 8 (narrow kernel)."""
    return 256 // (c // per_thread)


def exact_margin(out, bm):
    """The precondition of an exact comparison for the float64 result ``out`` of an EXACT draw and tiles of ``bm`` rows: every
    value is a multiple of GRANULE and a bfloat16 number (inf otherwise), and the return value -- the largest per-tile column
    sum of |out| and of out^2 in units of the granule -- must stay below 2^24 (EXACT_LIMIT)."""
    m = out / GRANULE
    if not (torch.equal(m, m.round()) and m.abs().max().item() < 256.0):
        return float("inf")
    return max(tile_rows(m.abs(), bm)[:, 0].max().item(), tile_rows(m, bm)[:, 1].max().item())


def exact_inputs(g, n, ho, wo, c, res_hw=None):
    """The operands of an EXACT case as float32 CPU tensors: y, scale, shift, alpha, mask, res ([n, *res_hw, c]; the output's
    grid by default), rs, rt."""
    hr, wr = res_hw if res_hw is not None else (ho, wo)
    d = {"y": pick(g, (n, ho, wo, c), Y_VALUES), "scale": pick(g, (c,), SCALE_VALUES), "shift": pick(g, (c,), SHIFT_VALUES),
         "alpha": pick(g, (c,), ALPHA_VALUES), "mask": pick(g, (n, ho, wo, c), MASK_VALUES),
         "res": pick(g, (n, hr, wr, c), Y_VALUES), "rs": pick(g, (c,), SCALE_VALUES), "rt": pick(g, (c,), SHIFT_VALUES)}
    return d


def factor_rows(p):
    """(N, Ho, Wo) with N Ho Wo == p, N > 1 and Ho != Wo wherever p allows."""
    for n in range(2, p):
        for ho in range(2, p):
            if n * ho * ho >= p:
                break
            if p % (n * ho) == 0:
                return n, ho, p // (n * ho)
    for n in range(2, p):
        if p % n == 0:
            return n, 1, p // n
    return 1, 1, p


# ---------------------------------------------------------------------------------------------- bn_finalize
def f32(v):
    """A Python float as the kernel receives it through a ``float`` argument."""
    return float(torch.tensor(v, dtype=torch.float32))


def finalize_ref(partials_f32, count, gamma, beta, rm=None, rv=None, momentum=0.1, eps=1e-5):
    """The float64 batch-norm formula from THE SAME fp32 partial sums [tiles, 2, C]: a dict with 'sums' [2, C], 'mean', 'var'
    (biased, clamped at 0), 'unbiased' (var count / (count - 1) for count > 1, else var), 'scale', 'shift' and, with running
    buffers, 'rm' / 'rv' after torch's update.  ``momentum`` and ``eps`` are rounded to float32 first, as the kernel gets them."""
    assert partials_f32.dtype == torch.float32 and partials_f32.dim() == 3 and partials_f32.shape[1] == 2
    momentum, eps, count = f32(momentum), f32(eps), float(count)
    sums = partials_f32.double().sum(0)
    mean = sums[0] / count
    var = (sums[1] / count - mean * mean).clamp_min(0.0)
    unbiased = var * count / (count - 1.0) if count > 1.0 else var
    scale = gamma.double() / torch.sqrt(var + eps)
    out = {"sums": sums, "mean": mean, "var": var, "unbiased": unbiased, "scale": scale, "shift": beta.double() - mean * scale}
    if rm is not None:
        out["rm"] = (1.0 - momentum) * rm.double() + momentum * mean
        out["rv"] = (1.0 - momentum) * rv.double() + momentum * unbiased
    return out


# ---------------------------------------------------------------------------------------------- fold_bn_3x3
def kpad_3x3(cin):
    """The packed K of a 3x3 weight: 9 Cin rounded up to the 32-wide K step of the conv kernels."""
    return (9 * cin + 31) // 32 * 32


def pack_3x3(w_oihw, fill=0.0):
    """[Cout, Cin, 3, 3] -> the packed [Cout, Kpad] with k = (kh * 3 + kw) * Cin + c, the padding columns holding ``fill``."""
    cout, cin = w_oihw.shape[:2]
    out = torch.full((cout, kpad_3x3(cin)), fill, dtype=w_oihw.dtype)
    out[:, :9 * cin] = w_oihw.permute(0, 2, 3, 1).reshape(cout, 9 * cin)
    return out


def fold_ref(w_oihw, s, t):
    """(w * s[cin] as [Cout, Cin, 3, 3], bias9 [9, Cout]) in float64; bias9[3 ry + rx][o] sums B[o][kh][kw] = sum_c w t[c] over
    kh in [ry == 0, 2 - (ry == 2)] and kw likewise: the taps that lie inside the image."""
    w, s, t = w_oihw.double(), s.double(), t.double()
    b = (w * t[None, :, None, None]).sum(1)                                # [Cout, 3, 3]
    bias9 = torch.zeros(9, w.shape[0], dtype=torch.float64)
    for ry in range(3):
        for rx in range(3):
            rows = range(1 if ry == 0 else 0, 2 if ry == 2 else 3)
            cols = range(1 if rx == 0 else 0, 2 if rx == 2 else 3)
            for kh in rows:
                for kw in cols:
                    bias9[3 * ry + rx] += b[:, kh, kw]
    return w * s[None, :, None, None], bias9
