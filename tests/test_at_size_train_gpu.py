"""Correctness of the encoder TRAINING kernels at the size bench.py --release 4 --hw 224 --batch 32 times (BASELINE cfg2):
N = 1024 frames of 224x224, R = 51.4 M pixel rows per stage-1 layer -- 3.3 G elements, 13.2 GB per fp32 tensor, where the
row BatchNorm takes its one-pass shifted statistics with ~50 k rows per slab, ``_prelu_bwd_chunked`` really chunks, and
the weight-gradient split chooser, the large-M conv tiles and the stride-2 data gradient get dispatches no small test makes.

A float64 oracle of a whole 1024-frame step is out of reach, so every stage is checked on the operands the kernel itself
saw: the released unit (or stem) runs through its autograd Function in the "raw" memory plan (z1 / z2 / statistics come
from ``grad_fn.saved_tensors``), the test restates the Function's backward op by op -- its gradients must be BIT-IDENTICAL
to the Function's, so the checked sequence is the shipped one -- and each stage's result is compared with a float64
computation on that stage's own inputs (Split tensors count as hi + lo, narrow planes as their exact value):

* elementwise / conv outputs at >= 256 sampled positions (the last frame's corners and border rows, frame 0, random pixels
  of the last 64 frames; all channels);
* per-channel reductions over all R rows in float64, frame chunk by frame chunk on the device;
* weight gradients at a grid of (co, ci) entries that includes index 0 and the last index, for every tap.

Bounds are worst-case: eps_op * sum |a||b| plus n * 2^-24 * sum |terms| with n the depth of the kernel's own fp32
accumulation (rows per slab / split plus the slab / split count -- not R).  Integer-valued cases check the reductions
EXACTLY, which catches a dropped, duplicated or misrouted row, slab, split or chunk that a relative bound can hide.
"""
import gc
import math
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

N = 1024
HW = 224
U = 2.0 ** -24          # fp32 unit roundoff
# hi + lo of a Split tensor against the fp32 value v it was made from: |v - hi| <= 2^-8 |v|, lo = bf16(v - hi) -> 2^-16 |v|
SPLIT = 2.0 ** -16
# one bf16x3 product a * b ~ a_hi b_hi + a_hi b_lo + a_lo b_hi: the two operands' split errors (2^-16 each) and the
# dropped a_lo b_lo (2^-16)
B3 = 3 * 2.0 ** -16
_cache = {}


# ------------------------------------------------------------------------------------------------ plumbing
def _ops():
    from feature_vs_text_compound_emotion_amd import ops
    return ops


def _state():
    if "sd" not in _cache:
        from feature_vs_text_compound_emotion_amd import synth
        _cache["sd"] = synth.make_state_dict(synth.visual_backbone_spec("", HW // 8), seed=11)
    return _cache["sd"]


def _load(mod, prefix):
    sd = {k[len(prefix):]: v for k, v in _state().items() if k.startswith(prefix)}
    mod.load_state_dict(sd, strict=True)
    return mod.cuda()


def _unit(i):
    from feature_vs_text_compound_emotion_amd.synth import ir50_units
    from feature_vs_text_compound_emotion_amd.visual_backbone import _Unit
    return _load(_Unit(*ir50_units()[i]), f"backbone.body.{i}.")


def _stem():
    from torch import nn
    return _load(nn.Sequential(nn.Conv2d(3, 64, 3, 1, 1, bias=False), nn.BatchNorm2d(64), nn.PReLU(64)), "backbone.input_layer.")


def _val(t):
    """float64 value of a kernel operand / result: Split = hi + lo, narrow = its exact value."""
    if isinstance(t, _ops().Split):
        return t.hi.double() + t.lo.double()
    return t.double()


def _sl(t, a, b):
    return _ops().Split(t.hi[a:b], t.lo[a:b]) if isinstance(t, _ops().Split) else t[a:b]


def _chunk(t):
    """frames per float64 chunk: at most 2^28 values (2 GB)"""
    per = (t.hi if isinstance(t, _ops().Split) else t)[0].numel()
    return max(1, (1 << 28) // max(1, per))


def _report(tag, worst):
    print(f"\n[at size train] {tag}: worst error / bound {worst:.3f}")
    assert worst < 1.0, f"{tag}: worst error / bound {worst:.3f}"


def _ratio(got, ref, bound):
    return ((got - ref).abs() / bound.clamp_min(1e-300)).max().item()


def _points(n, h, w, seed):
    """[P, 3] (frame, row, col): the last frame's four corners and border rows / columns, frame 0's corner, random pixels of
    the last 64 frames (highest addresses) -- 256 + 24 positions."""
    pts = [(n - 1, 0, 0), (n - 1, 0, w - 1), (n - 1, h - 1, 0), (n - 1, h - 1, w - 1), (0, 0, 0), (n // 2, h // 2, w - 1)]
    for i in range(6):
        j = (i * 37) % w
        pts += [(n - 1, 0, j), (n - 1, h - 1, j), (n - 1, j % h, 0), (n - 1, j % h, w - 1)]
    pts = torch.tensor(pts[:30], dtype=torch.long)
    g = torch.Generator().manual_seed(seed)
    rnd = torch.stack([torch.randint(max(0, n - 64), n, (250,), generator=g), torch.randint(0, h, (250,), generator=g),
                       torch.randint(0, w, (250,), generator=g)], 1)
    return torch.cat([pts, rnd]).cuda()


def _gather(t, n_, y_, x_):
    """float64 [P, C] of t[n, y, x, :] (zeros where (y, x) falls outside the image)."""
    hh, ww = t.shape[1], t.shape[2]
    ok = ((y_ >= 0) & (y_ < hh) & (x_ >= 0) & (x_ < ww)).double().unsqueeze(1)
    yc, xc = y_.clamp(0, hh - 1), x_.clamp(0, ww - 1)
    if isinstance(t, _ops().Split):
        v = t.hi[n_, yc, xc].double() + t.lo[n_, yc, xc].double()
    else:
        v = t[n_, yc, xc].double()
    return v * ok


def _conv_at(x, w, pts, stride, pad):
    """float64 conv output y[n, oy, ox, :] = sum_taps x[n, oy*s + kh - pad, ox*s + kw - pad, :] . w[:, :, kh, kw], and
    the same sum over |x| |w|."""
    w = w.double()
    ref = mag = 0.0
    for kh in range(w.shape[2]):
        for kw in range(w.shape[3]):
            p = _gather(x, pts[:, 0], pts[:, 1] * stride + kh - pad, pts[:, 2] * stride + kw - pad)
            wt = w[:, :, kh, kw]
            ref = ref + p @ wt.t()
            mag = mag + p.abs() @ wt.abs().t()
    return ref, mag


def _dgrad_at(dz, w, pts, stride, pad):
    """float64 data gradient dx[n, iy, ix, :] = sum over (o, tap) with o*s + k - pad = i of dz[n, o, :] . w[:, :, kh, kw]."""
    w = w.double()
    ref = mag = 0.0
    for kh in range(w.shape[2]):
        for kw in range(w.shape[3]):
            ty, tx = pts[:, 1] + pad - kh, pts[:, 2] + pad - kw
            ok = ((ty % stride) == 0) & ((tx % stride) == 0)
            oy = torch.where(ok, ty // stride, torch.full_like(ty, -1))
            p = _gather(dz, pts[:, 0], oy, tx // stride)
            wt = w[:, :, kh, kw]
            ref = ref + p @ wt
            mag = mag + p.abs() @ wt.abs()
    return ref, mag


def _check_conv(tag, got, x, w, pts, stride, pad, depth, eps_prod=B3, dgrad=False):
    """got (the kernel's fp32 / Split output) at pts against float64; bound (eps_prod + (depth + 1) 2^-24) sum |x||w|,
    depth = the kernel's fp32 accumulation depth (3 MFMAs per product for bf16x3)."""
    ref, mag = (_dgrad_at if dgrad else _conv_at)(x, w, pts, stride, pad)
    g = _gather(got, pts[:, 0], pts[:, 1], pts[:, 2])
    out_round = SPLIT if isinstance(got, _ops().Split) else U
    _report(tag, _ratio(g, ref, (eps_prod + (depth + 1) * U + out_round) * mag + 1e-30))


def _colsum_depth(r):
    """fp32 accumulation depth of cer_col_sum / col_sum_pair over r rows: a lane adds every 8th row of its slab, 8 lanes are
    added, then the slab partials the same way (tail_kernels.hip)."""
    rps = 256
    if (r + 255) // 256 > 1024:
        rps = ((r + 1023) // 1024 + 31) // 32 * 32
    slabs = (r + rps - 1) // rps
    return -(-rps // 8) + 8 + (-(-slabs // 8) + 8 if slabs > 1 else 0)


def _colsums64(fn, n, step):
    """(sum, sum |.|) per channel in float64 of fn(a, b) [frames a..b, ..., C] over all n frames."""
    s = sa = 0.0
    for a in range(0, n, step):
        v = fn(a, min(n, a + step))
        v = v.reshape(-1, v.shape[-1])
        s, sa = s + v.sum(0), sa + v.abs().sum(0)
    return s, sa


def _bn_bwd_sums_ref(dy, x, sm, si):
    """float64 (sum dy, sum dy * x_hat, sum |dy|, sum |dy * x_hat|) per channel, x_hat from the saved statistics."""
    n, step = dy.shape[0], _chunk(dy)
    mu, iv = sm.double(), si.double()
    s1, a1 = _colsums64(lambda a, b: _val(_sl(dy, a, b)), n, step)
    s2, a2 = _colsums64(lambda a, b: _val(_sl(dy, a, b)) * (_val(_sl(x, a, b)) - mu) * iv, n, step)
    return s1, s2, a1, a2


def _check_bn_bwd(tag, dy, x, sm, si, w, dg, db, dx, pts, add=None):
    """BatchNorm backward over the rows: dg / db against float64 sums with the col_sum depth; dx at pts against
    w * invstd * (dy - (db + x_hat * dg) / R) [+ add] in float64 on the kernel's own sums, bound 16 u times the same
    expression in absolute values (+ u for the add, + 2^-16 for a Split result)."""
    r = dy[0].numel() // dy.shape[-1] * dy.shape[0]
    s1, s2, a1, a2 = _bn_bwd_sums_ref(dy, x, sm, si)
    d = _colsum_depth(r) + 3
    _report(f"{tag} db", _ratio(db.double(), s1, d * U * a1 + 1e-30))
    _report(f"{tag} dg", _ratio(dg.double(), s2, d * U * a2 + 1e-30))
    g = _gather(dy, pts[:, 0], pts[:, 1], pts[:, 2])
    v = _gather(x, pts[:, 0], pts[:, 1], pts[:, 2])
    xh = (v - sm.double()) * si.double()
    k = (w.double() * si.double())
    ref = k * (g - (db.double() + xh * dg.double()) / r)
    mag = k.abs() * (g.abs() + (db.double().abs() + xh.abs() * dg.double().abs()) / r)
    bound = 16 * U * mag      # about a dozen fp32 roundings in the kernel's expression, fl(1 / R) included
    if add is not None:
        av = _gather(add, pts[:, 0], pts[:, 1], pts[:, 2])
        ref, bound = ref + av, bound + 2 * U * (ref.abs() + av.abs())
    got = _gather(dx, pts[:, 0], pts[:, 1], pts[:, 2])
    if isinstance(dx, _ops().Split):
        bound = bound + SPLIT * ref.abs()
    _report(f"{tag} dx", _ratio(got, ref, bound + 1e-30))


def _check_bn_stats(tag, x2d_fn, n, step, r, sm, si, rm0=None, rv0=None, rm=None, rv=None, shift=None, eps=1e-5, mom=0.1):
    """save_mean / save_invstd of the one-pass shifted statistics (s1 = sum (x - k), s2 = sum (x - k)^2 in fp32, k = the
    first row) against the float64 two-pass result.  With D = the column-sum depth + 2:
        |d mean| <= D u sum |x - k| / R + u |mean|
        |d var|  <= D u (sum (x - k)^2 + 2 |mean - k| sum |x - k|) / R        (+ u var)
        |d invstd| / invstd <= |d var| / 2 (var + eps) + 4 u                      (rsqrtf)
    and the running buffers against their torch update from the float64 statistics."""
    mean, _ = _colsums64(x2d_fn, n, step)
    mean = mean / r
    ssd, _ = _colsums64(lambda a, b: (x2d_fn(a, b) - mean) ** 2, n, step)
    var = ssd / r
    k = shift.double()
    s1a, _ = _colsums64(lambda a, b: (x2d_fn(a, b) - k).abs(), n, step)
    d = _colsum_depth(r) + 2
    b_mean = d * U * s1a / r + U * mean.abs()
    b_var = d * U * (ssd + r * (mean - k) ** 2 + 2 * (mean - k).abs() * s1a) / r + U * var
    invstd = 1.0 / torch.sqrt(var + eps)
    b_inv = invstd * (b_var / (2 * (var + eps)) + 4 * U)
    _report(f"{tag} save_mean", _ratio(sm.double(), mean, b_mean + 1e-30))
    _report(f"{tag} save_invstd", _ratio(si.double(), invstd, b_inv))
    if rm is not None:
        rm_ref = (1 - mom) * rm0.double() + mom * mean
        rv_ref = (1 - mom) * rv0.double() + mom * var * r / (r - 1)
        _report(f"{tag} running_mean", _ratio(rm.double(), rm_ref, mom * b_mean + 4 * U * rm_ref.abs() + 1e-30))
        _report(f"{tag} running_var", _ratio(rv.double(), rv_ref, mom * b_var * r / (r - 1) + 6 * U * rv_ref.abs() + 1e-30))


def _wgrad_splits(r, tiles, taps, ts):
    """wgrad_b3_splits (csrc/wgrad_b3.hip) restated: the row-split count of the weight-gradient kernel."""
    per, slots = tiles * taps, (256 if ts == 256 else 512)
    best, best_cost = 1, 1e300
    for s in range(1, min((r + 255) // 256, 4096) + 1):
        rows = ((r + s - 1) // s + 31) // 32 * 32
        steps = rows // 32
        if steps < 8 and s > 1:
            break
        rounds = (((s + 7) // 8) * per + slots // 8 - 1) // (slots // 8)
        cost = rounds * (steps + 24) + 0.02 * s
        if cost < best_cost:
            best, best_cost = s, cost
    return best


def _wgrad_depth(n, ho, wo, cout, cin, kh, kw, split_in):
    """(rows per split, splits) of the weight-gradient launch; the restated chooser is cross-checked against the workspace
    size the library reports (splits x Cout x Cin x taps floats for the larger of its two tile choices)."""
    r = n * ho * wo
    lib = _ops()._lib.load()

    def tile(split):
        if split and cout % 256 == 0 and cin % 256 == 0:
            return 256
        return 64 if (cout <= 64 or cin <= 64) else 128
    sp = {t: _wgrad_splits(r, -(-cout // t) * -(-cin // t), kh * kw, t) for t in {tile(False), tile(True)}}
    want = max(s if s > 1 else 0 for s in sp.values()) * cout * cin * kh * kw * 4
    assert lib.cer_conv2d_wgrad_b3_workspace_bytes(n, ho, wo, cout, cin, kh, kw) == want
    ts = tile(split_in)
    s = sp[ts]
    rps = ((r + s - 1) // s + 63) // 64 * 64 if ts == 64 else ((r + s - 1) // s + 31) // 32 * 32
    return rps, s, ts


def _tn(a, b, parts=4096):
    """a^T b for tall float64 a [K, m], b [K, n]: batched over row blocks (one GEMM with K = 10^7 .. 10^8 runs serially)"""
    q = a.shape[0] // parts
    out = torch.bmm(a[:q * parts].reshape(parts, q, -1).transpose(1, 2), b[:q * parts].reshape(parts, q, -1)).sum(0)
    return out + a[q * parts:].t() @ b[q * parts:]


def _wgrad_ref(dz, x, co, ci, kh, kw, stride, pad):
    """float64 dW[co, ci, tap] and sum |dz||x| over all rows, frame chunk by frame chunk."""
    import torch.nn.functional as F
    n, ho, wo = dz.shape[0], dz.shape[1], dz.shape[2]
    ref = torch.zeros(len(co), len(ci), kh, kw, dtype=torch.float64, device="cuda")
    mag = torch.zeros_like(ref)
    step = max(1, _chunk(x) // 2)
    for a in range(0, n, step):
        b = min(n, a + step)
        dzc = _val(_sl(dz, a, b)[..., co] if not isinstance(dz, _ops().Split) else _ops().Split(dz.hi[a:b][..., co], dz.lo[a:b][..., co]))
        xc = _val(_sl(x, a, b)[..., ci] if not isinstance(x, _ops().Split) else _ops().Split(x.hi[a:b][..., ci], x.lo[a:b][..., ci]))
        xp = F.pad(xc, (0, 0, pad, pad + stride, pad, pad + stride))
        dz2, dza = dzc.reshape(-1, len(co)), dzc.abs().reshape(-1, len(co))
        for i in range(kh):
            for j in range(kw):
                xs = xp[:, i:i + (ho - 1) * stride + 1:stride, j:j + (wo - 1) * stride + 1:stride].reshape(-1, len(ci))
                ref[:, :, i, j] += _tn(dz2, xs)
                mag[:, :, i, j] += _tn(dza, xs.abs())
        del dzc, xc, xp, dz2, dza
    return ref, mag


def _idx(c, extra, seed):
    g = torch.Generator().manual_seed(seed)
    return sorted(set([0, c - 1] + torch.randint(0, c, (extra,), generator=g).tolist()))


def _check_wgrad(tag, dw, dz, x, kh, kw, stride, pad):
    """dW at a (co, ci) grid x every tap: bound (2^-15 + (3 rows_per_split + splits + 1) 2^-24) sum |dz||x| (three MFMAs per
    product accumulate into one fp32 register per split; the splits are added in fixed order).  fp32 operands are split by
    the kernel's loader: the 2^-15 covers that."""
    n, ho, wo, cout = dz.shape
    cin = x.shape[-1]
    rps, s, ts = _wgrad_depth(n, ho, wo, cout, cin, kh, kw, isinstance(dz, _ops().Split) or isinstance(x, _ops().Split))
    co, ci = _idx(cout, 6, 1), _idx(cin, 6, 2)
    ref, mag = _wgrad_ref(dz, x, co, ci, kh, kw, stride, pad)
    got = dw[co][:, ci].double()
    print(f"\n[at size train] {tag}: {len(co) * len(ci) * kh * kw} entries, tile {ts}, {s} splits of {rps} rows")
    _report(tag, _ratio(got, ref, (B3 + (3 * rps + s + 1) * U) * mag + 1e-30))


def _begin():
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    return time.time()


def _end(tag, t0):
    torch.cuda.synchronize()
    print(f"\n[at size train] {tag}: peak {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB, {time.time() - t0:.1f} s")
    torch.cuda.empty_cache()


def _randn(shape, seed, scale=1.0, offset=0.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(shape, device="cuda", generator=g)
    if scale != 1.0:
        x.mul_(scale)
    if offset:
        x.add_(offset)
    return x


def _ternary(shape, seed, p_nonzero):
    """values in {-1, 0, 1}: nonzero with probability p_nonzero, signs even"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    u = torch.rand(shape, device="cuda", generator=g)
    out = torch.zeros(shape, device="cuda")
    out[u < p_nonzero / 2] = -1.0
    out[(u >= p_nonzero / 2) & (u < p_nonzero)] = 1.0
    del u
    return out


# ------------------------------------------------------------------------------------------------ BN statistics
def test_bn_row_statistics_at_51m_rows_hostile_channels():
    """ops.bn_rows_stats on [51.4 M, 64] rows (the stage-1 size): the one-pass shifted path through col_sum_pair with ~50 k
    rows per slab.  Channel 0 sits 200 standard deviations from 0 (a shift of 0 would cancel catastrophically in
    E[d^2] - E[d]^2); channel 1's FIRST row -- the shift -- is a 6-sigma outlier; the others have mixed offsets and scales.
    Bounds: see _check_bn_stats."""
    ops = _ops()
    t0 = _begin()
    r, c = N * HW * HW, 64
    sc = torch.linspace(0.5, 2.0, c, device="cuda")
    off = torch.linspace(-3.0, 3.0, c, device="cuda")
    sc[0], off[0], sc[1], off[1] = 1.0, 200.0, 1.0, 0.0
    x = _randn((r, c), 21)
    x.mul_(sc).add_(off)
    x[0, 1] = 6.0
    rm0, rv0 = torch.linspace(-1, 1, c, device="cuda"), torch.linspace(0.5, 1.5, c, device="cuda")
    rm, rv = rm0.clone(), rv0.clone()
    sm, si = ops.bn_rows_stats(x, rm, rv, 1e-5, 0.1)
    per = HW * HW
    _check_bn_stats("bn_rows_stats 51.4M x 64", lambda a, b: x[a * per:b * per].double(), N, 64, r, sm, si, rm0, rv0, rm, rv,
                    shift=x[0])
    del x
    _end("bn statistics", t0)


def test_bn_row_statistics_mean_is_exact_on_integer_data():
    """Integer data in {-1, 0, 1} (25 % nonzero: every fp32 partial sum < 2^24, exact) with a first row of zeros (the shift):
    the shifted sums are exact, so save_mean must be fp32(S / R) of the exact column sum S -- the finishing kernel rounds
    S / R in double, then to float: at most 1 ulp -- and save_invstd is rsqrtf of the exact variance (a few ulp)."""
    ops = _ops()
    t0 = _begin()
    r, c = N * HW * HW, 64
    x = _ternary((r, c), 22, 0.25)
    x[0] = 0.0
    rm, rv = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
    sm, si = ops.bn_rows_stats(x, rm, rv, 1e-5, 0.1)
    per = HW * HW
    s, _ = _colsums64(lambda a, b: x[a * per:b * per].double(), N, 64)
    s2, _ = _colsums64(lambda a, b: x[a * per:b * per].double() ** 2, N, 64)
    want = (s / r).float()
    ulp = (torch.nextafter(want.abs(), torch.full_like(want, math.inf)) - want.abs())
    err = ((sm - want).abs() / ulp).max().item()
    var = s2 / r - (s / r) ** 2
    inv = 1.0 / torch.sqrt(var + 1e-5)
    err_i = ((si.double() - inv).abs() / (inv * U)).max().item()
    print(f"\n[at size train] bn_rows_stats integer data: save_mean max error {err:.1f} ulp, save_invstd {err_i:.1f} u")
    assert err <= 1.0
    assert err_i <= 8.0
    del x
    _end("bn statistics exact", t0)


# ------------------------------------------------------------------------------------------------ exact reductions
@pytest.mark.parametrize("case", ["64x64_224_split", "stem_4ch_224_fp32", "512x512_28_split"])
def test_weight_gradient_is_exact_on_integer_data_at_size(case):
    """conv2d_wgrad (bf16x3) on {-1, 0, 1} data: bf16 holds every value (lo = 0), 50 % nonzero operands keep every partial
    sum below 2^24 (R / 4 = 12.8 M nonzero products at most), so each entry must equal the float64 dot product EXACTLY.
    A dropped, duplicated or misrouted row, tap or split changes it by an integer."""
    ops = _ops()
    t0 = _begin()
    if case == "64x64_224_split":
        n, hw, cin, cout, split = N, HW, 64, 64, True
    elif case == "stem_4ch_224_fp32":
        n, hw, cin, cout, split = N, HW, 4, 64, False
    else:
        n, hw, cin, cout, split = N, 28, 512, 512, True
    x = _ternary((n, hw, hw, cin), 31, 0.5)
    dz = _ternary((n, hw, hw, cout), 32, 0.5)
    if split:
        x, dz = ops.split_bf16(x), ops.split_bf16(dz)
        assert not x.lo.any() and not dz.lo.any()
    dw = ops.conv2d_wgrad(dz, x, 3, 3, stride=1, pad=(1, 1), b3=True)
    rps, s, ts = _wgrad_depth(n, hw, hw, cout, cin, 3, 3, split)
    co, ci = _idx(cout, 6, 3), _idx(cin, 6, 4)
    ref, _ = _wgrad_ref(dz, x, co, ci, 3, 3, 1, 1)
    got = dw[co][:, ci].double()
    bad = int((got != ref).sum())
    print(f"\n[at size train] wgrad exact {case}: tile {ts}, {s} splits of {rps} rows, {bad} of {ref.numel()} entries differ")
    assert bad == 0
    del x, dz
    _end(f"wgrad exact {case}", t0)


def test_bn_backward_sums_and_prelu_slope_are_exact_on_integer_data_at_size():
    """bn_rows_bwd_sums (and the split / add backward passes that share its col_sum_pair) with mean 0 and invstd 1 on
    {-1, 0, 1} data, dy 25 % nonzero: db = sum dy and dg = sum dy * x are integers below 2^24 at every partial sum -> EXACT.
    _prelu_bwd_chunked over the 13.2 GB tensor (four 4 GiB chunks): the slope gradient sum_{x <= 0} x * dy is exact too
    (12.5 % nonzero terms), and dx = dy or alpha * dy at sampled points to one rounding (+ the split)."""
    ops = _ops()
    from feature_vs_text_compound_emotion_amd.visual_backbone import _prelu_bwd_chunked
    t0 = _begin()
    c = 64
    x = _ternary((N, HW, HW, c), 41, 0.5)
    dy = _ternary((N, HW, HW, c), 42, 0.25)
    r = N * HW * HW
    zero, one = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
    s1, _ = _colsums64(lambda a, b: dy[a:b].double(), N, 64)
    s2, _ = _colsums64(lambda a, b: dy[a:b].double() * x[a:b].double(), N, 64)
    sums = ops.bn_rows_bwd_sums(dy.view(r, c), x.view(r, c), zero, one)
    assert torch.equal(sums[0].double(), s1) and torch.equal(sums[1].double(), s2)
    dxs, dg, db = ops.bn_rows_bwd(dy.view(r, c), x.view(r, c), zero, one, one, split_out=True)
    assert torch.equal(db.double(), s1) and torch.equal(dg.double(), s2)
    del dxs
    print("\n[at size train] bn_rows_bwd_sums / bn_rows_bwd(split_out) integer data: db, dg exact")
    alpha = torch.linspace(0.05, 0.4, c, device="cuda")
    step = max(1, (4 << 30) // (x[0].numel() * 4))
    assert -(-N // step) > 1
    dx, da = _prelu_bwd_chunked(dy, x, alpha, split_out=True)
    sa, _ = _colsums64(lambda a, b: torch.where(x[a:b] > 0, 0.0, x[a:b].double() * dy[a:b].double()), N, 64)
    bad = int((da.double() != sa).sum())
    print(f"\n[at size train] _prelu_bwd_chunked integer data, {-(-N // step)} chunks: {bad} of {c} slope-gradient entries differ")
    assert bad == 0
    pts = _points(N, HW, HW, 43)
    g = _gather(dy, pts[:, 0], pts[:, 1], pts[:, 2])
    v = _gather(x, pts[:, 0], pts[:, 1], pts[:, 2])
    ref = torch.where(v > 0, g, alpha.double() * g)
    _report("_prelu_bwd_chunked dx", _ratio(_gather(dx, pts[:, 0], pts[:, 1], pts[:, 2]), ref, (2 * U + SPLIT) * ref.abs() + 1e-30))
    del x, dy, dx
    _end("bn backward / prelu exact", t0)


# ------------------------------------------------------------------------------------------------ the stem
def test_released_stem_at_1024_frames_of_224():
    """_ReleasedStem (3 -> 64 at 224^2, R = 51.4 M): the fp32 direct conv, bn_rows_fwd's shifted one-pass statistics, PReLU
    forward / backward, bn_rows_bwd and the weight gradient over the 4-channel NHWC copy (64-wide tile), each against
    float64 on its own inputs; the restated backward is bit-identical to the Function's."""
    ops = _ops()
    from feature_vs_text_compound_emotion_amd.visual_backbone import _ReleasedStem, _bn_affine_from_saved
    t0 = _begin()
    st = _stem()
    bn = st[1]
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    x = _randn((N, 3, HW, HW), 51)
    w, g, b, a = (p.detach().clone().requires_grad_(True) for p in (st[0].weight, bn.weight, bn.bias, st[2].weight))
    y = _ReleasedStem.apply(x, bn, w, g, b, a)
    _, z, sm, si, _, _, _ = y.grad_fn.saved_tensors
    dy = _randn(y.shape, 52, 1e-3)
    grads = torch.autograd.grad(y, [w, g, b, a], dy, retain_graph=True)
    pts = _points(N, HW, HW, 53)
    # forward: the conv (fp32 products, 27 + 1 terms), the statistics, the BatchNorm + PReLU output
    xn = x.permute(0, 2, 3, 1)
    _check_conv("stem conv z", z, xn, w.detach(), pts, 1, 1, depth=28, eps_prod=U)
    per = HW * HW
    _check_bn_stats("stem bn_rows_fwd", lambda p0, p1: z[p0:p1].double(), N, _chunk(z), N * per, sm, si, rm0, rv0,
                    bn.running_mean, bn.running_var, shift=z.view(-1, 64)[0])
    sc, sh = _bn_affine_from_saved(sm, si, g.detach(), b.detach())
    zv = _gather(z, pts[:, 0], pts[:, 1], pts[:, 2])
    zb_ref = (zv - sm.double()) * si.double() * g.detach().double() + b.detach().double()
    y_ref = torch.where(zb_ref > 0, zb_ref, a.detach().double() * zb_ref)
    mag = ((zv - sm.double()).abs() * si.double() * g.detach().double().abs() + b.detach().double().abs())
    _report("stem bn apply + prelu y", _ratio(_gather(y, pts[:, 0], pts[:, 1], pts[:, 2]), y_ref, 6 * U * mag + 1e-30))
    # the backward, restated
    zb = torch.addcmul(sh, z, sc)
    dzb, da = ops.prelu_bwd(dy.contiguous(), zb, a.detach().contiguous())
    zbv, gv = _gather(zb, pts[:, 0], pts[:, 1], pts[:, 2]), _gather(dy, pts[:, 0], pts[:, 1], pts[:, 2])
    ref = torch.where(zbv > 0, gv, a.detach().double() * gv)
    _report("stem prelu_bwd dx", _ratio(_gather(dzb, pts[:, 0], pts[:, 1], pts[:, 2]), ref, 2 * U * ref.abs() + 1e-30))
    sa, saa = _colsums64(lambda p0, p1: torch.where(zb[p0:p1] > 0, 0.0, zb[p0:p1].double() * dy[p0:p1].double()), N, _chunk(zb))
    _report("stem prelu_bwd dalpha", _ratio(da.double(), sa, (_colsum_depth(N * per) + 1) * U * saa + 1e-30))
    del zb
    dz, dg, db = ops.bn_rows_bwd(dzb.view(-1, 64), z.view(-1, 64), sm, si, g.detach())
    _check_bn_bwd("stem bn_rows_bwd", dzb, z, sm, si, g.detach(), dg, db, dz.view(z.shape), pts)
    del dzb
    x4 = torch.zeros((N, HW, HW, 4), device="cuda")
    x4[..., :3] = xn
    dw4 = ops.conv2d_wgrad(dz.view(N, HW, HW, 64), x4, 3, 3, stride=1, pad=(1, 1), b3=True)
    _check_wgrad("stem wgrad (4-channel copy)", dw4, dz.view(N, HW, HW, 64), x4, 3, 3, 1, 1)
    dw = dw4[:, :3].contiguous()
    for got, want in zip((dw, dg, db, da), grads):
        assert torch.equal(got, want)
    del y, z, dz, x4, x, dy
    _end("stem", t0)


# ------------------------------------------------------------------------------------------------ released units
def _unit_args(u):
    pr, sc = u.res_layer, (u.shortcut_layer if u.cin != u.depth else None)
    ps = [pr[0].weight, pr[0].bias, pr[1].weight, pr[2].weight, pr[3].weight, pr[4].weight, pr[4].bias]
    ps += [sc[0].weight, sc[1].weight, sc[1].bias] if sc is not None else [None, None, None]
    return [p.detach().clone().requires_grad_(True) if p is not None else None for p in ps]


def _run_unit(u, x, dout, prec, memory, leaves, bufs0, retain=False):
    """one forward + backward of the released unit through its autograd Function from the same running buffers"""
    from feature_vs_text_compound_emotion_amd.visual_backbone import _ReleasedUnit
    for buf, v in zip(_bufs(u), bufs0):
        buf.copy_(v)
    xr = x.detach().requires_grad_(True)
    out = _ReleasedUnit.apply(xr, u, prec, memory, *leaves)
    live = [p for p in leaves if p is not None]
    grads = torch.autograd.grad(out, [xr] + live, dout, retain_graph=retain)
    return out, grads


def _bufs(u):
    bns = [u.res_layer[0], u.res_layer[4]] + ([u.shortcut_layer[1]] if u.cin != u.depth else [])
    return [t for bn in bns for t in (bn.running_mean, bn.running_var)]


@pytest.mark.parametrize("case", ["stage1_64x64_224", "stage2_64to128_s2_224", "stage4_512x512_28", "stage1_fp16_recompute16"])
def test_released_unit_at_1024_frames(case):
    """One released unit at N = 1024 through _ReleasedUnit (bf16x3 unless stated):
    - stage1: 64 -> 64, stride 1, 224^2 (R = 51.4 M): large-M forward / dgrad tiles, prelu_split, the chunked PReLU backward,
      bn_rows_bwd split and add, wgrad over 51.4 M rows; "recompute" gradients == "raw" bit for bit;
    - stage2: 64 -> 128, stride 2, 224 -> 112, projection shortcut: the four-parity stride-2 dgrad, the 1x1 stride-2 wgrad,
      the strided add of the shortcut's data gradient, bn_apply_nhwc with the residual affine;
    - stage4: 512 -> 512 at 28^2 (R = 803 k): the 256 x 256 wide weight-gradient kernel and its split chooser;
    - fp16 / recompute16: narrow forward convs, the normalised fp16 input plane, bf16x3 data gradients.
    The backward is restated op by op from the "raw" plan's saved tensors (recompute16: from its fp16 plane) with every stage
    checked, and the restated gradients must be bit-identical to the Function's."""
    ops = _ops()
    from feature_vs_text_compound_emotion_amd import visual_backbone as vbm
    t0 = _begin()
    idx, hw, prec, memory = {"stage1_64x64_224": (0, HW, "bf16x3", "raw"), "stage2_64to128_s2_224": (3, HW, "bf16x3", "raw"),
                             "stage4_512x512_28": (22, 28, "bf16x3", "raw"),
                             "stage1_fp16_recompute16": (0, HW, "fp16", "recompute16")}[case]
    u = _unit(idx)
    cin, depth, s = u.cin, u.depth, u.stride
    bufs0 = [t.clone() for t in _bufs(u)]
    leaves = _unit_args(u)
    x = _randn((N, hw, hw, cin), 61, 1.5, 0.25)
    ho = (hw - 1) // s + 1
    dout = _randn((N, ho, ho, depth), 62, 1e-3)
    pts_in, pts_out = _points(N, hw, hw, 63), _points(N, ho, ho, 64)
    if case == "stage1_64x64_224":
        # "recompute" (what memory="auto" picks at this size) must equal "raw" bit for bit
        out_rec, g_rec = _run_unit(u, x, dout, prec, "recompute", leaves, bufs0)
        del out_rec
    out, g_fn = _run_unit(u, x, dout, prec, memory, leaves, bufs0, retain=True)
    if case == "stage1_64x64_224":
        for a, b in zip(g_rec, g_fn):
            assert torch.equal(a, b)
        print("\n[at size train] stage1 unit: recompute == raw gradients, bit for bit")
        del g_rec
    saved = out.grad_fn.saved_tensors
    (xk, z1, z2, sm1, si1, sm2, si2, zs, sms, sis, g1, b1, w1, a1, w2, g2, ws, gs) = saved
    bs = leaves[9]
    b2 = leaves[6]
    bn1, bn2 = u.res_layer[0], u.res_layer[4]
    step = _chunk(x)
    # ---- forward stages
    _check_bn_stats(f"{case} BN1 stats", lambda a, b: x[a:b].double(), N, step, N * hw * hw, sm1, si1, bufs0[0], bufs0[1],
                    bn1.running_mean, bn1.running_var, shift=x.view(-1, cin)[0])
    narrow = prec == "fp16"
    if narrow:
        # the kept plane: fp16((x - mean) * invstd), one fp32 affine then one fp16 rounding
        xv = _gather(x, pts_in[:, 0], pts_in[:, 1], pts_in[:, 2])
        ref = (xv - sm1.double()) * si1.double()
        mag = xv.abs() * si1.double() + (sm1.double() * si1.double()).abs()
        _report(f"{case} normalised fp16 plane", _ratio(_gather(xk, pts_in[:, 0], pts_in[:, 1], pts_in[:, 2]), ref,
                                                        4 * U * mag + 2.0 ** -11 * ref.abs() + 2.0 ** -25))
        xh = ops.from_n16(xk)
        xb = torch.addcmul(b1, xh, g1)
        xop = xb.half()                                   # what the narrow conv multiplies (round-to-nearest-even)
        z1 = vbm._conv_prec(xb, ops.pack_conv_weight(w1.contiguous()), 3, 3, 1, (1, 1), prec)
        _check_conv(f"{case} conv1 z1 (fp16 operands)", z1, xop, w1.half(), pts_in, 1, 1, depth=9 * cin, eps_prod=0.0)
        del xop
    else:
        sc1, sh1 = vbm._bn_affine_from_saved(sm1, si1, g1, b1)
        xb = ops.split_bf16(x, sc1, sh1)
        xv = _gather(x, pts_in[:, 0], pts_in[:, 1], pts_in[:, 2])
        ref = xv * sc1.double() + sh1.double()
        _report(f"{case} BN1 affine + split", _ratio(_gather(xb, pts_in[:, 0], pts_in[:, 1], pts_in[:, 2]), ref,
                                                     (2 * U + SPLIT) * (xv.abs() * sc1.double().abs() + sh1.double().abs())))
        _check_conv(f"{case} conv1 z1", z1, xb, w1, pts_in, 1, 1, depth=3 * 9 * cin)
    t1 = ops.prelu_fwd(z1, a1.contiguous()) if narrow else ops.prelu_split(z1, a1.contiguous())
    zv = _gather(z1, pts_in[:, 0], pts_in[:, 1], pts_in[:, 2])
    ref = torch.where(zv > 0, zv, a1.double() * zv)
    _report(f"{case} prelu t1", _ratio(_gather(t1, pts_in[:, 0], pts_in[:, 1], pts_in[:, 2]), ref, (2 * U + SPLIT) * ref.abs() + 1e-30))
    if narrow:
        z2 = vbm._conv_prec(t1, ops.pack_conv_weight(w2.contiguous()), 3, 3, s, (1, 1), prec)
        top = t1.half()
        _check_conv(f"{case} conv2 z2 (fp16 operands)", z2, top, w2.half(), pts_out, s, 1, depth=9 * depth, eps_prod=0.0)
        del top
    else:
        _check_conv(f"{case} conv2 z2", z2, t1, w2, pts_out, s, 1, depth=3 * 9 * depth)
    if narrow:
        # recompute16 rebuilds z2 from the fp16 plane: the saved statistics (and the forward output) belong to the forward's
        # z2 from x itself, so they are not this tensor's -- the same kernels are checked by the bf16x3 cases
        del out
        return _unit_backward(case, u, x, xk, dout, z1, z2, t1, xb, xh, saved, leaves, g_fn, pts_in, pts_out, hw, ho, t0)
    _check_bn_stats(f"{case} BN2 stats", lambda a, b: z2[a:b].double(), N, _chunk(z2), N * ho * ho, sm2, si2, bufs0[2],
                    bufs0[3], bn2.running_mean, bn2.running_var, shift=z2.view(-1, depth)[0])
    sc2, sh2 = vbm._bn_affine_from_saved(sm2, si2, g2, b2.detach())
    zv = _gather(z2, pts_out[:, 0], pts_out[:, 1], pts_out[:, 2])
    o_ref = zv * sc2.double() + sh2.double()
    o_mag = zv.abs() * sc2.double().abs() + sh2.double().abs()
    if ws is not None:
        _check_conv(f"{case} shortcut conv zs", zs, x, ws, pts_out, s, 0, depth=3 * cin)
        _check_bn_stats(f"{case} shortcut BN stats", lambda a, b: zs[a:b].double(), N, _chunk(zs), N * ho * ho, sms, sis,
                        bufs0[4], bufs0[5], u.shortcut_layer[1].running_mean, u.shortcut_layer[1].running_var,
                        shift=zs.view(-1, depth)[0])
        scs, shs = vbm._bn_affine_from_saved(sms, sis, gs, bs.detach())
        rv = _gather(zs, pts_out[:, 0], pts_out[:, 1], pts_out[:, 2])
        o_ref, o_mag = o_ref + rv * scs.double() + shs.double(), o_mag + rv.abs() * scs.double().abs() + shs.double().abs()
    else:
        rv = _gather(x, pts_out[:, 0], pts_out[:, 1] * s, pts_out[:, 2] * s)
        o_ref, o_mag = o_ref + rv, o_mag + rv.abs()
    _report(f"{case} bn_apply_nhwc out", _ratio(_gather(out, pts_out[:, 0], pts_out[:, 1], pts_out[:, 2]), o_ref, 6 * U * o_mag + 1e-30))
    del out
    return _unit_backward(case, u, x, xk, dout, z1, z2, t1, xb, None, saved, leaves, g_fn, pts_in, pts_out, hw, ho, t0)


def _unit_backward(case, u, x, xk, dout, z1, z2, t1, xb, xh, saved, leaves, g_fn, pts_in, pts_out, hw, ho, t0):
    """_ReleasedUnit.backward restated op by op, every stage checked on its own inputs; bit-identical to the Function's."""
    ops = _ops()
    from feature_vs_text_compound_emotion_amd import visual_backbone as vbm
    (_, _, _, sm1, si1, sm2, si2, zs, sms, sis, g1, b1, w1, a1, w2, g2, ws, gs) = saved
    cin, depth, s = u.cin, u.depth, u.stride
    narrow = xh is not None
    split = not narrow
    dprec = "bf16x3"
    dz2, dg2, db2 = ops.bn_rows_bwd(dout.view(-1, depth), z2.view(-1, depth), sm2, si2, g2, split_out=split)
    dz2 = dz2.view(N, ho, ho, depth)
    _check_bn_bwd(f"{case} BN2 backward", dout, z2, sm2, si2, g2, dg2, db2, dz2, pts_out)
    dw2 = ops.conv2d_wgrad(dz2, t1, 3, 3, stride=s, pad=(1, 1), b3=True)
    _check_wgrad(f"{case} wgrad conv2", dw2, dz2, t1, 3, 3, s, 1)
    del t1
    dt1 = vbm._conv_dgrad(dz2, w2, s, 1, (hw, hw), dprec)
    _check_conv(f"{case} dgrad conv2 dt1", dt1, dz2, w2, pts_in, s, 1, depth=3 * 9 * depth, dgrad=True)
    del dz2
    dz1, da1 = vbm._prelu_bwd_chunked(dt1, z1, a1.contiguous(), split_out=split)
    gv, zv = _gather(dt1, pts_in[:, 0], pts_in[:, 1], pts_in[:, 2]), _gather(z1, pts_in[:, 0], pts_in[:, 1], pts_in[:, 2])
    ref = torch.where(zv > 0, gv, a1.double() * gv)
    _report(f"{case} prelu_bwd dz1", _ratio(_gather(dz1, pts_in[:, 0], pts_in[:, 1], pts_in[:, 2]), ref,
                                            (2 * U + SPLIT) * ref.abs() + 1e-30))
    per = (4 << 30) // (dt1[0].numel() * 4)
    chunks = -(-N // max(1, per))
    sa, saa = _colsums64(lambda a, b: torch.where(z1[a:b] > 0, 0.0, z1[a:b].double() * dt1[a:b].double()), N, _chunk(z1))
    d = _colsum_depth(min(N, max(1, per)) * hw * hw) + chunks + 1
    print(f"\n[at size train] {case}: PReLU backward in {chunks} chunk(s)")
    _report(f"{case} prelu_bwd dalpha", _ratio(da1.double(), sa, d * U * saa + 1e-30))
    del dt1, z1
    dw1 = ops.conv2d_wgrad(dz1, xb, 3, 3, stride=1, pad=(1, 1), b3=True)
    _check_wgrad(f"{case} wgrad conv1", dw1, dz1, xb, 3, 3, 1, 1)
    del xb
    dxb = vbm._conv_dgrad(dz1, w1, 1, 1, (hw, hw), dprec)
    _check_conv(f"{case} dgrad conv1 dxb", dxb, dz1, w1, pts_in, 1, 1, depth=3 * 9 * depth, dgrad=True)
    del dz1
    dws = dgs = dbs = addend = even = None
    if ws is not None:
        dzs, dgs, dbs = ops.bn_rows_bwd(dout.view(-1, depth), zs.view(-1, depth), sms, sis, gs)
        dzs = dzs.view(N, ho, ho, depth)
        _check_bn_bwd(f"{case} shortcut BN backward", dout, zs, sms, sis, gs, dgs, dbs, dzs, pts_out)
        if split and s == 1:
            dzs = ops.split_bf16(dzs)
        dws = ops.conv2d_wgrad(dzs, x, 1, 1, stride=s, pad=(0, 0), b3=True)
        _check_wgrad(f"{case} wgrad shortcut", dws, dzs, x, 1, 1, s, 0)
        if s == 1:
            addend = vbm._conv_dgrad(dzs, ws, 1, 0, (hw, hw), dprec)
        else:
            wt = ops.pack_conv_weight(ws.contiguous(), flip=False, transpose=True)
            even = vbm._conv_prec(dzs, wt, 1, 1, 1, (0, 0), dprec)
            _check_conv(f"{case} shortcut dgrad (even pixels)", even, dzs, ws.transpose(0, 1), pts_out, 1, 0, depth=3 * depth)
        del dzs
    elif s == 1:
        addend = dout
    rows_ok = addend is not None and cin % 4 == 0
    if narrow:
        dx, dg1, db1 = ops.bn_rows_bwd(dxb.view(-1, cin), xh.view(-1, cin), torch.zeros_like(sm1), torch.ones_like(si1),
                                       (g1 * si1).contiguous(), add=addend.view(-1, cin) if rows_ok else None)
        _check_bn_bwd(f"{case} BN1 backward", dxb, xh, torch.zeros_like(sm1), torch.ones_like(si1), (g1 * si1).contiguous(),
                      dg1, db1, dx.view(N, hw, hw, cin), pts_in, add=addend if rows_ok else None)
        del xh
    else:
        dx, dg1, db1 = ops.bn_rows_bwd(dxb.view(-1, cin), x.view(-1, cin), sm1, si1, g1,
                                       add=addend.view(-1, cin) if rows_ok else None)
        _check_bn_bwd(f"{case} BN1 backward", dxb, x, sm1, si1, g1, dg1, db1, dx.view(N, hw, hw, cin), pts_in,
                      add=addend if rows_ok else None)
    del dxb
    dx = dx.view(N, hw, hw, cin)
    if not rows_ok:
        ev = _gather(dx, pts_out[:, 0], pts_out[:, 1] * 2, pts_out[:, 2] * 2)
        add = _gather(even if ws is not None else dout, pts_out[:, 0], pts_out[:, 1], pts_out[:, 2])
        dx[:, ::2, ::2] += even if ws is not None else dout
        ref = ev + add
        _report(f"{case} strided shortcut add", _ratio(_gather(dx, pts_out[:, 0], pts_out[:, 1] * 2, pts_out[:, 2] * 2), ref,
                                                       2 * U * ref.abs() + 1e-30))
    mine = [dx, dg1, db1, dw1, da1, dw2, dg2, db2] + ([dws, dgs, dbs] if ws is not None else [])
    for i, (a, b) in enumerate(zip(mine, g_fn)):
        assert torch.equal(a, b), f"restated backward output {i} differs from the Function's"
    print(f"\n[at size train] {case}: restated backward == _ReleasedUnit.backward, bit for bit")
    del mine, g_fn, dx, x, dout, z2, zs, xk, even, addend, saved
    _end(case, t0)
