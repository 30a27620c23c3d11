"""The fusion tail's primitives called one by one against a float64 restatement of the same operation.

Every op of csrc/tail_kernels.hip that the LFAN / CAN / JMT heads and the TCN run on is compared here directly, at the
shapes where its dispatch changes path (head dims, modality counts, column-sum regimes, BatchNorm statistics paths, the
cross-entropy row loop) -- the whole-model golden fixtures run only one configuration of each.

Tolerances are derived, not picked: U is the fp32 unit roundoff, and a sum of n terms evaluated to a reduction depth d
(longest chain of additions any term passes through) is off by at most d * U * sum|terms|.  Each bound below names the
depth it uses and the data magnitude it scales; a factor of 2-4 covers the few ulp of expf / rsqrtf and the roundings that
are not sums.  Every comparison prints its observed error next to its bound (pytest -rP shows them).
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # fp32 unit roundoff (round to nearest)
LEAKY = 0.01            # ops.LEAKY_SLOPE, restated so a change there cannot move the reference with it


def _ops():
    from feature_vs_text_compound_emotion_amd import ops
    return ops


def _f32(x):
    """The value a float argument has after crossing the C ABI as float."""
    return float(torch.tensor(x, dtype=torch.float32))


def _check(name, got, ref, tol):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = (got - ref).abs().max().item() if got.numel() else 0.0
    print(f"[err] {name}: max|err| {err:.3e}  bound {tol:.3e}")
    assert err <= tol, f"{name}: max|err| {err:.3e} > bound {tol:.3e}"
    return err


def _wave_depth(n):
    """One-wave row reduction (layernorm, softmax gate): each lane adds ceil(n/64) terms serially, then 6 butterfly levels."""
    return -(-n // 64) + 6


def _col_depth(r):
    """cer_col_sum's reduction depth over r rows: slabs of 256 rows (enlarged above 1024 slabs to a multiple of 32), 8 row
    lanes per slab (serial), an 8-way fold, then the partial rows folded by the same kernel (8 lanes + 8-way fold)."""
    rps = 256
    if (r + 255) // 256 > 1024:
        rps = ((r + 1023) // 1024 + 31) // 32 * 32
    slabs = -(-r // rps)
    d = -(-min(r, rps) // 8) + 8
    return d + (-(-slabs // 8) + 8 if slabs > 1 else 0)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _slice_of_wide(t, offset, pitch):
    """t [R,C] copied into columns offset .. offset+C of a NaN-filled [R, pitch] buffer; returns (view, buffer)."""
    r, c = t.shape
    buf = torch.full((r, pitch), float("nan"), device="cuda")
    view = buf[:, offset:offset + c]
    view.copy_(t)
    return view, buf


# ------------------------------------------------------------------------------------------------ LFAN attention
def _attn_ref(qkv64, heads, hd):
    """vals_m = v_m + sum_n softmax_n(q_m . k_n / sqrt(hd)) v_n per (row, head), over the modalities
    (tail_kernels.hip, the comment above lfan_attn_fwd_kernel).  qkv rows are [head][q | k | v]."""
    r = qkv64[0].shape[0]
    parts = torch.stack([t.view(r, heads, 3, hd) for t in qkv64], dim=2)       # [R, H, M, 3, hd]
    q, k, v = parts[..., 0, :], parts[..., 1, :], parts[..., 2, :]
    p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd), dim=-1)       # [R, H, M, M]
    vals = v + p @ v
    return vals.reshape(r, -1), p


def _attn_bounds(qkv, go, heads, hd):
    """Forward: each logit is a butterfly dot product of depth L = log2(hd) + 1, so |dlogit| <= L U A with A the largest
    sum_d |q_d k_d| / sqrt(hd); a softmax probability then carries <= E U relative error with E = 2 L A + M + 4, and
    vals = v + sum p v at most 4 E U max|v|.  Backward: dp = go . v carries L U G (G = hd max|go| max|v|); dl = p (dp - dot)
    / sqrt(hd) and dq = sum_n dl k_n (dk alike) gather M such terms of size Q G / sqrt(hd); dv = go + sum_m p go_m."""
    m = len(qkv)
    r = qkv[0].shape[0]
    parts = torch.stack([t.double().view(r, heads, 3, hd) for t in qkv], dim=2)
    q, k, v = parts[..., 0, :].abs(), parts[..., 1, :].abs(), parts[..., 2, :].abs()
    L = math.log2(hd) + 1
    A = (q @ k.transpose(-1, -2)).max().item() / math.sqrt(hd)
    E = 2 * L * A + m + 4
    vmax, qmax = v.max().item(), max(q.max().item(), k.max().item())
    tol_p = 4 * E * U
    tol_vals = 4 * E * U * vmax * (1 + m)
    if go is None:
        return tol_vals, tol_p
    gmax = go.abs().max().item()
    G = hd * gmax * vmax
    tol_qk = 4 * U * m * qmax / math.sqrt(hd) * G * (2 * E + 2 * L + 2 * (m + 4))
    tol_v = 4 * U * m * gmax * (E + m + 1)
    return tol_qk, tol_v


ATTN_CASES = [(hd, m, h) for hd in (8, 16, 32, 64) for m in (1, 2, 3, 4) for h in (1, 2, 3)]


@pytest.mark.parametrize("hd,m,h", ATTN_CASES)
def test_lfan_attn_fwd_bwd_vs_float64(hd, m, h):
    ops = _ops()
    g = _gen(100 * hd + 10 * m + h)
    # R * H * hd not a multiple of 256: the last block holds dead (row, head) groups
    r = 37 if (37 * h * hd) % 256 else 39
    assert (r * h * hd) % 256
    qkv = [torch.randn(r, h * 3 * hd, generator=g) for _ in range(m)]
    dvals = torch.randn(r, h * m * hd, generator=g)
    qkv64 = [t.double().requires_grad_(True) for t in qkv]
    vals_ref, p_ref = _attn_ref(qkv64, h, hd)
    vals_ref.backward(dvals.double())

    vals, probs = ops.lfan_attn_fwd([t.cuda() for t in qkv], h, hd)
    tol_vals, tol_p = _attn_bounds(qkv, None, h, hd)
    _check(f"lfan_attn_fwd vals hd={hd} M={m} H={h}", vals, vals_ref, tol_vals)
    _check(f"lfan_attn_fwd probs hd={hd} M={m} H={h}", probs, p_ref, tol_p)

    dqkv = ops.lfan_attn_bwd([t.cuda() for t in qkv], dvals.cuda(), probs, h, hd)
    tol_qk, tol_v = _attn_bounds(qkv, dvals, h, hd)
    for i in range(m):
        got = dqkv[i].view(r, h, 3, hd)
        ref = qkv64[i].grad.view(r, h, 3, hd)
        _check(f"lfan_attn_bwd dq|dk hd={hd} M={m} H={h} mod={i}", got[:, :, :2], ref[:, :, :2], tol_qk)
        _check(f"lfan_attn_bwd dv hd={hd} M={m} H={h} mod={i}", got[:, :, 2], ref[:, :, 2], tol_v)
    # the bound is tight enough to see a dropped "+ V" residual gradient (dv would lose go_m itself)
    go_v = dvals.view(r, h, m, hd).abs().max().item()
    assert tol_v < 0.1 * go_v, (tol_v, go_v)


@pytest.mark.parametrize("hd,m", [(8, 4), (64, 3), (16, 2)])
def test_lfan_attn_large_logits_need_the_max_subtraction(hd, m):
    """Logits of a few hundred: expf without the max subtraction overflows to inf and the probabilities become NaN."""
    ops = _ops()
    g = _gen(7 * hd + m)
    r, h = 29, 2
    qkv = []
    for _ in range(m):
        t = torch.randn(r, h, 3, hd, generator=g)
        t[:, :, :2] *= 14.0                   # q, k ~ N(0, 14^2): q . k / sqrt(hd) has a std of 196
        qkv.append(t.reshape(r, -1).contiguous())
    qkv64 = [t.double().requires_grad_(True) for t in qkv]
    vals_ref, p_ref = _attn_ref(qkv64, h, hd)
    dvals = torch.randn(r, h * m * hd, generator=g)
    vals_ref.backward(dvals.double())
    logits = torch.stack([t.view(r, h, 3, hd)[:, :, 0] for t in qkv], 2) @ \
        torch.stack([t.view(r, h, 3, hd)[:, :, 1] for t in qkv], 2).transpose(-1, -2) / math.sqrt(hd)
    assert logits.abs().max().item() > 200.0  # expf(> 88.7) = inf in fp32
    vals, probs = ops.lfan_attn_fwd([t.cuda() for t in qkv], h, hd)
    tol_vals, tol_p = _attn_bounds(qkv, None, h, hd)
    _check(f"lfan_attn_fwd large-logit vals hd={hd} M={m}", vals, vals_ref, tol_vals)
    _check(f"lfan_attn_fwd large-logit probs hd={hd} M={m}", probs, p_ref, tol_p)
    dqkv = ops.lfan_attn_bwd([t.cuda() for t in qkv], dvals.cuda(), probs, h, hd)
    tol_qk, tol_v = _attn_bounds(qkv, dvals, h, hd)
    for i in range(m):
        got, ref = dqkv[i].view(r, h, 3, hd), qkv64[i].grad.view(r, h, 3, hd)
        _check(f"lfan_attn_bwd large-logit dq|dk hd={hd} M={m} mod={i}", got[:, :, :2], ref[:, :, :2], tol_qk)
        _check(f"lfan_attn_bwd large-logit dv hd={hd} M={m} mod={i}", got[:, :, 2], ref[:, :, 2], tol_v)


@pytest.mark.parametrize("hd,m,msg", [(12, 2, "head dim must be 8, 16, 32 or 64"), (128, 2, "head dim must be 8, 16, 32 or 64"),
                                      (16, 5, "1 <= modalities <= 4")])
def test_lfan_attn_refuses_unsupported_head_dim_and_modality_count(hd, m, msg):
    ops = _ops()
    qkv = [torch.zeros(5, 2 * 3 * hd, device="cuda") for _ in range(m)]
    with pytest.raises(RuntimeError, match=msg):
        ops.lfan_attn_fwd(qkv, 2, hd)
    dvals = torch.zeros(5, 2 * m * hd, device="cuda")
    probs = torch.zeros(5, 2, m, m, device="cuda")
    with pytest.raises(RuntimeError, match=msg):
        ops.lfan_attn_bwd(qkv, dvals, probs, 2, hd)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ LayerNorm
def _ln_ref(x, mask, gamma, beta, dy, eps=1e-5):
    """LN of x * mask over the last dim (biased variance), affine; grads w.r.t. the UNMASKED x, gamma and beta."""
    x64 = x.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    xm = x64 * mask.double() if mask is not None else x64
    y = F.layer_norm(xm, (x.shape[1],), g64, b64, eps)
    y.backward(dy.double())
    xmd = xm.detach()
    mean = xmd.mean(1)
    rstd = torch.rsqrt(xmd.var(1, unbiased=False) + eps)
    return y.detach(), mean, rstd, x64.grad, g64.grad, b64.grad


def _ln_bounds(x, mask, gamma, dy, y_ref, rstd_ref):
    """Row statistics are one-wave reductions of depth d = ceil(C/64) + 6: the mean carries d U max|xm|, which the
    normalisation scales by rstd (S = max|xm| rstd: large when mean >> std), so x_hat carries U Dx, Dx = d S + (d + 6) Xh.
    dx = rstd (g - s1 - xh s2) m with s1, s2 row means of g = dy gamma and g xh; dgamma / dbeta are column sums of depth
    dc = _col_depth(R) over dy xh and dy."""
    r, c = x.shape
    d = _wave_depth(c)
    xm = (x * mask if mask is not None else x).double()
    rs = rstd_ref.max().item()
    S = xm.abs().max().item() * rs
    xh = ((xm - xm.mean(1, keepdim=True)) * rstd_ref[:, None])
    Xh = xh.abs().max().item()
    gmax = gamma.abs().max().item()
    Dx = d * S + (d + 6) * Xh
    tol_y = 4 * U * (gmax * Dx + y_ref.abs().max().item())
    mm = mask.abs().max().item() if mask is not None else 1.0
    G = (dy.double() * gamma.double()).abs().max().item()
    tol_dx = 4 * U * rs * mm * (d * G + Xh * (d * G * Xh + G * Dx) + G * Xh * Dx + 4 * G * (2 + Xh * Xh))
    dc = _col_depth(r)
    dy64 = dy.double()
    tol_dg = 2 * U * (dc * (dy64 * xh).abs().sum(0).max().item() + dy64.abs().sum(0).max().item() * Dx)
    tol_db = 2 * U * dc * dy64.abs().sum(0).max().item()
    return tol_y, tol_dx, tol_dg, tol_db


def _run_ln(x, mask, gamma, beta, dy, layout, label):
    ops = _ops()
    r, c = x.shape
    y_ref, mean_ref, rstd_ref, dx_ref, dg_ref, db_ref = _ln_ref(x, mask, gamma, beta, dy)
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    md = mask.cuda() if mask is not None else None
    if layout == "slice":   # out / dy as column slices of wider buffers, at column offsets as the LFAN head uses them
        out, obuf = _slice_of_wide(torch.zeros(r, c), 5, c + 9)
        dyd, _ = _slice_of_wide(dy, 3, c + 11)
    else:
        out, obuf, dyd = None, None, dy.cuda()
    y, mean, rstd = ops.layernorm_fwd(xd, gd, bd, mask=md, eps=1e-5, out=out)
    tol_y, tol_dx, tol_dg, tol_db = _ln_bounds(x, mask, gamma, dy, y_ref, rstd_ref)
    _check(f"layernorm_fwd y {label}", y, y_ref, tol_y)
    _check(f"layernorm_fwd mean {label}", mean, mean_ref, 2 * U * _wave_depth(c) *
           (x * mask if mask is not None else x).abs().max().item())
    # rstd: the centred second pass is a sum of depth d (the mean's own error enters only squared), then rsqrt: relative
    # (d + 6) U
    _check(f"layernorm_fwd rstd {label}", rstd, rstd_ref, 4 * U * (_wave_depth(c) + 6) * rstd_ref.max().item())
    if obuf is not None:   # nothing written outside the slice
        assert torch.isnan(obuf[:, :5]).all() and torch.isnan(obuf[:, 5 + c:]).all()
    dx, dg, db = ops.layernorm_bwd(dyd, xd, gd, mean, rstd, mask=md)
    _check(f"layernorm_bwd dx {label}", dx, dx_ref, tol_dx)
    _check(f"layernorm_bwd dgamma {label}", dg, dg_ref, tol_dg)
    _check(f"layernorm_bwd dbeta {label}", db, db_ref, tol_db)
    if mask is not None:   # a forgotten "* m" in dx would leave the dropped elements a gradient
        assert (dx.cpu()[mask == 0] == 0).all()


LN_C = (1, 7, 63, 64, 65, 96, 768, 1000)
LN_R = (1, 3, 5, 257, 3000)


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("layout", ["dense", "slice"])
@pytest.mark.parametrize("c", LN_C)
@pytest.mark.parametrize("r", LN_R)
def test_layernorm_fwd_bwd_vs_float64(r, c, layout, masked):
    g = _gen(r * 1009 + c * 7 + (layout == "slice") * 3 + masked)
    x = torch.randn(r, c, generator=g) * 1.5 + 0.3
    gamma = torch.rand(c, generator=g) + 0.5
    beta = torch.randn(c, generator=g)
    dy = torch.randn(r, c, generator=g)
    mask = None
    if masked:  # dropout-style, p = 0.2: {0, 1.25}
        mask = (torch.rand(r, c, generator=g) >= 0.2).float() / 0.8
        mask.view(-1)[0] = 0.0
    _run_ln(x, mask, gamma, beta, dy, layout, f"R={r} C={c} {layout} mask={masked}")


@pytest.mark.parametrize("c", [64, 768, 1000])
def test_layernorm_rows_with_mean_far_above_std(c):
    """Rows at 1000 +- 1: a one-pass E[x^2] - E[x]^2 would cancel to noise; the kernel's centred second pass must not."""
    g = _gen(c)
    r = 300
    x = 1000.0 + torch.randn(r, c, generator=g)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    dy = torch.randn(r, c, generator=g)
    _run_ln(x, None, gamma, beta, dy, "slice", f"mean>>std C={c}")


# ------------------------------------------------------------------------------------------------ softmax gate
@pytest.mark.parametrize("c", [1, 3, 64, 65, 200])
def test_softmax_gate_fwd_bwd_vs_float64(c):
    """out = softmax(z) * c per row.  sum exp is a one-wave reduction of depth d: p carries (d + 4) U relative error (expf,
    division); dz = p (g c - sum p g c) adds the same on the row sum."""
    ops = _ops()
    g = _gen(c + 17)
    r = 133
    z = (torch.rand(r, c, generator=g) * 2 - 1) * 80.0       # logits up to +-80
    z[0] = 80.0                                               # a row of ties at the top
    cc = torch.randn(r, c, generator=g)
    dout = torch.randn(r, c, generator=g)
    z64, c64 = z.double().requires_grad_(True), cc.double().requires_grad_(True)
    p64 = torch.softmax(z64, 1)
    out64 = p64 * c64
    out64.backward(dout.double())
    out, prob = ops.softmax_gate_fwd(z.cuda(), cc.cuda())
    d = _wave_depth(c)
    pc = (p64 * c64).detach().abs()
    _check(f"softmax_gate_fwd prob C={c}", prob, p64, 4 * U * (d + 4) * p64.detach().max().item())
    _check(f"softmax_gate_fwd out C={c}", out, out64, 4 * U * (d + 4) * pc.max().item())
    dz, dc = ops.softmax_gate_bwd(dout.cuda(), prob, cc.cuda())
    gc = (dout.double() * c64.detach()).abs()
    s = (p64.detach() * gc).sum(1, keepdim=True)
    tol_dz = 4 * U * (d + 4) * (p64.detach() * (gc + s)).max().item() * 2
    _check(f"softmax_gate_bwd dz C={c}", dz, z64.grad, tol_dz)
    _check(f"softmax_gate_bwd dc C={c}", dc, c64.grad, 4 * U * (d + 4) * (dout.double().abs() * p64.detach()).max().item())


# ------------------------------------------------------------------------------------------------ TCN glue
def _elementwise_inputs(n, g):
    z = torch.randn(n, generator=g)
    z[::7] = 0.0                                              # exact zeros: leaky'(0) is the slope, as torch
    return z


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "dropmask"])
@pytest.mark.parametrize("slope", [0.0, LEAKY], ids=["relu", "leaky"])
def test_leaky_relu_and_act_mask_bwd_vs_autograd(slope, masked):
    """y = mask * leaky(z) (tail_kernels.hip, act_mask_bwd_kernel's comment); dz from float64 autograd.  leaky_relu is one
    fp32 product (<= U relative), dz = dy * m * slope two (<= 3 U relative, elementwise)."""
    ops = _ops()
    g = _gen(int(slope * 100) + masked)
    n = 4 * 1031                                              # n / 4 = 1031: not a multiple of 256
    z = _elementwise_inputs(n, g)
    dy = torch.randn(n, generator=g)
    s = _f32(slope)
    mask = ((torch.rand(n, generator=g) >= 0.2).float() / 0.8) if masked else None
    z64 = z.double().requires_grad_(True)
    y64 = F.leaky_relu(z64, s)
    _check(f"leaky_relu slope={slope}", ops.leaky_relu(z.cuda(), slope), y64, U * y64.detach().abs().max().item())
    a64 = y64 * mask.double() if masked else y64
    a64.backward(dy.double())
    y = ops.leaky_relu(z.cuda(), slope)
    if masked:
        y = y * mask.cuda()
    dz = ops.act_mask_bwd(dy.cuda(), y, mask.cuda() if masked else None, slope)
    err = (dz.double().cpu() - z64.grad).abs()
    print(f"[err] act_mask_bwd slope={slope} mask={masked}: max|err| {err.max():.3e} (bound 3 U |ref| elementwise)")
    assert (err <= 3 * U * z64.grad.abs()).all()


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "dropmask"])
@pytest.mark.parametrize("slope", [0.0, LEAKY], ids=["relu", "leaky"])
def test_tblock_tail_bwd_vs_autograd(slope, masked):
    """out = leaky(a2 + res), a2 = mask2 * leaky(z2) (tail_kernels.hip, tblock_tail_bwd_kernel's comment): du = d out / d res,
    dz2 = d out / d z2 by float64 autograd.  The kernel takes leaky'(.) from the signs of out and a2; the test first checks
    that the fp32 forward it feeds the kernel has the float64 signs.  du is one product (<= 2 U relative, elementwise), dz2
    three (<= 4 U)."""
    ops = _ops()
    g = _gen(int(slope * 1000) + 2 * masked + 5)
    n = 4 * 777
    z2, res = _elementwise_inputs(n, g), torch.randn(n, generator=g)
    res[::11] = 0.0
    dout = torch.randn(n, generator=g)
    s = _f32(slope)
    mask = ((torch.rand(n, generator=g) >= 0.5).float() * 2.0) if masked else None
    z64, r64 = z2.double().requires_grad_(True), res.double().requires_grad_(True)
    a64 = F.leaky_relu(z64, s) * (mask.double() if masked else 1.0)
    o64 = F.leaky_relu(a64 + r64, s)
    o64.backward(dout.double())
    a2 = ops.leaky_relu(z2.cuda(), slope)
    if masked:
        a2 = a2 * mask.cuda()
    out = ops.leaky_relu(a2 + res.cuda(), slope)
    assert torch.equal(torch.sign(a2.cpu().double()), torch.sign(a64.detach()))
    assert torch.equal(torch.sign(out.cpu().double()), torch.sign(o64.detach()))
    du, dz2 = ops.tblock_tail_bwd(dout.cuda(), out, a2, mask.cuda() if masked else None, slope)
    for name, got, ref, k in (("du", du, r64.grad, 2), ("dz2", dz2, z64.grad, 4)):
        err = (got.double().cpu() - ref).abs()
        print(f"[err] tblock_tail_bwd {name} slope={slope} mask={masked}: max|err| {err.max():.3e} "
              f"(bound {k} U |ref| elementwise)")
        assert (err <= k * U * ref.abs()).all(), name


# ------------------------------------------------------------------------------------------------ column sums
COL_LAYOUTS = ("dense", "slice_pitch4", "slice_pitch_odd", "slice_misaligned")
# R: one slab, one full slab, two slabs, many slabs, enlarged slabs (> 1024 of 256 rows).  C = 36, 132: C % 4 == 0 but
# not a multiple of 128 (a partly empty 128-column block); C = 70: C % 4 != 0.
COL_CASES = [(r, c, lay) for r in (1, 256, 257, 5000, 300_001) for c in (36, 132, 70) for lay in COL_LAYOUTS
             if not (r == 300_001 and c == 132 and lay != "dense")]   # (keeps the file's run time down)


def _col_input(t, layout):
    c = t.shape[1]
    if layout == "dense":
        return t.cuda()
    if layout == "slice_pitch4":       # start column 4, pitch % 4 == 0: 16-byte loads are legal
        return _slice_of_wide(t, 4, c + 8)[0]
    if layout == "slice_pitch_odd":    # pitch % 4 != 0
        return _slice_of_wide(t, 0, c + 3)[0]
    # start column 1, pitch % 4 == 0: the pitch allows float4 loads, the 4-byte-aligned base does not
    return _slice_of_wide(t, 1, (c + 1 + 3) // 4 * 4 + 4)[0]


@pytest.mark.parametrize("r,c,layout", COL_CASES)
def test_col_sum_every_regime_vs_float64(r, c, layout):
    """Integer inputs in [-8, 8] make every partial sum exact in fp32 (|sum| < 2^24), so the kernel must match EXACTLY in
    every regime -- a lost or doubled row or column shows.  Gaussian inputs then meet the d U sum|a| bound with
    d = _col_depth(R); and two calls are bit-identical (no atomics)."""
    ops = _ops()
    g = _gen(r + c)
    ai = torch.randint(-8, 9, (r, c), generator=g).float()
    a = _col_input(ai, layout)
    if layout == "slice_misaligned":
        assert a.data_ptr() % 16 == 4 and a.stride(0) % 4 == 0
    _check(f"col_sum exact R={r} C={c} {layout}", ops.col_sum(a), ai.double().sum(0), 0.0)
    an = torch.randn(r, c, generator=g)
    a = _col_input(an, layout)
    s1, s2 = ops.col_sum(a), ops.col_sum(a)
    assert torch.equal(s1, s2), "col_sum is not deterministic"
    _check(f"col_sum R={r} C={c} {layout}", s1, an.double().sum(0), _col_depth(r) * U * an.abs().sum(0).max().item())


# ------------------------------------------------------------------------------------------------ BatchNorm over rows
def _bn_bounds(x, w, b, rstd_ref, mean_ref, y_ref):
    """Mean: column sums of depth d = _col_depth(R) of |x| (or of |x - x[0]| in the shifted one-pass path, <= 2 max|x|):
    Dm = 2 d U max|x|.  Variance: d U max (x - k)^2 plus the mean's error carried through: Dv = 4 d U max|x|^2 + 2 max|x| Dm.
    invstd = rsqrt(var + eps) moves by rstd^3 Dv / 2; y = (x - mean) invstd w + b by |w| (rstd Dm + max|x - mean| Dinv)."""
    r = x.shape[0]
    d = _col_depth(r)
    xm = x.double().abs().max().item()
    Dm = 2 * d * U * xm
    Dv = 4 * d * U * xm * xm + 2 * xm * Dm
    rs = rstd_ref.max().item()
    tol_inv = 2 * (0.5 * rs ** 3 * Dv + 4 * U * rs)
    tol_mean = 2 * Dm
    dev = (x.double() - mean_ref).abs().max().item()
    tol_y = 2 * w.abs().max().item() * (rs * tol_mean + dev * tol_inv) + 4 * U * y_ref.abs().max().item()
    return tol_mean, tol_inv, tol_y, Dv


BN_CASES = [  # (R, C, x layout, id): every statistics path of cer_bn_rows_fwd and both of cer_bn_rows_bwd_sums
    (2, 36, "dense", "R2"),                          # kernel path, unbiased-variance denominator R - 1 = 1
    (300, 70, "dense", "small"),                     # one-block statistics kernel; bwd fallback (C % 4 != 0)
    (300, 36, "dense", "small_pair"),                # one-block statistics; bwd pair path (R > 256)
    (3000, 36, "dense", "pair"),                     # one-pass shifted statistics (col_sum_pair); bwd pair path
    (3000, 70, "dense", "big_c_odd"),                # two col_sum passes + bn_rows_mean_kernel (C % 4 != 0)
    (3000, 36, "slice", "big_slice"),                # two col_sum passes (column-slice x); bwd fallback
    (3000, 36, "misaligned", "big_misaligned"),      # dense rows at a 4-byte-aligned base: must not take float4 loads
    (9600, 64, "dense", "reference_window"),         # B * 300 rows with B = 32, as the LFAN BatchNorm runs
]


def _bn_x(x, layout):
    if layout == "dense":
        return x.cuda()
    if layout == "slice":
        return _slice_of_wide(x, 4, x.shape[1] + 12)[0]
    r, c = x.shape
    buf = torch.empty(r * c + 1, device="cuda")      # contiguous [R, C] one float into its buffer
    v = buf[1:].view(r, c)
    v.copy_(x)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("r,c,layout", [case[:3] for case in BN_CASES], ids=[case[3] for case in BN_CASES])
def test_bn_rows_fwd_stats_bwd_vs_float64(r, c, layout):
    ops = _ops()
    g = _gen(r * 3 + c)
    x = torch.randn(r, c, generator=g) * 2.0 + 3.0
    w, b = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    rm0, rv0 = torch.randn(c, generator=g) * 0.1, torch.rand(c, generator=g) + 0.5
    dy = torch.randn(r, c, generator=g)
    mom, eps = 0.1, 1e-5
    # float64 reference: torch's own train-mode BatchNorm (running var updated with the unbiased variance)
    x64, w64, b64 = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    rm64, rv64 = rm0.double().clone(), rv0.double().clone()
    y64 = F.batch_norm(x64, rm64, rv64, w64, b64, training=True, momentum=mom, eps=eps)
    y64.backward(dy.double())
    mean64 = x.double().mean(0)
    var64 = x.double().var(0, unbiased=False)
    rstd64 = torch.rsqrt(var64 + eps)
    tol_mean, tol_inv, tol_y, Dv = _bn_bounds(x, w, b, rstd64, mean64, y64)
    tol_rm = mom * tol_mean + 4 * U * rm64.abs().max().item()
    tol_rv = 2 * mom * Dv * r / max(r - 1, 1) + 4 * U * rv64.abs().max().item()
    if r == 2:   # the bound separates the unbiased running-variance update from the biased one
        biased = (1 - mom) * rv0.double() + mom * var64
        assert (biased - rv64).abs().max().item() > 10 * tol_rv

    xd = _bn_x(x, layout)
    out, obuf = _slice_of_wide(torch.zeros(r, c), 3, c + 7)     # out= a column slice, as the LFAN leader's BatchNorm
    rm, rv = rm0.cuda(), rv0.cuda()
    y, sm, si = ops.bn_rows_fwd(xd, w.cuda(), b.cuda(), rm, rv, True, eps, mom, out=out)
    _check(f"bn_rows_fwd train y [{layout} R={r} C={c}]", y, y64, tol_y)
    assert torch.isnan(obuf[:, :3]).all() and torch.isnan(obuf[:, 3 + c:]).all()
    _check(f"bn_rows_fwd save_mean [{layout} R={r} C={c}]", sm, mean64, tol_mean)
    _check(f"bn_rows_fwd save_invstd [{layout} R={r} C={c}]", si, rstd64, tol_inv)
    _check(f"bn_rows_fwd running_mean [{layout} R={r} C={c}]", rm, rm64, tol_rm)
    _check(f"bn_rows_fwd running_var [{layout} R={r} C={c}]", rv, rv64, tol_rv)

    rm2, rv2 = rm0.cuda(), rv0.cuda()
    sm2, si2 = ops.bn_rows_stats(xd, rm2, rv2, eps, mom)
    assert torch.equal(sm2, sm) and torch.equal(si2, si) and torch.equal(rm2, rm) and torch.equal(rv2, rv)

    # backward from the float64 statistics rounded to fp32 (each rounding moves x_hat by <= 2 U (max|x| rstd + max|x_hat|))
    smf, sif = mean64.float().cuda(), rstd64.float().cuda()
    dyd = dy.cuda() if layout != "slice" else _slice_of_wide(dy, 2, c + 5)[0]
    dx, dw, db = ops.bn_rows_bwd(dyd, xd, smf, sif, w.cuda(), True)
    d = _col_depth(r)
    xh = (x.double() - mean64) * rstd64
    Xh = xh.abs().max().item()
    Dxh = 4 * U * (x.double().abs().max().item() * rstd64.max().item() + Xh)
    sdy = dy.double().abs().sum(0)
    sdyxh = (dy.double() * xh).abs().sum(0)
    tol_db = 2 * d * U * sdy.max().item()
    tol_dw = 2 * d * U * sdyxh.max().item() + sdy.max().item() * Dxh
    _check(f"bn_rows_bwd db [{layout} R={r} C={c}]", db, b64.grad, tol_db)
    _check(f"bn_rows_bwd dw [{layout} R={r} C={c}]", dw, w64.grad, tol_dw)
    tol_dx = 2 * w.abs().max().item() * rstd64.max().item() * (
        (tol_db + Xh * tol_dw + sdyxh.max().item() * Dxh) / r
        + 4 * U * (dy.abs().max().item() + (sdy.max().item() + Xh * sdyxh.max().item()) / r))
    _check(f"bn_rows_bwd dx [{layout} R={r} C={c}]", dx, x64.grad, tol_dx)

    # eval: y = (x - running_mean) rsqrt(running_var + eps) w + b, dx = dy w invstd
    x64e = x.double().requires_grad_(True)
    ye64 = F.batch_norm(x64e, rm0.double(), rv0.double(), w.double(), b.double(), training=False, eps=eps)
    ye64.backward(dy.double())
    rme, rve = rm0.cuda(), rv0.cuda()
    ye, sme, sie = ops.bn_rows_fwd(xd, w.cuda(), b.cuda(), rme, rve, False, eps, mom)
    assert sme is None and sie is None and torch.equal(rme.cpu(), rm0) and torch.equal(rve.cpu(), rv0)
    rse = torch.rsqrt(rv0.double() + eps)
    tol_ye = 8 * U * (w.abs().max().item() * rse.max().item() * (x.double() - rm0.double()).abs().max().item()
                      + ye64.abs().max().item())
    _check(f"bn_rows_fwd eval y [{layout} R={r} C={c}]", ye, ye64, tol_ye)
    dxe, _, _ = ops.bn_rows_bwd(dyd, xd, rm0.cuda(), rse.float().cuda(), w.cuda(), False)
    _check(f"bn_rows_bwd eval dx [{layout} R={r} C={c}]", dxe, x64e.grad,
           4 * U * (dy.double().abs() * w.double().abs() * rse).max().item())


# ------------------------------------------------------------------------------------------------ cross entropy
@pytest.mark.parametrize("c", [1, 7, 1000])
@pytest.mark.parametrize("r", [1, 1023, 1025, 9600])
def test_cross_entropy_vs_float64(r, c):
    """Mean CE with ignore_index = -100 rows.  Logits at +-1e4: lse = max + log(sum exp) carries u (|max| + C + 4), z - lse
    E = 3 max|z| + C + 8 ulps, softmax (E + 4) U relative; the loss is the mean of per-row terms reduced to depth
    ceil(R / 1024) + 6 + 16 (rows per thread, butterfly, 16 waves)."""
    ops = _ops()
    g = _gen(r * 11 + c)
    z = torch.randn(r, c, generator=g) * 3.0 + torch.sign(torch.randn(r, 1, generator=g)) * 1e4
    labels = torch.randint(0, c, (r,), generator=g).float()
    ign = torch.rand(r, generator=g) < 0.2
    if r > 1:
        labels[ign] = -100.0
        labels[0] = float(c - 1)
    z64 = z.double().requires_grad_(True)
    loss64 = F.cross_entropy(z64, labels.long(), ignore_index=-100, reduction="mean")
    loss64.backward()
    loss, dl = ops.cross_entropy(z.cuda(), labels.cuda())
    ops.flush_label_check()
    nvalid = int((labels != -100).sum())
    zmax = z.abs().max().item()
    E = 3 * zmax + c + 8
    depth = -(-r // 1024) + 6 + 16
    per_row = (torch.logsumexp(z.double(), 1) - z.double().gather(1, labels.clamp(min=0).long()[:, None])[:, 0]).abs()
    tol_loss = 2 * U * (E + depth * per_row.max().item())
    _check(f"cross_entropy loss R={r} C={c}", loss.view(()), loss64, tol_loss)
    _check(f"cross_entropy dlogits R={r} C={c}", dl, z64.grad, 2 * U * (E + 4) / nvalid)
    assert (dl.cpu()[labels == -100] == 0).all()


def test_cross_entropy_all_rows_ignored_is_nan_like_torch():
    ops = _ops()
    z = torch.randn(40, 7, generator=_gen(3))
    labels = torch.full((40,), -100.0)
    ref = F.cross_entropy(z.double(), labels.long(), ignore_index=-100)
    loss, dl = ops.cross_entropy(z.cuda(), labels.cuda())
    ops.flush_label_check()
    assert torch.isnan(ref) and torch.isnan(loss.cpu())
    assert (dl.cpu() == 0).all()


# ------------------------------------------------------------------------------------------------ copy_cols
def test_copy_cols_between_wide_buffers():
    ops = _ops()
    r, c = 37, 13                                    # R * C = 481: not a multiple of 256
    x = torch.randn(r, c, generator=_gen(9))
    xs, _ = _slice_of_wide(x, 2, c + 6)              # source pitch 19
    buf = torch.full((r, c + 10), float("nan"), device="cuda")
    out = buf[:, 7:7 + c]                            # destination pitch 23, at column offset 7
    ops.copy_cols(xs, out)
    _check("copy_cols", out, x, 0.0)
    assert torch.isnan(buf[:, :7]).all() and torch.isnan(buf[:, 7 + c:]).all()


# ------------------------------------------------------------------------------------------------ wrapper refusals
# Only arguments that would stay in bounds even if they reached a kernel: column slices, oversized or transposed tensors,
# wrong dtypes.  Each must raise ValueError before anything is launched.
class _T:
    """The refusal cases' tensors (built on the GPU when a case runs, not at collection)."""
    def __init__(self):
        cu = dict(device="cuda")
        self.r, self.c = r, c = 8, 16
        self.x, self.wide = torch.randn(r, c, **cu), torch.randn(r, c + 8, **cu)
        self.vec, self.big_vec, self.rows = torch.ones(c, **cu), torch.ones(c + 4, **cu), torch.ones(r, **cu)
        self.qkv = [torch.randn(r, 2 * 3 * 8, **cu) for _ in range(2)]           # H = 2, hd = 8, M = 2
        self.dvals, self.probs = torch.randn(r, 2 * 2 * 8, **cu), torch.rand(r, 2, 2, 2, **cu)

    def __call__(self, *shape, dtype=torch.float32):
        return torch.randn(*shape, device="cuda", dtype=dtype)


REFUSALS = {
    "layernorm_bwd x column slice": lambda o, t: o.layernorm_bwd(t.x, t.wide[:, :t.c], t.vec, t.rows, t.rows),
    "layernorm_bwd mask transposed": lambda o, t: o.layernorm_bwd(t.x, t.x, t.vec, t.rows, t.rows, mask=t(t.c, t.r).t()),
    "layernorm_bwd gamma oversized": lambda o, t: o.layernorm_bwd(t.x, t.x, t.big_vec, t.rows, t.rows),
    "layernorm_bwd mean oversized": lambda o, t: o.layernorm_bwd(t.x, t.x, t.vec, t(t.r + 3), t.rows),
    "layernorm_bwd rstd float64": lambda o, t: o.layernorm_bwd(t.x, t.x, t.vec, t.rows, t.rows.double()),
    "layernorm_fwd x column slice": lambda o, t: o.layernorm_fwd(t.wide[:, :t.c], t.vec, t.vec),
    "layernorm_fwd gamma oversized": lambda o, t: o.layernorm_fwd(t.x, t.big_vec, t.vec),
    "layernorm_fwd beta float64": lambda o, t: o.layernorm_fwd(t.x, t.vec, t.vec.double()),
    "layernorm_fwd mask oversized": lambda o, t: o.layernorm_fwd(t.x, t.vec, t.vec, mask=t(t.r, t.c + 4)),
    "layernorm_fwd out oversized": lambda o, t: o.layernorm_fwd(t.x, t.vec, t.vec, out=t(t.r + 2, t.c)),
    "lfan_attn_fwd qkv oversized": lambda o, t: o.lfan_attn_fwd([t.qkv[0], t(t.r, 52)], 2, 8),
    "lfan_attn_fwd modality rows differ": lambda o, t: o.lfan_attn_fwd([t.qkv[0], t(t.r + 2, 48)], 2, 8),
    "lfan_attn_fwd qkv column slice": lambda o, t: o.lfan_attn_fwd([t.qkv[0], t(t.r, 64)[:, :48]], 2, 8),
    "lfan_attn_bwd qkv float64": lambda o, t: o.lfan_attn_bwd([t.qkv[0], t.qkv[1].double()], t.dvals, t.probs, 2, 8),
    "lfan_attn_bwd dvals oversized": lambda o, t: o.lfan_attn_bwd(t.qkv, t(t.r, 40), t.probs, 2, 8),
    "lfan_attn_bwd probs oversized": lambda o, t: o.lfan_attn_bwd(t.qkv, t.dvals, t(t.r, 2, 3, 3), 2, 8),
    "lfan_attn_bwd probs transposed": lambda o, t: o.lfan_attn_bwd(t.qkv, t.dvals, t.probs.transpose(2, 3), 2, 8),
    "softmax_gate_fwd c oversized": lambda o, t: o.softmax_gate_fwd(t.x, t(t.r, t.c + 1)),
    "softmax_gate_fwd z transposed": lambda o, t: o.softmax_gate_fwd(t(t.c, t.c).t(), t(t.c, t.c)),
    "softmax_gate_bwd c transposed": lambda o, t: o.softmax_gate_bwd(t(t.c, t.c), t(t.c, t.c), t(t.c, t.c).t()),
    "softmax_gate_bwd prob oversized": lambda o, t: o.softmax_gate_bwd(t.x, t(t.r + 1, t.c), t.x),
    "act_mask_bwd y oversized": lambda o, t: o.act_mask_bwd(t.x, t(t.r, t.c + 4)),
    "act_mask_bwd mask float64": lambda o, t: o.act_mask_bwd(t.x, t.x, t(t.r, t.c, dtype=torch.float64)),
    "tblock_tail_bwd a2 transposed": lambda o, t: o.tblock_tail_bwd(t(t.c, t.c), t(t.c, t.c), t(t.c, t.c).t()),
    "tblock_tail_bwd out oversized": lambda o, t: o.tblock_tail_bwd(t.x, t(t.r, t.c + 4), t.x),
    "tblock_tail_bwd mask2 oversized": lambda o, t: o.tblock_tail_bwd(t.x, t.x, t.x, t(t.r + 4, t.c)),
    # a narrow view into a wide buffer: 5 columns would land past the view's 2 (inside the buffer's pitch of 10)
    "copy_cols out narrower than x": lambda o, t: o.copy_cols(t(t.r, 5), t(t.r, 10)[:, :2]),
    "copy_cols out more rows than x": lambda o, t: o.copy_cols(t(t.r, 5), t(t.r + 3, 10)[:, :5]),
    "bn_rows_fwd w oversized": lambda o, t: o.bn_rows_fwd(t.x, t.big_vec, t.vec, t.vec.clone(), t.vec.clone(), True),
    "bn_rows_fwd out oversized": lambda o, t: o.bn_rows_fwd(t.x, t.vec, t.vec, t.vec.clone(), t.vec.clone(), True,
                                                            out=t(t.r + 1, t.c)),
    "bn_rows_stats running_var oversized": lambda o, t: o.bn_rows_stats(t.x, t.vec.clone(), t.big_vec.clone()),
    "bn_rows_bwd save_mean oversized": lambda o, t: o.bn_rows_bwd(t.x, t.x, t.big_vec, t.vec, t.vec),
    "bn_rows_bwd save_invstd float64": lambda o, t: o.bn_rows_bwd(t.x, t.x, t.vec, t.vec.double(), t.vec),
    "bn_rows_bwd w oversized": lambda o, t: o.bn_rows_bwd(t.x, t.x, t.vec, t.vec, t.big_vec),
    "bn_rows_bwd x more rows": lambda o, t: o.bn_rows_bwd(t.x, t(t.r + 2, t.c), t.vec, t.vec, t.vec),
    "cross_entropy logits column slice": lambda o, t: o.cross_entropy(t.wide[:, :t.c], torch.zeros(t.r, device="cuda")),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_wrapper_refuses_before_launch(case):
    t = _T()
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        REFUSALS[case](_ops(), t)
    torch.cuda.synchronize()


# The encoder-side wrappers read their per-channel vectors (PReLU slopes, BatchNorm scale / shift, the residual's affine)
# at channel index c of the tensor's last axis: a vector shorter than C would be read past its end.
class _E:
    def __init__(self):
        cu = dict(device="cuda")
        self.c = c = 64
        self.x = torch.randn(2, 4, 4, c, **cu)
        self.vec, self.short = torch.ones(c, **cu), torch.ones(c // 2, **cu)


ENCODER_REFUSALS = {
    "prelu_fwd alpha short": lambda o, t: o.prelu_fwd(t.x, t.short),
    "prelu_split alpha short": lambda o, t: o.prelu_split(t.x, t.short),
    "prelu_bwd alpha short": lambda o, t: o.prelu_bwd(t.x, t.x, t.short),
    "prelu_bwd dy fewer rows": lambda o, t: o.prelu_bwd(t.x[:1], t.x, t.vec),
    "split_bf16 scale short": lambda o, t: o.split_bf16(t.x, t.short, t.vec),
    "split_bf16 shift short": lambda o, t: o.split_bf16(t.x, t.vec, t.short),
    "to_n16 scale short": lambda o, t: o.to_n16(t.x, torch.float16, t.short, t.vec),
    "bn_apply_nhwc scale short": lambda o, t: o.bn_apply_nhwc(t.x, t.short, t.vec),
    "bn_apply_nhwc alpha short": lambda o, t: o.bn_apply_nhwc(t.x, t.vec, t.vec, alpha=t.short),
    "bn_apply_nhwc res_shift short": lambda o, t: o.bn_apply_nhwc(t.x, t.vec, t.vec, res=t.x, res_scale=t.vec,
                                                                  res_shift=t.short),
    "bn_apply_nhwc mask short": lambda o, t: o.bn_apply_nhwc(t.x, t.vec, t.vec, mask=t.x[:1].contiguous()),
    "bn_apply_nhwc_b3 shift short": lambda o, t: o.bn_apply_nhwc_b3(t.x, t.vec, t.short),
    "bn_apply_nhwc_b3 res_scale short": lambda o, t: o.bn_apply_nhwc_b3(t.x, t.vec, t.vec, res=t.x, res_scale=t.short,
                                                                        res_shift=t.vec),
    "bn_apply_nhwc_n16 scale short": lambda o, t: o.bn_apply_nhwc_n16(t.x, t.short, t.vec, dtype=torch.float16),
    "bn_apply_nhwc_n16 alpha short": lambda o, t: o.bn_apply_nhwc_n16(t.x, t.vec, t.vec, dtype=torch.float16, alpha=t.short),
}


@pytest.mark.parametrize("case", list(ENCODER_REFUSALS))
def test_encoder_wrapper_refuses_before_launch(case):
    t = _E()
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ENCODER_REFUSALS[case](_ops(), t)
    torch.cuda.synchronize()
