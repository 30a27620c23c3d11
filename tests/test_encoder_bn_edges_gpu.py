"""``csrc/encoder_bn.hip`` -- the train-mode BatchNorm passes of the IR-50 -- pinned to the float64 restatement of
``tests/encoder_bn_ref.py`` (proved on the CPU by ``tests/test_encoder_bn_ref_cpu.py``) at the edges of their launches.

(a) bn_apply, exact: all three wrappers and every output form return the reference BIT FOR BIT at every channel count and around
    every row count where the thread layout or the statistics partition changes; the per-tile statistics are the exact sums of
    the FINAL value over exactly the rows of their tile.  (b) the strided / cropped residual, with NaN wherever the kernel must
    not read.  (c) bn_apply on standard-normal data within the derived bound; 16-bit planes are the fp32 result rounded once.
(d) bn_finalize / bn_partial_sums / bn_finalize_sums around the steps of the two-stage reduction.  (e) fold_bn_3x3_packed on its
    own.  (f) one unit chained against ``F.batch_norm``.  (g) calls the wrappers or the library must refuse.

Every ``torch.equal`` against the reference asserts ``encoder_bn_ref.exact_margin`` first; every tolerance is a count of
roundings (U = 2^-24) written next to it or the bar of an existing test, none is measured."""
import math

import pytest
import torch
import torch.nn.functional as F

import encoder_bn_ref as br
import nonfinite_ref as nf

pytestmark = pytest.mark.gpu

U = br.U
NARROW = [torch.bfloat16, torch.float16]
FAMILIES = ("f32", "b3", "n16")


def _ops():
    from feature_vs_text_compound_emotion_amd import ops
    return ops


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _dev(t):
    return None if t is None else t.cuda()


def _split_of(t):
    """A ``Split`` on the GPU from the CPU restatement of the split (not from the kernel under test's sibling)."""
    hi, lo = nf.split_bf16(t)
    return _ops().Split(hi.bfloat16().cuda(), lo.bfloat16().cuda())


def _run(family, y, scale, shift, *, alpha=None, mask=None, res=None, res_stride=1, rs=None, rt=None, dtype=None, y_narrow=False,
         res_native=False, want_stats=True):
    """One launch of a wrapper with every output it has -> {name: CPU tensor}: 'y' (fp32), 'split.hi' / 'split.lo' (b3), 'n16'
    (narrow), 'stats'.  ``res_native``: the residual goes in as a Split (b3) or a narrow plane (n16) instead of fp32;
    ``y_narrow``: the narrow wrapper reads ``y`` from a narrow plane."""
    ops = _ops()
    kw = dict(alpha=_dev(alpha), mask=_dev(mask), res_stride=res_stride, res_scale=_dev(rs), res_shift=_dev(rt), want_stats=want_stats)
    if family == "f32":
        r = ops.bn_apply_nhwc(y.cuda(), scale.cuda(), shift.cuda(), res=_dev(res), **kw)
        out, stats = r if want_stats else (r, None)
        got = {"y": out}
    elif family == "b3":
        rr = None if res is None else (_split_of(res) if res_native else res.cuda())
        o = ops.bn_apply_nhwc_b3(y.cuda(), scale.cuda(), shift.cuda(), res=rr, out_f32=True, out_split=True, **kw)
        got, stats = {"y": o["y"], "split.hi": o["split"].hi.float(), "split.lo": o["split"].lo.float()}, o.get("stats")
    else:
        rr = None if res is None else (res.to(dtype).cuda() if res_native else res.cuda())
        o = ops.bn_apply_nhwc_n16((y.to(dtype) if y_narrow else y).cuda(), scale.cuda(), shift.cuda(), dtype=dtype, res=rr, out_f32=True,
                                  out_n16=True, **kw)
        assert o["n16"].dtype == dtype
        got, stats = {"y": o["y"], "n16": o["n16"].float()}, o.get("stats")
    if want_stats:
        got["stats"] = stats
    return {k: v.cpu() for k, v in got.items()}


def _assert_same_bits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what} [{k}]: a second launch gave other bits"


def _assert_exact(got, ref, p, what):
    """Every output of a launch on EXACT data equals the float64 reference; the precondition first."""
    bm = br.rows_per_block(p)
    assert br.exact_margin(ref, bm) < br.EXACT_LIMIT, what + ": the data do not meet the precondition of an exact comparison"
    c = ref.shape[-1]
    for name, t in got.items():
        if name == "stats":
            want = br.tile_rows(ref, bm)
            assert tuple(t.shape) == (br.tiles(p), 2, c) == tuple(want.shape), f"{what}: stats shape {tuple(t.shape)}"
            bad = (t.double() != want).nonzero()
            assert bad.numel() == 0, (f"{what} [stats]: {bad.shape[0]} of {want.numel()} per-tile sums differ, first (tile, sum / squares, "
                                      f"channel) = {tuple(bad[0].tolist())}")
        elif name == "split.lo":
            assert not t.any(), f"{what} [split.lo]: the value is a bfloat16 number, so the lo plane is zero"
        else:
            bad = (t.double() != ref).nonzero()
            assert bad.numel() == 0, f"{what} [{name}]: {bad.shape[0]} of {ref.numel()} values differ, first at {tuple(bad[0].tolist())}"


def _variants(d, native):
    """(name, keyword arguments of ``_run`` / of ``apply_ref``): the full epilogue and each part alone."""
    full = dict(alpha=d["alpha"], mask=d["mask"], res=d["res"], rs=d["rs"], rt=d["rt"])
    return [("full", dict(full, res_native=native)), ("alpha", dict(alpha=d["alpha"])), ("mask", dict(mask=d["mask"])),
            ("res", dict(res=d["res"])), ("res_affine", dict(res=d["res"], rs=d["rs"], rt=d["rt"], res_native=native)), ("plain", {})]


def _ref(d, kw, res_stride=1):
    return br.apply_ref(d["y"], d["scale"], d["shift"], alpha=kw.get("alpha"), mask=kw.get("mask"), res=kw.get("res"),
                        res_stride=res_stride, res_scale=kw.get("rs"), res_shift=kw.get("rt"))


# ================================================================================================ (a) bn_apply, exact
def _row_counts(c, per_thread):
    rpp = br.rows_per_pass(c, per_thread)
    return sorted({p for p in (1, rpp - 1, rpp + 1, 127, 128, 129, 300) if p > 0})


EXACT_F32 = [(c, p) for c in (4, 8, 16, 64, 128, 256, 512, 1024) for p in _row_counts(c, 4)]
EXACT_N16 = [(c, p) for c in (64, 128, 512, 2048) for p in _row_counts(c, 8)]


def _exact_case(family, c, p, dtype=None):
    n, ho, wo = br.factor_rows(p)
    d = br.exact_inputs(_gen(c, p, FAMILIES.index(family)), n, ho, wo, c)
    for name, kw in _variants(d, native=family != "f32"):
        ref, _ = _ref(d, kw)
        for y_narrow in ((False, True) if family == "n16" else (False,)):
            what = f"{family} C={c} P={p} ({n}x{ho}x{wo}) {name}" + (" y narrow" if y_narrow else "")
            got = _run(family, d["y"], d["scale"], d["shift"], dtype=dtype, y_narrow=y_narrow, **kw)
            _assert_exact(got, ref, p, what)
            if name == "full":
                _assert_same_bits(got, _run(family, d["y"], d["scale"], d["shift"], dtype=dtype, y_narrow=y_narrow, **kw), what)


@pytest.mark.parametrize("c,p", EXACT_F32)
def test_bn_apply_fp32_exact(c, p):
    _exact_case("f32", c, p)


@pytest.mark.parametrize("c,p", EXACT_F32)
def test_bn_apply_b3_exact(c, p):
    _exact_case("b3", c, p)


@pytest.mark.parametrize("dtype", NARROW, ids=["bf16", "fp16"])
@pytest.mark.parametrize("c,p", EXACT_N16)
def test_bn_apply_n16_exact(c, p, dtype):
    _exact_case("n16", c, p, dtype)


BIG_P = 264193                                           # the first row counts with 256-row statistics tiles start at 264192


def test_bn_apply_fp32_exact_at_256_row_tiles():
    assert br.rows_per_block(BIG_P) == 256 and br.rows_per_block(BIG_P - 2) == 128
    n, ho, wo = br.factor_rows(BIG_P)
    d = br.exact_inputs(_gen(BIG_P), n, ho, wo, 16)
    kw = _variants(d, False)[0][1]
    ref, _ = _ref(d, kw)
    _assert_exact(_run("f32", d["y"], d["scale"], d["shift"], **kw), ref, BIG_P, f"f32 C=16 P={BIG_P}")


def test_bn_apply_n16_exact_at_256_row_tiles():
    n, ho, wo = br.factor_rows(BIG_P)
    d = br.exact_inputs(_gen(BIG_P, 1), n, ho, wo, 64)
    kw = _variants(d, True)[0][1]
    ref, _ = _ref(d, kw)
    _assert_exact(_run("n16", d["y"], d["scale"], d["shift"], dtype=torch.bfloat16, y_narrow=True, **kw), ref, BIG_P, f"n16 C=64 P={BIG_P}")


# ================================================================================================ (b) residual geometry, exact
GEOMETRY = [(2, 5, 9), (2, 6, 10), (2, 5, 10), (1, 4, 5), (3, 7, 13)]         # (stride, Hr, Wr) for N = 3, (Ho, Wo) = (3, 5)
RES_FORMS = [("f32", None, False), ("b3", None, False), ("b3", None, True), ("n16", torch.bfloat16, True), ("n16", torch.float16, True),
             ("n16", torch.float16, False)]


@pytest.mark.parametrize("family,dtype,native", RES_FORMS, ids=[f"{f}_{'native' if nat else 'fp32res'}{'' if dt is None else '_' + str(dt)[6:]}"
                                                                  for f, dt, nat in RES_FORMS])
@pytest.mark.parametrize("stride,hr,wr", GEOMETRY)
def test_bn_apply_reads_the_strided_residual_and_nothing_else(stride, hr, wr, family, dtype, native):
    n, ho, wo, c = 3, 3, 5, 64
    d = br.exact_inputs(_gen(stride, hr, wr), n, ho, wo, c, res_hw=(hr, wr))
    wanted = torch.zeros(n, hr, wr, 1, dtype=torch.bool)
    wanted[:, 0:(ho - 1) * stride + 1:stride, 0:(wo - 1) * stride + 1:stride] = True
    assert int(wanted.sum()) == n * ho * wo and int((~wanted).sum()) > 0
    d["res"] = torch.where(wanted, d["res"], torch.full_like(d["res"], float("nan")))      # read one of these and the sum is NaN
    for name, kw in _variants(d, native)[:1] + _variants(d, native)[3:5]:
        kw = dict(kw, res_native=native)
        ref, _ = _ref(d, kw, stride)
        assert torch.isfinite(ref).all()
        got = _run(family, d["y"], d["scale"], d["shift"], dtype=dtype, res_stride=stride, **kw)
        _assert_exact(got, ref, n * ho * wo, f"{family} residual {hr}x{wr} / {stride} {name}")


# ================================================================================================ (c) bn_apply, random
def _random_inputs(c, seed):
    g = _gen(c, seed)
    n, ho, wo = 2, 10, 15                                                     # P = 300: three statistics tiles, the last of 44 rows
    d = {"y": torch.randn(n, ho, wo, c, generator=g), "res": torch.randn(n, ho, wo, c, generator=g),
         "scale": torch.rand(c, generator=g) + 0.5, "shift": torch.randn(c, generator=g), "alpha": torch.rand(c, generator=g) * 0.3 + 0.1,
         "rs": -(torch.rand(c, generator=g) + 0.5), "rt": torch.randn(c, generator=g),
         "mask": (torch.rand(n, ho, wo, c, generator=g) > 0.3).float() * 2.0}
    d["scale"][::3] *= -1.0
    return d


def _check_random(got, d, what):
    ref, bound = br.apply_ref(d["y"], d["scale"], d["shift"], alpha=d["alpha"], mask=d["mask"], res=d["res"], res_scale=d["rs"],
                              res_shift=d["rt"])
    y = got["y"]
    ratio = ((y.double() - ref).abs() / bound).max().item()
    print(f"{what}: fp32 output at {ratio:.3f} of the bound")
    assert ratio <= 1.0, f"{what} [y]: {ratio:.2f} of the bound"
    for name, want in (("split.hi", lambda: nf.split_bf16(y)[0]), ("split.lo", lambda: nf.split_bf16(y)[1]),
                       ("n16", lambda: nf.round_to(y, got["n16_dtype"]))):
        if name in got:
            assert nf.nan_equal(got[name], want()), f"{what} [{name}] is not the fp32 output rounded once: {nf.describe_mismatch(got[name], want())}"
    # the statistics: sums of the FINAL fp32 value.  A tile of r rows adds r values (r - 1 roundings, each at most U of the sum
    # of magnitudes); the squares round once more before they are added.
    st, o = got["stats"].double(), y.double()
    p, c = o.numel() // o.shape[-1], o.shape[-1]
    bm = br.rows_per_block(p)
    assert tuple(st.shape) == (br.tiles(p), 2, c)
    for t, blk in enumerate(o.reshape(p, c).split(bm)):
        rows = blk.shape[0]
        e1, b1 = (st[t, 0] - blk.sum(0)).abs(), rows * U * blk.abs().sum(0)
        e2, b2 = (st[t, 1] - (blk * blk).sum(0)).abs(), rows * U * (blk * blk).sum(0)
        print(f"{what}: tile {t} ({rows} rows) sums at {(e1 / b1).max().item():.3f}, squares at {(e2 / b2).max().item():.3f} of the bound")
        assert (e1 <= b1).all() and (e2 <= b2).all(), f"{what}: statistics of tile {t}"


@pytest.mark.parametrize("c", [64, 256])
def test_bn_apply_fp32_random(c):
    d = _random_inputs(c, 0)
    got = _run("f32", d["y"], d["scale"], d["shift"], alpha=d["alpha"], mask=d["mask"], res=d["res"], rs=d["rs"], rt=d["rt"])
    _check_random(got, d, f"bn_apply_nhwc C={c}")


@pytest.mark.parametrize("native", [False, True], ids=["fp32res", "splitres"])
@pytest.mark.parametrize("c", [64, 256])
def test_bn_apply_b3_random(c, native):
    d = _random_inputs(c, 1)
    got = _run("b3", d["y"], d["scale"], d["shift"], alpha=d["alpha"], mask=d["mask"], res=d["res"], rs=d["rs"], rt=d["rt"], res_native=native)
    if native:                                             # the reference from the residual the kernel is given: hi + lo
        hi, lo = nf.split_bf16(d["res"])
        d["res"] = hi.double() + lo.double()
    _check_random(got, d, f"bn_apply_nhwc_b3 C={c} {'split' if native else 'fp32'} residual")


@pytest.mark.parametrize("y_narrow", [False, True], ids=["y32", "y16"])
@pytest.mark.parametrize("dtype", NARROW, ids=["bf16", "fp16"])
@pytest.mark.parametrize("c", [64, 256])
def test_bn_apply_n16_random(c, dtype, y_narrow):
    d = _random_inputs(c, 2)
    got = _run("n16", d["y"], d["scale"], d["shift"], alpha=d["alpha"], mask=d["mask"], res=d["res"], rs=d["rs"], rt=d["rt"], dtype=dtype,
               y_narrow=y_narrow, res_native=True)
    got["n16_dtype"] = dtype
    d["res"] = nf.round_to(d["res"], dtype)                # the reference from the rounded operands
    if y_narrow:
        d["y"] = nf.round_to(d["y"], dtype)
    _check_random(got, d, f"bn_apply_nhwc_n16 C={c} {dtype} y {'narrow' if y_narrow else 'fp32'}")


# ================================================================================================ (d) bn_finalize and its two halves
MOMENTUM, EPS = 0.1, 1e-5
ROWS = 4                                                  # rows behind each synthetic partial


def _partials(tiles, c, g):
    x = torch.randn(tiles, ROWS, c, generator=g) * 2.0 + 3.0
    return torch.stack([x.sum(1), (x * x).sum(1)], dim=1).contiguous()        # [tiles, 2, C] float32


def _check_finalize(partials, count, gamma, beta, rm0, rv0, scale_ulps, what):
    """Both routes on the GPU against ``finalize_ref`` from the same partials.  Bars of tests/test_conv_fp32_edges_gpu.py:
    ``scale_ulps`` U on scale (2: one rounding of 1 / sqrt and an exact product with a power of two; 3: a rounded product),
    8 U of the summed magnitudes on the results of two fp32 terms; tests/test_sync_bn_gpu.py: 1e-12 on the float64 sums."""
    ops = _ops()
    dev = (lambda t: None if t is None else t.clone().cuda())
    rm_a, rv_a, rm_b, rv_b = dev(rm0), dev(rv0), dev(rm0), dev(rv0)
    pg, gg, bg = partials.cuda(), gamma.cuda(), beta.cuda()
    s_a, t_a = ops.bn_finalize(pg, count, gg, bg, rm_a, rv_a, momentum=MOMENTUM, eps=EPS)
    sums = ops.bn_partial_sums(pg)
    s_b, t_b = ops.bn_finalize_sums(sums, count, gg, bg, rm_b, rv_b, momentum=MOMENTUM, eps=EPS)
    ref = br.finalize_ref(partials, count, gamma, beta, rm0, rv0, MOMENTUM, EPS)
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (2, partials.shape[2])
    assert ((sums.cpu() - ref["sums"]).abs() <= 1e-12 * ref["sums"].abs().clamp_min(1.0)).all(), what + ": sums"
    pairs = [(s_a, s_b, "scale"), (t_a, t_b, "shift")] + ([(rm_a, rm_b, "running_mean"), (rv_a, rv_b, "running_var")] if rm0 is not None else [])
    for a, b, name in pairs:
        assert torch.equal(a, b), f"{what}: {name} of the two routes differs"
    s, t = s_a.cpu().double(), t_a.cpu().double()
    assert ((s - ref["scale"]).abs() <= scale_ulps * U * ref["scale"].abs()).all(), \
        f"{what}: scale at {((s - ref['scale']).abs() / (U * ref['scale'].abs().clamp_min(1e-300))).max().item():.2f} U"
    assert ((t - ref["shift"]).abs() <= 8 * U * (beta.double().abs() + (ref["mean"] * ref["scale"]).abs())).all(), what + ": shift"
    if rm0 is not None:
        assert ((rm_a.cpu().double() - ref["rm"]).abs() <= 8 * U * (rm0.double().abs() + ref["mean"].abs())).all(), what + ": running_mean"
        assert ((rv_a.cpu().double() - ref["rv"]).abs() <= 8 * U * (rv0.double().abs() + ref["unbiased"].abs())).all(), what + ": running_var"
    return s, t, ref


def _affine(c, g, pow2):
    gamma = br.pick(g, (c,), [0.5, 1.0, 2.0, -1.0]) if pow2 else torch.rand(c, generator=g) + 0.5
    return gamma, torch.randn(c, generator=g), torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5


@pytest.mark.parametrize("c", [1, 3, 64, 130, 2048])
@pytest.mark.parametrize("tiles", [1, 2, 511, 512, 513, 1023, 1024, 1025, 4097])
def test_bn_finalize_around_the_steps_of_its_reduction(tiles, c):
    g = _gen(tiles, c)
    partials = _partials(tiles, c, g)
    for pow2 in (True, False):
        gamma, beta, rm0, rv0 = _affine(c, g, pow2)
        _check_finalize(partials, tiles * ROWS, gamma, beta, rm0, rv0, 2 if pow2 else 3, f"tiles={tiles} C={c} pow2={pow2}")


def test_bn_finalize_of_a_single_value_per_channel():
    c = 130
    g = _gen(1, c)
    x = torch.randn(1, 1, c, generator=g) * 2.0 + 3.0
    partials = torch.stack([x.sum(1), (x * x).sum(1)], dim=1).contiguous()
    gamma, beta, rm0, rv0 = _affine(c, g, True)
    _, _, ref = _check_finalize(partials, 1, gamma, beta, rm0, rv0, 2, "count == 1")
    assert torch.equal(ref["unbiased"], ref["var"]) and torch.isfinite(ref["rv"]).all()     # no division by count - 1 = 0


@pytest.mark.parametrize("tiles", [2, 513])
def test_bn_finalize_with_a_count_that_is_not_tiles_times_rows(tiles):
    c = 64
    g = _gen(tiles, c, 7)
    partials = _partials(tiles, c, g)
    gamma, beta, rm0, rv0 = _affine(c, g, False)
    _check_finalize(partials, tiles * ROWS - 3, gamma, beta, rm0, rv0, 3, f"count = {tiles * ROWS - 3}")


def test_bn_finalize_without_running_buffers():
    c = 130
    g = _gen(9, c)
    partials = _partials(7, c, g)
    gamma, beta, rm0, rv0 = _affine(c, g, False)
    s0, t0, _ = _check_finalize(partials, 7 * ROWS, gamma, beta, None, None, 3, "no running buffers")
    s1, t1, _ = _check_finalize(partials, 7 * ROWS, gamma, beta, rm0, rv0, 3, "running buffers")
    assert torch.equal(s0, s1) and torch.equal(t0, t1)


def test_bn_finalize_with_zero_and_negative_gamma():
    c = 64
    g = _gen(11, c)
    partials = _partials(5, c, g)
    gamma, beta, rm0, rv0 = _affine(c, g, False)
    gamma[::4] = 0.0
    gamma[1::4] *= -1.0
    s, t, _ = _check_finalize(partials, 5 * ROWS, gamma, beta, rm0, rv0, 3, "gamma zero / negative")
    assert not s[::4].any() and torch.equal(t[::4], beta[::4].double())          # scale 0, shift beta, exactly
    assert (s[1::4] < 0).all() and (s[2::4] > 0).all()


def test_bn_finalize_of_constant_channels():
    """Channels that hold one value v: the variance is 0 and scale = gamma / sqrt(eps).  v = 3.0 cancels exactly.  For v = 0.1
    and its like the partial sum of squares is 8 fl(v^2), off from 8 v^2 by the float32 rounding of the square, so the float64
    expression s2 / count - mean^2 comes out as +-1e-9 v^2: where it is negative the clamp has to send it to 0 (unclamped, the
    scale would move by |var| / (2 eps), hundreds of U).  There 4 U: the rounding of 1 / sqrt, the product with gamma, the
    float32 eps.  Where it is positive, ``finalize_ref`` from the same partials is the bar, as everywhere."""
    vals = torch.tensor([3.0, 0.1, 0.2, 0.3, 0.7, 1.1, 1.3, 1.7, 2.3, 5.1], dtype=torch.float32)
    c, tiles, rows = vals.numel(), 3, 8
    partials = torch.stack([rows * vals, rows * (vals * vals)]).expand(tiles, 2, c).contiguous()
    count = tiles * rows
    raw_var = (partials.double().sum(0)[1] / count) - (partials.double().sum(0)[0] / count) ** 2
    assert raw_var[0] == 0.0 and raw_var.abs().max().item() < 1e-6 and (raw_var < 0).sum() >= 2 and (raw_var > 0).sum() >= 2
    g = _gen(13)
    gamma, beta, rm0, rv0 = _affine(c, g, False)
    s, _, ref = _check_finalize(partials, count, gamma, beta, rm0, rv0, 3, "constant channels")
    clamped = raw_var <= 0
    assert not ref["var"][clamped].any()
    want = gamma.double() / math.sqrt(br.f32(EPS))
    assert ((s - want).abs() <= 4 * U * want.abs())[clamped].all()


# ================================================================================================ (e) fold_bn_3x3_packed
def _poison_next_allocations(shape, dtype, blocks=1):
    """Fill ``blocks`` blocks of the output's size with NaN and free them: the allocator is likely to hand the same blocks to the call."""
    junk = [torch.full(shape, float("nan"), device="cuda", dtype=dtype) for _ in range(blocks)]
    torch.cuda.synchronize()
    del junk


@pytest.mark.parametrize("cout", [1, 5, 64])
@pytest.mark.parametrize("cin", [1, 3, 32, 100, 320])
def test_fold_bn_3x3_packed_on_its_own(cin, cout):
    ops = _ops()
    g = _gen(cin, cout)
    w = torch.randn(cout, cin, 3, 3, generator=g)
    s, t = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g)
    s[::2] *= -1.0
    kpad = br.kpad_3x3(cin)
    assert kpad == ops.conv_kpad(3, 3, cin) and (kpad - 9 * cin) == {1: 23, 3: 5, 32: 0, 100: 28, 320: 0}[cin]
    wp = br.pack_3x3(w, fill=7.0)                                               # padding columns of the INPUT are not zero
    prod = wp[:, :9 * cin] * s.repeat(9)                                        # one IEEE multiply per weight, float32
    pad = torch.zeros(cout, kpad - 9 * cin)
    wg, sg, tg = wp.cuda(), s.cuda(), t.cuda()                                  # before the poison: they must not take its blocks
    outs = {}
    for form, dt in (("f32", torch.float32), ("split", torch.bfloat16), (torch.bfloat16, torch.bfloat16), (torch.float16, torch.float16)):
        _poison_next_allocations((cout, kpad), dt, blocks=2 if form == "split" else 1)
        outs[form] = ops.fold_bn_3x3_packed(wg, sg, tg, form)
    wf = outs["f32"][0].cpu()
    assert torch.equal(wf[:, :9 * cin], prod) and torch.equal(wf[:, 9 * cin:], pad), "f32: not the single product, or a padding column is not 0"
    hi, lo = nf.split_bf16(prod)
    sp = outs["split"][0]
    assert torch.equal(sp.hi.float().cpu()[:, :9 * cin], hi) and torch.equal(sp.lo.float().cpu()[:, :9 * cin], lo), "split planes"
    assert torch.equal(sp.hi.float().cpu()[:, 9 * cin:], pad) and torch.equal(sp.lo.float().cpu()[:, 9 * cin:], pad), "split padding"
    for dt in NARROW:
        wn = outs[dt][0]
        assert wn.dtype == dt
        assert torch.equal(wn.float().cpu()[:, :9 * cin], nf.round_to(prod, dt)), f"{dt}: not the product rounded once"
        assert torch.equal(wn.float().cpu()[:, 9 * cin:], pad), f"{dt} padding"
    # bias9: a run of ceil(Cin / 256) products per thread, an 8-level tree over the 256 threads, up to 9 taps: that many
    # roundings, each at most U of the sum of |w| |t| over the taps of the case
    _, b9_ref = br.fold_ref(w, s, t)
    _, b9_mag = br.fold_ref(w.abs(), s, t.abs())
    b9 = outs["f32"][1].cpu()
    assert tuple(b9.shape) == (9, cout)
    bound = (math.ceil(cin / 256) + 8 + 9) * U * b9_mag
    err = (b9.double() - b9_ref).abs()
    assert (err <= bound).all(), f"bias9 at {(err / bound).max().item():.2f} of the bound in case {int((err / bound).argmax()) // cout}"
    for form in ("split", torch.bfloat16, torch.float16):
        assert torch.equal(outs[form][1].cpu(), b9), f"bias9 of the {form} form differs from the fp32 form's"


# ================================================================================================ (f) one unit chained
def test_apply_statistics_finalize_apply_is_batch_norm_of_the_first_result():
    """y -> bn_apply(want_stats) -> bn_finalize -> bn_apply against float64 F.batch_norm(training=True) of the first result x.
    The bar is the sum of the stages' bounds.  Statistics (c): the tile's sums are off by at most r U sum|x| and r U sum x^2
    (r = 60 rows, one tile), which moves the mean by dm and the variance by dv = d(E x^2) + 2 |mean| dm + dm^2, hence scale by
    ds = |s| dv / (2 (var + eps)) (1.01: second order) and shift by |s| dm + |mean| ds.  Finalize (d): 3 U |s| on scale,
    8 U (|beta| + |mean s|) on shift, 8 U of the summed magnitudes on the buffers.  Apply (c): ``apply_ref``'s bound."""
    ops = _ops()
    n, ho, wo, c = 2, 6, 5, 64
    p = n * ho * wo
    g = _gen(2, 6, 5, 64)
    y = torch.randn(n, ho, wo, c, generator=g) * 2.0 + 1.0
    sc0, sh0, al0 = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g), torch.rand(c, generator=g) * 0.3 + 0.1
    gamma, beta, rm0, rv0 = _affine(c, g, False)
    x32, stats = ops.bn_apply_nhwc(y.cuda(), sc0.cuda(), sh0.cuda(), alpha=al0.cuda(), want_stats=True)
    assert tuple(stats.shape) == (1, 2, c)
    rm, rv = rm0.clone().cuda(), rv0.clone().cuda()
    scale, shift = ops.bn_finalize(stats, p, gamma.cuda(), beta.cuda(), rm, rv, momentum=MOMENTUM, eps=EPS)
    z = ops.bn_apply_nhwc(x32, scale, shift).cpu().double()
    x = x32.cpu().double()
    mom, eps = br.f32(MOMENTUM), br.f32(EPS)
    rm_ref, rv_ref = rm0.double().clone(), rv0.double().clone()
    want = F.batch_norm(x.permute(0, 3, 1, 2), rm_ref, rv_ref, gamma.double(), beta.double(), True, mom, eps).permute(0, 2, 3, 1)
    x2 = x.reshape(p, c)
    mean, ex2 = x2.sum(0) / p, (x2 * x2).sum(0) / p
    var = ex2 - mean * mean
    s = gamma.double() / torch.sqrt(var + eps)
    r = p                                                                     # rows of the one statistics tile
    dm = r * U * x2.abs().sum(0) / p
    dv = r * U * (x2 * x2).sum(0) / p + 2 * mean.abs() * dm + dm * dm
    ds_stats = 1.01 * s.abs() * dv / (2 * (var + eps))
    ds = 3 * U * s.abs() + ds_stats
    dt = 8 * U * (beta.double().abs() + (mean * s).abs()) + s.abs() * dm + mean.abs() * ds_stats
    _, b_apply = br.apply_ref(x32.cpu(), scale.cpu(), shift.cpu())
    bound = x.abs() * ds + dt + b_apply
    err = (z - want).abs()
    print(f"chained unit: output at {(err / bound).max().item():.3f} of the bound")
    assert (err <= bound).all(), f"{(err / bound).max().item():.2f} of the bound"
    unbiased = var * p / (p - 1)
    assert ((rm.cpu().double() - rm_ref).abs() <= 8 * U * (rm0.double().abs() + mean.abs()) + mom * dm).all()
    assert ((rv.cpu().double() - rv_ref).abs() <= 8 * U * (rv0.double().abs() + unbiased.abs()) + mom * dv * p / (p - 1)).all()


# ================================================================================================ (g) rejected calls
# Every mismatched tensor is LARGER than what the kernel would touch: a wrapper that let the call through would still read in bounds.
def _apply_call(family, y, c, **kw):
    ops = _ops()
    v = torch.ones(c, device="cuda")
    if family == "f32":
        return ops.bn_apply_nhwc(y, v, v, **kw)
    if family == "b3":
        return ops.bn_apply_nhwc_b3(y, v, v, **kw)
    return ops.bn_apply_nhwc_n16(y, v, v, dtype=torch.bfloat16, **kw)


def test_bn_finalize_refuses_mismatched_shapes():
    ops = _ops()
    tiles, c = 4, 64
    v = torch.ones(c, device="cuda")
    good = torch.ones(tiles, 2, c, device="cuda")
    ops.bn_finalize(good, 8, v, v)                                             # the call itself is fine
    with pytest.raises(ValueError, match="partials"):
        ops.bn_finalize(torch.ones(tiles, 3, c, device="cuda"), 8, v, v)
    long = torch.ones(c + 4, device="cuda")
    with pytest.raises(ValueError, match="gamma"):
        ops.bn_finalize(good, 8, long, v)
    with pytest.raises(ValueError, match="beta"):
        ops.bn_finalize(good, 8, v, long)
    with pytest.raises(ValueError, match="running_var"):
        ops.bn_finalize(good, 8, v, v, v.clone(), long)
    with pytest.raises(RuntimeError, match="bn_finalize"):                     # the library's own check
        ops.bn_finalize(good, 8, v, v, running_mean=v.clone())


@pytest.mark.parametrize("family", FAMILIES)
def test_bn_apply_refuses_a_residual_of_other_images_or_channels(family):
    n, ho, wo, c = 2, 3, 5, 64
    y = torch.zeros(n, ho, wo, c, device="cuda")
    _apply_call(family, y, c, res=torch.zeros(n, ho, wo, c, device="cuda"))    # the call itself is fine
    with pytest.raises(ValueError, match="res shape"):
        _apply_call(family, y, c, res=torch.zeros(n + 1, ho, wo, c, device="cuda"))
    with pytest.raises(ValueError, match="res shape"):
        _apply_call(family, y, c, res=torch.zeros(n, ho, wo, 2 * c, device="cuda"))
    native = {"f32": None, "b3": _split_of(torch.zeros(n + 1, ho, wo, c)), "n16": torch.zeros(n + 1, ho, wo, c, device="cuda", dtype=torch.bfloat16)}[family]
    if native is not None:
        with pytest.raises(ValueError, match="res shape"):
            _apply_call(family, y, c, res=native)


def test_the_library_refuses_channel_counts_and_geometry_it_cannot_run():
    with pytest.raises(RuntimeError, match=r"C must be 4\.\.1024"):
        _apply_call("f32", torch.zeros(2, 3, 5, 20, device="cuda"), 20)
    for c in (72, 32):
        with pytest.raises(RuntimeError, match=r"C must be 64\.\.2048"):
            _apply_call("n16", torch.zeros(2, 3, 5, c, device="cuda"), c)
    n, ho, wo, c = 2, 3, 5, 64
    y = torch.zeros(n, ho, wo, c, device="cuda")
    for family in FAMILIES:
        for hr, wr in ((4, 10), (6, 8)):                                       # (Ho - 1) 2 = 4 >= Hr; (Wo - 1) 2 = 8 >= Wr
            with pytest.raises(RuntimeError, match="residual geometry"):
                _apply_call(family, y, c, res=torch.zeros(n, hr, wr, c, device="cuda"), res_stride=2)
        with pytest.raises(RuntimeError, match="residual geometry"):
            _apply_call(family, y, c, res=torch.zeros(n, ho, wo, c, device="cuda"), res_stride=0)
