"""NaN / Inf propagation and batch isolation of the kernels, pinned to torch ("Non-finite values").

A. conv families: one poisoned input element; the non-finite outputs are the reference's, everything else is bit-identical to
   the clean launch.  B. the same for the epilogue's inputs (residual, statistics).  C. the activation table through the conv
   epilogues.  D. elementwise and row passes against the tables of nonfinite_ref.py.  E. whole encoders and LFAN in eval mode:
   a poisoned batch item never changes its neighbours.

The references, masks and tables come from tests/nonfinite_ref.py and are validated without a GPU by
tests/test_nonfinite_ref_cpu.py.  Nothing here has a tolerance except the finite values of GELU (erff) and the sanity check
that a clean launch computes the conv at all."""
import pytest
import torch
import torch.nn.functional as F

import nonfinite_ref as nf
from encoder_bn_ref import bn_apply_ref as _bn_apply_ref

pytestmark = pytest.mark.gpu

NARROW = [torch.bfloat16, torch.float16]
NAN, INF = nf.NAN, nf.INF


def _ops():
    from feature_vs_text_compound_emotion_amd import ops
    return ops


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _same(got, want, what, ignore_zero_sign=True):
    assert nf.nan_equal(got, want, ignore_zero_sign=ignore_zero_sign), f"{what}: {nf.describe_mismatch(got, want)}"


def _bits_equal(got, want, what):
    """``torch.equal`` with a message (finite data: no NaN on either side is expected to compare equal)."""
    g, w = got.detach().cpu(), want.detach().cpu()
    assert torch.equal(g, w), f"{what}: {nf.describe_mismatch(g, w)}"


# ================================================================================================ A. conv families
def _conv_launcher(case, w, dtype, **kw):
    """(run, post): ``run(x_cpu_nhwc)`` launches the case and returns {name: CPU tensor [n, ho, wo, cout]}; ``post`` maps the
    float64 conv reference to what the launch computes (the stem's affine + PReLU).  ``exact``: the outputs whose non-finite
    VALUES must equal the reference's (fp32 and narrow paths)."""
    ops = _ops()
    p, k, s = case.k // 2, case.k, case.stride
    post = (lambda ref: ref)
    if case.path == "fp32":
        wp = ops.pack_conv_weight(w.cuda())

        def run(x):
            r = ops.conv2d(x.cuda(), wp, k, k, stride=s, pad=(p, p), tile=case.tile, out_split=True, **kw)
            h = ops.conv2d(x.cuda(), wp, k, k, stride=s, pad=(p, p), tile=case.tile, out_n16=torch.float16, **kw)
            _bits_equal(h["y"].view(torch.int32), r["y"].view(torch.int32), f"{case.name}: y with a narrow instead of a split copy")
            return {"y": r["y"].cpu(), "split.hi": r["split"].hi.float().cpu(), "split.lo": r["split"].lo.float().cpu(),
                    "n16": h["n16"].float().cpu()}
        exact = ("y", "split.hi", "n16")
    elif case.path == "stem":
        g = _gen(3)
        scale, shift, alpha = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.3, torch.rand(64, generator=g) * 0.3 + 0.1
        wp = ops.pack_conv_weight(w.cuda())

        def run(x):
            xd = x.permute(0, 3, 1, 2).contiguous().cuda()
            args = (xd, wp, scale.cuda(), shift.cuda(), alpha.cuda())
            sp = ops.stem_conv(*args, out="split")["split"]
            return {"y": ops.stem_conv(*args, out="f32")["y"].cpu(), "split.hi": sp.hi.float().cpu(), "split.lo": sp.lo.float().cpu(),
                    "n16": ops.stem_conv(*args, out=torch.float16)["n16"].float().cpu()}

        def post(ref):
            z = ref * scale.double() + shift.double()
            return nf.prelu(z, alpha.double())
        exact = ("y", "split.hi", "n16")
    elif case.path == "b3":
        ws = ops.split_bf16(ops.pack_conv_weight(w.cuda()))
        if case.s2d:
            ws = ops.pack_s2d_weight(ws, case.cin)

        def run(x):
            xs = ops.split_bf16(x.cuda())
            if case.s2d:
                xs = ops.space_to_depth(xs)
            r = ops.conv2d_b3(xs, ws, k, k, stride=s, pad=(p, p), tile=case.tile, out_f32=True, out_split=True, x_s2d=case.s2d, **kw)
            return {"y": r["y"].cpu(), "split.hi": r["split"].hi.float().cpu(), "split.lo": r["split"].lo.float().cpu()}
        exact = ()                                   # bf16x3: split(inf) = (inf, nan), only "non-finite" is required
    else:
        wd = ops.to_n16(ops.pack_conv_weight(w.cuda()), dtype)          # exact: w is already rounded
        if case.s2d:
            wd = ops.pack_s2d_weight(wd, case.cin)
        both = case.tile != 79                        # the persistent kernel takes the specialised (one-output) epilogues only

        def run(x):
            xd = x.to(dtype).cuda()                   # exact for the clean values; inf / nan stay what they are
            if case.s2d:
                xd = ops.space_to_depth(xd)
            r = ops.conv2d_n16(xd, wd, k, k, stride=s, pad=(p, p), tile=case.tile, out_f32=both, out_n16=True, x_s2d=case.s2d, **kw)
            out = {"n16": r["n16"].float().cpu()}
            if both:
                out["y"] = r["y"].cpu()
                _same(r["n16"].float(), r["y"].to(dtype).float(), f"{case.name}: the narrow output is the fp32 one rounded once")
            return out
        exact = ("y", "n16")
    return run, post, exact


def _run_conv_case(case, dtype=None):
    x, w = nf.make_conv(case, dtype)
    run, post, exact = _conv_launcher(case, w, dtype)
    clean = run(x)
    ref = post(nf.clean_reference(case, dtype))
    for name, t in clean.items():
        assert tuple(t.shape) == tuple(ref.shape) and torch.isfinite(t).all(), name
    main = clean["y"] if "y" in clean else clean["n16"]
    assert ((main.double() - ref).abs() <= 2.0 ** -7 * ref.abs() + 1e-3).all(), "the clean launch is not the conv"
    for label, where in nf.poisons(case):
        for vname, _ in nf.POISON_VALUES:
            p = nf.poison_reference(case, where, vname, dtype)
            nf.check_poisoned(run(p.x), clean, p.ref_mask, post(p.ref), vname, exact, f"{case.name} poison ({label}) {vname} at {where}")


@pytest.mark.parametrize("case", nf.FP32 + nf.STEM, ids=lambda c: c.name)
def test_conv_fp32_poison_stays_in_its_receptive_field(case):
    _run_conv_case(case)


@pytest.mark.parametrize("case", nf.B3, ids=lambda c: c.name)
def test_conv_b3_poison_stays_in_its_receptive_field(case):
    _run_conv_case(case)


@pytest.mark.parametrize("dtype", NARROW, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", nf.N16, ids=lambda c: c.name)
def test_conv_n16_poison_stays_in_its_receptive_field(case, dtype):
    _run_conv_case(case, dtype)


# ================================================================================================ B. epilogue inputs
# one flat, one window and one patch tile per path (the fp32 path has flat tiles only)
EPI_CASES = ([nf.conv_case("fp32", 5, 3, 32, 36, 7, 7)] +
             [nf.conv_case("b3", 42, 3, 64, 96, 7, 7), nf.conv_case("b3", 56, 3, 64, 128, 13, 21), nf.conv_case("b3", 58, 3, 64, 100, 32, 32)] +
             [nf.conv_case("n16", 64, 3, 64, 96, 7, 7), nf.conv_case("n16", 76, 3, 64, 128, 13, 21), nf.conv_case("n16", 72, 3, 64, 100, 32, 32)])
EPI_PARAMS = [(c, d) for c in EPI_CASES for d in (NARROW if c.path == "n16" else [None])]
_epi_ids = [c.name + ("" if d is None else "_" + str(d).split(".")[1]) for c, d in EPI_PARAMS]


def _epi_run(case, dtype, x, w, *, out_f32, **kw):
    """One launch with the 16-bit output of the path (and the fp32 one with ``out_f32``); residual / bias as given in kw."""
    ops = _ops()
    p, k = case.k // 2, case.k
    if case.path == "fp32":
        r = ops.conv2d(x.cuda(), ops.pack_conv_weight(w.cuda()), k, k, pad=(p, p), tile=case.tile, **kw)
        if isinstance(r, tuple):
            return {"y": r[0].cpu(), "stats": r[1]}
        return {"y": r.cpu()}
    if case.path == "b3":
        r = ops.conv2d_b3(ops.split_bf16(x.cuda()), ops.split_bf16(ops.pack_conv_weight(w.cuda())), k, k, pad=(p, p), tile=case.tile,
                          out_f32=out_f32, out_split=True, **kw)
        out = {"split.hi": r["split"].hi.float().cpu(), "split.lo": r["split"].lo.float().cpu()}
    else:
        r = ops.conv2d_n16(x.to(dtype).cuda(), ops.to_n16(ops.pack_conv_weight(w.cuda()), dtype), k, k, pad=(p, p), tile=case.tile,
                           out_f32=out_f32, out_n16=True, **kw)
        out = {"n16": r["n16"].float().cpu()}
    if out_f32:
        out["y"] = r["y"].cpu()
    if "stats" in r:
        out["stats"] = r["stats"]
    return out


def _residual(case, dtype, res):
    ops = _ops()
    if case.path == "b3":
        return ops.split_bf16(res.cuda())
    return res.cuda() if case.path == "fp32" else res.to(dtype).cuda()


@pytest.mark.parametrize("value", [NAN, INF], ids=["nan", "inf"])
@pytest.mark.parametrize("case,dtype", EPI_PARAMS, ids=_epi_ids)
def test_residual_poison_reaches_exactly_its_output(case, dtype, value):
    """bias + same-geometry residual, 16-bit output only: the specialised row epilogue of the 16-bit paths.  One residual
    element is poisoned: exactly that output element is non-finite; NaN gives NaN; the fp32 and narrow paths keep +inf."""
    x, w = nf.make_conv(case, dtype)
    g = _gen(11)
    bias = torch.randn(case.cout, generator=g)
    res = torch.randn(case.n, case.h, case.w, case.cout, generator=g)
    if dtype is not None:
        res = nf.round_to(res, dtype)
    where = (1, case.h - 1, 0, 5)
    bad = nf.poisoned(res, where, value)
    kw = dict(out_f32=False, bias=bias.cuda())
    clean = _epi_run(case, dtype, x, w, residual=_residual(case, dtype, res), **kw)
    got = _epi_run(case, dtype, x, w, residual=_residual(case, dtype, bad), **kw)
    mask = torch.zeros(case.n, case.h, case.w, case.cout, dtype=torch.bool)
    mask[where] = True
    for name, t in got.items():
        assert torch.isfinite(clean[name]).all()
        assert torch.equal(~torch.isfinite(t), mask), f"{case.name} [{name}]: the non-finite set is not the poisoned element"
        if value != value:
            assert torch.isnan(t[where])
        elif case.path != "b3" and name != "split.lo":
            assert t[where] == INF
        _bits_equal(t[~mask], clean[name][~mask], f"{case.name} [{name}] vs the clean launch")


@pytest.mark.parametrize("value", [NAN, INF], ids=["nan", "inf"])
@pytest.mark.parametrize("case,dtype", EPI_PARAMS, ids=_epi_ids)
def test_strided_residual_poison_at_an_unread_position_changes_nothing(case, dtype, value):
    """res_stride = 2 reads the even positions of a [n, 2h, 2w, cout] residual: poison at odd positions is never loaded."""
    x, w = nf.make_conv(case, dtype)
    g = _gen(12)
    res = torch.randn(case.n, 2 * case.h, 2 * case.w, case.cout, generator=g)
    if dtype is not None:
        res = nf.round_to(res, dtype)
    bad = res.clone()
    bad[:, 1::2] = value            # every odd row, every odd column
    bad[:, :, 1::2] = value
    kw = dict(out_f32=True, res_stride=2)
    clean = _epi_run(case, dtype, x, w, residual=_residual(case, dtype, res), **kw)
    got = _epi_run(case, dtype, x, w, residual=_residual(case, dtype, bad), **kw)
    ref = nf.clean_reference(case, dtype) + res.double()[:, ::2, ::2]
    main = clean["y"]
    assert ((main.double() - ref).abs() <= 2.0 ** -7 * ref.abs() + 1e-3).all(), "the clean launch does not add the strided residual"
    for name, t in got.items():
        _bits_equal(t, clean[name], f"{case.name} [{name}]")


@pytest.mark.parametrize("value_name", ["nan", "inf"])
@pytest.mark.parametrize("case,dtype", EPI_PARAMS, ids=_epi_ids)
def test_stats_keep_a_non_finite_value(case, dtype, value_name):
    """want_stats on a poisoned input: the poisoned pixel reaches every output channel (all weights non-zero), so every
    channel's summed statistics are non-finite, and so are the scale and shift ``bn_finalize`` makes of them."""
    ops = _ops()
    _, w = nf.make_conv(case, dtype)
    label, where = nf.poisons(case)[2]
    p = nf.poison_reference(case, where, value_name, dtype)
    assert p.ref_mask.any(0).any(0).any(0).all()
    out = _epi_run(case, dtype, p.x, w, out_f32=(case.path != "fp32"), want_stats=True)
    stats = out["stats"]
    total = stats.double().cpu().sum(0)
    assert tuple(total.shape) == (2, case.cout)
    assert (~torch.isfinite(total)).all(), f"{case.name}: a non-finite value was dropped from the batch statistics"
    gamma, beta = torch.ones(case.cout).cuda(), torch.zeros(case.cout).cuda()
    scale, shift = ops.bn_finalize(stats, float(case.n * case.h * case.w), gamma, beta)
    assert (~torch.isfinite(scale)).all() and (~torch.isfinite(shift)).all()


# ================================================================================================ C. activation table
ACT_NAMES = ["none", "prelu", "leaky", "relu", "gelu"]
SLOPE = 0.25


def _act_expected(bias, act, alpha, slope):
    """The torch-CPU activation of the bias (float64, rounded once to float32).  GELU: the kernels' formula."""
    v = bias.double()
    if act == "prelu":
        v = nf.prelu(v, alpha.double())
        assert nf.nan_equal(v[None], F.prelu(bias.double()[None], alpha.double()))      # [1, C]: channels on axis 1
    elif act == "leaky":
        v = nf.leaky(v, slope)
        assert nf.nan_equal(v, F.leaky_relu(bias.double(), slope))
    elif act == "relu":
        v = nf.relu(v)
        assert nf.nan_equal(v, torch.relu(bias.double()), ignore_zero_sign=True)
    elif act == "gelu":
        v = nf.gelu(v)
    return v.float()


def _check_act_rows(got, expected, act, what):
    """Every pixel row of ``got`` [.., C] is ``expected`` [C]."""
    rows = got.reshape(-1, got.shape[-1]).cpu().float()
    want = expected[None].expand_as(rows)
    if act != "gelu":
        _same(rows, want, what)
        return
    # GELU: NaN gives NaN, +-Inf something non-finite (accepted divergence), finite values within erff's accuracy
    src = nf.tiled_specials(expected.numel())
    assert torch.isnan(rows[:, torch.isnan(src)]).all(), what
    assert (~torch.isfinite(rows[:, torch.isinf(src)])).all(), what
    fin = torch.isfinite(src)
    assert ((rows[:, fin].double() - want[:, fin].double()).abs() <= 1e-6 * want[:, fin].double().abs() + 1e-37).all(), what


def _act_ids(act):
    ops = _ops()
    return {"none": ops.ACT_NONE, "prelu": ops.ACT_PRELU, "leaky": ops.ACT_LEAKY, "relu": ops.ACT_RELU, "gelu": ops.ACT_GELU}[act]


@pytest.mark.parametrize("force", ["fast", "aux", "mask"])
@pytest.mark.parametrize("act", ACT_NAMES)
def test_activation_table_through_the_fp32_epilogue(act, force):
    """x = 0, so the pre-activation is the bias: the special values.  ``fast``: epi_store4_direct (none / PReLU / ReLU) or the
    general epilogue (leaky / GELU); ``aux`` / a mask of ones force the general epilogue."""
    ops = _ops()
    n, h, w_, cin, cout = 3, 5, 5, 32, 64
    g = _gen(21)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    bias, alpha = nf.tiled_specials(cout), torch.rand(cout, generator=g) * 0.3 + 0.1
    kw = dict(bias=bias.cuda(), act1=_act_ids(act), slope=SLOPE)
    if act == "prelu":
        kw["alpha"] = alpha.cuda()
    aux = None
    if force == "aux":
        aux = kw["aux"] = torch.empty(n, h, w_, cout).cuda()
    if force == "mask":
        kw["mask"] = torch.ones(n, h, w_, cout).cuda()
    expected = _act_expected(bias, act, alpha, SLOPE)
    for tile in (0, 5):
        y = ops.conv2d(torch.zeros(n, h, w_, cin).cuda(), ops.pack_conv_weight(wt.cuda()), 3, 3, pad=(1, 1), tile=tile, **kw)
        _check_act_rows(y, expected, act, f"fp32 tile {tile} {act} {force}")
        if aux is not None:
            _check_act_rows(aux, expected, act, f"fp32 tile {tile} {act} aux")


# geometry every family takes: 16x16 images (patch), W <= 86 (window), Cin = 64
ACT_TILES = {"b3": (42, 56, 59), "n16": (65, 76, 71)}


@pytest.mark.parametrize("outputs", ["narrow_only", "both", "general"])
@pytest.mark.parametrize("act", ACT_NAMES)
@pytest.mark.parametrize("tile", ACT_TILES["b3"])
def test_activation_table_through_the_b3_epilogues(tile, act, outputs):
    """``narrow_only`` / ``both``: the row epilogue epi_store4 (none / PReLU / ReLU; leaky and GELU fall to the general one);
    ``general``: a second output (next_affine with scale 1, shift 0) forces epilogue_store4 for every activation."""
    ops = _ops()
    n, hw, cin, cout = 3, 16, 64, 64
    g = _gen(22)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    bias, alpha = nf.tiled_specials(cout), torch.rand(cout, generator=g) * 0.3 + 0.1
    kw = dict(bias=bias.cuda(), act1=_act_ids(act), slope=SLOPE, out_f32=(outputs != "narrow_only"), out_split=True)
    if act == "prelu":
        kw["alpha"] = alpha.cuda()
    if outputs == "general":
        kw["next_affine"] = (torch.ones(cout).cuda(), torch.zeros(cout).cuda())
    xs = ops.split_bf16(torch.zeros(n, hw, hw, cin).cuda())
    r = ops.conv2d_b3(xs, ops.split_bf16(ops.pack_conv_weight(wt.cuda())), 3, 3, pad=(1, 1), tile=tile, **kw)
    expected = _act_expected(bias, act, alpha, SLOPE)
    tag = f"b3 tile {tile} {act} {outputs}"
    if "y" in r:
        _check_act_rows(r["y"], expected, act, tag + " y")
    if act != "gelu":                                   # the split planes of the table, value by value
        hi, lo = nf.split_bf16(expected)
        for key in ("split",) + (("next",) if outputs == "general" else ()):
            rows_hi, rows_lo = r[key].hi.float().cpu().reshape(-1, cout), r[key].lo.float().cpu().reshape(-1, cout)
            _same(rows_hi, hi[None].expand_as(rows_hi), tag + f" {key}.hi")
            _same(rows_lo, lo[None].expand_as(rows_lo), tag + f" {key}.lo")
    else:
        src = nf.tiled_specials(cout)
        hi = r["split"].hi.float().cpu().reshape(-1, cout)
        assert torch.isnan(hi[:, torch.isnan(src)]).all() and (~torch.isfinite(hi[:, torch.isinf(src)])).all(), tag


@pytest.mark.parametrize("dtype", NARROW, ids=["bf16", "fp16"])
@pytest.mark.parametrize("outputs", ["narrow_only", "both", "general"])
@pytest.mark.parametrize("act", ACT_NAMES)
@pytest.mark.parametrize("tile", ACT_TILES["n16"])
def test_activation_table_through_the_narrow_epilogues(tile, act, outputs, dtype):
    """As the bf16x3 test; ``general`` is forced by act2 = leaky with slope 1 (the identity, NaN and Inf included), so the
    leaky case of that leg runs with slope 1 too."""
    ops = _ops()
    n, hw, cin, cout = 3, 16, 64, 64
    g = _gen(23)
    wt = nf.round_to(torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5, dtype)
    bias, alpha = nf.tiled_specials(cout), torch.rand(cout, generator=g) * 0.3 + 0.1
    slope = 1.0 if outputs == "general" else SLOPE
    kw = dict(bias=bias.cuda(), act1=_act_ids(act), slope=slope, out_f32=(outputs != "narrow_only"), out_n16=True)
    if act == "prelu":
        kw["alpha"] = alpha.cuda()
    if outputs == "general":
        kw["act2"] = ops.ACT_LEAKY
    xd = torch.zeros(n, hw, hw, cin, dtype=dtype).cuda()
    r = ops.conv2d_n16(xd, ops.to_n16(ops.pack_conv_weight(wt.cuda()), dtype), 3, 3, pad=(1, 1), tile=tile, **kw)
    expected = _act_expected(bias, act, alpha, slope)
    tag = f"n16 {dtype} tile {tile} {act} {outputs}"
    if "y" in r:
        _check_act_rows(r["y"], expected, act, tag + " y")
        _same(r["n16"].float(), r["y"].to(dtype).float(), tag + " n16 is y rounded once")
    elif act != "gelu":
        _check_act_rows(r["n16"].float(), nf.round_to(expected, dtype), act, tag + " n16")
    else:
        src = nf.tiled_specials(cout)
        rows = r["n16"].float().cpu().reshape(-1, cout)
        assert torch.isnan(rows[:, torch.isnan(src)]).all() and (~torch.isfinite(rows[:, torch.isinf(src)])).all(), tag


# ================================================================================================ D. elementwise and rows
def _pairs(rows, cols):
    """(a, g) [rows, cols]: every special value of a under every special value of g, tiled."""
    s = nf.special_values()
    a, g = torch.meshgrid(s, s, indexing="ij")
    k = rows * cols
    rep = (k + 99) // 100
    return a.reshape(-1).repeat(rep)[:k].reshape(rows, cols).clone(), g.reshape(-1).repeat(rep)[:k].reshape(rows, cols).clone()


def test_maxpool_propagates_nan_like_torch():
    """NaN and +-Inf (and the other specials) in each of the four window positions, several blocks of threads."""
    ops = _ops()
    s = nf.special_values()
    x = torch.randn(3, 12, 10, 64, generator=_gen(31))
    k = 0
    for pos in range(4):
        for j in range(s.numel()):
            for rep in range(3):
                x[k % 3, (k // 3) % 6 * 2 + pos // 2, (k // 18) % 5 * 2 + pos % 2, (7 * k) % 64] = s[j]
                k += 1
    want = F.max_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    assert torch.isnan(want).sum() >= 4 and nf.nan_equal(nf.maxpool2x2(x), want)
    _same(ops.maxpool2x2_nhwc(x.cuda()), want, "maxpool2x2_nhwc")
    # a window of four NaN, and NaN against +inf in every order
    y = torch.zeros(1, 2, 8, 4)
    y[0, :, 0:2] = NAN
    for i, pos in enumerate(((0, 2), (0, 3), (1, 2), (1, 3))):
        y[0, :, 2:4, i] = INF
        y[0, pos[0], pos[1], i] = NAN
    got = ops.maxpool2x2_nhwc(y.cuda()).cpu()
    assert torch.isnan(got[0, 0, 0]).all() and torch.isnan(got[0, 0, 1]).all() and (got[0, 0, 2:] == 0).all()


def test_prelu_passes_follow_the_table():
    ops = _ops()
    rows, c = 130, 64
    x, g = _pairs(rows, c)
    alpha = torch.rand(c, generator=_gen(32)) * 0.3 + 0.1
    want = nf.prelu(x.double(), alpha.double()).float()
    assert nf.nan_equal(want, F.prelu(x.double(), alpha.double()).float())
    _same(ops.prelu_fwd(x.cuda(), alpha.cuda()), want, "prelu_fwd")
    sp = ops.prelu_split(x.cuda(), alpha.cuda())
    hi, lo = nf.split_bf16(want)
    _same(sp.hi.float(), hi, "prelu_split hi")
    _same(sp.lo.float(), lo, "prelu_split lo")
    dx64, terms64 = nf.prelu_bwd(x.double(), g.double(), alpha.double())
    dx, dalpha = ops.prelu_bwd(g.cuda(), x.cuda(), alpha.cuda())
    _same(dx, dx64.float(), "prelu_bwd dx")
    col_bad = ~torch.isfinite(terms64).all(0)
    assert col_bad.all() and (~torch.isfinite(dalpha.cpu())).all(), "prelu_bwd dalpha dropped a non-finite term"
    dxs, dalpha2 = ops.prelu_bwd(g.cuda(), x.cuda(), alpha.cuda(), split_out=True)
    hi, lo = nf.split_bf16(dx64.float())
    _same(dxs.hi.float(), hi, "prelu_bwd split dx hi")
    _same(dxs.lo.float(), lo, "prelu_bwd split dx lo")
    assert (~torch.isfinite(dalpha2.cpu())).all()


BN_APPLY_ROW = 200                                      # of P = 300 rows: the second of three 128-row statistics tiles


def _bn_apply_setup(dtype=None):
    g = _gen(33)
    n, h, c = 3, 10, 64
    y = torch.randn(n, h, h, c, generator=g)
    res = torch.randn(n, h, h, c, generator=g)
    if dtype is not None:
        res = nf.round_to(res, dtype)
    scale, shift = torch.rand(c, generator=g) * 0.45 + 0.5, torch.randn(c, generator=g)       # < 1: FLT_MAX * scale stays finite
    alpha = torch.rand(c, generator=g) * 0.3 + 0.1
    rs, rt = torch.rand(c, generator=g) * 0.45 + 0.5, torch.randn(c, generator=g)
    mask = nf.round_bf16((torch.rand(n, h, h, c, generator=g) > 0.3).float() * 2.0)
    bad = y.clone()
    bad.view(-1, c)[BN_APPLY_ROW] = nf.tiled_specials(c)
    return y, bad, res, scale, shift, alpha, rs, rt, mask


def _check_bn_apply(run, ref_and_bound, what):
    """``run(poison)`` -> {name: tensor [P, C] float32 on the CPU, 'stats': [tiles, 2, C]}.  The fp32 output 'y' is held to the
    reference (NaN and Inf exactly, finite values to the float32 bound); every 16-bit output must be that 'y' rounded once."""
    ref_bad, bound = ref_and_bound
    clean, got = run(False), run(True)
    row_bound = bound.view(300, -1)[BN_APPLY_ROW]
    y_row = got["y"].view(300, -1)[BN_APPLY_ROW]
    others = torch.ones(300, dtype=torch.bool)
    others[BN_APPLY_ROW] = False
    row_ref = ref_bad.view(300, -1)[BN_APPLY_ROW]
    assert (~torch.isfinite(row_ref)).any() and torch.isfinite(row_ref).any()
    for name, t in got.items():
        if name == "stats":
            assert t.shape[0] == 3
            _bits_equal(t[0], clean[name][0], what + " stats tile 0")
            _bits_equal(t[2], clean[name][2], what + " stats tile 2")
            bad_cols = ~torch.isfinite(row_ref)
            assert (~torch.isfinite(t[1]))[:, bad_cols].all(), what + ": the poisoned tile's statistics lost a non-finite value"
            assert torch.isfinite(t[1][0][~bad_cols]).all(), what + ": a finite column's sum became non-finite"
            continue
        t, c = t.view(300, -1), clean[name].view(300, -1)
        assert torch.isfinite(c).all()
        _bits_equal(t[others], c[others], what + f" [{name}] rows beside the poisoned one")
        row = t[BN_APPLY_ROW]
        if name != "y":                                   # a 16-bit plane: the fp32 result rounded once, exactly
            want = {"split.hi": nf.split_bf16(y_row)[0], "split.lo": nf.split_bf16(y_row)[1], "bf16": nf.round_bf16(y_row),
                    "f16": nf.round_f16(y_row)}[name]
            _same(row, want, what + f" [{name}] is y rounded once")
            continue
        assert torch.equal(torch.isnan(row), torch.isnan(row_ref)), what + " [y] NaN positions"
        inf = torch.isinf(row_ref)
        assert torch.equal(row[inf], row_ref[inf]) and torch.equal(torch.isinf(row), inf), what + " [y] infinities"
        fin = torch.isfinite(row_ref)
        err = (row[fin].double() - row_ref[fin].double()).abs()
        assert (err <= row_bound[fin]).all(), what + f" [y] finite values: {(err / row_bound[fin]).max().item():.2f} of the bound"


def test_bn_apply_fp32_keeps_non_finite_values_in_their_row():
    ops = _ops()
    y, bad, res, scale, shift, alpha, rs, rt, mask = _bn_apply_setup()

    def run(poison):
        out, stats = ops.bn_apply_nhwc((bad if poison else y).cuda(), scale.cuda(), shift.cuda(), alpha=alpha.cuda(), res=res.cuda(),
                                       res_scale=rs.cuda(), res_shift=rt.cuda(), mask=mask.cuda(), want_stats=True)
        return {"y": out.cpu(), "stats": stats.cpu()}
    _check_bn_apply(run, _bn_apply_ref(bad, res, scale, shift, alpha, rs, rt, mask), "bn_apply_nhwc")


def test_bn_apply_b3_keeps_non_finite_values_in_their_row():
    ops = _ops()
    y, bad, res, scale, shift, alpha, rs, rt, mask = _bn_apply_setup()
    rsp = ops.split_bf16(res.cuda())
    res_eff = rsp.float().cpu()

    def run(poison):
        o = ops.bn_apply_nhwc_b3((bad if poison else y).cuda(), scale.cuda(), shift.cuda(), alpha=alpha.cuda(), res=rsp, res_scale=rs.cuda(),
                                 res_shift=rt.cuda(), mask=mask.cuda(), want_stats=True, out_f32=True, out_split=True)
        return {"y": o["y"].cpu(), "split.hi": o["split"].hi.float().cpu(), "split.lo": o["split"].lo.float().cpu(), "stats": o["stats"].cpu()}
    _check_bn_apply(run, _bn_apply_ref(bad, res_eff, scale, shift, alpha, rs, rt, mask), "bn_apply_nhwc_b3")


@pytest.mark.parametrize("dtype", NARROW, ids=["bf16", "fp16"])
def test_bn_apply_n16_keeps_non_finite_values_in_their_row(dtype):
    ops = _ops()
    y, bad, res, scale, shift, alpha, rs, rt, mask = _bn_apply_setup(dtype)
    key = "bf16" if dtype == torch.bfloat16 else "f16"

    def run(poison):
        o = ops.bn_apply_nhwc_n16((bad if poison else y).cuda(), scale.cuda(), shift.cuda(), dtype=dtype, alpha=alpha.cuda(),
                                  res=res.to(dtype).cuda(), res_scale=rs.cuda(), res_shift=rt.cuda(), mask=mask.cuda(), want_stats=True,
                                  out_f32=True, out_n16=True)
        return {"y": o["y"].cpu(), key: o["n16"].float().cpu(), "stats": o["stats"].cpu()}
    _check_bn_apply(run, _bn_apply_ref(bad, res, scale, shift, alpha, rs, rt, mask), f"bn_apply_nhwc_n16 {dtype}")


@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
def test_storage_conversions_on_specials_and_ties(affine):
    """split_bf16 / to_n16 / from_n16 against ``Tensor.bfloat16()`` / ``.half()`` on the special values and on exact ties.  The
    affine uses powers of two and a zero shift, so x * s + t is one exact (or once-rounded) product however it is contracted."""
    ops = _ops()
    c = 64
    for dtype in NARROW:
        v = torch.cat([nf.special_values(), nf.ties(dtype), torch.tensor([65504.0, 65520.0, 3.0e-8, -2.9e-8, 6.0e-8, 1e-40])])
        v = v.repeat((4 * c + v.numel() - 1) // v.numel() + 1)[: 4 * c].reshape(4, c).contiguous()
        s = t = None
        src = v
        if affine:
            s = torch.tensor([0.5, 2.0, 1.0, -4.0]).repeat(c // 4)
            t = torch.zeros(c)
            src = v * s
        kw = dict(scale=s.cuda(), shift=t.cuda()) if affine else {}
        got = ops.to_n16(v.cuda(), dtype, **kw)
        _same(got.float(), src.to(dtype).float(), f"to_n16 {dtype}", ignore_zero_sign=affine)
        _same(got.float(), nf.round_to(src, dtype), f"to_n16 {dtype} vs the table", ignore_zero_sign=affine)
        _same(ops.from_n16(got), got.cpu().float(), f"from_n16 {dtype}", ignore_zero_sign=False)
        if dtype == torch.bfloat16:
            sp = ops.split_bf16(v.cuda(), **kw)
            hi = src.bfloat16().float()
            _same(sp.hi.float(), hi, "split_bf16 hi", ignore_zero_sign=affine)
            _same(sp.lo.float(), (src - hi).bfloat16().float(), "split_bf16 lo")


@pytest.mark.parametrize("cols", [512, 100])
def test_l2norm_rows_keep_a_poisoned_row_to_itself(cols):
    """rows = 5 (two blocks of four rows).  Row 1 is poisoned, row 3 is all zero: 0 / 0 = NaN as the reference (no epsilon)."""
    ops = _ops()
    g = _gen(34 + cols)
    x, dy = torch.randn(5, cols, generator=g), torch.randn(5, cols, generator=g)
    x[3] = 0.0
    clean_y, clean_dx = ops.l2norm_rows(x.cuda()).cpu(), ops.l2norm_rows_bwd(dy.cuda(), x.cuda()).cpu()
    assert torch.isnan(clean_y[3]).all() and torch.isnan(clean_dx[3]).all()
    ok = [0, 2, 4]
    assert torch.isfinite(clean_y[ok]).all() and torch.isfinite(clean_dx[ok]).all()
    for value in (NAN, INF):
        bad = x.clone()
        bad[1, cols // 3] = value
        y, dx = ops.l2norm_rows(bad.cuda()).cpu(), ops.l2norm_rows_bwd(dy.cuda(), bad.cuda()).cpu()
        _bits_equal(y[ok], clean_y[ok], "l2norm_rows: the other rows")
        _bits_equal(dx[ok], clean_dx[ok], "l2norm_rows_bwd: the other rows")
        assert torch.isnan(y[3]).all() and torch.isnan(dx[3]).all()
        b64 = bad.double().requires_grad_(True)
        ref = b64 / b64.pow(2).sum(1, keepdim=True).sqrt()
        ref.backward(dy.double())
        _same(y[1], ref[1].detach().float(), f"l2norm_rows poisoned row ({value})")
        assert torch.equal(~torch.isfinite(dx[1]), ~torch.isfinite(b64.grad[1])), f"l2norm_rows_bwd poisoned row ({value})"


def test_gather_rows_never_reads_unselected_rows():
    ops = _ops()
    src = torch.randn(9, 64, generator=_gen(35))
    src[[1, 4, 8]] = NAN
    src[6, ::3] = INF
    index = torch.tensor([0, -1, 2, 3, -1, 5, 7, 7, 0, -1, 6], dtype=torch.int64)
    got = ops.gather_rows(src.cuda(), index.cuda()).cpu()
    want = torch.where((index >= 0)[:, None], src[index.clamp_min(0)], torch.zeros(1))
    _same(got, want, "gather_rows", ignore_zero_sign=False)
    assert not torch.isnan(got).any() and (got[index < 0] == 0).all() and not torch.signbit(got[index < 0]).any()


def _fc_act(kind, a):
    """(the tensor handed to fc_bwd, the activation values the kernel sees)"""
    ops = _ops()
    if kind == "none":
        return None, torch.ones_like(a)
    if kind == "f32":
        return a.cuda(), a
    if kind == "split":
        sp = ops.split_bf16(a.cuda())
        return sp, sp.hi.float().cpu() + sp.lo.float().cpu()
    dt = torch.bfloat16 if kind == "bf16" else torch.float16
    return a.to(dt).cuda(), a.to(dt).float()


@pytest.mark.parametrize("kind", ["none", "f32", "split", "bf16", "f16"])
def test_fc_bwd_mask_is_relu_backward_from_the_saved_output(kind):
    """dz = a <= 0 ? 0 : da on every pair (saved activation, incoming gradient) of special values: a zero activation gives 0
    under an inf / nan gradient, a NaN activation lets the gradient through (torch's threshold_backward)."""
    ops = _ops()
    rows, c = 70, 64
    a, g = _pairs(rows, c)
    act, a_eff = _fc_act(kind, a)
    r = ops.fc_bwd(g.cuda(), act, out_split=True, out_f32=True)
    want = nf.relu_bwd(a_eff, g) if kind != "none" else g
    if kind != "none":
        z = a_eff.double().clone().requires_grad_(True)
        torch.relu(z).backward(g.double())
        assert nf.nan_equal(want, z.grad.float(), ignore_zero_sign=True)          # the table is autograd's answer
        zero = a_eff == 0
        assert zero.any() and (r["f32"].cpu()[zero] == 0).all(), "a == 0 must give 0 whatever the gradient"
        nan = torch.isnan(a_eff)
        assert nan.any() and nf.nan_equal(r["f32"].cpu()[nan], g[nan]), "a == nan must let the gradient through"
    _same(r["f32"], want, f"fc_bwd[{kind}] f32")
    hi, lo = nf.split_bf16(want)
    _same(r["split"].hi.float(), hi, f"fc_bwd[{kind}] split hi")
    _same(r["split"].lo.float(), lo, f"fc_bwd[{kind}] split lo")
    assert (~torch.isfinite(r["db"].cpu())).all()


@pytest.mark.parametrize("kind", ["none", "f32", "split", "bf16", "f16"])
def test_fc_bwd_bias_gradient_keeps_poison_in_its_column(kind):
    ops = _ops()
    rows, c = 300, 64                                        # more than one slab of rows per column block
    gen = _gen(36)
    da = torch.randn(rows, c, generator=gen)
    a = torch.relu(torch.randn(rows, c, generator=gen))
    a[17, 9] = 0.0
    a[250, 5] = 1.0
    act, _ = _fc_act(kind, a)
    clean = ops.fc_bwd(da.cuda(), act, out_split=False, out_f32=True)
    assert torch.isfinite(clean["db"]).all()
    for value in (NAN, INF):
        bad = da.clone()
        bad[250, 5] = value                                  # passes: db[5] is non-finite
        bad[17, 9] = value                                   # stopped by a == 0 (not when there is no mask)
        got = ops.fc_bwd(bad.cuda(), act, out_split=False, out_f32=True)
        db, hit = got["db"].cpu(), torch.zeros(c, dtype=torch.bool)
        hit[5] = True
        hit[9] = kind == "none"
        assert torch.equal(~torch.isfinite(db), hit), f"fc_bwd[{kind}] db"
        _bits_equal(db[~hit], clean["db"].cpu()[~hit], f"fc_bwd[{kind}] db beside the poisoned column")
        cell = torch.zeros(rows, c, dtype=torch.bool)
        cell[250, 5] = True
        cell[17, 9] = kind == "none"
        _bits_equal(got["f32"].cpu()[~cell], clean["f32"].cpu()[~cell], f"fc_bwd[{kind}] dz")


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("slope", [0.0, 0.01], ids=["relu", "leaky"])
def test_tcn_glue_follows_the_table(slope, masked):
    """leaky_relu, act_mask_bwd and tblock_tail_bwd on every pair of special values.  slope = 0 is ReLU: its backward is the
    select ``a <= 0 ? 0 : g`` (torch's threshold_backward), not a product with 0."""
    ops = _ops()
    rows, c = 40, 64
    a, g = _pairs(rows, c)
    s32 = float(torch.tensor(slope, dtype=torch.float32))
    _same(ops.leaky_relu(a.cuda(), slope), nf.leaky(a.double(), s32).float(), f"leaky_relu slope {slope}")
    mask = nf.round_bf16((torch.rand(rows, c, generator=_gen(37)) > 0.3).float() * 2.0) if masked else None
    md = mask.cuda() if masked else None
    gm = ((g * mask) if masked else g).double()                     # the kernels' fp32 product with the mask, then ONE more product
    want = nf.leaky_bwd(a.double(), gm, s32).float()
    _same(ops.act_mask_bwd(g.cuda(), a.cuda(), md, slope), want, f"act_mask_bwd slope {slope}")
    # the tail: out and a2 both run over the specials, shifted against each other
    out = a.roll(7, 1).contiguous()
    du32 = nf.leaky_bwd(out.double(), g.double(), s32).float()
    dz32 = nf.leaky_bwd(a.double(), ((du32 * mask) if masked else du32).double(), s32).float()
    du, dz2 = ops.tblock_tail_bwd(g.cuda(), out.cuda(), a.cuda(), md, slope)
    _same(du, du32, f"tblock_tail_bwd du slope {slope}")
    _same(dz2, dz32, f"tblock_tail_bwd dz2 slope {slope}")
    if slope == 0.0:
        zero, nan = a == 0, torch.isnan(a)
        got = ops.act_mask_bwd(g.cuda(), a.cuda(), None, 0.0).cpu()
        assert (got[zero] == 0).all() and nf.nan_equal(got[nan], g[nan])


@pytest.mark.parametrize("value", [NAN, INF], ids=["nan", "inf"])
def test_row_passes_keep_a_poisoned_row_to_itself(value):
    """layernorm_fwd, softmax_gate_fwd and eval-mode bn_rows_fwd: rows beside the poisoned one are bit-identical; the poisoned
    row is non-finite where the float64 reference is."""
    ops = _ops()
    g = _gen(38)
    r, c, row, col = 9, 64, 4, 21
    x = torch.randn(r, c, generator=g)
    bad = nf.poisoned(x, (row, col), value)
    others = [i for i in range(r) if i != row]
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    rm, rv = torch.randn(c, generator=g) * 0.1, torch.rand(c, generator=g) + 0.5
    cc = torch.randn(r, c, generator=g)

    def ln(t):
        y, mean, rstd = ops.layernorm_fwd(t.cuda(), gamma.cuda(), beta.cuda())
        return y.cpu(), mean.cpu(), rstd.cpu()

    def gate(t):
        out, prob = ops.softmax_gate_fwd(t.cuda(), cc.cuda())
        return out.cpu(), prob.cpu()

    def bn(t):
        return (ops.bn_rows_fwd(t.cuda(), gamma.cuda(), beta.cuda(), rm.cuda(), rv.cuda(), False)[0].cpu(),)

    refs = {"layernorm": (F.layer_norm(bad.double(), (c,), gamma.double(), beta.double()),),
            "softmax_gate": (torch.softmax(bad.double(), 1) * cc.double(), torch.softmax(bad.double(), 1)),
            "bn_rows eval": (F.batch_norm(bad.double(), rm.double(), rv.double(), gamma.double(), beta.double(), training=False),)}
    for name, fn in (("layernorm", ln), ("softmax_gate", gate), ("bn_rows eval", bn)):
        clean, got = fn(x), fn(bad)
        for i, (cl, gt) in enumerate(zip(clean, got)):
            assert torch.isfinite(cl).all()
            _bits_equal(gt[others], cl[others], f"{name} output {i}: rows beside the poisoned one")
            assert not torch.isfinite(gt[row]).all(), f"{name} output {i}: the poison vanished"
        for i, ref in enumerate(refs[name]):
            assert torch.equal(~torch.isfinite(got[i][row]), ~torch.isfinite(ref[row])), f"{name} output {i}: non-finite positions"
            if value != value:
                assert torch.equal(torch.isnan(got[i][row]), torch.isnan(ref[row]))


BN_ROWS_ROUTES = [(300, False), (2500, False), (2500, True)]      # one block; > 2048 rows: one pass over dense rows, two passes over a slice


@pytest.mark.parametrize("value", [NAN, INF], ids=["nan", "inf"])
@pytest.mark.parametrize("r,sliced", BN_ROWS_ROUTES, ids=["one_block", "slabs_one_pass", "slabs_two_pass"])
def test_bn_rows_train_keeps_a_poisoned_column_to_itself(r, sliced, value):
    """Train-mode row BatchNorm: the statistics are per column.  A poisoned element makes its whole column (output, saved mean and
    inverse deviation, both running buffers) non-finite, as torch does, and leaves every other column bit-identical.  The three
    routes of ``cer_bn_rows_fwd``: R <= 2048 (one block per 32 channels), R > 2048 on dense rows (slab sums about a shift row,
    one pass) and on a column slice (x_ld != C: two passes of slab sums)."""
    ops = _ops()
    g = _gen(39 + r)
    c, row, col = 64, r * 2 // 5 + 3, 21
    x = torch.randn(r, c, generator=g)
    bad = nf.poisoned(x, (row, col), value)
    w, b = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)

    def run(t):
        rm, rv = torch.zeros(c).cuda(), torch.ones(c).cuda()
        td = t.cuda()
        if sliced:
            wide = torch.full((r, c + 8), NAN).cuda()
            wide[:, 4:4 + c] = td
            td = wide[:, 4:4 + c]
        y, sm, si = ops.bn_rows_fwd(td, w.cuda(), b.cuda(), rm, rv, True)
        return {"y": y.cpu(), "save_mean": sm.cpu()[None], "save_invstd": si.cpu()[None], "running_mean": rm.cpu()[None],
                "running_var": rv.cpu()[None]}
    clean, got = run(x), run(bad)
    keep = torch.ones(c, dtype=torch.bool)
    keep[col] = False
    ref = F.batch_norm(bad.double(), None, None, w.double(), b.double(), training=True)
    assert (~torch.isfinite(ref[:, col])).all() and torch.isfinite(ref[:, keep]).all()
    for name in got:
        assert torch.isfinite(clean[name]).all(), name
        _bits_equal(got[name][:, keep], clean[name][:, keep], f"bn_rows_fwd train {name}: the other columns")
        assert (~torch.isfinite(got[name][:, col])).all(), f"bn_rows_fwd train {name}: the poisoned column must be non-finite"
    assert ((clean["y"].double() - F.batch_norm(x.double(), None, None, w.double(), b.double(), training=True)).abs() < 1e-4).all()


@pytest.mark.parametrize("value", [NAN, INF], ids=["nan", "inf"])
@pytest.mark.parametrize("r,large", [(300, False), (2500, True)], ids=["one_block", "slabs"])
def test_bn_rows_moments_and_merge_keep_a_poisoned_column_to_itself(r, large, value):
    """The synchronised statistics: (count, mean, M2) of ``bn_rows_moments`` / ``bn_rows_moments_large`` and what
    ``bn_rows_merge`` makes of two such blocks.  The poisoned column's mean and M2, its saved mean and inverse deviation and both
    running buffers are non-finite; every other column is bit-identical to the clean run."""
    ops = _ops()
    g = _gen(40 + r)
    c, row, col = 64, r * 3 // 5 + 1, 37
    x, other = torch.randn(r, c, generator=g), torch.randn(r, c, generator=g)
    bad = nf.poisoned(x, (row, col), value)
    moments = ops.bn_rows_moments_large if large else ops.bn_rows_moments

    def run(t):
        m = torch.stack([moments(t.cuda()), moments(other.cuda())])
        rm, rv = torch.zeros(c).cuda(), torch.ones(c).cuda()
        sm, si = ops.bn_rows_merge(m, rm, rv)
        return {"mean": m[0, 1:2].cpu(), "M2": m[0, 2:3].cpu(), "save_mean": sm.cpu()[None], "save_invstd": si.cpu()[None],
                "running_mean": rm.cpu()[None], "running_var": rv.cpu()[None]}
    clean, got = run(x), run(bad)
    keep = torch.ones(c, dtype=torch.bool)
    keep[col] = False
    for name in got:
        assert torch.isfinite(clean[name]).all(), name
        _bits_equal(got[name][:, keep], clean[name][:, keep], f"bn_rows moments / merge {name}: the other columns")
        assert (~torch.isfinite(got[name][:, col])).all(), f"bn_rows moments / merge {name}: the poisoned column must be non-finite"


# ================================================================================================ E. whole models, eval mode
def _assert_item_isolated(clean, got, what, all_nan=False):
    """Three items per batch, the middle one poisoned: items 0 and 2 bit-identical, item 1 non-finite."""
    clean, got = clean.cpu(), got.cpu()
    assert torch.isfinite(clean).all(), what
    _bits_equal(got[0], clean[0], what + ": item 0")
    _bits_equal(got[2], clean[2], what + ": item 2")
    if all_nan:
        assert torch.isnan(got[1]).all(), what + ": the poisoned item's embedding is all NaN"
    else:
        assert (~torch.isfinite(got[1])).all(), what + ": the poisoned item's output is non-finite"


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "fp16", "bf16"])
def test_visual_backbone_eval_isolates_a_poisoned_frame(precision):
    """Eval-mode IR-50 batches frames of unrelated videos and streams: one bad frame must not change another frame's embedding.
    The poisoned frame's embedding is all NaN (the head's unit normalisation divides NaN / Inf by its own norm)."""
    from feature_vs_text_compound_emotion_amd import synth
    from test_backbone_gpu import _build
    hw = 40
    vsd = synth.make_state_dict(synth.visual_backbone_spec("", hw // 8), seed=11)
    vb = _build(vsd, hw // 8, precision)
    frames = torch.randn(3, 3, hw, hw, generator=_gen(41))
    with torch.no_grad():
        clean = vb(frames.cuda())
        for value in (NAN, INF):
            bad = nf.poisoned(frames, (1, 1, 17, 23), value)
            _assert_item_isolated(clean, vb(bad.cuda()), f"VisualBackbone {precision} {value}", all_nan=True)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "fp16", "bf16"])
def test_vggish_eval_isolates_a_poisoned_example_and_keeps_it_non_finite(precision):
    """VGGish is ReLU convs, max-pools and ReLU FC layers: with a ReLU that swallows NaN the poisoned example's embedding comes
    out FINITE.  This is the case --amp depends on: an overflow in the forward pass has to reach the loss as NaN / Inf for the
    loss-scale check (found_inf) to skip the step.  (The max-pool is not what this test detects: after the first 3x3 conv the NaN
    fills whole 2x2 windows, and a max of four NaN is NaN either way; test_maxpool_propagates_nan_like_torch pins the pool.)"""
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.audio_backbone import AudioBackbone
    vsd = synth.make_state_dict(synth.vggish_spec(""), seed=41)
    ab = AudioBackbone()
    ab.backbone.load_state_dict(vsd, strict=True)
    ab.backbone.precision = precision
    ab = ab.cuda().eval()
    x = torch.randn(3, 96, 64, generator=_gen(42))
    with torch.no_grad():
        clean = ab(x)
        for value in (NAN, INF):
            bad = nf.poisoned(x, (1, 40, 30), value)
            _assert_item_isolated(clean, ab(bad), f"VGGish {precision} {value}")


def test_lfan_eval_isolates_a_poisoned_video():
    """Three videos of pre-computed features (the modalities of test_lfan_eval_logits_match_reference_fixture): the logits of
    videos 0 and 2 are bit-identical, video 1's are non-finite."""
    from feature_vs_text_compound_emotion_amd import synth
    from helpers import MODS
    from test_tail_gpu import _build_lfan
    b, l, hw = 3, 8, 40
    sd = synth.lfan_state_dict(MODS, n_cls=7, head_hw=hw // 8, seed=3)
    x, _ = synth.make_clip_batch(MODS, b, l, hw=hw, seed=77)
    model = _build_lfan(MODS, sd, l).eval()
    feature_mod = [m for m in MODS if m != "video"][0]
    assert "video" in x and feature_mod in x
    with torch.no_grad():
        clean = model({k: v.clone().cuda() for k, v in x.items()})
        # the first frame: the causal temporal convs carry it to every later frame of the video
        for mod, where in ((feature_mod, (1, 0, 0, 5)), ("video", (1, 0, 1, 17, 23))):
            for value in (NAN, INF):
                bad = {k: v.clone() for k, v in x.items()}
                bad[mod][where] = value
                got = model({k: v.cuda() for k, v in bad.items()})
                assert tuple(got.shape) == tuple(clean.shape) and got.shape[0] == b
                g3, c3 = got.reshape(b, -1).cpu(), clean.reshape(b, -1).cpu()
                _bits_equal(g3[0], c3[0], f"LFAN {mod} {value}: video 0")
                _bits_equal(g3[2], c3[2], f"LFAN {mod} {value}: video 2")
                assert (~torch.isfinite(g3[1])).all(), f"LFAN {mod} {value}: video 1 has finite logits"
