"""The preconditions of tests/test_nonfinite_gpu.py, checked without a GPU: the poison masks of nonfinite_ref.py agree with
float64 ``F.conv2d``, an Inf poison gives +-inf and never NaN, every weight survives rounding, and the elementwise tables
agree with torch's own operators."""
import pytest
import torch
import torch.nn.functional as F

import nonfinite_ref as nf

_GEOMETRIES = {}
for _c in nf.CONV_CASES:
    _GEOMETRIES.setdefault((tuple(_c[3:]), nf.CHUNK[_c.path], _c.tile % 2), _c)     # one case per geometry and poison set
GEOMETRIES = list(_GEOMETRIES.values())


def test_case_tables_cover_what_the_contract_names():
    names = [c.name for c in nf.CONV_CASES]
    assert len(set(names)) == len(names)
    tiles = {p: {c.tile for c in nf.CONV_CASES if c.path == p} for p in ("fp32", "b3", "n16")}
    assert tiles["fp32"] == set(nf.FP32_TILES)
    assert tiles["b3"] == {0, 41, 42, 44, 45, 48, 53, 56, 59, 58, 51, 52}
    assert tiles["n16"] == {0, 63, 64, 65, 66, 67, 91, 94, 73, 76, 77, 71, 72, 78, 79, 81, 82}
    for c in nf.CONV_CASES:
        assert c.n >= 3, c.name                                       # an image with a neighbour on both sides
        if c.path == "n16":
            assert c.cin % (128 if c.s2d else 64) == 0 and (c.tile not in (71, 77, 79) or c.cin == 64), c.name
        if c.path == "b3":
            assert c.cin % (64 if c.s2d else 32) == 0, c.name
        where = dict(nf.poisons(c))
        assert where["a"] == (0, c.h - 1, c.w - 1, c.cin - 1) and where["b"] == (1, 0, 0, 0) and where["c"][0] == c.n - 1
        if nf.CHUNK[c.path]:
            assert where["c"][3] in (nf.CHUNK[c.path] - 1, nf.CHUNK[c.path]), c.name
    # both sides of a chunk boundary are poisoned somewhere on each 16-bit path
    for p in ("b3", "n16"):
        assert {dict(nf.poisons(c))["c"][3] for c in nf.CONV_CASES if c.path == p} == {nf.CHUNK[p] - 1, nf.CHUNK[p]}


def test_special_values_are_what_they_claim():
    s = nf.special_values()
    assert s.dtype == torch.float32 and s.numel() == 10
    assert torch.isnan(s[0]) and s[1] == nf.INF and s[2] == -nf.INF
    assert s[3] == 0 and not torch.signbit(s[3]) and s[4] == 0 and torch.signbit(s[4])
    assert s[5] > 0 and s[5].view(torch.int32).item() == 1                      # the smallest denormal
    assert s[6] == torch.finfo(torch.float32).max and s[7] == -s[6] and s[8] == 1 and s[9] == -1
    assert nf.tiled_specials(64).numel() == 64 and nf.nan_equal(nf.tiled_specials(64)[:10], s)


def test_nan_equal_sees_nan_positions_values_and_the_sign_of_zero():
    s = nf.special_values()
    assert nf.nan_equal(s, s.clone())
    assert not nf.nan_equal(s, torch.nan_to_num(s, nan=0.0, posinf=nf.INF, neginf=-nf.INF))       # a NaN lost
    t = s.clone()
    t[1] = -nf.INF
    assert not nf.nan_equal(s, t)                                                  # the sign of an infinity
    t = s.clone()
    t[4] = 0.0
    assert not nf.nan_equal(s, t) and nf.nan_equal(s, t, ignore_zero_sign=True)    # the sign of a zero, on request only
    assert not nf.nan_equal(s, s[:8])
    assert "differ" in nf.describe_mismatch(s, t)


@pytest.mark.parametrize("case", GEOMETRIES, ids=lambda c: c.name)
def test_geometric_poison_mask_is_the_float64_conv_mask(case):
    """For every geometry and poison: the mask from the geometry equals the non-finite mask of float64 ``F.conv2d`` in EVERY
    output channel; a NaN poison gives NaN there, a +Inf poison +-inf by the sign of the tap's weight and never NaN; all other
    outputs equal the clean conv bit for bit (the float64 reference itself is isolated)."""
    dtypes = (None,) if case.path in ("fp32", "stem") else ((None,) if case.path == "b3" else (torch.bfloat16, torch.float16))
    for dtype in dtypes:
        x, w = nf.make_conv(case, dtype)
        assert nf.weights_survive_rounding(w) and (w != 0).all()
        clean = nf.clean_reference(case, dtype)
        assert torch.isfinite(clean).all()
        masks = []
        for label, where in nf.poisons(case):
            for vname, value in nf.POISON_VALUES:
                p = nf.poison_reference(case, where, vname, dtype)
                assert p.geo_mask.any(), (label, "the poison reaches no output")
                assert torch.equal(p.ref_mask, p.geo_mask[..., None].expand_as(p.ref_mask)), (label, vname)
                bad = p.ref[p.ref_mask]
                if vname == "nan":
                    assert torch.isnan(bad).all()
                else:
                    assert torch.isinf(bad).all(), (label, "an Inf poison must not turn into NaN in the reference")
                assert nf.nan_equal(p.ref[p.ref_mask], p.geo_value[p.ref_mask]), (label, vname)
                assert torch.equal(p.ref[~p.ref_mask], clean[~p.ref_mask])
            masks.append(p.geo_mask)
        # the three poisons can be told apart, and each leaves the other images alone
        assert not (masks[0] & masks[1]).any() and not (masks[1] & masks[2]).any() and not (masks[0] & masks[2]).any()
        assert not masks[0][1:].any() and not masks[1][0].any() and not masks[1][2:].any() and not masks[2][:-1].any()


def test_poison_check_catches_a_border_handled_by_a_zero_factor():
    """What the isolation rule is for: a conv that multiplies an out-of-image tap by 0 instead of selecting it away equals the
    correct one on finite data and leaks a neighbour's NaN / Inf into the wrong image.  ``check_poisoned`` passes the selecting
    conv on every poison and fails the multiplying one, with no tolerance involved."""
    case = nf.conv_case("fp32", 0, 3, 32, 36, 7, 7)
    x, w = nf.make_conv(case)
    clean = {b: {"y": nf.flat_conv(case, x, w, b)} for b in ("select", "zero_factor")}
    assert torch.equal(clean["select"]["y"], clean["zero_factor"]["y"])                 # indistinguishable on finite data
    assert (clean["select"]["y"] - nf.clean_reference(case)).abs().max().item() < 1e-12
    caught = 0
    for label, where in nf.poisons(case):
        for vname, _ in nf.POISON_VALUES:
            p = nf.poison_reference(case, where, vname)
            args = (p.ref_mask, p.ref, vname, ("y",), f"poison ({label}) {vname}")
            nf.check_poisoned({"y": nf.flat_conv(case, p.x, w, "select")}, clean["select"], *args)
            if label in ("a", "b"):                 # a pixel at an image's edge: the neighbouring image's border taps land on it
                with pytest.raises(AssertionError, match="outside the receptive field"):
                    nf.check_poisoned({"y": nf.flat_conv(case, p.x, w, "zero_factor")}, clean["zero_factor"], *args)
                caught += 1
    assert caught == 4


def test_activation_tables_agree_with_torch():
    s = nf.special_values()
    v = torch.cat([s, torch.tensor([2.5, -2.5, 1e-30, -1e-30])]).double()
    assert nf.nan_equal(nf.relu(v), torch.relu(v), ignore_zero_sign=True)
    assert torch.isnan(nf.relu(torch.tensor(nf.NAN))) and nf.relu(torch.tensor(-nf.INF)) == 0
    for slope in (0.01, 0.25):
        assert nf.nan_equal(nf.leaky(v, slope), F.leaky_relu(v, slope))
    alpha = torch.tensor([0.25], dtype=torch.float64)
    assert nf.nan_equal(nf.prelu(v, alpha), F.prelu(v, alpha))
    finite = v[torch.isfinite(v)]
    assert (nf.gelu(finite) - F.gelu(finite)).abs().max().item() < 1e-15
    # GELU at the non-finite values: NaN gives NaN, +-Inf something non-finite (torch-CPU: nan at both; the formula: +inf, nan)
    for x in (nf.NAN, nf.INF, -nf.INF):
        assert not torch.isfinite(nf.gelu(torch.tensor(x, dtype=torch.float64))) and not torch.isfinite(F.gelu(torch.tensor(x, dtype=torch.float64)))
    assert torch.isnan(nf.gelu(torch.tensor(nf.NAN, dtype=torch.float64)))


def test_backward_tables_agree_with_autograd():
    s = nf.special_values().double()
    a, g = torch.meshgrid(s, s, indexing="ij")                  # every saved value under every incoming gradient
    a, g = a.reshape(-1).clone(), g.reshape(-1).clone()
    # ReLU from the saved OUTPUT (what the kernels keep): relu(a) has the sign class of a for a >= 0 and NaN
    z = a.clone().requires_grad_(True)
    torch.relu(z).backward(g)
    assert nf.nan_equal(nf.relu_bwd(a, g), z.grad, ignore_zero_sign=True)
    saved = torch.relu(a)
    assert nf.nan_equal(nf.relu_bwd(saved, g), z.grad, ignore_zero_sign=True)
    zero, nan = a == 0, torch.isnan(a)
    assert (nf.relu_bwd(a, g)[zero] == 0).all()                 # a zero activation stops an inf / nan gradient
    assert nf.nan_equal(nf.relu_bwd(a, g)[nan], g[nan])         # a NaN activation lets it through
    assert nf.nan_equal(nf.leaky_bwd(a, g, 0.0), nf.relu_bwd(a, g))
    for slope in (0.01, 0.25):
        z = a.clone().requires_grad_(True)
        F.leaky_relu(z, slope).backward(g)
        assert nf.nan_equal(nf.leaky_bwd(a, g, slope), z.grad)
        assert nf.nan_equal(nf.leaky_bwd(F.leaky_relu(a, slope), g, slope), z.grad)      # from the saved output: the same
    alpha = torch.tensor([0.25], dtype=torch.float64, requires_grad=True)
    z = a.clone().requires_grad_(True)
    F.prelu(z, alpha).backward(g)
    dx, terms = nf.prelu_bwd(a, g, alpha.detach())
    assert nf.nan_equal(dx, z.grad)
    assert not torch.isfinite(terms.sum()) and not torch.isfinite(alpha.grad).all()
    fin = torch.isfinite(a) & torch.isfinite(g)
    z = a[fin].clone().requires_grad_(True)
    al = alpha.detach().clone().requires_grad_(True)
    F.prelu(z, al).backward(g[fin])
    assert torch.allclose(terms[fin].sum(), al.grad.sum(), rtol=1e-12, atol=0.0)


def test_maxpool_table_agrees_with_torch():
    s = nf.special_values()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 4, 6, 40, generator=g)
    k = 0
    for pos in range(4):                                        # every special in each of the four window positions
        for j in range(s.numel()):
            x[k % 3, (k // 3) % 2 * 2 + pos // 2, (k // 6) % 3 * 2 + pos % 2, (7 * k) % 40] = s[j]
            k += 1
    want = F.max_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    assert torch.isnan(want).any() and torch.isinf(want).any()
    assert nf.nan_equal(nf.maxpool2x2(x), want)
    # an odd height / width drops the last row / column, as torch does
    assert nf.nan_equal(nf.maxpool2x2(x[:, :3, :5]), F.max_pool2d(x[:, :3, :5].permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_rounding_tables_agree_with_torch(dtype):
    g = torch.Generator().manual_seed(1)
    v = torch.cat([nf.special_values(), nf.ties(dtype), torch.randn(4096, generator=g) * 37.0,
                   torch.randn(256, generator=g) * 1e-6, torch.tensor([65504.0, 65519.9, 65520.0, 3.38e38, 3.39e38, 6e-8, 2.9e-8, 3.0e-8])])
    assert nf.nan_equal(nf.round_to(v, dtype), v.to(dtype).float())
    t = nf.ties(dtype)
    assert t.numel() % 4 == 0 and torch.isfinite(t).all()
    r = t.to(dtype).float()
    fin = torch.isfinite(r)
    assert (r != t)[fin].all() and fin.sum() >= t.numel() - 4          # a tie is never representable; the top ones overflow
    up, down = (r > t)[fin].sum().item(), (r < t)[fin].sum().item()
    assert up > 0 and down > 0                                         # ties go both ways: to the even neighbour
    hi, lo = nf.split_bf16(nf.special_values())
    assert nf.nan_equal(hi, nf.special_values().bfloat16().float())
    assert nf.nan_equal(lo, (nf.special_values() - nf.special_values().bfloat16().float()).bfloat16().float())
    assert hi[1] == nf.INF and torch.isnan(lo[1])                      # split(inf) = (inf, nan): bf16x3 turns Inf into NaN
    assert torch.isinf(hi[6]) and not torch.isfinite(lo[6])            # FLT_MAX rounds up to inf in bf16
