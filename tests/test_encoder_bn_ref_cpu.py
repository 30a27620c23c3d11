"""``tests/encoder_bn_ref.py`` proved against torch, without a GPU: the restatement that ``tests/test_encoder_bn_edges_gpu.py`` holds
``csrc/encoder_bn.hip`` to, its statistics partition against the library's host function, and the exactness of its data."""
import pytest
import torch
import torch.nn.functional as F

import encoder_bn_ref as br
import nonfinite_ref as nf


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------- apply + finalize == F.batch_norm
@pytest.mark.parametrize("n,h,w,c,rows", [(2, 6, 5, 64, 128), (3, 7, 4, 5, 16), (1, 1, 1, 3, 128), (4, 9, 9, 8, 100)])
def test_finalize_then_apply_is_train_mode_batch_norm(n, h, w, c, rows):
    g = _gen(n * 100 + c)
    x = (torch.randn(n, h, w, c, generator=g, dtype=torch.float64) * 2.0 + 1.0).float()
    gamma, beta = torch.randn(c, generator=g), torch.randn(c, generator=g)
    rm0, rv0 = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    mom, eps = br.f32(0.1), br.f32(1e-5)
    # fp32 partials that ARE the float64 sums: multiples of 1/8 below 16, so every sum of <= 128 of them and of their squares fits
    x = (x * 8.0).round() / 8.0
    partials = br.tile_rows(x.double(), rows)
    assert torch.equal(partials.float().double(), partials)
    p = n * h * w
    fin = br.finalize_ref(partials.float(), p, gamma, beta, rm0, rv0, mom, eps)
    out, _ = br.apply_ref(x, fin["scale"], fin["shift"])
    rm, rv = rm0.double().clone(), rv0.double().clone()
    if p > 1:
        want = F.batch_norm(x.double().permute(0, 3, 1, 2), rm, rv, gamma.double(), beta.double(), True, mom, eps).permute(0, 2, 3, 1)
        assert torch.allclose(fin["rm"], rm, rtol=1e-12, atol=1e-13) and torch.allclose(fin["rv"], rv, rtol=1e-12, atol=1e-13)
    else:                                            # torch refuses one value per channel: the formula at count == 1
        want = beta.double().expand(x.shape)
        assert torch.equal(fin["var"], torch.zeros(c, dtype=torch.float64)) and torch.equal(fin["unbiased"], fin["var"])
        assert torch.allclose(fin["rm"], (1 - mom) * rm0.double() + mom * x.double().reshape(c), rtol=1e-12, atol=1e-13)
        assert torch.allclose(fin["rv"], (1 - mom) * rv0.double(), rtol=1e-12, atol=1e-13)
    assert torch.allclose(out, want, rtol=1e-10, atol=1e-10)
    assert torch.equal(fin["sums"], torch.stack([x.double().reshape(p, c).sum(0), (x.double() ** 2).reshape(p, c).sum(0)]))


def test_finalize_ref_clamps_the_variance_and_takes_the_biased_one_for_a_single_value():
    c = 4
    gamma, beta = torch.ones(c), torch.zeros(c)
    # sum of squares below count * mean^2: a negative variance that must read as 0
    partials = torch.tensor([[[8.0] * c, [7.9] * c]])
    fin = br.finalize_ref(partials, 8, gamma, beta, torch.zeros(c), torch.ones(c), 0.5, 0.25)
    assert torch.equal(fin["var"], torch.zeros(c, dtype=torch.float64))
    assert torch.equal(fin["scale"], torch.full((c,), 2.0, dtype=torch.float64)) and torch.equal(fin["shift"], torch.full((c,), -2.0, dtype=torch.float64))
    assert torch.equal(fin["rv"], torch.full((c,), 0.5, dtype=torch.float64))
    one = br.finalize_ref(torch.tensor([[[3.0] * c, [10.0] * c]]), 1, gamma, beta, torch.zeros(c), torch.zeros(c), 0.5, 0.25)
    assert torch.equal(one["var"], torch.ones(c, dtype=torch.float64)) and torch.equal(one["unbiased"], one["var"])
    two = br.finalize_ref(torch.tensor([[[6.0] * c, [20.0] * c]]), 2, gamma, beta)
    assert torch.equal(two["unbiased"], 2.0 * two["var"]) and "rm" not in two


def test_apply_ref_is_the_moved_helper_and_each_part_alone():
    g = _gen(5)
    n, h, w, c = 2, 3, 5, 8
    y, res = torch.randn(n, h, w, c, generator=g), torch.randn(n, h, w, c, generator=g)
    scale, shift, alpha = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g), torch.rand(c, generator=g) * 0.3 + 0.1
    rs, rt = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    mask = (torch.rand(n, h, w, c, generator=g) > 0.3).float() * 2.0
    want, bound = br.bn_apply_ref(y, res, scale, shift, alpha, rs, rt, mask)
    out, b = br.apply_ref(y, scale, shift, alpha, mask, res, 1, rs, rt)
    assert torch.equal(out.float(), want) and torch.equal(b, bound)
    # against torch's own operators, part by part
    v = y.double() * scale.double() + shift.double()
    assert torch.equal(br.apply_ref(y, scale, shift)[0], v)
    assert torch.equal(br.apply_ref(y, scale, shift, alpha=alpha)[0], F.prelu(v.permute(0, 3, 1, 2), alpha.double()).permute(0, 2, 3, 1))
    assert torch.equal(br.apply_ref(y, scale, shift, mask=mask)[0], v * mask.double())
    assert torch.equal(br.apply_ref(y, scale, shift, res=res)[0], v + res.double())
    # a negative scale keeps the bound positive
    assert (br.apply_ref(y, -scale, shift, res=res, res_scale=-rs, res_shift=rt)[1] > 0).all()


@pytest.mark.parametrize("stride,hr,wr", [(2, 5, 9), (2, 6, 10), (2, 5, 10), (1, 4, 5), (3, 7, 13)])
def test_apply_ref_reads_the_strided_residual_pixel_by_pixel(stride, hr, wr):
    n, ho, wo, c = 3, 3, 5, 4
    g = _gen(stride * 100 + hr)
    d = br.exact_inputs(g, n, ho, wo, c, res_hw=(hr, wr))
    out, _ = br.apply_ref(d["y"], d["scale"], d["shift"], res=d["res"], res_stride=stride)
    base = d["y"].double() * d["scale"].double() + d["shift"].double()
    for b in range(n):
        for i in range(ho):
            for j in range(wo):
                assert torch.equal(out[b, i, j], base[b, i, j] + d["res"][b, i * stride, j * stride].double())
    with pytest.raises(AssertionError):
        br.apply_ref(d["y"], d["scale"], d["shift"], res=d["res"][:, :(ho - 1) * stride], res_stride=stride)


# ---------------------------------------------------------------------------------------------- the statistics partition
PARTITION_P = [1, 127, 128, 129, 262144, 264191, 264192, 264193, 2048 * 2048 + 1]


@pytest.mark.parametrize("p", PARTITION_P)
def test_tiles_is_the_librarys_host_function(p):
    from feature_vs_text_compound_emotion_amd import _lib
    assert br.tiles(p) == _lib.load().cer_bn_apply_stats_tiles(p)
    r = br.rows_per_block(p)
    assert r % 128 == 0 and 128 <= r <= 2048 and (br.tiles(p) - 1) * r < p <= br.tiles(p) * r


def test_partition_steps_where_the_kernels_comment_says():
    assert br.tiles(0) == 0
    assert [br.rows_per_block(p) for p in (1, 262144, 264191, 264192, 264193)] == [128, 128, 128, 256, 256]
    assert br.rows_per_block(2048 * 2048 + 1) == 2048 and br.rows_per_block(2 ** 31 - 1) == 2048
    assert br.tiles(2048 * 2048) == 2048 and br.tiles(2048 * 2048 + 1) == 2049
    assert [br.rows_per_pass(c, 4) for c in (4, 8, 16, 64, 128, 256, 512, 1024)] == [256, 128, 64, 16, 8, 4, 2, 1]
    assert [br.rows_per_pass(c, 8) for c in (64, 128, 512, 2048)] == [32, 16, 4, 1]


def test_factor_rows_gives_rectangular_multi_image_shapes():
    for p in (1, 2, 3, 5, 7, 9, 15, 17, 63, 65, 127, 128, 129, 255, 257, 300, 264193):
        n, ho, wo = br.factor_rows(p)
        assert n * ho * wo == p and min(n, ho, wo) >= 1
    assert br.factor_rows(300) == (2, 2, 75) and br.factor_rows(128) == (2, 2, 32)
    assert all(br.factor_rows(p)[0] > 1 for p in (9, 15, 63, 65, 128, 129, 255, 300))


# ---------------------------------------------------------------------------------------------- the exact family
def test_exact_sets_meet_the_precondition_for_2048_row_tiles():
    """Two full 2048-row tiles of the full epilogue (and of each part alone): every value a multiple of 1/8 below 2^8 granules,
    every per-tile sum and sum of squares below 2^24 granules, and the float32, bfloat16 and float16 roundings all exact."""
    g = _gen(2048)
    n, ho, wo, c = 2, 32, 64, 16
    d = br.exact_inputs(g, n, ho, wo, c)
    variants = [dict(alpha=d["alpha"], mask=d["mask"], res=d["res"], res_scale=d["rs"], res_shift=d["rt"]), dict(alpha=d["alpha"]),
                dict(mask=d["mask"]), dict(res=d["res"]), dict(res=d["res"], res_scale=d["rs"], res_shift=d["rt"]), dict()]
    for kw in variants:
        out, _ = br.apply_ref(d["y"], d["scale"], d["shift"], **kw)
        assert out.abs().max().item() <= br.MAX_EXACT
        margin = br.exact_margin(out, 2048)
        assert margin < br.EXACT_LIMIT, margin
        assert margin > 2.0 ** 16                                      # the sums are not trivially small either
        assert torch.equal(out.float().double(), out)
        assert torch.equal(nf.round_bf16(out.float()).double(), out) and torch.equal(nf.round_f16(out.float()).double(), out)
        hi, lo = nf.split_bf16(out.float())
        assert torch.equal(hi.double(), out) and not lo.any()
        st = br.tile_rows(out, 2048)
        assert st.shape == (2, 2, c) and torch.equal(st.float().double(), st)
    for k in ("y", "res"):                                             # the operands a narrow plane carries
        assert torch.equal(nf.round_bf16(d[k]), d[k]) and torch.equal(nf.round_f16(d[k]), d[k])


def test_exact_margin_rejects_what_is_not_exact():
    ok = torch.full((1, 1, 4, 2), 0.125, dtype=torch.float64)
    assert br.exact_margin(ok, 128) == 4.0
    assert br.exact_margin(ok + 0.01, 128) == float("inf")                      # no multiple of the granule
    assert br.exact_margin(ok * 8 * 256, 128) == float("inf")                   # more than eight significant bits
    big = torch.full((1, 1, 2048, 1), 21.0, dtype=torch.float64)
    assert br.exact_margin(big, 2048) >= br.EXACT_LIMIT                         # the worst case of the sets is NOT covered
    assert br.exact_margin(big, 128) < br.EXACT_LIMIT


# ---------------------------------------------------------------------------------------------- fold_bn_3x3
@pytest.mark.parametrize("cin,cout,exact", [(1, 1, True), (3, 5, True), (100, 5, False), (32, 64, False)])
def test_fold_ref_is_the_conv_of_a_constant_shift_image(cin, cout, exact):
    g = _gen(cin * 10 + cout)
    if exact:
        w, s, t = (torch.randint(-4, 5, sh, generator=g).float() for sh in ((cout, cin, 3, 3), (cin,), (cin,)))
    else:
        w, s, t = torch.randn(cout, cin, 3, 3, generator=g), torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g)
    wf, b9 = br.fold_ref(w, s, t)
    assert torch.equal(wf, w.double() * s.double()[None, :, None, None])
    img = t.double()[None, :, None, None].expand(1, cin, 3, 3)
    want = F.conv2d(img, w.double(), None, 1, 1)[0]                          # [Cout, 3, 3]: border, inner and far-border pixels
    got = b9.reshape(3, 3, cout).permute(2, 0, 1)
    assert torch.equal(got, want) if exact else torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    # and the whole identity on a random image: conv(pad0(s x + t)) == conv'(pad0(x)) + bias9 by border case
    x = torch.randn(2, cin, 4, 5, generator=g, dtype=torch.float64)
    lhs = F.conv2d(x * s.double()[None, :, None, None] + t.double()[None, :, None, None], w.double(), None, 1, 1)
    ry = torch.tensor([0, 1, 1, 2])
    rx = torch.tensor([0, 1, 1, 1, 2])
    rhs = F.conv2d(x, wf, None, 1, 1) + b9[(3 * ry[:, None] + rx[None, :])].permute(2, 0, 1)[None]
    assert torch.allclose(lhs, rhs, rtol=1e-11, atol=1e-11)


def test_pack_3x3_layout_and_padding():
    assert [br.kpad_3x3(c) for c in (1, 3, 32, 100, 320)] == [32, 32, 288, 928, 2880]
    from feature_vs_text_compound_emotion_amd import _lib
    assert all(br.kpad_3x3(c) == _lib.load().cer_conv_kpad(3, 3, c) for c in (1, 3, 32, 100, 320))
    w = torch.arange(2 * 3 * 9, dtype=torch.float32).reshape(2, 3, 3, 3)
    p = br.pack_3x3(w, fill=7.0)
    assert p.shape == (2, 32) and (p[:, 27:] == 7.0).all()
    for o in range(2):
        for kh in range(3):
            for kw in range(3):
                for c in range(3):
                    assert p[o, (kh * 3 + kw) * 3 + c] == w[o, c, kh, kw]
