"""The Python marshalling under the conv wrappers and the IR-50 packers: ``ops.conv2d`` launches through ``cer_conv2d_run``
like the bf16x3 / narrow wrappers (and stays bit-equal to the documented C call ``cer_conv2d_fwd``), keeps its three return
conventions, stays out of ``CONV_TRACE``; the pack caches live in one dict."""
import copy
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

# (N, H, W, Cin, Cout, stride): the scalar small-Cin kernel and the vector (Cin % 32 == 0) kernel
SCALAR = (1, 5, 5, 3, 8, 1)
VECTOR = (1, 6, 6, 32, 64, 2)


def _operands(shape, seed):
    from feature_vs_text_compound_emotion_amd import ops
    n, h, w, cin, cout, _ = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, cin, generator=g).cuda()
    wp = ops.pack_conv_weight((torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5).cuda())
    bias, alpha = torch.randn(cout, generator=g).cuda(), (torch.rand(cout, generator=g) * 0.3 + 0.1).cuda()
    return x, wp, bias, alpha


@pytest.mark.parametrize("shape,epilogue", [(SCALAR, True), (VECTOR, False)], ids=["scalar", "vector"])
def test_cer_conv2d_fwd_is_bit_equal_to_ops_conv2d(shape, epilogue):
    """Nothing in Python calls ``cer_conv2d_fwd`` any more: it stays the C call for integrators, so it is called here."""
    from feature_vs_text_compound_emotion_amd import _lib, ops
    n, h, w, cin, cout, stride = shape
    x, wp, bias, alpha = _operands(shape, 11)
    if not epilogue:
        bias = alpha = None
    act1 = ops.ACT_PRELU if epilogue else ops.ACT_NONE
    want = ops.conv2d(x, wp, 3, 3, stride=stride, pad=(1, 1), bias=bias, alpha=alpha, act1=act1)
    d = ops._conv_desc(n, h, w, cin, cout, 3, 3, stride=stride, pad=(1, 1), act1=act1)
    assert tuple(want.shape) == (n, d.Ho, d.Wo, cout)
    got = torch.full_like(want, float("nan"))
    rc = _lib.load().cer_conv2d_fwd(ctypes.byref(d), _lib.ptr(x), _lib.ptr(wp), None, None, _lib.ptr(bias), _lib.ptr(alpha), None,
                                    None, _lib.ptr(got), None, None, None, 0, _lib.current_stream())
    _lib.check(rc, "cer_conv2d_fwd")
    assert torch.equal(got, want)


@pytest.mark.parametrize("shape", [SCALAR, VECTOR], ids=["scalar", "vector"])
def test_conv2d_return_conventions(shape):
    from feature_vs_text_compound_emotion_amd import ops
    n, h, w, cin, cout, stride = shape
    x, wp, bias, alpha = _operands(shape, 12)
    kw = dict(stride=stride, pad=(1, 1), bias=bias, alpha=alpha, act1=ops.ACT_PRELU)
    y = ops.conv2d(x, wp, 3, 3, **kw)
    assert isinstance(y, torch.Tensor)
    pair = ops.conv2d(x, wp, 3, 3, want_stats=True, **kw)
    assert isinstance(pair, tuple) and len(pair) == 2
    assert torch.equal(pair[0], y) and pair[1].shape[1:] == (2, cout)
    s2, t2 = (torch.rand(cout) + 0.5).cuda(), torch.randn(cout).cuda()
    for extra, key in ((dict(out_split=True), "split"), (dict(next_affine=(s2, t2)), "next"), (dict(out_n16=torch.bfloat16), "n16")):
        for want_stats in (False, True):
            r = ops.conv2d(x, wp, 3, 3, want_stats=want_stats, **extra, **kw)
            assert isinstance(r, dict) and set(r) == {"y", "stats", key}
            assert torch.equal(r["y"], y)
            assert tuple(r[key].shape) == tuple(y.shape)
            if want_stats:
                assert torch.equal(r["stats"], pair[1])
            else:
                assert r["stats"] is None
    # the extra outputs are the fp32 result in their storage
    ref = ops.split_bf16(y)
    r = ops.conv2d(x, wp, 3, 3, out_split=True, **kw)["split"]
    assert torch.equal(r.hi, ref.hi) and torch.equal(r.lo, ref.lo)
    assert torch.equal(ops.conv2d(x, wp, 3, 3, out_n16=torch.bfloat16, **kw)["n16"], y.to(torch.bfloat16))


def test_conv_trace_takes_the_bf16x3_and_narrow_convs_only():
    from feature_vs_text_compound_emotion_amd import ops
    n, hw, cin, cout = 1, 8, 64, 64
    g = torch.Generator().manual_seed(13)
    x = torch.randn(n, hw, hw, cin, generator=g).cuda()
    wp = ops.pack_conv_weight((torch.randn(cout, cin, 3, 3, generator=g) / 24.0).cuda())
    xs, ws = ops.split_bf16(x), ops.split_bf16(wp)
    xn, wn = ops.to_n16(x, torch.bfloat16), ops.to_n16(wp, torch.bfloat16)
    nout = n * hw * hw * cout
    flops = 2.0 * n * hw * hw * cout * cin * 3 * 3
    assert ops.CONV_TRACE is None
    ops.CONV_TRACE = trace = []
    try:
        ops.conv2d(x, wp, 3, 3, pad=(1, 1))
        assert trace == []
        ops.conv2d_b3(xs, ws, 3, 3, pad=(1, 1))
        assert len(trace) == 1 and len(trace[0]) == 5
        ops.conv2d_n16(xn, wn, 3, 3, pad=(1, 1))
        assert len(trace) == 2 and len(trace[1]) == 5
        ops.conv2d(x, wp, 3, 3, pad=(1, 1), out_split=True)
        assert len(trace) == 2
    finally:
        ops.CONV_TRACE = None
    b3, n16 = trace
    assert b3[0] == ops.conv2d_b3_tile(n, hw, hw, cin, cout, 3, 3, 1, (1, 1)) != 0
    assert n16[0] == ops.conv2d_n16_tile(n, hw, hw, cin, cout, 3, 3, 1, (1, 1)) != 0
    assert b3[1] == flops and n16[1] == flops
    # split input (4 B/elt) + the one Split output + split weights; narrow: 2 B/elt each
    assert b3[4] == 4.0 * n * hw * hw * cin + 4.0 * nout * (0 + 1 + 0) + 4.0 * cout * cin * 3 * 3 + 0.0
    assert n16[4] == 2.0 * n * hw * hw * cin + nout * (4.0 * 0 + 2.0 * 1) + 2.0 * cout * cin * 3 * 3 + 0.0
    torch.cuda.synchronize()
    for e in (b3, n16):
        assert e[2].elapsed_time(e[3]) >= 0.0


def test_ir50_pack_caches():
    from feature_vs_text_compound_emotion_amd.visual_backbone import IR50
    torch.manual_seed(14)
    model = IR50(head_hw=5).cuda().eval()
    for p in model.parameters():
        p.requires_grad = False
    P = model.pack_b3()
    assert model.pack_b3() is P
    bn = model.body[3].res_layer[4]
    bn.running_mean.add_(0)                       # same values, new version: the fold is stale as far as the cache can tell
    P2 = model.pack_b3()
    assert P2 is not P and model.pack_b3() is P2
    Nb = model.pack_n16(torch.bfloat16)
    assert model.pack_n16(torch.bfloat16) is Nb
    Nh = model.pack_n16(torch.float16)
    assert Nh is not Nb and Nh["head_w"].dtype == torch.float16 and model.pack_n16(torch.float16) is Nh
    F = model.pack()
    assert {k for k in model._packs} == {("fp32", False), ("b3", False), ("n16", False)}

    clone = copy.deepcopy(model)
    assert clone._packs == {} and clone._packs is not model._packs
    assert model.pack_b3() is P2 and model.pack_n16(torch.float16) is Nh and model.pack() is F   # the original's cache is intact
    theirs = clone.pack_b3()
    assert theirs is not P2 and torch.equal(theirs["head_w"].hi, P2["head_w"].hi)
    assert theirs["units"][0]["w1"].hi.data_ptr() != P2["units"][0]["w1"].hi.data_ptr()

    T = model.pack_train_b3()
    assert model.pack_train_b3() is T
    model.train()
    x = torch.randn(2, 3, 40, 40, generator=torch.Generator().manual_seed(15)).cuda()
    with torch.no_grad():
        model(x)                                  # bf16x3, batch statistics: the running statistics move
    assert set(model._packs) == {("b3", True)} and model.pack_train_b3() is T
    assert model.pack_b3() is not P2
