"""``ops._conv_desc``, the one place a conv's geometry is worked out, against the formula written out here.  Pure Python and
ctypes: nothing in this file loads the library (no ``kpad`` is passed, so ``conv_kpad`` is never asked)."""
import pytest

from feature_vs_text_compound_emotion_amd import _lib, ops


def _out(size, k, stride, pad, dil):
    return (size + 2 * pad - dil * (k - 1) - 1) // stride + 1


@pytest.mark.parametrize("hw", [5, 6, 7])
@pytest.mark.parametrize("stride", [1, 2])
def test_3x3_pad1_output_size(hw, stride):
    d = ops._conv_desc(2, hw, hw + 1, 16, 32, 3, 3, stride=stride, pad=(1, 1))
    assert (d.N, d.H, d.W, d.Cin, d.Cout, d.KH, d.KW) == (2, hw, hw + 1, 16, 32, 3, 3)
    assert (d.stride, d.dil_h, d.dil_w, d.pad_t, d.pad_l) == (stride, 1, 1, 1, 1)
    assert d.Ho == _out(hw, 3, stride, 1, 1) and d.Wo == _out(hw + 1, 3, stride, 1, 1)
    # stride 1 keeps the size; stride 2 gives ceil(size / 2) on odd and even sizes alike
    assert (d.Ho, d.Wo) == ((hw, hw + 1) if stride == 1 else ((hw + 1) // 2, (hw + 2) // 2))


def test_dilation_and_asymmetric_padding():
    d = ops._conv_desc(1, 20, 11, 8, 8, 5, 3, dil=(2, 1), pad=(4, 0))
    assert (d.dil_h, d.dil_w, d.pad_t, d.pad_l) == (2, 1, 4, 0)
    assert d.Ho == _out(20, 5, 1, 4, 2) == 20
    assert d.Wo == _out(11, 3, 1, 0, 1) == 9


def test_explicit_out_hw_overrides_the_formula():
    d = ops._conv_desc(1, 9, 9, 4, 4, 3, 3, stride=2, pad=(1, 1), out_hw=(4, 3))
    assert (d.Ho, d.Wo) == (4, 3)
    assert (d.H, d.W) == (9, 9)


def test_x_s2d_unfolds_the_tensor_shape():
    d = ops._conv_desc(1, 3, 4, 256, 128, 3, 3, stride=2, pad=(1, 1), x_s2d=True)
    assert (d.N, d.H, d.W, d.Cin) == (1, 6, 8, 64)
    assert (d.Ho, d.Wo) == (_out(6, 3, 2, 1, 1), _out(8, 3, 2, 1, 1)) == (3, 4)
    assert d.x_s2d == 1 and d.y_s2d == 0


def test_x_s2d_needs_four_channel_blocks():
    with pytest.raises(ValueError, match="space-to-depth"):
        ops._conv_desc(1, 3, 4, 254, 128, 3, 3, stride=2, pad=(1, 1), x_s2d=True)


def test_defaults_are_the_wrappers_defaults():
    d = ops._conv_desc(1, 4, 4, 8, 8, 1, 1)
    assert (d.stride, d.dil_h, d.dil_w, d.pad_t, d.pad_l) == (1, 1, 1, 0, 0)
    assert (d.split_k, d.res_stride, d.Hr, d.Wr, d.storage) == (1, 1, 0, 0, _lib.STORE_NONE)
    assert (d.act1, d.act2, d.tile, d.x_nchw, d.x_ld, d.y_ld, d.x_s2d, d.y_s2d) == (_lib.ACT_NONE, _lib.ACT_NONE, 0, 0, 0, 0, 0, 0)
    assert d.slope == pytest.approx(ops.LEAKY_SLOPE, rel=1e-7)  # a C float


def test_optional_fields_land_in_their_slots():
    d = ops._conv_desc(2, 8, 8, 3, 16, 3, 3, pad=(1, 1), res_stride=2, Hr=16, Wr=15, act1=_lib.ACT_PRELU, act2=_lib.ACT_RELU,
                       slope=0.25, split_k=4, tile=7, x_nchw=True, x_ld=96, y_ld=48, storage=_lib.STORE_F16, y_s2d=True)
    assert (d.res_stride, d.Hr, d.Wr, d.act1, d.act2, d.slope) == (2, 16, 15, _lib.ACT_PRELU, _lib.ACT_RELU, 0.25)
    assert (d.split_k, d.tile, d.x_nchw, d.x_ld, d.y_ld, d.storage, d.x_s2d, d.y_s2d) == (4, 7, 1, 96, 48, _lib.STORE_F16, 0, 1)
