"""NV12 / I420 pixel formats without a GPU: the coefficient function against the recorded table, the fixed-point conversion
against the float64 matrix over every byte triple, the numpy reference's two layouts, every refusal that must come before a
launch, and the four C entries."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import yuv_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cer_frames_transform_yuv", "cer_frames_stream_append_yuv", "cer_frames_transform_boxes_yuv",
           "cer_frames_stream_append_boxes_yuv")
PAIRS = sorted(yuv_ref.COEFFICIENTS)


def _frames():
    from feature_vs_text_compound_emotion_amd import frames
    return frames


@pytest.mark.parametrize("matrix,range_", PAIRS)
def test_coefficients_equal_the_recorded_table(matrix, range_):
    frames = _frames()
    got = frames.yuv_coefficients(matrix, range_)
    assert got == yuv_ref.COEFFICIENTS[matrix, range_] and all(type(v) is int for v in got)
    assert frames.yuv_coefficients() == yuv_ref.COEFFICIENTS["bt601", "limited"]            # the defaults
    d = frames.yuv_desc("i420", matrix, range_)
    assert (d.layout, d.cy, d.crv, d.cgu, d.cgv, d.cbu, d.yoff) == (1,) + got
    assert frames.yuv_desc("nv12", matrix, range_).layout == 0 and frames.yuv_desc("rgb24", matrix, range_) is None


@pytest.mark.parametrize("matrix,range_", PAIRS)
def test_fixed_point_is_within_one_of_the_float_matrix_over_every_byte_triple(matrix, range_):
    """All 2^24 (Y, U, V): the integers differ from clip(floor(float64 + 0.5)) by at most 1 in any channel, in at most 0.39 %
    of the triples; and no intermediate sum leaves 9.3e6 (int32 suffices)."""
    u, v = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    worst, differ = 0, 0
    for y in range(256):
        fixed, exact = yuv_ref.convert(y + 0 * u, u, v, matrix, range_), yuv_ref.convert_float(y + 0 * u, u, v, matrix, range_)
        d = np.abs(fixed.astype(np.int16) - exact)
        worst, differ = max(worst, int(d.max())), differ + int(d.any(axis=-1).sum())
    print(matrix, range_, "max difference", worst, "triples that differ", differ, f"{100 * differ / 2 ** 24:.3f} %")
    assert worst == 1 and differ <= 0.0039 * 2 ** 24
    cy, crv, cgu, cgv, cbu, yoff = yuv_ref.COEFFICIENTS[matrix, range_]
    assert cy * max(255 - yoff, yoff) + 128 * max(abs(crv), abs(cgu) + abs(cgv), abs(cbu)) + (1 << 13) < 9.3e6


def test_reference_layouts_and_siting():
    rng = np.random.default_rng(3)
    y = rng.integers(0, 256, (2, 4, 6), dtype=np.uint8)
    u, v = rng.integers(0, 256, (2, 2, 2, 3), dtype=np.uint8)
    nv12, i420 = yuv_ref.pack(y, u, v, "nv12"), yuv_ref.pack(y, u, v, "i420")
    assert nv12.shape == i420.shape == (2, 6, 6) and np.array_equal(nv12[:, :4], y) and np.array_equal(i420[:, :4], y)
    assert nv12[0, 4].tolist() == [u[0, 0, 0], v[0, 0, 0], u[0, 0, 1], v[0, 0, 1], u[0, 0, 2], v[0, 0, 2]]      # U first
    assert i420[0, 4].tolist() == u[0].ravel().tolist() and i420[0, 5].tolist() == v[0].ravel().tolist()
    for frames, layout in ((nv12, "nv12"), (i420, "i420")):
        for got, want in zip(yuv_ref.planes(frames, layout), (y, u, v)):
            assert np.array_equal(got, want)
    rgb = yuv_ref.yuv_to_rgb(nv12, "nv12")
    assert rgb.shape == (2, 4, 6, 3) and np.array_equal(rgb, yuv_ref.yuv_to_rgb(i420, "i420"))
    assert np.array_equal(rgb[1, 3, 5], yuv_ref.convert(y[1, 3, 5], u[1, 1, 2], v[1, 1, 2]))      # (x >> 1, y >> 1)
    # limited-range black, white and grey; zero bytes are not black
    assert yuv_ref.convert(16, 128, 128).tolist() == [0, 0, 0] and yuv_ref.convert(235, 128, 128).tolist() == [255, 255, 255]
    assert yuv_ref.convert(0, 0, 0).tolist() == [0, 136, 0] and yuv_ref.convert(255, 255, 255).tolist() == [255, 125, 255]
    assert yuv_ref.convert(126, 128, 128, range="full").tolist() == [126] * 3


def test_constructors_refuse_unknown_names():
    frames = _frames()
    from feature_vs_text_compound_emotion_amd import live
    for make in (lambda **kw: frames.FrameTransform(48, 40, train=False, **kw), lambda **kw: frames.FrameStream(2, **kw)):
        for kw, match in (({"pixel_format": "nv21"}, "pixel_format"), ({"pixel_format": "NV12"}, "pixel_format"),
                          ({"pixel_format": "nv12", "matrix": "bt2020"}, "matrix"), ({"matrix": "bt2020"}, "matrix"),
                          ({"pixel_format": "i420", "range": "tv"}, "range"), ({"range": None}, "range")):
            with pytest.raises(ValueError, match=match):
                make(**kw)
    assert frames.FrameTransform().yuv is None and frames.FrameStream(2)._xf.yuv is None
    fs = frames.FrameStream(2, pixel_format="i420", matrix="bt709", range="full")
    assert (fs.pixel_format, fs._xf.yuv.layout, fs._xf.yuv.cbu, fs._xf.yuv.yoff) == ("i420", 1, 30402, 0)
    mine = ("pixel_format", "matrix", "range")
    for cls, names in ((frames.FrameTransform, mine), (frames.FrameStream, mine),
                       (live.AVStream, ("video_format", "video_matrix", "video_range"))):
        sig = inspect.signature(cls.__init__).parameters
        assert [sig[n].default for n in names] == ["rgb24", "bt601", "limited"], cls
    sig = inspect.signature(live.AVStream.__init__).parameters
    assert all(sig[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("video_format", "video_matrix", "video_range"))


BAD_FRAMES = [
    ((2, 9, 7), "even W"),                      # odd W
    ((2, 9, 0), "even W"),
    ((2, 8, 8), r"H \* 3 / 2"),                 # 8 rows: no even H has them
    ((2, 10, 8), r"H \* 3 / 2"),                # H = 20 / 3
    ((2, 2, 8), r"H \* 3 / 2"),
    ((2, 0, 8), r"H \* 3 / 2"),
    ((2, 6, 8, 3), r"\[M, H \* 3 / 2, W\]"),    # an RGB tensor
    ((2, 6), r"\[M, H \* 3 / 2, W\]"),
    ((2, 6, 8), "must be on the GPU"),          # a good shape: the CPU tensor is what is refused
]


@pytest.mark.parametrize("layout", yuv_ref.LAYOUTS)
@pytest.mark.parametrize("shape,match", BAD_FRAMES)
def test_frame_stream_refuses_bad_yuv_frames_with_the_ints_unchanged(shape, match, layout):
    frames = _frames()
    fs = frames.FrameStream(2, hold=4, max_new=3, pixel_format=layout)
    fs.frames_seen, fs.frames_taken = [3, 1], [2, 0]
    u8 = torch.zeros(shape, dtype=torch.uint8)
    for call in (fs.check_push, fs.push):
        with pytest.raises(ValueError, match="frames: .*" + match):
            call(u8, [1, 1])
        with pytest.raises(ValueError, match="frames: .*" + match):
            call(u8, [1, 1], boxes=[[0, 0, 4, 4], [1, 1, 2, 2]])
    with pytest.raises(ValueError, match="uint8 tensor"):
        fs.check_push(torch.zeros((2, 6, 8)), [1, 1])
    with pytest.raises(ValueError, match="boxes: .*empty"):           # the boxes are still looked at first
        fs.check_push(torch.zeros((2, 6, 8), dtype=torch.uint8), [1, 1], [[0, 0, 4, 4], [5, 0, 5, 4]])
    assert fs.frames_seen == [3, 1] and fs.frames_taken == [2, 0] and fs.ring is None


def test_rgb_mode_refusal_texts_are_unchanged():
    frames = _frames()
    fs = frames.FrameStream(2, hold=4, max_new=3)
    for shape in ((2, 6, 8), (2, 6, 8, 3)):
        with pytest.raises(ValueError, match=r"frames: expected raw RGB frames as a uint8 GPU tensor \[M, H, W, 3\] \(there is no CPU "
                                             r"fallback\), got \(torch.uint8, device\(type='cpu'\), "):
            fs.check_push(torch.zeros(shape, dtype=torch.uint8), [1, 1])
    with pytest.raises(RuntimeError, match=r"FrameTransform needs a uint8 CUDA tensor \[B,L,H,W,3\] \(there is no CPU fallback\)"):
        frames.FrameTransform(48, 40, train=False)(torch.zeros((1, 2, 6, 8, 3), dtype=torch.uint8))


@pytest.mark.parametrize("shape,match", [((1, 2, 9, 7), "even W"), ((2, 8, 8), r"H \* 3 / 2"), ((1, 2, 6, 8, 3), "uint8 tensor"),
                                         ((6, 8), "uint8 tensor"), ((2, 6, 8), "must be on the GPU")])
def test_frame_transform_refuses_bad_yuv_clips(shape, match):
    xf = _frames().FrameTransform(48, 40, train=False, pixel_format="nv12")
    with pytest.raises(ValueError, match=match):
        xf(torch.zeros(shape, dtype=torch.uint8))
    with pytest.raises(ValueError, match=match):
        xf(torch.zeros(shape, dtype=torch.uint8), boxes=[[0, 0, 4, 4]] * 2)


def test_yuv_picture():
    frames = _frames()
    assert frames.yuv_picture(3, 2) == (2, 2) and frames.yuv_picture(1080, 1280) == (720, 1280) and frames.yuv_picture(147, 130) == (98, 130)


def test_the_four_entries_are_declared_exported_and_bound():
    from feature_vs_text_compound_emotion_amd import _lib
    text = open(os.path.join(ROOT, "include", "cer_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _lib.exported_symbols() and getattr(raw, name) is not None
        assert getattr(_lib.load(), name).argtypes == _lib._SIGNATURES[name][1]
        # the sibling's arguments, with the descriptor after the frames
        rgb = _lib._SIGNATURES[name[:-4]][1]
        assert _lib._SIGNATURES[name][1] == [rgb[0], ctypes.POINTER(_lib.Yuv420Desc)] + rgb[1:], name
    assert re.search(r"#define\s+CER_YUV_PREC\s+14\b", text) and _lib.YUV_PREC == 14
    assert re.search(r"#define\s+CER_YUV_NV12\s+0\b", text) and re.search(r"#define\s+CER_YUV_I420\s+1\b", text)
    assert (_lib.YUV_NV12, _lib.YUV_I420) == (0, 1) and ctypes.sizeof(_lib.Yuv420Desc) == 28


def test_c_entries_refuse_the_picture_and_the_descriptor_before_any_launch():
    from feature_vs_text_compound_emotion_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))      # never dereferenced: every case below is refused first
    good = (0,) + yuv_ref.COEFFICIENTS["bt601", "limited"]

    def desc(d):
        return None if d is None else ctypes.byref(_lib.Yuv420Desc(*d))

    calls = {
        "frames_transform_yuv": lambda d, h, w: lib.cer_frames_transform_yuv(
            p, desc(d), 1, h, w, p, p, 3, p, p, 3, 6, 4, p, 1, 2, 0.5, 0.5, p, None, None),
        "frames_stream_append_yuv": lambda d, h, w: lib.cer_frames_stream_append_yuv(
            p, desc(d), 1, h, w, p, p, 3, p, p, 3, 6, 4, p, 2, p, p, 1, 1, p, 1, 8, None),
        "frames_transform_boxes_yuv": lambda d, h, w: lib.cer_frames_transform_boxes_yuv(
            p, desc(d), 1, h, w, p, p, p, 16, 8, 7, 6, 4, p, 1, 0.5, 0.5, p, None, None),
        "frames_stream_append_boxes_yuv": lambda d, h, w: lib.cer_frames_stream_append_boxes_yuv(
            p, desc(d), 1, h, w, p, p, p, 16, 8, 7, 6, 4, p, p, p, 1, 1, p, 1, 8, None),
    }
    cases = [(None, 8, 8, b"null"), (good, 7, 8, b"even H and W"), (good, 8, 9, b"even H and W"), (good, 0, 8, b"even H and W"),
             (good, 1 << 15, 1 << 15, b"2^29"), ((2,) + good[1:], 8, 8, b"layout"), ((-1,) + good[1:], 8, 8, b"layout"),
             (good[:2] + (1 << 21,) + good[3:], 8, 8, b"coefficient"), (good[:5] + (-(1 << 21),) + good[6:], 8, 8, b"coefficient"),
             (good[:6] + (256,), 8, 8, b"yoff"), (good[:6] + (-1,), 8, 8, b"yoff")]
    for name, call in calls.items():
        for d, h, w, text in cases:
            assert call(d, h, w) != 0, (name, d, h, w)
            msg = lib.cer_last_error()
            assert msg.startswith(name.encode() + b":") and text in msg, (name, msg)
    # what the RGB sibling refuses is refused too: crop above size through the boxed pair, a ring length of 6
    assert lib.cer_frames_transform_boxes_yuv(p, desc(good), 1, 8, 8, p, p, p, 16, 8, 7, 6, 7, p, 1, 0.5, 0.5, p, None, None) != 0
    assert lib.cer_last_error().startswith(b"frames_transform_boxes_yuv:") and b"exceeds size" in lib.cer_last_error()
    assert lib.cer_frames_stream_append_yuv(p, desc(good), 1, 8, 8, p, p, 3, p, p, 3, 6, 4, p, 2, p, p, 1, 1, p, 1, 6, None) != 0
    assert b"power of two" in lib.cer_last_error()
