"""Surfaces without a GPU: the numpy reference of the new pixel formats against hand-written bytes, ``surface_layout`` and its
refusals, the shape refusals of the new formats with the state unchanged, the six ``_surface`` C entries and everything they
refuse before a launch, and the stand-alone argument-check program under the host sanitizers."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import surface_ref
import yuv_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIBLINGS = ("cer_frames_transform", "cer_frames_stream_append", "cer_frames_transform_boxes", "cer_frames_stream_append_boxes",
            "cer_frames_transform_affine", "cer_frames_stream_append_affine")
NEW = ("bgr24", "rgba32", "bgra32", "yuyv422", "uyvy422")


def _frames():
    from feature_vs_text_compound_emotion_amd import frames
    return frames


# ---------------------------------------------------------------------------------------------- 1. the reference
def test_reference_byte_orders_and_siting():
    px = np.array([[[[10, 20, 30, 99], [40, 50, 60, 98]]]], np.uint8)                       # [1, 1, 2, 4]
    assert surface_ref.to_rgb(px[..., :3], "rgb24").tolist() == [[[[10, 20, 30], [40, 50, 60]]]]
    assert surface_ref.to_rgb(px[..., :3], "bgr24").tolist() == [[[[30, 20, 10], [60, 50, 40]]]]
    assert surface_ref.to_rgb(px, "rgba32").tolist() == [[[[10, 20, 30], [40, 50, 60]]]]      # the fourth byte is dropped
    assert surface_ref.to_rgb(px, "bgra32").tolist() == [[[[30, 20, 10], [60, 50, 40]]]]
    # one row of four pixels: Y = 100, 110, 120, 130; pair 0 has (U, V) = (90, 200), pair 1 (160, 70)
    yuyv = np.array([100, 90, 110, 200, 120, 160, 130, 70], np.uint8).reshape(1, 1, 4, 2)
    uyvy = np.array([90, 100, 200, 110, 160, 120, 70, 130], np.uint8).reshape(1, 1, 4, 2)
    want = np.stack([yuv_ref.convert(y, u, v) for y, u, v in ((100, 90, 200), (110, 90, 200), (120, 160, 70), (130, 160, 70))])
    assert np.array_equal(surface_ref.to_rgb(yuyv, "yuyv422")[0, 0], want) and np.array_equal(surface_ref.to_rgb(uyvy, "uyvy422")[0, 0], want)
    assert not np.array_equal(surface_ref.to_rgb(uyvy, "yuyv422"), surface_ref.to_rgb(uyvy, "uyvy422"))
    # chroma is taken from the pixel's own row: two rows with different chroma differ
    two = np.concatenate([yuyv, yuyv], axis=1)
    two[0, 1, :, 1] = 7
    rgb = surface_ref.to_rgb(two, "yuyv422", "bt709", "full")
    assert np.array_equal(rgb[0, 1, 2], yuv_ref.convert(120, 7, 7, "bt709", "full")) and np.array_equal(rgb[0, 0], surface_ref.to_rgb(yuyv, "yuyv422", "bt709", "full")[0, 0])
    nv12 = np.random.default_rng(0).integers(0, 256, (2, 6, 4), dtype=np.uint8)
    assert np.array_equal(surface_ref.to_rgb(nv12, "nv12"), yuv_ref.yuv_to_rgb(nv12, "nv12"))


@pytest.mark.parametrize("fmt", surface_ref.FORMATS)
def test_embed_and_extract_round_trip(fmt):
    frames = _frames()
    h, w, m = 6, 8, 3
    kw = dict(pitch=w * 4 + 7, frame_stride=None)
    if fmt in yuv_ref.LAYOUTS:
        kw = dict(pitch=w + 7, chroma_pitch=w + 3, offsets=(5, 5 + (h + 3) * (w + 7)) if fmt == "nv12" else
                  (5, 5 + (h + 3) * (w + 7), 5 + (h + 3) * (w + 7) + (h // 2 + 3) * (w + 3)), frame_stride=400)
    lay = frames.surface_layout(fmt, h, w, **kw)
    rng = np.random.default_rng(1)
    tight = rng.integers(0, 256, surface_ref.tight_shape(fmt, m, h, w), dtype=np.uint8)
    fill = rng.integers(0, 256, (m, lay.frame_stride), dtype=np.uint8)
    buf = surface_ref.embed(tight, lay, fill)
    assert buf.shape == (m, lay.frame_stride) and np.array_equal(surface_ref.extract(buf, lay), tight)
    touched = buf != fill
    per_frame = tight[0].size
    assert touched.sum(axis=1).max() <= per_frame                     # nothing but the picture's bytes was written
    other = surface_ref.embed(tight, lay, 255 - fill)
    assert (other != buf).sum() == m * (lay.frame_stride - per_frame)   # and every other byte is the fill's
    # the library's own account of the planes is the reference's
    assert [(o, p, r, b) for o, p, r, b in lay.planes()] == surface_ref._planes(lay)
    assert lay.extent == max(o + (r - 1) * p + b for o, p, r, b in surface_ref._planes(lay))


# ---------------------------------------------------------------------------------------------- 2. layouts
def test_layout_defaults_are_tight_packing():
    frames = _frames()
    h, w = 98, 130
    for fmt, row in (("rgb24", 3 * w), ("bgr24", 3 * w), ("rgba32", 4 * w), ("bgra32", 4 * w), ("yuyv422", 2 * w), ("uyvy422", 2 * w)):
        lay = frames.surface_layout(fmt, h, w)
        assert (lay.pitch, lay.chroma_pitch, lay.offsets, lay.frame_stride, lay.chroma) == (row, None, (0,), row * h, "uv")
        assert lay.extent == lay.frame_stride == int(np.prod(surface_ref.tight_shape(fmt, 1, h, w)))
    nv12 = frames.surface_layout("nv12", h, w)
    assert (nv12.pitch, nv12.chroma_pitch, nv12.offsets, nv12.frame_stride) == (130, 130, (0, 12740), 19110)
    i420 = frames.surface_layout("i420", h, w)
    assert (i420.pitch, i420.chroma_pitch, i420.offsets, i420.frame_stride) == (130, 65, (0, 12740, 12740 + 49 * 65), 19110)
    assert frames.surface_layout("yuyv422", 1, 2).frame_stride == 4 and frames.surface_layout("bgr24", 1, 1).frame_stride == 3
    # a decoder's surface: pitch 256, luma padded to 112 rows
    dec = frames.surface_layout("nv12", h, w, pitch=256, offsets=(0, 256 * 112))
    assert (dec.chroma_pitch, dec.frame_stride, dec.extent) == (256, 256 * 112 + 49 * 256, 256 * 112 + 48 * 256 + 130)
    assert frames.surface_layout("i420", h, w, pitch=256).chroma_pitch == 128
    assert isinstance(nv12, frames.SurfaceLayout) and nv12 == frames.SurfaceLayout("nv12", h, w)
    assert all(type(v) is int for v in (nv12.pitch, nv12.frame_stride, *nv12.offsets))
    assert frames.surface_layout("bgr24", np.int64(4), np.int32(6), pitch=np.int64(20)).frame_stride == 80


def test_chroma_vu_exchanges_the_chroma_bytes_or_planes():
    frames = _frames()
    for fmt in ("nv12", "i420"):
        uv, vu = (frames.Surface(frames.surface_layout(fmt, 8, 8, chroma=c)).desc() for c in ("uv", "vu"))
        assert (uv.offset[1], uv.offset[2]) == (vu.offset[2], vu.offset[1]) and uv.offset[1] != uv.offset[2]
        assert uv.offset[0] == vu.offset[0] == 0 and list(uv.pitch) == list(vu.pitch) and uv.format == vu.format == 1
    d = frames.Surface(frames.surface_layout("nv12", 8, 8)).desc()
    assert (list(d.step), list(d.offset), list(d.pitch), d.frame_stride) == ([1, 2], [0, 64, 65], [8, 8], 96)
    d = frames.Surface(frames.surface_layout("i420", 8, 8, chroma="vu")).desc()                       # YV12
    assert (list(d.step), list(d.offset), list(d.pitch)) == ([1, 1], [0, 80, 64], [8, 4])
    d = frames.Surface(frames.surface_layout("bgra32", 8, 8, pitch=40), yuv_ref.COEFFICIENTS["bt709", "full"]).desc()
    assert (d.format, list(d.step), list(d.pos), list(d.pitch), list(d.offset), d.frame_stride) == (0, [4, 4], [2, 1, 0], [40, 40], [0, 0, 0], 320)
    assert (d.cy, d.crv, d.cgu, d.cgv, d.cbu, d.yoff) == yuv_ref.COEFFICIENTS["bt709", "full"]
    d = frames.Surface(frames.surface_layout("uyvy422", 8, 8)).desc()
    assert (d.format, list(d.step), list(d.pos)) == (2, [2, 4], [1, 0, 2])
    assert list(frames.Surface(frames.surface_layout("yuyv422", 8, 8)).desc().pos) == [0, 1, 3]
    assert (d.cy, d.yoff) == (19077, 16)                                                                # the defaults


REFUSED = [
    (("nv21", 8, 8), {}, "pixel_format"), (("NV12", 8, 8), {}, "pixel_format"),
    (("bgr24", 8.0, 8), {}, "height"), (("bgr24", 8, True), {}, "width"), (("bgr24", 0, 8), {}, "height"), (("bgr24", 8, -2), {}, "width"),
    (("bgr24", 8, 8), {"pitch": 24.0}, "pitch"), (("bgr24", 8, 8), {"pitch": True}, "pitch"), (("bgr24", 8, 8), {"pitch": "24"}, "pitch"),
    (("bgr24", 8, 8), {"frame_stride": 192.5}, "frame_stride"), (("bgr24", 8, 8), {"offsets": (0.0,)}, "offsets"),
    (("bgr24", 8, 8), {"offsets": 0}, "offsets"), (("bgr24", 8, 8), {"offsets": (0, 0)}, "offsets"),
    (("nv12", 8, 8), {"offsets": (0,)}, "offsets"), (("i420", 8, 8), {"offsets": (0, 64)}, "offsets"),
    (("nv12", 8, 8), {"chroma_pitch": False}, "chroma_pitch"),
    (("bgr24", 8, 8), {"pitch": 23}, "pitch"), (("rgba32", 8, 8), {"pitch": 31}, "pitch"), (("yuyv422", 8, 8), {"pitch": 15}, "pitch"),
    (("nv12", 8, 8), {"pitch": 7}, "pitch"), (("nv12", 8, 8), {"chroma_pitch": 7}, "chroma_pitch"),
    (("i420", 8, 8), {"chroma_pitch": 3}, "chroma_pitch"), (("bgr24", 8, 8), {"pitch": -24}, "pitch"),
    (("i420", 8, 8), {"pitch": 9}, "pitch"),                                          # odd, and no chroma_pitch
    (("bgr24", 8, 8), {"chroma_pitch": 24}, "chroma_pitch"),
    (("bgr24", 8, 8), {"frame_stride": 191}, "frame_stride"), (("bgr24", 8, 8), {"offsets": (1,), "frame_stride": 192}, "offsets"),
    (("bgr24", 8, 8), {"offsets": (-1,)}, "offsets"), (("nv12", 8, 8), {"offsets": (0, 65), "frame_stride": 96}, "offsets"),
    (("bgr24", 8, 8), {"frame_stride": 0}, "frame_stride"),
    (("yuyv422", 8, 7), {}, "width"), (("uyvy422", 8, 1), {}, "width"), (("nv12", 8, 7), {}, "width"), (("i420", 7, 8), {}, "height"),
    (("bgr24", 1 << 15, (1 << 14) + 1), {}, "2\\^29"),
    (("bgr24", 8, 8), {"pitch": 1 << 40}, "pitch"), (("bgr24", 8, 8), {"frame_stride": 1 << 40}, "frame_stride"),
    (("bgr24", 8, 8), {"offsets": (1 << 40,)}, "offsets"), (("bgr24", 8, 8), {"frame_stride": 1 << 62}, "frame_stride"),
    (("bgr24", 1 << 20, 8), {"pitch": (1 << 40) - 1}, "frame_stride"),                # the default stride leaves 2^40
    (("bgr24", 8, 8), {"chroma": "vu"}, "chroma"), (("yuyv422", 8, 8), {"chroma": "vu"}, "chroma"), (("nv12", 8, 8), {"chroma": "VU"}, "chroma"),
]


@pytest.mark.parametrize("args,kw,match", REFUSED)
def test_surface_layout_refusals_name_the_argument(args, kw, match):
    with pytest.raises(ValueError, match=match):
        _frames().surface_layout(*args, **kw)


def test_layouts_need_no_alignment_and_planes_may_overlap():
    frames = _frames()
    lay = frames.surface_layout("i420", 8, 8, pitch=9, chroma_pitch=5, offsets=(3, 3, 3), frame_stride=77)
    assert lay.extent == 3 + 7 * 9 + 8 and lay.frame_stride == 77
    assert frames.surface_layout("bgr24", 8, 8, pitch=25, offsets=(1,), frame_stride=201).extent == 1 + 7 * 25 + 24
    sig = inspect.signature(frames.surface_layout).parameters
    assert list(sig) == ["pixel_format", "height", "width", "pitch", "chroma_pitch", "offsets", "frame_stride", "chroma"]
    assert all(sig[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig)[3:]) and sig["chroma"].default == "uv"


def test_of_view_reads_the_strides():
    frames = _frames()
    big = torch.zeros((3, 8 + 3, 6 + 5, 4), dtype=torch.uint8)
    view = big[:, 1:9, 2:8]
    lay = frames.SurfaceLayout.of_view(view, "bgra32")
    assert (lay.height, lay.width, lay.pitch, lay.frame_stride, lay.offsets) == (8, 6, 11 * 4, 11 * 11 * 4, (0,))
    assert lay.fits_view(view) and lay.fits_view(view[1:]) and lay.fits_view(view[2:]) and not lay.fits_view(view[:, :, 1:])
    assert frames.SurfaceLayout.of_view(big, "rgba32") == frames.surface_layout("rgba32", 11, 11)
    for bad in (big[..., :3], big[:, :, ::2], big.permute(0, 2, 1, 3), big[:, :, :, 1:].expand(3, 11, 11, 3)):
        with pytest.raises(ValueError, match="frames"):
            frames.SurfaceLayout.of_view(bad, "bgr24" if bad.shape[3] == 3 else "bgra32")
    with pytest.raises(ValueError, match="pixel_format"):
        frames.SurfaceLayout.of_view(torch.zeros((1, 6, 4), dtype=torch.uint8), "nv12")


# ---------------------------------------------------------------------------------------------- 3. names and shapes
def test_constructors_accept_the_new_names_and_keep_their_defaults():
    frames = _frames()
    from feature_vs_text_compound_emotion_amd import live
    assert frames.PIXEL_FORMATS[:3] == ("rgb24", "nv12", "i420") and set(frames.PIXEL_FORMATS[3:]) == set(NEW)
    for fmt in NEW:
        xf = frames.FrameTransform(48, 40, train=False, pixel_format=fmt, matrix="bt709", range="full")
        fs = frames.FrameStream(2, pixel_format=fmt)
        assert (xf.pixel_format, fs.pixel_format, xf.yuv, fs._xf.yuv) == (fmt, fmt, None, None)
    assert frames.FrameTransform().yuv is None and frames.FrameTransform(pixel_format="nv12").yuv.layout == 0
    for make in (lambda **kw: frames.FrameTransform(48, 40, train=False, **kw), lambda **kw: frames.FrameStream(2, **kw)):
        for name in ("nv21", "NV12", "bgr", "yuyv", "BGRA32"):
            with pytest.raises(ValueError, match="pixel_format"):
                make(pixel_format=name)
        with pytest.raises(ValueError, match="matrix"):
            make(pixel_format="yuyv422", matrix="bt2020")
    for cls, names in ((frames.FrameTransform, ("pixel_format", "matrix", "range")), (frames.FrameStream, ("pixel_format", "matrix", "range")),
                       (live.AVStream, ("video_format", "video_matrix", "video_range"))):
        sig = inspect.signature(cls.__init__).parameters
        assert [sig[n].default for n in names] == ["rgb24", "bt601", "limited"], cls


BAD_FRAMES = [
    ("bgr24", (2, 6, 8, 4), r"\[M, H, W, 3\]"), ("bgr24", (2, 6, 8), r"\[M, H, W, 3\]"), ("bgr24", (2, 0, 8, 3), "empty"),
    ("rgba32", (2, 6, 8, 3), r"\[M, H, W, 4\]"), ("bgra32", (2, 6, 8, 2), r"\[M, H, W, 4\]"), ("bgra32", (1, 2, 6, 8, 4), r"\[M, H, W, 4\]"),
    ("yuyv422", (2, 6, 8, 3), r"\[M, H, W, 2\]"), ("yuyv422", (2, 6, 7, 2), "even W"), ("uyvy422", (2, 9, 8), r"\[M, H, W, 2\]"),
    ("uyvy422", (2, 6, 1, 2), "even W"), ("uyvy422", (2, 6, 0, 2), "empty"),
    ("bgr24", (2, 6, 8, 3), "must be on the GPU"), ("yuyv422", (2, 5, 8, 2), "must be on the GPU"),      # good shapes: the device
]


@pytest.mark.parametrize("fmt,shape,match", BAD_FRAMES)
def test_frame_stream_refuses_bad_frames_of_the_new_formats_with_the_state_unchanged(fmt, shape, match):
    frames = _frames()
    fs = frames.FrameStream(2, hold=4, max_new=3, pixel_format=fmt)
    fs.frames_seen, fs.frames_taken = [3, 1], [2, 0]
    u8 = torch.zeros(shape, dtype=torch.uint8)
    aff = [[1.0, 0, 0, 0, 1.0, 0]] * 2
    for check, push, extra in ((fs.check_push, fs.push, ()), (fs.check_push, fs.push, ([[0, 0, 4, 4], [1, 1, 2, 2]],)),
                               (fs.check_push_aligned, fs.push_aligned, (aff,))):
        for call in (check, push):
            with pytest.raises(ValueError, match="frames: .*" + match):
                call(u8, [1, 1], *extra)
    with pytest.raises(ValueError, match="uint8 tensor"):
        fs.check_push(torch.zeros(shape), [1, 1])
    with pytest.raises(ValueError, match="boxes: .*empty"):           # the boxes are still looked at first
        fs.check_push(u8, [1, 1], [[0, 0, 4, 4], [5, 0, 5, 4]])
    assert fs.frames_seen == [3, 1] and fs.frames_taken == [2, 0] and fs.ring is None


@pytest.mark.parametrize("fmt,shape,match", [(f, (1,) + s if len(s) == 4 else s, m.replace("M, H", "B, L, H")) for f, s, m in BAD_FRAMES
                                             if s != (1, 2, 6, 8, 4)] + [("bgra32", (1, 1, 2, 6, 8, 4), r"\[B, L, H, W, 4\]")])
def test_frame_transform_refuses_bad_clips_of_the_new_formats(fmt, shape, match):
    xf = _frames().FrameTransform(48, 40, train=False, pixel_format=fmt)
    u8 = torch.zeros(shape, dtype=torch.uint8)
    with pytest.raises(ValueError, match=match):
        xf(u8)
    with pytest.raises(ValueError, match=match):
        xf(u8, boxes=[[0, 0, 4, 4]] * 2)
    with pytest.raises(ValueError, match=match):
        xf._clip(u8)


def test_layout_refusals_leave_the_state_unchanged():
    frames = _frames()
    lay = frames.surface_layout("bgr24", 6, 8, pitch=31)
    fs = frames.FrameStream(2, hold=4, max_new=3, pixel_format="bgr24")
    fs.frames_seen, fs.frames_taken = [3, 1], [2, 0]
    good = torch.zeros((2, 6, 31), dtype=torch.uint8)
    cases = [(good, frames.surface_layout("bgra32", 6, 8), "layout: .*pixel_format"), (good, "bgr24", "layout: .*SurfaceLayout"),
             (good[:, :5], lay, "frames: .*frame_stride = 186"), (good[:, :, :30], lay, "frames: .*frame_stride"),
             (good.to(torch.int16), lay, "frames: .*uint8"), (good, lay, "must be on the GPU")]
    for f, layout, match in cases:
        for call in (fs.check_push, fs.push):
            with pytest.raises(ValueError, match=match):
                call(f, [1, 1], layout=layout)
        with pytest.raises(ValueError, match=match):
            fs.push_aligned(f, [1, 1], [[1.0, 0, 0, 0, 1.0, 0]] * 2, layout=layout)
    assert fs.frames_seen == [3, 1] and fs.frames_taken == [2, 0] and fs.ring is None
    xf = frames.FrameTransform(48, 40, train=False, pixel_format="bgr24")
    for f, layout, match in cases:
        with pytest.raises(ValueError, match=match.replace("frames: ", "")):
            xf(f.unsqueeze(0), layout=layout)
    # the 4:2:0 formats take a layout too; without one they keep today's checks and words
    fs = frames.FrameStream(2, pixel_format="nv12")
    with pytest.raises(ValueError, match="must be on the GPU"):
        fs.check_push(torch.zeros((2, 9, 8), dtype=torch.uint8), [1, 1], layout=frames.surface_layout("nv12", 6, 8))
    with pytest.raises(ValueError, match=r"frames: .*\[M, H \* 3 / 2, W\]"):
        fs.check_push(torch.zeros((2, 6, 8, 3), dtype=torch.uint8), [1, 1])
    with pytest.raises(ValueError, match="layout without frames_u8"):
        fs.push(layout=frames.surface_layout("nv12", 6, 8))


def test_layout_is_a_keyword_of_every_call_that_takes_frames():
    frames = _frames()
    from feature_vs_text_compound_emotion_amd import live
    xf = frames.FrameTransform(48, 40, train=False, pixel_format="bgr24")
    fs = frames.FrameStream(1, pixel_format="bgr24")
    cpu, lay = torch.zeros((1, 6, 24), dtype=torch.uint8), frames.surface_layout("bgr24", 6, 8)
    aff = [[1.0, 0, 0, 0, 1.0, 0]]
    for call in (lambda: xf(cpu[None], layout=lay), lambda: xf.aligned(cpu[None], aff, layout=lay), lambda: fs.push(cpu, [1], layout=lay),
                 lambda: fs.push_aligned(cpu, [1], aff, layout=lay), lambda: fs.check_push(cpu, [1], layout=lay),
                 lambda: fs.check_push_aligned(cpu, [1], aff, layout=lay), lambda: fs.push(frames_u8=cpu, counts=[1], layout=lay)):
        with pytest.raises(ValueError, match="must be on the GPU"):       # the layout arrived: the good shape is what passed
            call()
    # the session's spelling reaches the same wrapper: without video it is refused by name, before anything else is looked at
    for f in (live.AVStream.push, live.AVStream.push_aligned):
        with pytest.raises(ValueError, match="video_layout without video"):
            f(object(), video_layout=lay)


# ---------------------------------------------------------------------------------------------- 4. the C entries
def _header():
    text = open(os.path.join(ROOT, "include", "cer_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_the_six_entries_are_declared_exported_and_bound():
    from feature_vs_text_compound_emotion_amd import _lib
    text = _header()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for sibling in SIBLINGS:
        name = sibling + "_surface"
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _lib.exported_symbols() and getattr(raw, name) is not None
        assert getattr(_lib.load(), name).argtypes == _lib._SIGNATURES[name][1]
        rgb = _lib._SIGNATURES[sibling][1]
        assert _lib._SIGNATURES[name][1] == [rgb[0], ctypes.c_size_t, ctypes.POINTER(_lib.SurfaceDesc)] + rgb[1:], name
        # and so says the header: the sibling's parameter list with the two after `frames`
        params = lambda n: re.sub(r"\s+", " ", re.search(r"\bint\s+" + n + r"\s*\(([^)]*)\)", text).group(1)).strip()      # noqa: E731
        assert params(name) == params(sibling).replace("const uint8_t *frames,", "const uint8_t *frames, size_t frames_bytes, "
                                                       "const cer_surface *surface,", 1), name
    for i, macro in enumerate(("CER_SURFACE_PACKED", "CER_SURFACE_YUV420", "CER_SURFACE_YUV422")):
        assert re.search(r"#define\s+" + macro + r"\s+" + str(i) + r"\b", text)
    assert (_lib.SURFACE_PACKED, _lib.SURFACE_YUV420, _lib.SURFACE_YUV422) == (0, 1, 2)
    # the struct of the header, field by field, under the C layout rules
    body = re.search(r"typedef struct cer_surface \{(.*?)\} cer_surface;", text, flags=re.S).group(1)
    fields = []
    for ctype, names in re.findall(r"(int32_t|int64_t)\s+([^;]+);", body):
        for n in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", n)
            base = ctypes.c_int32 if ctype == "int32_t" else ctypes.c_int64
            fields.append((m.group(1), base * int(m.group(2)) if m.group(2) else base))
    header_struct = type("HeaderSurface", (ctypes.Structure,), {"_fields_": fields})
    assert [f[0] for f in fields] == [f[0] for f in _lib.SurfaceDesc._fields_]
    assert ctypes.sizeof(_lib.SurfaceDesc) == ctypes.sizeof(header_struct) == 96
    for name, _ in fields:
        assert getattr(_lib.SurfaceDesc, name).offset == getattr(header_struct, name).offset, name
    # the existing entries and cer_yuv420 are what they were
    assert ctypes.sizeof(_lib.Yuv420Desc) == 28 and len(_lib._SIGNATURES["cer_frames_transform_yuv"][1]) == 21


def _desc(**kw):
    from feature_vs_text_compound_emotion_amd import _lib
    d = _lib.SurfaceDesc(0, *yuv_ref.COEFFICIENTS["bt601", "limited"])
    d.step[:], d.pos[:], d.frame_stride, d.pitch[:], d.offset[:] = (3, 3), (2, 1, 0), 192, (24, 24), (0, 0, 0)
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(d, k)[:] = v
        else:
            setattr(d, k, v)
    return d


def test_c_entries_refuse_the_descriptor_the_picture_and_the_extent_before_any_launch():
    from feature_vs_text_compound_emotion_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))      # never dereferenced: every case below is refused first

    def head(d, nbytes, n, h, w):
        return (p, nbytes, None if d is None else ctypes.byref(d), n, h, w)

    calls = {
        "frames_transform_surface": lambda *a: lib.cer_frames_transform_surface(*head(*a), p, p, 3, p, p, 3, 6, 4, p, 1, 2, 0.5, 0.5, p, None, None),
        "frames_stream_append_surface": lambda *a: lib.cer_frames_stream_append_surface(
            *head(*a), p, p, 3, p, p, 3, 6, 4, p, 2, p, p, 1, 1, p, 1, 8, None),
        "frames_transform_boxes_surface": lambda *a: lib.cer_frames_transform_boxes_surface(
            *head(*a), p, p, p, 16, 8, 7, 6, 4, p, 1, 0.5, 0.5, p, None, None),
        "frames_stream_append_boxes_surface": lambda *a: lib.cer_frames_stream_append_boxes_surface(
            *head(*a), p, p, p, 16, 8, 7, 6, 4, p, p, p, 1, 1, p, 1, 8, None),
        "frames_transform_affine_surface": lambda *a: lib.cer_frames_transform_affine_surface(
            *head(*a), p, p, p, 3, 8, 8, 6, 4, p, 1, 0.5, 0.5, p, None, None),
        "frames_stream_append_affine_surface": lambda *a: lib.cer_frames_stream_append_affine_surface(
            *head(*a), p, p, p, 3, 8, 8, 6, 4, p, p, p, 1, 1, p, 1, 8, None),
    }
    nv12 = dict(format=1, step=(1, 2), pos=(0, 0, 0), pitch=(8, 8), offset=(0, 64, 65), frame_stride=96)
    yuyv = dict(format=2, step=(2, 4), pos=(0, 1, 3), pitch=(16, 16), frame_stride=128)
    big = 1 << 62
    cases = [
        (None, 192, 1, 8, 8, b"null"), (_desc(format=3), 192, 1, 8, 8, b"format"), (_desc(format=-1), 192, 1, 8, 8, b"format"),
        (_desc(cgu=1 << 21), 192, 1, 8, 8, b"coefficient"), (_desc(cbu=-(1 << 21)), 192, 1, 8, 8, b"coefficient"),
        (_desc(yoff=256), 192, 1, 8, 8, b"yoff"), (_desc(yoff=-1), 192, 1, 8, 8, b"yoff"),
        (_desc(step=(5, 5)), 192, 1, 8, 8, b"byte pattern"), (_desc(pos=(3, 1, 0)), 192, 1, 8, 8, b"byte pattern"),
        (_desc(**{**yuyv, "pos": (2, 1, 3)}), 128, 1, 8, 8, b"byte pattern"), (_desc(**{**nv12, "step": (1, 3)}), 96, 1, 8, 8, b"byte pattern"),
        (_desc(**yuyv), 128, 1, 8, 7, b"even W"), (_desc(**nv12), 96, 1, 7, 8, b"even H and W"), (_desc(**nv12), 96, 1, 8, 9, b"even H and W"),
        (_desc(), 192, 1, 1 << 15, 1 << 15, b"2^29"),
        (_desc(offset=(-1, -1, -1)), 192, 1, 8, 8, b"negative"), (_desc(pitch=(-24, -24)), 192, 1, 8, 8, b"negative"),
        (_desc(frame_stride=-192), 192, 1, 8, 8, b"negative"),
        (_desc(pitch=(23, 23)), 192, 1, 8, 8, b"below"), (_desc(**{**nv12, "pitch": (8, 7)}), 96, 1, 8, 8, b"below"),
        (_desc(**{**yuyv, "pitch": (15, 15)}), 128, 1, 8, 8, b"below"),
        (_desc(frame_stride=191), 192, 1, 8, 8, b"past frame_stride"), (_desc(offset=(1, 1, 1)), 192, 1, 8, 8, b"past frame_stride"),
        (_desc(**{**nv12, "offset": (0, 64, 66)}), 96, 1, 8, 8, b"past frame_stride"),
        (_desc(), 191, 1, 8, 8, b"frames_bytes"), (_desc(), 192, 2, 8, 8, b"frames_bytes"), (_desc(), 383, 2, 8, 8, b"frames_bytes"),
        (_desc(**nv12), 95, 1, 8, 8, b"frames_bytes"), (_desc(), 0, 1, 8, 8, b"frames_bytes"),
        (_desc(frame_stride=big), 192, 1, 8, 8, b"2^40"), (_desc(frame_stride=big), 192, 5, 8, 8, b"2^40"),      # 4 * 2^62 wraps to 0
        (_desc(pitch=(big, big)), 192, 1, 8, 8, b"2^40"), (_desc(offset=(big, big, big)), 192, 1, 8, 8, b"2^40"),
        (_desc(frame_stride=1 << 40), 192, 1, 8, 8, b"2^40"),
        (_desc(frame_stride=(1 << 40) - 1), 192, 65535, 8, 8, b"frames_bytes"),
        (_desc(pitch=((1 << 40) - 1,) * 2, frame_stride=(1 << 40) - 1), 192, 1, 1 << 20, 8, b"past frame_stride"),
        (_desc(), 192, 0, 8, 8, b">= 1"), (_desc(), 192, 1, 0, 8, b">= 1"),
    ]
    for name, call in calls.items():
        for d, nbytes, n, h, w, text in cases:
            assert call(d, nbytes, n, h, w) != 0, (name, text)
            msg = lib.cer_last_error()
            assert msg.startswith(name.encode() + b":") and text in msg, (name, text, msg)
    # what the RGB sibling refuses is refused too: crop above size through the boxed pair, a ring length of 6
    assert lib.cer_frames_transform_boxes_surface(*head(_desc(), 192, 1, 8, 8), p, p, p, 16, 8, 7, 6, 7, p, 1, 0.5, 0.5, p, None, None) != 0
    assert lib.cer_last_error().startswith(b"frames_transform_boxes_surface:") and b"exceeds size" in lib.cer_last_error()
    assert lib.cer_frames_stream_append_surface(*head(_desc(), 192, 1, 8, 8), p, p, 3, p, p, 3, 6, 4, p, 2, p, p, 1, 1, p, 1, 6, None) != 0
    assert b"power of two" in lib.cer_last_error()
    assert lib.cer_frames_stream_append_affine_surface(*head(_desc(), 192, 1, 8, 8), p, p, p, 3, 8, 8, 6, 4, p, p, p, 1, 1, p, 1, 6, None) != 0
    assert lib.cer_last_error().startswith(b"frames_stream_append_affine_surface:") and b"power of two" in lib.cer_last_error()


def test_ops_wrappers_refuse_a_wrong_surface_on_the_host():
    from feature_vs_text_compound_emotion_amd import ops
    frames = _frames()
    like = torch.zeros(1)
    with pytest.raises(ValueError, match="surface: expected a frames.Surface"):
        ops._surface_frames(torch.zeros((1, 6, 24), dtype=torch.uint8), frames.surface_layout("bgr24", 6, 8), like)
    with pytest.raises(ValueError, match="frames: expected a uint8"):
        ops._surface_frames(torch.zeros((1, 6, 24), dtype=torch.uint8), frames.Surface(frames.surface_layout("bgr24", 6, 8)), like)
    with pytest.raises(ValueError, match="layout: expected a SurfaceLayout"):
        frames.Surface("bgr24")
    with pytest.raises(ValueError, match="exclude each other"):
        ops._yuv_entry("cer_frames_transform", frames.yuv_desc("nv12"), frames.Surface(frames.surface_layout("nv12", 6, 8)), 72)


# ---------------------------------------------------------------------------------------------- 5. the stand-alone program
def test_stand_alone_argument_checks_run_clean_under_the_host_sanitizers(tmp_path):
    """tools/frames_surface_args_check.cpp has its own ``main`` and calls the six entries with bad descriptors, pictures and
    extents, up to 2^62-scale values; compiled with the four frame translation units and the error recorder under
    AddressSanitizer and UndefinedBehaviorSanitizer on the host side only, and run here as a program of its own.  No GPU is
    touched: every call is refused first."""
    from feature_vs_text_compound_emotion_amd import build
    csrc = os.path.join(ROOT, "feature_vs_text_compound_emotion_amd", "csrc")
    exe = str(tmp_path / "frames_surface_args_check")
    cmd = [build.HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tools", "frames_surface_args_check.cpp"),
           *(os.path.join(csrc, f) for f in ("frames.hip", "frames_stream.hip", "frames_box.hip", "frames_affine.hip", "cer_common.hip")),
           "-o", exe]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and re.search(r"^ok: \d+ refusals$", run.stdout, flags=re.M), (run.stdout[-2000:], run.stderr[-2000:])
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-2000:]
