"""Surfaces in numpy: what the new pixel formats mean and where a layout puts a picture's bytes, restated from their
definitions and not from the kernel.

Tightly packed frames of an H x W picture:
  ``rgb24`` / ``bgr24`` [M, H, W, 3], ``rgba32`` / ``bgra32`` [M, H, W, 4] (the fourth byte means nothing);
  ``yuyv422`` / ``uyvy422`` [M, H, W, 2]: a row is ``Y0 U Y1 V ...`` / ``U Y0 V Y1 ...``; pixel (x, y) takes its own Y and the
  U and V of pair x >> 1 of its row;
  ``nv12`` / ``i420`` [M, H * 3 / 2, W] as in ``yuv_ref``.
A layout (any object with ``pixel_format, height, width, pitch, chroma_pitch, offsets, frame_stride``) puts row r of plane i at
byte ``offsets[i] + r * pitch_i`` of a frame of ``frame_stride`` bytes.
"""
import numpy as np

import yuv_ref

PACKED = {"rgb24": (3, (0, 1, 2)), "bgr24": (3, (2, 1, 0)), "rgba32": (4, (0, 1, 2)), "bgra32": (4, (2, 1, 0))}
YUV422 = {"yuyv422": (0, 1, 3), "uyvy422": (1, 0, 2)}      # byte of Y0, U, V in a pair of pixels
FORMATS = tuple(PACKED) + tuple(YUV422) + yuv_ref.LAYOUTS


def tight_shape(pixel_format, m, h, w):
    if pixel_format in yuv_ref.LAYOUTS:
        return (m, h * 3 // 2, w)
    return (m, h, w, 2 if pixel_format in YUV422 else PACKED[pixel_format][0])


def to_rgb(frames, pixel_format, matrix="bt601", range="limited"):
    """Tightly packed frames of ``pixel_format`` -> uint8 [M, H, W, 3] RGB."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.shape == tight_shape(pixel_format, frames.shape[0], *_picture(pixel_format, frames))
    if pixel_format in PACKED:
        return np.ascontiguousarray(frames[..., list(PACKED[pixel_format][1])])
    if pixel_format in YUV422:
        m, h, w, _ = frames.shape
        assert w % 2 == 0
        y0, u, v = YUV422[pixel_format]
        pairs = frames.reshape(m, h, w // 2, 4)
        y = np.stack([pairs[..., y0], pairs[..., y0 + 2]], axis=-1).reshape(m, h, w)
        return np.ascontiguousarray(yuv_ref.convert(y, np.repeat(pairs[..., u], 2, axis=2), np.repeat(pairs[..., v], 2, axis=2),
                                                    matrix, range))
    return yuv_ref.yuv_to_rgb(frames, pixel_format, matrix, range)


def _picture(pixel_format, frames):
    return (frames.shape[1] // 3 * 2, frames.shape[2]) if pixel_format in yuv_ref.LAYOUTS else frames.shape[1:3]


def _planes(layout):
    """(offset, pitch, rows, bytes of a row) per plane, in the order the tight frame holds them."""
    fmt, h, w = layout.pixel_format, layout.height, layout.width
    if fmt == "nv12":
        shapes = [(layout.pitch, h, w), (layout.chroma_pitch, h // 2, w)]
    elif fmt == "i420":
        shapes = [(layout.pitch, h, w), (layout.chroma_pitch, h // 2, w // 2), (layout.chroma_pitch, h // 2, w // 2)]
    else:
        shapes = [(layout.pitch, h, w * (2 if fmt in YUV422 else PACKED[fmt][0]))]
    assert len(shapes) == len(layout.offsets)
    return [(o, *s) for o, s in zip(layout.offsets, shapes)]


def embed(tight_frames, layout, fill):
    """Tightly packed frames -> uint8 [M, frame_stride]: the picture's rows where the layout puts them, every other byte from
    ``fill`` [>= M, frame_stride]."""
    tight = np.asarray(tight_frames)
    m = tight.shape[0]
    assert tight.shape == tight_shape(layout.pixel_format, m, layout.height, layout.width)
    out = np.array(np.asarray(fill)[:m], dtype=np.uint8, copy=True)
    assert out.shape == (m, layout.frame_stride)
    flat, at = tight.reshape(m, -1), 0
    for offset, pitch, rows, row in _planes(layout):
        for r in range(rows):
            out[:, offset + r * pitch:offset + r * pitch + row] = flat[:, at:at + row]
            at += row
    assert at == flat.shape[1]
    return out


def extract(surface_frames, layout):
    """The inverse of ``embed``: uint8 [M, frame_stride] -> tightly packed frames."""
    buf = np.asarray(surface_frames)
    m = buf.shape[0]
    buf = buf.reshape(m, layout.frame_stride)
    parts = [buf[:, offset + r * pitch:offset + r * pitch + row] for offset, pitch, rows, row in _planes(layout) for r in range(rows)]
    return np.ascontiguousarray(np.concatenate(parts, axis=1).reshape(tight_shape(layout.pixel_format, m, layout.height, layout.width)))


def swap_uv(tight_frames, pixel_format):
    """Tight ``nv12`` / ``i420`` frames with U and V exchanged (NV21 / YV12 bytes of the same picture, and back)."""
    y, u, v = yuv_ref.planes(tight_frames, pixel_format)
    return yuv_ref.pack(y, v, u, pixel_format)
