"""On-GPU video-frame input transform (the reference Dataset's ``get_3D_transforms``).

Mirrors /root/reference/base/dataset.py:487-508 + base/transforms3D.py: ``GroupScale(48)`` ->
``GroupRandomCrop(48, 40)`` / ``GroupCenterCrop(40)`` -> ``GroupRandomHorizontalFlip`` -> ``Stack`` ->
``ToTorchFormatTensor`` -> ``GroupNormalize(.5, .5)``, as ONE HIP kernel (csrc/frames.hip) over uint8
frames that are already resident in HBM.  The resize is bit-identical to ``PIL.Image.resize(BILINEAR)``
(what torchvision's Resize runs for a PIL image): the host computes Pillow's integer coefficient tables
(``precompute_coeffs`` + ``normalize_coeffs_8bpc`` of Pillow's Resample.c, third-party, restated) once per
geometry and the kernel does the two fixed-point passes.
"""
import dataclasses
import functools
import math
import random

import numpy as np
import torch

from . import _lib, ops

PRECISION_BITS = 32 - 8 - 2


def resample_tables(in_size, out_size):
    """Pillow's bilinear (triangle, support 1) tables: bounds int32 [out,2], coefficients int32 [out,ksize]."""
    scale = float(np.float32(in_size)) / out_size      # the box edges are C floats in Pillow
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    coef = np.zeros((out_size, ksize), np.int32)
    inv = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        cnt = min(int(center + support + 0.5), in_size) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * inv)) for x in range(cnt)]
        total = 0.0
        for v in w:
            total += v
        for x in range(cnt):
            v = (w[x] / total if total != 0.0 else w[x]) * (1 << PRECISION_BITS)
            coef[xx, x] = int(v - 0.5) if v < 0 else int(v + 0.5)
        bounds[xx] = (xmin, cnt)
    return bounds, coef


def _resample_tables_np(in_size, out_size):
    """``resample_tables`` with the taps of every output computed at once: the same float64 operations in the same order
    (the running sum is ``np.add.accumulate``, left to right), so the same integers.  tests/test_frames_boxes_cpu.py holds the
    two equal for every side the table store can hold."""
    scale = float(np.float32(in_size)) / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    inv = 1.0 / filterscale
    center = ((np.arange(out_size, dtype=np.float64) + 0.5) * scale)[:, None]
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)
    cnt = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    live = x < cnt
    w = np.where(live, np.maximum(0.0, 1.0 - np.abs(((x + xmin) - center + 0.5) * inv)), 0.0)
    total = np.add.accumulate(w, axis=1)[:, -1:]
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where(total != 0.0, w / total, w) * (1 << PRECISION_BITS)
    coef = np.where(live, np.where(v < 0, v - 0.5, v + 0.5).astype(np.int64), 0).astype(np.int32)
    return np.concatenate([xmin, cnt], axis=1).astype(np.int32), coef


BOX_MAX_SIDE = 1024     # default of ``max_side``: the largest box side the table store holds
BOX_COORD = 1 << 20     # |box coordinate| bound of csrc/frames_box.hip (FB_COORD)


class BoxTables:
    """The table store of the boxed entries (csrc/frames_box.hip): Pillow's bounds and coefficients of EVERY side
    n = 1 .. ``max_side`` resampled to ``size``, concatenated in one int32 array ``data``, and ``meta`` [max_side + 1, 4] =
    (offset of the bounds, offset of the coefficients, ksize, band span) of side n.  The band span is the most box rows one
    band of ``cer_frames_band_rows()`` output rows needs, over every crop offset; ``max_rows`` and ``max_ks`` are the largest
    span and ksize of the store and size the kernel's LDS.  Built on the host once per (size, max_side) by ``box_tables``,
    uploaded once per device."""

    def __init__(self, size, max_side):
        band = _lib.load().cer_frames_band_rows()
        self.size, self.max_side = int(size), int(max_side)
        meta = np.zeros((self.max_side + 1, 4), np.int64)
        parts, at = [], 0
        y0 = np.arange(self.size)
        y1 = np.minimum(self.size, y0 + band) - 1
        for n in range(1, self.max_side + 1):
            b, k = _resample_tables_np(n, self.size)
            span = int((b[y1, 0] + b[y1, 1] - b[y0, 0]).max())
            meta[n] = (at, at + b.size, k.shape[1], span)
            parts += [b.ravel(), k.ravel()]
            at += b.size + k.size
        if at >= 1 << 31:
            raise ValueError(f"the table store of size {size}, max_side {max_side} exceeds int32 offsets")
        meta[0] = meta[1]
        self.meta, self.data = meta.astype(np.int32), np.concatenate(parts)
        self.max_rows, self.max_ks = int(meta[1:, 3].max()), int(meta[1:, 2].max())
        self._dev = {}

    def rows(self, n):
        """(bounds [size, 2], coefficients [size, ksize]) of side n, as ``resample_tables(n, size)`` gives them."""
        b, k, ks, _ = (int(v) for v in self.meta[n])
        return self.data[b:b + 2 * self.size].reshape(self.size, 2), self.data[k:k + self.size * ks].reshape(self.size, ks)

    def on(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.meta).to(device), torch.from_numpy(self.data).to(device))
        return self._dev[key]

    stem = "boxes"      # of the C entries cer_frames_transform_boxes / cer_frames_stream_append_boxes

    def check_rows(self, boxes, rows, size, crop, like):
        """What the entries ask of the device table, int32 [rows, 4] on the GPU of ``like``, and of the store."""
        if self.size != int(size):
            raise ValueError(f"store: built for size {self.size}, not {size}")
        ops._i32_table(boxes, "boxes", (rows, 4), like)

    def entry_args(self, device):
        """The two device tables and three integers the entries take after the boxes."""
        return (*self.on(device), self.max_side, self.max_rows, self.max_ks)


_BOX_TABLES = {}


def box_tables(size, max_side=BOX_MAX_SIDE):
    """The ``BoxTables`` of (size, max_side), built by the first call that asks for it."""
    key = (int(size), int(max_side))
    if key not in _BOX_TABLES:
        _BOX_TABLES[key] = BoxTables(*key)
    return _BOX_TABLES[key]


def check_boxes(boxes, rows, max_side):
    """Everything the boxed calls refuse about ``boxes``, on the host: -> int32 numpy [rows, 4] = (x0, y0, x1, y1), PIL's
    (left, upper, right, lower).  Boxes are host integers like ``counts``: checking a GPU tensor would cost a
    synchronisation, so one is refused."""
    if torch.is_tensor(boxes):
        if boxes.is_cuda:
            raise ValueError("boxes: expected host integers (a list, a numpy array or a CPU tensor), got a GPU tensor")
        if boxes.is_floating_point() or boxes.is_complex() or boxes.dtype == torch.bool:
            raise ValueError(f"boxes: expected integers, got dtype {boxes.dtype}")
        arr = boxes.numpy()
    else:
        arr = np.asarray(boxes)
    if arr.size == 0 and rows == 0:
        return np.zeros((0, 4), np.int32)
    if arr.dtype.kind not in "iu":
        raise ValueError(f"boxes: expected integers, got dtype {arr.dtype}")
    if arr.ndim == 3:
        arr = arr.reshape(-1, arr.shape[2])
    if arr.shape != (rows, 4):
        raise ValueError(f"boxes: expected one (x0, y0, x1, y1) per frame [{rows}, 4], got {arr.shape}")
    arr = arr.astype(np.int64)
    w, h = arr[:, 2] - arr[:, 0], arr[:, 3] - arr[:, 1]
    if (w < 1).any() or (h < 1).any():
        i = int(np.nonzero((w < 1) | (h < 1))[0][0])
        raise ValueError(f"boxes: box {i} = {arr[i].tolist()} is empty (x1 <= x0 or y1 <= y0)")
    if (w > max_side).any() or (h > max_side).any():
        i = int(np.nonzero((w > max_side) | (h > max_side))[0][0])
        raise ValueError(f"boxes: box {i} = {arr[i].tolist()} has a side above max_side = {max_side}")
    if (np.abs(arr) > BOX_COORD).any():
        raise ValueError(f"boxes: a coordinate lies beyond +-{BOX_COORD}")
    return arr.astype(np.int32)


ALIGN_SIZE = 256        # default of ``align_size``: the side of the reference's aligned faces
ARCFACE_TEMPLATE = ((38.2946, 51.6963), (73.5318, 51.5014), (56.0252, 71.7366), (41.5493, 92.3655), (70.7299, 92.2041))
"""The ArcFace five-point template on a 112 x 112 face (left eye, right eye, nose, left mouth, right mouth), (x, y)."""


class AffineGeometry:
    """What the affine entries (csrc/frames_affine.hip) need of (align_size, size): Pillow's bounds and coefficients of
    ``resample_tables(align_size, size)`` -- one table for both passes, the aligned face is square -- their tap count ``ks``
    and ``span``, the most rows of the face one band of ``cer_frames_band_rows()`` output rows needs over every crop offset.
    Built on the host once per (align_size, size) by ``affine_geometry``, uploaded once per device."""

    def __init__(self, align_size, size):
        self.align_size, self.size = int(align_size), int(size)
        self.bounds, self.coef = resample_tables(self.align_size, self.size)
        self.ks = int(self.coef.shape[1])
        band = _lib.load().cer_frames_band_rows()
        y0 = np.arange(self.size)
        y1 = np.minimum(self.size, y0 + band) - 1
        self.span = int((self.bounds[y1, 0] + self.bounds[y1, 1] - self.bounds[y0, 0]).max())
        self._dev = {}

    def lds_bytes(self, crop):
        return int(_lib.load().cer_frames_affine_lds_bytes(self.align_size, self.span, self.ks, int(crop)))

    def check_crop(self, crop):
        """Refuse, by name, an ``align_size`` whose warped band and coefficient rows exceed the kernel's LDS."""
        need = self.lds_bytes(crop)
        if need > AFFINE_LDS_BYTES:
            raise ValueError(f"align_size = {self.align_size}: the warped band of {self.span} rows and {self.ks}-tap coefficient rows "
                             f"at size {self.size}, crop {crop} need {need} bytes of the {AFFINE_LDS_BYTES // 1024} KiB LDS")

    def on(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.bounds).to(device), torch.from_numpy(self.coef).to(device))
        return self._dev[key]

    stem = "affine"     # of the C entries cer_frames_transform_affine / cer_frames_stream_append_affine

    def check_rows(self, affines, rows, size, crop, like):
        """What the entries ask of the device table, 8-byte aligned float64 [rows, 6] on the GPU of ``like``, and of the
        geometry."""
        if self.size != int(size):
            raise ValueError(f"geom: built for size {self.size}, not {size}")
        if not (torch.is_tensor(affines) and affines.is_cuda and affines.device == like.device and affines.dtype == torch.float64
                and affines.is_contiguous() and tuple(affines.shape) == (rows, 6) and affines.data_ptr() % 8 == 0):
            raise ValueError(f"affines: expected a contiguous, 8-byte aligned float64 [{rows}, 6] tensor on the GPU ({like.device}), got "
                             f"{(affines.dtype, affines.device, tuple(affines.shape)) if torch.is_tensor(affines) else type(affines)}")
        self.check_crop(crop)

    def entry_args(self, device):
        """The two device tables and three integers the entries take after the affines."""
        return (*self.on(device), self.ks, self.align_size, self.span)


AFFINE_LDS_BYTES = 160 * 1024     # what one block of csrc/frames_affine.hip may hold
AFFINE_MAX_ALIGN = 1 << 14        # FA_MAX_ALIGN
_AFFINE_GEOMETRY = {}


def check_align_size(align_size):
    if isinstance(align_size, bool) or not isinstance(align_size, (int, np.integer)) or not 1 <= align_size <= AFFINE_MAX_ALIGN:
        raise ValueError(f"align_size = {align_size!r}: must be an integer in 1 .. {AFFINE_MAX_ALIGN}")
    return int(align_size)


def affine_geometry(align_size, size):
    """The ``AffineGeometry`` of (align_size, size), built by the first call that asks for it."""
    key = (check_align_size(align_size), int(size))
    if key not in _AFFINE_GEOMETRY:
        _AFFINE_GEOMETRY[key] = AffineGeometry(*key)
    return _AFFINE_GEOMETRY[key]


def check_affines(affines, rows):
    """Everything the aligned calls refuse about ``affines``, on the host: -> float64 numpy [rows, 6], Pillow's
    ``Image.transform(..., AFFINE, data)`` coefficients per frame, all finite.  Affines are host numbers like ``counts``:
    checking a GPU tensor would cost a synchronisation, so one is refused."""
    if torch.is_tensor(affines):
        if affines.is_cuda:
            raise ValueError("affines: expected host numbers (a list, a numpy array or a CPU tensor), got a GPU tensor")
        if affines.is_complex() or affines.dtype == torch.bool:
            raise ValueError(f"affines: expected real numbers, got dtype {affines.dtype}")
        arr = affines.numpy()
    else:
        try:
            arr = np.asarray(affines)
        except ValueError:
            raise ValueError("affines: expected six coefficients per frame, got a ragged sequence") from None
    if arr.size == 0 and rows == 0:
        return np.zeros((0, 6), np.float64)
    if arr.dtype.kind not in "iuf":
        raise ValueError(f"affines: expected real numbers, got dtype {arr.dtype}")
    if arr.ndim == 3:
        arr = arr.reshape(-1, arr.shape[2])
    if arr.shape != (rows, 6):
        raise ValueError(f"affines: expected six coefficients (a0 .. a5) per frame [{rows}, 6], got {arr.shape}")
    arr = np.ascontiguousarray(arr, dtype=np.float64)
    if not np.isfinite(arr).all():
        i = int(np.nonzero(~np.isfinite(arr).all(axis=1))[0][0])
        raise ValueError(f"affines: affine {i} = {arr[i].tolist()} is not finite")
    return arr


def similarity_from_landmarks(landmarks, align_size=ALIGN_SIZE):
    """Five landmarks per face -> the Pillow coefficients that align it: float64 numpy [M, 6] for ``aligned`` /
    ``push_aligned``.  ``landmarks`` [M, 5, 2] (or [5, 2]) host numbers, (x, y) pixel coordinates of left eye, right eye,
    nose, left mouth corner, right mouth corner, as a face detector returns them.

    The non-reflective similarity u = a x - b y + tx, v = b x + a y + ty that takes the landmarks to
    ``ARCFACE_TEMPLATE * align_size / 112`` in the least-squares sense is fitted in closed form in float64 (the direction the
    reference's aligners fit), inverted, and converted from a map between integer pixel centres to Pillow's half-pixel
    convention: Pillow samples output pixel (x, y) at A (x + 0.5, y + 0.5) + (a2, a5) and reads pixel centres at +0.5, so
    a2 = t_x - 0.5 (a0 + a1) + 0.5 and a5 likewise.  Landmarks that all coincide have no fit and raise ValueError."""
    align_size = check_align_size(align_size)
    p = np.asarray(landmarks, dtype=np.float64)
    if p.ndim == 2:
        p = p[None]
    if p.ndim != 3 or p.shape[1:] != (5, 2):
        raise ValueError(f"landmarks: expected five (x, y) points per face [M, 5, 2], got {p.shape}")
    if not np.isfinite(p).all():
        raise ValueError("landmarks: a coordinate is not finite")
    q = np.asarray(ARCFACE_TEMPLATE, dtype=np.float64) * align_size / 112.0
    pm, qm = p.mean(axis=1, keepdims=True), q.mean(axis=0, keepdims=True)
    pc, qc = p - pm, (q - qm)[None]
    den = (pc * pc).sum(axis=(1, 2))
    if (den == 0).any():
        raise ValueError(f"landmarks: the five points of face {int(np.nonzero(den == 0)[0][0])} coincide; no similarity fits them")
    a = (pc * qc).sum(axis=(1, 2)) / den
    b = (pc[:, :, 0] * qc[:, :, 1] - pc[:, :, 1] * qc[:, :, 0]).sum(axis=1) / den
    if ((a * a + b * b) == 0).any():
        raise ValueError("landmarks: the fitted similarity has scale 0 and cannot be inverted")
    tx = qm[0, 0] - (a * pm[:, 0, 0] - b * pm[:, 0, 1])
    ty = qm[0, 1] - (b * pm[:, 0, 0] + a * pm[:, 0, 1])
    # the inverse x = (a u + b v - (a tx + b ty)) / s, y = (-b u + a v - (-b tx + a ty)) / s, s = a^2 + b^2
    s = a * a + b * b
    ia, ib = a / s, b / s
    out = np.empty((p.shape[0], 6), np.float64)
    out[:, 0], out[:, 1], out[:, 3], out[:, 4] = ia, ib, -ib, ia
    itx, ity = -(ia * tx + ib * ty), -(-ib * tx + ia * ty)
    out[:, 2] = itx - 0.5 * (out[:, 0] + out[:, 1]) + 0.5
    out[:, 5] = ity - 0.5 * (out[:, 3] + out[:, 4]) + 0.5
    return out


PIXEL_FORMATS = ("rgb24", "nv12", "i420", "bgr24", "rgba32", "bgra32", "yuyv422", "uyvy422")
PACKED_FORMATS = {"rgb24": (3, (0, 1, 2)), "bgr24": (3, (2, 1, 0)), "rgba32": (4, (0, 1, 2)), "bgra32": (4, (2, 1, 0))}
"""Bytes per pixel and the byte of R, G, B inside one; a fourth byte is never read."""
YUV422_FORMATS = {"yuyv422": (0, 1, 3), "uyvy422": (1, 0, 2)}
"""The byte of Y0, U, V inside the four bytes of a pixel pair; Y1 is two after Y0."""
SURFACE_MAX = 1 << 40       # every offset, pitch and stride of a layout is below this (csrc/frames_kernel.h)
SURFACE_MAX_PIXELS = 1 << 29
YUV_MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}                    # (kr, kb)
YUV_RANGES = {"limited": (255.0 / 219.0, 255.0 / 224.0, 16), "full": (1.0, 1.0, 0)}      # (luma scale, chroma scale, yoff)


def yuv_coefficients(matrix="bt601", range="limited"):
    """(cy, crv, cgu, cgv, cbu, yoff) of the 4:2:0 pixel formats: the YCbCr -> RGB matrix of (kr, kb) and the range's scales
    in Python floats, each entry rounded to 2^14 fixed point.  With c = Y - yoff, u = U - 128, v = V - 128 and int32
    arithmetic, R = clip8((cy c + crv v + 2^13) >> 14), G = clip8((cy c + cgu u + cgv v + 2^13) >> 14),
    B = clip8((cy c + cbu u + 2^13) >> 14); every sum stays below 9.3e6 in magnitude."""
    if matrix not in YUV_MATRICES:
        raise ValueError(f"matrix = {matrix!r}: expected one of {sorted(YUV_MATRICES)}")
    if range not in YUV_RANGES:
        raise ValueError(f"range = {range!r}: expected one of {sorted(YUV_RANGES)}")
    (kr, kb), (ys, cs, yoff) = YUV_MATRICES[matrix], YUV_RANGES[range]
    kg = 1 - kr - kb
    floats = (ys, 2 * (1 - kr) * cs, -2 * (1 - kb) * kb / kg * cs, -2 * (1 - kr) * kr / kg * cs, 2 * (1 - kb) * cs)
    return tuple(round(x * 2 ** _lib.YUV_PREC) for x in floats) + (yoff,)


def yuv_desc(pixel_format="rgb24", matrix="bt601", range="limited"):
    """What a stream or transform keeps of its pixel format for the 4:2:0 entries: the ``cer_yuv420`` for ``nv12`` / ``i420``,
    None for ``rgb24`` (and for the formats that only the surface entries read).  Unknown names raise ValueError, whatever
    the format."""
    if pixel_format not in PIXEL_FORMATS:
        raise ValueError(f"pixel_format = {pixel_format!r}: expected one of {list(PIXEL_FORMATS)}")
    coef = yuv_coefficients(matrix, range)
    if pixel_format not in ("nv12", "i420"):
        return None
    return _lib.Yuv420Desc(_lib.YUV_NV12 if pixel_format == "nv12" else _lib.YUV_I420, *coef)


def _layout_int(name, v, least=0):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{name} = {v!r}: must be an integer")
    if not least <= v < SURFACE_MAX:
        raise ValueError(f"{name} = {v}: must be in {least} .. 2^40 - 1")
    return int(v)


@dataclasses.dataclass(frozen=True)
class SurfaceLayout:
    """Where the bytes of an H x W picture lie in a frame of ``frame_stride`` bytes: host ints only, checked when built
    (``surface_layout`` is the spelling with keywords).  ``offsets`` are (plane 0,) for the packed formats, (Y, chroma) for
    ``nv12`` and (Y, first chroma plane, second chroma plane) for ``i420``; ``chroma`` says whether U (``"uv"``) or V
    (``"vu"``: NV21, YV12) is the first chroma byte or plane.  Nothing has to be aligned and planes may overlap."""
    pixel_format: str
    height: int
    width: int
    pitch: int = None
    chroma_pitch: int = None
    offsets: tuple = None
    frame_stride: int = None
    chroma: str = "uv"

    def __post_init__(self):
        fmt, put = self.pixel_format, lambda k, v: object.__setattr__(self, k, v)      # noqa: E731
        if fmt not in PIXEL_FORMATS:
            raise ValueError(f"pixel_format = {fmt!r}: expected one of {list(PIXEL_FORMATS)}")
        h, w = _layout_int("height", self.height, 1), _layout_int("width", self.width, 1)
        put("height", h), put("width", w)
        planar = fmt in ("nv12", "i420")
        if w % 2 and (planar or fmt in YUV422_FORMATS):
            raise ValueError(f"width = {w}: a {fmt} picture needs an even width")
        if h % 2 and planar:
            raise ValueError(f"height = {h}: a {fmt} picture needs an even height")
        if h * w > SURFACE_MAX_PIXELS:
            raise ValueError(f"height = {h}, width = {w}: more than 2^29 pixels")
        if self.chroma not in ("uv", "vu"):
            raise ValueError(f"chroma = {self.chroma!r}: expected 'uv' or 'vu'")
        if self.chroma == "vu" and not planar:
            raise ValueError(f"chroma = 'vu': only nv12 and i420 have a chroma order to exchange, not {fmt}")
        row = w * (1 if planar else 2 if fmt in YUV422_FORMATS else PACKED_FORMATS[fmt][0])
        pitch = row if self.pitch is None else _layout_int("pitch", self.pitch)
        if pitch < row:
            raise ValueError(f"pitch = {pitch}: below the {row} bytes of a row")
        put("pitch", pitch)
        if not planar:
            if self.chroma_pitch is not None:
                raise ValueError(f"chroma_pitch = {self.chroma_pitch!r}: {fmt} has no chroma plane")
            plane_rows = [(h, pitch, row)]
        else:
            crow = w if fmt == "nv12" else w // 2
            if self.chroma_pitch is None:
                if fmt == "i420" and pitch % 2:
                    raise ValueError(f"pitch = {pitch}: odd, so i420 needs a chroma_pitch of its own")
                cpitch = pitch if fmt == "nv12" else pitch // 2
            else:
                cpitch = _layout_int("chroma_pitch", self.chroma_pitch)
            if cpitch < crow:
                raise ValueError(f"chroma_pitch = {cpitch}: below the {crow} bytes of a chroma row")
            put("chroma_pitch", cpitch)
            plane_rows = [(h, pitch, row)] + [(h // 2, cpitch, crow)] * (1 if fmt == "nv12" else 2)
        if self.offsets is None:
            offsets, at = [], 0
            for rows, p, _ in plane_rows:
                offsets.append(at)
                at += rows * p
        else:
            try:
                offsets = list(self.offsets)
            except TypeError:
                raise ValueError(f"offsets = {self.offsets!r}: expected {len(plane_rows)} byte offsets") from None
            if len(offsets) != len(plane_rows):
                raise ValueError(f"offsets = {self.offsets!r}: {fmt} has {len(plane_rows)} plane offsets")
        offsets = tuple(_layout_int(f"offsets[{i}]", v) for i, v in enumerate(offsets))
        put("offsets", offsets)
        ends = [o + rows * p for o, (rows, p, _) in zip(offsets, plane_rows)]
        stride = max(ends) if self.frame_stride is None else _layout_int("frame_stride", self.frame_stride, 1)
        _layout_int("frame_stride", stride, 1)
        put("frame_stride", stride)
        for i, (o, (rows, p, used)) in enumerate(zip(offsets, plane_rows)):
            if o + (rows - 1) * p + used > stride:
                raise ValueError(f"offsets[{i}] = {o}: the plane's last row ends at {o + (rows - 1) * p + used}, past frame_stride = "
                                 f"{stride}")

    def planes(self):
        """(offset, pitch, rows, bytes of a row) of every plane, in the order of ``offsets``."""
        fmt, h, w = self.pixel_format, self.height, self.width
        if fmt == "nv12":
            shapes = [(h, self.pitch, w), (h // 2, self.chroma_pitch, w)]
        elif fmt == "i420":
            shapes = [(h, self.pitch, w)] + [(h // 2, self.chroma_pitch, w // 2)] * 2
        else:
            shapes = [(h, self.pitch, w * (2 if fmt in YUV422_FORMATS else PACKED_FORMATS[fmt][0]))]
        return [(o, p, rows, row) for o, (rows, p, row) in zip(self.offsets, shapes)]

    @property
    def extent(self):
        """Bytes of a frame up to the end of the last row that is read."""
        return max(o + (rows - 1) * p + row for o, p, rows, row in self.planes())

    @classmethod
    def of_view(cls, frames, pixel_format):
        """The layout of a packed-format tensor [M, H, W, C] as its strides give it: the last two are (C, 1), the row stride is
        the pitch, the frame stride the stride.  Any other stride pattern raises ValueError (such a view is copied)."""
        chan = 2 if pixel_format in YUV422_FORMATS else PACKED_FORMATS.get(pixel_format, (None,))[0]
        if chan is None:
            raise ValueError(f"pixel_format = {pixel_format!r}: only the packed formats have a layout in their strides")
        if not (torch.is_tensor(frames) and frames.dim() == 4 and frames.shape[3] == chan and min(frames.shape) >= 1):
            raise ValueError(f"frames: expected a {pixel_format} tensor [M >= 1, H, W, {chan}], got "
                             f"{tuple(frames.shape) if torch.is_tensor(frames) else type(frames)}")
        return _layout_of_strides(pixel_format, chan, tuple(frames.shape), tuple(frames.stride()))

    def fits_view(self, frames):
        """Whether the strides of ``frames`` [M, H, W, C] are this layout (``of_view`` of it, or of frames sliced off it)."""
        try:
            got = SurfaceLayout.of_view(frames, self.pixel_format)
        except ValueError:
            return False
        return (self.offsets == (0,) and (got.height, got.width) == (self.height, self.width) and
                (got.height == 1 or got.pitch == self.pitch) and (frames.shape[0] == 1 or got.frame_stride == self.frame_stride))


@functools.lru_cache(maxsize=256)
def _layout_of_strides(pixel_format, chan, shape, strides):
    """``SurfaceLayout.of_view`` on host ints; kept per (format, shape, strides), so a stream of equal frames builds one."""
    (m, h, w, _), (sm, sh, sw, sc) = shape, strides
    if (sw, sc) != (chan, 1) or (h > 1 and sh < w * chan) or (m > 1 and sm <= 0):
        raise ValueError(f"frames: strides {strides} are not rows of {chan}-byte pixels")
    pitch = sh if h > 1 else w * chan
    extent = (h - 1) * pitch + w * chan
    return SurfaceLayout(pixel_format, h, w, pitch=pitch, frame_stride=sm if m > 1 else max(sm, extent))


def surface_layout(pixel_format, height, width, *, pitch=None, chroma_pitch=None, offsets=None, frame_stride=None, chroma="uv"):
    """The ``SurfaceLayout`` of an H x W picture.  ``pitch``: bytes from one row of plane 0 to the next (default: tight);
    ``chroma_pitch``: of the chroma planes (default ``pitch`` for nv12, ``pitch / 2`` for i420); ``offsets``: of every plane
    inside a frame (default: tight after the pitches); ``frame_stride``: bytes from frame m to frame m + 1 (default: the end
    of the last plane); ``chroma="vu"``: the V byte or plane comes first (NV21, YV12).  Refusals are ValueErrors that name
    the argument."""
    return SurfaceLayout(pixel_format, height, width, pitch, chroma_pitch, offsets, frame_stride, chroma)


class Surface:
    """What the ``surface=`` of the frame wrappers in ``ops`` is: a ``SurfaceLayout`` and the (cy, crv, cgu, cgv, cbu, yoff)
    of ``yuv_coefficients``; ``desc()`` is the ``cer_surface`` of the C entries."""

    def __init__(self, layout, coef=None):
        if not isinstance(layout, SurfaceLayout):
            raise ValueError(f"layout: expected a SurfaceLayout (frames.surface_layout), got {type(layout).__name__}")
        self.layout, self.coef, self._desc = layout, tuple(yuv_coefficients() if coef is None else coef), None

    def desc(self):
        """The ``cer_surface``, built once: the entries only read it."""
        if self._desc is None:
            self._desc = self._build()
        return self._desc

    def _build(self):
        lay, fmt = self.layout, self.layout.pixel_format
        d = _lib.SurfaceDesc(0, *self.coef)
        d.frame_stride = lay.frame_stride
        if fmt in ("nv12", "i420"):
            d.format, first = _lib.SURFACE_YUV420, 0 if lay.chroma == "uv" else 1
            if fmt == "nv12":
                y, c = lay.offsets
                step, offset = (1, 2), (y, c + first, c + 1 - first)
            else:
                y, c1, c2 = lay.offsets
                step, offset = (1, 1), (y, (c1, c2)[first], (c1, c2)[1 - first])
            pos, pitch = (0, 0, 0), (lay.pitch, lay.chroma_pitch)
        else:
            if fmt in YUV422_FORMATS:
                d.format, step, pos = _lib.SURFACE_YUV422, (2, 4), YUV422_FORMATS[fmt]
            else:
                d.format, step, pos = _lib.SURFACE_PACKED, (PACKED_FORMATS[fmt][0],) * 2, PACKED_FORMATS[fmt][1]
            pitch, offset = (lay.pitch,) * 2, lay.offsets * 3
        d.step[:], d.pos[:], d.pitch[:], d.offset[:] = step, pos, pitch, offset
        return d


class _Laid:
    """Frames and the ``layout=`` they came with, as one argument."""
    __slots__ = ("frames", "layout")

    def __init__(self, frames, layout):
        self.frames, self.layout = frames, layout


def _unlaid(frames):
    return (frames.frames, frames.layout) if isinstance(frames, _Laid) else (frames, None)


def takes_layout(arg, key="layout"):
    """Gives a method that takes frames as ``arg`` the keyword ``key``: the ``SurfaceLayout`` of those frames, which then
    travel with it as one argument down to the check that looks at frames (``FrameTransform._source``).  One spelling of the
    keyword for every call that takes frames; the methods' own signatures stay what they were."""
    def wrap(method):
        @functools.wraps(method)
        def call(self, *args, **kw):
            layout = kw.pop(key, None)
            if layout is not None:
                if args:
                    args = (_Laid(args[0], layout),) + args[1:]
                elif kw.get(arg) is not None:
                    kw[arg] = _Laid(kw[arg], layout)
                else:
                    raise ValueError(f"{key} without {arg}")
            return method(self, *args, **kw)
        return call
    return wrap


def yuv_picture(rows, width):
    """(H, W) of the picture a 4:2:0 frame of ``rows`` rows of ``width`` bytes holds: rows = H * 3 / 2, H and W even (an odd
    H has no whole number of rows, so it shows as a row count that 3 does not divide)."""
    rows, width = int(rows), int(width)
    if rows < 3 or rows % 3:
        raise ValueError(f"frames: {rows} rows are not H * 3 / 2 of a 4:2:0 picture with even H (the Y plane, then half as many "
                         "chroma rows)")
    if width < 2 or width % 2:
        raise ValueError(f"frames: a 4:2:0 picture needs an even W, got {width}")
    return rows // 3 * 2, width


class FrameTransform:
    """``FrameTransform(size=48, crop=40, train=True)(frames_u8[B,L,H,W,3]) -> float32 [B,L,3,crop,crop]``.

    train=True draws one (x1, y1) crop offset and one flip per clip with Python's ``random`` in the
    reference's call order (transforms3D.py:52-53,80); train=False uses GroupCenterCrop's offset.

    ``boxes`` [B, L, 4] or [B * L, 4] host integers: the frames are full camera frames and frame f is first cropped to its
    box (x0, y0, x1, y1) as ``PIL.Image.crop`` does -- right and lower exclusive, zero outside the frame -- so the result is
    what the unboxed call gives the contiguous zero-padded slice; a box equal to the whole frame gives the unboxed bits.
    One launch for any mix of boxes (csrc/frames_box.hip); sides up to ``max_side``.

    ``pixel_format``: ``"rgb24"`` (packed RGB, above) or the 8-bit 4:2:0 a decoder hands out, converted where the kernel
    reads a pixel.  A frame of an H x W picture, H and W even, is then H * 3 / 2 rows of W bytes, uint8 [B, L, H * 3 / 2, W]:
    the Y plane [H][W], then for ``"nv12"`` the interleaved chroma [H / 2][W / 2][2], U first, for ``"i420"`` the U plane
    [H / 2][W / 2] and the V plane.  Pixel (x, y) takes the chroma sample (x >> 1, y >> 1) -- nearest siting -- and the
    integers of ``yuv_coefficients(matrix, range)``; the result is the bits the RGB call gives the converted frames.  Boxes
    stay in luma pixels.  An odd H or W, a wrong rank and unknown names raise ValueError before any launch.

    The other formats are read in place by the ``_surface`` entries: ``"bgr24"`` [B, L, H, W, 3], ``"rgba32"`` / ``"bgra32"``
    [B, L, H, W, 4] (the fourth byte is never read), ``"yuyv422"`` / ``"uyvy422"`` [B, L, H, W, 2] with W even (a row is
    ``Y0 U Y1 V`` / ``U Y0 V Y1``; pixel (x, y) takes its own Y and the chroma of pair x >> 1 of its row, the integers of
    ``yuv_coefficients``).  A view of a packed format whose strides are rows of pixels is read through them, not copied.
    ``layout=`` (keyword, on ``aligned`` too): the ``surface_layout`` of the frames -- row pitches, plane offsets, frame
    stride, chroma order -- of any format, ``"rgb24"``, ``"nv12"`` and ``"i420"`` included; ``frames`` is then a contiguous
    uint8 tensor [B, L, ...] with ``layout.frame_stride`` bytes per frame.  Either way the result is the bits the
    ``"rgb24"`` call gives the converted, tightly packed frames.
    """

    def __init__(self, size=48, crop=40, train=True, mean=0.5, std=0.5, max_side=BOX_MAX_SIDE, pixel_format="rgb24",
                 matrix="bt601", range="limited"):
        self.size, self.crop, self.train, self.mean, self.std = size, crop, train, float(mean), float(std)
        self.pixel_format, self.matrix, self.range = pixel_format, matrix, range
        self.yuv = yuv_desc(pixel_format, matrix, range)
        self._coef, self._surfaces = yuv_coefficients(matrix, range), {}
        if isinstance(max_side, bool) or int(max_side) != max_side or not 1 <= max_side <= BOX_COORD:
            raise ValueError(f"max_side = {max_side!r}: must be an integer in 1 .. {BOX_COORD}")
        self.max_side = int(max_side)
        self._tables = {}

    def _get_tables(self, h, w, device):
        key = (h, w, str(device))
        if key not in self._tables:
            hb, hk = resample_tables(w, self.size)
            vb, vk = resample_tables(h, self.size)
            band = _lib.load().cer_frames_band_rows()
            # the largest input-row span of any band, over every crop offset
            span = 0
            for y0 in range(self.size):
                y1 = min(self.size, y0 + band) - 1
                span = max(span, int(vb[y1, 0] + vb[y1, 1] - vb[y0, 0]))
            dev = [torch.from_numpy(a).to(device) for a in (hb, hk, vb, vk)]
            self._tables[key] = (dev, hk.shape[1], vk.shape[1], span)
        return self._tables[key]

    def draw(self, n_clips, rng=None):
        """(x1, y1, flip) per clip -- the reference's random calls, in its order.  ``rng``: a ``random.Random`` instance to
        draw from (the prefetcher's own stream); default the global ``random`` module the reference uses."""
        rng = random if rng is None else rng
        out = np.zeros((n_clips, 3), np.int32)
        for i in range(n_clips):
            if self.train:
                out[i, 0] = rng.randint(0, self.size - self.crop)
                out[i, 1] = rng.randint(0, self.size - self.crop)
                out[i, 2] = 1 if rng.random() < 0.5 else 0
            else:
                out[i, 0] = out[i, 1] = int(round((self.size - self.crop) / 2.0))
        return out

    def _source(self, frames, layout, lead, who="frames"):
        """How frames that do not go through the RGB and 4:2:0 entries are read in place: None when they do go through
        them -- a contiguous ``rgb24`` tensor, ``nv12`` / ``i420`` without a layout -- else (the frames with their ``lead``
        leading dimensions flattened into one, those dimensions, H, W, the ``Surface``).  Under ``layout`` the frames are a
        contiguous uint8 tensor with ``layout.frame_stride`` bytes per frame; without one they are [..., H, W, C] of a packed
        format, and a view whose strides are rows of pixels is read through them (``SurfaceLayout.of_view``), any other is
        copied.  Every refusal is a ValueError; the shape is looked at first, then the device."""
        fmt, f = self.pixel_format, frames
        if layout is not None:
            if not isinstance(layout, SurfaceLayout):
                raise ValueError(f"layout: expected a SurfaceLayout (frames.surface_layout), got {type(layout).__name__}")
            if layout.pixel_format != fmt:
                raise ValueError(f"layout: its pixel_format {layout.pixel_format!r} is not this one's, {fmt!r}")
            if not (torch.is_tensor(f) and f.dtype == torch.uint8 and f.dim() > lead and f.is_contiguous()
                    and int(np.prod(f.shape[lead:])) == layout.frame_stride):
                raise ValueError(f"{who}: expected a contiguous uint8 tensor of layout.frame_stride = {layout.frame_stride} bytes per "
                                 f"frame after {lead} leading dimension(s), got "
                                 f"{(f.dtype, tuple(f.shape), f.is_contiguous()) if torch.is_tensor(f) else type(f)}")
            if not f.is_cuda:
                raise ValueError(f"{who}: on {f.device}; they must be on the GPU (there is no CPU fallback)")
            return f.view(-1, layout.frame_stride), tuple(f.shape[:lead]), layout.height, layout.width, self._surface(layout)
        if fmt in ("nv12", "i420"):
            return None
        chan, dims = 2 if fmt in YUV422_FORMATS else PACKED_FORMATS[fmt][0], (4,) if lead == 1 else (4, 5)
        if fmt == "rgb24":      # what today's entries take, and what they refuse in their own words
            if not (torch.is_tensor(f) and f.is_cuda and f.dtype == torch.uint8 and f.dim() in dims
                    and f.shape[-1] == 3 and min(f.shape) >= 1 and not f.is_contiguous()):
                return None
        elif not (torch.is_tensor(f) and f.dtype == torch.uint8 and f.dim() in dims and f.shape[-1] == chan):
            raise ValueError(f"{who}: expected raw {fmt} frames as a uint8 tensor [{'B, L' if lead == 2 else 'M'}, H, W, {chan}], got "
                             f"{(f.dtype, tuple(f.shape)) if torch.is_tensor(f) else type(f)}")
        if f.dim() == 4 and lead == 2:
            f = f.unsqueeze(0)
        h, w = f.shape[-3], f.shape[-2]
        if fmt in YUV422_FORMATS and w % 2:
            raise ValueError(f"{who}: a 4:2:2 picture needs an even W, got {w}")
        if min(f.shape[:-3]) and (h < 1 or w < 1):
            raise ValueError(f"{who}: empty images {tuple(f.shape)}")
        if not f.is_cuda:
            raise ValueError(f"{who}: on {f.device}; they must be on the GPU (there is no CPU fallback)")
        shape, flat = tuple(f.shape[:lead]), f.flatten(0, lead - 1)
        if not flat.numel():
            return flat, shape, h, w, None
        try:
            layout = SurfaceLayout.of_view(flat, fmt)
        except ValueError:
            if fmt == "rgb24":
                return None
            flat = flat.contiguous()
            layout = SurfaceLayout.of_view(flat, fmt)
        return flat, shape, h, w, self._surface(layout)

    def _surface(self, layout):
        """The ``Surface`` of a layout under this transform's conversion, kept per layout."""
        if layout not in self._surfaces:
            if len(self._surfaces) >= 64:
                self._surfaces.clear()
            self._surfaces[layout] = Surface(layout, self._coef)
        return self._surfaces[layout]

    def _clip(self, frames):
        """The clip as a contiguous [B, L, ...] tensor, (B, L, H, W) of its pictures, and None -- or, for frames read in place
        (``_source``), the frames as [B * L, ...] and the ``Surface`` they are read through."""
        frames, layout = _unlaid(frames)
        src = self._source(frames, layout, 2, "FrameTransform: frames")
        if src is not None:
            flat, (b, l), h, w, surface = src
            return flat, b, l, h, w, surface
        return (*self._clip_packed(frames), None)

    def _clip_packed(self, frames):
        if self.yuv is not None:      # the shape is looked at first, then the device
            if not (torch.is_tensor(frames) and frames.dtype == torch.uint8 and frames.dim() in (3, 4)):
                raise ValueError(f"FrameTransform: {self.pixel_format} frames are a uint8 tensor [B, L, H * 3 / 2, W], got "
                                 f"{(frames.dtype, tuple(frames.shape)) if torch.is_tensor(frames) else type(frames)}")
            if frames.dim() == 3:
                frames = frames.unsqueeze(0)
            h, w = yuv_picture(frames.shape[2], frames.shape[3])
            if not frames.is_cuda:
                raise ValueError(f"FrameTransform: frames on {frames.device}; they must be on the GPU (there is no CPU fallback)")
            return (frames.contiguous(), *frames.shape[:2], h, w)
        if not frames.is_cuda or frames.dtype != torch.uint8:
            raise RuntimeError("FrameTransform needs a uint8 CUDA tensor [B,L,H,W,3] (there is no CPU fallback)")
        if frames.dim() == 4:
            frames = frames.unsqueeze(0)
        b, l, h, w, c = frames.shape
        if c != 3:
            raise RuntimeError("FrameTransform: frames must be RGB, channels last")
        return frames.contiguous(), b, l, h, w

    @takes_layout("frames")
    def __call__(self, frames, crop_xyf=None, return_u8=False, boxes=None):
        clip = self._clip(frames)
        if boxes is None:
            return self._run(clip, crop_xyf, return_u8, None, self._plain, ops.frames_transform)
        return self._run(clip, crop_xyf, return_u8, lambda rows: check_boxes(boxes, rows, self.max_side),
                         lambda *_: (box_tables(self.size, self.max_side),), ops.frames_transform_boxes)

    def _plain(self, h, w, device):
        """What the plain wrappers take after the frames: (the four resample tables of an H x W picture, the band span)."""
        tables, _, _, span = self._get_tables(h, w, device)
        return tables, span

    def _run(self, clip, crop_xyf, return_u8, table, how, call):
        """Everything after ``_clip()``: the crop entries, the outputs, and the launches over chunks of whole clips of at most
        65535 frames.  ``table(rows)``: the checked host table that comes with the frames (boxes, affines), or None;
        ``how(H, W, device)``: what ``call`` takes between the frames (and their table) and ``size`` -- ``_plain``, the box
        store, the affine geometry; ``call``: the ``ops.frames_transform*`` that runs one chunk."""
        frames, b, l, h, w, surface = clip
        if crop_xyf is None:
            crop_xyf = self.draw(b)
        crop_xyf = np.ascontiguousarray(crop_xyf, dtype=np.int32).reshape(b, 3)
        if (crop_xyf[:, :2] < 0).any() or (crop_xyf[:, :2] + self.crop > self.size).any():
            raise RuntimeError("FrameTransform: crop offset outside the resized image")
        rows = None if table is None else table(b * l)
        if l > 65535:
            raise RuntimeError("FrameTransform: clip longer than 65535 frames")
        how = how(h, w, frames.device)
        cx = torch.from_numpy(crop_xyf).to(frames.device)
        rows = None if rows is None else torch.from_numpy(rows).to(frames.device)
        out = torch.empty((b, l, 3, self.crop, self.crop), dtype=torch.float32, device=frames.device)
        u8 = torch.empty((b, l, self.crop, self.crop, 3), dtype=torch.uint8, device=frames.device) if return_u8 else None
        n, step = b * l, 65535 // l * l
        flat_in = frames if surface is not None else frames.view(n, *frames.shape[2:])
        flat_out = out.view(n, 3, self.crop, self.crop)
        flat_u8 = u8.view(n, self.crop, self.crop, 3) if return_u8 else None
        for s in range(0, n, step):
            e = min(n, s + step)
            call(flat_in[s:e], *([] if rows is None else [rows[s:e]]), *how, self.size, cx[s // l:e // l], l, self.mean, self.std,
                 flat_out[s:e], flat_u8[s:e] if return_u8 else None, **({"yuv": self.yuv} if surface is None else {"surface": surface}))
        return (out, u8) if return_u8 else out

    @takes_layout("frames")
    def aligned(self, frames, affines, crop_xyf=None, return_u8=False, align_size=ALIGN_SIZE):
        """``__call__`` of full camera frames with one affine map per frame: ``affines`` [B, L, 6] or [B * L, 6] host
        float64, Pillow's coefficients (``similarity_from_landmarks`` makes them from five landmarks).  Frame f is first
        warped to an ``align_size`` x ``align_size`` face as ``PIL.Image.transform((A, A), AFFINE, affines[f], BILINEAR)``
        does -- zero outside the frame -- so the result is what the plain call gives those faces.  One launch for any mix of
        maps (csrc/frames_affine.hip); the pixel format is the transform's."""
        geom = affine_geometry(align_size, self.size)
        geom.check_crop(self.crop)
        rank = 5 if self.yuv is None else 4
        if torch.is_tensor(frames) and frames.dim() in (rank - 1, rank):      # the table is looked at first, like boxes
            check_affines(affines, int(np.prod(frames.shape[:frames.dim() - rank + 2])))
        return self._run(self._clip(frames), crop_xyf, return_u8, lambda rows: check_affines(affines, rows), lambda *_: (geom,),
                         ops.frames_transform_affine)


def hold_ring(hold, max_new):
    """Slots of a ring in which up to ``hold`` rows wait while a push adds up to ``max_new``: the power of two >= their sum."""
    return ops.pow2_at_least(hold + max_new)


class FrameStream:
    """``FrameTransform(size, crop, train=False)`` for ``streams`` live cameras, a few raw frames at a time; the video
    counterpart of ``LogMelStream``.

      push(frames_u8 [M, H, W, 3], counts, boxes=None)
                                            stream s brings ``counts[s]`` (0 .. max_new) new frames, packed stream-major in
                                            ascending stream order, each stream's in time order.  H and W may differ from push
                                            to push (the ring holds crops; coefficient tables are cached per geometry).
                                            Returns nothing: the frames wait.  ``boxes`` [M, 4] host integers, one
                                            (x0, y0, x1, y1) per packed frame: the frames are full camera frames and each
                                            is cropped to its box first, as ``FrameTransform(..., boxes=)`` does (sides up
                                            to ``max_side``; still one upload and one launch).  Boxed and unboxed pushes
                                            may alternate: the ring holds crops.
      push_aligned(frames_u8, counts, affines, align_size=256)
                                            the same for full camera frames with one affine map per packed frame,
                                            ``affines`` [M, 6] host float64 (``similarity_from_landmarks``): each frame is
                                            warped to an ``align_size`` face as ``FrameTransform.aligned`` does; one upload
                                            and one launch, and it may alternate with the other two.
      take(pairs)                           pairs = (stream, frame number) per row -> float32 [M, 3, crop, crop], the bits
                                            ``FrameTransform`` gives those frames.  A stream's frames up to the largest one
                                            taken are released; the others go on waiting.
      reset(streams=None)                   forget those streams.
      frames_seen, frames_taken             host lists, one int per stream; ``held`` their difference.

    State (csrc/frames_stream.hip): one uint8 ring [S, Rf, crop, crop, 3] on the device that holds the resized, cropped and
    flipped bytes, Rf = ``hold_ring(hold, max_new)``, and the two host ints per stream.  A push uploads one row table and runs
    one launch, a take one more of each, whatever the number of streams.  The crop is GroupCenterCrop's offset for every stream
    unless ``crop_xyf`` [S, 3] = (x1, y1, flip) per stream says otherwise.

    ``pixel_format`` / ``matrix`` / ``range``: as for ``FrameTransform``.  Under ``"nv12"`` or ``"i420"`` a push brings
    uint8 [M, H * 3 / 2, W], H and W even; everything else is as under ``"rgb24"``, and so are the ring's bytes for the
    converted frames.  The format is the stream's, not a push's.  ``"bgr24"``, ``"rgba32"``, ``"bgra32"`` [M, H, W, 3 | 4]
    and ``"yuyv422"``, ``"uyvy422"`` [M, H, W, 2] are read in place, as ``FrameTransform`` reads them, and so is a strided
    view of a packed format.  ``layout=`` on ``push``, ``push_aligned`` and their checks is the ``surface_layout`` of that
    push's frames, a contiguous uint8 tensor [M, ...] of ``layout.frame_stride`` bytes per frame (a pitched or padded
    surface); it belongs to the push, as H and W do, and its ``pixel_format`` must be the stream's.

    A push that would leave more than ``hold`` untaken frames in a stream, bad counts, and a tensor that is not uint8 RGB on
    the GPU (or not a 4:2:0 frame of an even-sized picture, under those formats) raise ValueError before any launch and leave
    the state as it was."""

    def __init__(self, streams, size=48, crop=40, hold=64, max_new=32, mean=0.5, std=0.5, device="cuda", crop_xyf=None,
                 max_side=BOX_MAX_SIDE, pixel_format="rgb24", matrix="bt601", range="limited"):
        for name, v in (("streams", streams), ("size", size), ("crop", crop), ("hold", hold), ("max_new", max_new),
                        ("max_side", max_side)):
            if isinstance(v, bool) or int(v) != v or v < 1:
                raise ValueError(f"{name} = {v!r}: must be an integer >= 1")
        if crop > size:
            raise ValueError(f"crop = {crop} exceeds size = {size}")
        if float(std) == 0.0:
            raise ValueError("std = 0")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"FrameStream runs on the HIP kernels only (no CPU fallback), got device {device!r}")
        self.streams, self.size, self.crop, self.hold, self.max_new = int(streams), int(size), int(crop), int(hold), int(max_new)
        self.ring_frames = hold_ring(self.hold, self.max_new)
        self._xf = FrameTransform(self.size, self.crop, train=False, mean=mean, std=std, max_side=max_side,
                                  pixel_format=pixel_format, matrix=matrix, range=range)
        self.pixel_format = pixel_format
        self.max_side = self._xf.max_side
        if crop_xyf is None:
            crop_xyf = self._xf.draw(self.streams)
        crop_xyf = np.ascontiguousarray(crop_xyf, dtype=np.int32)
        if crop_xyf.shape != (self.streams, 3):
            raise ValueError(f"crop_xyf: expected one (x1, y1, flip) per stream [{self.streams}, 3], got {crop_xyf.shape}")
        if (crop_xyf[:, :2] < 0).any() or (crop_xyf[:, :2] + self.crop > self.size).any():
            raise ValueError("crop_xyf: crop offset outside the resized image")
        self.crop_xyf = crop_xyf
        self.frames_seen = [0] * self.streams
        self.frames_taken = [0] * self.streams
        self._base = [0] * self.streams   # ring position of a stream's frame 0
        self.ring = self._cx = None       # allocated by the first push that launches

    @property
    def held(self):
        return [n - t for n, t in zip(self.frames_seen, self.frames_taken)]

    def _indices(self, streams):
        idx = list(range(self.streams)) if streams is None else [int(s) for s in streams]
        for s in idx:
            if not 0 <= s < self.streams:
                raise IndexError(f"stream {s} of {self.streams}")
        return idx

    def reset(self, streams=None):
        """Forget ``streams`` (indices; None = all).  Only host ints change: no slot is read that was not written since."""
        for s in self._indices(streams):
            self.frames_seen[s] = self.frames_taken[s] = 0

    @takes_layout("frames_u8")
    def check_push(self, frames_u8, counts, boxes=None):
        """Everything ``push`` refuses, without a launch or a change of state.  Returns the counts as ints."""
        return self._check_push(frames_u8, counts, self._box_rows(boxes))[0]

    @takes_layout("frames_u8")
    def check_push_aligned(self, frames_u8, counts, affines, align_size=ALIGN_SIZE):
        """Everything ``push_aligned`` refuses, without a launch or a change of state.  Returns the counts as ints."""
        return self._check_push(frames_u8, counts, self._affine_rows(affines, align_size))[0]

    def _box_rows(self, boxes):
        return None if boxes is None else lambda rows: check_boxes(boxes, rows, self.max_side)

    def _affine_rows(self, affines, align_size):
        def table(rows):
            arr = check_affines(affines, rows)
            affine_geometry(align_size, self.size).check_crop(self.crop)
            return arr
        return table

    def _check_push(self, frames_u8, counts, table):
        """The checks of every kind of push; ``table(rows)`` checks the per-frame table that comes with the frames (None: there
        is none).  Returns (the counts as ints, that table as ``table`` returns it, how the frames are read: None or what
        ``FrameTransform._source`` returns)."""
        try:
            counts = [int(c) for c in counts]
        except TypeError:
            raise ValueError(f"counts: expected a sequence of {self.streams} ints, got {type(counts).__name__}") from None
        if len(counts) != self.streams:
            raise ValueError(f"counts: expected one count per stream ({self.streams}), got {len(counts)}")
        for s, c in enumerate(counts):
            if not 0 <= c <= self.max_new:
                raise ValueError(f"counts: stream {s} brings {c} frames, outside 0 .. max_new = {self.max_new}")
            if self.held[s] + c > self.hold:
                raise ValueError(f"stream {s}: {self.held[s]} frames wait and {c} more exceed hold = {self.hold}; take some first")
        rows = None if table is None else table(sum(counts))
        f, layout = _unlaid(frames_u8)
        src = self._xf._source(f, layout, 1)
        if src is not None:
            f = src[0]
        elif self._xf.yuv is not None:      # the shape is looked at first, then the device
            if not (torch.is_tensor(f) and f.dtype == torch.uint8 and f.dim() == 3):
                raise ValueError(f"frames: expected raw {self.pixel_format} frames as a uint8 tensor [M, H * 3 / 2, W], got "
                                 f"{(f.dtype, tuple(f.shape)) if torch.is_tensor(f) else type(f)}")
            if f.shape[0]:
                yuv_picture(f.shape[1], f.shape[2])
            if not f.is_cuda:
                raise ValueError(f"frames: on {f.device}; they must be on the GPU (there is no CPU fallback)")
        elif not (torch.is_tensor(f) and f.is_cuda and f.dtype == torch.uint8 and f.dim() == 4 and f.shape[3] == 3):
            raise ValueError("frames: expected raw RGB frames as a uint8 GPU tensor [M, H, W, 3] (there is no CPU fallback), got "
                             f"{(f.dtype, f.device, tuple(f.shape)) if torch.is_tensor(f) else type(f)}")
        if f.shape[0] != sum(counts):
            raise ValueError(f"frames: {f.shape[0]} frames for counts that sum to {sum(counts)}")
        if f.shape[0] > 65535:
            raise ValueError(f"frames: {f.shape[0]} frames in one push exceed 65535")
        if src is None and f.shape[0] and (f.shape[1] < 1 or f.shape[2] < 1):
            raise ValueError(f"frames: empty images {tuple(f.shape)}")
        return counts, rows, src

    def _alloc(self):
        if self.ring is None:
            self.ring = torch.zeros((self.streams, self.ring_frames, self.crop, self.crop, 3), device=self.device,
                                    dtype=torch.uint8)
            self._cx = torch.from_numpy(self.crop_xyf).to(self.device)

    @torch.no_grad()
    def _push(self, frames_u8, counts, table, how, upload, append):
        """The body of every kind of push.  ``table``: as for ``_check_push``; ``how``: as for ``FrameTransform._run``;
        ``upload``: the ``ops.stream_row_*table`` that takes what ``table`` returns; ``append``: the
        ``ops.frames_stream_append*`` of the one launch."""
        counts, rows, src = self._check_push(frames_u8, counts, table)
        if not sum(counts):
            return
        if src is not None:
            frames, _, h, w, surface = src
            read = {"surface": surface}
        else:
            frames, yuv = frames_u8.contiguous(), self._xf.yuv
            h, w = frames.shape[1:3] if yuv is None else yuv_picture(frames.shape[1], frames.shape[2])
            read = {"yuv": yuv}
        how = how(h, w, frames.device)
        self._alloc()
        first = [b + n for b, n in zip(self._base, self.frames_seen)]
        row_stream, row_pos, *rows = upload(first, counts, *([] if rows is None else [rows]), self.device)
        append(frames, *rows, *how, self.size, self._cx, row_stream, row_pos, max(counts), self.ring, **read)
        self.frames_seen = [n + c for n, c in zip(self.frames_seen, counts)]

    @takes_layout("frames_u8")
    def push(self, frames_u8, counts, boxes=None):
        if boxes is None:
            return self._push(frames_u8, counts, None, self._xf._plain, ops.stream_row_table, ops.frames_stream_append)
        return self._push(frames_u8, counts, self._box_rows(boxes), lambda *_: (box_tables(self.size, self.max_side),),
                          ops.stream_row_box_table, ops.frames_stream_append_boxes)

    @takes_layout("frames_u8")
    def push_aligned(self, frames_u8, counts, affines, align_size=ALIGN_SIZE):
        """``push`` of full camera frames with one affine map per packed frame: ``affines`` [M, 6] host float64, Pillow's
        coefficients (``similarity_from_landmarks`` makes them from five landmarks).  Frame m is warped to an
        ``align_size`` x ``align_size`` face as ``PIL.Image.transform((A, A), AFFINE, affines[m], BILINEAR)`` does and that
        face goes through GroupScale -> crop -> flip: the ring gets the bytes ``push`` gives the warped faces.  Still one
        upload and one launch (csrc/frames_affine.hip); aligned, boxed and plain pushes may alternate."""
        return self._push(frames_u8, counts, self._affine_rows(affines, align_size),
                          lambda *_: (affine_geometry(align_size, self.size),), ops.stream_row_affine_table, ops.frames_stream_append_affine)

    def check_take(self, pairs):
        """What ``take`` refuses.  Returns the pairs as ints."""
        pairs = [(int(s), int(i)) for s, i in pairs]
        for s, i in pairs:
            if not 0 <= s < self.streams:
                raise ValueError(f"take: stream {s} of {self.streams}")
            if not self.frames_taken[s] <= i < self.frames_seen[s]:
                raise ValueError(f"take: frame {i} of stream {s} is not held (frames {self.frames_taken[s]} .. "
                                 f"{self.frames_seen[s] - 1} are)")
        if len(pairs) > 65535:
            raise ValueError(f"take: {len(pairs)} frames in one call exceed 65535")
        return pairs

    @torch.no_grad()
    def take(self, pairs):
        pairs = self.check_take(pairs)
        if not pairs:
            return torch.empty((0, 3, self.crop, self.crop), device=self.device, dtype=torch.float32)
        row_stream, row_pos = ops.stream_pair_table([(s, self._base[s] + i) for s, i in pairs], self.device)
        out = ops.frames_stream_gather(self.ring, row_stream, row_pos, self._xf.mean, self._xf.std)
        for s, i in pairs:
            self.frames_taken[s] = max(self.frames_taken[s], i + 1)
        return out
