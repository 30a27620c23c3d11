"""8-bit 4:2:0 frames to RGB in numpy: the stated conversion of the ``nv12`` / ``i420`` pixel formats, restated from its
definition and not from the kernel.

A frame of an H x W picture (H, W even) is H * 3 / 2 rows of W bytes.  The Y plane [H][W] comes first; ``nv12`` follows it with
the interleaved chroma [H / 2][W / 2][2], U first; ``i420`` with the U plane [H / 2][W / 2] and then the V plane.  Pixel (x, y)
takes the chroma sample (x >> 1, y >> 1).  With c = Y - yoff, u = U - 128, v = V - 128 in int32 and ``>>`` the arithmetic shift,

    R = clip8((cy c + crv v + 2^13) >> 14),  G = clip8((cy c + cgu u + cgv v + 2^13) >> 14),  B = clip8((cy c + cbu u + 2^13) >> 14)
"""
import numpy as np

# (matrix, range) -> cy, crv, cgu, cgv, cbu, yoff: the recorded table
COEFFICIENTS = {
    ("bt601", "limited"): (19077, 26149, -6419, -13320, 33050, 16),
    ("bt601", "full"): (16384, 22970, -5638, -11700, 29032, 0),
    ("bt709", "limited"): (19077, 29372, -3494, -8731, 34610, 16),
    ("bt709", "full"): (16384, 25802, -3069, -7670, 30402, 0),
}
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
SCALES = {"limited": (255 / 219, 255 / 224, 16), "full": (1.0, 1.0, 0)}     # luma scale, chroma scale, yoff
LAYOUTS = ("nv12", "i420")


def convert(y, u, v, matrix="bt601", range="limited"):
    """Integer arrays of one shape (bytes) -> uint8 [..., 3]."""
    cy, crv, cgu, cgv, cbu, yoff = COEFFICIENTS[matrix, range]
    c = cy * (np.asarray(y, np.int32) - yoff) + (1 << 13)
    u, v = np.asarray(u, np.int32) - 128, np.asarray(v, np.int32) - 128
    rgb = np.stack([(c + crv * v) >> 14, (c + cgu * u + cgv * v) >> 14, (c + cbu * u) >> 14], axis=-1)
    return np.clip(rgb, 0, 255).astype(np.uint8)


def convert_float(y, u, v, matrix="bt601", range="limited"):
    """The same matrix in float64, rounded half up and clipped: what the fixed point approximates."""
    (kr, kb), (ys, cs, yoff) = KR_KB[matrix], SCALES[range]
    kg = 1 - kr - kb
    c = ys * (np.asarray(y, np.float64) - yoff)
    u, v = np.asarray(u, np.float64) - 128, np.asarray(v, np.float64) - 128
    rgb = np.stack([c + 2 * (1 - kr) * cs * v,
                    c - 2 * (1 - kb) * kb / kg * cs * u - 2 * (1 - kr) * kr / kg * cs * v,
                    c + 2 * (1 - kb) * cs * u], axis=-1)
    return np.clip(np.floor(rgb + 0.5), 0, 255).astype(np.uint8)


def planes(frames, layout):
    """uint8 [M, H * 3 / 2, W] -> (Y [M, H, W], U [M, H / 2, W / 2], V [M, H / 2, W / 2])."""
    frames = np.asarray(frames)
    m, rows, w = frames.shape
    assert frames.dtype == np.uint8 and rows % 3 == 0 and w % 2 == 0 and layout in LAYOUTS
    h = rows // 3 * 2
    y, chroma = frames[:, :h], frames[:, h:].reshape(m, -1)
    if layout == "nv12":
        uv = chroma.reshape(m, h // 2, w // 2, 2)
        return y, uv[..., 0], uv[..., 1]
    quarter = (h // 2) * (w // 2)
    return y, chroma[:, :quarter].reshape(m, h // 2, w // 2), chroma[:, quarter:].reshape(m, h // 2, w // 2)


def pack(y, u, v, layout):
    """The inverse of ``planes``: -> uint8 [M, H * 3 / 2, W]."""
    y, u, v = (np.asarray(a, np.uint8) for a in (y, u, v))
    m, h, w = y.shape
    assert h % 2 == 0 and w % 2 == 0 and u.shape == v.shape == (m, h // 2, w // 2) and layout in LAYOUTS
    chroma = np.stack([u, v], axis=-1) if layout == "nv12" else np.stack([u, v], axis=1)
    return np.concatenate([y.reshape(m, -1), chroma.reshape(m, -1)], axis=1).reshape(m, h * 3 // 2, w)


def yuv_to_rgb(frames, layout, matrix="bt601", range="limited"):
    """uint8 [M, H * 3 / 2, W] -> uint8 [M, H, W, 3], chroma sample (x >> 1, y >> 1) for pixel (x, y)."""
    y, u, v = planes(frames, layout)
    up = lambda p: np.repeat(np.repeat(p, 2, axis=1), 2, axis=2)      # noqa: E731
    return np.ascontiguousarray(convert(y, up(u), up(v), matrix, range))
