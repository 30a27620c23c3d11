"""What an affine map means, restated without the kernels: ``PIL.Image.transform((A, A), Image.AFFINE, a, Image.BILINEAR)`` of an
RGB picture in numpy float64 (Pillow's affine_transform + bilinear_filter32RGB of Geometry.c, third-party, restated), and the
closed-form similarity fit of five landmarks to the ArcFace template.  Shared by tests/test_frames_affine_cpu.py,
tests/test_frames_affine_gpu.py and tools/gen_golden_frames_affine.py.

For output pixel (x, y), every step in float64, none fused (numpy's elementwise operations round each result):

    xin = x + 0.5; yin = y + 0.5
    X = (a0 xin + a1 yin) + a2;  Y = (a3 xin + a4 yin) + a5
    inside = X >= 0 and X < W and Y >= 0 and Y < H          (else the pixel is 0, 0, 0)
    X -= 0.5; Y -= 0.5; ix = floor(X); iy = floor(Y); dx = X - ix; dy = Y - iy
    x0 = clamp(ix, 0, W - 1); x1 = clamp(ix + 1, 0, W - 1); row0 = clamp(iy, 0, H - 1)
    v1 = p[row0][x0] + (p[row0][x1] - p[row0][x0]) dx
    v2 = p[iy + 1][x0] + (p[iy + 1][x1] - p[iy + 1][x0]) dx  if 0 <= iy + 1 < H  else v1
    byte = uint8(trunc(v1 + (v2 - v1) dy))
"""
import math

import numpy as np

TEMPLATE = np.array([[38.2946, 51.6963], [73.5318, 51.5014], [56.0252, 71.7366], [41.5493, 92.3655], [70.7299, 92.2041]])

GOLDEN_ALIGN = 32


def similarity(angle_deg, scale, cx, cy, align):
    """Pillow coefficients of the map that samples an ``align`` x ``align`` picture around frame point (cx, cy): the output
    centre lands on (cx, cy), one output pixel spans ``scale`` frame pixels, rotated by ``angle_deg``."""
    c, s = math.cos(math.radians(angle_deg)) * scale, math.sin(math.radians(angle_deg)) * scale
    return [c, s, cx - (c + s) * align / 2, -s, c, cy - (-s + c) * align / 2]


# the affines of tests/golden/frames_affine.npz, on its 90 x 120 frame at align 32: the identity on the upper left corner, a
# plain 2.5x reduction, two rotations (one leaving the frame), a magnification, dyadic coefficients that put X on integers
# and halves, a shear that is no similarity, a map wholly outside the frame
GOLDEN_AFFINES = [
    [1.0, 0.0, 0.0, 0.0, 1.0, 0.0],
    similarity(0.0, 2.5, 60.0, 45.0, GOLDEN_ALIGN),
    similarity(17.0, 1.7, 50.0, 40.0, GOLDEN_ALIGN),
    similarity(-33.0, 3.6, 100.0, 70.0, GOLDEN_ALIGN),
    similarity(8.0, 0.3, 31.3, 22.9, GOLDEN_ALIGN),
    [1.25, 0.5, -3.0, -0.25, 1.5, 2.75],
    [2.0, 0.7, 10.0, 0.1, 1.1, 20.0],
    [1.0, 0.0, 500.0, 0.0, 1.0, -300.0],
]


def warp_affine(frame, a, align):
    """frame uint8 [H, W, 3], a = six float64 -> uint8 [align, align, 3]."""
    frame = np.asarray(frame)
    h, w = frame.shape[:2]
    a = [np.float64(v) for v in a]
    xin = (np.arange(align, dtype=np.float64) + 0.5)[None, :]
    yin = (np.arange(align, dtype=np.float64) + 0.5)[:, None]
    with np.errstate(all="ignore"):
        X = (a[0] * xin + a[1] * yin) + a[2]
        Y = (a[3] * xin + a[4] * yin) + a[5]
        inside = (X >= 0) & (X < w) & (Y >= 0) & (Y < h)
    X, Y = np.where(inside, X, 0.5) - 0.5, np.where(inside, Y, 0.5) - 0.5
    fx, fy = np.floor(X), np.floor(Y)
    dx, dy = (X - fx)[..., None], (Y - fy)[..., None]
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    x0, x1, row0 = np.clip(ix, 0, w - 1), np.clip(ix + 1, 0, w - 1), np.clip(iy, 0, h - 1)
    p = frame.astype(np.float64)
    v1 = p[row0, x0] + (p[row0, x1] - p[row0, x0]) * dx
    below = ((iy + 1 >= 0) & (iy + 1 < h))[..., None]
    row1 = np.clip(iy + 1, 0, h - 1)
    v2 = np.where(below, p[row1, x0] + (p[row1, x1] - p[row1, x0]) * dx, v1)
    out = np.trunc(v1 + (v2 - v1) * dy).astype(np.uint8)
    return np.where(inside[..., None], out, np.uint8(0))


def warp_all(frames, affines, align):
    """frames [M, H, W, 3] (or one frame for every affine), affines [M, 6] -> uint8 [M, align, align, 3]."""
    frames = np.asarray(frames)
    pick = (lambda i: frames) if frames.ndim == 3 else (lambda i: frames[i])
    return np.stack([warp_affine(pick(i), a, align) for i, a in enumerate(affines)])


def fit_similarity(landmarks, align):
    """Five (x, y) landmarks -> Pillow's six coefficients, through complex numbers: the least-squares c, t of q = c p + t
    (c = a + i b is the rotation and scale), inverted to p = (q - t) / c, then moved from integer pixel centres to Pillow's
    half-pixel convention."""
    p = np.asarray(landmarks, np.float64)
    q = TEMPLATE * align / 112.0
    zp, zq = p[:, 0] + 1j * p[:, 1], q[:, 0] + 1j * q[:, 1]
    pc, qc = zp - zp.mean(), zq - zq.mean()
    c = (np.conj(pc) * qc).sum() / (np.abs(pc) ** 2).sum()
    t = zq.mean() - c * zp.mean()
    ic, it = 1 / c, -t / c                       # p = ic q + it
    a0, a1, a3, a4 = ic.real, -ic.imag, ic.imag, ic.real
    return np.array([a0, a1, it.real - 0.5 * (a0 + a1) + 0.5, a3, a4, it.imag - 0.5 * (a3 + a4) + 0.5])
