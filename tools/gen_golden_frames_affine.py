"""Golden fixture for per-frame affine maps, from PIL itself: ``Image.transform((32, 32), Image.AFFINE, a, Image.BILINEAR)`` of
one 90 x 120 RGB frame for each of ``affine_ref.GOLDEN_AFFINES`` -- the warp the reference's aligners apply to every face.

    python tools/gen_golden_frames_affine.py
"""
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from affine_ref import GOLDEN_AFFINES, GOLDEN_ALIGN  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "frames_affine.npz")
SEED = 2026


def main():
    frame = np.random.default_rng(SEED).integers(0, 256, (90, 120, 3), dtype=np.uint8)
    pil = Image.fromarray(frame)
    size = (GOLDEN_ALIGN, GOLDEN_ALIGN)
    warped = np.stack([np.asarray(pil.transform(size, Image.AFFINE, tuple(a), resample=Image.BILINEAR)) for a in GOLDEN_AFFINES])
    np.savez_compressed(OUT, seed=np.array([SEED]), frame=frame, affines=np.array(GOLDEN_AFFINES, np.float64),
                        align=np.array([GOLDEN_ALIGN]), warped=warped)
    print(OUT, os.path.getsize(OUT))


if __name__ == "__main__":
    main()
