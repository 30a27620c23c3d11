"""Golden fixture for per-frame face boxes, from PIL itself: ``Image.crop(box)`` of an integer box that may leave the picture,
then ``Image.resize((48, 48), BILINEAR)`` -- the crop-then-resize the reference's aligner falls back to.

    python tools/gen_golden_frames_boxes.py
"""
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from frames_box_ref import GOLDEN_BOXES  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "frames_boxes.npz")
SEED = 2025


def main():
    frame = np.random.default_rng(SEED).integers(0, 256, (90, 120, 3), dtype=np.uint8)
    pil = Image.fromarray(frame)
    resized = np.stack([np.asarray(pil.crop(box).resize((48, 48), Image.BILINEAR)) for box in GOLDEN_BOXES])
    np.savez_compressed(OUT, seed=np.array([SEED]), frame=frame, boxes=np.array(GOLDEN_BOXES, np.int32), resized=resized)
    print(OUT, os.path.getsize(OUT))


if __name__ == "__main__":
    main()
