"""What a face box means, restated without the kernels: ``PIL.Image.crop`` of an integer box (x0, y0, x1, y1), right and lower
exclusive, zero outside the picture, as a contiguous array.  Shared by tests/test_frames_boxes_cpu.py and
tests/test_frames_boxes_gpu.py."""
import numpy as np
import torch

# the boxes of tests/golden/frames_boxes.npz, on its 90 x 120 frame: inside, the whole frame, out on the left / top, out on
# the right / bottom, 1 x 1, tall and narrow, enclosing the frame, 3 x 70
GOLDEN_BOXES = [(10, 5, 74, 69), (0, 0, 120, 90), (-7, -3, 40, 50), (100, 70, 131, 97), (33, 21, 34, 22), (5, 5, 18, 44),
                (-20, -20, 140, 110), (50, 10, 53, 80)]


def pad_slice(frame, box):
    """frame [H, W, 3] (numpy or torch, any device), box = (x0, y0, x1, y1) -> the contiguous [y1 - y0, x1 - x0, 3] slice,
    zero where the box leaves the frame."""
    x0, y0, x1, y1 = (int(v) for v in box)
    h, w = frame.shape[0], frame.shape[1]
    if torch.is_tensor(frame):
        out = torch.zeros((y1 - y0, x1 - x0, frame.shape[2]), dtype=frame.dtype, device=frame.device)
    else:
        out = np.zeros((y1 - y0, x1 - x0, frame.shape[2]), dtype=frame.dtype)
    sx0, sy0, sx1, sy1 = max(x0, 0), max(y0, 0), min(x1, w), min(y1, h)
    if sx1 > sx0 and sy1 > sy0:
        out[sy0 - y0:sy1 - y0, sx0 - x0:sx1 - x0] = frame[sy0:sy1, sx0:sx1]
    return out
