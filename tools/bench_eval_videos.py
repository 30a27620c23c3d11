"""Whole-video evaluation throughput of ``Trainer.inference`` with the HIP LFAN (video + vggish + bert, 40x40 frames,
window 300 / hop 200) over synthetic videos, for several ``eval_video_batch`` settings: videos/s and model forwards per
video.  ``eval_video_batch`` 1 is the per-video path (one forward per video of one window, one forward per group of
windows of a longer video); > 1 lets the windows of several videos share forwards.  Prints one JSON line per setting."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.modules.setdefault("triton", None)
from feature_vs_text_compound_emotion_amd import metrics, synth  # noqa: E402
from feature_vs_text_compound_emotion_amd.lfan import LFAN  # noqa: E402
from feature_vs_text_compound_emotion_amd.trainer import Trainer  # noqa: E402

MODS = ["video", "vggish", "bert"]


def make_loader(n_videos, window, hw, seed):
    """Half of the videos exactly one window long, the rest 1.1x - 2.5x the window; one class per video."""
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)
    loader = []
    for v in range(n_videos):
        n = window if v % 2 == 0 else int(rng.integers(window + window // 10, 5 * window // 2))
        u8 = torch.randint(0, 256, (1, n, hw, hw, 3), generator=g, dtype=torch.uint8)
        X = {"video": ((u8.float() / 255.0 - 0.5) / 0.5).permute(0, 1, 4, 2, 3).contiguous()}
        for m in MODS[1:]:
            X[m] = torch.randn(1, 1, n, synth.EMBEDDING_DIM[m], generator=g)
        X["EXPR_continuous_label"] = torch.full((1, n, 1), float(rng.integers(0, 7)))
        loader.append((X, [f"v{v}"], [n], [np.arange(n)]))
    return loader


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=32)
    ap.add_argument("--window", type=int, default=300)
    ap.add_argument("--hop", type=int, default=200)
    ap.add_argument("--hw", type=int, default=40)
    ap.add_argument("--budget-windows", type=int, default=16, help="eval_frame_budget in windows")
    ap.add_argument("--video-batch", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--keep-logits", action="store_true", help="also copy every video's logits to the host")
    a = ap.parse_args()
    sd = synth.lfan_state_dict(MODS, n_cls=7, head_hw=a.hw // 8, seed=0)
    model = LFAN(backbone_settings={}, output_dim=7, task="CLASSIFICATION", modality=MODS, example_length=a.window,
                 kernel_size=5, tcn_channel=synth.TCN_CHANNELS, root_dir="", device="cuda", head_hw=a.hw // 8)
    model.init(load_backbone=False)
    model.load_state_dict(sd, strict=True)
    model = model.cuda().eval()
    loader = make_loader(a.videos, a.window, a.hw, seed=1)
    frames = sum(int(x[2][0]) for x in loader)
    tr = Trainer(model, device="cuda", window_length=a.window, hop_length=a.hop, number_classes=7)
    tr.eval_frame_budget = a.budget_windows * a.window
    calls = []
    model.register_forward_pre_hook(lambda mod, args: calls.append(1))
    base = None
    for vb in a.video_batch:
        tr.eval_video_batch = vb
        perf, _ = tr.inference(loader, keep_logits=a.keep_logits)      # warm-up (first-call allocations, weight packing)
        torch.cuda.synchronize()
        calls.clear()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            perf, _ = tr.inference(loader, keep_logits=a.keep_logits)   # ends with the device -> host copy of the counts
        torch.cuda.synchronize()
        sec = (time.perf_counter() - t0) / a.iters
        master = perf[None][metrics.W_F1][metrics.FRAME_LEVEL]["master"]
        rec = {"eval_video_batch": vb, "videos": a.videos, "frames": frames, "window": a.window, "hop": a.hop, "hw": a.hw,
               "budget_windows": a.budget_windows, "keep_logits": a.keep_logits, "sec_per_pass": sec,
               "videos_per_s": a.videos / sec, "forwards_per_video": len(calls) / a.iters / a.videos, "frame_w_f1": master}
        if base is None:
            base = sec
        rec["speedup_vs_first"] = base / sec
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
