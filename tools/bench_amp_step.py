"""ms per training step of ``Trainer.train_step`` with ``data_parallel`` (one rank, ``FlatNesterovSGD``) under three
regimes: amp off; ``--amp`` with torch's stock ``GradScaler`` (per-parameter foreach unscale + the host read of found_inf in
``_maybe_opt_step`` -- forced here by hiding the optimiser's ``_step_supports_amp_scaling``); ``--amp`` with
``FlatGradScaler`` (one bucket check, the fused update skips / unscales on the device, no host read).

    python tools/bench_amp_step.py [--hw 40] [--batch 32] [--length 32] [--steps 20] [--warmup 3] [--only flat]

LFAN on pre-computed VGGish / BERT features (bench.py's ``--encoders off``), dropout as in training.  Each time is the
wall-clock mean over ``--steps`` steps after warm-up, between two device synchronisations.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

sys.modules.setdefault("triton", None)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

MODS = ["video", "vggish", "bert"]


def build(hw, batch, length, mode):
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.data_parallel import ClipDataParallel, FlatNesterovSGD
    from feature_vs_text_compound_emotion_amd.lfan import LFAN
    from feature_vs_text_compound_emotion_amd.trainer import Trainer
    model = LFAN(backbone_settings={}, output_dim=7, task="CLASSIFICATION", modality=MODS, example_length=length,
                 kernel_size=5, tcn_channel=synth.TCN_CHANNELS, root_dir="", device="cuda", head_hw=hw // 8)
    model.init(load_backbone=False)
    model.load_state_dict(synth.lfan_state_dict(MODS, n_cls=7, head_hw=hw // 8, seed=0), strict=True)
    model = model.cuda().train()
    ddp = ClipDataParallel(model, world_size=1)
    opt = FlatNesterovSGD(ddp, lr=1e-3)
    tr = Trainer(model, optimizer=opt, device="cuda", data_parallel=ddp, train_batch_size=batch, window_length=length)
    tr.args.amp = mode != "off"
    if mode == "stock":
        opt._step_supports_amp_scaling = False           # torch's generic route: foreach unscale, .item() on found_inf
        tr.scaler = torch.amp.GradScaler("cuda")
    x, labels = synth.make_clip_batch(MODS, batch, length, hw=hw, seed=1234)
    X = {**{k: v.cuda() for k, v in x.items()}, "continuous_label": labels.cuda()}
    return tr, X, ddp


def time_mode(hw, batch, length, mode, steps, warmup):
    tr, X, ddp = build(hw, batch, length, mode)
    for _ in range(warmup):
        tr.train_step(X)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.train_step(X)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    out = {"ms_per_step": round(ms, 3), "bucket_floats": ddp.flat.numel()}
    if tr.scaler is not None:
        out["scale"] = tr.scaler.get_scale()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", type=int, default=40, help="40 (the reference's crop) or 224")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--length", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["off", "stock", "flat"], default=None, help="time one regime (for a profiler run)")
    a = ap.parse_args()
    modes = [a.only] if a.only else ["off", "stock", "flat"]
    res = {m: time_mode(a.hw, a.batch, a.length, m, a.steps, a.warmup) for m in modes}
    print(json.dumps({"tool": "bench_amp_step", "hw": a.hw, "batch": a.batch, "length": a.length, "steps": a.steps,
                      "device": torch.cuda.get_device_name(0), **res}))


if __name__ == "__main__":
    main()
