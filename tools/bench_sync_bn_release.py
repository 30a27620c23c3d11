"""Cost of synchronised statistics through the RELEASED encoder units (``ClipDataParallel(sync_bn=..., sync_released=True)``)
on ONE GPU, in one process, with HIP events and warm-up, the compared variants alternating repeat by repeat:

* the statistics pass alone: ``ops.bn_rows_moments_large`` (+ the one-block merge) against ``ops.bn_rows_stats`` at the
  released units' row counts -- 1024 frames of 224x224 through the stem / stage 1 (51.4 M x 64), stage 3 (3.2 M x 256) and
  stage 4 (0.8 M x 512).  Both read x once; the goal is <= 1.25x;
* the LFAN training step with release groups 1-3 at 224x224 (1 clip x 32 frames): ``sync_bn=False`` against
  ``sync_bn="force", sync_released=True`` on a single-rank RCCL communicator (every collective an identity, so the difference
  is the split kernels plus one latency-bound collective per BatchNorm pass).  N > 1 ranks are not measured here.

    python tools/bench_sync_bn_release.py [--repeats 5] [--iters 20] [--steps 5] [--out results/bench_sync_bn_release.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.modules.setdefault("triton", None)

MODS = ["video", "vggish", "bert"]
SHAPES = [(1024 * 224 * 224, 64), (1024 * 56 * 56, 256), (1024 * 28 * 28, 512)]


def _time(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def bench_stats(repeats, iters):
    from feature_vs_text_compound_emotion_amd import ops
    out = []
    for r, c in SHAPES:
        x = torch.randn(r, c, device="cuda")
        rm, rv = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
        variants = {"bn_rows_stats": lambda: ops.bn_rows_stats(x, rm, rv),
                    "moments_large": lambda: ops.bn_rows_merge(ops.bn_rows_moments_large(x).unsqueeze(0), rm, rv)}
        for fn in variants.values():      # warm-up
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(repeats):          # alternating repeats
            for k, fn in variants.items():
                ms[k].append(_time(fn, iters))
        best = {k: min(v) for k, v in ms.items()}
        gb = r * c * 4 / 1e9
        row = {"rows": r, "channels": c, "GB": round(gb, 3),
               **{f"ms_{k}": round(v, 4) for k, v in best.items()},
               **{f"TBps_{k}": round(gb / v, 2) for k, v in best.items()},
               "ratio": round(best["moments_large"] / best["bn_rows_stats"], 3)}
        row["goal_1.25x_met"] = row["ratio"] <= 1.25
        print(json.dumps(row), flush=True)
        out.append(row)
        del x
        torch.cuda.empty_cache()
    return out


def _model(hw):
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.lfan import LFAN
    from feature_vs_text_compound_emotion_amd.parameter_control import ResnetParamControl
    sd = synth.lfan_state_dict(MODS, n_cls=7, head_hw=hw // 8, seed=0)
    m = LFAN(backbone_settings={}, output_dim=7, task="CLASSIFICATION", modality=MODS, example_length=32, kernel_size=5,
             tcn_channel=synth.TCN_CHANNELS, root_dir="", device="cuda", head_hw=hw // 8)
    m.init(load_backbone=False)
    m.load_state_dict(sd, strict=True)
    pc = ResnetParamControl(trainer=None)
    for _ in range(3):                     # output layer, stage 4, second half of stage 3
        pc.release_param(m.spatial)
    return m.cuda().train()


def bench_step(repeats, steps, hw=224, clips=1, frames=32):
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.data_parallel import ClipDataParallel, FlatNesterovSGD
    from feature_vs_text_compound_emotion_amd.lfan import cross_entropy_loss
    x, labels = synth.make_clip_batch(MODS, clips, frames, hw=hw, seed=55)
    xd, ld = {k: v.cuda() for k, v in x.items()}, labels.cuda()
    runs = {}
    for name, kw in (("sync_off", dict(sync_bn=False)), ("sync_released", dict(sync_bn="force", sync_released=True))):
        model = _model(hw)
        ddp = ClipDataParallel(model, **kw)
        opt = FlatNesterovSGD(ddp, lr=1e-3)

        def step(model=model, ddp=ddp, opt=opt):
            ddp.zero_grad()
            cross_entropy_loss(model(dict(xd)), ld).backward()
            ddp.all_reduce_gradients()
            opt.step()
        runs[name] = step
        step()                             # warm-up
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(repeats):
        for k, fn in runs.items():
            ms[k].append(_time(fn, steps))
    best = {k: min(v) for k, v in ms.items()}
    row = {"hw": hw, "clips": clips, "frames": clips * frames, "release_groups": 3,
           **{f"ms_{k}": round(v, 2) for k, v in best.items()},
           "overhead_ms": round(best["sync_released"] - best["sync_off"], 2),
           "overhead_pct": round(100.0 * (best["sync_released"] - best["sync_off"]) / best["sync_off"], 2)}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sync_bn_release needs the GPU")
    os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    import torch.distributed as dist
    from feature_vs_text_compound_emotion_amd.data_parallel import init_process_group_from_env
    init_process_group_from_env(backend="nccl", single_rank_group=True)
    res = {"gpus": torch.cuda.device_count(), "world": dist.get_world_size(), "stats": bench_stats(args.repeats, args.iters),
           "step": bench_step(args.repeats, args.steps)}
    dist.destroy_process_group()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
