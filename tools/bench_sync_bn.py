"""Cost of synchronised batch statistics (``ClipDataParallel(sync_bn=...)``) on ONE GPU: the LFAN training step (model.train(),
batch-statistics BatchNorm in the frozen encoder and the tail) with ``sync_bn=False`` against ``sync_bn="force"`` on a
single-rank RCCL communicator.  With one rank every collective is an identity, so the difference is the price of the split
kernels plus one latency-bound collective per BatchNorm pass (53 encoder BatchNorm2d + the head BatchNorm1d forwards, 3 tail
forwards and 3 tail backwards per step); what N > 1 ranks add on top needs several GPUs and is not measured here.

    python tools/bench_sync_bn.py [--steps 20] [--warmup 5] [--out results/bench_sync_bn.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.modules.setdefault("triton", None)

MODS = ["video", "vggish", "bert"]


def _model(hw):
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.lfan import LFAN
    sd = synth.lfan_state_dict(MODS, n_cls=7, head_hw=hw // 8, seed=0)
    m = LFAN(backbone_settings={}, output_dim=7, task="CLASSIFICATION", modality=MODS, example_length=8, kernel_size=5,
             tcn_channel=synth.TCN_CHANNELS, root_dir="", device="cuda", head_hw=hw // 8)
    m.init(load_backbone=False)
    m.load_state_dict(sd, strict=True)
    return m.cuda().train()


def _ms_per_step(hw, batch, sync, steps, warmup):
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.data_parallel import ClipDataParallel, FlatNesterovSGD
    from feature_vs_text_compound_emotion_amd.lfan import cross_entropy_loss
    model = _model(hw)
    ddp = ClipDataParallel(model, sync_bn=sync)
    opt = FlatNesterovSGD(ddp, lr=1e-3)
    x, labels = synth.make_clip_batch(MODS, batch, 8, hw=hw, seed=55)
    xd, ld = {k: v.cuda() for k, v in x.items()}, labels.cuda()

    def step():
        ddp.zero_grad()
        loss = cross_entropy_loss(model(dict(xd)), ld)
        loss.backward()
        ddp.all_reduce_gradients()
        opt.step()

    for _ in range(warmup):
        step()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sync_bn needs the GPU")
    os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29531")
    from feature_vs_text_compound_emotion_amd.data_parallel import init_process_group_from_env
    import torch.distributed as dist
    init_process_group_from_env(backend="nccl", single_rank_group=True)
    res = {"gpus": torch.cuda.device_count(), "world": dist.get_world_size(), "steps": args.steps, "configs": []}
    for hw, batch in ((40, 4), (224, 1)):
        off = _ms_per_step(hw, batch, False, args.steps, args.warmup)
        on = _ms_per_step(hw, batch, "force", args.steps, args.warmup)
        res["configs"].append({"hw": hw, "clips": batch, "frames": batch * 8, "ms_sync_off": round(off, 3),
                               "ms_sync_force": round(on, 3), "overhead_ms": round(on - off, 3),
                               "overhead_pct": round(100.0 * (on - off) / off, 1)})
        print(json.dumps(res["configs"][-1]), flush=True)
    dist.destroy_process_group()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
