"""Train-step time of LFAN(logmel, vggish) with 0 / 1 / 2 / 3 audio groups of the gradual release (base/parameter_control.py:
58,85-103: embeddings.4, then .2, then .0 of VGGish), at B x L = 32 x 32 and 8 x 32 clips x frames, VGGish in bf16x3 and fp16
(the latter under autocast + GradScaler, like --amp).  Prints one JSON line per configuration.

    python tools/bench_audio_release.py [--steps 10 --warmup 3 --batches 32,8 --modes bf16x3,fp16]

Kernel times per layer (the 1x1 weight gradients are ``conv2d_wgrad_b3s`` launches of shape 4096x12288 / 4096x4096 /
128x4096 over B*L rows; the fused mask / split / bias pass is ``fc_bwd_elem_kernel``):

    rocprofv3 --kernel-trace --stats -d prof_audio_release -- python tools/bench_audio_release.py --steps 3 --warmup 1
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.modules.setdefault("triton", None)

import torch  # noqa: E402

MODS = ["logmel", "vggish"]


def _model(release, precision, length):
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.lfan import LFAN
    from feature_vs_text_compound_emotion_amd.parameter_control import ResnetParamControl
    spec, alias = synth.lfan_spec(MODS, n_cls=7)
    m = LFAN(backbone_settings={}, output_dim=7, task="CLASSIFICATION", modality=MODS, example_length=length, kernel_size=5,
             tcn_channel=synth.TCN_CHANNELS, root_dir="", device="cuda")
    m.init(load_backbone=False)
    m.load_state_dict(synth.make_state_dict(spec, alias, seed=0), strict=True)
    pc = ResnetParamControl(trainer=None)
    for _ in range(release):
        pc.release_param(m.spatial, modalities=("visual", "audio"))
    m.spatial["audio"].backbone.precision = precision
    return m.cuda().train()


def run(release, precision, batch, length, steps, warmup):
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.data_parallel import ClipDataParallel, FlatNesterovSGD
    from feature_vs_text_compound_emotion_amd.lfan import cross_entropy_loss
    m = _model(release, precision, length)
    ddp = ClipDataParallel(m, world_size=1)
    opt = FlatNesterovSGD(ddp, lr=1e-3)
    x, labels = synth.make_clip_batch(MODS, batch, length, seed=1)
    x = {k: v.cuda() for k, v in x.items()}
    labels = labels.cuda()
    scaler = torch.amp.GradScaler("cuda") if precision == "fp16" else None

    def step():
        ddp.zero_grad()
        with torch.autocast("cuda", dtype=torch.float16, enabled=scaler is not None):
            loss = cross_entropy_loss(m(dict(x)), labels)
        (scaler.scale(loss) if scaler is not None else loss).backward()
        ddp.all_reduce_gradients()
        opt.step()

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    n_rel = sum(p.numel() for p in m.spatial["audio"].parameters() if p.requires_grad)
    print(json.dumps({"bench": "audio_release", "released_groups": release, "precision": precision, "batch": batch,
                      "length": length, "released_params": n_rel, "ms_per_step": round(ms, 3), "steps": steps}), flush=True)
    del m, ddp, opt
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="32,8")
    ap.add_argument("--length", type=int, default=32)
    ap.add_argument("--modes", default="bf16x3,fp16")
    ap.add_argument("--releases", default="0,1,2,3")
    a = ap.parse_args()
    for b in [int(v) for v in a.batches.split(",")]:
        for mode in a.modes.split(","):
            for r in [int(v) for v in a.releases.split(",")]:
                run(r, mode, b, a.length, a.steps, a.warmup)


if __name__ == "__main__":
    main()
