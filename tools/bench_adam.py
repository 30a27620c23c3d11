"""One ``cer_adam_flat`` launch vs one ``torch.optim.Adam.step()`` (foreach, the GPU default) on the trainable parameters
of the benchmark's released-encoder model (``bench.py --release 4``: the whole IR-50 plus the LFAN tail; at ``--hw 224`` the
IR-50 output layer alone is a 205 M-parameter Linear, at the reference's 40x40 crop 6.6 M).

    python tools/bench_adam.py [--release 4] [--hw 224] [--iters 50]

Both optimisers see the same parameters and gradients; each time is the mean over ``--iters`` calls between two HIP
events after warm-up.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

sys.modules.setdefault("triton", None)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def released_params(release, hw=224, length=32):
    """The trainable parameters bench.py's LFAN has after ``--release`` (same release steps)."""
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.lfan import LFAN
    from feature_vs_text_compound_emotion_amd.parameter_control import ResnetParamControl
    mods = ["video", "vggish", "bert"]
    model = LFAN(backbone_settings={}, output_dim=7, task="CLASSIFICATION", modality=mods, example_length=length,
                 kernel_size=5, tcn_channel=synth.TCN_CHANNELS, root_dir="", device="cuda", head_hw=hw // 8)
    model.init(load_backbone=False)
    model = model.cuda()
    if release:
        pc = ResnetParamControl(trainer=None, release_count=min(release, 3))
        for _ in range(min(release, 3)):
            pc.release_param(model.spatial)
        if release == 4:
            bb = model.spatial["visual"].backbone
            for part in (bb.input_layer, bb.body, bb.output_layer):
                for p in part.parameters():
                    p.requires_grad = True
    return model


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--release", type=int, default=4, choices=[0, 1, 2, 3, 4])
    ap.add_argument("--hw", type=int, default=224, help="frame size: 224 (bench.py's default) or 40 (reference crop)")
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    from feature_vs_text_compound_emotion_amd import ops
    from feature_vs_text_compound_emotion_amd.data_parallel import ClipDataParallel, FlatAdam
    model = released_params(a.release, hw=a.hw)
    ddp = ClipDataParallel(model, world_size=1, broadcast=False)
    flat = FlatAdam(ddp, weight_decay=1e-4)
    n = sum(p.numel() for p in ddp.params)
    g = torch.Generator(device="cuda").manual_seed(0)
    ddp.flat.normal_(generator=g)                         # p.grad of every trainable parameter is a view into it
    ref_params = [p.detach().clone().requires_grad_(True) for p in ddp.params]
    for r, p in zip(ref_params, ddp.params):
        r.grad = p.grad.clone()
    ref = torch.optim.Adam(ref_params, weight_decay=1e-4)
    # one step each, compared before timing
    flat.step()
    ref.step()
    diff = max((p - r).abs().max().item() for p, r in zip(ddp.params, ref_params))
    equal = all(torch.equal(p, r) for p, r in zip(ddp.params, ref_params))
    hp = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4, amsgrad=False)
    kernel_ms = timed(lambda: ops.adam_flat(flat.flat_param, ddp.flat, flat.exp_avg, flat.exp_avg_sq, None, 1e-3, 2, **hp),
                      a.iters)
    flat_ms = timed(flat.step, a.iters)
    torch_ms = timed(ref.step, a.iters)
    gbps = 28.0 * flat.flat_param.numel() / (kernel_ms * 1e-3) / 1e9
    print(json.dumps({"release": a.release, "hw": a.hw, "params": n, "cer_adam_flat_ms": round(kernel_ms, 4),
                      "FlatAdam_step_ms": round(flat_ms, 4), "torch_adam_step_ms": round(torch_ms, 4),
                      "speedup": round(torch_ms / kernel_ms, 2), "kernel_GBps_at_28B": round(gbps, 1),
                      "first_step_max_abs_diff": diff, "first_step_bit_identical": equal}))


if __name__ == "__main__":
    main()
