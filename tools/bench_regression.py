"""``ccc_loss`` forward + backward (``cer_ccc_loss``: two launches, plus the ``dpred * gout`` of the autograd node) vs the same
formula written in torch ops (base/loss_function.py:12-24) with torch autograd, on the same GPU, at the reference's training
window: B = 32, L = 300, D = 1.

    python tools/bench_regression.py [--batch 32] [--length 300] [--dim 1] [--iters 200]

Both see the same float32 gold / pred; each time is the mean over ``--iters`` forward + backward calls between two HIP events
after warm-up.  The loss and gradient of the two are compared once before timing.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

sys.modules.setdefault("triton", None)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def torch_ccc_loss(gold, pred):
    gm, pm = torch.mean(gold, 1, keepdim=True), torch.mean(pred, 1, keepdim=True)
    cov = (gold - gm) * (pred - pm)
    gv, pv = torch.var(gold, 1, keepdim=True, unbiased=True), torch.var(pred, 1, keepdim=True, unbiased=True)
    return torch.mean(1.0 - 2.0 * cov / (gv + pv + (gm - pm) * (gm - pm) + 1e-50))


def timed(fn, iters, warmup=20):
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
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--length", type=int, default=300)
    ap.add_argument("--dim", type=int, default=1)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    from feature_vs_text_compound_emotion_amd.lfan import ccc_loss
    g = torch.Generator(device="cuda").manual_seed(0)
    shape = (a.batch, a.length, a.dim)
    gold = torch.rand(shape, device="cuda", generator=g) * 2.0 - 1.0
    pred = torch.tanh(torch.randn(shape, device="cuda", generator=g)).requires_grad_(True)

    def step(criterion):
        pred.grad = None
        loss = criterion(gold, pred)
        loss.backward()
        return loss

    l_hip = step(ccc_loss).item()
    g_hip = pred.grad.clone()
    l_torch = step(torch_ccc_loss).item()
    g_torch = pred.grad.clone()
    hip_ms = timed(lambda: step(ccc_loss), a.iters)
    torch_ms = timed(lambda: step(torch_ccc_loss), a.iters)
    print(json.dumps({"B": a.batch, "L": a.length, "D": a.dim, "iters": a.iters, "cer_ccc_loss_fwd_bwd_ms": round(hip_ms, 4),
                      "torch_ops_fwd_bwd_ms": round(torch_ms, 4), "speedup": round(torch_ms / hip_ms, 2),
                      "loss_abs_diff": abs(l_hip - l_torch), "grad_max_abs_diff": (g_hip - g_torch).abs().max().item()}))


if __name__ == "__main__":
    main()
