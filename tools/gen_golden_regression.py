"""Records of the reference's regression criterion and scores (base/loss_function.py, base/logger.py).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_regression.py <reference checkout>

Writes tests/golden/regression_ccc.npz (arrays only):

* per loss case ``k``: ``gold{k}`` / ``pred{k}`` float32 [B, L, D]; ``loss32_{k}``: ``CCCLoss()(gold, pred)`` as the reference
  runs it (float32 tensors); ``loss64_{k}`` / ``grad64_{k}``: the same class on the float64 copies of those inputs, and torch
  autograd's gradient with respect to pred; ``err32_{k}`` = |loss32 - loss64|, the reference's own float32 rounding.
* per video ``v``: ``vid_pred{v}`` / ``vid_label{v}`` float64 and ``vid_scores{v}`` = [rmse, r, p_value, ccc] from
  ``ContinuousMetricsCalculator.calculator``; ``overall_scores``: the same on the concatenation (base/logger.py:343-351).

Before writing, the float64 restatement the tests use (tests/regression_ref.py) and the package's numpy mirror
(metrics.regression_scores / compute_regression_perf) are asserted against the reference's results.
"""
import os
import sys

sys.modules["triton"] = None
import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "regression_ccc.npz")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LOSS_CASES = [(1, 2, 1), (2, 64, 1), (3, 65, 2), (2, 300, 1), (5, 8, 3)]
VIDEO_FRAMES = [2, 3, 65, 300]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    from base.logger import ContinuousMetricsCalculator  # the reference's scores
    from base.loss_function import CCCLoss  # the reference's criterion

    import regression_ref as rr
    from feature_vs_text_compound_emotion_amd import metrics

    out = {"loss_shapes": np.asarray(LOSS_CASES, dtype=np.int64)}
    crit = CCCLoss()
    for k, shape in enumerate(LOSS_CASES):
        gold, pred = rr.loss_case(shape, seed=1)
        loss32 = crit(torch.from_numpy(gold.copy()), torch.from_numpy(pred.copy()))
        p64 = torch.from_numpy(pred.astype(np.float64)).requires_grad_(True)
        loss64 = crit(torch.from_numpy(gold.astype(np.float64)), p64)
        loss64.backward()
        mine, grad = rr.ccc_loss64(gold, pred)
        assert abs(mine - loss64.item()) <= 4e-16 * max(1.0, abs(mine)), (shape, mine, loss64.item())
        assert np.abs(grad - p64.grad.numpy()).max() <= 1e-15, (shape, np.abs(grad - p64.grad.numpy()).max())
        out[f"gold{k}"], out[f"pred{k}"] = gold, pred
        out[f"loss32_{k}"] = np.asarray(loss32.item(), dtype=np.float32)
        out[f"loss64_{k}"] = np.asarray(loss64.item(), dtype=np.float64)
        out[f"grad64_{k}"] = p64.grad.numpy().copy()
        out[f"err32_{k}"] = np.asarray(abs(float(loss32.item()) - loss64.item()), dtype=np.float64)
        print(f"loss case {shape}: loss64 {loss64.item():.17g}  |loss32 - loss64| {out[f'err32_{k}']:.3g}")

    calc = ContinuousMetricsCalculator.calculator
    rng = np.random.default_rng(7)
    per_video = {}
    for v, n in enumerate(VIDEO_FRAMES):
        p, l = np.tanh(rng.standard_normal(n)), rng.uniform(-1.0, 1.0, n)
        per_video[f"trial{v}"] = {"outputs": p, "labels": l}

    def reference_scores(p, l):
        r = calc(None, p, l, "pcc")
        return np.array([calc(None, p, l, "rmse"), r[0], r[1], calc(None, p, l, "ccc")], dtype=np.float64)

    mirror = metrics.compute_regression_perf(per_video)
    cat_p = np.concatenate([d["outputs"] for d in per_video.values()])
    cat_l = np.concatenate([d["labels"] for d in per_video.values()])
    wanted = {t: reference_scores(d["outputs"], d["labels"]) for t, d in per_video.items()}
    wanted[metrics.OVERALL] = reference_scores(cat_p, cat_l)
    for t, w in wanted.items():
        m = mirror[t]
        got = np.array([m["rmse"], m["pcc"][0], m["pcc"][1], m["ccc"]])
        assert np.abs(got - w).max() <= 1e-12, (t, got, w)
    for v, (t, d) in enumerate(per_video.items()):
        out[f"vid_pred{v}"], out[f"vid_label{v}"], out[f"vid_scores{v}"] = d["outputs"], d["labels"], wanted[t]
    out["overall_scores"] = wanted[metrics.OVERALL]
    out["n_videos"] = np.asarray(len(VIDEO_FRAMES), dtype=np.int64)
    np.savez(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
