"""The regression task without a GPU: the numpy scores against the reference's recorded ones, the moment fold behind the
device accumulator, sharded scoring over two gloo ranks, and the trainer's two label conventions on a stub model.

The float64 restatement (``regression_ref.py``) is itself pinned here to the fixture that
``tools/gen_golden_regression.py`` recorded from the reference."""
import datetime
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import regression_ref as rr
from helpers import golden


# ---------------------------------------------------------------------------------------------------- restatement, mirror
def test_float64_restatement_equals_the_reference_records():
    g = golden("regression_ccc.npz")
    for k, shape in enumerate(g["loss_shapes"].tolist()):
        gold, pred = g[f"gold{k}"], g[f"pred{k}"]
        assert gold.dtype == np.float32 and gold.shape == tuple(shape)
        loss, grad = rr.ccc_loss64(gold, pred)
        assert abs(loss - float(g[f"loss64_{k}"])) <= 4e-16 * max(1.0, abs(loss))
        assert np.abs(grad - g[f"grad64_{k}"]).max() <= 1e-15
        ref32 = rr.ccc_loss_torch(torch.from_numpy(gold), torch.from_numpy(pred)).item()
        assert abs(ref32 - float(g[f"loss32_{k}"])) <= 2 * rr.spacing32(ref32)     # the 1e-50 the restatement omits is 0 in fp32


@pytest.mark.parametrize("shape", rr.LOSS_SHAPES)
def test_closed_form_gradient_equals_float64_autograd(shape):
    gold, pred = rr.loss_case(shape)
    p = torch.tensor(pred, dtype=torch.float64, requires_grad=True)
    loss = rr.ccc_loss_torch(torch.tensor(gold, dtype=torch.float64), p)
    loss.backward()
    mine, grad = rr.ccc_loss64(gold, pred)
    assert abs(mine - loss.item()) <= 4e-16 * max(1.0, abs(mine))
    assert np.abs(grad - p.grad.numpy()).max() <= 1e-15


def test_numpy_scores_equal_the_reference_records():
    from feature_vs_text_compound_emotion_amd import metrics
    g = golden("regression_ccc.npz")
    n = int(g["n_videos"])
    per_video = {f"trial{v}": {"outputs": g[f"vid_pred{v}"], "labels": g[f"vid_label{v}"]} for v in range(n)}
    perf = metrics.compute_regression_perf(per_video)
    assert list(perf) == [f"trial{v}" for v in range(n)] + ["overall"]
    want = {f"trial{v}": g[f"vid_scores{v}"] for v in range(n)}
    want["overall"] = g["overall_scores"]
    for t, (rmse, r, p_value, ccc) in want.items():
        assert set(perf[t]) == {"rmse", "pcc", "ccc"} and len(perf[t]["pcc"]) == 2
        assert abs(perf[t]["rmse"] - rmse) <= 1e-12 and abs(perf[t]["pcc"][0] - r) <= 1e-12 and abs(perf[t]["ccc"] - ccc) <= 1e-12
        try:
            import scipy  # noqa: F401
        except ImportError:
            assert np.isnan(perf[t]["pcc"][1])
        else:
            assert abs(perf[t]["pcc"][1] - p_value) <= 1e-12


def test_moment_fold_equals_the_concatenated_computation():
    from feature_vs_text_compound_emotion_amd import metrics
    vids = rr.videos()
    rows = [np.append(rr.moments64(p, l)[0], 0.0) for _, p, l in vids]
    cat_p, cat_l = np.concatenate([p for _, p, _ in vids]), np.concatenate([l for _, _, l in vids])
    want, mass = rr.moments64(cat_p, cat_l)
    got = metrics.fold_moments(rows)
    assert got[0] == want[0] == cat_p.size and got[7] == 0.0
    assert np.all(np.abs(got[:7] - want) <= 1e-14 * np.maximum(mass, 1.0)), (got[:7] - want)
    direct = metrics.regression_scores(cat_p, cat_l)
    folded = metrics.scores_from_moments(got)
    for _, p, l in vids:                                  # a row alone gives the video's own scores
        a, b = metrics.scores_from_moments(np.append(rr.moments64(p, l)[0], 0.0)), metrics.regression_scores(p, l)
        assert abs(a["rmse"] - b["rmse"]) <= 1e-14 and abs(a["pcc"][0] - b["pcc"][0]) <= 1e-14 and abs(a["ccc"] - b["ccc"]) <= 1e-14
        if not np.isnan(b["pcc"][1]):
            assert abs(a["pcc"][1] - b["pcc"][1]) <= 1e-9
    assert abs(folded["rmse"] - direct["rmse"]) <= 1e-15 and abs(folded["pcc"][0] - direct["pcc"][0]) <= 1e-15
    assert abs(folded["ccc"] - direct["ccc"]) <= 1e-15


# ---------------------------------------------------------------------------------------------------- sharded scoring
def _filled(positions):
    """An accumulator holding the synthetic moment rows of the videos at ``positions`` (one ``add``'s worth each)."""
    from feature_vs_text_compound_emotion_amd.eval_device import DeviceRegressionAccumulator
    acc = DeviceRegressionAccumulator(device="cpu")
    vids = rr.videos()
    for pos in positions:
        trial, p, l = vids[pos]
        acc.rows.append(torch.from_numpy(np.append(rr.moments64(p, l)[0], 0.0)).reshape(1, 8))
        acc.keys.append((pos, trial))
    return acc


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    import sys
    sys.modules.setdefault("triton", None)
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=120))
    try:
        acc = _filled([p for p in range(len(rr.VIDEO_FRAMES)) if p % world == rank])
        acc.merge_ranks()
        out[rank] = acc.compute()
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        for m in ("rmse", "ccc"):
            assert a[k][m] == b[k][m], (k, m)
        assert a[k]["pcc"][0] == b[k]["pcc"][0] and np.array_equal(a[k]["pcc"][1], b[k]["pcc"][1], equal_nan=True), k


def test_two_ranks_report_the_single_rank_scores_exactly():
    world, port = 2, _free_port()
    single = _filled(range(len(rr.VIDEO_FRAMES))).compute()
    assert list(single) == [t for t, _, _ in rr.videos()] + ["overall"]
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        out = mgr.dict()
        mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
        res = dict(out)
    for rank in range(world):
        _same(res[rank], single)


# ---------------------------------------------------------------------------------------------------- trainer on a stub
class Scale(torch.nn.Module):
    """[B, 1, L, 4] features -> a * (first ``d`` features) [B, L, d]; frame-wise, so windows are exact."""

    def __init__(self, a=0.2, d=1):
        super().__init__()
        self.a, self.d = torch.nn.Parameter(torch.tensor(float(a))), d

    def forward(self, X):
        return (X["vggish"][:, 0, :, :self.d] * self.a).contiguous()


def _video(n, seed, trial):
    x = torch.randn(1, 1, n, 4, generator=torch.Generator().manual_seed(seed))
    return ({"vggish": x, "continuous_label": x[:, 0, :, :1].clone()}, [trial], [n], [np.arange(n)])


def test_regression_train_step_hands_the_criterion_float_labels_in_three_dimensions():
    from feature_vs_text_compound_emotion_amd.lfan import ccc_loss
    from feature_vs_text_compound_emotion_amd.trainer import Trainer
    seen = []

    def criterion(gold, pred):
        seen.append((gold.detach().clone(), pred.detach().clone()))
        return ((gold - pred) ** 2).mean()

    model = Scale(0.2, d=2)
    tr = Trainer(model, optimizer=torch.optim.SGD(model.parameters(), lr=0.1), criterion=criterion, device="cpu", task="regression",
                 train_batch_size=3)
    assert tr.task == "REGRESSION"
    assert Trainer(Scale(), device="cpu", task="REGRESSION").criterion is ccc_loss
    x = torch.randn(3, 1, 5, 4, generator=torch.Generator().manual_seed(1))
    labels = x[:, 0, :, :2] * 0.5 + 0.123                       # fractional: .long() would destroy them
    loss = tr.train_step({"vggish": x, "continuous_label": labels.clone()})
    (gold, pred), = seen
    assert gold.dtype == torch.float32 and tuple(gold.shape) == tuple(pred.shape) == (3, 5, 2)
    assert torch.equal(gold, labels) and torch.equal(pred, x[:, 0, :, :2] * 0.2)
    assert loss.item() == ((gold - pred) ** 2).mean().item() and model.a.item() != pytest.approx(0.2)
    with pytest.raises(AssertionError):                         # outputs and labels must have one shape
        tr.train_step({"vggish": x, "continuous_label": labels[:, :, :1].clone()})
    with pytest.raises(ValueError, match="task"):
        Trainer(Scale(), device="cpu", task="RANKING")


def test_default_task_still_hands_the_criterion_flat_long_labels():
    from feature_vs_text_compound_emotion_amd.lfan import cross_entropy_loss
    from feature_vs_text_compound_emotion_amd.trainer import Trainer
    seen = []

    def criterion(outputs, labels):
        seen.append((outputs.detach().clone(), labels.clone()))
        return outputs.sum() * 0.0

    model = Scale(0.2, d=4)
    tr = Trainer(model, optimizer=torch.optim.SGD(model.parameters(), lr=0.1), criterion=criterion, device="cpu",
                 number_classes=4, train_batch_size=3)
    assert tr.task == "CLASSIFICATION" and Trainer(Scale(), device="cpu").criterion is cross_entropy_loss
    x = torch.randn(3, 1, 5, 4, generator=torch.Generator().manual_seed(2))
    labels = torch.tensor([[0.0, 1.0, 2.9, 3.0, 1.5]] * 3).view(3, 5, 1)
    tr.train_step({"vggish": x, "EXPR_continuous_label": labels})
    (outputs, flat), = seen
    assert tuple(outputs.shape) == (15, 4) and flat.dtype == torch.int64 and flat.tolist() == [0, 1, 2, 3, 1] * 3
    tr.set_args({"task": "REGRESSION"})                         # the argparse namespace decides, as for the window rule
    assert tr.task == "REGRESSION" and tr.criterion is criterion


def test_host_inference_scores_windowed_videos_like_the_numpy_mirror():
    from feature_vs_text_compound_emotion_amd import metrics
    from feature_vs_text_compound_emotion_amd.trainer import Trainer
    loader = [_video(8, 1, "a"), _video(21, 2, "b"), _video(5, 3, "c")]
    tr = Trainer(Scale(0.5), device="cpu", window_length=8, hop_length=5, task="REGRESSION")
    perf, per_video = tr.inference(loader)
    assert list(per_video) == ["a", "b", "c"] and list(perf) == ["a", "b", "c", "overall"]
    for (X, (trial,), _, _) in loader:
        lab = X["continuous_label"].reshape(-1).numpy()
        assert per_video[trial]["labels"].dtype == np.float32 and np.array_equal(per_video[trial]["labels"], lab)
        assert np.allclose(per_video[trial]["outputs"], 0.5 * lab, atol=1e-7)          # windows of a frame-wise model
        assert perf[trial]["pcc"][0] == pytest.approx(1.0, abs=1e-12)
    want = metrics.compute_regression_perf(per_video)
    assert perf["overall"]["ccc"] == want["overall"]["ccc"] and perf["b"]["rmse"] == want["b"]["rmse"]
    assert 0.7 < perf["overall"]["ccc"] < 0.8              # 2a / (1 + a^2) = 0.8 at a = 0.5, less the mean and 1 / n terms
    with pytest.raises(ValueError, match="needs a GPU"):
        tr.inference(loader, aggregate="device")


def test_optimize_keeps_the_epoch_with_the_highest_overall_ccc(monkeypatch):
    from feature_vs_text_compound_emotion_amd.trainer import Trainer
    model = Scale(0.2)
    tr = Trainer(model, optimizer=torch.optim.SGD(model.parameters(), lr=0.1), device="cpu", window_length=8, hop_length=5,
                 task="REGRESSION", max_epoch=3, criterion=lambda gold, pred: ((gold - pred) ** 2).mean())
    schedule = iter([0.5, 1.0, 0.7])                            # overall ccc ~ 2a / (1 + a^2): 0.38 -> 0.8, 1.0, 0.94

    def epoch(dataloader=None):
        with torch.no_grad():
            model.a.fill_(next(schedule))
        return 0.0
    monkeypatch.setattr(tr, "train_one_epoch", epoch)
    loaders = {"train": [], "valid": [_video(8, 1, "a"), _video(13, 2, "b")], "test": [_video(9, 4, "t")]}
    hist = tr.optimize(loaders)
    ccc = [p["overall"]["ccc"] for p in hist["valid"]]
    assert len(ccc) == 4 and int(np.argmax(ccc)) - 1 == hist["best_epoch"] == 1
    assert model.a.item() == 1.0 and hist["test"]["overall"]["ccc"] == pytest.approx(8 / 9, abs=1e-7)   # (n - 1) / n
    assert list(hist["test_logits"]["t"]) == ["labels", "outputs"]
