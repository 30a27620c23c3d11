"""The regression task on the device against its float64 restatement (``regression_ref.py``): the tanh output, the CCC loss
and its gradient, the per-video moments behind RMSE / Pearson's r / Lin's CCC, and the models / trainer on top of them.

The kernels compute in double on float32 data, so the bars are roundings: one float32 spacing for anything stored as
float32, the any-order summation bound for the float64 moments."""
import numpy as np
import pytest
import torch

import regression_ref as rr
from helpers import golden

pytestmark = pytest.mark.gpu

ENTRY_POINTS = ("cer_tanh_fwd", "cer_tanh_bwd", "cer_ccc_loss", "cer_regression_moments")


def _ops():
    from feature_vs_text_compound_emotion_amd import ops
    return ops


def _within_one_spacing(got, want64, what=""):
    got, want64 = np.asarray(got, dtype=np.float64), np.asarray(want64, dtype=np.float64)
    assert got.shape == want64.shape, (got.shape, want64.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want64)), what
    ok = ~np.isnan(want64)
    excess = np.abs(got[ok] - want64[ok]) - rr.spacing32(want64[ok])
    assert excess.size == 0 or excess.max() <= 0.0, (what, float(excess.max()))


# ---------------------------------------------------------------------------------------------------- tanh
@pytest.mark.parametrize("n", rr.TANH_SIZES)
def test_tanh_forward_and_backward_are_correctly_rounded(n):
    ops = _ops()
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * 3.0).astype(np.float32)
    edges = np.asarray(rr.TANH_EDGES, dtype=np.float32)
    x[:min(n, edges.size)] = edges[:min(n, edges.size)]
    xd = torch.from_numpy(x).cuda()
    y = ops.tanh_fwd(xd)
    assert y.dtype == torch.float32 and y.shape == xd.shape
    with np.errstate(invalid="ignore"):
        _within_one_spacing(y.cpu().numpy(), rr.tanh64(x), "tanh")
    dy = rng.standard_normal(n).astype(np.float32)
    dx = ops.tanh_bwd(torch.from_numpy(dy).cuda(), y)
    y64 = y.cpu().numpy().astype(np.float64)
    _within_one_spacing(dx.cpu().numpy(), dy.astype(np.float64) * (1.0 - y64 * y64), "tanh backward")


def test_tanh_edge_values_are_exact():
    ops = _ops()
    x = torch.tensor(rr.TANH_EDGES + [25.0, -1e4, 3e38], dtype=torch.float32).cuda().view(1, -1, 1)
    y = ops.tanh_fwd(x).cpu().view(-1)
    want = [0.0, 1e-30, -1e-30, 1.0, -1.0, 1.0, -1.0, float("nan"), 1.0, -1.0, 1.0]
    assert torch.equal(y[:7], torch.tensor(want[:7], dtype=torch.float32)) and torch.isnan(y[7])
    assert y[8:].tolist() == want[8:]
    assert torch.signbit(ops.tanh_fwd(torch.tensor([-0.0]).cuda())).item()


# ---------------------------------------------------------------------------------------------------- the loss
@pytest.mark.parametrize("shape", rr.LOSS_SHAPES)
def test_ccc_loss_and_gradient_equal_the_float64_restatement(shape):
    ops = _ops()
    gold, pred = rr.loss_case(shape)
    gd, pd = torch.from_numpy(gold.copy()).cuda(), torch.from_numpy(pred.copy()).cuda()
    loss, dp = ops.ccc_loss(gd, pd)
    want, grad = rr.ccc_loss64(gold, pred)
    assert loss.shape == () and loss.dtype == torch.float32 and dp.shape == pd.shape
    _within_one_spacing(loss.item(), want, "loss")
    _within_one_spacing(dp.cpu().numpy(), grad, "gradient")
    loss2, dp2 = ops.ccc_loss(gd, pd)                             # no atomics: the same bits
    assert torch.equal(loss, loss2) and torch.equal(dp, dp2)
    loss3, none = ops.ccc_loss(gd, pd, want_grad=False)
    assert none is None and torch.equal(loss3, loss)


@pytest.mark.parametrize("name", ["L=1", "gold=pred=c", "gold=c"])
def test_degenerate_columns_are_nan_where_the_restatement_is_and_nowhere_else(name):
    ops = _ops()
    gold, pred, col = rr.degenerate_cases()[name]
    loss, dp = ops.ccc_loss(torch.from_numpy(gold).cuda(), torch.from_numpy(pred).cuda())
    want, grad = rr.ccc_loss64(gold, pred)
    got = dp.cpu().numpy()
    assert np.isnan(loss.item()) == np.isnan(want) and np.array_equal(np.isnan(got), np.isnan(grad))
    if name == "L=1":
        assert np.isnan(loss.item()) and np.isnan(got).all()
    elif name == "gold=pred=c":                                   # NaN stays in that column's gradient (and the loss)
        mask = np.zeros(gold.shape, dtype=bool)
        mask[col[0], :, col[1]] = True
        assert np.isnan(loss.item()) and np.array_equal(np.isnan(got), mask)
        _within_one_spacing(got[~mask], grad[~mask])
    else:                                                         # S = 0 exactly: the column's term is L, its gradient 0
        assert np.isfinite(got).all() and np.isfinite(loss.item())
        assert not got[col[0], :, col[1]].any()
        b, l, d = gold.shape
        others = [(i, j) for i in range(b) for j in range(d) if (i, j) != col]
        terms = sum(rr.ccc_loss64(gold[i:i + 1, :, j:j + 1], pred[i:i + 1, :, j:j + 1])[0] * l for i, j in others)
        _within_one_spacing(loss.item(), (terms + l) / gold.size)
        _within_one_spacing(got, grad)


def test_loss_equals_the_reference_record_within_the_reference_own_rounding():
    ops = _ops()
    g = golden("regression_ccc.npz")
    for k in range(len(g["loss_shapes"])):
        loss, dp = ops.ccc_loss(torch.from_numpy(g[f"gold{k}"]).cuda(), torch.from_numpy(g[f"pred{k}"]).cuda())
        ref32 = float(g[f"loss32_{k}"])
        assert abs(loss.item() - ref32) <= float(g[f"err32_{k}"]) + rr.spacing32(ref32), (k, loss.item(), ref32)
        _within_one_spacing(dp.cpu().numpy(), g[f"grad64_{k}"], f"gradient {k}")


# ---------------------------------------------------------------------------------------------------- refusals
@pytest.fixture
def launches(monkeypatch):
    """Call counters around the four library entry points; the calls still go through."""
    from feature_vs_text_compound_emotion_amd import _lib
    lib = _lib.load()
    calls = {}
    for name in ENTRY_POINTS:
        fn = getattr(lib, name)
        calls[name] = 0

        def counted(*a, _fn=fn, _name=name):
            calls[_name] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, counted)
    return calls


def test_bad_arguments_are_refused_before_any_launch(launches):
    from feature_vs_text_compound_emotion_amd.eval_device import DeviceRegressionAccumulator
    ops = _ops()
    good = torch.zeros(2, 6, 3).cuda()
    bad = {"cpu": torch.zeros(2, 6, 3), "fp16": good.half(), "shape": torch.zeros(2, 6, 2).cuda(),
           "strided": torch.zeros(2, 3, 6).cuda().transpose(1, 2)}
    assert not bad["strided"].is_contiguous() and bad["strided"].shape == good.shape
    for why, t in bad.items():
        with pytest.raises(ValueError):
            ops.ccc_loss(good, t)
        with pytest.raises(ValueError):
            ops.ccc_loss(t, good)
        with pytest.raises(ValueError):
            ops.tanh_bwd(t, good)
        if why != "shape":
            with pytest.raises(ValueError):
                ops.tanh_fwd(t)
            with pytest.raises(ValueError):
                ops.regression_moments(t.reshape(-1) if why != "strided" else torch.zeros(72).cuda()[::2], good.reshape(-1), [0, 36])
    with pytest.raises(ValueError):
        ops.ccc_loss(good[0], good[0])                              # [L, D]: not three-dimensional
    flat = torch.zeros(10).cuda()
    for off in ([0, 1, 10], [0, 9, 10], [0, 4, 5, 10]):             # a video of one frame
        with pytest.raises(ValueError, match="fewer than 2 frames"):
            DeviceRegressionAccumulator().add(flat, flat, video_offsets=off)
    with pytest.raises(ValueError, match="fewer than 2 frames"):
        DeviceRegressionAccumulator().add(flat[:1], flat[:1])
    with pytest.raises(ValueError, match="ONE output column"):
        DeviceRegressionAccumulator().add(torch.zeros(10, 2).cuda(), flat)
    for off in ([1, 10], [0, 5, 5, 10], [0, 12], [0, 5, 9]):
        with pytest.raises(ValueError, match="video_offsets"):
            DeviceRegressionAccumulator().add(flat, flat, video_offsets=off)
        with pytest.raises(ValueError, match="video_offsets"):
            ops.regression_moments(flat, flat, off)
    assert launches == dict.fromkeys(ENTRY_POINTS, 0)
    acc = DeviceRegressionAccumulator()
    acc.add(torch.arange(10.0).cuda().view(10, 1), torch.arange(10.0).cuda().flip(0), video_offsets=[0, 4, 10])
    assert launches["cer_regression_moments"] == 1 and acc.compute()["overall"]["pcc"][0] == pytest.approx(-1.0, abs=1e-12)


# ---------------------------------------------------------------------------------------------------- autograd
def test_loss_of_tanh_chain_against_float64_autograd_and_under_a_loss_scale():
    """``ccc_loss(gold, TanhFn(x))``.  The float64 chain differs from the device's only through float32 roundings, taken to first
    order: y = tanh(x) is stored within one spacing s_k of tanh64 (the bar above), which moves the loss by at most
    sum |dL/dy_k| s_k and the loss gradient dL/dy_j by at most sum_k |H_jk| s_k (H: the float64 Hessian of the loss in y);
    1 - y_j^2 moves by at most 2 |y_j| s_j; dL/dy and the product are each rounded once to float32 (two spacings of the
    result).  A 1 % allowance covers the second-order terms."""
    from feature_vs_text_compound_emotion_amd.fusion_heads import TanhFn
    from feature_vs_text_compound_emotion_amd.lfan import ccc_loss
    shape = (3, 65, 2)
    gold, _ = rr.loss_case(shape, seed=2)
    x = (np.random.default_rng(12).standard_normal(shape) * 1.5).astype(np.float32)
    want, gx = rr.chain64(gold, x)
    y64 = torch.tanh(torch.tensor(x, dtype=torch.float64))
    g64 = torch.tensor(gold, dtype=torch.float64)
    _, gy = rr.ccc_loss64(gold, y64.numpy())
    hess = torch.autograd.functional.hessian(lambda y: rr.ccc_loss_torch(g64, y), y64).reshape(x.size, x.size).abs().numpy()
    s = rr.spacing32(y64.numpy()).reshape(-1)
    yf, gyf = y64.numpy().reshape(-1), gy.reshape(-1)
    tol_loss = 1.01 * float(np.abs(gyf) @ s) + rr.spacing32(want)
    tol_grad = 1.01 * ((hess @ s) * (1.0 - yf * yf) + np.abs(gyf) * 2.0 * np.abs(yf) * s) + 2.0 * rr.spacing32(gx.reshape(-1))

    def run(scale):
        xd = torch.from_numpy(x.copy()).cuda().requires_grad_(True)
        loss = ccc_loss(torch.from_numpy(gold.copy()).cuda(), TanhFn.apply(xd))
        (loss * scale).backward()
        return loss.detach(), xd.grad

    loss, grad = run(1.0)
    assert abs(loss.item() - want) <= tol_loss, (loss.item(), want, tol_loss)
    excess = np.abs(grad.cpu().numpy().reshape(-1).astype(np.float64) - gx.reshape(-1)) - tol_grad
    assert excess.max() <= 0.0, float(excess.max())
    loss_s, grad_s = run(65536.0)
    assert torch.equal(loss_s, loss) and torch.equal(grad_s, grad * 65536.0)
    with torch.autocast("cuda", dtype=torch.float16):                 # --amp: half-precision outputs are cast up
        half = ccc_loss(torch.from_numpy(gold.copy()).cuda(), torch.from_numpy(x.copy()).cuda().half())
    assert half.dtype == torch.float32 and torch.isfinite(half)


# ---------------------------------------------------------------------------------------------------- models
def _lfan(mods, sd, length, output_dim, task):
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.lfan import LFAN
    m = LFAN(backbone_settings={}, output_dim=output_dim, task=task, modality=mods, example_length=length, kernel_size=5,
             tcn_channel=synth.TCN_CHANNELS, modal_dim=32, num_heads=2, root_dir="", device="cuda")
    m.init(load_backbone=False)
    m.load_state_dict(sd, strict=True)
    return m.cuda()


LOGIT_BAR = 1e-4        # test_tail_gpu.py's bar for this model's logits against the oracle (fp32, other summation order)


@pytest.mark.parametrize("output_dim", [1, 2])
def test_lfan_regression_output_is_tanh_of_the_oracle_logits(output_dim):
    from feature_vs_text_compound_emotion_amd import synth
    from oracle.lfan import lfan_forward
    mods = ["vggish", "bert"]
    sd = synth.lfan_state_dict(mods, n_cls=output_dim, seed=31)
    x, _ = synth.make_clip_batch(mods, 2, 8, seed=32)
    with torch.no_grad():
        want = rr.tanh64(lfan_forward(x, sd, mods).numpy())
        out = _lfan(mods, sd, 8, output_dim, "REGRESSION").eval()({k: v.cuda() for k, v in x.items()})
    assert tuple(out.shape) == (2, 8, output_dim) and out.dtype == torch.float32
    excess = np.abs(out.cpu().numpy() - want) - (LOGIT_BAR + rr.spacing32(want))      # tanh is 1-Lipschitz
    assert excess.max() <= 0.0, float(excess.max())


@pytest.mark.parametrize("name", ["CAN", "JMT"])
def test_tail_models_regression_output_is_tanh_of_their_classification_output(name):
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.fusion_heads import CAN, JMT
    mods = ["video", "vggish"]
    spec, alias = synth.can_spec(mods, n_cls=1) if name == "CAN" else synth.jmt_spec(mods, name, n_cls=1)
    sd = synth.make_state_dict(spec, alias, seed=41)
    x, _ = synth.make_clip_batch(mods, 2, 8, hw=40, seed=42)
    outs = {}
    for task in ("CLASSIFICATION", "REGRESSION"):
        kw = dict(task=task, modalities=mods, tcn_settings=synth.TCN_SETTINGS, backbone_settings={}, output_dim=1, root_dir="",
                  device="cuda", load_backbone=False)
        m = CAN(**kw) if name == "CAN" else JMT(model_name=name, **kw)
        m.load_state_dict(sd, strict=True)
        with torch.no_grad():
            outs[task] = m.cuda().eval()({k: v.cuda() for k, v in x.items()}).cpu().numpy()
    assert outs["REGRESSION"].shape == (2, 8, 1)
    _within_one_spacing(outs["REGRESSION"], rr.tanh64(outs["CLASSIFICATION"]), name)


# ---------------------------------------------------------------------------------------------------- the accumulator
@pytest.mark.parametrize("mode", ["per_video", "two_adds", "one_add"])
def test_moments_and_scores_equal_numpy_float64(mode):
    from feature_vs_text_compound_emotion_amd import metrics
    from feature_vs_text_compound_emotion_amd.eval_device import DeviceRegressionAccumulator
    vids = rr.videos()
    assert [len(p) for _, p, _ in vids] == rr.VIDEO_FRAMES
    for _, p, l in vids:                                              # a condition on the inputs: no vanishing variance
        assert p.astype(np.float64).var(ddof=1) >= 0.05 and l.astype(np.float64).var(ddof=1) >= 0.05
    groups = {"per_video": [[i] for i in range(len(vids))], "two_adds": [[0, 1, 2], [3, 4, 5, 6, 7]],
              "one_add": [list(range(len(vids)))]}[mode]
    acc = DeviceRegressionAccumulator()
    for grp in groups:
        p = torch.from_numpy(np.concatenate([vids[i][1] for i in grp])).cuda().view(-1, 1)
        l = torch.from_numpy(np.concatenate([vids[i][2] for i in grp])).cuda()
        off = np.cumsum([0] + [len(vids[i][1]) for i in grp]).tolist()
        acc.add(p, l, video_offsets=None if len(grp) == 1 else off, keys=[(i, vids[i][0]) for i in grp])
    rows = torch.cat(acc.rows).cpu().numpy()
    assert rows.shape == (len(vids), 8) and rows.dtype == np.float64 and not rows[:, 7].any()
    for row, (_, p, l) in zip(rows, vids):
        want, mass = rr.moments64(p, l)
        assert row[0] == len(p)
        excess = np.abs(row[:7] - want) - rr.moment_bound(len(p), mass)
        assert excess.max() <= 0.0, (len(p), excess)
    got = acc.compute()
    want = metrics.compute_regression_perf({t: {"outputs": p, "labels": l} for t, p, l in vids})
    assert list(got) == list(want) == [t for t, _, _ in vids] + ["overall"]
    for t in want:
        assert abs(got[t]["rmse"] - want[t]["rmse"]) <= 1e-10 and abs(got[t]["ccc"] - want[t]["ccc"]) <= 1e-10, t
        assert abs(got[t]["pcc"][0] - want[t]["pcc"][0]) <= 1e-10, t


# ---------------------------------------------------------------------------------------------------- the trainer
MODS, WINDOW, HOP = ["vggish", "bert"], 8, 5


def test_one_regression_train_step_on_lfan():
    """The loss against the float64 chain on the ORACLE's logits: the device's logits lie within LOGIT_BAR of those, tanh is
    1-Lipschitz and stored within one spacing, so to first order the loss moves by at most
    sum |dL/dy_k| (LOGIT_BAR + spacing(y_k)); one more spacing for the stored loss, 1 % for the second-order terms."""
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.trainer import Trainer
    from oracle.lfan import lfan_forward
    sd = synth.lfan_state_dict(MODS, n_cls=1, seed=51)
    x, _ = synth.make_clip_batch(MODS, 2, WINDOW, seed=52)
    labels = torch.rand(2, WINDOW, 1, generator=torch.Generator().manual_seed(53)) * 2.0 - 1.0
    with torch.no_grad():
        y = rr.tanh64(lfan_forward(x, sd, MODS, train=True).numpy())
    want, gy = rr.ccc_loss64(labels.numpy(), y)
    tol = 1.01 * float((np.abs(gy) * (LOGIT_BAR + rr.spacing32(y))).sum()) + rr.spacing32(want)
    model = _lfan(MODS, sd, WINDOW, 1, "REGRESSION").train()
    for net in model.temporal.values():
        net.dropout = 0.0
    model.fusion.layers.dropout.p = 0.0
    params = [p for p in model.parameters() if p.requires_grad]
    before = [p.detach().clone() for p in params]
    tr = Trainer(model, optimizer=torch.optim.SGD(params, lr=1e-2), device="cuda", window_length=WINDOW, hop_length=HOP,
                 task="REGRESSION", train_batch_size=2)
    loss = tr.train_step({**x, "continuous_label": labels})
    assert abs(loss.item() - want) <= tol, (loss.item(), want, tol)
    moved = [not torch.equal(a, p.detach()) for a, p in zip(before, params)]
    assert all(torch.isfinite(p).all() for p in params) and moved[-1] and sum(moved) >= len(moved) // 2, moved


def _loader(frames, seed=61):
    from feature_vs_text_compound_emotion_amd import synth
    g = torch.Generator().manual_seed(seed)
    out = []
    for v, n in enumerate(frames):
        X = {m: torch.randn(1, 1, n, synth.EMBEDDING_DIM[m], generator=g) for m in MODS}
        X["continuous_label"] = torch.rand(1, n, 1, generator=g) * 2.0 - 1.0
        out.append((X, [f"clip{v}"], [n], [np.arange(n)]))
    return out


def _scores_close(a, b, tol):
    assert list(a) == list(b)
    for t in a:
        assert abs(a[t]["rmse"] - b[t]["rmse"]) <= tol and abs(a[t]["ccc"] - b[t]["ccc"]) <= tol, t
        assert abs(a[t]["pcc"][0] - b[t]["pcc"][0]) <= tol, t


def test_regression_inference_device_scores_equal_the_host_scores():
    """Three videos through a window-8 / hop-5 LFAN, one of exactly one window and two longer (stitched).  With one window per
    forward on both paths the stitched outputs are the same numbers, so the device aggregation must reproduce the host's
    (numpy float64) scores to 1e-10; it must also reproduce the host mirror on its OWN outputs when windows of several
    videos share forwards (``eval_video_batch`` = 2), where the outputs themselves may move by the 1e-5 that
    test_eval_batched_gpu.py grants batched forwards (and rmse, 1-Lipschitz in them, by no more)."""
    from feature_vs_text_compound_emotion_amd import metrics, synth
    from feature_vs_text_compound_emotion_amd.trainer import Trainer
    sd = synth.lfan_state_dict(MODS, n_cls=1, seed=51)
    model = _lfan(MODS, sd, WINDOW, 1, "REGRESSION").eval()
    loader = _loader([8, 21, 13])

    def trainer(video_batch=1, budget=WINDOW):
        tr = Trainer(model, device="cuda", window_length=WINDOW, hop_length=HOP, task="REGRESSION", train_batch_size=1)
        tr.eval_video_batch, tr.eval_frame_budget = video_batch, budget
        return tr
    dev, pv_dev = trainer().inference(loader)
    host, pv_host = trainer().inference(loader, aggregate="host")
    assert list(dev) == ["clip0", "clip1", "clip2", "overall"] and list(pv_dev) == list(pv_host) == ["clip0", "clip1", "clip2"]
    for (X, (trial,), (n,), _) in loader:
        assert pv_dev[trial]["outputs"].shape == (n,) and np.abs(pv_dev[trial]["outputs"]).max() < 1.0
        assert np.array_equal(pv_dev[trial]["labels"], X["continuous_label"].reshape(-1).numpy())
        assert np.array_equal(pv_dev[trial]["outputs"], pv_host[trial]["outputs"]), trial
    _scores_close(dev, host, 1e-10)
    _scores_close(dev, metrics.compute_regression_perf(pv_dev), 1e-10)
    bat, pv_bat = trainer(video_batch=2, budget=3 * WINDOW).inference(loader)
    _scores_close(bat, metrics.compute_regression_perf(pv_bat), 1e-10)
    for trial in pv_dev:
        assert np.abs(pv_bat[trial]["outputs"] - pv_dev[trial]["outputs"]).max() < 1e-5, trial
        assert abs(bat[trial]["rmse"] - dev[trial]["rmse"]) <= 1e-5
    assert abs(bat["overall"]["rmse"] - dev["overall"]["rmse"]) <= 1e-5
    none, pv_none = trainer(video_batch=2, budget=3 * WINDOW).inference(loader, keep_logits=False)
    assert pv_none == {}
    _scores_close(none, bat, 0.0)
