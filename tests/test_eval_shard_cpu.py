"""Sharded evaluation (``DeviceEvalMixin.eval_shard``) on the host path: two gloo ranks on the CPU, a small deterministic
torch model.  Rank r evaluates the videos at loader positions p % world == r; the per-video logits are gathered back into
loader order and scored once, so every rank returns exactly what one process returns.  The regression task goes through
the same loop with a frame-wise one-column stub and fractional float labels."""
import datetime
import socket

import numpy as np
import torch
import torch.multiprocessing as mp

N_CLS = 5
WINDOW, HOP = 8, 5
# (trial id, frames, label): uneven shards over two ranks, videos shorter than, equal to and longer than the window,
# and a trial id that comes back (the later video wins, as in one process)
VIDEOS = [("a", 8, 1), ("b", 21, 3), ("c", 5, 0), ("a", 13, 2), ("d", 8, 4), ("e", 30, 3), ("f", 11, 1)]


class StubModel(torch.nn.Module):
    """[1, 1, L, 16] features -> [1, L, N_CLS] logits; frame-wise, so windows are exact."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        self.w = torch.nn.Parameter(torch.randn(16, N_CLS, generator=g))

    def forward(self, X):
        x = X["vggish"]
        return (x[:, 0] @ self.w).contiguous()


class ScaleModel(torch.nn.Module):
    """[1, 1, L, 16] features -> 0.5 * (the first feature) [1, L, 1]; frame-wise, so windows are exact."""

    def __init__(self):
        super().__init__()
        self.a = torch.nn.Parameter(torch.tensor(0.5))

    def forward(self, X):
        return (X["vggish"][:, 0, :, :1] * self.a).contiguous()


def _loader(task=None):
    """``task`` = "REGRESSION": the same videos with fractional labels in (-1, 1) under the regression label key.  The
    5-frame video stays: the host path forwards a video shorter than the window whole, and [1, 5, 1] labels pass."""
    g = torch.Generator().manual_seed(11)
    out = []
    for trial, n, label in VIDEOS:
        X = {"vggish": torch.randn(1, 1, n, 16, generator=g)}
        if task == "REGRESSION":
            X["continuous_label"] = torch.rand(1, n, 1, generator=g) * 2.0 - 1.0
        else:
            X["EXPR_continuous_label"] = torch.full((1, n, 1), float(label))
        out.append((X, [trial], [n], [np.arange(n)]))
    return out


class RecordingLoader:
    """The loader of every rank yields every video; the trainer must skip the other ranks' videos itself."""

    def __init__(self, items):
        self.items, self.seen = items, []

    def __iter__(self):
        for p, item in enumerate(self.items):
            yield item
            self.seen.append(p)


def _trainer(shard, task=None):
    from feature_vs_text_compound_emotion_amd.trainer import Trainer
    model = ScaleModel() if task == "REGRESSION" else StubModel()
    tr = Trainer(model, device="cpu", window_length=WINDOW, hop_length=HOP, number_classes=N_CLS, task=task)
    tr.eval_shard = shard
    return tr


def _forwarded(tr, loader):
    """Frame counts of the forwards ``tr.inference`` runs."""
    seen = []
    hook = tr.model.register_forward_pre_hook(lambda mod, args: seen.append(args[0]["vggish"].shape[2]))
    try:
        tr.inference(loader)
    finally:
        hook.remove()
    return seen


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out, task=None):
    import sys
    sys.modules.setdefault("triton", None)
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=120))
    try:
        tr = _trainer(True, task)
        loader = RecordingLoader(_loader(task))
        perf, pv = tr.inference(loader)
        frames = _forwarded(_trainer(True, task), _loader(task))
        perf_off, pv_off = _trainer(False, task).inference(_loader(task))      # eval_shard off: every rank evaluates everything
        out[rank] = (perf, pv, frames, perf_off, pv_off, loader.seen)
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _same(a, b):
    if isinstance(a, dict):
        assert list(a) == list(b)
        for k in a:
            _same(a[k], b[k])
    elif a is None:
        assert b is None
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b)), (a, b)


def _same_videos(a, b, field="logits"):
    assert list(a) == list(b)
    for k in a:
        assert list(a[k]) == list(b[k]) == ["labels", field]
        assert np.array_equal(a[k]["labels"], b[k]["labels"]) and np.array_equal(a[k][field], b[k][field])


def _same_regression_scores(a, b):
    assert list(a) == list(b)
    for k in a:
        for m in ("rmse", "ccc"):
            assert a[k][m] == b[k][m], (k, m)
        assert a[k]["pcc"][0] == b[k]["pcc"][0] and np.array_equal(a[k]["pcc"][1], b[k]["pcc"][1], equal_nan=True), k


def _frames_of(positions):
    """Forward lengths the stub sees for the videos at ``positions`` (longer videos: one forward per window)."""
    from feature_vs_text_compound_emotion_amd.trainer import windowing
    out = []
    for p in positions:
        n = VIDEOS[p][1]
        out += [WINDOW] * len(windowing(np.arange(n), WINDOW, HOP)) if n > WINDOW else [n]
    return out


def test_two_ranks_shard_by_position_and_return_the_single_process_result():
    world, port = 2, _free_port()
    perf1, pv1 = _trainer(False).inference(_loader())
    assert list(pv1) == ["a", "b", "c", "d", "e", "f"] and pv1["a"]["labels"].shape == (13,)   # the later "a" wins
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        out = mgr.dict()
        mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
        res = dict(out)
    for rank in range(world):
        perf, pv, frames, perf_off, pv_off, seen = res[rank]
        assert seen == list(range(len(VIDEOS)))                               # the full loader on every rank ...
        assert frames == _frames_of([p for p in range(len(VIDEOS)) if p % world == rank])   # ... forwards of its shard only
        _same(perf, perf1)
        _same_videos(pv, pv1)
        _same(perf_off, perf1)
        _same_videos(pv_off, pv1)


def test_two_ranks_score_the_regression_task_like_a_single_process():
    world, port = 2, _free_port()
    perf1, pv1 = _trainer(False, "REGRESSION").inference(_loader("REGRESSION"))
    assert list(pv1) == ["a", "b", "c", "d", "e", "f"] and list(perf1) == list(pv1) + ["overall"]
    assert pv1["a"]["labels"].shape == (13,) and pv1["a"]["labels"].dtype == np.float32            # the later "a" wins
    assert np.any(pv1["b"]["labels"] != np.round(pv1["b"]["labels"]))                               # fractional labels survive
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        out = mgr.dict()
        mp.spawn(_worker, args=(world, port, out, "REGRESSION"), nprocs=world, join=True)
        res = dict(out)
    for rank in range(world):
        perf, pv, frames, perf_off, pv_off, seen = res[rank]
        assert seen == list(range(len(VIDEOS)))
        assert frames == _frames_of([p for p in range(len(VIDEOS)) if p % world == rank])
        _same_regression_scores(perf, perf1)
        _same_videos(pv, pv1, field="outputs")
        _same_regression_scores(perf_off, perf1)
        _same_videos(pv_off, pv1, field="outputs")


def test_eval_shard_without_a_process_group_changes_nothing():
    import torch.distributed as dist
    assert not dist.is_initialized()
    perf1, pv1 = _trainer(False).inference(_loader())
    perf2, pv2 = _trainer(True).inference(_loader())
    _same(perf2, perf1)
    _same_videos(pv2, pv1)
    assert _forwarded(_trainer(True), _loader()) == _frames_of(range(len(VIDEOS)))
