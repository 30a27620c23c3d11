"""Host loop around the hot path: one optimisation step, whole-video inference, window stitching.

Mirror of the reference's ``Trainer`` for the parts that call the model (trainer.py:315-434
``train_one_epoch``, :436-523 ``inference``, :611-770 ``optimize``, :788-892 ``window_input`` /
``inference_forward_windows``, :894-912 ``windowing``) plus the dataset-side window rule
(base/dataset.py:434-453, which uses ``>`` where the trainer uses ``>=``).

Two ways in:

* ``Trainer(**trainer_kwards)`` takes the keyword dictionary ``experiment.py:153-175`` builds (``models``, ``device``,
  ``model_name``, ``criterion``, ``train_batch_size`` ... -- unknown keys are kept as attributes like
  ``base/trainer.py:21-45,96-115`` does) and answers the calls ``experiment.py:178-214`` makes next: ``set_args``,
  ``post_set_args``, ``set_number_classes``, ``init_optimizer_and_scheduler``, ``optimize``; ``inference(dataloader)`` and
  ``inference_forward_windows(data)`` have the reference's signatures and read the window rule from ``self.args``.
* ``DeviceEvalMixin`` carries only the evaluation side (window stitching and confusion counts on the device, SURVEY.md
  section 8 f3): ``class MyTrainer(DeviceEvalMixin, reference_trainer.Trainer)`` keeps the reference's own fit loop, logging
  and checkpoints and replaces its two evaluation methods.

What differs between the classification and the regression task -- criterion, label handling, output check, accumulator,
per-video entry, scores -- is stated once, in ``_Classification`` / ``_Regression``; the step, the evaluation loop and
``optimize`` read it from ``_task(...)``.

Logging (dllogger), pickled outputs, PerfTracker reports and best-model files stay with the reference's trainer: they are
its control plane, not this path.
"""
import contextlib
import math
from collections import Counter
from types import SimpleNamespace

import numpy as np
import torch

from . import metrics
from .lfan import CLASSIFICATION, REGRESSION, TASKS, ccc_loss, cross_entropy_loss

VIDEO, VGGISH, BERT, LOGMEL = "video", "vggish", "bert", "logmel"
EXPR = "EXPR_continuous_label"
TRAINSET, VALIDSET, TESTSET = "train", "valid", "test"   # constants.py: TRAINSET / VALIDSET / TESTSET


def windowing(x, window_length, hop_length):
    """trainer.py:894-912 (inclusive ``>=``): inference-time windows of a whole video."""
    n = len(x)
    if n >= window_length:
        steps = (n - window_length) // hop_length + 1
        out = [x[i * hop_length:i * hop_length + window_length] for i in range(steps)]
        if out[-1][-1] < n - 1:
            out.append(x[-window_length:])
        return out
    return [x]


def dataset_windowing(x, window_length, hop_length):
    """base/dataset.py:434-453 (strict ``>``): training-time windows of a trial."""
    n = len(x)
    if n > window_length:
        steps = (n - window_length) // hop_length + 1
        out = [x[i * hop_length:i * hop_length + window_length] for i in range(steps)]
        if out[-1][-1] < n - 1:
            out.append(x[-window_length:])
        return out
    return [x]


def _num_frames(modality, t):
    if modality == VIDEO:
        return t.shape[1]
    if modality in (VGGISH, BERT, LOGMEL):
        return t.shape[2]
    raise NotImplementedError(modality)


def _take(modality, t, wd):
    return t[:, wd, ...] if modality == VIDEO else t[:, :, wd, ...]


def _is_gpu(device):
    return torch.device(device).type == "cuda"


def _inputs_and_labels(X, device):
    """A loader item's tensors on ``device``, the labels (either of the reference's two label keys) taken out."""
    inputs = {k: v.to(device) for k, v in X.items()}
    labels = inputs.pop("continuous_label", None)
    if labels is None:
        labels = inputs.pop(EXPR, None)
    return inputs, labels


class _Classification:
    """Class logits [B, L, n_cls] against class indices that arrive as [B, L, 1] floats; scored from confusion counts."""
    name = CLASSIFICATION
    criterion = staticmethod(cross_entropy_loss)
    field, label_dtype = "logits", torch.int64       # a per-video entry: {"labels": int64 [n], "logits": float32 [n, n_cls]}

    def labels(self, labels, batch_size, indices, nframes=None):
        """The reference's "todo : fix this." label hack, in training (trainer.py:360-363) and in evaluation (:468-472)."""
        if labels.numel() == batch_size:
            n = len(indices[0]) if indices is not None else labels.shape[1]
            return torch.zeros((batch_size, n, 1), dtype=torch.float32, device=labels.device)
        return labels

    def check(self, outputs, labels, n_cls):
        bsz, nfms, d = labels.shape
        assert d == 1, d
        assert outputs.ndim == 3 and tuple(outputs.shape) == (bsz, nfms, n_cls), tuple(outputs.shape)

    def loss(self, criterion, outputs, labels, n_cls):
        self.check(outputs, labels, n_cls)
        rows = labels.shape[0] * labels.shape[1]
        return criterion(outputs.contiguous().view(rows, -1), labels.contiguous().view(rows).long())   # trainer.py:380-383

    def rows(self, outputs):
        return outputs.reshape(-1, outputs.shape[-1])

    def accumulator(self, n_cls, ignore_classes, device):
        from .eval_device import DeviceEvalAccumulator
        return DeviceEvalAccumulator(n_cls, ignore_classes, device=device)

    def score(self, per_video, ignore_classes):
        return metrics.compute_perf(per_video, ignore_classes)

    def master(self, perf, ignore_classes):
        return perf[ignore_classes[0]][metrics.W_F1][metrics.FRAME_LEVEL]["master"]


class _Regression:
    """One output column in [-1, 1] against float labels of the same shape (base/trainer.py:262-313); scored with RMSE /
    Pearson's r / Lin's CCC per trial and overall (base/logger.py:89-129,274-351) from per-video moments."""
    name = REGRESSION
    criterion = staticmethod(ccc_loss)
    field, label_dtype = "outputs", torch.float32    # a per-video entry: {"labels": float32 [n], "outputs": float32 [n]}

    def labels(self, labels, batch_size, indices, nframes=None):
        if nframes is not None:                       # evaluation: one whole video per loader item
            assert tuple(labels.shape) == (1, nframes, 1), tuple(labels.shape)
        return labels.float()

    def check(self, outputs, labels, n_cls):
        if outputs.shape[-1] != 1:
            raise ValueError(f"output_dim = {outputs.shape[-1]}: the regression scores cover ONE output column (the "
                             "reference scores column 0 only, base/logger.py:105-108)")
        assert tuple(outputs.shape) == tuple(labels.shape), (tuple(outputs.shape), tuple(labels.shape))

    def loss(self, criterion, outputs, labels, n_cls):
        assert outputs.ndim == 3 and tuple(outputs.shape) == tuple(labels.shape), (tuple(outputs.shape), tuple(labels.shape))
        return criterion(labels.float(), outputs)    # base/trainer.py:278: float labels, [B, L, D], gold first

    def rows(self, outputs):
        return outputs.reshape(-1)

    def accumulator(self, n_cls, ignore_classes, device):
        from .eval_device import DeviceRegressionAccumulator
        return DeviceRegressionAccumulator(device=device)

    def score(self, per_video, ignore_classes):
        return metrics.compute_regression_perf(per_video)

    def master(self, perf, ignore_classes):
        return perf[metrics.OVERALL][metrics.CCC]    # base/trainer.py:174-176


_CLASSIFICATION, _REGRESSION = _Classification(), _Regression()


def _task(task):
    """The description of ``task``: None -> classification; otherwise one of the reference's two task names
    (constants.py:17-20), any letter case."""
    name = CLASSIFICATION if task is None else str(task).upper()
    if name not in TASKS:
        raise ValueError(f"task must be one of {TASKS}, got {name!r}")
    return _REGRESSION if name == REGRESSION else _CLASSIFICATION


class DeviceEvalMixin:
    """``inference`` / ``inference_forward_windows`` / ``window_input`` with the reference's signatures
    (trainer.py:436,788,832) on top of whatever trainer provides ``self.model``, ``self.device``, ``self.number_classes``,
    ``self.train_batch_size`` and ``self.args`` (``window_length``, ``hop_length``, ``model_name``; optional ``amp``).

    ``self.eval_aggregate``: "device" (default on a GPU) keeps logits on the card, stitches overlapping windows with one
    kernel and folds every video into device-side confusion counts; "host" is the reference's own sequence (one forward
    per window, indexed adds, numpy scores) and the checker of the device path.  ``self.eval_frame_budget`` bounds the frames
    one forward may carry when windows are batched (default: ``train_batch_size x window_length``, the training
    footprint), so a long video never needs more activation memory than a training step.

    ``self.eval_video_batch`` > 1 (device aggregation, LFAN, videos of at least one window): the windows of several videos
    share forwards -- groups of at most ``eval_frame_budget`` frames that may span videos -- and every ``eval_video_batch``
    videos are stitched with one launch and folded into the counts with one call.  ``self.eval_shard`` under an initialised
    ``torch.distributed`` with world > 1: rank r evaluates the videos at loader positions p % world == r, the device counts
    are summed with one all-reduce and the per-video logits are gathered back into loader order.

    ``task`` = "REGRESSION" (``self.args.task`` or ``self.task``): the model's [1, n, 1] outputs go through the same windows,
    stitch kernel, batching and sharding, and are scored with RMSE / Pearson's r / Lin's CCC per trial and overall
    (``DeviceRegressionAccumulator``, or ``metrics.compute_regression_perf`` on the host path)."""

    eval_aggregate = None          # None -> "device" on a GPU, "host" otherwise
    eval_frame_budget = None
    eval_video_batch = 1           # 1: one forward (group) per video, as the reference
    eval_shard = False             # True: split the videos over the torch.distributed ranks
    eval_keep_logits = True        # the reference always returns (and pickles) the per-video logits (trainer.py:500-523)
    ignore_classes = (None,)

    # ---- small accessors so the mixin works on the reference trainer (args namespace) and on ours
    def _arg(self, name, default=None):
        args = getattr(self, "args", None)
        if args is not None and hasattr(args, name):
            return getattr(args, name)
        return getattr(self, name, default)

    def _aggregate(self, aggregate=None):
        aggregate = aggregate or self.eval_aggregate or ("device" if _is_gpu(self.device) else "host")
        if aggregate not in ("device", "host"):
            raise ValueError(aggregate)
        if aggregate == "device" and not _is_gpu(self.device):
            raise ValueError("aggregate='device' needs a GPU trainer (the stitch / confusion kernels take device pointers)")
        return aggregate

    def window_input(self, data):
        sizes = [[t.shape[0], _num_frames(m, t)] for m, t in data.items()]
        for s in sizes:
            assert s == sizes[0], f"{s} | {sizes[0]}"
        windows = windowing(np.arange(sizes[0][1]), self._arg("window_length"), self._arg("hop_length"))
        return [[{m: _take(m, t, wd) for m, t in data.items()}, wd] for wd in windows]

    def _windows_per_forward(self, wlen):
        """How many ``wlen``-frame windows one forward may carry: ``eval_frame_budget`` (default: the training footprint,
        ``train_batch_size x window_length``) in whole windows, at least one."""
        budget = self.eval_frame_budget or max(1, int(self._arg("train_batch_size", 1))) * int(self._arg("window_length"))
        return max(1, budget // max(wlen, 1))

    def inference_forward_windows(self, data, aggregate=None):
        """Forward a video longer than the model's window (trainer.py:832-892).  Device path: the windows go through the
        model in groups of at most ``eval_frame_budget`` frames (eval mode: clips are independent), then ONE kernel
        scatter-adds them in window order and divides by the overlap counts -- a ``_VideoWindowBatch`` of one video.  Host path:
        the reference's own sequence.  A batch of several videos (bsz > 1; the reference asserts bsz == 1 in ``inference``
        but not here) always takes the host path, whose indexed adds carry the batch dimension."""
        total = _num_frames(*next(iter(data.items())))
        chunks = self.window_input(data)
        last = int(chunks[-1][1][-1])
        assert total == last + 1, f"{total} | {last + 1}"
        aggregate = self._aggregate(aggregate)
        bsz = next(iter(data.values())).shape[0]
        if aggregate == "device" and bsz == 1:
            video = _VideoWindowBatch(self.model, self._windows_per_forward(len(chunks[0][1])))
            video.add(None, chunks, total)
            return video.flush()[0].unsqueeze(0)
        results = []
        for chunk, wd in chunks:
            out = self.model({m: t.contiguous() for m, t in chunk.items()})
            assert out.ndim == 3, out.ndim
            results.append((out, wd))
        final = torch.zeros((results[-1][0].shape[0], total, results[-1][0].shape[2]), device=results[-1][0].device,
                            dtype=results[-1][0].dtype)
        idx = []
        for out, wd in results:
            final[:, wd, ...] = final[:, wd, ...] + out
            idx += wd.tolist()
        counts = sorted(Counter(idx).items())
        freqs = torch.tensor([c for _, c in counts], dtype=final.dtype, device=final.device).view(1, -1, 1)
        where = np.asarray([i for i, _ in counts], dtype=np.int64)
        final[:, where, ...] = final[:, where, ...] / freqs
        return final

    def _eval_shard_rank_world(self):
        """(rank, world) of sharded evaluation, read from torch.distributed (the mixin also serves trainers without
        ``self.ddp``); (0, 1) when ``eval_shard`` is off or no process group is initialised."""
        if not self.eval_shard:
            return 0, 1
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return 0, 1
        return dist.get_rank(), dist.get_world_size()

    @torch.no_grad()
    def inference(self, dataloader, keep_logits=None, aggregate=None):
        """Trainer.inference (trainer.py:436-523): returns ``(current_perf, per_video)``.  Device path: each video is folded
        into the task's device-side accumulator (confusion counts, or one row of moments per video) and the scores come from
        one small copy at the end; the per-video ``{labels, logits}`` (regression: ``{labels, outputs}``) dictionary the
        reference returns is filled when ``keep_logits`` (default ``self.eval_keep_logits`` = True, as the reference; False
        skips the per-video copies).  ``eval_video_batch`` / ``eval_shard``: see the class docstring; the returned dictionary
        has the same keys in the same (loader) order either way.  Regression scores (base/trainer.py:262-313):
        ``{trial: {"rmse", "pcc", "ccc"}, ..., "overall": {...}}``."""
        task = _task(self._arg("task"))
        aggregate = self._aggregate(aggregate)
        keep_logits = self.eval_keep_logits if keep_logits is None else keep_logits
        video_batch = int(self.eval_video_batch or 1)
        if video_batch < 1:
            raise ValueError(f"eval_video_batch must be >= 1, got {self.eval_video_batch!r}")
        self.model.eval()
        rank, world = self._eval_shard_rank_world()
        acc = task.accumulator(self.number_classes, self.ignore_classes, self.device) if aggregate == "device" else None
        record = keep_logits or acc is None
        entries = []                                      # (loader position, trial, {labels, logits / outputs})
        amp = bool(self._arg("amp", False)) and _is_gpu(self.device)
        wlen = int(self._arg("window_length"))

        def forward(batch):
            with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
                return self.model(batch)

        batched = None
        if acc is not None and video_batch > 1 and self._arg("model_name") == "LFAN":
            batched = _VideoWindowBatch(forward, self._windows_per_forward(wlen))

        def fold(values, labels, offsets, keys):
            """Rows of one or several videos (``task.rows``) with one label per row."""
            if acc is not None:
                acc.add(values, labels, video_offsets=offsets, keys=keys)
            if record:
                v, lb = values.cpu().numpy(), labels.to(task.label_dtype).cpu().numpy()
                for (pos, trial), a, b in zip(keys, offsets, offsets[1:]):
                    entries.append((pos, trial, {"labels": lb[a:b], task.field: v[a:b]}))

        def flush():
            stitched, offsets, videos = batched.flush()
            fold(task.rows(stitched), torch.cat([lb for _, lb in videos]), offsets, [key for key, _ in videos])

        for pos, (X, trials, lengths, indices) in enumerate(dataloader):
            if pos % world != rank:
                continue
            inputs, labels = _inputs_and_labels(X, self.device)
            nframes = 0
            for m, t in inputs.items():
                assert t.shape[0] == 1, f"{t.shape[0]} | {m}"
                nframes = _num_frames(m, t)
            labels = task.labels(labels, self.train_batch_size, indices, nframes)
            if batched is not None and nframes >= wlen:
                assert tuple(labels.shape) == (1, nframes, 1), tuple(labels.shape)
                batched.add(((pos, trials[0]), labels.reshape(-1)), self.window_input(inputs), nframes)
                if len(batched) >= video_batch:
                    flush()
                continue
            with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
                if nframes > wlen and self._arg("model_name") == "LFAN":
                    outputs = self.inference_forward_windows(inputs, aggregate)
                else:
                    outputs = self.model(inputs)
            outputs = outputs.detach().float()
            task.check(outputs, labels, self.number_classes)
            fold(task.rows(outputs), labels.reshape(-1), [0, labels.numel()], [(pos, trials[0])])
        if batched is not None and len(batched):
            flush()
        if world > 1:                                   # every rank takes part, with or without videos of its own
            import torch.distributed as dist
            if acc is not None:
                acc.merge_ranks()
            if record:
                parts = [None] * world
                dist.all_gather_object(parts, entries)
                entries = [e for part in parts for e in part]
        per_video = {}
        for _, trial, entry in sorted(entries, key=lambda e: e[0]):   # loader order; a repeated trial id: the last one wins
            per_video[trial] = entry
        return (acc.compute() if acc is not None else task.score(per_video, self.ignore_classes)), per_video


class _VideoWindowBatch:
    """The videos of one ``eval_video_batch`` on the batched LFAN path (or the one video of ``inference_forward_windows``).
    Their windows go through ``forward`` in groups of ``group`` windows as soon as a group is full (a group may span videos;
    at most one group of inputs is held beyond the current video's windows), only the window outputs are kept, and ``flush``
    stitches every video with ONE launch."""

    def __init__(self, forward, group):
        self.forward, self.group = forward, group
        self._reset()

    def _reset(self):
        self.pending, self.outs = [], []             # window inputs not forwarded yet; [g, Lw, C] float32 outputs
        self.starts, self.win_off, self.frame_off = [], [0], [0]
        self.videos = []

    def __len__(self):
        return len(self.videos)

    def add(self, video, windows, nframes):
        """``windows``: ``window_input``'s [(inputs, frame indices)] of one ``nframes``-frame video; ``video``: whatever the
        caller wants back from ``flush`` for it."""
        for chunk, wd in windows:
            self.pending.append(chunk)
            self.starts.append(int(wd[0]))
            if len(self.pending) == self.group:
                self._run()
        self.win_off.append(len(self.starts))
        self.frame_off.append(self.frame_off[-1] + nframes)
        self.videos.append(video)

    def _run(self):
        part, self.pending = self.pending, []
        out = self.forward({m: torch.cat([c[m] for c in part], dim=0).contiguous() for m in part[0]})
        assert out.ndim == 3 and out.shape[0] == len(part), tuple(out.shape)
        self.outs.append(out.detach().float())

    def flush(self):
        """-> (stitched outputs [R, C], frame offsets [V+1], the V ``video`` items); the batch is empty afterwards."""
        from .eval_device import stitch_windows_multi
        if self.pending:
            self._run()
        out = self.outs[0] if len(self.outs) == 1 else torch.cat(self.outs, dim=0)
        res = (stitch_windows_multi(out, self.starts, self.win_off, self.frame_off), list(self.frame_off), list(self.videos))
        self._reset()
        return res


_SCHEDULER_DEFAULTS = {"gamma": 0.1, "step_size": 40, "last_epoch": -1, "min_lr": 1e-7, "t_max": 100}   # default_config.py


class FlooredStepLR(torch.optim.lr_scheduler.LRScheduler):
    """base/scheduler.py:167-197 ``MyStepLR``: ``max(base_lr * gamma ** (last_epoch // step_size), min_lr)``."""

    def __init__(self, optimizer, step_size, gamma=0.1, last_epoch=-1, min_lr=1e-6):
        self.step_size, self.gamma, self.min_lr = step_size, gamma, min_lr
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        return [max(base * self.gamma ** (self.last_epoch // self.step_size), self.min_lr) for base in self.base_lrs]


class CosineFromEpochOneLR(torch.optim.lr_scheduler.LRScheduler):
    """base/scheduler.py:200-243 ``MyCosineLR``: ``max(base_lr * coef * (1 + cos((last_epoch - 1) * pi / max_epochs)),
    min_lr)``."""

    def __init__(self, optimizer, coef, max_epochs, min_lr=1e-9, last_epoch=-1):
        if not isinstance(coef, float) or coef <= 0.0:
            raise ValueError(f"MYCOSINE: `coef` must be a float > 0, got {coef!r}")
        if not max_epochs > 0:
            raise ValueError(f"MYCOSINE: `max_epochs` must be > 0, got {max_epochs!r}")
        self.coef, self.max_epochs, self.min_lr = coef, float(max_epochs), min_lr
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        return [max(base * self.coef * (1.0 + math.cos((self.last_epoch - 1) * math.pi / self.max_epochs)), self.min_lr)
                for base in self.base_lrs]


def make_lr_scheduler(optimizer, hp):
    """instantiators.py:140-185 on the ``opt__`` hyper-parameters ``hp`` (prefix stripped).  Keys ``default_config.py``
    defines fall back to its values; ``coef``, ``max_epochs`` and ``milestones`` (read by MYCOSINE / MULTISTEP, defined
    nowhere in the reference's defaults) must be given."""
    name = str(hp.get("name_lr_scheduler")).upper()

    def get(key):
        if key in hp:
            return hp[key]
        if key in _SCHEDULER_DEFAULTS:
            return _SCHEDULER_DEFAULTS[key]
        raise ValueError(f"lr scheduler {name}: missing hyper-parameter `opt__{key}`")

    if name == "MYWARMUP":
        raise NotImplementedError("lr scheduler MYWARMUP: MyWarmupScheduler.step(epoch, metrics) needs the validation metric, "
                                  "but the reference's training loop calls scheduler.step() without arguments "
                                  "(trainer.py:694)")
    if not isinstance(optimizer, torch.optim.Optimizer):
        raise TypeError(f"lr scheduler {name} cannot drive {type(optimizer).__name__}: not a torch.optim.Optimizer")
    sch = torch.optim.lr_scheduler
    if name == "STEP":
        return sch.StepLR(optimizer, step_size=get("step_size"), gamma=get("gamma"), last_epoch=get("last_epoch"))
    if name == "MYSTEP":
        return FlooredStepLR(optimizer, step_size=get("step_size"), gamma=get("gamma"), last_epoch=get("last_epoch"),
                             min_lr=get("min_lr"))
    if name == "COSINE":
        return sch.CosineAnnealingLR(optimizer, T_max=get("t_max"), eta_min=get("min_lr"), last_epoch=get("last_epoch"))
    if name == "MYCOSINE":
        return CosineFromEpochOneLR(optimizer, coef=get("coef"), max_epochs=get("max_epochs"), min_lr=get("min_lr"),
                                    last_epoch=get("last_epoch"))
    if name == "MULTISTEP":
        return sch.MultiStepLR(optimizer, milestones=get("milestones"), gamma=get("gamma"), last_epoch=get("last_epoch"))
    raise ValueError(f"Unsupported learning rate scheduler `{hp.get('name_lr_scheduler')}`")


_REFERENCE_KWARGS = ("device", "emotion", "model_name", "models", "save_path", "fold", "min_epoch", "max_epoch",
                     "early_stopping", "learning_rate", "min_learning_rate", "patience", "train_batch_size",
                     "eval_batch_size", "criterion", "factor", "verbose", "milestone", "metrics",
                     "load_best_at_each_epoch", "save_plot")   # experiment.py:153-175


class Trainer(DeviceEvalMixin):
    """``Trainer(**trainer_kwards)`` as ``experiment.py:153-178`` builds it, or the short form
    ``Trainer(model, optimizer=..., window_length=..., ...)`` the benches and parity tests use."""

    def __init__(self, model=None, optimizer=None, criterion=None, device="cuda", window_length=300, hop_length=200,
                 model_name="LFAN", train_batch_size=2, number_classes=None, data_parallel=None, ignore_classes=(None,),
                 task=None, **kwargs):
        if model is None:
            if "models" not in kwargs:
                raise TypeError("Trainer needs the model: Trainer(model, ...) or Trainer(models=model, ...) as experiment.py does")
            model = kwargs.pop("models")
        for k in _REFERENCE_KWARGS:                      # base/trainer.py:21-45,96-115 keep them as attributes
            if k in kwargs:
                setattr(self, k, kwargs.pop(k))
        if kwargs:
            raise TypeError(f"unexpected Trainer arguments: {sorted(kwargs)}")
        self.device = device
        self.model = model.to(device) if hasattr(model, "to") else model     # base/trainer.py:25
        self.optimizer, self.scheduler = optimizer, None
        self.scaler = None                               # the --amp GradScaler (trainer.py:341), one per train_one_epoch
        self._default_criterion = criterion is None      # then the criterion follows the task: cross entropy / CCC loss
        self.criterion = criterion if criterion is not None else _task(task).criterion
        self.model_name, self.train_batch_size = model_name, train_batch_size
        self.number_classes = number_classes if number_classes is not None else 7
        self.ddp, self.ignore_classes = data_parallel, tuple(ignore_classes)
        # trainer.py:436-523,832 read the window rule and model name from the argparse namespace
        self.args = SimpleNamespace(window_length=window_length, hop_length=hop_length, model_name=model_name, amp=False,
                                    task=_task(task).name)
        self.epoch, self.counter, self.seed = 0, 0, 0
        self.dataloaders = None
        self.fit_finished = False
        self.start_epoch = 0
        self.cl_to_int, self.int_to_cl = {}, {}
        self.max_epoch = getattr(self, "max_epoch", 0)

    # the short form's attribute names stay readable
    window_length = property(lambda self: self.args.window_length)
    hop_length = property(lambda self: self.args.hop_length)
    task = property(lambda self: _task(self.args.task).name)

    # ------------------------------------------------------------------ the calls experiment.py:178-182 makes
    def set_args(self, args):
        """trainer.py:92-93.  ``args`` is the argparse namespace (or any object / dict with its fields)."""
        if isinstance(args, dict):
            args = SimpleNamespace(**args)
        for k, v in vars(self.args).items():            # keep the short form's window rule unless args overrides it
            if not hasattr(args, k):
                setattr(args, k, v)
        self.args = args
        if getattr(args, "model_name", None):
            self.model_name = args.model_name
        if self._default_criterion:
            self.criterion = _task(args.task).criterion

    def post_set_args(self, class_id=None):
        """trainer.py:95-105 loads ``<folds_dir>/split-<fold>/class_id.yaml``; the file belongs to the dataset folds, which
        are not on this path -- pass the mapping directly (``{class name: int}``) or leave it empty."""
        assert self.args is not None
        self.cl_to_int = dict(class_id or {})
        self.int_to_cl = {v: k for k, v in self.cl_to_int.items()}
        assert len(self.int_to_cl) == len(self.cl_to_int), "more than 1 key with same value. wrong."

    def set_number_classes(self, ncls):
        assert isinstance(ncls, int), type(ncls)
        assert ncls > 0, ncls
        self.number_classes = ncls

    def get_parameters(self):
        """base/trainer.py:83-93"""
        return [p for _, p in self.model.named_parameters() if p.requires_grad]

    def init_optimizer_and_scheduler(self, epoch=0):
        """trainer.py:127-134 -> instantiators.py:62-185: ``opt__``-prefixed hyper-parameters, names compared
        case-insensitively (the reference's constants are ``'SGD'`` / ``'MYSTEP'`` ...).  SGD and Adam are built WITHOUT
        ``lr`` (instantiators.py:74-92: torch's default 1e-3 applies until a scheduler changes it).  With ``data_parallel``
        the same update runs as ONE fused launch over the flat bucket (``FlatNesterovSGD`` / ``FlatAdam``), and the
        scheduler drives that optimiser like any other."""
        a = {k.split("__", 1)[1] if k.startswith("opt") and "__" in k else k: v for k, v in vars(self.args).items()}
        name = str(a.get("name_optimizer", "sgd")).upper()
        params = self.get_parameters()
        if name == "SGD":
            hp = dict(momentum=a.get("momentum", 0.9), dampening=a.get("dampening", 0.0),
                      weight_decay=a.get("weight_decay", 1e-4), nesterov=a.get("nesterov", True))
            if self.ddp is not None and hp["nesterov"] and hp["dampening"] == 0.0:
                from .data_parallel import FlatNesterovSGD
                self.optimizer = FlatNesterovSGD(self.ddp, lr=1e-3, momentum=hp["momentum"], weight_decay=hp["weight_decay"])
            else:
                self.optimizer = torch.optim.SGD(params=params, **hp)
        elif name == "ADAM":
            hp = dict(betas=(a.get("beta1", 0.9), a.get("beta2", 0.999)), eps=a.get("eps_adam", 1e-8),
                      weight_decay=a.get("weight_decay", 0.0), amsgrad=a.get("amsgrad", False))
            if self.ddp is not None:
                from .data_parallel import FlatAdam
                self.optimizer = FlatAdam(self.ddp, lr=1e-3, **hp)
            else:
                self.optimizer = torch.optim.Adam(params=params, **hp)
        else:
            raise ValueError(f"Unsupported optimizer `{a.get('name_optimizer')}`")
        self.scheduler = make_lr_scheduler(self.optimizer, a) if a.get("lr_scheduler") else None

    # ------------------------------------------------------------------ training
    def _split(self, X):
        return _inputs_and_labels(X, self.device)

    def _train_amp(self):
        """``--amp`` on a GPU: the step runs the forward and the loss under fp16 autocast, as ``inference`` does, with loss
        scaling (trainer.py:341,365-391)."""
        return bool(self._arg("amp", False)) and _is_gpu(self.device)

    def _new_scaler(self):
        """``FlatGradScaler`` with ``data_parallel`` (one launch over the flat bucket, no host read in the step), torch's
        ``GradScaler`` otherwise."""
        if self.ddp is not None:
            from .data_parallel import FlatGradScaler
            return FlatGradScaler("cuda")
        return torch.amp.GradScaler("cuda")

    def train_step(self, X, indices=None):
        """One iteration of trainer.py:345-391.  Returns the (detached) loss tensor.  With ``args.amp`` (GPU): autocast
        forward and loss, then ``scaler.scale(loss).backward()``, the gradient all-reduce, ``scaler.step``, ``scaler.update``
        -- a step with a non-finite gradient is skipped and halves the scale, as the reference's GradScaler does."""
        task = _task(self.args.task)
        inputs, labels = self._split(X)
        labels = task.labels(labels, self.train_batch_size, indices)
        if self.ddp is not None:
            self.ddp.zero_grad()
        else:
            self.optimizer.zero_grad(set_to_none=True)
        amp = self._train_amp()
        with torch.autocast("cuda", dtype=torch.float16) if amp else contextlib.nullcontext():
            outputs = self.model(inputs)
            loss = task.loss(self.criterion, outputs, labels, self.number_classes)
        if not amp:
            loss.backward()
            if self.ddp is not None:
                self.ddp.all_reduce_gradients()
            self.optimizer.step()
            return loss.detach()
        if self.scaler is None:
            self.scaler = self._new_scaler()
        self.scaler.scale(loss).backward()
        if self.ddp is not None:
            self.ddp.all_reduce_gradients()   # found_inf is taken after it: every rank sees the summed bucket
        self.scaler.step(self.optimizer)
        self.scaler.update()
        return loss.detach()

    def train_one_epoch(self, dataloader=None):
        """trainer.py:315-434 (the reference reads ``self.dataloaders[TRAINSET]``; a loader may also be passed).  Like the
        reference, ``--amp`` starts every epoch with a fresh GradScaler (trainer.py:341)."""
        if dataloader is None:
            dataloader = self.dataloaders[TRAINSET]
        self.model.train()
        self.scaler = self._new_scaler() if self._train_amp() else None
        running, count = 0.0, 0
        for X, trials, lengths, indices in dataloader:
            running = running + self.train_step(X, indices)
            count += 1
        self.counter += 1
        return float(running / max(count, 1))

    def optimize(self, dataloader_dict, checkpoint_controller=None, parameter_controller=None):
        """trainer.py:611-770 without its control plane: validate, ``max_epoch`` x (train epoch, scheduler step,
        validate, remember the best weights by frame-level weighted F1 -- by the overall CCC when ``task`` is "REGRESSION",
        base/trainer.py:174-176), then test the best weights.  Returns
        ``{"valid": [perf per evaluation], "loss": [epoch losses], "test": perf, "best_epoch": i}``."""
        self.dataloaders = dataloader_dict
        if self.optimizer is None:
            self.init_optimizer_and_scheduler(epoch=0)
        history = {"valid": [], "loss": []}

        def master(perf):
            return _task(self.args.task).master(perf, self.ignore_classes)

        def evaluate(loader, **kwargs):
            if self.eval_shard and self.ddp is not None:   # one set of BatchNorm statistics: every shard scores the same model
                self.ddp.sync_buffers()
            return self.inference(loader, **kwargs)
        perf, _ = evaluate(dataloader_dict[VALIDSET], keep_logits=False)
        history["valid"].append(perf)
        best, best_state, best_epoch = master(perf), {k: v.detach().clone() for k, v in self.model.state_dict().items()}, -1
        for epoch in range(int(self.max_epoch)):
            history["loss"].append(self.train_one_epoch())
            if self.scheduler is not None:
                self.scheduler.step()
            if parameter_controller is not None and hasattr(parameter_controller, "step"):
                parameter_controller.step(epoch)
            perf, _ = evaluate(dataloader_dict[VALIDSET], keep_logits=False)
            history["valid"].append(perf)
            if master(perf) > best:
                best, best_epoch = master(perf), epoch
                best_state = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
        self.fit_finished = True
        if TESTSET in dataloader_dict:
            self.model.load_state_dict(best_state, strict=True)
            history["test"], history["test_logits"] = evaluate(dataloader_dict[TESTSET])
        history["best_epoch"] = best_epoch
        return history
