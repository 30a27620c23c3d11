"""Per-component statistics of the ``vggish`` and ``bert`` rows, and their standardisation, on the device.

The reference never hands the model raw ``vggish`` or ``bert`` rows: ``GenericDataset.get_feature_transform``
(base/dataset.py:516-539) wraps every modality other than ``video`` and ``logmel`` in ``transforms.Normalize(mean, std)``, with
the per-component dataset statistics of ``calculate_mean_std`` (base/dataset.py:272-325), stored as
``mean_std_info_fold-{j}.pkl`` (base/experiment.py:242-269).  ``trial_dataset.TrialDataset`` applies that rule to precomputed
``.npy`` features; this module is the same rule for rows that are made on the GPU (``feature_extractor``, ``live.AVStream``):

  FeatureMoments       float64 sums of x and x * x per component, fed [M, C] device rows (``ops.feature_moments_update``), merged
                       across accumulators or ranks, finalised on the host by the reference's formulas.
  save_mean_std / load_mean_std   the reference's pickle of {feature: {"mean", "std"}} (base/utils.py:16-28).
  FeatureStandardizer  fp32 device copies of such a dict; ``(rows - mean) / std`` in one launch (``ops.standardize_rows``).

``video`` and ``logmel`` stay out of it: the frames have their own transform, and with ``logmel`` the model runs VGGish itself
on examples the reference passes through ``ToTensor`` only.

The statistics differ from a reference-made pickle in the last bits: the reference sums float32 rows in float32 numpy
arithmetic (pairwise per file, then file by file), these are float64 sums of the same float32 values, rounded to float32
once at the end.  They are the more accurate ones; a file from either side loads on the other.
"""
import pickle

import numpy as np
import torch

from . import ops

EXEMPT = ("video", "logmel")   # base/dataset.py:516-539: these two are not wrapped in Normalize


def _device(device):
    """``torch.device`` with the index filled in ("cuda" -> the current GPU), so that it compares equal to a tensor's."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def _check_dims(dims):
    try:
        dims = {str(f): int(c) for f, c in dict(dims).items()}
    except (TypeError, ValueError):
        raise ValueError(f"dims: expected {{feature: C}}, got {dims!r}") from None
    if not dims:
        raise ValueError("dims: no feature")
    for f, c in dims.items():
        if f in EXEMPT:
            raise ValueError(f"{f!r} is not standardised (the reference wraps neither 'video' nor 'logmel' in Normalize)")
        if not 1 <= c <= ops.FEATURE_NORM_MAX_C:
            raise ValueError(f"dims[{f!r}] = {c}: expected 1 .. {ops.FEATURE_NORM_MAX_C}")
    return dims


def finalize_sums(s1, s2, n):
    """float64 sums of x and of x * x over ``n`` rows -> (mean, std) as float32 arrays, by the formulas of
    base/dataset.py:272-325 in float64: mean = S1 / (n + 1e-10); std = sqrt((S2 - 2 mean S1 + n mean^2) / (n - 1)), the sum of
    squared deviations about THAT mean, expanded.  A sum of squares that cancellation left below zero counts as zero.  Each
    result is rounded to float32 once.  No GPU."""
    n = int(n)
    if n < 2:
        raise ValueError(f"{n} rows: the unbiased std needs at least 2")
    s1, s2 = np.asarray(s1, np.float64), np.asarray(s2, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        mean = s1 / (n + 1e-10)
        ssd = s2 - 2.0 * mean * s1 + n * mean * mean
        std = np.sqrt(np.where(ssd < 0, 0.0, ssd) / (n - 1))
    return mean.astype(np.float32), std.astype(np.float32)


class FeatureMoments:
    """Running float64 sums of x and x * x per component of the features in ``dims`` = {feature: C}, on ``device``.

      update(feature, rows)   rows [M, C] float32 on the device, or [..., C]: one launch, no host synchronisation.  The sums of
                              a column are float64 adds in row order, so they depend on the sequence of rows only, not on
                              how it was cut into calls.
      count                   {feature: rows seen}, host ints.
      sums                    {feature: [2, C] float64 on the device} (row 0: sum of x, row 1: sum of x * x).
      merge(other)            add another accumulator's sums and counts (same features and sizes).
      all_reduce(group=None)  the same over ``torch.distributed``: a SUM of the sums and of the counts.
      finalize()              {feature: {"mean": float32 [C], "std": float32 [C]}}: the reference's dict (``finalize_sums``).

    On ``device="cpu"`` the state, ``merge``, ``all_reduce`` and ``finalize`` work (a gloo group, a host-side merge of
    saved sums); ``update`` needs the GPU, there is no CPU path for the kernel."""

    def __init__(self, dims, device="cuda"):
        self.dims = _check_dims(dims)
        self.device = _device(device)
        self.sums = {f: torch.zeros((2, c), dtype=torch.float64, device=self.device) for f, c in self.dims.items()}
        self.count = {f: 0 for f in self.dims}

    def _feature(self, feature):
        if feature not in self.dims:
            raise ValueError(f"{feature!r}: not one of {sorted(self.dims)}")
        return self.dims[feature]

    def update(self, feature, rows):
        c = self._feature(feature)
        if not torch.is_tensor(rows) or rows.dim() < 1 or rows.shape[-1] != c or rows.numel() < c:
            raise ValueError(f"{feature}: expected float32 rows [..., {c}] with at least one row, got "
                             f"{tuple(rows.shape) if torch.is_tensor(rows) else type(rows).__name__}")
        if not rows.is_contiguous():
            raise ValueError(f"{feature}: rows are not contiguous")
        if rows.device != self.device:
            raise ValueError(f"{feature}: rows on {rows.device}, the accumulator on {self.device}")
        flat = rows.view(-1, c)
        ops.feature_moments_update(flat, self.sums[feature])
        self.count[feature] += flat.shape[0]

    def merge(self, other):
        if not isinstance(other, FeatureMoments) or other.dims != self.dims:
            raise ValueError(f"merge: expected a FeatureMoments over {self.dims}, got "
                             f"{other.dims if isinstance(other, FeatureMoments) else type(other).__name__}")
        for f in self.dims:
            self.sums[f] += other.sums[f].to(self.device)
            self.count[f] += other.count[f]
        return self

    def all_reduce(self, group=None):
        import torch.distributed as dist
        feats = sorted(self.dims)
        counts = torch.tensor([self.count[f] for f in feats], dtype=torch.int64, device=self.device)
        dist.all_reduce(counts, op=dist.ReduceOp.SUM, group=group)
        for f in feats:
            dist.all_reduce(self.sums[f], op=dist.ReduceOp.SUM, group=group)
        for f, n in zip(feats, counts.tolist()):
            self.count[f] = int(n)
        return self

    def finalize(self):
        out = {}
        for f in self.dims:
            try:
                host = self.sums[f].cpu().numpy()
                mean, std = finalize_sums(host[0], host[1], self.count[f])
            except ValueError as err:
                raise ValueError(f"{f}: {err}") from None
            out[f] = {"mean": mean, "std": std}
        return out


def save_mean_std(path, mean_std):
    """The reference's ``save_to_pickle(path, data, replace=True)`` (base/utils.py:21-28): a plain pickle of the dict."""
    with open(path, "wb") as handle:
        pickle.dump({f: {"mean": np.asarray(v["mean"]), "std": np.asarray(v["std"])} for f, v in mean_std.items()}, handle)


def load_mean_std(path):
    """The reference's ``load_pickle`` (base/utils.py:16-19).  A pickle can run code when it is loaded: load your own files."""
    with open(path, "rb") as handle:
        return pickle.load(handle)


def _vector(value, what):
    a = np.asarray(value)
    if a.ndim == 2 and a.shape[0] == 1:   # the [1, C] that Normalize is handed
        a = a[0]
    if a.ndim != 1 or a.dtype.kind not in "fiu":
        raise ValueError(f"{what}: expected a numeric vector [C], got shape {a.shape} of {a.dtype}")
    return a.astype(np.float32)


class FeatureStandardizer:
    """``(rows - mean) / std`` per component for the features of ``mean_std`` = {feature: {"mean": [C], "std": [C]}} (what
    ``FeatureMoments.finalize``, ``load_mean_std`` or the reference's pickle give), as torchvision's ``Normalize`` computes it:
    the statistics are rounded to float32 first, then one float32 subtraction and one division per element.

    Refused at construction (ValueError): the keys ``video`` and ``logmel``; a mean or std that is no vector, of different
    lengths, of a length that is no multiple of 4 or, with ``dims`` = {feature: C}, not C; a non-finite entry; a std of 0
    after the rounding to float32 (as torchvision's ``normalize`` refuses it).  ``device``: where the fp32 copies live (made
    at once); None: made for the device of the first rows.

      __call__(feature, rows, out=None)   rows [..., C] float32 on the GPU, contiguous -> the standardised rows in ``out``
                                          (``rows`` itself: in place; None: a fresh tensor), one ``ops.standardize_rows``."""

    def __init__(self, mean_std, device=None, dims=None):
        if isinstance(mean_std, FeatureStandardizer):
            mean_std = mean_std.mean_std
        try:
            items = {str(f): (v["mean"], v["std"]) for f, v in dict(mean_std).items()}
        except (TypeError, ValueError, KeyError, IndexError):
            raise ValueError("mean_std: expected {feature: {'mean': [C], 'std': [C]}}") from None
        if not items:
            raise ValueError("mean_std: no feature")
        self.mean_std = {}
        for f, (mean, std) in items.items():
            if f in EXEMPT:
                raise ValueError(f"mean_std[{f!r}]: {f!r} is not standardised (the reference wraps neither 'video' nor 'logmel' "
                                 f"in Normalize)")
            mean, std = _vector(mean, f"mean_std[{f!r}]['mean']"), _vector(std, f"mean_std[{f!r}]['std']")
            if mean.shape != std.shape:
                raise ValueError(f"mean_std[{f!r}]: mean has {mean.shape[0]} components, std {std.shape[0]}")
            c = mean.shape[0]
            if c < 4 or c % 4 or c > ops.FEATURE_NORM_MAX_C:
                raise ValueError(f"mean_std[{f!r}]: {c} components: expected a multiple of 4 up to {ops.FEATURE_NORM_MAX_C}")
            if dims is not None and f in dims and int(dims[f]) != c:
                raise ValueError(f"mean_std[{f!r}]: {c} components, the rows of {f!r} have {int(dims[f])}")
            if not (np.isfinite(mean).all() and np.isfinite(std).all()):
                raise ValueError(f"mean_std[{f!r}]: a mean or std is not finite")
            if (std == 0).any():
                raise ValueError(f"mean_std[{f!r}]: std evaluated to zero after conversion to float32 at component "
                                 f"{int(np.flatnonzero(std == 0)[0])}, leading to division by zero")
            self.mean_std[f] = {"mean": mean, "std": std}
        self._dev = {}
        self.device = None if device is None else _device(device)
        if self.device is not None:
            for f in self.mean_std:
                self._copies(f, self.device)

    def __contains__(self, feature):
        return feature in self.mean_std

    def keys(self):
        return self.mean_std.keys()

    def dim(self, feature):
        return self.mean_std[feature]["mean"].shape[0]

    def to(self, device):
        """Make (or keep) the fp32 copies on ``device`` and accept rows from there only."""
        self.device = _device(device)
        for f in self.mean_std:
            self._copies(f, self.device)
        return self

    def _copies(self, feature, device):
        key = (feature, device)
        if key not in self._dev:
            v = self.mean_std[feature]
            self._dev[key] = (torch.from_numpy(v["mean"]).to(device), torch.from_numpy(v["std"]).to(device))
        return self._dev[key]

    def __call__(self, feature, rows, out=None):
        if feature not in self.mean_std:
            raise ValueError(f"{feature!r}: no statistics (have {sorted(self.mean_std)})")
        c = self.dim(feature)
        if not torch.is_tensor(rows) or rows.dim() < 1 or rows.shape[-1] != c or rows.numel() < c:
            raise ValueError(f"{feature}: expected float32 rows [..., {c}] with at least one row, got "
                             f"{tuple(rows.shape) if torch.is_tensor(rows) else type(rows).__name__}")
        if not rows.is_contiguous():
            raise ValueError(f"{feature}: rows are not contiguous")
        if out is not None and (not torch.is_tensor(out) or out.shape != rows.shape or not out.is_contiguous()):
            raise ValueError(f"{feature}: out: expected a contiguous tensor of the rows' shape {tuple(rows.shape)}")
        if self.device is not None and rows.device != self.device:
            raise ValueError(f"{feature}: rows on {rows.device}, the statistics on {self.device}")
        mean, std = self._copies(feature, rows.device)
        res = ops.standardize_rows(rows.view(-1, c), mean, std, out=None if out is None else out.view(-1, c))
        return res.view(rows.shape)


def as_standardizer(mean_std, device=None, dims=None, allowed=None, who="mean_std"):
    """None -> None; a dict or a ``FeatureStandardizer`` -> a ``FeatureStandardizer`` whose keys lie in ``allowed`` and whose
    sizes agree with ``dims`` (ValueError otherwise).  The one check of the extractor's and the live session's argument."""
    if mean_std is None:
        return None
    sd = FeatureStandardizer(mean_std, device=device, dims=dims)
    if allowed is not None:
        for f in sd.keys():
            if f not in allowed:
                raise ValueError(f"{who}[{f!r}]: the rows standardised here are those of {sorted(allowed)}")
    return sd
