"""The reference's feature statistics and their use, restated in numpy float64 (no GPU, no package code).

``mean_std(chunks)`` is base/dataset.py:272-325: two passes over the files (here: arrays), the first sums the rows and divides
by ``n + 1e-10``, the second sums the squared deviations about that mean and divides by ``n - 1``.  ``normalize`` is the
``transforms.Normalize`` of base/dataset.py:516-539 on float32 rows: ``tensor.sub_(mean).div_(std)`` with float32 statistics.
"""
import numpy as np
import torch


def mean_std(chunks):
    """``chunks``: arrays [n_i, C] (one per file) -> (mean, std) as float64 [C]."""
    chunks = [np.asarray(c, np.float64) for c in chunks]
    lengths, sums = 0, 0
    for samples in chunks:
        lengths = lengths + samples.shape[0]
        sums = sums + samples.sum(axis=0)
    mean = sums / (lengths + 1e-10)
    lengths, x_minus_mean_square = 0, 0
    for samples in chunks:
        lengths = lengths + samples.shape[0]
        x_minus_mean_square = x_minus_mean_square + ((samples - mean) ** 2).sum(axis=0)
    return mean, np.sqrt(x_minus_mean_square / (lengths - 1))


def from_sums(s1, s2, n):
    """The same two quantities from float64 sums of x and x * x: the squared deviations about ``mean`` expanded,
    sum (x - m)^2 = S2 - 2 m S1 + n m^2 (``mean`` is not exactly S1 / n, so the last two terms do not merge)."""
    s1, s2 = np.asarray(s1, np.float64), np.asarray(s2, np.float64)
    mean = s1 / (n + 1e-10)
    return mean, np.sqrt((s2 - 2.0 * mean * s1 + n * mean * mean) / (n - 1))


def normalize(x, mean, std):
    """x [..., C] float32 CPU tensor; mean, std [C] (any float type: rounded to float32 first, as Normalize does)."""
    mean = torch.as_tensor(np.asarray(mean, np.float32))
    std = torch.as_tensor(np.asarray(std, np.float32))
    return x.detach().cpu().clone().sub_(mean).div_(std)


def same_bits(a, b):
    """Equal float32 tensors bit for bit, except that any NaN equals any NaN (x86 makes -NaN of inf - inf, the GPU +NaN)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    bits = torch.int32 if a.dtype == torch.float32 else torch.int64
    return torch.equal(a.view(bits)[~na], b.view(bits)[~nb])
