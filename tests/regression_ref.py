"""The regression task restated in float64: what ``test_regression_cpu.py`` and ``test_regression_gpu.py`` compare against.

* ``ccc_loss64``: the reference's ``CCCLoss()(gold, pred)`` (base/loss_function.py:6-24) and its gradient with respect to
  ``pred`` in closed form, in numpy float64 on the given (float32) inputs.  ``tools/gen_golden_regression.py`` asserts it
  against float64 autograd of the reference class; ``ccc_loss_torch`` is the same formula in torch ops for autograd chains.
  The reference's ``+ 1e-50`` is 0 in its float32 arithmetic and is left out, so a column with Q = 0 or L = 1 is NaN here
  as it is there.
* ``moments64``: the seven moments ``cer_regression_moments`` leaves per video, with the sum of the absolute values of each
  moment's terms (the any-order summation bound ``2 (n - 1) 2^-53 sum |terms|`` is stated on those).
* the case tables of both test files, generated once per process and never modified.
"""
import functools

import numpy as np
import torch

LOSS_SHAPES = [(1, 2, 1), (1, 63, 1), (2, 64, 1), (3, 65, 2), (1, 257, 1), (2, 300, 1), (5, 8, 3)]
TANH_SIZES = [1, 63, 64, 65, 1025]
TANH_EDGES = [0.0, 1e-30, -1e-30, 20.0, -20.0, float("inf"), float("-inf"), float("nan")]
VIDEO_FRAMES = [2, 3, 64, 65, 255, 256, 257, 1000]
U = 2.0 ** -53


def spacing32(x):
    """One float32 spacing at the float32 nearest to |x| (elementwise)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def tanh64(x):
    return np.tanh(np.asarray(x, dtype=np.float64))


def ccc_loss64(gold, pred):
    """-> (loss, d loss / d pred) in float64; gold, pred [B, L, D]."""
    g, p = np.asarray(gold, dtype=np.float64), np.asarray(pred, dtype=np.float64)
    assert g.ndim == 3 and g.shape == p.shape
    n, big_n = g.shape[1], g.size
    with np.errstate(divide="ignore", invalid="ignore"):
        gm, pm = g.mean(axis=1, keepdims=True), p.mean(axis=1, keepdims=True)
        dg, dp = g - gm, p - pm
        s = (dg * dp).sum(axis=1, keepdims=True)
        vg = (dg * dg).sum(axis=1, keepdims=True) / np.float64(n - 1)
        vp = (dp * dp).sum(axis=1, keepdims=True) / np.float64(n - 1)
        m = gm - pm
        q = vg + vp + m * m
        loss = (n - 2.0 * s / q).sum() / big_n
        grad = (-2.0 * dg / q + (2.0 * s / (q * q)) * (2.0 * dp / np.float64(n - 1) - 2.0 * m / n)) / big_n
    return float(loss), grad


def ccc_loss_torch(gold, pred):
    """base/loss_function.py:12-24 with ``weights=None`` and without the ``1e-50``, on torch tensors of any float dtype."""
    gm, pm = gold.mean(1, keepdim=True), pred.mean(1, keepdim=True)
    cov = (gold - gm) * (pred - pm)
    q = gold.var(1, keepdim=True, unbiased=True) + pred.var(1, keepdim=True, unbiased=True) + (gm - pm) * (gm - pm)
    return torch.mean(1.0 - 2.0 * cov / q)


def chain64(gold, x, scale=1.0):
    """``scale * ccc_loss(gold, tanh(x))`` and its gradient with respect to ``x`` by float64 torch autograd."""
    x64 = torch.tensor(np.array(x), dtype=torch.float64, requires_grad=True)
    loss = ccc_loss_torch(torch.tensor(np.array(gold), dtype=torch.float64), torch.tanh(x64)) * scale
    loss.backward()
    return loss.item(), x64.grad.numpy()


@functools.lru_cache(maxsize=None)
def loss_case(shape, seed=0):
    """(gold, pred) float32 [B, L, D]: labels uniform in [-1, 1], predictions tanh(normal) -- the ranges of the task."""
    rng = np.random.default_rng(1000 * seed + sum(s * 31 ** i for i, s in enumerate(shape)))
    gold = rng.uniform(-1.0, 1.0, size=shape).astype(np.float32)
    pred = np.tanh(rng.standard_normal(size=shape)).astype(np.float32)
    gold.setflags(write=False)
    pred.setflags(write=False)
    return gold, pred


def degenerate_cases():
    """name -> (gold, pred, index of the column (b, d) that is special)."""
    out = {}
    g, p = (a.copy() for a in loss_case((2, 1, 2), 5))
    out["L=1"] = (g, p, None)
    g, p = (a.copy() for a in loss_case((2, 9, 3), 6))
    g[1, :, 1] = 0.25
    p[1, :, 1] = 0.25
    out["gold=pred=c"] = (g, p, (1, 1))
    g, p = (a.copy() for a in loss_case((2, 9, 3), 7))
    g[0, :, 2] = -0.5
    out["gold=c"] = (g, p, (0, 2))
    return out


@functools.lru_cache(maxsize=None)
def videos(seed=3):
    """[(trial, pred float32 [n], label float32 [n])] for VIDEO_FRAMES: pred = tanh(normal), label uniform in [-1, 1]."""
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(VIDEO_FRAMES):
        p = np.tanh(rng.standard_normal(n)).astype(np.float32)
        l = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        if n <= 3:                       # keep the two- and three-frame videos away from a vanishing variance
            p[:2] = [-0.6, 0.5]
            l[:2] = [0.7, -0.4]
        p.setflags(write=False)
        l.setflags(write=False)
        out.append((f"trial{i}", p, l))
    return tuple(out)


def moments64(pred, label):
    """-> (row [7] = n, mean_p, mean_l, M2_p, M2_l, C_pl, SSE; sum |terms| of each)."""
    p, l = np.asarray(pred, dtype=np.float64), np.asarray(label, dtype=np.float64)
    n = p.size
    dp, dl = p - p.mean(), l - l.mean()
    terms = [None, p / n, l / n, dp * dp, dl * dl, dp * dl, (p - l) ** 2]
    row = np.array([n, p.mean(), l.mean()] + [t.sum() for t in terms[3:]])
    mass = np.array([0.0] + [np.abs(t).sum() for t in terms[1:]])
    return row, mass


def moment_bound(n, mass):
    """Any-order summation of n terms in binary64, for the kernel's tree and numpy's pairwise sum alike:
    ``|error| <= (n - 1) 2^-53 sum |terms|`` each, so the two differ by at most twice that."""
    return 2.0 * (n - 1) * U * mass
