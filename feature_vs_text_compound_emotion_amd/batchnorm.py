"""Where the batch statistics of the HIP modules' BatchNorms come from.

``BatchNormLocal`` takes them over this process's own batch with the one-call ops; ``data_parallel.BatchNormSync``
overrides the statistics and the backward's sums with those of the global batch.  The modules (``IR50`` and its released
units, ``LFAN``, ``CAN`` / ``JMT``) call one of these objects and never branch on which it is: their ``bn_sync`` when it
applies, else ``LOCAL``.
"""
import torch

from . import ops


class BatchNormLocal:
    """Statistics of the local batch: ``ops.bn_finalize``, ``ops.bn_rows_stats`` / ``ops.bn_rows_fwd`` and the row backward
    over the local rows."""

    def encoder_finalize(self, partials, count, bn):
        """Encoder BatchNorm2d ``bn`` from the [tiles,2,C] partial sums over ``count`` elements: (scale, shift), running
        buffers updated."""
        return ops.bn_finalize(partials, count, bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var,
                               momentum=bn.momentum, eps=bn.eps)

    def rows_stats(self, x, running_mean, running_var, eps, momentum, large=False):
        """Train-mode statistics of the rows of x [R,C]: (save_mean, save_invstd), running buffers updated.  ``large``: the
        released encoder units' dense rows (0.8 M .. 51 M of them)."""
        return ops.bn_rows_stats(x, running_mean, running_var, eps, momentum)

    def rows_fwd(self, x, w, b, running_mean, running_var, eps, momentum, train=True, out=None, large=False):
        """Row BatchNorm: (y, save_mean, save_invstd).  In eval mode the saves are the statistics the running buffers
        gave, (running_mean, 1 / sqrt(running_var + eps)), which the eval-mode backward reads."""
        y, sm, si = ops.bn_rows_fwd(x, w, b, running_mean, running_var, train, eps, momentum, out=out)
        if not train:
            sm, si = running_mean, torch.rsqrt(running_var + eps)
        return y, sm, si

    def rows_bwd(self, dy, x, save_mean, save_invstd, w, train=True, split_out=False, add=None):
        """``ops.bn_rows_bwd`` with dx over the rows that ``global_sums`` gives (train mode): (dx, dw, db), dw / db of the
        local rows."""
        return ops._bn_rows_bwd(dy, x, save_mean, save_invstd, w, train, split_out, add, self.global_sums)

    def global_sums(self, sums, rows):
        """The backward's [2,C] (sum dy, sum dy * x_hat) over ``rows`` local rows -> (sums, row count) that dx is taken over."""
        return sums, rows

    def agree_min(self, flag, device):
        """The minimum of an integer flag over the processes that share the statistics (e.g. "this memory plan fits")."""
        return int(flag)


LOCAL = BatchNormLocal()
