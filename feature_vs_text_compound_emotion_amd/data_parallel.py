"""Data parallelism over clips: one process per GPU, RCCL all-reduce over xGMI.

The reference has no distributed code at all; clips are
independent, so the path shards over clips with ONE exchange per step: the sum
of the trainable-parameter gradients (2.2-5.0 M floats = 9-20 MB, latency
bound on the xGMI mesh).  All gradients live in a single flat fp32 bucket:
``p.grad`` of every trainable parameter is a view into it, autograd accumulates
into the views in place, one ``all_reduce`` (RCCL picks direct/tree for this
size) covers the whole model, and the optimiser reads the same views -- no
flatten / unflatten copies.  The frozen encoders are replicated and exchange
nothing.

Semantics: each rank equals the single-process reference run on its shard of
the global batch, and the applied gradient is the mean over ranks
(== the gradient of the mean loss over the global batch when every rank holds
the same number of frames).  BatchNorm statistics stay local to the rank, like
torch DDP without SyncBN -- unless ``sync_bn`` is set: then every train-mode
BatchNorm of the encoder and the tail normalises with the statistics of the
GLOBAL batch (``BatchNormSync``), and N ranks x B/N clips compute the
single-process step on B clips.
"""
import os

import torch
import torch.distributed as dist

from . import ops
from .batchnorm import BatchNormLocal


def init_process_group_from_env(backend=None, single_rank_group=False):
    """RANK / WORLD_SIZE / LOCAL_RANK / MASTER_* come from the launcher (torch.distributed.run).  ``single_rank_group``:
    create the process group for WORLD_SIZE == 1 as well (a one-rank RCCL communicator is legal; the tests use it to drive
    the collectives' stream semantics on one GPU)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if (world > 1 or single_rank_group) and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        if backend is None:
            backend = "nccl" if torch.cuda.is_available() else "gloo"  # "nccl" is RCCL on ROCm
        if backend == "nccl":
            torch.cuda.set_device(local)
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    return rank, world, local


class BatchNormSync(BatchNormLocal):
    """Synchronised batch statistics for the train-mode BatchNorms of the HIP modules (``IR50``, ``LFAN``, ``CAN`` / ``JMT``),
    which call it in place of ``batchnorm.LOCAL`` while it is attached to them as ``bn_sync``: it overrides the statistics, the
    encoder finalize, the backward's sums (``global_sums``) and ``agree_min``.  The collectives run on a process group of
    their own, so they never interleave with the gradient slices that the overlapped exchange issues from autograd hooks on
    the default group; with RCCL they are stream-ordered (no host synchronisation).

    * encoder BatchNorm2d: float64 (sum, sum of squares) per channel, all-reduced, finalized over ``world x`` the local
      element count;
    * row BatchNorm1d forward: float64 (count, mean, M2) per rank, all-gathered and merged in rank order (identical bits on
      every rank; see cer_bn_rows_merge);
    * row BatchNorm1d backward: the float32 (sum dy, sum dy * x_hat) all-reduced, dx from the global sums over
      ``world x`` the local rows; dw and db stay the rank's own (the gradient all-reduce averages them);
    * released encoder units / stem / head (``sync_released``): the same exchanges over 0.8 M .. 51 M rows -- the moments of
      ``bn_rows_moments_large`` (one read of x), and the backward's fused split / addend apply passes from the global sums.

    The element counts assume equal shards (what ``ClipDataParallel.shard`` gives when the global batch divides by the
    world size) -- the same assumption under which the mean of the ranks' gradients is the full-batch gradient."""

    def __init__(self, group, world, rank):
        self.group, self.world, self.rank = group, world, rank

    def __deepcopy__(self, memo):
        return self      # a handle on the process group: a deep-copied model (best-model snapshots) shares it

    def _all_reduce(self, t):
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return t

    def encoder_finalize(self, partials, count, bn):
        """``ops.bn_finalize`` over the global batch: (scale, shift), running buffers updated with the global statistics."""
        sums = self._all_reduce(ops.bn_partial_sums(partials))
        return ops.bn_finalize_sums(sums, count * self.world, bn.weight.detach(), bn.bias.detach(), bn.running_mean,
                                    bn.running_var, momentum=bn.momentum, eps=bn.eps)

    def rows_stats(self, x, running_mean, running_var, eps, momentum, large=False):
        """``ops.bn_rows_stats`` over the global batch: (save_mean, save_invstd), the same bits on every rank, running buffers
        updated with the global statistics.  ``large``: dense rows of any size, read once (``bn_rows_moments_large``)."""
        local = ops.bn_rows_moments_large(x) if large else ops.bn_rows_moments(x)
        gathered = torch.empty((self.world * 3, local.shape[1]), device=local.device, dtype=local.dtype)
        dist.all_gather_into_tensor(gathered, local, group=self.group)
        return ops.bn_rows_merge(gathered.view(self.world, 3, -1), running_mean, running_var, eps, momentum)

    def rows_fwd(self, x, w, b, running_mean, running_var, eps, momentum, train=True, out=None, large=False):
        """``ops.bn_rows_fwd`` over the global batch in train mode: (y, save_mean, save_invstd)."""
        if not train:
            return super().rows_fwd(x, w, b, running_mean, running_var, eps, momentum, train=False, out=out)
        sm, si = self.rows_stats(x, running_mean, running_var, eps, momentum, large)
        return ops.bn_rows_apply(x, sm, si, w, b, out=out), sm, si

    def global_sums(self, sums, rows):
        """The ranks' backward sums all-reduced, over ``world x`` the local rows."""
        return self._all_reduce(sums.clone()), rows * self.world

    def agree_min(self, flag, device):
        """The minimum of an integer flag over the ranks (e.g. "this rank's memory fits the plan"), on the sync group."""
        t = torch.tensor([int(flag)], device=device, dtype=torch.int32)
        dist.all_reduce(t, op=dist.ReduceOp.MIN, group=self.group)
        return int(t.item())


def _bn_sync_owners(model):
    """The modules that run train-mode BatchNorms through HIP calls and read ``bn_sync``."""
    return [m for m in model.modules() if hasattr(type(m), "bn_sync")]


class ClipDataParallel:
    """Gradient bucket + collectives for a model whose trainable part is small."""

    def __init__(self, model, world_size=None, broadcast=True, overlap=False, bucket_mb=25.0, sync_bn=False,
                 sync_released=False):
        """``sync_bn``: train-mode BatchNorms of the encoder and the tail normalise with the statistics of the global batch
        (``BatchNormSync``; needs an initialised process group).  ``"force"`` runs the collectives with one rank too, like
        ``overlap="force"``.  Off by default: each rank's BatchNorms see its own shard.

        ``sync_released`` (needs ``sync_bn``): the RELEASED parts of the IR-50 encoder (the reference's gradual release:
        output layer, stage 4, half of stage 3 -- or the whole encoder) normalise with the global statistics too, forward and
        backward.  Off by default: with ``sync_bn`` alone a released encoder parameter is refused (NotImplementedError).

        ``overlap``: cut the flat bucket into slices of ``bucket_mb`` (in parameter order) and start the all-reduce of a
        slice from an autograd hook as soon as the last gradient of the slice has been accumulated -- backward produces
        the gradients from the top of the model down, so with released encoder units (28-43 M parameters, 112-172 MB) the
        exchange of the tail's and the upper units' gradients runs under the backward of the units below.  Needs ONE
        ``backward()`` per ``zero_grad()`` (the reference's training loop); off by default."""
        if sync_released and not sync_bn:
            raise ValueError("sync_released=True needs sync_bn (synchronised statistics of the released encoder units)")
        self.model = model
        self.world = world_size if world_size is not None else (dist.get_world_size() if dist.is_initialized() else 1)
        self.params = [p for p in model.parameters() if p.requires_grad]
        if not self.params:
            raise ValueError("model has no trainable parameter")
        dev = self.params[0].device
        total = (sum(p.numel() for p in self.params) + 3) // 4 * 4  # the fused optimiser works on float4
        self.flat = torch.zeros(total, device=dev, dtype=torch.float32)
        off = 0
        for p in self.params:
            p.grad = self.flat[off:off + p.numel()].view_as(p)
            off += p.numel()
        if broadcast and self.world > 1:
            self.broadcast_state()
        # independent dropout streams per rank: the models draw their masks from (dropout_seed, counter), and every rank
        # starts dropout_seed at 0 -- fold the rank in (2^20 steps apart)
        if self.world > 1 and dist.is_initialized() and hasattr(model, "dropout_seed"):
            model.dropout_seed += dist.get_rank() << 20
        # ``overlap="force"`` keeps the hook-driven slices on with ONE rank too (a single-rank RCCL communicator is legal):
        # the path the first multi-GPU run will take, exercised on one GPU (tests/test_rccl_single_rank_gpu.py)
        self.overlap = bool(overlap) and dist.is_initialized() and (self.world > 1 or overlap == "force")
        self._gathered = True          # p.grad are bucket views right now
        self.buckets, self._works = [], []
        if self.overlap:
            self._build_buckets(bucket_mb)
        self.bn_sync = None
        if sync_bn and (self.world > 1 or sync_bn == "force"):
            if not dist.is_initialized():
                raise RuntimeError("sync_bn needs an initialised process group (init_process_group_from_env)")
            self.bn_sync = BatchNormSync(dist.new_group(), dist.get_world_size(), dist.get_rank())
            for m in _bn_sync_owners(model):
                m.bn_sync = self.bn_sync
                if hasattr(type(m), "sync_released"):    # (IR50) a plain flag: deep copies of the model keep it
                    m.sync_released = bool(sync_released)

    # ------------------------------------------------------------------ bucketed, overlapped exchange
    def _build_buckets(self, bucket_mb):
        cap = max(1, int(bucket_mb * (1 << 20)) // 4)
        start = off = 0
        count = 0
        index_of = []
        for p in self.params:
            if count and off + p.numel() - start > cap:
                self.buckets.append([start, off, count])
                start, count = off, 0
            index_of.append(len(self.buckets))
            off += p.numel()
            count += 1
        self.buckets.append([start, off, count])
        self._pending = [b[2] for b in self.buckets]
        self._launched = [False] * len(self.buckets)
        self._next = len(self.buckets) - 1
        for p, b in zip(self.params, index_of):
            p.register_post_accumulate_grad_hook(self._make_hook(b))

    def _make_hook(self, b):
        def hook(_param):
            self._pending[b] -= 1
            self._launch_ready()
        return hook

    def _launch_ready(self):
        """Collectives are issued STRICTLY in reverse slice order (last slice first, what a top-down backward completes
        first anyway): slice b goes out only when every slice above it has.  The issue order is then the same on every rank
        even when a parameter gets no gradient on one of them (a data-dependent branch, a modality absent from a shard) --
        that rank's slice, and everything below it, simply waits for ``all_reduce_gradients`` -- instead of following each
        rank's own autograd firing order, which would pair differently sized collectives across ranks."""
        while self._next >= 0 and self._pending[self._next] == 0:
            self._launch(self._next)
            self._next -= 1

    def _launch(self, b):
        s, e, _ = self.buckets[b]
        self._launched[b] = True
        self._works.append(dist.all_reduce(self.flat[s:e], op=dist.ReduceOp.SUM, async_op=True))

    def broadcast_state(self, src=0):
        """Replicate rank ``src``'s parameters and buffers (one flat message each).  The copies go through the tensors
        themselves (not ``.data``), so their version counters move and every packed-weight cache keyed on
        (data_ptr, _version) -- IR50.pack*, the VGGish / BERT caches -- is rebuilt on the next forward."""
        for tensors in (list(self.model.parameters()), [b for b in self.model.buffers() if b.dtype == torch.float32]):
            if not tensors:
                continue
            flat = torch.cat([t.detach().reshape(-1) for t in tensors])
            dist.broadcast(flat, src)
            off = 0
            with torch.no_grad():
                for t in tensors:
                    t.copy_(flat[off:off + t.numel()].view_as(t))
                    off += t.numel()

    def sync_buffers(self, mode="mean", force=False):
        """BatchNorm running statistics are rank-local during training (each rank == the reference on its shard).  Before
        a checkpoint or an evaluation make them one set again: ``mean`` averages the float buffers over the ranks (every
        shard's statistics count), ``broadcast`` takes rank 0's.  Integer buffers (num_batches_tracked) are equal already."""
        if self.world == 1 and not (force and dist.is_initialized()):   # ``force``: run the collective with one rank too (tests)
            return
        bufs = [b for b in self.model.buffers() if b.dtype == torch.float32]
        if not bufs:
            return
        flat = torch.cat([b.detach().reshape(-1) for b in bufs])
        if mode == "mean":
            dist.all_reduce(flat, op=dist.ReduceOp.SUM)
            flat.mul_(1.0 / self.world)
        elif mode == "broadcast":
            dist.broadcast(flat, 0)
        else:
            raise ValueError(mode)
        off = 0
        with torch.no_grad():
            for b in bufs:
                b.copy_(flat[off:off + b.numel()].view_as(b))
                off += b.numel()

    def zero_grad(self):
        """Overlapped exchange: the bucket is zeroed and every ``p.grad`` is (again) a view into it, so autograd accumulates in
        place and the slice hooks see the gradients land.  Otherwise (round 3): ``p.grad = None`` -- autograd then ADOPTS the
        gradient tensor a backward function returns instead of launching one ``grad += g`` kernel per parameter (102 launches
        of ~2 us work each per step for the tri-modal LFAN tail), and ``gather_gradients()`` moves them into the bucket with a
        few multi-tensor copies before the all-reduce / the fused optimiser reads it."""
        if not self.overlap:
            for p in self.params:
                p.grad = None
            self._gathered = False
            return
        self.flat.zero_()
        self._pending = [b[2] for b in self.buckets]
        self._launched = [False] * len(self.buckets)
        self._next = len(self.buckets) - 1
        self._works = []
        self._gathered = True
        off = 0
        for p in self.params:
            if p.grad is None or p.grad.data_ptr() != self.flat.data_ptr() + 4 * off:
                p.grad = self.flat[off:off + p.numel()].view_as(p)
            off += p.numel()

    def gather_gradients(self):
        """Bring every parameter's gradient into the flat bucket (a no-op when they already live there) and make ``p.grad`` the
        bucket views again; parameters that received no gradient read as zeros.  Idempotent per ``zero_grad()``."""
        if getattr(self, "_gathered", True):
            return
        base = self.flat.data_ptr()
        dsts, srcs, zeros, off = [], [], [], 0
        views = []
        for p in self.params:
            v = self.flat[off:off + p.numel()].view_as(p)
            views.append(v)
            g = p.grad
            if g is None:
                zeros.append(v)
            elif g.data_ptr() != base + 4 * off:
                dsts.append(v)
                srcs.append(g if g.dtype == torch.float32 else g.float())
            off += p.numel()
        if off < self.flat.numel():
            zeros.append(self.flat[off:])
        with torch.no_grad():
            if dsts:
                torch._foreach_copy_(dsts, srcs)
            if zeros:
                torch._foreach_zero_(zeros)
        for p, v in zip(self.params, views):
            p.grad = v
        self._gathered = True

    def all_reduce_gradients(self):
        """Mean of the gradients over ranks, in place in the bucket."""
        self.gather_gradients()
        if self.world > 1 or self.overlap:
            if self.overlap:
                while self._next >= 0:   # slices at / below one whose parameters got no gradient this step, same order
                    self._launch(self._next)
                    self._next -= 1
                for w in self._works:
                    w.wait()
                self._works = []
            else:
                dist.all_reduce(self.flat, op=dist.ReduceOp.SUM)
            self.flat.mul_(1.0 / self.world)

    def flatten_parameters(self):
        """Re-home every trainable parameter in ONE flat fp32 buffer (same order and padding as the gradient bucket) so
        that the optimiser update is a single launch.  ``p.data`` becomes a view; values are preserved."""
        if getattr(self, "flat_param", None) is None:
            self.flat_param = torch.empty_like(self.flat)
            off = 0
            for p in self.params:
                view = self.flat_param[off:off + p.numel()].view_as(p)
                view.copy_(p.data)
                p.data = view
                off += p.numel()
            self.flat_param[off:].zero_()
        return self.flat_param

    def shard(self, global_batch_indices, rank):
        """Distributed-sampler rule: rank r takes clips r::world of every global batch."""
        return global_batch_indices[rank::self.world]


class _FlatOptimizer(torch.optim.Optimizer):
    """A ``torch.optim.Optimizer`` over ``ddp.params`` whose update is one HIP launch over the flat parameter / gradient
    buffers of a ``ClipDataParallel``.  Being an ``Optimizer`` is what lets torch's schedulers (and the reference's
    ``MyStepLR`` / ``MyCosineLR``, base/scheduler.py:167-256) drive it: they type-check for it and read / write
    ``param_groups[*]['lr']`` and ``initial_lr``.  The state lives in flat buffers, not in ``self.state``, so ``state_dict``
    / ``load_state_dict`` are the subclasses' own.

    Loss scaling: ``_step_supports_amp_scaling`` makes ``torch.amp.GradScaler.step`` hand the update ``grad_scale`` and
    ``found_inf`` as device tensors (attributes set around ``step()``) instead of reading ``found_inf`` on the host; the update
    then unscales and skips on the device (``ops.*_flat_amp``).  The applied-step count those launches need lives on the
    device (``_applied``, int64) from the first such step on; ``steps`` reads it (one host read) and a plain step folds it
    back into the host count."""

    _step_supports_amp_scaling = True

    def __init__(self, ddp, defaults):
        super().__init__(ddp.params, defaults)
        self.ddp = ddp
        self.flat_param = ddp.flatten_parameters()
        self._steps, self._applied, self._amp_bound = 0, None, 0

    @property
    def steps(self):
        """Applied steps (skipped loss-scaled steps do not count).  A host read once a loss-scaled step has run."""
        return self._steps if self._applied is None else int(self._applied.item())

    @steps.setter
    def steps(self, value):
        self._steps, self._applied = int(value), None

    def _amp_state(self):
        """(grad_scale, found_inf) when a GradScaler drives this step, else None.  GradScaler sets ``found_inf`` always and
        ``grad_scale`` unless the gradients were unscaled already (an explicit ``scaler.unscale_(opt)``)."""
        found_inf = getattr(self, "found_inf", None)
        if found_inf is None:
            return None
        grad_scale = getattr(self, "grad_scale", None)
        if grad_scale is not None:
            grad_scale = grad_scale.reshape(1).to(torch.float32)
        return grad_scale, found_inf.reshape(1).to(torch.float32)

    def _device_applied(self):
        """The device-resident applied-step counter, started from the host count (a fill launch, no host read); advances
        ``_amp_bound``, the host's upper bound of the count after this step."""
        if self._applied is None:
            self._applied = torch.full((1,), self._steps, dtype=torch.int64, device=self.flat_param.device)
            self._amp_bound = self._steps
        self._amp_bound += 1
        return self._applied

    def _fold_applied(self):
        """Before a plain step: bring a device-resident count back to the host (no-op unless a loss-scaled step ran)."""
        if self._applied is not None:
            self.steps = self.steps

    def zero_grad(self, set_to_none=False):
        self.ddp.zero_grad()

    def _bump_versions(self):
        # the kernel wrote through raw pointers: move the version counters like an in-place torch op would, so caches keyed
        # on (data_ptr, _version) see the update.  Semantics note: every trainable parameter always has a (dense) gradient
        # view in the bucket, so weight decay and momentum apply to all of them every step -- torch's optimisers skip a
        # parameter whose grad is None after zero_grad(set_to_none=True); the two only differ for a parameter that
        # receives no gradient at all in a step, which the models here do not have.
        torch.autograd.graph.increment_version(self.ddp.params)

    def _groups_state(self):
        return [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]

    def _load_groups(self, sd):
        for g, h in zip(self.param_groups, sd["param_groups"]):
            g.update(h)


class FlatNesterovSGD(_FlatOptimizer):
    """torch.optim.SGD(momentum, nesterov, weight_decay) of the reference (instantiators.py:74-92) as ONE HIP launch over
    the flat parameter / gradient / momentum buffers of a ``ClipDataParallel`` (bit-identical arithmetic, tested against
    torch.optim.SGD).  ``param_groups[0]['lr']`` is what the reference's scheduler mutates (base/scheduler.py:167-197)."""

    def __init__(self, ddp, lr=1e-3, momentum=0.9, dampening=0.0, weight_decay=1e-4, nesterov=True):
        super().__init__(ddp, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                   nesterov=nesterov))
        self.buf = torch.zeros_like(self.flat_param)

    def step(self):
        from . import ops
        self.ddp.gather_gradients()
        g = self.param_groups[0]
        amp = self._amp_state()
        if amp is not None:
            ops.sgd_nesterov_flat_amp(self.flat_param, self.ddp.flat, self.buf, g["lr"], *amp, self._device_applied(),
                                      momentum=g["momentum"], dampening=g["dampening"], weight_decay=g["weight_decay"],
                                      nesterov=g["nesterov"])
            self._bump_versions()
            return
        self._fold_applied()
        ops.sgd_nesterov_flat(self.flat_param, self.ddp.flat, self.buf, g["lr"], g["momentum"], g["dampening"],
                              g["weight_decay"], g["nesterov"], first_step=self.steps == 0)
        self.steps += 1
        self._bump_versions()

    def state_dict(self):
        return {"momentum_buffer": self.buf, "steps": self.steps, "param_groups": self._groups_state()}

    def load_state_dict(self, sd):
        self.buf.copy_(sd["momentum_buffer"])
        self.steps = int(sd["steps"])
        self._load_groups(sd)


class FlatAdam(_FlatOptimizer):
    """torch.optim.Adam(betas, eps, weight_decay, amsgrad) of the reference (instantiators.py:81-92; L2 weight decay, not
    AdamW) as ONE HIP launch over the flat buffers of a ``ClipDataParallel`` plus flat moment buffers beside them.  Per
    element the arithmetic is the non-capturable branch of torch's ``_multi_tensor_adam``; ``steps`` is the one step count
    of all parameters (torch keeps one per parameter, all equal here)."""

    def __init__(self, ddp, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False):
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid betas: {betas}")
        super().__init__(ddp, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad))
        self.exp_avg = torch.zeros_like(self.flat_param)
        self.exp_avg_sq = torch.zeros_like(self.flat_param)
        self.max_exp_avg_sq = torch.zeros_like(self.flat_param) if amsgrad else None
        self._bias, self._bias_betas, self._bias_saturated = None, None, False

    def _bias_table(self, betas, need):
        """[T, 2] float64 on the device: (1 - b1^k, sqrt(1 - b2^k)) for k = 1..T, computed with the Python-float arithmetic
        torch.optim.Adam uses (and cer_adam_flat's std::pow), T >= ``need`` -- or shorter once both columns have reached 1.0,
        after which every later k has the same entry (the kernel clamps k to T).  Grown by doubling; the copy goes from
        pinned memory without a host synchronisation."""
        b1, b2 = float(betas[0]), float(betas[1])
        if self._bias is not None and self._bias_betas == (b1, b2) and (self._bias.shape[0] >= need or self._bias_saturated):
            return self._bias
        cap = max(need, 1024, 2 * (self._bias.shape[0] if self._bias is not None and self._bias_betas == (b1, b2) else 0))
        rows = []
        for k in range(1, cap + 1):
            rows.append((1 - b1 ** k, (1 - b2 ** k) ** 0.5))
            if rows[-1] == (1.0, 1.0):
                break
        self._bias_saturated = rows[-1] == (1.0, 1.0)
        host = torch.tensor(rows, dtype=torch.float64).pin_memory()
        self._bias = host.to(self.flat_param.device, non_blocking=True)
        self._bias_betas = (b1, b2)
        return self._bias

    def step(self):
        from . import ops
        self.ddp.gather_gradients()
        g = self.param_groups[0]
        amp = self._amp_state()
        if amp is not None:
            applied = self._device_applied()       # _amp_bound: the largest step number this launch can use
            ops.adam_flat_amp(self.flat_param, self.ddp.flat, self.exp_avg, self.exp_avg_sq, self.max_exp_avg_sq, g["lr"],
                              self._bias_table(g["betas"], self._amp_bound), *amp, applied, betas=g["betas"], eps=g["eps"],
                              weight_decay=g["weight_decay"], amsgrad=g["amsgrad"])
            self._bump_versions()
            return
        self._fold_applied()
        ops.adam_flat(self.flat_param, self.ddp.flat, self.exp_avg, self.exp_avg_sq, self.max_exp_avg_sq, g["lr"],
                      self.steps + 1, betas=g["betas"], eps=g["eps"], weight_decay=g["weight_decay"], amsgrad=g["amsgrad"])
        self.steps += 1
        self._bump_versions()

    def state_dict(self):
        sd = {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq, "steps": self.steps,
              "param_groups": self._groups_state()}
        if self.max_exp_avg_sq is not None:
            sd["max_exp_avg_sq"] = self.max_exp_avg_sq
        return sd

    def load_state_dict(self, sd):
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        if self.max_exp_avg_sq is not None:
            self.max_exp_avg_sq.copy_(sd["max_exp_avg_sq"])
        self.steps = int(sd["steps"])
        self._load_groups(sd)


class FlatGradScaler(torch.amp.GradScaler):
    """``torch.amp.GradScaler`` whose gradient check / unscale is ONE launch over the flat bucket of a ``_FlatOptimizer``
    (``ops.amp_check_unscale_flat``) instead of torch's foreach chain over the per-parameter views; any other optimiser goes
    through torch's own route.  With the flat optimisers' ``_step_supports_amp_scaling``, ``step`` then hands ``grad_scale``
    and ``found_inf`` to the fused update as device tensors, so ``scale -> backward -> step -> update`` reads nothing back to
    the host.  ``update`` is torch's (``_amp_update_scale_``): the scale trajectory is torch's by construction.

    Data parallel: call ``ddp.all_reduce_gradients()`` between ``backward`` and ``step``.  The check then runs on the
    all-reduced bucket, and since the all-reduce SUMS the ranks' buckets, a non-finite gradient on any rank is non-finite on
    every rank: all ranks find the same ``found_inf``, skip the same steps and move their scales in lockstep, without a
    collective of their own."""

    def _unscale_grads_(self, optimizer, inv_scale, found_inf, allow_fp16):
        """``unscale_()`` (explicit, e.g. before clipping): check and unscale the bucket; the following ``step`` gets
        ``grad_scale=None`` and only skips."""
        if not isinstance(optimizer, _FlatOptimizer):
            return super()._unscale_grads_(optimizer, inv_scale, found_inf, allow_fp16)
        from . import ops
        optimizer.ddp.gather_gradients()
        ops.amp_check_unscale_flat(optimizer.ddp.flat, found_inf.reshape(1), inv_scale.reshape(1))
        return {found_inf.device: found_inf}

    def _check_inf_per_device(self, optimizer):
        """``step()`` without a preceding ``unscale_()``: check only (the bucket is not written; the fused update unscales)."""
        if not isinstance(optimizer, _FlatOptimizer):
            return super()._check_inf_per_device(optimizer)
        from . import ops
        scale, _ = self._check_scale_growth_tracker("_check_inf_per_device")
        found_inf = torch.full((), 0.0, dtype=torch.float32, device=scale.device)
        optimizer.ddp.gather_gradients()
        ops.amp_check_unscale_flat(optimizer.ddp.flat, found_inf.reshape(1))
        self._per_optimizer_states[id(optimizer)]["found_inf_per_device"] = {found_inf.device: found_inf}
        return self._per_optimizer_states[id(optimizer)]["found_inf_per_device"]
