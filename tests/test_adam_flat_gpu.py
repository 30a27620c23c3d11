"""Fused flat Adam (``FlatAdam`` -> ``cer_adam_flat``) vs torch.optim.Adam (the reference's other optimiser,
instantiators.py:81-92), state round trip, and lr schedulers driving the flat optimisers, alone and through
``Trainer`` with ``data_parallel``."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "schedulers.npz")
ULP1 = 2.0 ** -23        # ulp(x) <= ULP1 * |x| in fp32

# Exactness.  Per element the kernel runs the operation sequence of torch's _multi_tensor_adam (non-capturable branch) with
# every rounding spelled out, and the step terms come from the host in double as in torch's Python code.  The only freedom
# torch's kernels have is whether a*b+c is contracted (lerp, addcmul, the weight-decay add, addcdiv); the kernel contracts
# all four, and on the MI355X with this torch build the result is bit-identical to torch.optim.Adam (foreach), so the
# Adam comparisons below assert torch.equal.  Were torch's kernels not to contract, a step would move p by u = step_size *
# m / denom with an error of at most ~1 ulp of |p| plus a few ulp of |u|, i.e. within 4 ulp(|p|) + 4 ulp(|u|) per step,
# accumulating over the steps (PER_STEP_ULPS, still used for the SGD comparison, whose reference is torch's SGD as in
# test_optim_gpu.py).
PER_STEP_ULPS = 4.0


class _Toy(torch.nn.Module):
    def __init__(self, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.a = torch.nn.Parameter(torch.randn(37, 5, generator=g))
        self.b = torch.nn.Parameter(torch.randn(129, generator=g))
        self.c = torch.nn.Parameter(torch.randn(4, 3, 5, generator=g))  # total 374: not a multiple of 4


def _fixture(name):
    d = np.load(GOLDEN)
    return json.loads(str(d[f"{name}_config"])), d[f"{name}_lr"]


def _set_grads(models, g):
    for ps in zip(*[m.parameters() for m in models]):
        grad = torch.randn(ps[0].shape, generator=g).cuda()
        for p in ps:
            p.grad = grad.clone()


@pytest.mark.parametrize("amsgrad", [False, True])
@pytest.mark.parametrize("wd", [0.0, 1e-4])
def test_flat_adam_matches_torch_adam(wd, amsgrad):
    from feature_vs_text_compound_emotion_amd.data_parallel import ClipDataParallel, FlatAdam
    ref, mine = _Toy(1).cuda(), _Toy(1).cuda()
    opt_ref = torch.optim.Adam(ref.parameters(), lr=1e-3, weight_decay=wd, amsgrad=amsgrad)   # GPU default: foreach
    opt = FlatAdam(ClipDataParallel(mine, world_size=1, broadcast=False), lr=1e-3, weight_decay=wd, amsgrad=amsgrad)
    g = torch.Generator().manual_seed(2)
    for step in range(50):
        if step == 20:
            opt_ref.param_groups[0]["lr"] = opt.param_groups[0]["lr"] = 3e-4
        opt_ref.zero_grad()
        opt.zero_grad()
        _set_grads([ref, mine], g)
        opt_ref.step()
        opt.step()
        for pr, pm in zip(ref.parameters(), mine.parameters()):
            assert torch.equal(pr, pm), (step, (pr - pm).abs().max().item())
    keys = ["exp_avg", "exp_avg_sq"] + (["max_exp_avg_sq"] if amsgrad else [])
    for pr, pm in zip(ref.parameters(), mine.parameters()):
        off = (pm.data_ptr() - opt.flat_param.data_ptr()) // 4
        for k in keys:
            assert torch.equal(getattr(opt, k)[off:off + pm.numel()].view_as(pm), opt_ref.state[pr][k]), k
    assert opt.steps == 50 and mine.a.data_ptr() == opt.flat_param.data_ptr()


def test_flat_adam_state_dict_round_trip():
    from feature_vs_text_compound_emotion_amd.data_parallel import ClipDataParallel, FlatAdam
    a, b = _Toy(3).cuda(), _Toy(3).cuda()
    opt_a = FlatAdam(ClipDataParallel(a, world_size=1, broadcast=False), weight_decay=1e-4, amsgrad=True)
    g = torch.Generator().manual_seed(4)
    for _ in range(7):
        opt_a.zero_grad()
        _set_grads([a], g)
        opt_a.step()
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt_a.state_dict().items()}
    with torch.no_grad():
        for pa, pb in zip(a.parameters(), b.parameters()):
            pb.copy_(pa)
    opt_b = FlatAdam(ClipDataParallel(b, world_size=1, broadcast=False), weight_decay=1e-4, amsgrad=True)
    opt_b.load_state_dict(sd)
    assert opt_b.steps == 7
    opt_a.zero_grad()
    opt_b.zero_grad()
    _set_grads([a, b], g)
    opt_a.step()
    opt_b.step()
    assert torch.equal(opt_a.flat_param, opt_b.flat_param)
    for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
        assert torch.equal(getattr(opt_a, k), getattr(opt_b, k))


@pytest.mark.parametrize("sched", ["MYSTEP", "COSINE"])
@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_schedulers_drive_the_flat_optimisers(kind, sched):
    from feature_vs_text_compound_emotion_amd.data_parallel import ClipDataParallel, FlatAdam, FlatNesterovSGD
    from feature_vs_text_compound_emotion_amd.trainer import make_lr_scheduler
    cfg, lrs = _fixture(sched)
    ref, mine = _Toy(5).cuda(), _Toy(5).cuda()
    ddp = ClipDataParallel(mine, world_size=1, broadcast=False)
    if kind == "sgd":
        opt = FlatNesterovSGD(ddp)
        opt_ref = torch.optim.SGD(ref.parameters(), momentum=0.9, weight_decay=1e-4, nesterov=True)
    else:
        opt = FlatAdam(ddp, weight_decay=1e-4)
        opt_ref = torch.optim.Adam(ref.parameters(), weight_decay=1e-4)
    assert isinstance(opt, torch.optim.Optimizer)
    s, s_ref = make_lr_scheduler(opt, cfg), make_lr_scheduler(opt_ref, cfg)
    g = torch.Generator().manual_seed(6)
    tol = [torch.zeros_like(p) for p in ref.parameters()]
    for epoch in range(25):      # the MYSTEP floor binds from epoch 20
        assert opt.param_groups[0]["lr"] == lrs[epoch] == opt_ref.param_groups[0]["lr"], epoch
        opt.zero_grad()
        opt_ref.zero_grad()
        _set_grads([ref, mine], g)
        before = [p.detach().clone() for p in ref.parameters()]
        opt.step()               # uses the scheduled lr: checked against torch's optimiser under the same schedule
        opt_ref.step()
        for t, b, pr, pm in zip(tol, before, ref.parameters(), mine.parameters()):
            if kind == "adam":
                assert torch.equal(pr, pm), (epoch, (pr - pm).abs().max().item())
            else:
                t += PER_STEP_ULPS * ULP1 * (pr.detach().abs() + (pr.detach() - b).abs())
                assert ((pr - pm).abs() <= t).all(), (epoch, (pr - pm).abs().max().item())
        s.step()
        s_ref.step()


class _Tail(torch.nn.Module):
    """A small trainable head over the VGGish features: 2183 parameters (not a multiple of 4)."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(11)
        self.l1 = torch.nn.Linear(128, 16)
        self.l2 = torch.nn.Linear(16, 7)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)

    def forward(self, X):
        return self.l2(torch.relu(self.l1(X["vggish"][:, 0])))


def _loaders():
    g = torch.Generator().manual_seed(0)
    w_true = torch.randn(128, 7, generator=g)

    def clips(n_clips, length, batch):
        out = []
        for i in range(0, n_clips, batch):
            x = torch.randn(batch, 1, length, 128, generator=g)
            y = (x[:, 0].mean(1) @ w_true).argmax(-1).view(batch, 1, 1).expand(batch, length, 1).float().contiguous()
            out.append(({"vggish": x, "EXPR_continuous_label": y}, [f"c{i + j}" for j in range(batch)], [length] * batch,
                        [np.arange(length)] * batch))
        return out
    return {"train": clips(8, 6, 2), "valid": clips(3, 9, 1)}       # no test split: optimize() keeps the last weights


def _train(optimizer, data_parallel):
    from feature_vs_text_compound_emotion_amd.data_parallel import ClipDataParallel
    from feature_vs_text_compound_emotion_amd.trainer import Trainer
    model = _Tail().cuda()
    ddp = ClipDataParallel(model, world_size=1, broadcast=False) if data_parallel else None
    tr = Trainer(model, device="cuda", data_parallel=ddp, train_batch_size=2, max_epoch=3)
    # the reference's literal constants (default_config.py:91,103)
    tr.set_args(SimpleNamespace(opt__name_optimizer=optimizer, opt__momentum=0.9, opt__dampening=0.0,
                                opt__nesterov=True, opt__weight_decay=1e-4, opt__beta1=0.9, opt__beta2=0.999,
                                opt__eps_adam=1e-8, opt__amsgrad=False, opt__lr_scheduler=True,
                                opt__name_lr_scheduler="MYSTEP", opt__step_size=1, opt__gamma=0.5, opt__last_epoch=-1,
                                opt__min_lr=1e-7))
    tr.init_optimizer_and_scheduler(epoch=0)
    hist = tr.optimize(_loaders())
    assert len(hist["loss"]) == 3
    return tr, model


def test_trainer_data_parallel_follows_the_schedule():
    from feature_vs_text_compound_emotion_amd.data_parallel import FlatNesterovSGD
    tr, _ = _train("SGD", data_parallel=True)
    assert isinstance(tr.optimizer, FlatNesterovSGD)
    assert tr.scheduler is not None and tr.optimizer.param_groups[0]["lr"] == 1e-3 * 0.5 ** 3


def test_trainer_data_parallel_adam_matches_single_process_adam():
    from feature_vs_text_compound_emotion_amd.data_parallel import FlatAdam
    tr, model = _train("ADAM", data_parallel=True)
    tr_ref, model_ref = _train("ADAM", data_parallel=False)
    assert isinstance(tr.optimizer, FlatAdam) and type(tr_ref.optimizer) is torch.optim.Adam
    assert tr.optimizer.param_groups[0]["lr"] == tr_ref.optimizer.param_groups[0]["lr"] == 1e-3 * 0.5 ** 3
    steps = tr.optimizer.steps
    assert steps == 12
    for pm, pr in zip(model.parameters(), model_ref.parameters()):
        assert torch.equal(pm, pr), (pm - pr).abs().max().item()   # same gradients, bit-identical update every step
