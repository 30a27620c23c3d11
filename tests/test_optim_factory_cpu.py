"""The reference's optimiser / lr-scheduler factory (instantiators.py:62-185, base/scheduler.py:167-256) as
``Trainer.init_optimizer_and_scheduler`` builds it from the reference's own argument values, and the argument checks of
the fused flat Adam (no GPU needed)."""
import ctypes
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from feature_vs_text_compound_emotion_amd.trainer import Trainer

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "schedulers.npz")


def _fixture():
    d = np.load(GOLDEN)
    return {str(k): (json.loads(str(d[f"{k}_config"])), d[f"{k}_lr"]) for k in d["names"]}


def _trainer(**opt):
    tr = Trainer(torch.nn.Linear(4, 3), device="cpu")
    tr.set_args(SimpleNamespace(**{f"opt__{k}": v for k, v in opt.items()}))
    tr.init_optimizer_and_scheduler(epoch=0)
    return tr


def _lr_sequence(tr, epochs):
    out = []
    for _ in range(epochs):
        out.append(tr.optimizer.param_groups[0]["lr"])
        tr.optimizer.step()
        tr.scheduler.step()
    return np.asarray(out, dtype=np.float64)


# default_config.py:89-110, the literal constants included
REFERENCE_OPT = dict(weight_decay=1e-4, name_optimizer="SGD", lr=1e-3, momentum=0.9, dampening=0.0, nesterov=True,
                     beta1=0.9, beta2=0.999, eps_adam=1e-8, amsgrad=False, lr_scheduler=True, name_lr_scheduler="MYSTEP",
                     gamma=0.1, step_size=40, last_epoch=-1, min_lr=1e-7, t_max=100)


def test_reference_constants_build_sgd_and_the_floored_step_schedule():
    cfg, lrs = _fixture()["MYSTEP"]
    tr = _trainer(**{**REFERENCE_OPT, **cfg})
    assert type(tr.optimizer) is torch.optim.SGD and tr.optimizer.defaults["nesterov"]
    assert tr.optimizer.defaults["lr"] == 1e-3
    got = _lr_sequence(tr, len(lrs))
    assert np.array_equal(got, lrs), (got, lrs)
    assert lrs[-1] == cfg["min_lr"]       # the floor binds in the fixture


@pytest.mark.parametrize("optimizer,cls", [("SGD", torch.optim.SGD), ("ADAM", torch.optim.Adam), ("adam", torch.optim.Adam)])
@pytest.mark.parametrize("sched", ["STEP", "MYSTEP", "COSINE", "MYCOSINE", "MULTISTEP"])
def test_every_scheduler_matches_the_reference_sequence(optimizer, cls, sched):
    cfg, lrs = _fixture()[sched]
    tr = _trainer(**{**REFERENCE_OPT, "name_optimizer": optimizer, **cfg})
    assert type(tr.optimizer) is cls
    got = _lr_sequence(tr, len(lrs))
    assert np.array_equal(got, lrs), (sched, got, lrs)


def test_reference_default_config_runs_as_is():
    tr = _trainer(**REFERENCE_OPT)
    assert tr.scheduler is not None
    assert _lr_sequence(tr, 41)[-1] == pytest.approx(1e-4, rel=1e-12)   # gamma 0.1 every 40 epochs


def test_adam_reads_the_reference_hyper_parameters():
    tr = _trainer(**{**REFERENCE_OPT, "name_optimizer": "ADAM", "beta1": 0.8, "beta2": 0.99, "eps_adam": 1e-6,
                     "amsgrad": True})
    d = tr.optimizer.defaults
    assert d["betas"] == (0.8, 0.99) and d["eps"] == 1e-6 and d["amsgrad"] and d["weight_decay"] == 1e-4
    assert d["lr"] == 1e-3


@pytest.mark.parametrize("sched,key", [("MYCOSINE", "coef"), ("MYCOSINE", "max_epochs"), ("MULTISTEP", "milestones")])
def test_missing_scheduler_keys_are_named(sched, key):
    cfg = dict(_fixture()[sched][0])
    del cfg[key]
    with pytest.raises(ValueError, match=f"opt__{key}"):
        _trainer(**{**REFERENCE_OPT, **cfg})


def test_warmup_scheduler_is_refused_with_the_reason():
    with pytest.raises(NotImplementedError, match="MYWARMUP.*step"):
        _trainer(**{**REFERENCE_OPT, "name_lr_scheduler": "MYWARMUP"})


def test_unknown_names_are_refused():
    with pytest.raises(ValueError, match="RMSPROP"):
        _trainer(**{**REFERENCE_OPT, "name_optimizer": "RMSPROP"})
    with pytest.raises(ValueError, match="PLATEAU"):
        _trainer(**{**REFERENCE_OPT, "name_lr_scheduler": "PLATEAU"})


def test_no_scheduler_when_not_requested():
    tr = _trainer(**{**REFERENCE_OPT, "lr_scheduler": False})
    assert tr.scheduler is None


def test_adam_flat_argument_checks_need_no_gpu():
    """The checks run before any launch, so host addresses serve as stand-ins (test_abi_cpu.py does the same)."""
    from feature_vs_text_compound_emotion_amd import _lib
    lib = _lib.load()
    hp = (1e-3, 0.9, 0.999, 1e-8, 0.0)
    assert lib.cer_adam_flat(None, None, None, None, None, 8, *hp, 0, 1, None) == -1
    assert b"adam_flat" in lib.cer_last_error()
    host = (ctypes.c_float * 16)()
    p = ctypes.addressof(host)
    p += (-p) % 16                                  # 16-byte aligned, 12 floats left
    assert lib.cer_adam_flat(p, p, p, p, None, 6, *hp, 0, 1, None) == -1        # n % 4 != 0
    assert b"adam_flat" in lib.cer_last_error() and b"multiple of 4" in lib.cer_last_error()
    assert lib.cer_adam_flat(p + 4, p, p, p, None, 4, *hp, 0, 1, None) == -1    # misaligned
    assert b"aligned" in lib.cer_last_error()
    assert lib.cer_adam_flat(p, p, p, p, None, 4, *hp, 1, 1, None) == -1        # AMSGrad without its buffer
    assert b"max_exp_avg_sq" in lib.cer_last_error()
    assert lib.cer_adam_flat(p, p, p, p, None, 4, *hp, 0, 0, None) == -1        # the step count starts at 1
    assert b"step" in lib.cer_last_error()


def test_adam_flat_wrapper_rejects_cpu_tensors():
    from feature_vs_text_compound_emotion_amd import ops
    t = torch.zeros(8)
    with pytest.raises(ValueError):
        ops.adam_flat(t, t, t, t, None, 1e-3, 1)
