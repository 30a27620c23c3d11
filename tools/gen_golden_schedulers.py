"""Golden lr sequences of the reference's learning-rate schedulers (base/scheduler.py + torch.optim.lr_scheduler).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_schedulers.py <reference checkout>

Each scheduler drives a one-parameter torch.optim.SGD built WITHOUT lr (torch's default 1e-3, as instantiators.py:74-79
builds it) for 60 epochs; the fixture records param_groups[0]['lr'] before every epoch's optimizer step (index 0: right
after construction) plus the configuration as a JSON string.
"""
import json
import os
import sys

sys.modules["triton"] = None
import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "schedulers.npz")
EPOCHS = 60

# opt__ hyper-parameters (prefix stripped) per case; the floors bind: MYSTEP from epoch 20 (1e-3 * 0.3^4 < 2e-5),
# MYCOSINE around epoch 41 (cos -> -1)
CASES = {
    "STEP": dict(name_lr_scheduler="STEP", step_size=7, gamma=0.5, last_epoch=-1),
    "MYSTEP": dict(name_lr_scheduler="MYSTEP", step_size=5, gamma=0.3, min_lr=2e-5, last_epoch=-1),
    "COSINE": dict(name_lr_scheduler="COSINE", t_max=25, min_lr=1e-6, last_epoch=-1),
    "MYCOSINE": dict(name_lr_scheduler="MYCOSINE", coef=0.5, max_epochs=40, min_lr=1e-5, last_epoch=-1),
    "MULTISTEP": dict(name_lr_scheduler="MULTISTEP", milestones=[10, 25, 40], gamma=0.2, last_epoch=-1),
}


def reference_scheduler(opt, hp, scheduler_mod):
    sch = torch.optim.lr_scheduler
    name = hp["name_lr_scheduler"]
    if name == "STEP":
        return sch.StepLR(opt, step_size=hp["step_size"], gamma=hp["gamma"], last_epoch=hp["last_epoch"])
    if name == "MYSTEP":
        return scheduler_mod.MyStepLR(opt, step_size=hp["step_size"], gamma=hp["gamma"], last_epoch=hp["last_epoch"],
                                      min_lr=hp["min_lr"])
    if name == "COSINE":
        return sch.CosineAnnealingLR(opt, T_max=hp["t_max"], eta_min=hp["min_lr"], last_epoch=hp["last_epoch"])
    if name == "MYCOSINE":
        return scheduler_mod.MyCosineLR(opt, coef=hp["coef"], max_epochs=hp["max_epochs"], min_lr=hp["min_lr"],
                                        last_epoch=hp["last_epoch"])
    return sch.MultiStepLR(opt, milestones=hp["milestones"], gamma=hp["gamma"], last_epoch=hp["last_epoch"])


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.path.insert(0, os.path.join(os.path.abspath(sys.argv[1]), "base"))
    import scheduler as scheduler_mod  # the reference's base/scheduler.py (needs only torch)
    out = {}
    for key, hp in CASES.items():
        p = torch.nn.Parameter(torch.zeros(1))
        opt = torch.optim.SGD([p])
        s = reference_scheduler(opt, hp, scheduler_mod)
        lrs = []
        for _ in range(EPOCHS):
            lrs.append(opt.param_groups[0]["lr"])
            opt.step()
            s.step()
        out[f"{key}_lr"] = np.asarray(lrs, dtype=np.float64)
        out[f"{key}_config"] = np.asarray(json.dumps(hp))
    np.savez(OUT, names=np.asarray(list(CASES)), **out)
    print(f"wrote {OUT}: {list(CASES)}")


if __name__ == "__main__":
    main()
