"""Fixture generator (build container only: imports /root/reference read-only): two SGD steps of the reference's LFAN with
the 'logmel' modality (models/model.py:458-462,500-508) after ALL THREE audio groups of the gradual release
(base/parameter_control.py:58,85-103: VGGish parameters 16-17, 14-15, 12-13 = embeddings.4 / .2 / .0) -- seeded synthetic
weights and inputs, trained on the CPU with SGD as instantiators.py:74-79 builds it, dropout off.  Writes
tests/golden/lfan_logmel_audio_release.npz: losses and logits of both steps, the three bias gradients and the per-row L2
norms of the three weight gradients of step 1, and the post-step weights of the three layers at a seeded sample of indices.

    python tools/gen_golden_audio_release.py
"""
import os
import sys

import numpy as np
import torch

sys.modules.setdefault("triton", None)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, ROOT)

import models.model as ref_model  # noqa: E402
from feature_vs_text_compound_emotion_amd import synth  # noqa: E402

MODS, B, L, N_CLS, WSEED, DSEED, SSEED, NSAMPLE = ["logmel", "vggish"], 2, 6, 7, 3, 9, 5, 512
LAYERS = ("0", "2", "4")


def main():
    torch.set_num_threads(8)
    spec, alias = synth.lfan_spec(MODS, n_cls=N_CLS)
    sd = synth.make_state_dict(spec, alias, seed=WSEED)
    ref_model.LFAN.load_audio_backbone = lambda self, backbone_settings: ref_model.AudioBackbone()
    m = ref_model.LFAN(backbone_settings={}, output_dim=N_CLS, task="CLASSIFICATION", modality=MODS, example_length=L,
                       kernel_size=5, tcn_channel=synth.TCN_CHANNELS, root_dir="", device="cpu")
    m.init()
    m.load_state_dict(sd, strict=True)
    audio = list(m.spatial["audio"].parameters())
    for p in audio:
        p.requires_grad = False
    for group in ([16, 17], [14, 15], [12, 13]):           # ResnetParamControl.init_module_list()["audio"], popped in order
        for i in group:
            audio[i].requires_grad = True
    names = [k for k, p in m.named_parameters() if p.requires_grad]
    emb = {f"spatial.audio.backbone.embeddings.{i}.{w}" for i in LAYERS for w in ("weight", "bias")}
    assert emb <= set(names), sorted(emb - set(names))
    assert not any(k.startswith("spatial.audio.backbone.features") for k in names)
    m.train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    params = [p for p in m.parameters() if p.requires_grad]
    opt = torch.optim.SGD(params=params, lr=1e-3, momentum=0.9, dampening=0.0, weight_decay=1e-4, nesterov=True)
    loss_fn = torch.nn.CrossEntropyLoss()
    out = {"meta": np.asarray([B, L, N_CLS, WSEED, DSEED, SSEED, NSAMPLE])}
    named = dict(m.named_parameters())
    for step in range(2):
        x, labels = synth.make_clip_batch(MODS, B, L, seed=DSEED + step)
        opt.zero_grad()
        logits = m({k: v.clone() for k, v in x.items()})
        loss = loss_fn(logits.reshape(-1, N_CLS), labels.reshape(-1).long())
        loss.backward()
        out[f"loss{step}"] = np.asarray([loss.item()])
        out[f"logits{step}"] = logits.detach().numpy()
        if step == 0:
            for i in LAYERS:
                pre = f"spatial.audio.backbone.embeddings.{i}."
                out[f"db{i}"] = named[pre + "bias"].grad.numpy().copy()
                out[f"dw{i}_rownorm"] = named[pre + "weight"].grad.double().norm(dim=1).numpy()
        opt.step()
    g = torch.Generator().manual_seed(SSEED)
    for i in LAYERS:
        w = named[f"spatial.audio.backbone.embeddings.{i}.weight"].detach().reshape(-1)
        idx = torch.randint(0, w.numel(), (NSAMPLE,), generator=g)
        out[f"w{i}_after"] = w[idx].numpy().copy()
        out[f"b{i}_after"] = named[f"spatial.audio.backbone.embeddings.{i}.bias"].detach().numpy().copy()
    path = os.path.join(ROOT, "tests", "golden", "lfan_logmel_audio_release.npz")
    np.savez_compressed(path, **out)
    print(path, len(out), "arrays,", os.path.getsize(path), "bytes; losses", out["loss0"], out["loss1"])


if __name__ == "__main__":
    main()
