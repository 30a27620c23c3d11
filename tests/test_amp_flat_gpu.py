"""Training under ``--amp``: the bucket check / unscale kernel against torch's ``_amp_foreach_non_finite_check_and_unscale_``,
the flat optimisers under ``torch.amp.GradScaler`` and ``FlatGradScaler`` against torch.optim.SGD / Adam under
``GradScaler`` (skips, scale trajectory, applied step counts), the absence of host reads in the fused step, and
``Trainer.train_step`` with ``args.amp`` against the reference's loop (trainer.py:341,365-391), on one rank and on two."""
import copy
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")


def _same(a, b):
    """Equal bits except that NaN positions only have to agree (NaN payloads are not part of the contract)."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(torch.where(na, 0.0, a), torch.where(nb, 0.0, b))


# ------------------------------------------------------------------ 1. the bucket kernel vs torch
@pytest.mark.parametrize("n", [4, (1 << 20) + 4])
@pytest.mark.parametrize("scale", [65536.0, 3.0, 1.0])
@pytest.mark.parametrize("bad", [None, "first", "middle", "last", "all3"])
def test_check_unscale_matches_torch(n, scale, bad):
    from feature_vs_text_compound_emotion_amd import ops
    g = torch.randn(n, generator=torch.Generator().manual_seed(n)).cuda() * 1e3
    if bad is not None:
        pos = {"first": [0], "middle": [n // 2], "last": [n - 1], "all3": [0, n // 2, n - 1]}[bad]
        for p, v in zip(pos, [INF, -INF, NAN] if bad == "all3" else [{"first": INF, "middle": -INF, "last": NAN}[bad]]):
            g[p] = v
    inv = torch.full((), scale, device="cuda").double().reciprocal().float()      # what GradScaler.unscale_ hands over
    ref, ref_found = g.clone(), torch.zeros((), device="cuda")
    torch._amp_foreach_non_finite_check_and_unscale_([ref], ref_found, inv)
    mine, found = g.clone(), torch.zeros((), device="cuda")
    ops.amp_check_unscale_flat(mine, found, inv)
    assert _same(mine, ref)
    assert torch.equal(found, ref_found) and found.item() == (0.0 if bad is None else 1.0)
    # check only: the flag, and not one bit of the bucket written
    chk, found2 = g.clone(), torch.zeros((), device="cuda")
    ops.amp_check_unscale_flat(chk, found2)
    assert torch.equal(chk.view(torch.int32), g.view(torch.int32)) and torch.equal(found2, ref_found)
    # found_inf accumulates (never reset), like torch's
    already = torch.ones((), device="cuda")
    ops.amp_check_unscale_flat(g.clone(), already)
    assert already.item() == 1.0


def test_check_unscale_above_2gib():
    from feature_vs_text_compound_emotion_amd import ops
    n = (1 << 29) + 8                                   # 2 GiB + 32 bytes: byte offsets past 2^31
    free, _ = torch.cuda.mem_get_info()
    if free < 4 * 4 * n:
        pytest.skip("not enough device memory for two 2 GiB buffers")
    g = torch.empty(n, device="cuda").uniform_(-1e4, 1e4)
    inv = torch.full((), 65536.0, device="cuda").double().reciprocal().float()
    ref, ref_found = g.clone(), torch.zeros((), device="cuda")
    torch._amp_foreach_non_finite_check_and_unscale_([ref], ref_found, inv)
    ops.amp_check_unscale_flat(g, found := torch.zeros((), device="cuda"), inv)
    assert torch.equal(g, ref) and found.item() == 0.0 == ref_found.item()
    del ref
    g[n - 1] = NAN                                      # only the very last element is bad
    ops.amp_check_unscale_flat(g, found)
    assert found.item() == 1.0


def test_check_unscale_argument_errors():
    from feature_vs_text_compound_emotion_amd import ops
    found = torch.zeros((), device="cuda")
    with pytest.raises(ValueError):
        ops.amp_check_unscale_flat(torch.zeros(8, device="cuda", dtype=torch.float16), found)
    with pytest.raises(ValueError):
        ops.amp_check_unscale_flat(torch.zeros(8, device="cuda"), torch.zeros((), device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.amp_check_unscale_flat(torch.zeros(8, device="cuda"), torch.zeros(2, device="cuda"))
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.amp_check_unscale_flat(torch.zeros(6, device="cuda"), found)
    with pytest.raises(RuntimeError, match="aligned"):
        ops.amp_check_unscale_flat(torch.zeros(12, device="cuda")[1:9], found)


# ------------------------------------------------------------------ 2. flat optimisers under a GradScaler vs torch
class _Toy(torch.nn.Module):
    def __init__(self, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.a = torch.nn.Parameter(torch.randn(37, 5, generator=g))
        self.b = torch.nn.Parameter(torch.randn(129, generator=g))
        self.c = torch.nn.Parameter(torch.randn(4, 3, 5, generator=g))  # total 374: not a multiple of 4


BAD_STEPS = {0: INF, 4: NAN, 11: -INF, 12: INF, 23: NAN}      # step 0 included: the first applied step comes later
N_STEPS = 30


def _loss(model, gs):
    """sum(p * G): the gradient of the SCALED loss is G * scale exactly (scales are powers of two)."""
    return sum((p * g).sum() for p, g in zip(model.parameters(), gs))


def _grads(step, gen):
    gs = [torch.randn(s, generator=gen).cuda() for s in [(37, 5), (129,), (4, 3, 5)]]
    if step in BAD_STEPS:
        gs[step % 3].view(-1)[step] = BAD_STEPS[step]
    return gs


def _run_pair(kind, scaler_kind, explicit_unscale, wd=0.0, amsgrad=False):
    from feature_vs_text_compound_emotion_amd.data_parallel import ClipDataParallel, FlatAdam, FlatGradScaler, FlatNesterovSGD
    ref, mine = _Toy(1).cuda(), _Toy(1).cuda()
    ddp = ClipDataParallel(mine, world_size=1, broadcast=False)
    if kind == "sgd":
        opt_ref = torch.optim.SGD(ref.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4, nesterov=True)
        opt = FlatNesterovSGD(ddp, lr=1e-3, momentum=0.9, weight_decay=1e-4)
    else:
        opt_ref = torch.optim.Adam(ref.parameters(), lr=1e-3, weight_decay=wd, amsgrad=amsgrad)
        opt = FlatAdam(ddp, lr=1e-3, weight_decay=wd, amsgrad=amsgrad)
    sc_ref = torch.amp.GradScaler("cuda", growth_interval=3)
    sc = (FlatGradScaler if scaler_kind == "flat" else torch.amp.GradScaler)("cuda", growth_interval=3)
    gen = torch.Generator().manual_seed(2)
    applied = 0
    for step in range(N_STEPS):
        if step == 15:
            opt_ref.param_groups[0]["lr"] = opt.param_groups[0]["lr"] = 3e-4
        gs = _grads(step, gen)
        before = [p.detach().clone() for p in mine.parameters()]
        for model, o, s in ((ref, opt_ref, sc_ref), (mine, opt, sc)):
            o.zero_grad(set_to_none=True)
            s.scale(_loss(model, gs)).backward()
            if explicit_unscale:
                s.unscale_(o)
            s.step(o)
            s.update()
        ok = step not in BAD_STEPS
        applied += ok
        yield step, ok, ref, mine, opt_ref, opt, ddp, sc_ref, sc, before, applied


def _check_step(kind, step, ok, ref, mine, opt_ref, opt, ddp, sc_ref, sc, before, applied, explicit_unscale):
    assert sc.get_scale() == sc_ref.get_scale(), step
    assert sc._get_growth_tracker() == sc_ref._get_growth_tracker(), step
    assert opt.steps == applied, step
    off = 0
    for pr, pm, b in zip(ref.parameters(), mine.parameters(), before):
        if not ok:
            assert torch.equal(pm, b), step                     # a skipped step changes nothing
        if kind == "sgd":
            # test_optim_gpu.py's bar for flat SGD vs torch.optim.SGD (torch's kernels may or may not contract a*b+c)
            assert (pr - pm).abs().max().item() <= 2.4e-7 * max(1.0, pr.abs().max().item()) * max(applied, 1), step
        else:
            assert torch.equal(pr, pm), (step, (pr - pm).abs().max().item())
        if ok or explicit_unscale:
            # the bucket holds the unscaled gradients, as p.grad does after torch's unscale (a skipped step of the fused
            # route leaves them scaled: the launch changes nothing)
            assert _same(ddp.flat[off:off + pm.numel()].view_as(pm), pr.grad), step
        off += pm.numel()
    if kind == "adam":
        keys = ["exp_avg", "exp_avg_sq"] + (["max_exp_avg_sq"] if opt.max_exp_avg_sq is not None else [])
        for pr, pm in zip(ref.parameters(), mine.parameters()):
            st = opt_ref.state.get(pr)
            o = (pm.data_ptr() - opt.flat_param.data_ptr()) // 4
            if st is None:
                assert applied == 0
                continue
            assert int(st["step"].item()) == applied
            for k in keys:
                assert torch.equal(getattr(opt, k)[o:o + pm.numel()].view_as(pm), st[k]), (step, k)


@pytest.mark.parametrize("explicit_unscale", [False, True])
@pytest.mark.parametrize("scaler_kind", ["torch", "flat"])
def test_flat_sgd_under_grad_scaler_matches_torch_sgd(scaler_kind, explicit_unscale):
    for st in _run_pair("sgd", scaler_kind, explicit_unscale):
        _check_step("sgd", *st, explicit_unscale)
    opt = st[5]
    assert opt.state_dict()["steps"] == N_STEPS - len(BAD_STEPS)


@pytest.mark.parametrize("explicit_unscale", [False, True])
@pytest.mark.parametrize("scaler_kind", ["torch", "flat"])
@pytest.mark.parametrize("amsgrad", [False, True])
@pytest.mark.parametrize("wd", [0.0, 1e-4])
def test_flat_adam_under_grad_scaler_matches_torch_adam(wd, amsgrad, scaler_kind, explicit_unscale):
    for st in _run_pair("adam", scaler_kind, explicit_unscale, wd=wd, amsgrad=amsgrad):
        _check_step("adam", *st, explicit_unscale)


def test_flat_sgd_momentum_buffer_under_grad_scaler_matches_torch():
    """The momentum buffer is initialised on the first APPLIED step (step 0 is skipped here)."""
    for st in _run_pair("sgd", "flat", False):
        pass
    ref, mine, opt_ref, opt = st[2], st[3], st[4], st[5]
    for pr, pm in zip(ref.parameters(), mine.parameters()):
        o = (pm.data_ptr() - opt.flat_param.data_ptr()) // 4
        b = opt.buf[o:o + pm.numel()].view_as(pm)
        assert (b - opt_ref.state[pr]["momentum_buffer"]).abs().max().item() <= 1e-6 * max(1.0, b.abs().max().item())


def test_state_dict_after_loss_scaled_steps_round_trips():
    """``state_dict`` reports the applied count; ``load_state_dict`` restores it, and a plain step after loss-scaled ones
    continues from it (bias corrections of step applied + 1)."""
    from feature_vs_text_compound_emotion_amd.data_parallel import ClipDataParallel, FlatAdam, FlatGradScaler
    mine = _Toy(1).cuda()
    opt = FlatAdam(ClipDataParallel(mine, world_size=1, broadcast=False), lr=1e-3)
    sc = FlatGradScaler("cuda", growth_interval=3)
    gen = torch.Generator().manual_seed(2)
    for step in range(6):
        opt.zero_grad()
        sc.scale(_loss(mine, _grads(step, gen))).backward()
        sc.step(opt)
        sc.update()
    sd = opt.state_dict()
    assert sd["steps"] == 4                               # steps 0 and 4 carry an Inf / a NaN
    other = FlatAdam(ClipDataParallel(_Toy(1).cuda(), world_size=1, broadcast=False), lr=1e-3)
    other.load_state_dict(sd)
    assert other.steps == 4
    opt.zero_grad()
    _loss(mine, _grads(1, gen)).backward()
    opt.step()                                            # plain step: folds the device count back to the host
    assert opt.steps == 5 and opt._applied is None


# ------------------------------------------------------------------ 3. no host read in the fused step
def _forbid_host_reads(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("host read of a device tensor inside the loss-scaled step")
    for name in ("item", "cpu", "tolist"):
        monkeypatch.setattr(torch.Tensor, name, refuse)


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_flat_grad_scaler_step_has_no_host_sync(kind, monkeypatch):
    from feature_vs_text_compound_emotion_amd.data_parallel import ClipDataParallel, FlatAdam, FlatGradScaler, FlatNesterovSGD
    mine = _Toy(1).cuda()
    ddp = ClipDataParallel(mine, world_size=1, broadcast=False)
    opt = FlatNesterovSGD(ddp, lr=1e-3) if kind == "sgd" else FlatAdam(ddp, lr=1e-3)
    sc = FlatGradScaler("cuda", growth_interval=3)
    gen = torch.Generator().manual_seed(2)
    for step in range(2):                                 # warm-up: lazy state (scale, counter, Adam's table) exists
        opt.zero_grad()
        sc.scale(_loss(mine, _grads(1, gen))).backward()
        sc.step(opt)
        sc.update()
    torch.cuda.synchronize()
    for step in range(3):
        opt.zero_grad()
        sc.scale(_loss(mine, _grads(step, gen))).backward()
        ddp.all_reduce_gradients()
        with monkeypatch.context() as m:
            _forbid_host_reads(m)
            torch.cuda.set_sync_debug_mode("error")
            try:
                sc.step(opt)
                sc.update()
            finally:
                torch.cuda.set_sync_debug_mode(0)
    assert opt.steps == 4                                 # 2 warm-up + steps 1, 2 (step 0 carries an Inf)


def test_stock_route_reads_the_host(monkeypatch):
    """Control for the test above: torch.optim.SGD under torch's GradScaler goes through ``_maybe_opt_step``'s ``.item()``,
    which the patch catches."""
    ref = _Toy(1).cuda()
    opt = torch.optim.SGD(ref.parameters(), lr=1e-3, momentum=0.9, nesterov=True)
    sc = torch.amp.GradScaler("cuda")
    sc.scale(_loss(ref, _grads(1, torch.Generator().manual_seed(2)))).backward()
    with monkeypatch.context() as m:
        _forbid_host_reads(m)
        with pytest.raises(AssertionError, match="host read"):
            sc.step(opt)


# ------------------------------------------------------------------ 4. Trainer under amp (LFAN 40x40, B = 2, L = 32)
MODS = ["video", "vggish", "bert"]
B, L, HW = 2, 32, 40


def _model(seed=0):
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.lfan import LFAN
    sd = synth.lfan_state_dict(MODS, n_cls=7, head_hw=HW // 8, seed=seed)
    model = LFAN(backbone_settings={}, output_dim=7, task="CLASSIFICATION", modality=MODS, example_length=L, kernel_size=5,
                 tcn_channel=synth.TCN_CHANNELS, root_dir="", device="cuda", head_hw=HW // 8)
    model.init(load_backbone=False)
    model.load_state_dict(sd, strict=True)
    model = model.cuda().train()
    for mod in model.modules():                      # dropout-free steps: the comparisons need no mask plumbing
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    for net in model.temporal.values():
        net.dropout = 0.0
    return model


def _batch(b=B, seed=56):
    from feature_vs_text_compound_emotion_amd import synth
    x, labels = synth.make_clip_batch(MODS, b, L, hw=HW, seed=seed)
    return {k: v.cuda() for k, v in x.items()}, labels.cuda()


def _trainer(model, opt, ddp=None, amp=True, criterion=None, b=B):
    from feature_vs_text_compound_emotion_amd.trainer import Trainer
    tr = Trainer(model, optimizer=opt, criterion=criterion, device="cuda", data_parallel=ddp, train_batch_size=b,
                 window_length=L)
    tr.args.amp = amp
    return tr


def _trainable(model):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters() if p.requires_grad])


def _reference_loop(model, x, labels, n_steps=2, amp=True):
    """trainer.py:341 (GradScaler), :365 (zero_grad(set_to_none=True)), :367-383 (autocast forward + CE), :389-391
    (scale / step / update) with instantiators.py:74-79's SGD."""
    from feature_vs_text_compound_emotion_amd.lfan import cross_entropy_loss
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.SGD(params=params, lr=1e-3, momentum=0.9, dampening=0.0, weight_decay=1e-4, nesterov=True)
    scaler = torch.amp.GradScaler("cuda", enabled=amp)
    losses = []
    for _ in range(n_steps):
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
            out = model(dict(x))                     # a fresh dict: LFAN updates its input dict in place (model.py:511-515)
            bsz, nfms, _ = labels.shape
            loss = cross_entropy_loss(out.contiguous().view(bsz * nfms, -1), labels.contiguous().view(bsz * nfms).long())
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        losses.append(loss.detach())
    return losses, _trainable(model), scaler


def test_amp_train_step_runs_the_encoder_on_fp16_kernels(monkeypatch):
    """The precision ``inference()`` selects under --amp (fp16 narrow storage) is the one the training step runs."""
    from feature_vs_text_compound_emotion_amd import ops
    seen = []
    real = ops.conv2d_n16

    def spy(x, *a, **k):
        seen.append(x.dtype)
        return real(x, *a, **k)
    monkeypatch.setattr(ops, "conv2d_n16", spy)
    model = _model()
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-3, momentum=0.9, nesterov=True)
    x, labels = _batch()
    _trainer(model, opt, amp=True).train_step({**x, "continuous_label": labels})
    assert seen and set(seen) == {torch.float16}
    seen.clear()
    _trainer(model, opt, amp=False).train_step({**x, "continuous_label": labels})
    assert torch.float16 not in seen                  # amp off: the encoder stays on its own (bf16x3) kernels


def test_amp_train_steps_equal_the_reference_loop():
    model = _model()
    ref_model = copy.deepcopy(model)
    x, labels = _batch()
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-3, momentum=0.9, dampening=0.0,
                          weight_decay=1e-4, nesterov=True)
    tr = _trainer(model, opt)
    losses = [tr.train_step({**x, "continuous_label": labels}) for _ in range(2)]
    ref_losses, w_ref, sc_ref = _reference_loop(ref_model, x, labels)
    assert all(torch.equal(a, b) for a, b in zip(losses, ref_losses)), (losses, ref_losses)
    assert torch.equal(_trainable(model), w_ref)
    assert tr.scaler.get_scale() == sc_ref.get_scale() and type(tr.scaler) is torch.amp.GradScaler


def test_amp_train_steps_with_flat_sgd_equal_the_reference_loop():
    from feature_vs_text_compound_emotion_amd.data_parallel import ClipDataParallel, FlatGradScaler, FlatNesterovSGD
    model = _model()
    ref_model = copy.deepcopy(model)
    x, labels = _batch()
    w0 = _trainable(model)
    ddp = ClipDataParallel(model, world_size=1)
    tr = _trainer(model, FlatNesterovSGD(ddp, lr=1e-3), ddp=ddp)
    losses = [tr.train_step({**x, "continuous_label": labels}) for _ in range(2)]
    ref_losses, w_ref, sc_ref = _reference_loop(ref_model, x, labels)
    assert isinstance(tr.scaler, FlatGradScaler)
    assert torch.equal(losses[0], ref_losses[0])           # same weights before step 1: the same forward
    assert abs(losses[1].item() - ref_losses[1].item()) <= 1e-6 * abs(ref_losses[1].item())
    w = _trainable(model)
    # test_optim_gpu.py's bar for flat SGD vs torch.optim.SGD, per step
    assert (w - w_ref).abs().max().item() <= 2 * 2.4e-7 * max(1.0, w_ref.abs().max().item())
    assert not torch.equal(w, w0) and tr.optimizer.steps == 2 and tr.scaler.get_scale() == sc_ref.get_scale()


@pytest.mark.parametrize("flat", [False, True])
def test_amp_step_with_an_infinite_loss_is_skipped(flat):
    from feature_vs_text_compound_emotion_amd.data_parallel import ClipDataParallel, FlatNesterovSGD
    from feature_vs_text_compound_emotion_amd.lfan import cross_entropy_loss
    calls = []

    def criterion(out, lab):
        calls.append(1)
        loss = cross_entropy_loss(out, lab)
        return loss * INF if len(calls) == 2 else loss
    model = _model()
    if flat:
        ddp = ClipDataParallel(model, world_size=1)
        opt = FlatNesterovSGD(ddp, lr=1e-3)
    else:
        ddp, opt = None, torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-3, momentum=0.9,
                                         nesterov=True, weight_decay=1e-4)
    tr = _trainer(model, opt, ddp=ddp, criterion=criterion)
    x, labels = _batch()
    tr.train_step({**x, "continuous_label": labels})
    w1, s1 = _trainable(model), tr.scaler.get_scale()
    tr.train_step({**x, "continuous_label": labels})
    assert torch.equal(_trainable(model), w1)
    assert torch.isfinite(w1).all()
    assert tr.scaler.get_scale() == s1 / 2
    if flat:
        assert opt.steps == 1


def test_amp_off_train_step_is_the_plain_sequence():
    from feature_vs_text_compound_emotion_amd.lfan import cross_entropy_loss
    model = _model()
    ref_model = copy.deepcopy(model)
    x, labels = _batch()

    def sgd(m):
        return torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=1e-3, momentum=0.9, weight_decay=1e-4,
                               nesterov=True)
    tr = _trainer(model, sgd(model), amp=False)
    losses = [tr.train_step({**x, "continuous_label": labels}) for _ in range(2)]
    assert tr.scaler is None
    opt = sgd(ref_model)
    for i in range(2):                                    # the step as it was before --amp training existed
        opt.zero_grad(set_to_none=True)
        out = ref_model(dict(x))
        loss = cross_entropy_loss(out.contiguous().view(B * L, -1), labels.contiguous().view(B * L).long())
        loss.backward()
        opt.step()
        assert torch.equal(loss.detach(), losses[i])
    assert torch.equal(_trainable(model), _trainable(ref_model))


def test_train_one_epoch_starts_a_fresh_scaler():
    from feature_vs_text_compound_emotion_amd.data_parallel import ClipDataParallel, FlatGradScaler, FlatNesterovSGD
    import numpy as np
    model = _model()
    ddp = ClipDataParallel(model, world_size=1)
    tr = _trainer(model, FlatNesterovSGD(ddp, lr=1e-3), ddp=ddp)
    x, labels = _batch()
    loader = [({**{k: v.cpu() for k, v in x.items()}, "continuous_label": labels.cpu()}, ["a", "b"], [L, L],
               [np.arange(L)] * B)]
    tr.train_one_epoch(loader)
    first = tr.scaler
    tr.train_one_epoch(loader)
    assert isinstance(first, FlatGradScaler) and tr.scaler is not first and tr.optimizer.steps == 2


# ------------------------------------------------------------------ 5. two ranks (gloo, both on the one GPU)
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    import sys
    sys.modules.setdefault("triton", None)
    import torch.distributed as dist
    from feature_vs_text_compound_emotion_amd.data_parallel import ClipDataParallel, FlatNesterovSGD, init_process_group_from_env
    init_process_group_from_env(backend="gloo")
    torch.cuda.set_device(0)
    model = _model(seed=rank).eval()       # running-statistics BatchNorm: each clip's gradient is independent of its batch
    ddp = ClipDataParallel(model)
    tr = _trainer(model, FlatNesterovSGD(ddp, lr=1e-3), ddp=ddp, b=1)
    x, labels = _batch(b=2)
    idx = ddp.shard(list(range(2)), rank)
    xs, ls = {k: v[idx] for k, v in x.items()}, labels[idx]
    loss = tr.train_step({**xs, "continuous_label": ls})
    res = [(loss.cpu(), ddp.flat.clone().cpu(), ddp.flat_param.clone().cpu(), tr.scaler.get_scale(), tr.optimizer.steps)]
    poison = [rank == 1]
    hook = model.regressor.weight.register_hook(lambda g: g * INF if poison[0] else g)   # rank 1 only
    tr.train_step({**xs, "continuous_label": ls})
    hook.remove()
    res.append((None, None, ddp.flat_param.clone().cpu(), tr.scaler.get_scale(), tr.optimizer.steps))
    out[rank] = res
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_amp_step_equals_one_process_and_skip_together():
    from feature_vs_text_compound_emotion_amd.data_parallel import ClipDataParallel, FlatNesterovSGD
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        out = mgr.dict()
        mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
        r0, r1 = out[0], out[1]
    (_, g0, w0, s0, n0), (_, g1, w1, s1, n1) = r0[0], r1[0]
    assert torch.equal(g0, g1) and torch.equal(w0, w1) and s0 == s1 and n0 == n1 == 1
    # a non-finite gradient on rank 1 only: the summed bucket is non-finite on both, both skip and back off together
    (_, _, w0b, s0b, n0b), (_, _, w1b, s1b, n1b) = r0[1], r1[1]
    assert torch.equal(w0b, w0) and torch.equal(w1b, w1)
    assert s0b == s1b == s0 / 2 and n0b == n1b == 1
    # one process on the global batch
    model = _model(seed=0).eval()
    ddp = ClipDataParallel(model, world_size=1)
    tr = _trainer(model, FlatNesterovSGD(ddp, lr=1e-3), ddp=ddp)
    x, labels = _batch(b=2)
    tr.train_step({**x, "continuous_label": labels})
    g, w = ddp.flat.cpu(), ddp.flat_param.cpu()
    gerr = (g - g0).abs().max().item() / g.abs().max().item()
    werr = (w - w0).abs().max().item()
    print(f"\n[dp amp] 2 ranks x 1 clip vs 1 rank x 2 clips: relative gradient difference {gerr:.2e}, weights {werr:.2e}")
    assert gerr < 2e-5 and werr < 1e-7            # the bars of tests/test_dp_amp_gpu.py
    assert tr.scaler.get_scale() == s0
