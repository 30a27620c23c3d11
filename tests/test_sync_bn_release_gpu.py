"""Synchronised batch statistics through the RELEASED parts of the IR-50 encoder (``ClipDataParallel(sync_bn=...,
sync_released=True)``): the large-row moments kernel and the fused backward apply passes against float64, the synchronised
backward of one rank against the local one, 2 gloo ranks x B/2 clips against 1 process x B clips with the reference's release
groups and the whole encoder, the forced single-rank RCCL path and the agreed memory plan."""
import math
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1


# ------------------------------------------------------------------ (a) kernels
def _offset_data(r, c, seed):
    """Channel means up to 1e3 with std 1; channel 1 a further 200 sigma out; channel 2's first row 6 sigma from its mean (the
    shift row of the one-pass statistics)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    means = (torch.rand(c, device="cuda", generator=g) * 2.0 - 1.0) * 1e3
    means[1] += 200.0
    x = torch.randn(r, c, device="cuda", generator=g)
    x[0, 2] = 6.0
    x += means
    return x


def _truth(x, chunk=1 << 22):
    """float64 (mean, biased var) per column, in row chunks (two passes)."""
    r = x.shape[0]
    s = torch.zeros(x.shape[1], device=x.device, dtype=torch.float64)
    for i in range(0, r, chunk):
        s += x[i:i + chunk].double().sum(0)
    mean = s / r
    m2 = torch.zeros_like(mean)
    for i in range(0, r, chunk):
        m2 += ((x[i:i + chunk].double() - mean) ** 2).sum(0)
    return mean, m2 / r


def _stat_errors(x, rm0, rv0, stats_fn):
    """Relative errors (to max(|truth|, 1)) of save_mean, save_invstd, running_mean, running_var against float64."""
    r = x.shape[0]
    mean, var = _truth(x)
    rm, rv = rm0.clone(), rv0.clone()
    sm, si = stats_fn(x, rm, rv)
    truth = (mean, 1.0 / torch.sqrt(var + EPS), (1 - MOM) * rm0.double() + MOM * mean,
             (1 - MOM) * rv0.double() + MOM * var * r / (r - 1))
    return [((got.double() - t).abs() / t.abs().clamp_min(1.0)).max().item() for got, t in zip((sm, si, rm, rv), truth)]


def _large(x, rm, rv):
    from feature_vs_text_compound_emotion_amd import ops
    return ops.bn_rows_merge(ops.bn_rows_moments_large(x).unsqueeze(0), rm, rv, EPS, MOM)


def _local(x, rm, rv):
    from feature_vs_text_compound_emotion_amd import ops
    return ops.bn_rows_stats(x, rm, rv, EPS, MOM)


# Floors: the float64 results are rounded once to fp32 (mean: 2^-24 relative) and the fp32 running update adds two roundings;
# rsqrt-free 1 / sqrt in float64 then one rounding for invstd.  2^-22 covers every one of them with room.
FLOOR = 2.0 ** -22


def _check_against_local(x, seed):
    c = x.shape[1]
    g = torch.Generator(device="cuda").manual_seed(seed)
    rm0 = torch.randn(c, device="cuda", generator=g)
    rv0 = torch.rand(c, device="cuda", generator=g) + 0.5
    new = _stat_errors(x, rm0, rv0, _large)
    old = _stat_errors(x, rm0, rv0, _local)
    print(f"\n[moments_large {tuple(x.shape)}] mean / invstd / running_mean / running_var: new "
          + " ".join(f"{e:.2e}" for e in new) + " | bn_rows_stats " + " ".join(f"{e:.2e}" for e in old))
    for n, o in zip(new, old):
        assert n <= 1.5 * o + FLOOR, (new, old)


@pytest.mark.parametrize("c", [64, 256, 512])
@pytest.mark.parametrize("r", [2049, 40000, 1000003])
def test_large_moments_match_float64_at_least_as_well_as_bn_rows_stats(r, c):
    _check_against_local(_offset_data(r, c, seed=r + c), seed=7)


def test_large_moments_of_uneven_blocks_merge_to_the_statistics_of_their_concatenation():
    from feature_vs_text_compound_emotion_amd import ops
    c = 256
    x = _offset_data(2049 + 40000 + 777, c, seed=3)
    blocks = [x[:2049], x[2049:42049], x[42049:]]
    merged = torch.stack([ops.bn_rows_moments_large(b.contiguous()) for b in blocks])
    sm, si = ops.bn_rows_merge(merged, eps=EPS)
    mean, var = _truth(x)
    assert (sm.double() - mean).abs().div(mean.abs().clamp_min(1.0)).max().item() < FLOOR
    assert (si.double() - 1.0 / torch.sqrt(var + EPS)).abs().div(1.0 / torch.sqrt(var + EPS)).max().item() < FLOOR
    whole = ops.bn_rows_merge(ops.bn_rows_moments_large(x).unsqueeze(0), eps=EPS)
    assert (sm - whole[0]).abs().div(sm.abs().clamp_min(1.0)).max().item() < FLOOR
    assert (si - whole[1]).abs().div(si).max().item() < FLOOR


def _bwd_inputs(r, c, seed):
    from feature_vs_text_compound_emotion_amd import ops
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(r, c, device="cuda", generator=g) * 3.0 + 5.0
    dy = torch.randn(r, c, device="cuda", generator=g)
    w = torch.randn(c, device="cuda", generator=g)
    add = torch.randn(r, c, device="cuda", generator=g)
    sm, si = ops.bn_rows_stats(x, torch.zeros(c, device="cuda"), torch.ones(c, device="cuda"))
    return x, dy, w, add, sm, si


BWD_CASES = [(2049, 64), (40000, 256), (1000003, 512)]


def _child_one_rank_backward(rank, port, cases, out):
    """``BatchNormSync.rows_bwd`` on a one-rank RCCL group against ``BatchNormLocal.rows_bwd`` in the three output forms: the
    all-reduced sums over R x 1 rows drive the same apply pass as the local sums over R rows."""
    os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    import sys
    sys.modules.setdefault("triton", None)
    import torch.distributed as dist
    from feature_vs_text_compound_emotion_amd.batchnorm import LOCAL
    from feature_vs_text_compound_emotion_amd.data_parallel import BatchNormSync, init_process_group_from_env
    init_process_group_from_env(backend="nccl", single_rank_group=True)
    sync = BatchNormSync(dist.new_group(), 1, 0)
    res = {}
    for r, c, seed in cases:
        x, dy, w, add, sm, si = _bwd_inputs(r, c, seed)
        for form, kw in (("fp32", {}), ("split", {"split_out": True}), ("add", {"add": add})):
            ref, got = LOCAL.rows_bwd(dy, x, sm, si, w, **kw), sync.rows_bwd(dy, x, sm, si, w, **kw)
            dx_equal = (torch.equal(got[0].hi, ref[0].hi) and torch.equal(got[0].lo, ref[0].lo) if form == "split"
                        else torch.equal(got[0], ref[0]))
            res[(r, c, form)] = (dx_equal, torch.equal(got[1], ref[1]), torch.equal(got[2], ref[2]))
            del ref, got
            torch.cuda.empty_cache()
    out.update(res)
    dist.barrier()
    dist.destroy_process_group()


def _one_rank_backward(cases):
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        out = mgr.dict()
        mp.spawn(_child_one_rank_backward, args=(_free_port(), cases, out), nprocs=1, join=True)
        return dict(out)


def _check_one_rank_equal(res, r, c):
    for form in ("fp32", "split", "add"):
        assert res[(r, c, form)] == (True, True, True), (r, c, form, res[(r, c, form)])


@pytest.fixture(scope="module")
def one_rank_backward():
    return _one_rank_backward([(r, c, r) for r, c in BWD_CASES])


@pytest.mark.parametrize("r,c", BWD_CASES)
def test_one_rank_synchronised_backward_is_the_local_backward_bit_for_bit(one_rank_backward, r, c):
    _check_one_rank_equal(one_rank_backward, r, c)


def test_at_the_timed_size():
    """1024 frames of 224x224 x 64 channels (the stem and stage 1 of the whole-encoder release): R * C = 3.3 G > 2^31."""
    r, c = 1024 * 224 * 224, 64
    x = _offset_data(r, c, seed=11)
    _check_against_local(x, seed=12)
    del x
    torch.cuda.empty_cache()
    _check_one_rank_equal(_one_rank_backward([(r, c, 13)]), r, c)


@pytest.mark.parametrize("r,c", [(2049, 64), (40000, 256)])
def test_fused_backward_apply_with_summed_sums_of_two_blocks_matches_float64_autograd(r, c):
    """Bar: dx = w * invstd * (dy - (s1 + x_hat * s2) / count) with fp32 sums over 2R rows; each term is within ~1e-6 relative
    of float64 (fp32 tree sums, a float64-merged invstd rounded once), so 2e-5 of max |dx| has a 10x margin."""
    from feature_vs_text_compound_emotion_amd import ops
    x, dy, w, _, _, _ = _bwd_inputs(2 * r, c, seed=5)
    b = torch.randn(c, device="cuda")
    blocks = [(x[:r].contiguous(), dy[:r].contiguous()), (x[r:].contiguous(), dy[r:].contiguous())]
    sm, si = ops.bn_rows_merge(torch.stack([ops.bn_rows_moments_large(xb) for xb, _ in blocks]), eps=EPS)
    sums = sum(ops.bn_rows_bwd_sums(dyb, xb, sm, si) for xb, dyb in blocks)
    dx = torch.cat([ops.bn_rows_bwd_apply(dyb, xb, sm, si, w, sums, 2 * r, add=torch.zeros_like(dyb)) for xb, dyb in blocks])
    dxs = torch.cat([ops.bn_rows_bwd_apply(dyb, xb, sm, si, w, sums, 2 * r, split_out=True).float()
                     for xb, dyb in blocks])
    x64 = x.double().requires_grad_(True)
    y = torch.nn.functional.batch_norm(x64, None, None, w.double(), b.double(), training=True, eps=EPS)
    y.backward(dy.double())
    ref = x64.grad
    scale = ref.abs().max().item()
    err = (dx.double() - ref).abs().max().item() / scale
    errs = (dxs.double() - ref).abs().max().item() / scale
    print(f"\n[fused apply, 2 blocks x {r} x {c}] dx vs float64 autograd: fp32 {err:.2e}, split {errs:.2e}")
    assert err < 2e-5 and errs < 2e-5


# ------------------------------------------------------------------ (b) 2 gloo ranks x B/2 == 1 process x B
MODS = ["video", "vggish", "bert"]
B, L, HW = 4, 8, 40
# (release set, precision, memory plan, sync) run by both ranks in one spawn
CASES = [("head", "bf16x3", "raw", True), ("head", "bf16x3", "raw", False),
         ("g123", "bf16x3", "raw", True), ("g123", "bf16x3", "raw", False), ("g123", "fp32", "raw", True),
         ("all", "bf16x3", "raw", True), ("all", "bf16x3", "raw", False), ("all", "bf16x3", "recompute", True),
         ("g123", "bf16x3", "auto", True)]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _model(release, precision, memory, hw=HW, seed=0):
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.lfan import LFAN
    from feature_vs_text_compound_emotion_amd.parameter_control import ResnetParamControl
    sd = synth.lfan_state_dict(MODS, n_cls=7, head_hw=hw // 8, seed=seed)
    m = LFAN(backbone_settings={}, output_dim=7, task="CLASSIFICATION", modality=MODS, example_length=L, kernel_size=5,
             tcn_channel=synth.TCN_CHANNELS, root_dir="", device="cuda", head_hw=hw // 8)
    m.init(load_backbone=False)
    m.load_state_dict(sd, strict=True)
    vis = m.spatial["visual"].backbone
    vis.precision = precision
    vis.activation_memory = memory
    if release == "all":
        for p in vis.parameters():
            p.requires_grad = True
    else:
        pc = ResnetParamControl(trainer=None)
        for _ in range({"head": 1, "g123": 3}[release]):
            pc.release_param(m.spatial)
    m = m.cuda().train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    for net in m.temporal.values():
        net.dropout = 0.0
    return m


def _running(model):
    return {n: b.detach().clone().cpu() for n, b in model.named_buffers() if "running_" in n}


def _step(model, ddp, opt, x, labels):
    from feature_vs_text_compound_emotion_amd.lfan import cross_entropy_loss
    ddp.zero_grad()
    out = model(dict(x))
    loss = cross_entropy_loss(out, labels)
    loss.backward()
    ddp.all_reduce_gradients()
    g = ddp.flat.clone()
    opt.step()
    return out.detach(), g, ddp.flat_param.clone()


def _worker(rank, world, port, out):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    import sys
    sys.modules.setdefault("triton", None)
    import torch.distributed as dist
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.data_parallel import ClipDataParallel, FlatNesterovSGD, init_process_group_from_env
    init_process_group_from_env(backend="gloo")
    torch.cuda.set_device(0)
    res = {}
    real_mem_get_info, real_memory_reserved = torch.cuda.mem_get_info, torch.cuda.memory_reserved
    for case in CASES:
        release, precision, memory, sync = case
        model = _model(release, precision, memory, seed=rank)   # different weights per rank: broadcast_state makes them rank 0's
        ddp = ClipDataParallel(model, overlap=True, bucket_mb=2.0, sync_bn=sync, sync_released=sync)
        opt = FlatNesterovSGD(ddp, lr=1e-3)
        x, labels = synth.make_clip_batch(MODS, B, L, hw=HW, seed=55)
        idx = ddp.shard(list(range(B)), rank)
        if memory == "auto" and rank == 1:   # this rank alone sees no free memory (nor a reusable cache): both must run "recompute"
            torch.cuda.mem_get_info = lambda device=None: (0, real_mem_get_info(device)[1])
            torch.cuda.memory_reserved = torch.cuda.memory_allocated
        try:
            _, g, w = _step(model, ddp, opt, {k: v[idx].cuda() for k, v in x.items()}, labels[idx].cuda())
        finally:
            torch.cuda.mem_get_info, torch.cuda.memory_reserved = real_mem_get_info, real_memory_reserved
        res[case] = (g.cpu(), w.cpu(), _running(model), model.spatial["visual"].backbone._act_mem)
    out[rank] = res
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_ranks():
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        out = mgr.dict()
        mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
        return out[0], out[1]


def _single(release, precision, memory):
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.data_parallel import ClipDataParallel, FlatNesterovSGD
    model = _model(release, precision, memory, seed=0)
    ddp = ClipDataParallel(model, world_size=1)
    opt = FlatNesterovSGD(ddp, lr=1e-3)
    x, labels = synth.make_clip_batch(MODS, B, L, hw=HW, seed=55)
    _, g, w = _step(model, ddp, opt, {k: v.cuda() for k, v in x.items()}, labels.cuda())
    return g.cpu(), w.cpu(), _running(model)


def _errors(ref, got):
    g, w, run = ref[:3]
    g1, w1, run1 = got[:3]
    gerr = (g - g1).abs().max().item() / g.abs().max().item()
    werr = (w - w1).abs().max().item()
    berr = max((run[n] - run1[n]).abs().max().item() / max(run[n].abs().max().item(), 1e-30) for n in run)
    return gerr, werr, berr


# Bars (gradient relative to its max, weights absolute, running buffers relative), per release set.  Why they are not
# zero: the encoder picks its conv kernels by the output pixel count (frames x Ho x Wo), so B/2 and B frames accumulate the
# same products in different orders, and every batch-statistics BatchNorm passes these differences on; the BatchNorm
# backwards of the released units then amplify the relative difference of small gradients (tests/test_sync_bn_gpu.py
# explains the same for the frozen encoder).  The synchronised path itself adds almost nothing: forced on one rank it stays
# within 5e-6 of the local step (below).  Measured on the MI355X, worst over the parametrisations of a set:
#   head          gradient 3.9e-5, weights 6.0e-8, running buffers 2.3e-6
#   groups 1-3    gradient 1.15e-3 (bf16x3; fp32 7.2e-4), weights 1.4e-6, running buffers 2.1e-6
#   whole encoder gradient 1.02e-3 (raw == recompute, bit for bit), weights 1.3e-6, running buffers 1.7e-6
# The bars sit at 2x those values; weights keep at least 2 fp32 ulps of a weight in [1, 2) (2.4e-7), since a gradient
# difference far below the bar can flip the last bit of w - lr * update.  Without sync_bn the same 2-rank runs miss by
# 5e2 .. 3e4 x (gradient 1.19, running buffers 0.13).
BARS = {"head": (8e-5, 2.4e-7, 4.6e-6), "g123": (2.3e-3, 2.9e-6, 4.3e-6), "all": (2.1e-3, 2.6e-6, 3.4e-6)}


@pytest.mark.parametrize("release,precision,memory", [("head", "bf16x3", "raw"), ("g123", "bf16x3", "raw"),
                                                      ("g123", "fp32", "raw"), ("all", "bf16x3", "raw"),
                                                      ("all", "bf16x3", "recompute"), ("g123", "bf16x3", "auto")])
def test_two_synced_ranks_with_released_units_equal_one_process_on_the_full_batch(two_ranks, release, precision, memory):
    r0, r1 = two_ranks
    s0, s1 = r0[(release, precision, memory, True)], r1[(release, precision, memory, True)]
    assert torch.equal(s0[0], s1[0]) and torch.equal(s0[1], s1[1])     # one reduced gradient, weights in lockstep
    assert set(s0[2]) == set(s1[2]) and len(s0[2]) >= 2 * 54
    for n in s0[2]:                                                     # every running buffer stays one set
        assert torch.equal(s0[2][n], s1[2][n]), n
    if memory == "auto":                                                # rank 1 lacked memory for "raw": both ran "recompute"
        assert s0[3] == s1[3] == "recompute", (s0[3], s1[3])
    ref = _single(release, precision, memory)
    gerr, werr, berr = _errors(ref, s0)
    gbar, wbar, bbar = BARS[release]
    print(f"\n[sync_released {release} {precision} {memory}] 2 synced ranks x {B // 2} clips vs 1 process x {B} clips: "
          f"gradient {gerr:.2e}, weights {werr:.2e}, running buffers {berr:.2e}")
    unsync = r0.get((release, precision, memory, False))
    if unsync is not None:
        ugerr, uwerr, uberr = _errors(ref, unsync)
        print(f"[sync_released {release} {precision} {memory}] the same without sync_bn: gradient {ugerr:.2e}, weights "
              f"{uwerr:.2e}, running buffers {uberr:.2e}")
        assert max(ugerr / gbar, uberr / bbar) >= 100
    assert gerr < gbar and werr < wbar and berr < bbar


# ------------------------------------------------------------------ (c) world 1, forced, on RCCL
FORCED = [("g123", "bf16x3", "raw"), ("all", "fp16", "recompute16")]


def _child_forced(rank, port, out):
    os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    import sys
    sys.modules.setdefault("triton", None)
    import torch.distributed as dist
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.data_parallel import ClipDataParallel, FlatNesterovSGD, init_process_group_from_env
    init_process_group_from_env(backend="nccl", single_rank_group=True)
    assert dist.get_backend() == "nccl" and dist.get_world_size() == 1
    x, labels = synth.make_clip_batch(MODS, B, L, hw=HW, seed=55)
    xd, ld = {k: v.cuda() for k, v in x.items()}, labels.cuda()
    runs = {}
    for release, precision, memory in FORCED:
        for sync in (False, "force"):
            model = _model(release, precision, memory)
            ddp = ClipDataParallel(model, overlap="force", bucket_mb=1.0, sync_bn=sync, sync_released=bool(sync))
            opt = FlatNesterovSGD(ddp, lr=1e-3)
            _, g, w = _step(model, ddp, opt, xd, ld)
            torch.cuda.synchronize()
            frozen = sorted(n for n, m in model.named_modules() if isinstance(m, torch.nn.BatchNorm2d) and
                            not m.weight.requires_grad)
            released = sorted(n for n, m in model.spatial["visual"].backbone.named_modules()
                              if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.BatchNorm1d)) and m.weight.requires_grad)
            runs[(release, precision, memory, str(sync))] = (g.cpu(), w.cpu(), _running(model), frozen, len(released))
    # one short step at the 224x224 geometry: 1 clip x 8 frames, release groups 1-3
    model = _model("g123", "bf16x3", "auto", hw=224)
    ddp = ClipDataParallel(model, overlap="force", bucket_mb=25.0, sync_bn="force", sync_released=True)
    opt = FlatNesterovSGD(ddp, lr=1e-3)
    x, labels = synth.make_clip_batch(MODS, 1, L, hw=224, seed=56)
    _, g, _ = _step(model, ddp, opt, {k: v.cuda() for k, v in x.items()}, labels.cuda())
    out["at224"] = (bool(torch.isfinite(g).all().item()), g.abs().max().item(), g.numel())
    out["runs"] = runs
    dist.barrier()
    dist.destroy_process_group()


# (gradient relative to its max, running buffers other than the frozen encoder's, relative).  One rank: the collectives are
# identities, so only the statistics' arithmetic differs -- float64-merged slab moments against the fp32 one-pass local
# statistics (~1e-7 relative, see the kernel tests).  Measured on the MI355X: groups 1-3 in bf16x3, gradients 5.0e-6 and
# buffers 5.2e-7 (the BatchNorm backwards amplify the 1e-7 as in the two-rank test); the whole encoder under recompute16 with
# fp16 storage, gradients 2.1e-2 and buffers 1.5e-4 -- there a 1e-7 change of a statistic flips fp16 roundings (2^-11) of the
# normalised plane and of every narrow activation, the per-operation error of that plan, which its own test holds at ~1e-2
# against float64 (tests/test_head_release_gpu.py).  Bars at 2x the measured values.
FORCED_BARS = {"g123": (1.1e-5, 1.1e-6), "all": (4.2e-2, 3e-4)}


def test_forced_single_rank_sync_released_matches_the_unsynced_step():
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        out = mgr.dict()
        mp.spawn(_child_forced, args=(_free_port(), out), nprocs=1, join=True)
        res = dict(out)
    checks = []
    for release, precision, memory in FORCED:
        off = res["runs"][(release, precision, memory, "False")]
        on = res["runs"][(release, precision, memory, "force")]
        frozen = [n for n in off[2] if n.rsplit(".", 1)[0] in off[3]]
        for n in frozen:                                # frozen encoder BatchNorm2d: the finalize of one rank is the identity
            assert torch.equal(off[2][n], on[2][n]), n
        rest = [n for n in off[2] if n not in frozen]
        gerr = (off[0] - on[0]).abs().max().item() / off[0].abs().max().item()
        berr = max((off[2][n] - on[2][n]).abs().max().item() / max(off[2][n].abs().max().item(), 1e-30) for n in rest)
        print(f"\n[sync_released force x1 {release} {precision} {memory}] {len(frozen) // 2} frozen BatchNorm2d bit-identical, "
              f"{on[4]} released BatchNorms; gradients {gerr:.2e}, other running buffers {berr:.2e}")
        # groups 1-3 leave the stem and units 0-17 frozen: 1 + 2 x 18 BatchNorm2d + the shortcut BatchNorms of units 3 and 7
        assert len(frozen) == 2 * ({"g123": 39, "all": 0}[release]) and on[4] == {"g123": 15, "all": 2 + 1 + 2 * 24 + 3}[release]
        checks.append((release, gerr, berr))
    finite, gmax, n = res["at224"]
    print(f"[sync_released force x1 224x224 1 clip x {L} frames, groups 1-3] {n} gradients, finite {finite}, max |g| {gmax:.2e}")
    assert finite and gmax > 0 and math.isfinite(gmax)
    for release, gerr, berr in checks:
        gbar, bbar = FORCED_BARS[release]
        assert gerr < gbar and berr < bbar, (release, gerr, berr)
