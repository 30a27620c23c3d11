"""Synchronised batch statistics across data-parallel ranks (``ClipDataParallel(sync_bn=...)``).

(a) The split BatchNorm kernels against float64: partial sums + finalize-from-sums == ``cer_bn_finalize`` bit for bit;
    the rank-order merge of (count, mean, M2) of uneven row blocks (means ~1e3, std 1) against the statistics of the
    concatenated rows; the backward apply with global sums against float64 autograd BatchNorm on the concatenated rows.
(b) 2 gloo ranks x B/2 clips with ``sync_bn=True`` equal 1 process x B clips in train mode (batch-statistics BatchNorm in
    the encoder and the tail) -- the test that an unsynchronised data-parallel step fails, shown by running it too.
(c) ``sync_bn="force"`` on a single-rank RCCL communicator: the encoder's BatchNorm2d statistics are bit-identical to
    ``sync_bn=False``, the row BatchNorms within a stated fp32 bound.
"""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # fp32 unit roundoff
EPS, MOMENTUM = 1e-5, 0.1


# ------------------------------------------------------------------ (a) kernels against float64
@pytest.mark.parametrize("tiles,c", [(1, 64), (7, 100), (600, 64), (1500, 512)])
def test_partial_sums_then_finalize_equals_bn_finalize_bit_for_bit(tiles, c):
    from feature_vs_text_compound_emotion_amd import ops
    g = torch.Generator().manual_seed(tiles * 1000 + c)
    x = (torch.randn(tiles, 8, c, generator=g) * 2.0 + 3.0)
    partials = torch.stack([x.sum(1), (x * x).sum(1)], dim=1).float().cuda()        # [tiles, 2, C]
    count = float(tiles * 8)
    gamma = (torch.rand(c, generator=g) + 0.5).cuda()
    beta = torch.randn(c, generator=g).cuda()
    rm0, rv0 = torch.randn(c, generator=g).cuda(), (torch.rand(c, generator=g) + 0.5).cuda()
    rm_a, rv_a, rm_b, rv_b = rm0.clone(), rv0.clone(), rm0.clone(), rv0.clone()
    s_a, t_a = ops.bn_finalize(partials, count, gamma, beta, rm_a, rv_a, momentum=MOMENTUM, eps=EPS)
    sums = ops.bn_partial_sums(partials)
    s_b, t_b = ops.bn_finalize_sums(sums, count, gamma, beta, rm_b, rv_b, momentum=MOMENTUM, eps=EPS)
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (2, c)
    ref = partials.double().sum(0).cpu()
    assert ((sums.cpu() - ref).abs() <= 1e-12 * ref.abs().clamp_min(1.0)).all()
    for a, b in ((s_a, s_b), (t_a, t_b), (rm_a, rm_b), (rv_a, rv_b)):
        assert torch.equal(a, b)
    # without running buffers (the statistics alone)
    s_c, t_c = ops.bn_finalize_sums(sums, count, gamma, beta, momentum=MOMENTUM, eps=EPS)
    assert torch.equal(s_c, s_a) and torch.equal(t_c, t_a)


def _blocks(sizes, c, seed, offset=1000.0):
    """Row blocks with per-channel means around ``offset`` (std 1) and a small shift per block, so that the between-block
    term of the merge matters."""
    g = torch.Generator().manual_seed(seed)
    base = offset + 5.0 * torch.randn(c, generator=g)
    return [(base + 0.5 * torch.randn(1, c, generator=g) + torch.randn(n, c, generator=g)).float() for n in sizes]


SIZES = [5, 17, 1, 33]


@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("pitched", [False, True])
def test_merged_moments_of_uneven_blocks_match_float64_over_the_concatenated_rows(k, pitched):
    from feature_vs_text_compound_emotion_amd import ops
    c = 48
    blocks = _blocks(SIZES[:k], c, seed=k)
    mom = []
    for b in blocks:
        xb = b.cuda()
        if pitched:                     # a column slice of a wider buffer, as LFAN's leader rows are
            wide = torch.zeros(b.shape[0], c + 16, device="cuda")
            wide[:, 3:3 + c] = xb
            xb = wide[:, 3:3 + c]
        mom.append(ops.bn_rows_moments(xb))
    moments = torch.stack(mom)                                      # [K, 3, C], rank order
    g = torch.Generator().manual_seed(77)
    rm0, rv0 = torch.randn(c, generator=g).cuda(), (torch.rand(c, generator=g) + 0.5).cuda()
    rm, rv = rm0.clone(), rv0.clone()
    sm, si = ops.bn_rows_merge(moments, rm, rv, EPS, MOMENTUM)
    x64 = torch.cat(blocks).double()
    n = x64.shape[0]
    mean = x64.mean(0)
    var = x64.var(0, unbiased=False)
    unbiased = x64.var(0, unbiased=True) if n > 1 else var
    invstd = 1.0 / torch.sqrt(var + EPS)
    # the float64 merge is exact to ~1e-12 here; what remains is ONE rounding of each result to fp32 (<= U relative) and,
    # for the running buffers, the fp32 update (1 - m) * r + m * v (a few roundings of values of size |r| + |v|)
    assert ((sm.cpu().double() - mean).abs() <= 2 * U * mean.abs()).all()
    assert ((si.cpu().double() - invstd).abs() <= 2 * U * invstd.abs()).all()
    rm_ref = (1 - MOMENTUM) * rm0.cpu().double() + MOMENTUM * mean
    rv_ref = (1 - MOMENTUM) * rv0.cpu().double() + MOMENTUM * unbiased
    assert ((rm.cpu().double() - rm_ref).abs() <= 8 * U * (rm0.cpu().double().abs() + mean.abs())).all()
    assert ((rv.cpu().double() - rv_ref).abs() <= 8 * U * (rv0.cpu().double().abs() + unbiased.abs())).all()
    # statistics from raw sums in fp32 would be far off at this offset: the test data discriminates
    s1, s2 = x64.float().sum(0), (x64.float() ** 2).sum(0)
    naive_var = (s2 / n - (s1 / n) ** 2).double()
    assert (naive_var - var).abs().max().item() > 0.01
    # every rank merges the same gathered blocks: same bits
    sm2, si2 = ops.bn_rows_merge(moments.clone())
    assert torch.equal(sm, sm2) and torch.equal(si, si2)
    # the apply pass into a pitched output
    w = torch.rand(c, generator=g).cuda() + 0.5
    b = torch.randn(c, generator=g).cuda()
    x0 = blocks[0].cuda()
    z = torch.full((x0.shape[0], c + 8), 7.0, device="cuda")
    y = ops.bn_rows_apply(x0, sm, si, w, b, out=z[:, :c])
    assert y.data_ptr() == z.data_ptr() and (z[:, c:] == 7.0).all()
    y_ref = (x0.double() - sm.double()) * si.double() * w.double() + b.double()
    assert ((y.double() - y_ref).abs() <= 8 * U * (1.0 + y_ref.abs())).all()      # a few fp32 roundings of O(1) terms


@pytest.mark.parametrize("k", [1, 2, 4])
def test_backward_apply_with_global_sums_matches_float64_autograd_on_the_concatenated_rows(k):
    """Each block plays a rank with dy = world x (its rows of the full-batch dy), as a mean loss over a 1/world shard gives;
    its dx must then be world x the full-batch dx of its rows, and its local sums are its dw / db."""
    from feature_vs_text_compound_emotion_amd import ops
    c = 48
    blocks = _blocks(SIZES[:k], c, seed=10 + k)
    g = torch.Generator().manual_seed(5)
    dys = [torch.randn(b.shape[0], c, generator=g) for b in blocks]
    w = torch.rand(c, generator=g) + 0.5
    bias = torch.randn(c, generator=g)
    x64 = torch.cat(blocks).double().requires_grad_(True)
    w64, b64 = w.double().requires_grad_(True), bias.double().requires_grad_(True)
    y64 = torch.nn.functional.batch_norm(x64, None, None, w64, b64, training=True, eps=EPS)
    dy64 = torch.cat(dys).double()
    (y64 * dy64).sum().backward()
    n = x64.shape[0]
    sm, si = ops.bn_rows_merge(torch.stack([ops.bn_rows_moments(b.cuda()) for b in blocks]))
    world = float(k)
    local = [ops.bn_rows_bwd_sums((world * dy).cuda(), b.cuda(), sm, si) for dy, b in zip(dys, blocks)]
    total = local[0].clone()
    for s in local[1:]:
        total += s
    xhat64 = ((x64.detach() - x64.detach().mean(0)) / torch.sqrt(x64.detach().var(0, unbiased=False) + EPS))
    r0 = 0
    for dy, b, s in zip(dys, blocks, local):
        r1 = r0 + b.shape[0]
        dx = ops.bn_rows_bwd_apply((world * dy).cuda(), b.cuda(), sm, si, w.cuda(), total, n)
        ref = world * x64.grad[r0:r1]
        # x_hat is formed in fp32 from x ~ 1e3 and the fp32 mean: an absolute error up to |mean| * U / std ~ 6e-5, which
        # the sum over the n rows and the 1/n of the formula bring back to that order times |w| * invstd * world
        tol = 32 * 1000.0 * U * world * (1.0 + dy64.abs().max().item()) * (w.abs().max().item() + 1.0)
        err = (dx.cpu().double() - ref).abs().max().item()
        assert err <= tol, (err, tol)
        db_ref = world * dy.double().sum(0)
        dw_ref = world * (dy.double() * xhat64[r0:r1]).sum(0)
        assert (s[0].cpu().double() - db_ref).abs().max().item() <= 64 * U * world * dy.abs().sum(0).max().item() + 1e-6
        assert (s[1].cpu().double() - dw_ref).abs().max().item() <= tol * b.shape[0]
        r0 = r1
    # the global sums are the full batch's dw / db (times world)
    assert (total[0].cpu().double() - world * b64.grad).abs().max().item() <= 1e-4 * world * n
    assert (total[1].cpu().double() - world * w64.grad).abs().max().item() <= 1e-3 * world * n


def test_split_wrappers_check_their_arguments_before_launching():
    from feature_vs_text_compound_emotion_amd import ops
    c = 32
    x = torch.randn(6, c, device="cuda")
    v = torch.ones(c, device="cuda")
    sm, si = ops.bn_rows_merge(ops.bn_rows_moments(x).unsqueeze(0))
    with pytest.raises(ValueError):
        ops.bn_partial_sums(torch.zeros(4, c, device="cuda"))                      # not [tiles, 2, C]
    with pytest.raises(ValueError):
        ops.bn_finalize_sums(torch.zeros(2, c, device="cuda"), 10, v, v)           # float32 sums
    with pytest.raises(ValueError):
        ops.bn_finalize_sums(torch.zeros(2, c, device="cuda", dtype=torch.float64), 0, v, v)   # count 0
    with pytest.raises(ValueError):
        ops.bn_finalize_sums(torch.zeros(2, c, device="cuda", dtype=torch.float64), 10, v, v[:8])
    with pytest.raises(ValueError):
        ops.bn_rows_moments(x.double())
    with pytest.raises(ValueError):
        ops.bn_rows_merge(ops.bn_rows_moments(x).float().unsqueeze(0))            # float32 moments
    with pytest.raises(ValueError):
        ops.bn_rows_merge(ops.bn_rows_moments(x))                                  # not [K, 3, C]
    with pytest.raises(ValueError):
        ops.bn_rows_merge(ops.bn_rows_moments(x).unsqueeze(0), v, None)            # running buffers go together
    with pytest.raises(ValueError):
        ops.bn_rows_apply(x, sm, si, v, v, out=torch.empty(6, c + 1, device="cuda"))
    with pytest.raises(ValueError):
        ops.bn_rows_bwd_sums(x, x[:5], sm, si)
    with pytest.raises(ValueError):
        ops.bn_rows_bwd_apply(x, x, sm, si, v, torch.zeros(c, device="cuda"), 6)   # sums not [2, C]
    with pytest.raises(ValueError):
        ops.bn_rows_bwd_apply(x, x, sm, si, v, torch.zeros(2, c, device="cuda"), 0)


# ------------------------------------------------------------------ (b) 2 ranks x B/2 == 1 process x B, train mode
MODS_LFAN, MODS_CAN = ["video", "vggish", "bert"], ["video", "vggish"]
B, L, HW = 4, 8, 40
# (model, precision, sync_bn) run by the two ranks in one spawn
CASES = [("lfan", "bf16x3", True), ("lfan", "bf16x3", False), ("can", "bf16x3", True), ("can", "bf16x3", False),
         ("lfan", "fp32", True)]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _model(kind, precision, seed=0):
    from feature_vs_text_compound_emotion_amd import synth
    if kind == "lfan":
        from feature_vs_text_compound_emotion_amd.lfan import LFAN
        sd = synth.lfan_state_dict(MODS_LFAN, n_cls=7, head_hw=HW // 8, seed=seed)
        m = LFAN(backbone_settings={}, output_dim=7, task="CLASSIFICATION", modality=MODS_LFAN, example_length=L,
                 kernel_size=5, tcn_channel=synth.TCN_CHANNELS, root_dir="", device="cuda", head_hw=HW // 8)
        m.init(load_backbone=False)
    else:
        from feature_vs_text_compound_emotion_amd.fusion_heads import CAN
        spec, alias = synth.can_spec(MODS_CAN, head_hw=HW // 8)
        sd = synth.make_state_dict(spec, alias, seed=seed)
        m = CAN(task="CLASSIFICATION", modalities=MODS_CAN, tcn_settings=synth.TCN_SETTINGS, backbone_settings={},
                output_dim=7, root_dir="", device="cuda", head_hw=HW // 8, load_backbone=False)
    m.load_state_dict(sd, strict=True)
    m.spatial["visual"].backbone.precision = precision
    m = m.cuda().train()                               # batch-statistics BatchNorm everywhere, dropout off
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    for net in m.temporal.values():
        net.dropout = 0.0
    return m


def _batch(kind):
    from feature_vs_text_compound_emotion_amd import synth
    return synth.make_clip_batch(MODS_LFAN if kind == "lfan" else MODS_CAN, B, L, hw=HW, seed=55)


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
    from feature_vs_text_compound_emotion_amd.data_parallel import ClipDataParallel, FlatNesterovSGD, init_process_group_from_env
    init_process_group_from_env(backend="gloo")
    torch.cuda.set_device(0)
    res = {}
    for kind, precision, sync in CASES:
        model = _model(kind, precision, seed=rank)      # different weights per rank: broadcast_state makes them rank 0's
        ddp = ClipDataParallel(model, overlap=True, bucket_mb=2.0, sync_bn=sync)
        assert (ddp.bn_sync is not None) == sync
        opt = FlatNesterovSGD(ddp, lr=1e-3)
        x, labels = _batch(kind)
        idx = ddp.shard(list(range(B)), rank)
        _, g, w = _step(model, ddp, opt, {k: v[idx].cuda() for k, v in x.items()}, labels[idx].cuda())
        res[(kind, precision, sync)] = (g.cpu(), w.cpu(), _running(model))
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


def _single(kind, precision):
    from feature_vs_text_compound_emotion_amd.data_parallel import ClipDataParallel, FlatNesterovSGD
    model = _model(kind, precision, seed=0)
    ddp = ClipDataParallel(model, world_size=1)
    opt = FlatNesterovSGD(ddp, lr=1e-3)
    x, labels = _batch(kind)
    _, g, w = _step(model, ddp, opt, {k: v.cuda() for k, v in x.items()}, labels.cuda())
    return g.cpu(), w.cpu(), _running(model)


def _errors(ref, got):
    g, w, run = ref
    g1, w1, run1 = got
    gerr = (g - g1).abs().max().item() / g.abs().max().item()
    werr = (w - w1).abs().max().item()
    berr = max((run[n] - run1[n]).abs().max().item() / run[n].abs().max().item() for n in run)
    return gerr, werr, berr


@pytest.mark.parametrize("kind,precision", [("lfan", "bf16x3"), ("can", "bf16x3"), ("lfan", "fp32")])
def test_two_synced_ranks_on_half_batches_equal_one_process_on_the_full_batch_in_train_mode(two_ranks, kind, precision):
    r0, r1 = two_ranks
    s0, s1 = r0[(kind, precision, True)], r1[(kind, precision, True)]
    assert torch.equal(s0[0], s1[0]) and torch.equal(s0[1], s1[1])     # one reduced gradient, weights in lockstep
    assert set(s0[2]) == set(s1[2]) and len(s0[2]) >= 2 * 54
    for n in s0[2]:                                                     # the running buffers stay one set
        assert torch.equal(s0[2][n], s1[2][n]), n
    ref = _single(kind, precision)
    gerr, werr, berr = _errors(ref, s0)
    print(f"\n[sync_bn {kind} {precision}] 2 synced ranks x {B // 2} clips vs 1 process x {B} clips: gradient {gerr:.2e}, "
          f"weights {werr:.2e}, running buffers {berr:.2e}")
    if (kind, precision, False) in r0:
        ugerr, uwerr, uberr = _errors(ref, r0[(kind, precision, False)])
        print(f"[sync_bn {kind} {precision}] the same without sync_bn: gradient {ugerr:.2e}, weights {uwerr:.2e}, "
              f"running buffers {uberr:.2e}")
        assert max(ugerr / 1e-4, uberr / 5e-6) > 100      # the bars below tell a synchronised step from a local one
    # Bars.  Weights: one fp32 ulp of a weight in [1, 2) is 2^-23 = 1.19e-7, and a gradient difference far below the bar
    # can still flip the last bit of w - lr * update (measured: exactly 1.19e-7 for LFAN fp32), so the eval-mode test's
    # 1e-7 becomes 2 ulps of such a weight, 2.4e-7.  The gradient and running-buffer bars of that test
    # (2e-5, 1e-6) do not hold in train mode, and not because of the exchange: the encoder picks its conv kernels by the
    # output pixel count M = frames x Ho x Wo (conv_b3_tile_dims, conv_igemm), so B/2 and B frames accumulate the same
    # products in different orders -- ~U * sqrt(K) per element, as in eval mode -- and 53 batch-statistics BatchNorms pass
    # these differences on to the statistics (E[x^2] - E[x]^2 over fp32 tile partials whose grouping also follows M).  The
    # BatchNorm backward (dy minus its projections on 1 and x_hat) then amplifies the relative difference of small gradients.
    # Measured on the MI355X: gradient 5.0e-5 / 1.5e-5 / 2.5e-5 (LFAN bf16x3 / CAN / LFAN fp32), running buffers 2.1e-6 /
    # 2.1e-6 / 3.7e-7; the forced single-rank run, where only the row statistics' precision differs, stays below both.
    # The bars sit at 2x the worst measured value; the unsynchronised step misses them by four orders of magnitude.
    assert gerr < 1e-4
    assert werr < 2.4e-7
    assert berr < 5e-6


# ------------------------------------------------------------------ (c) world 1, forced, on RCCL
def _child_forced(rank, port, out):
    os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    import sys
    sys.modules.setdefault("triton", None)
    import torch.distributed as dist
    from feature_vs_text_compound_emotion_amd.data_parallel import ClipDataParallel, FlatNesterovSGD, init_process_group_from_env
    init_process_group_from_env(backend="nccl", single_rank_group=True)
    assert dist.get_backend() == "nccl" and dist.get_world_size() == 1
    x, labels = _batch("lfan")
    xd, ld = {k: v.cuda() for k, v in x.items()}, labels.cuda()
    runs = {}
    for sync in (False, "force"):
        model = _model("lfan", "bf16x3")
        ddp = ClipDataParallel(model, overlap="force", bucket_mb=1.0, sync_bn=sync)
        assert (ddp.bn_sync is not None) == bool(sync)
        opt = FlatNesterovSGD(ddp, lr=1e-3)
        steps = [_step(model, ddp, opt, xd, ld) for _ in range(2)]
        torch.cuda.synchronize()
        bn2d = {n for n, m in model.named_modules() if isinstance(m, torch.nn.BatchNorm2d)}
        runs[sync] = (torch.stack([s[0] for s in steps]).cpu(), torch.stack([s[1] for s in steps]).cpu(), _running(model),
                      bn2d)
    out["runs"] = {str(k): v for k, v in runs.items()}
    # a released encoder unit is refused before anything runs: no buffer moves, no dropout stream advances
    model = _model("lfan", "bf16x3")
    for p in model.spatial["visual"].backbone.body[-1].parameters():
        p.requires_grad = True
    for p in model.spatial["visual"].backbone.output_layer.parameters():
        p.requires_grad = True
    ddp = ClipDataParallel(model, sync_bn="force")
    before, seed = _running(model), model.dropout_seed
    torch.cuda.synchronize()
    try:
        model(dict(xd))
        out["released"] = "no error"
    except NotImplementedError as e:
        torch.cuda.synchronize()
        after = _running(model)
        out["released"] = str(e) if all(torch.equal(before[n], after[n]) for n in before) and model.dropout_seed == seed \
            else "state moved"
    dist.barrier()
    dist.destroy_process_group()


def test_forced_single_rank_sync_matches_the_unsynced_step():
    """Bars.  Encoder BatchNorm2d: the all-reduce of one rank is the identity and the finalize is cer_bn_finalize's formula,
    so its running buffers must match bit for bit.  Row BatchNorms: the synchronised path takes the statistics in float64
    (moments + merge) where the local path sums the R = 32 rows in fp32 -- a relative difference of at most ~R * U = 1.9e-6
    in mean and variance, 4e-6 allowing for the fp32 running update.  Logits carry that perturbation at about its own size
    (bar 2e-5); gradients pass it through the BatchNorm backwards, which amplify small relative differences (see the bars of
    the two-rank test), so they get that test's 1e-4."""
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        out = mgr.dict()
        mp.spawn(_child_forced, args=(_free_port(), out), nprocs=1, join=True)
        res = dict(out)
    off, on = res["runs"]["False"], res["runs"]["force"]
    lerr = (off[0] - on[0]).abs().max().item() / off[0].abs().max().item()
    gerr = (off[1] - on[1]).abs().max().item() / off[1].abs().max().item()
    bn2d = off[3]
    enc = [n for n in off[2] if n.rsplit(".", 1)[0] in bn2d]
    rows = [n for n in off[2] if n not in enc]
    assert len(enc) == 2 * 53 and len(rows) == 2 * (1 + len(MODS_LFAN))
    for n in enc:
        assert torch.equal(off[2][n], on[2][n]), n
    rerr = max((off[2][n] - on[2][n]).abs().max().item() / off[2][n].abs().max().item() for n in rows)
    print(f"\n[sync_bn force x1] logits {lerr:.2e}, gradients {gerr:.2e}, row BatchNorm running buffers {rerr:.2e}; "
          f"released unit: {res['released']}")
    assert lerr < 2e-5 and gerr < 1e-4
    assert rerr < 4e-6
    assert "not implemented" in res["released"] and "_ReleasedUnit" in res["released"], res["released"]
