"""Host side of ``ClipDataParallel(sync_bn=..., sync_released=True)``, no GPU: the switch needs ``sync_bn``, reaches the IR-50
encoder and survives a deep copy, lets released encoder parameters through (and only then), and the new BatchNorm wrappers
check their arguments before any launch."""
import copy
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

MODS = ["video", "vggish", "bert"]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _lfan():
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.lfan import LFAN
    m = LFAN(backbone_settings={}, output_dim=7, task="CLASSIFICATION", modality=MODS, example_length=8, kernel_size=5,
             tcn_channel=synth.TCN_CHANNELS, root_dir="", device="cpu", head_hw=5)
    m.init(load_backbone=False)
    return m


def _release_groups_1_to_3(m):
    from feature_vs_text_compound_emotion_amd.parameter_control import ResnetParamControl
    pc = ResnetParamControl(trainer=None)
    return sum(len(pc.release_param(m.spatial)) for _ in range(3))


def test_sync_released_without_sync_bn_is_a_value_error():
    from feature_vs_text_compound_emotion_amd.data_parallel import ClipDataParallel
    for sync_bn in (False, None, 0):
        with pytest.raises(ValueError, match="sync_bn"):
            ClipDataParallel(_lfan(), world_size=1, sync_bn=sync_bn, sync_released=True)
    # one rank without "force": nothing to synchronise, the switch is accepted and attaches nothing
    m = _lfan()
    ddp = ClipDataParallel(m, world_size=1, sync_bn=True, sync_released=True)
    assert ddp.bn_sync is None and not m.spatial["visual"].backbone.sync_released


def _child(rank, port, out):
    os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import sys
    sys.modules.setdefault("triton", None)
    import torch.distributed as dist
    from feature_vs_text_compound_emotion_amd.data_parallel import ClipDataParallel, init_process_group_from_env
    init_process_group_from_env(backend="gloo", single_rank_group=True)
    res = {}
    for released in (False, True):
        m = _lfan()
        res[f"n_released_{released}"] = _release_groups_1_to_3(m)
        ddp = ClipDataParallel(m, sync_bn="force", sync_released=released)
        vis = m.spatial["visual"].backbone
        res[f"flag_{released}"] = vis.sync_released
        res[f"sync_{released}"] = vis.bn_sync is ddp.bn_sync and ddp.bn_sync is not None
        c = copy.deepcopy(m).spatial["visual"].backbone
        res[f"copy_flag_{released}"] = c.sync_released
        res[f"copy_sync_{released}"] = c.bn_sync is ddp.bn_sync
        m.train()
        try:
            vis.check_sync_release()
            res[f"check_{released}"] = "passed"
        except NotImplementedError as e:
            res[f"check_{released}"] = str(e)
    dist.destroy_process_group()
    out.update(res)


def test_flag_reaches_the_encoder_survives_deepcopy_and_gates_released_units():
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        out = mgr.dict()
        mp.spawn(_child, args=(_free_port(), out), nprocs=1, join=True)
        res = dict(out)
    # groups 1-3 of the reference's release: output layer (6 tensors), stage 4 (24), the second half of stage 3 (21)
    assert res["n_released_False"] == res["n_released_True"] == 6 + 24 + 21
    assert res["flag_True"] is True and res["copy_flag_True"] is True
    assert res["flag_False"] is False and res["copy_flag_False"] is False
    assert res["sync_True"] and res["sync_False"] and res["copy_sync_True"] and res["copy_sync_False"]
    assert res["check_True"] == "passed"
    # sync_bn alone: still refused, with the message the existing tests assert
    assert "not implemented" in res["check_False"] and "_ReleasedUnit" in res["check_False"], res["check_False"]
    assert "sync_released=True" in res["check_False"]


def test_new_batchnorm_wrappers_reject_bad_arguments_before_launching():
    from feature_vs_text_compound_emotion_amd import ops
    c = 8
    x, v = torch.zeros(4, c), torch.ones(c)
    sums = torch.zeros(2, c)
    calls = [
        lambda: ops.bn_rows_moments_large(x),                                          # host tensor
        lambda: ops.bn_rows_moments_large(torch.zeros(4, c, dtype=torch.float64)),
        lambda: ops.bn_rows_moments_large(torch.zeros(4, c)[:, :6]),
        lambda: ops.bn_rows_moments_large(torch.zeros(c)),
        lambda: ops.bn_rows_bwd_apply(x, x, v, v, v, sums, 4),
        lambda: ops.bn_rows_bwd_apply(x, x, v, v, v, sums, 4, split_out=True),
        lambda: ops.bn_rows_bwd_apply(x, x, v, v, v, sums, 4, add=x),
        lambda: ops.bn_rows_bwd_apply(x, x, v, v, None, sums, 4),
    ]
    for call in calls:
        with pytest.raises(ValueError):
            call()
