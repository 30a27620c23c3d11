"""Ragged streaming on the GPU: streams that advance independently (``push_ragged``, the row-table entry points) return, bit
for bit, what each stream returns when it is pushed alone through the lockstep path; a wrong row table stays inside the rings;
and ``CANStream`` returns what the offline CAN returns, the same bits however the frames are pushed."""
import functools
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import stream_ref  # noqa: E402
from helpers import golden  # noqa: E402
from stream_ref import BLOCK_CASES, SLOPE  # noqa: E402
from test_stream_gpu import BIMODAL, LFAN_TOL, _Arena, _bimodal, _fixture, _lfan, _push_all, _push_lfan, _tcn  # noqa: E402

CAN_TOL = 1e-4      # tests/test_heads_gpu.py:40, the bar the offline CAN forward is held to on the same fixture


def _pkg():
    from feature_vs_text_compound_emotion_amd import ops, streaming
    return ops, streaming


def _schedule(total, streams, max_new, seed, late=None, lonely_every=0):
    """Ticks of per-stream counts in 0 .. max_new until every stream has had ``total`` frames.  ``late`` = (stream, ticks):
    that stream gets nothing during its first ticks.  Every ``lonely_every``-th tick brings one frame to one stream only."""
    rng, fed, ticks = random.Random(seed), [0] * streams, []
    while min(fed) < total:
        tick = len(ticks)
        open_ = [s for s in range(streams) if fed[s] < total and not (late and s == late[0] and tick < late[1])]
        counts = [0] * streams
        if lonely_every and tick % lonely_every == lonely_every - 1:
            if open_:
                counts[rng.choice(open_)] = 1
        else:
            for s in open_:
                counts[s] = min(rng.randint(0, max_new), total - fed[s])
        fed = [f + c for f, c in zip(fed, counts)]
        ticks.append(counts)
    return ticks


def _pack(x, fed, counts):
    """The next counts[s] frames of every stream of x [S, T, C], packed stream-major: [M, C]."""
    return torch.cat([x[s, fed[s]:fed[s] + c] for s, c in enumerate(counts)])


def _unpack(out, counts, into):
    row = 0
    for s, c in enumerate(counts):
        into[s].append(out[row:row + c])
        row += c
    assert row == out.shape[0]


def _drive(push, x, ticks, fed=None):
    """x [S, T, C] through ``push(packed rows, counts)`` tick by tick: per-stream outputs [n_s, Cout] and the final ``fed``."""
    fed = [0] * x.shape[0] if fed is None else list(fed)
    outs = [[] for _ in range(x.shape[0])]
    for counts in ticks:
        _unpack(push(_pack(x, fed, counts), counts), counts, outs)
        fed = [f + c for f, c in zip(fed, counts)]
    return [torch.cat(o) for o in outs], fed


# ---------------------------------------------------------------------------------------------- 1. ragged = alone, bitwise
_NETS = {"": (40, [32, 32, 16, 16]), "-gather40-L5": None, "-odd39": (39, [30, 16])}


def _net_of(geometry):
    if geometry == "-gather40-L5":
        from test_tail_gpu import _TCN_GEOMETRIES
        cin, channels, _, _ = _TCN_GEOMETRIES[geometry]
        return cin, channels
    return _NETS[geometry]


@pytest.mark.parametrize("geometry", list(_NETS))
def test_each_stream_of_a_ragged_schedule_equals_that_stream_pushed_alone(geometry):
    """S = 5, 200 frames per stream, max_new = 8 (rings of 16 to 64 frames: every ring wraps several times, at another phase
    per stream); stream 3 joins 40 ticks late and every fifth tick brings one frame to one stream.  "-odd39": channel counts
    that are no multiple of 4, the element-wise load path."""
    _, streaming = _pkg()
    cin, channels = _net_of(geometry)
    net, _ = _tcn(cin, channels)
    s, total, max_new = 5, 200, 8
    x = torch.randn(s, total, cin, generator=torch.Generator().manual_seed(31)).cuda()
    ticks = _schedule(total, s, max_new, seed=5, late=(3, 40), lonely_every=5)
    assert all(t[3] == 0 for t in ticks[:40]) and any(sum(t) == 1 for t in ticks) and max(max(t) for t in ticks) == max_new
    assert len({tuple(t) for t in ticks}) > 20
    stream = streaming.TCNStream(net, s, max_new=max_new)
    if geometry == "":
        assert stream.ring_frames == [16, 16, 32, 64]
    got, fed = _drive(stream.push_ragged, x, ticks)
    assert fed == [total] * s and stream.frames_seen == [total] * s
    for pick in range(s):
        alone = _push_all(streaming.TCNStream(net, 1, max_new=max_new), x[pick:pick + 1].contiguous(), [2, 5, 8])
        assert torch.isfinite(alone).all() and alone.abs().max().item() > 0
        assert torch.equal(got[pick], alone[0]), pick
    empty = stream.push_ragged(x.new_empty(0, cin), [0] * s)
    assert tuple(empty.shape) == (0, channels[-1]) and stream.frames_seen == [total] * s


# ---------------------------------------------------------------------------------------------- 2. mixed use
def test_dense_and_ragged_pushes_mix():
    """Dense pushes while the positions are equal run the lockstep launches; after ragged pushes the same dense call goes
    through the row table (also in chunks of max_new), and every stream still equals itself alone."""
    ops, streaming = _pkg()
    net, _ = _tcn(40, [32, 32, 16, 16])
    s, total, max_new = 3, 90, 4
    x = torch.randn(s, total, 40, generator=torch.Generator().manual_seed(33)).cuda()
    stream = streaming.TCNStream(net, s, max_new=max_new)
    outs = [[] for _ in range(s)]
    ops.STREAM_TRACE = trace = []
    try:
        dense = stream.push_rows(x[:, :10].contiguous())                  # 10 frames in chunks of 4, 4, 2: lockstep
        assert {n for n, _ in trace} == {"append", "conv"} and stream.frames_seen == [10, 10, 10]
        for i in range(s):
            outs[i].append(dense[i])
        fed = [10] * s
        for counts in ([4, 0, 1], [0, 3, 0], [1, 1, 4], [0, 0, 0], [2, 4, 0]):
            _unpack(stream.push_ragged(_pack(x, fed, counts), counts), counts, outs)
            fed = [f + c for f, c in zip(fed, counts)]
            assert stream.frames_seen == fed
        assert fed == [17, 18, 15]
        del trace[:]
        for c in (1, 9, 4):                                               # dense again, the positions now unequal
            block = torch.stack([x[i, fed[i]:fed[i] + c] for i in range(s)])
            dense = stream.push_rows(block)
            for i in range(s):
                outs[i].append(dense[i])
            fed = [f + c for f in fed]
            assert stream.frames_seen == fed
        assert {n for n, _ in trace} == {"append_rows", "conv_rows"}
        assert [n for n, _ in trace].count("append_rows") == 1 + 3 + 1   # c = 9 goes in chunks of 4, 4, 1
        rest = [[total - f for f in fed]]
        while any(rest[-1]):                                              # ragged to the end of every stream
            counts = [min(max_new, r) for r in rest[-1]]
            _unpack(stream.push_ragged(_pack(x, fed, counts), counts), counts, outs)
            fed = [f + c for f, c in zip(fed, counts)]
            rest.append([total - f for f in fed])
    finally:
        ops.STREAM_TRACE = None
    assert stream.frames_seen == [total] * s
    for pick in range(s):
        alone = _push_all(streaming.TCNStream(net, 1, max_new=max_new), x[pick:pick + 1].contiguous(), [3, 4])
        assert torch.equal(torch.cat(outs[pick]), alone[0]), pick


# ---------------------------------------------------------------------------------------------- 3. one exact block
_ROWS_CASE = next(c for c in BLOCK_CASES if c.ds and c.misalign and c.s >= 2)


@functools.lru_cache(maxsize=None)
def _rows_block():
    case = _ROWS_CASE
    d = stream_ref.make_block(case)
    ref = stream_ref.block_ref(d["x"], d["w1"], d["b1"], d["w2"], d["b2"], d["dsw"], d["dsb"], case.k, case.dil)
    return case, d, ref


def _rows_arena(ops, streaming):
    case, d, ref = _rows_block()
    r = streaming.ring_frames(case.k, case.dil, case.max_new)
    arena = _Arena([(case.s, r, case.cin), (case.s, r, case.cout), (case.s, 2 * r, case.cout)], case.misalign)
    assert arena.rings[0].data_ptr() % 16 == 4 * case.misalign
    dev = {n: (None if v is None else v.cuda()) for n, v in d.items()}
    pack = {"k": case.k, "dil": case.dil, "w1": ops.pack_tcn_stream_weight(dev["w1"]), "b1": dev["b1"],
            "w2": ops.pack_tcn_stream_weight(dev["w2"]), "b2": dev["b2"],
            "dsw": ops.pack_tcn_stream_weight(dev["dsw"]), "dsb": dev["dsb"]}
    return case, dev, ref, r, arena, pack


def test_one_exact_block_through_the_rows_entry_equals_the_float64_block_bit_for_bit():
    """The projected, misaligned exact case of ``stream_ref.BLOCK_CASES`` with its streams at different positions (they start
    0, 5 and 2^30 - 3 frames in, so one of them crosses the wrap of ``row_pos``): bit-equal to the float64 whole-sequence
    block, nothing but the new slots changes, the guards stay NaN."""
    ops, streaming = _pkg()
    case, dev, ref, r, arena, pack = _rows_arena(ops, streaming)
    xring, hring, oring = arena.rings
    s, total = case.s, dev["x"].shape[1]
    start = [0, 5, 2 ** 30 - 3][:s]
    ticks = _schedule(total, s, case.max_new, seed=8, lonely_every=4)
    assert len({tuple(t) for t in ticks}) > 4
    fed, outs = [0] * s, [[] for _ in range(s)]
    stray = torch.zeros((), dtype=torch.bool, device="cuda")
    mirrored = torch.ones((), dtype=torch.bool, device="cuda")
    for counts in ticks:
        if not sum(counts):
            continue
        row_stream, row_pos = ops.stream_row_table([a + f for a, f in zip(start, fed)], counts, "cuda")
        before = arena.flat.clone()
        allowed = torch.zeros_like(arena.flat, dtype=torch.bool)
        for i, ring_len in enumerate((r, r, 2 * r)):
            for st, c in enumerate(counts):
                for j in range(c):
                    arena.view(allowed, i)[st, (start[st] + fed[st] + j) & (ring_len - 1)] = True
        dense = torch.empty(sum(counts), case.cout, device="cuda")
        ops.tcn_stream_append_rows(_pack(dev["x"], fed, counts), xring, row_stream, row_pos, max(counts))
        streaming.block_push_rows(pack, xring, hring, row_stream, row_pos, max(counts), out_ring=oring, out_dense=dense,
                                  slope=SLOPE)
        same = (arena.flat == before) | (torch.isnan(arena.flat) & torch.isnan(before))
        stray |= (~same & ~allowed).any()
        row = 0
        for st, c in enumerate(counts):
            for j in range(c):
                mirrored &= torch.equal(oring[st, (start[st] + fed[st] + j) & (2 * r - 1)], dense[row + j])
            row += c
        _unpack(dense, counts, outs)
        fed = [f + c for f, c in zip(fed, counts)]
    assert fed == [total] * s
    assert not stray.item()
    assert mirrored.item()
    assert arena.guards_are_nan()
    got = torch.stack([torch.cat(o) for o in outs]).cpu()
    assert torch.equal(got.double(), ref["out"])
    tail = torch.arange(total - r, total)
    for st in range(s):
        slots = ((tail + start[st]) & (r - 1)).cuda()
        assert torch.equal(hring[st, slots].cpu().double(), ref["h"][st, tail])


# ---------------------------------------------------------------------------------------------- 4. a poisoned table
def test_a_poisoned_row_table_stays_inside_the_rings():
    """Stream indices of -7 and S + 100 are clamped into [0, S) and every slot is masked by its ring length, so this launch
    is in bounds by construction: it returns OK, writes inside the rings only, and the NaN guards around them stay NaN."""
    ops, streaming = _pkg()
    case, dev, _, r, arena, pack = _rows_arena(ops, streaming)
    xring, hring, oring = arena.rings
    s = case.s
    g = torch.Generator().manual_seed(12)
    m = 19                                                     # three row tiles, the last one ragged
    row_stream = torch.tensor(([-7, s + 100, 1, -2 ** 31, 2 ** 31 - 1, 0, s] * 3)[:m], dtype=torch.int32).cuda()
    row_pos = torch.randint(0, 2 ** 30, (m,), generator=g, dtype=torch.int32)
    row_pos[:3] = torch.tensor([2 ** 30 - 1, 0, 123456789], dtype=torch.int32)
    row_pos = row_pos.cuda()
    rows = torch.ones(m, case.cin, device="cuda")
    dense = torch.empty(m, case.cout, device="cuda")
    ops.tcn_stream_append_rows(rows, xring, row_stream, row_pos, case.max_new)
    ops.tcn_stream_conv_rows(xring, row_stream, row_pos, case.max_new, pack["w1"], pack["b1"], case.k, case.dil, out_ring=hring,
                             slope=SLOPE)
    ops.tcn_stream_conv_rows(hring, row_stream, row_pos, case.max_new, pack["w2"], pack["b2"], case.k, case.dil, res_ring=xring,
                             res_w=pack["dsw"], res_bias=pack["dsb"], out_ring=oring, out_dense=dense, slope=SLOPE)
    torch.cuda.synchronize()
    assert arena.guards_are_nan()
    assert torch.isfinite(dense).all() and all(torch.isfinite(ring).all() for ring in arena.rings)
    assert xring.sum().item() > 0                               # the append did land, in some stream's ring


# ---------------------------------------------------------------------------------------------- 5. reset under ragged use
def test_reset_of_one_stream_in_the_middle_of_a_ragged_schedule():
    _, streaming = _pkg()
    net, _ = _tcn(40, [32, 32, 16, 16])
    total, max_new = 120, 4
    x = torch.randn(2, total, 40, generator=torch.Generator().manual_seed(41)).cuda()
    ticks = _schedule(total, 2, max_new, seed=6, lonely_every=3)
    cut = next(i for i in range(len(ticks)) if sum(t[1] for t in ticks[:i]) >= 37)
    stream = streaming.TCNStream(net, 2, max_new=max_new)
    head, fed = _drive(stream.push_ragged, x, ticks[:cut])
    t1 = fed[1]
    assert 37 <= t1 < 37 + max_new and fed[0] != fed[1] and stream.frames_seen == fed
    stream.reset([1])
    assert stream.frames_seen == [fed[0], 0]
    tail, fed = _drive(stream.push_ragged, x, ticks[cut:], fed)
    assert fed == [total, total] and stream.frames_seen == [total, total - t1]
    undisturbed = _push_all(streaming.TCNStream(net, 1, max_new=max_new), x[:1].contiguous(), [4, 1, 3])
    fresh = _push_all(streaming.TCNStream(net, 1, max_new=max_new), x[1:, t1:].contiguous(), [3])
    history = _push_all(streaming.TCNStream(net, 1, max_new=max_new), x[1:].contiguous(), [4])
    assert torch.equal(torch.cat([head[0], tail[0]]), undisturbed[0])
    assert torch.equal(tail[1], fresh[0])
    assert not torch.equal(tail[1], history[0, t1:])                 # the history did matter


# ---------------------------------------------------------------------------------------------- 6. LFAN
def _drive_model(push, x, ticks, axes):
    """x[m] with streams on axis 0 and time on axes[m], through ``push(packed dict, counts)``: per-stream logits."""
    s = next(iter(x.values())).shape[0]
    fed, outs = [0] * s, [[] for _ in range(s)]
    for counts in ticks:
        packed = {}
        for m, v in x.items():
            parts = [v[i].narrow(axes[m] - 1, fed[i], c) for i, c in enumerate(counts)]
            parts = [p.squeeze(0) if axes[m] == 2 else p for p in parts]        # [1, c, E] -> [c, E]
            packed[m] = torch.cat(parts, dim=0).contiguous()
        _unpack(push(packed, counts), counts, outs)
        fed = [f + c for f, c in zip(fed, counts)]
    return [torch.cat(o) for o in outs]


def test_lfan_ragged_pushes_equal_lockstep_bitwise_and_meet_the_oracle():
    _, streaming = _pkg()
    sd, x, ref = _bimodal()
    model = _lfan(BIMODAL, sd)
    total = ref.shape[1]
    lockstep = _push_lfan(streaming.LFANStream(model, 2, max_new=8), x, [1, 3, 2, 8, 1])
    ticks = _schedule(total, 2, 8, seed=7, late=(1, 6), lonely_every=4)
    axes = {m: 2 for m in BIMODAL}
    for how in ("push_ragged", "push_features_ragged"):
        stream = streaming.LFANStream(model, 2, max_new=8)
        got = torch.stack(_drive_model(getattr(stream, how), x, ticks, axes))
        assert stream.frames_seen == [total, total]
        err = (got.cpu().double() - ref).abs().max().item()
        print(f"LFAN {how}, {total} frames, against the float64 oracle: {err:.3e} (bar {LFAN_TOL:.0e})")
        assert torch.equal(got, lockstep), how
        assert err < LFAN_TOL, err
    reg = streaming.LFANStream(_lfan(BIMODAL, sd, task="REGRESSION"), 2, max_new=8)
    got = _drive_model(reg.push_features_ragged, x, ticks[:12], axes)
    assert sum(len(o) for o in got) > 20
    for i, o in enumerate(got):                                    # ops.tanh_fwd: double tanh, rounded once
        assert torch.equal(o.cpu(), torch.tanh(lockstep[i, :len(o)].cpu().double()).float())


def test_lfan_trimodal_ragged_push_through_the_encoders_meets_the_reference_fixture():
    _, streaming = _pkg()
    model, x, want, (b, l) = _fixture()
    assert b == 2 and l == 8
    ticks = [[3, 1], [0, 2], [2, 3], [0, 0], [3, 2]]
    stream = streaming.LFANStream(model, b, max_new=4)
    got = torch.stack(_drive_model(stream.push_ragged, x, ticks, {"video": 1, "vggish": 2, "bert": 2}))
    assert stream.frames_seen == [l] * b and tuple(got.shape) == want.shape
    err = np.abs(got.cpu().numpy() - want).max()
    print(f"LFAN tri-modal ragged push against the reference fixture: {err:.3e} (bar {LFAN_TOL:.0e})")
    assert err < LFAN_TOL, err


# ---------------------------------------------------------------------------------------------- 7. CAN
CAN_MODS = ["video", "vggish"]


def _can(sd, task="CLASSIFICATION"):
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.fusion_heads import CAN
    m = CAN(task=task, modalities=CAN_MODS, tcn_settings=synth.TCN_SETTINGS, backbone_settings={}, output_dim=7, root_dir="",
            device="cuda", load_backbone=False)
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


@functools.lru_cache(maxsize=None)
def _can_fixture():
    from feature_vs_text_compound_emotion_amd import synth
    g = golden("heads_can_jmt_mt.npz")
    b, l, hw, ncls, wseed, dseed = [int(v) for v in g["meta"]]
    assert ncls == 7
    spec, alias = synth.can_spec(CAN_MODS)
    sd = synth.make_state_dict(spec, alias, seed=wseed)
    x, _ = synth.make_clip_batch(CAN_MODS, b, l, hw=hw, seed=dseed)
    return sd, {k: v.cuda() for k, v in x.items()}, g["CAN_eval_logits"], (b, l)


def _frames(x, t0, c):
    return {m: v.narrow(1 if m == "video" else 2, t0, c) for m, v in x.items()}


@functools.lru_cache(maxsize=None)
def _can_runs():
    """The fixture's three clips through ``CANStream`` in every way of pushing, computed once: name -> logits [B, L, 7]."""
    _, streaming = _pkg()
    sd, x, want, (b, l) = _can_fixture()
    assert b == 3 and l == 8
    model = _can(sd)
    keys, shapes = list(x), {m: tuple(v.shape) for m, v in x.items()}
    got = {}
    stream = streaming.CANStream(model, b)
    got["frame_by_frame"] = torch.cat([stream.push(_frames(x, t, 1)) for t in range(l)], dim=1)
    assert stream.frames_seen == [l] * b
    stream.reset()
    assert stream.frames_seen == [0] * b
    got["one_push"] = stream.push(x)
    got["stream_forward"] = streaming.stream_forward(model, x, chunk=3)
    ticks = _schedule(l, b, 3, seed=4, late=(1, 2))                    # stream 1 starts two ticks behind the others
    assert ticks[0][1] == 0 and ticks[1][1] == 0 and len({tuple(t) for t in ticks}) >= 5
    ragged = streaming.CANStream(model, b, max_new=3)
    got["ragged"] = torch.stack(_drive_model(ragged.push_ragged, x, ticks, {"video": 1, "vggish": 2}))
    assert ragged.frames_seen == [l] * b
    # B = 2: the first two clips of the fixture as two streams offset against each other (a stream's logits do not depend on
    # its neighbours, so the fixture's rows of those clips are their reference)
    pair_ticks = _schedule(l, 2, 3, seed=3, late=(1, 2))
    assert pair_ticks[0][1] == 0 and pair_ticks[1][1] == 0 and pair_ticks[2] == [2, 3]
    pair = streaming.CANStream(model, 2, max_new=3)
    got["ragged_B2"] = torch.stack(_drive_model(pair.push_ragged, {m: v[:2] for m, v in x.items()}, pair_ticks,
                                                {"video": 1, "vggish": 2}))
    assert pair.frames_seen == [l, l]
    assert list(x) == keys and {m: tuple(v.shape) for m, v in x.items()} == shapes      # the caller's dict is left alone
    return model, ticks, got


def test_can_stream_matches_the_reference_fixture_however_it_is_pushed():
    """B = 3, L = 8, 40 x 40 frames through the IR-50: frame by frame, in one push, via ``stream_forward`` and ragged (three
    streams, and the first two clips as B = 2 streams offset against each other) against the logits recorded from the
    reference's CAN, at the offline model's bar."""
    _, _, want, (b, l) = _can_fixture()
    _, _, got = _can_runs()
    for how, logits in got.items():
        ref = want[:logits.shape[0]]
        assert tuple(logits.shape) == ref.shape, how
        err = np.abs(logits.cpu().numpy() - ref).max()
        print(f"CAN stream ({how}) against the reference fixture: {err:.3e} (bar {CAN_TOL:.0e})")
        assert err < CAN_TOL, (how, err)


def test_can_stream_returns_the_same_bits_however_the_frames_are_pushed():
    """The four ways of pushing frames are ``torch.equal`` to one another, through the IR-50 too: the streams hand the encoders
    their frames in calls of a fixed size (``encoder_batch``), so a frame's embedding does not depend on how many frames its
    push brought.  (One encoder call per push would not do: the bf16x3 convs pick their tile variant from the row count, and
    at 40 x 40 a call of 12 or more frames differs from a call of fewer by up to 3.6e-06 on the embedding, 1.5e-08 on the
    logits.)"""
    _, _, got = _can_runs()
    for how, logits in got.items():
        base = got["frame_by_frame"][:logits.shape[0]]
        print(f"CAN stream ({how}) against frame by frame: {(logits - base).abs().max().item():.3e}")
    for how, logits in got.items():
        assert torch.equal(logits, got["frame_by_frame"][:logits.shape[0]]), how


def test_can_stream_on_embeddings_returns_the_same_bits_however_they_are_pushed_and_regression_is_tanh():
    """The encoders skipped (the IR-50 run once on all frames): one push, frame by frame, chunks of 3 and ragged, bit for
    bit; through the frames at fewer than 12 per push, the same bits again; REGRESSION is tanh of the logits."""
    _, streaming = _pkg()
    sd, x, want, (b, l) = _can_fixture()
    model, ticks, runs = _can_runs()
    with torch.no_grad():
        emb = model.spatial["visual"](x["video"].reshape(-1, *x["video"].shape[2:]), None).view(b, l, -1)
    feats = {"video": emb, "vggish": x["vggish"][:, 0].contiguous()}
    cut = (lambda t0, c: {m: v[:, t0:t0 + c].contiguous() for m, v in feats.items()})
    one = streaming.CANStream(model, b).push_features(feats)
    assert np.abs(one.cpu().numpy() - want).max() < CAN_TOL
    for step in (1, 3):
        stream = streaming.CANStream(model, b)
        assert torch.equal(torch.cat([stream.push_features(cut(t, min(step, l - t))) for t in range(0, l, step)], dim=1), one)
    by_rows = streaming.CANStream(model, b, max_new=3)
    fed, outs = [0] * b, [[] for _ in range(b)]
    for counts in ticks:
        packed = {m: torch.cat([v[i, fed[i]:fed[i] + c] for i, c in enumerate(counts)]) for m, v in feats.items()}
        _unpack(by_rows.push_features_ragged(packed, counts), counts, outs)
        fed = [f + c for f, c in zip(fed, counts)]
    assert by_rows.frames_seen == [l] * b
    assert torch.equal(torch.stack([torch.cat(o) for o in outs]), one)
    assert torch.equal(streaming.CANStream(model, b).push(x), runs["one_push"])          # the same call, the same bits
    whole = streaming.CANStream(model, b, encoder_batch=None).push(x)                    # one encoder call for the 24 frames
    assert np.abs(whole.cpu().numpy() - want).max() < CAN_TOL
    assert torch.equal(streaming.stream_forward(model, x, chunk=l, encoder_batch=None), whole)
    reg_model = _can(sd, task="REGRESSION")
    reg = streaming.CANStream(reg_model, b).push(x)
    assert torch.equal(reg.cpu(), torch.tanh(runs["one_push"].cpu().double()).float())   # ops.tanh_fwd: double tanh, rounded once
    reg_rows = streaming.CANStream(reg_model, b, max_new=3)
    got = _drive_model(reg_rows.push_ragged, x, ticks, {"video": 1, "vggish": 2})
    assert torch.equal(torch.stack(got).cpu(), torch.tanh(runs["ragged"].cpu().double()).float())


# ---------------------------------------------------------------------------------------------- 8. errors
def test_bad_counts_are_refused_before_any_launch():
    ops, streaming = _pkg()
    sd, x, _ = _bimodal()
    model = _lfan(BIMODAL, sd)
    stream = streaming.LFANStream(model, 2)
    tcn = stream.tcn["bert"]
    rows = (lambda n: {m: x[m][0, 0, :n].contiguous() for m in BIMODAL})
    ops.STREAM_TRACE = trace = []
    try:
        for push in (stream.push_ragged, stream.push_features_ragged):
            with pytest.raises(ValueError, match="one count per stream"):
                push(rows(2), [2])
            with pytest.raises(ValueError, match="one count per stream"):
                push(rows(2), [1, 1, 0])
            with pytest.raises(ValueError, match="outside 0"):
                push(rows(2), [3, -1])
            with pytest.raises(ValueError, match="max_new"):
                push(rows(33), [33, 0])
            with pytest.raises(ValueError, match="sum to 4"):
                push(rows(3), [2, 2])
            with pytest.raises(ValueError, match="sum to 2"):                      # the second modality is the bad one
                push({"vggish": rows(2)["vggish"], "bert": rows(3)["bert"]}, [2, 0])
            with pytest.raises(ValueError, match="GPU"):
                push({"vggish": rows(2)["vggish"], "bert": rows(2)["bert"].cpu()}, [2, 0])
            with pytest.raises(KeyError):
                push({"vggish": rows(2)["vggish"]}, [2, 0])
        with pytest.raises(ValueError, match="one count per stream"):
            tcn.push_ragged(rows(2)["bert"], [2])
        with pytest.raises(ValueError, match="outside 0"):
            tcn.push_ragged(rows(2)["bert"], [-1, 3])
        with pytest.raises(ValueError, match="max_new"):
            tcn.push_ragged(rows(33)["bert"], [0, 33])
        with pytest.raises(ValueError, match="sum to 3"):
            tcn.push_ragged(rows(2)["bert"], [2, 1])
        with pytest.raises(ValueError, match=r"\[M, 768\]"):
            tcn.push_ragged(rows(2)["vggish"], [2, 0])
        assert trace == [] and stream.frames_seen == [0, 0] and tcn.frames_seen == [0, 0] and tcn._pos == [0, 0]
        nothing = stream.push_ragged(rows(0), [0, 0])
        assert tuple(nothing.shape) == (0, 7) and trace == [] and stream.frames_seen == [0, 0]
        out = stream.push_ragged(rows(2), [2, 0])
        names = [name for name, _ in trace]
        assert names.count("conv_rows") == 2 * 2 * 4 and names.count("append_rows") == 2 and set(names) == {"conv_rows", "append_rows"}
        assert tuple(out.shape) == (2, 7) and stream.frames_seen == [2, 0]
    finally:
        ops.STREAM_TRACE = None
