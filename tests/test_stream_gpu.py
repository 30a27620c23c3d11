"""Streaming TCN / LFAN on the GPU: frame-at-a-time evaluation over device-side rings returns what the whole-sequence forward
returns -- bit for bit where that can be asked (exact data; one stream against itself under another chunking, ring size, ring
position or set of neighbours), and within the offline forward's own tolerance against the float64 oracles."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import stream_ref  # noqa: E402
from helpers import MODS, golden  # noqa: E402
from stream_ref import BLOCK_CASES, SLOPE  # noqa: E402

TOL = 2e-5          # tests/test_tail_gpu.py:11, the bar test_tcn_forward_backward_vs_oracle holds the offline TCN forward to
LFAN_TOL = 1e-4     # tests/test_tail_gpu.py:279, the offline LFAN forward against the reference fixture


def _pkg():
    from feature_vs_text_compound_emotion_amd import ops, streaming
    return ops, streaming


# ---------------------------------------------------------------------------------------------- 1. one block, exact
@functools.lru_cache(maxsize=None)
def _block_operands(case):
    d = stream_ref.make_block(case)
    ref = stream_ref.block_ref(d["x"], d["w1"], d["b1"], d["w2"], d["b2"], d["dsw"], d["dsb"], case.k, case.dil)
    return d, ref


class _Arena:
    """Rings carved out of one NaN-filled allocation with NaN guards between them."""
    GUARD = 64

    def __init__(self, shapes, misalign):
        self.spans, off = [], self.GUARD
        for shape in shapes:
            off = (off + 3) // 4 * 4 + misalign          # 16-byte aligned plus the case's shift
            n = int(np.prod(shape))
            self.spans.append((off, n, shape))
            off += n + self.GUARD
        self.flat = torch.full((off,), float("nan"), device="cuda")
        self.rings = [self.view(self.flat, i) for i in range(len(shapes))]
        for r in self.rings:
            r.zero_()

    def view(self, flat, i):
        off, n, shape = self.spans[i]
        return flat[off:off + n].view(shape)

    def guards_are_nan(self):
        keep = torch.ones_like(self.flat, dtype=torch.bool)
        for off, n, _ in self.spans:
            keep[off:off + n] = False
        return bool(torch.isnan(self.flat[keep]).all())


# every case through both entry families; the lockstep ids stay the bare case names
@pytest.mark.parametrize("case,via", [pytest.param(c, via, id=c.name if via == "lockstep" else f"{c.name}-{via}")
                                      for via in ("lockstep", "rows") for c in BLOCK_CASES])
def test_block_streamed_equals_the_float64_whole_sequence_block_bit_for_bit(case, via):
    """Exact data (stream_ref; precondition asserted in test_stream_cpu.py): any reduction order is exact, so no tolerance.
    T >= 3 R frames, so every ring wraps at least twice.  The rings are slices of a NaN-filled allocation: the guards stay NaN,
    and a push changes nothing but its c new slots.  ``via``: the lockstep entry points, or the row-table ones with the table
    of the same dense push (every stream at ``pos`` brings c frames)."""
    ops, streaming = _pkg()
    d, ref = _block_operands(case)
    s, total = case.s, d["x"].shape[1]
    r = streaming.ring_frames(case.k, case.dil, case.max_new)
    assert r == stream_ref.ring_frames(case.k, case.dil, case.max_new)
    arena = _Arena([(s, r, case.cin), (s, r, case.cout), (s, 2 * r, case.cout)], case.misalign)
    xring, hring, oring = arena.rings
    assert xring.data_ptr() % 16 == 4 * case.misalign
    dev = {n: (None if v is None else v.cuda()) for n, v in d.items()}
    pack = {"k": case.k, "dil": case.dil, "w1": ops.pack_tcn_stream_weight(dev["w1"]), "b1": dev["b1"],
            "w2": ops.pack_tcn_stream_weight(dev["w2"]), "b2": dev["b2"],
            "dsw": ops.pack_tcn_stream_weight(dev["dsw"]) if case.ds else None, "dsb": dev["dsb"]}
    stray = torch.zeros((), dtype=torch.bool, device="cuda")      # a slot other than the new ones changed
    mirrored = torch.ones((), dtype=torch.bool, device="cuda")    # the ring output equals the dense output
    outs, pos = [], 0
    for c in stream_ref.chunks_of(case, total):
        before = arena.flat.clone()
        allowed = torch.zeros_like(arena.flat, dtype=torch.bool)
        for i, ring_len in enumerate((r, r, 2 * r)):
            slots = [(pos + j) & (ring_len - 1) for j in range(c)]
            arena.view(allowed, i)[:, slots] = True
        dense = torch.empty(s * c, case.cout, device="cuda")
        new = dev["x"][:, pos:pos + c].contiguous()
        if via == "lockstep":
            ops.tcn_stream_append(new, xring, pos & (r - 1))
            streaming.block_push(pack, xring, hring, pos, c, out_ring=oring, out_pos=pos, out_dense=dense, slope=SLOPE)
        else:
            row_stream, row_pos = ops.stream_row_table([pos] * s, [c] * s, "cuda")
            ops.tcn_stream_append_rows(new.view(s * c, case.cin), xring, row_stream, row_pos, c)
            streaming.block_push_rows(pack, xring, hring, row_stream, row_pos, max_count=c, out_ring=oring, out_dense=dense,
                                      slope=SLOPE)
        same = (arena.flat == before) | (torch.isnan(arena.flat) & torch.isnan(before))
        stray |= (~same & ~allowed).any()
        mirrored &= torch.equal(oring[:, [(pos + j) & (2 * r - 1) for j in range(c)]], dense.view(s, c, -1))
        outs.append(dense.view(s, c, -1))
        pos += c
    got = torch.cat(outs, dim=1).cpu()
    assert not stray.item()
    assert mirrored.item()
    assert arena.guards_are_nan()
    assert torch.equal(got.double(), ref["out"])
    # the first conv's ring holds the last R activations of the sequence, each at its slot
    tail = torch.arange(total - r, total)
    assert torch.equal(hring[:, (tail & (r - 1)).cuda()].cpu().double(), ref["h"][:, tail])


# ---------------------------------------------------------------------------------------------- 2. the invariant, bitwise
def _tcn(cin, channels, k=5, seed=21):
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.temporal_convnet import TemporalConvNet
    spec, alias = synth.tcn_spec("", cin, channels, k)
    sd = synth.make_state_dict(spec, alias, seed)
    net = TemporalConvNet(cin, channels, kernel_size=k, dropout=0.1)
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval(), sd


def _push_all(stream, x, chunks):
    """x [S, T, C] pushed in ``chunks`` (cycled until T is used up): [S, T, Cout]."""
    outs, pos, i = [], 0, 0
    while pos < x.shape[1]:
        c = min(chunks[i % len(chunks)], x.shape[1] - pos)
        outs.append(stream.push_rows(x[:, pos:pos + c]))
        pos, i = pos + c, i + 1
    return torch.cat(outs, dim=1)


def test_an_output_depends_on_its_own_streams_history_only():
    """randn data, 40 -> [32, 32, 16, 16], k = 5, 200 frames (the 64-frame ring of the last level wraps three times): the
    same bits one frame at a time, in mixed chunks, with max_new = 3 against max_new = 32, and for one stream of a batch of
    five against that stream alone."""
    _, streaming = _pkg()
    net, _ = _tcn(40, [32, 32, 16, 16])
    s, total = 5, 200
    x = torch.randn(s, total, 40, generator=torch.Generator().manual_seed(31)).cuda()
    one = _push_all(streaming.TCNStream(net, s, max_new=32), x, [1])
    assert torch.isfinite(one).all() and one.abs().max().item() > 0
    mixed = _push_all(streaming.TCNStream(net, s, max_new=32), x, [1, 3, 2, 32, 1, 7])
    assert torch.equal(mixed, one)
    small = streaming.TCNStream(net, s, max_new=3)
    large = streaming.TCNStream(net, s, max_new=32)
    assert small.ring_frames == [8, 16, 32, 64] and large.ring_frames == [64, 64, 64, 64]
    assert torch.equal(small.push_rows(x), one) and torch.equal(large.push_rows(x), one)
    assert small.frames_seen == [total] * s
    for pick in (0, 3):
        alone = _push_all(streaming.TCNStream(net, 1, max_new=32), x[pick:pick + 1].contiguous(), [2, 5])
        assert torch.equal(alone[0], one[pick])


# ---------------------------------------------------------------------------------------------- 3. TCN against the oracle
def _tcn_geometries():
    from test_tail_gpu import _TCN_GEOMETRIES
    return _TCN_GEOMETRIES


@pytest.mark.parametrize("geometry", ["", "-gather40-L5"])
def test_streamed_tcn_vs_oracle_on_150_frames(geometry):
    from oracle.tcn import tcn_forward
    _, streaming = _pkg()
    cin, channels, s, _ = _tcn_geometries()[geometry]
    net, sd = _tcn(cin, channels)
    total = 150
    x = torch.randn(s, cin, total, generator=torch.Generator().manual_seed(22))
    ref = tcn_forward(x.double(), {k: v.double() for k, v in sd.items()}, "")
    got = _push_all(streaming.TCNStream(net, s, max_new=32), x.transpose(1, 2).contiguous().cuda(), [1, 3, 2, 32, 1])
    err = (got.cpu().double().transpose(1, 2) - ref).abs().max().item()
    print(f"streamed TCN{geometry}: worst error against the float64 oracle {err:.3e} (bar {TOL:.0e})")
    assert err < TOL, err


def test_the_geometries_above_are_those_of_the_offline_test():
    assert sorted(_tcn_geometries()) == ["", "-gather40-L5"]


# ---------------------------------------------------------------------------------------------- 4. LFAN, reference fixture
def _lfan(mods, sd, n_cls=7, head_hw=5, task="CLASSIFICATION", example_length=3):
    """``example_length`` is deliberately not the length of anything that is pushed."""
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.lfan import LFAN
    m = LFAN(backbone_settings={}, output_dim=n_cls, task=task, modality=mods, example_length=example_length, kernel_size=5,
             tcn_channel=synth.TCN_CHANNELS, modal_dim=32, num_heads=2, root_dir="", device="cuda", head_hw=head_hw)
    m.init(load_backbone=False)
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


_TIME = {"video": 1}


def _frames(x, t0, c):
    return {m: v.narrow(_TIME.get(m, 2), t0, c) for m, v in x.items()}


@functools.lru_cache(maxsize=None)
def _fixture():
    from feature_vs_text_compound_emotion_amd import synth
    g = golden("lfan_trimodal_eval.npz")
    b, l, hw, ncls, wseed, dseed = [int(v) for v in g["meta"]]
    sd = synth.lfan_state_dict(MODS, n_cls=ncls, head_hw=hw // 8, seed=wseed)
    x, _ = synth.make_clip_batch(MODS, b, l, hw=hw, seed=dseed)
    return _lfan(MODS, sd, n_cls=ncls, head_hw=hw // 8), {k: v.cuda() for k, v in x.items()}, g["logits"], (b, l)


@pytest.mark.parametrize("how", ["frame_by_frame", "one_push", "stream_forward"])
def test_lfan_stream_matches_reference_fixture(how):
    """B = 2, L = 8, 40 x 40 frames through the encoders: most taps fall before the start of the stream."""
    _, streaming = _pkg()
    model, x, want, (b, l) = _fixture()
    keys, shapes = list(x), {m: tuple(v.shape) for m, v in x.items()}
    if how == "stream_forward":
        got = streaming.stream_forward(model, x, chunk=3)
    else:
        stream = streaming.LFANStream(model, b)
        step = 1 if how == "frame_by_frame" else l
        got = torch.cat([stream.push(_frames(x, t, step)) for t in range(0, l, step)], dim=1)
        assert stream.frames_seen == [l] * b
    assert list(x) == keys and {m: tuple(v.shape) for m, v in x.items()} == shapes      # the caller's dict is left alone
    assert tuple(got.shape) == want.shape
    err = np.abs(got.cpu().numpy() - want).max()
    print(f"LFAN stream ({how}) against the reference fixture: {err:.3e} (bar {LFAN_TOL:.0e})")
    assert err < LFAN_TOL, err


# ---------------------------------------------------------------------------------------------- 5. LFAN, a long history
BIMODAL = ["vggish", "bert"]


@functools.lru_cache(maxsize=None)
def _bimodal(seed=9, n_cls=7, s=2, total=150):
    from feature_vs_text_compound_emotion_amd import synth
    from oracle.lfan import lfan_forward
    sd = synth.lfan_state_dict(BIMODAL, n_cls=n_cls, seed=seed)
    x, _ = synth.make_clip_batch(BIMODAL, s, total, seed=seed + 1)
    with torch.no_grad():
        ref = lfan_forward({m: v.double() for m, v in x.items()}, {k: v.double() if v.is_floating_point() else v
                                                                     for k, v in sd.items()}, BIMODAL)
    return sd, {m: v.cuda() for m, v in x.items()}, ref


def _push_lfan(stream, x, chunks):
    total = next(iter(x.values())).shape[2]
    outs, pos, i = [], 0, 0
    while pos < total:
        c = min(chunks[i % len(chunks)], total - pos)
        outs.append(stream.push(_frames(x, pos, c)))
        pos, i = pos + c, i + 1
    return torch.cat(outs, dim=1)


def test_lfan_stream_with_a_long_history_vs_oracle_and_regression_is_tanh_of_the_logits():
    _, streaming = _pkg()
    sd, x, ref = _bimodal()
    chunks = [1, 3, 2, 32, 1]
    logits = _push_lfan(streaming.LFANStream(_lfan(BIMODAL, sd), 2), x, chunks)
    err = (logits.cpu().double() - ref).abs().max().item()
    print(f"LFAN stream, 150 frames, against the float64 oracle: {err:.3e} (bar {LFAN_TOL:.0e})")
    assert err < LFAN_TOL, err
    reg = _push_lfan(streaming.LFANStream(_lfan(BIMODAL, sd, task="REGRESSION"), 2), x, chunks)
    assert torch.equal(reg.cpu(), torch.tanh(logits.cpu().double()).float())      # ops.tanh_fwd: double tanh, rounded once
    whole = streaming.stream_forward(_lfan(BIMODAL, sd), x, chunk=32)
    assert (whole.cpu().double() - ref).abs().max().item() < LFAN_TOL
    feats = {m: x[m][:, 0].contiguous() for m in BIMODAL}                          # [S, T, embedding_dim]
    by_features = streaming.LFANStream(_lfan(BIMODAL, sd), 2, max_new=32).push_features(feats)
    assert (by_features.cpu().double() - ref).abs().max().item() < LFAN_TOL


# ---------------------------------------------------------------------------------------------- 6. reset
def test_reset_of_one_stream_leaves_the_other_alone():
    _, streaming = _pkg()
    net, _ = _tcn(40, [32, 32, 16, 16])
    total, t0 = 120, 37
    x = torch.randn(2, total, 40, generator=torch.Generator().manual_seed(41)).cuda()
    undisturbed = _push_all(streaming.TCNStream(net, 2, max_new=4), x, [4, 1, 3])
    stream = streaming.TCNStream(net, 2, max_new=4)
    head = _push_all(stream, x[:, :t0].contiguous(), [4, 1, 3])
    stream.reset([1])
    assert stream.frames_seen == [t0, 0]
    tail = _push_all(stream, x[:, t0:].contiguous(), [2, 4])
    fresh = _push_all(streaming.TCNStream(net, 2, max_new=4), x[:, t0:].contiguous(), [3])
    assert torch.equal(torch.cat([head, tail], dim=1)[0], undisturbed[0])
    assert torch.equal(tail[1], fresh[1])
    assert not torch.equal(tail[1], undisturbed[1, t0:])            # the history did matter
    stream.reset()
    assert stream.frames_seen == [0, 0] and all(not r.any() for r in stream.xrings + stream.hrings)

    sd, xl, _ = _bimodal()
    model = _lfan(BIMODAL, sd)
    lf = streaming.LFANStream(model, 2, max_new=8)
    before = _push_lfan(lf, _frames(xl, 0, t0), [8, 1])
    lf.reset([1])
    after = _push_lfan(lf, _frames(xl, t0, 60), [5])
    calm = _push_lfan(streaming.LFANStream(model, 2, max_new=8), _frames(xl, 0, t0 + 60), [8, 1])
    new = _push_lfan(streaming.LFANStream(model, 2, max_new=8), _frames(xl, t0, 60), [5])
    assert torch.equal(torch.cat([before, after], dim=1)[0], calm[0]) and torch.equal(after[1], new[1])


# ---------------------------------------------------------------------------------------------- 7. stale weights
def test_a_later_load_state_dict_is_honoured():
    from feature_vs_text_compound_emotion_amd import synth
    _, streaming = _pkg()
    sd, x, _ = _bimodal()
    model = _lfan(BIMODAL, sd)
    stream = streaming.LFANStream(model, 2)
    first = stream.push(_frames(x, 0, 5))
    packs = stream.tcn["bert"]._packs
    assert stream.tcn["bert"]._pack() is packs                       # cached while the parameters stand
    model.load_state_dict(synth.lfan_state_dict(BIMODAL, n_cls=7, seed=77), strict=True)
    stream.reset()
    again = stream.push(_frames(x, 0, 5))
    assert stream.tcn["bert"]._packs is not packs
    assert torch.equal(again, streaming.LFANStream(model, 2).push(_frames(x, 0, 5)))
    assert not torch.equal(again, first)


# ---------------------------------------------------------------------------------------------- 8. errors
def test_errors_are_raised_before_any_launch():
    ops, streaming = _pkg()
    sd, x, _ = _bimodal()
    model = _lfan(BIMODAL, sd)
    stream = streaming.LFANStream(model, 2)
    ok = _frames(x, 0, 2)
    ops.STREAM_TRACE = trace = []
    try:
        model.train()
        with pytest.raises(RuntimeError, match="train mode"):
            stream.push(ok)
        with pytest.raises(RuntimeError, match="train mode"):
            streaming.LFANStream(model, 2)
        model.eval()
        with pytest.raises(ValueError, match="2 streams"):          # three streams' worth of frames
            stream.push({m: torch.cat([v, v[:1]]) for m, v in ok.items()})
        with pytest.raises(ValueError, match="GPU"):                # the second modality is the bad one
            stream.push({"vggish": ok["vggish"], "bert": ok["bert"].cpu()})
        with pytest.raises(ValueError, match="different numbers"):
            stream.push({"vggish": ok["vggish"], "bert": _frames(x, 0, 3)["bert"]})
        with pytest.raises(ValueError, match="GPU"):
            stream.push_features({m: v[:, 0].cpu() for m, v in ok.items()})
        with pytest.raises(KeyError):
            stream.push({"vggish": ok["vggish"]})
        with pytest.raises(TypeError):
            streaming.LFANStream(model.temporal["bert"], 2)
        assert trace == [] and stream.frames_seen == [0, 0]
        stream.push(ok)
        assert [name for name, _ in trace].count("conv") == 2 * 2 * 4 and stream.frames_seen == [2, 2]
    finally:
        ops.STREAM_TRACE = None
