"""Per-frame face boxes on full camera frames, on the GPU (csrc/frames_box.hip).  Frame f with box b must give exactly the bytes,
and the floats, that today's ``FrameTransform`` gives the contiguous zero-padded slice of that frame (``pad_slice``): the two
passes are the same integer sums over the coefficient rows of the box's own width and height, so every comparison is
``torch.equal``."""
import functools
import random

import numpy as np
import pytest
import torch

from frames_box_ref import GOLDEN_BOXES, pad_slice
from helpers import golden

pytestmark = pytest.mark.gpu

OUTSIDE = (200, 200, 230, 215)      # no pixel of it lies in any frame used here


def _mod():
    from feature_vs_text_compound_emotion_amd import frames, ops
    return frames, ops


@functools.lru_cache(maxsize=None)
def _clip(n, h, w, seed=0):
    """n random frames [n, h, w, 3] whose first byte sits at an odd address."""
    g = torch.Generator().manual_seed(1000 * h + w + seed)
    buf = torch.empty(n * h * w * 3 + 1, dtype=torch.uint8, device="cuda")
    view = buf[1:].view(n, h, w, 3)
    view.copy_(torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8))
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    return view


def _sliced(xf, frames, boxes, entry):
    """Today's path on the zero-padded slice of every frame: (float [n, 3, crop, crop], u8 [n, crop, crop, 3])."""
    outs = [xf(pad_slice(f, b)[None, None], crop_xyf=[entry], return_u8=True) for f, b in zip(frames, boxes)]
    return torch.cat([o[0][0] for o in outs]), torch.cat([o[1][0] for o in outs])


def _random_boxes(n, h, w, max_side, seed):
    """Boxes of every size up to max_side that stick out of an h x w frame on any side."""
    rng, out = random.Random(seed), []
    for _ in range(n):
        bw, bh = rng.randint(1, max_side), rng.randint(1, max_side)
        x0, y0 = rng.randint(-bw // 2, w - 1), rng.randint(-bh // 2, h - 1)
        out.append((x0, y0, x0 + bw, y0 + bh))
    return out


# ---------------------------------------------------------------------------------------------- 1. offline
def test_offline_boxes_equal_the_pil_fixture():
    frames, _ = _mod()
    g = golden("frames_boxes.npz")
    frame = torch.from_numpy(g["frame"]).cuda()
    clip = frame[None].expand(len(GOLDEN_BOXES), -1, -1, -1).contiguous()
    xf = frames.FrameTransform(48, 40, train=False)                       # max_side = 1024, the default store
    out, u8 = xf(clip, boxes=np.array(GOLDEN_BOXES), return_u8=True)
    want = torch.from_numpy(g["resized"][:, 4:44, 4:44]).cuda()
    assert u8.shape == (1, 8, 40, 40, 3) and torch.equal(u8[0], want)
    # the float stage is three IEEE operations on the byte (numpy: a GPU division by a constant may multiply by its inverse)
    center = g["resized"][:, 4:44, 4:44].astype(np.float32)
    ref = torch.from_numpy(((center / np.float32(255.0) - np.float32(0.5)) / np.float32(0.5)).transpose(0, 3, 1, 2)).cuda()
    assert torch.equal(out[0], ref)
    out3, u83 = xf(clip.view(2, 4, 90, 120, 3), boxes=np.array(GOLDEN_BOXES).reshape(2, 4, 4), return_u8=True)   # [B, L, 4]
    assert torch.equal(u83.view(8, 40, 40, 3), want) and torch.equal(out3.view(8, 3, 40, 40), ref)


@pytest.mark.parametrize("size,crop", [(48, 40), (8, 6), (112, 100)])
@pytest.mark.parametrize("h,w", [(90, 120), (37, 53)])
def test_offline_boxes_equal_todays_path_on_the_padded_slice(h, w, size, crop):
    frames, _ = _mod()
    boxes = GOLDEN_BOXES + [OUTSIDE]
    clip = _clip(len(boxes), h, w)
    xf = frames.FrameTransform(size, crop, train=False, max_side=160)
    for entry in (xf.draw(1)[0].tolist(), [size - crop, 1, 1], [0, size - crop, 1]):      # centre; two corners, flipped
        out, u8 = xf(clip, crop_xyf=[entry], boxes=boxes, return_u8=True)
        ref, ref_u8 = _sliced(xf, clip, boxes, entry)
        assert torch.equal(u8[0], ref_u8) and torch.equal(out[0], ref), (entry,)
        assert not u8[0, -1].any()                                                        # the box outside the frame
        assert torch.equal(xf(clip, crop_xyf=[entry], boxes=boxes)[0], ref)                # without the uint8 output


def test_many_taps_at_size_8():
    """Sides up to 150 at size 8: 2 * ceil(150 / 8) + 1 = 39 taps, beyond the 13-tap fast path and the 16-tap LDS tiles of the
    fixed-geometry kernel."""
    frames, _ = _mod()
    h, w = 150, 160
    boxes = [(0, 0, 150, 150), (10, 0, 160, 149), (-30, -20, 120, 130), (3, 0, 4, 150), (100, 90, 250, 240), (0, 0, 129, 121)]
    assert frames.box_tables(8, 150).max_ks == 39
    clip = _clip(len(boxes), h, w)
    xf = frames.FrameTransform(8, 6, train=False, max_side=150)
    for entry in ([1, 1, 0], [2, 0, 1]):
        out, u8 = xf(clip, crop_xyf=[entry], boxes=boxes, return_u8=True)
        ref, ref_u8 = _sliced(xf, clip, boxes, entry)
        assert torch.equal(u8[0], ref_u8) and torch.equal(out[0], ref)


@pytest.mark.parametrize("h,w", [(256, 256), (100, 77), (40, 52)])
def test_a_box_equal_to_the_frame_gives_the_unboxed_bits(h, w):
    frames, _ = _mod()
    clip = _clip(3, h, w)
    xf = frames.FrameTransform(48, 40, train=False)
    for entry in ([4, 4, 0], [8, 0, 1]):
        ref, ref_u8 = xf(clip, crop_xyf=[entry], return_u8=True)
        out, u8 = xf(clip, crop_xyf=[entry], boxes=[(0, 0, w, h)] * 3, return_u8=True)
        assert torch.equal(out, ref) and torch.equal(u8, ref_u8)


def test_max_side_runs_and_one_more_is_refused():
    frames, _ = _mod()
    clip = _clip(2, 90, 120)
    xf = frames.FrameTransform(48, 40, train=False, max_side=70)
    boxes = [(20, 10, 90, 80), (-5, 30, 65, 31)]
    out, u8 = xf(clip, boxes=boxes, return_u8=True)
    ref, ref_u8 = _sliced(xf, clip, boxes, [4, 4, 0])
    assert torch.equal(out[0], ref) and torch.equal(u8[0], ref_u8)
    fs = frames.FrameStream(1, hold=4, max_new=2, max_side=70)
    fs.push(clip, [2], boxes)
    assert torch.equal(fs.take([(0, 0), (0, 1)]), ref)
    for bad in ([(20, 10, 91, 80), boxes[1]], [boxes[0], (0, 0, 5, 71)]):
        with pytest.raises(ValueError, match="max_side = 70"):
            xf(clip, boxes=bad)
        with pytest.raises(ValueError, match="max_side = 70"):
            fs.push(clip, [2], bad)
    with pytest.raises(ValueError, match="GPU tensor"):
        fs.push(clip, [2], torch.tensor(boxes, device="cuda"))
    assert fs.frames_seen == [2] and fs.frames_taken == [2]


# ---------------------------------------------------------------------------------------------- 2. streamed
N, H, W, SIDE = 12, 90, 120, 160


@functools.lru_cache(maxsize=None)
def _stream_case(seed):
    """(frames [N, H, W, 3], boxes, offline boxed floats [N, 3, 40, 40])."""
    frames, _ = _mod()
    clip, boxes = _clip(N, H, W, seed), _random_boxes(N, H, W, SIDE, seed)
    return clip, boxes, frames.FrameTransform(48, 40, train=False, max_side=SIDE)(clip, boxes=boxes)[0]


def _chunks(n, how, seed=0):
    rng, out = random.Random(seed), []
    while sum(out) < n:
        out.append(min(n - sum(out), {"ones": 1, "threes": 3}.get(how) or rng.randint(1, 5)))
    return out


@pytest.mark.parametrize("how", ["ones", "threes", "random"])
def test_one_stream_in_chunks_equals_the_offline_boxed_call(how):
    frames, _ = _mod()
    clip, boxes, ref = _stream_case(1)
    fs = frames.FrameStream(1, hold=16, max_new=5, max_side=SIDE)
    at = 0
    for c in _chunks(N, how, seed=3):
        fs.push(clip[at:at + c], [c], boxes[at:at + c])
        at += c
    assert fs.frames_seen == [N]
    assert torch.equal(fs.take([(0, i) for i in range(N)]), ref)


def test_ragged_streams_equal_each_stream_alone():
    """Three streams, 0 .. 3 frames each per push, stream 2 joins at the fourth push."""
    frames, _ = _mod()
    cases = [_stream_case(s) for s in (1, 2, 3)]
    rng, at, ticks = random.Random(7), [0, 0, 0], []
    while min(at) < N:
        c = [min(N - at[s], rng.randint(0, 3)) if s < 2 or len(ticks) >= 3 else 0 for s in range(3)]
        ticks.append((list(at), c))
        at = [a + k for a, k in zip(at, c)]
    assert any(0 in c and max(c) > 0 for _, c in ticks)
    fs = frames.FrameStream(3, hold=16, max_new=3, max_side=SIDE)
    alone = [frames.FrameStream(1, hold=16, max_new=3, max_side=SIDE) for _ in range(3)]
    for start, c in ticks:
        if not sum(c):
            continue
        fs.push(torch.cat([cases[s][0][start[s]:start[s] + c[s]] for s in range(3)]), c,
                [b for s in range(3) for b in cases[s][1][start[s]:start[s] + c[s]]])
        for s in range(3):
            if c[s]:
                alone[s].push(cases[s][0][start[s]:start[s] + c[s]], [c[s]], cases[s][1][start[s]:start[s] + c[s]])
    got = fs.take([(s, i) for s in range(3) for i in range(N)]).view(3, N, 3, 40, 40)
    for s in range(3):
        assert torch.equal(got[s], alone[s].take([(0, i) for i in range(N)])) and torch.equal(got[s], cases[s][2])


def test_boxed_and_unboxed_pushes_alternate_within_a_stream():
    frames, _ = _mod()
    clip, boxes, ref = _stream_case(1)
    plain = frames.FrameTransform(48, 40, train=False)(clip)[0]
    fs = frames.FrameStream(1, hold=16, max_new=3, max_side=SIDE)
    for i in range(0, N, 3):
        fs.push(clip[i:i + 3], [3], boxes[i:i + 3] if (i // 3) % 2 == 0 else None)
    got = fs.take([(0, i) for i in range(N)])
    for i in range(0, N, 3):
        assert torch.equal(got[i:i + 3], (ref if (i // 3) % 2 == 0 else plain)[i:i + 3]), i


def test_reset_in_mid_schedule_equals_a_fresh_stream_and_positions_wrap():
    frames, _ = _mod()
    clip, boxes, ref = _stream_case(2)
    other = _stream_case(3)
    fs = frames.FrameStream(2, hold=16, max_new=4, max_side=SIDE)
    fs._base = [(1 << 30) - 5, 0]                   # host positions pass 2^30 during the schedule
    fs.push(torch.cat([clip[:4], other[0][:3]]), [4, 3], boxes[:4] + other[1][:3])
    fs.reset([1])
    fs.push(torch.cat([clip[4:8], clip[:4]]), [4, 4], boxes[4:8] + boxes[:4])      # stream 1 starts over, with other frames
    fs.push(torch.cat([clip[8:], clip[4:8]]), [4, 4], boxes[8:] + boxes[4:8])
    assert fs._base[0] + fs.frames_seen[0] > 1 << 30 and fs.frames_seen == [12, 8]
    assert torch.equal(fs.take([(0, i) for i in range(N)]), ref)
    assert torch.equal(fs.take([(1, i) for i in range(8)]), ref[:8])


# ---------------------------------------------------------------------------------------------- 3. tables are clamped
def test_tables_nobody_vetted_stay_inside_the_frames_and_the_ring():
    """Boxes handed straight to ``ops``: coordinates of +-2^30, zero and negative widths and heights.  The packed frames sit
    between guard frames of 255 (a box pixel outside the frame must read 0, not a neighbour) and the ring between sentinel
    slabs.  The kernel clamps a coordinate into +-2^20 and a side into 1 .. max_side and range-checks every pixel, so the
    wild rows have a defined meaning, the sane rows of the same launch keep their bits, and nothing is written or read
    outside."""
    frames, ops = _mod()
    S, rf, size, crop, h, w, n, side = 2, 8, 48, 40, 40, 52, 3, 64
    slab, fb, sent = rf * crop * crop * 3, h * w * 3, 0x5A
    big_ring = torch.full(((S + 2) * slab,), sent, device="cuda", dtype=torch.uint8)
    big_in = torch.full(((n + 4) * fb,), 255, device="cuda", dtype=torch.uint8)
    ring = big_ring[slab:(S + 1) * slab].view(S, rf, crop, crop, 3)
    packed = big_in[2 * fb:(2 + n) * fb].view(n, h, w, 3)
    ring.zero_()
    packed.copy_(_clip(n, h, w))
    xf = frames.FrameTransform(size, crop, train=False, max_side=side)
    store = frames.box_tables(size, side)
    big = 1 << 30
    wild = [(-big, -big, big, big),          # clamped to +-2^20, sides to 64: wholly outside, all zero
            (10, 10, 10, 10),                # zero width and height: the 1 x 1 box at (10, 10)
            (30, 20, 5, -big),               # negative width and height: the 1 x 1 box at (30, 20)
            (big, 3, big + 9, 12),           # far right: zero
            (-3, -4, 45, 200),               # height 204 above max_side: cut to 64
            (4, 2, 36, 38), (-6, 30, 50, 47)]      # two sane rows
    meaning = [OUTSIDE, (10, 10, 11, 11), (30, 20, 31, 21), OUTSIDE, (-3, -4, 45, 60), wild[5], wild[6]]
    rows = [(0, 0), (0, 1), (1, 9), (-1, 3), (S, 4), (1, 5), (0, 6)]      # stream -1 is 0, stream S is S - 1, position 9 is slot 1
    source = [0, 1, 2, 2, 2, 2, 2]                                        # a row past the packed input reads its last frame
    bx = torch.tensor(wild, dtype=torch.int32, device="cuda")
    cx = torch.tensor([[size - crop + 3, -3, 1], [-2, size - crop + 5, 0]], dtype=torch.int32, device="cuda")
    entries = [[size - crop, 0, 1], [0, size - crop, 0]]                  # what the crop entries are clamped to
    row_stream, row_pos = ops.stream_pair_table(rows, "cuda")
    ops.frames_stream_append_boxes(packed, bx, store, size, cx, row_stream, row_pos, 4, ring)
    out = torch.empty((n, 3, crop, crop), device="cuda")
    out_u8 = torch.empty((n, crop, crop, 3), device="cuda", dtype=torch.uint8)
    ops.frames_transform_boxes(packed, bx[[0, 4, 6]].contiguous(), store, size, cx[:1].contiguous(), 3, 0.5, 0.5, out, out_u8)
    torch.cuda.synchronize()
    for guard, lo, hi, v in ((big_ring, slab, (S + 1) * slab, sent), (big_in, 2 * fb, (2 + n) * fb, 255)):
        assert bool((guard[:lo] == v).all()) and bool((guard[hi:] == v).all())
    slots = [(0, 0), (0, 1), (1, 1), (0, 3), (1, 4), (1, 5), (0, 6)]
    for (s, slot), src, box in zip(slots, source, meaning):
        _, want = _sliced(xf, [packed[src]], [box], entries[s])
        assert torch.equal(ring[s, slot], want[0]), (s, slot, box)
    assert not ring[0, 0].any() and not ring[0, 3].any()
    assert bool((ring[0, [2, 4, 5, 7]] == 0).all()) and bool((ring[1, [0, 2, 3, 6, 7]] == 0).all())      # no row named them
    for i, (src, box) in enumerate(zip((0, 1, 2), (OUTSIDE, meaning[4], meaning[6]))):
        ref, ref_u8 = _sliced(xf, [packed[src]], [box], entries[0])
        assert torch.equal(out[i], ref[0]) and torch.equal(out_u8[i], ref_u8[0]), i


# ---------------------------------------------------------------------------------------------- 4. the session
def test_session_with_video_boxes_equals_the_offline_forward_on_padded_slices():
    """A ``logmel`` LFAN on two ragged streams of full 64 x 56 camera frames, a new face box per frame: the logits are the bits
    ``stream_forward`` gives the clip prepared offline through ``pad_slice``, for both streams together, for each alone, and
    through ``finish``; a refused push leaves every stage as it was."""
    from test_live_gpu import FPS, NCLS, _cat, _cut_and_repeat, _examples, _model, _pcm, _raw, _ticks
    from feature_vs_text_compound_emotion_amd import live, streaming
    frames, _ = _mod()
    model, L = _model("logmel"), 4
    raws, pcms = [_raw(L, 1), _raw(L, 2)], [_pcm(0.3, 81), _pcm(0.3, 82)]
    boxes = [_random_boxes(L, 64, 56, 80, seed=11), _random_boxes(L, 64, 56, 80, seed=12)]
    xf = frames.FrameTransform(48, 40, train=False)
    video = torch.stack([_sliced(xf, r, b, [4, 4, 0])[0] for r, b in zip(raws, boxes)])
    ex = _examples(pcms)
    assert ex.shape[1] == 4 and video.shape == (2, L, 3, 40, 40)
    with torch.no_grad():
        ref = streaming.stream_forward(model, {"video": video, "logmel": _cut_and_repeat(ex, L).permute(0, 3, 1, 2).contiguous()})

    def drive(idx, ticks, refuse=False):
        sess = live.AVStream(model, len(idx), FPS, hold=6, lead=4, max_new=2, max_samples=1024, max_side=80)
        out, fv, fa = [[] for _ in idx], [0] * len(idx), [0] * len(idx)

        def collect(logits, counts):
            at = 0
            for s, c in enumerate(counts):
                out[s].append(logits[at:at + c])
                at += c

        for vc, ac in ticks:
            video = _cat([raws[i][f:f + c] for i, f, c in zip(idx, fv, vc)], raws[0]) if sum(vc) else None
            audio = _cat([pcms[i][f:f + c] for i, f, c in zip(idx, fa, ac)], pcms[0]) if sum(ac) else None
            bx = [b for i, f, c in zip(idx, fv, vc) for b in boxes[i][f:f + c]] if sum(vc) else None
            if refuse and sum(vc) and sum(ac):
                state = (list(sess.frames_seen), list(sess.examples_seen), list(sess.audio_stream.samples_seen))
                with pytest.raises(ValueError, match="max_side = 80"):
                    sess.push(video, vc, audio, ac, video_boxes=[(0, 0, 81, 5)] * sum(vc))
                assert state == (sess.frames_seen, sess.examples_seen, list(sess.audio_stream.samples_seen))
                refuse = False
            collect(*sess.push(video, vc if sum(vc) else None, audio, ac if sum(ac) else None, video_boxes=bx))
            fv, fa = [a + b for a, b in zip(fv, vc)], [a + b for a, b in zip(fa, ac)]
        collect(*sess.finish())
        assert not refuse
        return [torch.cat(o) for o in out]

    total = pcms[0].shape[0]
    both = drive([0, 1], _ticks([L, L], [total] * 2, seed=1), refuse=True)
    assert torch.equal(torch.stack(both), ref) and both[0].shape == (L, NCLS)
    for i in (0, 1):
        assert torch.equal(drive([i], _ticks([L], [total], seed=5 + i))[0], ref[i])
