"""NV12 / I420 frames on the GPU.  The invariant: a 4:2:0 call gives exactly what the RGB call gives ``yuv_ref``'s conversion
of the same frames -- the ring bytes through ``take``, the fp32 clip output and ``return_u8`` -- because only the pixel fetch
differs and everything after it is the same integer arithmetic.  Every comparison is ``torch.equal``."""
import functools
import random

import numpy as np
import pytest
import torch

import yuv_ref

pytestmark = pytest.mark.gpu

PAIRS = sorted(yuv_ref.COEFFICIENTS)
# W x H: the smallest picture; a small one; W * 3 no multiple of 4 (the generic horizontal path) and W no multiple of 16 (byte
# staging in the RGB call); the 13-tap dword fast path
SIZES = [(2, 2), (64, 48), (130, 98), (256, 256)]


def _mod():
    from feature_vs_text_compound_emotion_amd import frames
    return frames


def _boxes(w, h):
    """Odd corners and odd sides, one pixel, 7 x 5 (upscaled to 48), over each edge, the picture, and wholly outside (last)."""
    return [(1, 1, min(w, 1 + 33), min(h, 1 + 27)) if w > 2 else (1, 1, 2, 2), (w // 2 - 1, h // 2 - 1, w // 2, h // 2),
            (max(0, w - 9), max(0, h - 7), max(0, w - 9) + 7, max(0, h - 7) + 5), (-5, 3 % h, 16, 3 % h + 9),
            (3 % w, -4, 3 % w + 11, 15),
            (w - 6, 1 % h, w + 9, 1 % h + 21), (1 % w, h - 3, 1 % w + 13, h + 8), (0, 0, w, h), (-3, -3, w + 3, h + 3),
            (w + 40, h + 40, w + 70, h + 55)]


def _on_gpu_at_an_odd_address(arr):
    t = torch.from_numpy(np.ascontiguousarray(arr))
    buf = torch.empty(t.numel() + 1, dtype=torch.uint8, device="cuda")
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    return view


@functools.lru_cache(maxsize=None)
def _case(n, w, h, layout, matrix="bt601", range_="limited", seed=0):
    """(n random 4:2:0 frames [n, h * 3 / 2, w], their conversion [n, h, w, 3] by the numpy reference), both on the GPU."""
    yuv = np.random.default_rng(1000 * h + w + seed).integers(0, 256, (n, h * 3 // 2, w), dtype=np.uint8)
    return _on_gpu_at_an_odd_address(yuv), _on_gpu_at_an_odd_address(yuv_ref.yuv_to_rgb(yuv, layout, matrix, range_))


def _same(xf_yuv, xf_rgb, yuv, rgb, boxes=None, entries=([4, 4, 0], [8, 0, 1])):
    """The clip form: floats, ``return_u8`` and the call without it.  Returns the bytes."""
    for entry in entries:
        out, u8 = xf_yuv(yuv, crop_xyf=[entry], return_u8=True, boxes=boxes)
        ref, ref_u8 = xf_rgb(rgb, crop_xyf=[entry], return_u8=True, boxes=boxes)
        assert out.shape == ref.shape and torch.equal(u8, ref_u8) and torch.equal(out, ref), (entry,)
        assert torch.equal(xf_yuv(yuv, crop_xyf=[entry], boxes=boxes), ref)
    return u8


def _ring(fs, frames, boxes=None):
    n, first = frames.shape[0], fs.frames_seen[0]
    fs.push(frames, [n], boxes)
    return fs.take([(0, first + i) for i in range(n)])


# ---------------------------------------------------------------------------------------------- 1. clip and ring, every size
@pytest.mark.parametrize("layout", yuv_ref.LAYOUTS)
@pytest.mark.parametrize("w,h", SIZES)
def test_unboxed_and_boxed_calls_equal_the_rgb_calls_on_the_converted_frames(w, h, layout):
    frames = _mod()
    boxes = _boxes(w, h)
    yuv, rgb = _case(len(boxes), w, h, layout)
    xf_yuv, xf_rgb = frames.FrameTransform(48, 40, train=False, pixel_format=layout), frames.FrameTransform(48, 40, train=False)
    _same(xf_yuv, xf_rgb, yuv, rgb)
    u8 = _same(xf_yuv, xf_rgb, yuv, rgb, boxes)
    assert not u8[0, -1].any() and u8[0, -3].any()     # the box outside the picture is RGB 0, not YUV 0 converted
    for bx in (None, boxes):
        got = _ring(frames.FrameStream(1, hold=16, max_new=len(boxes), pixel_format=layout), yuv, bx)
        assert torch.equal(got, _ring(frames.FrameStream(1, hold=16, max_new=len(boxes)), rgb, bx))
        assert torch.equal(got, xf_rgb(rgb, boxes=bx)[0])
    two = [[4, 4, 0], [0, 8, 1]]                                                      # [B, L, H * 3 / 2, W], a crop entry per clip
    out4 = xf_yuv(yuv.view(2, len(boxes) // 2, h * 3 // 2, w), crop_xyf=two, boxes=np.array(boxes).reshape(2, -1, 4))
    assert torch.equal(out4, xf_rgb(rgb.view(2, len(boxes) // 2, h, w, 3), crop_xyf=two, boxes=boxes))


@pytest.mark.parametrize("size,crop", [(8, 6), (112, 100)])
def test_other_output_sizes(size, crop):
    """Size 8 takes many taps (beyond the fast path), size 112 upscales a 64 x 48 picture."""
    frames = _mod()
    boxes = _boxes(64, 48)
    yuv, rgb = _case(len(boxes), 64, 48, "nv12")
    xf_yuv, xf_rgb = (frames.FrameTransform(size, crop, train=False, max_side=160, pixel_format=f) for f in ("nv12", "rgb24"))
    entries = ([1, 1, 0], [size - crop, 0, 1])
    _same(xf_yuv, xf_rgb, yuv, rgb, entries=entries)
    _same(xf_yuv, xf_rgb, yuv, rgb, boxes, entries=entries)


# ---------------------------------------------------------------------------------------------- 2. matrices, ranges, layouts
@pytest.mark.parametrize("layout", yuv_ref.LAYOUTS)
@pytest.mark.parametrize("matrix,range_", PAIRS)
def test_every_matrix_and_range(matrix, range_, layout):
    frames = _mod()
    boxes = _boxes(64, 48)
    yuv, rgb = _case(len(boxes), 64, 48, layout, matrix, range_)
    xf_yuv = frames.FrameTransform(48, 40, train=False, pixel_format=layout, matrix=matrix, range=range_)
    xf_rgb = frames.FrameTransform(48, 40, train=False)
    _same(xf_yuv, xf_rgb, yuv, rgb, entries=([4, 4, 0],))
    _same(xf_yuv, xf_rgb, yuv, rgb, boxes, entries=([4, 4, 0],))
    fs = frames.FrameStream(1, hold=16, max_new=len(boxes), pixel_format=layout, matrix=matrix, range=range_)
    assert torch.equal(_ring(fs, yuv, boxes), xf_rgb(rgb, boxes=boxes)[0])


@pytest.mark.parametrize("value", [0, 255])
@pytest.mark.parametrize("matrix,range_", PAIRS)
def test_planes_of_all_0_and_all_255_clip_both_ways(matrix, range_, value):
    frames = _mod()
    w, h = 64, 48
    boxes = _boxes(w, h)
    yuv = np.full((len(boxes), h * 3 // 2, w), value, np.uint8)
    colour = yuv_ref.convert(value, value, value, matrix, range_).tolist()
    assert 0 in colour or 255 in colour                                   # a channel is clipped
    xf_rgb = frames.FrameTransform(48, 40, train=False)
    for layout in yuv_ref.LAYOUTS:
        rgb = yuv_ref.yuv_to_rgb(yuv, layout, matrix, range_)
        assert rgb.reshape(-1, 3).min(0).tolist() == rgb.reshape(-1, 3).max(0).tolist() == colour
        xf_yuv = frames.FrameTransform(48, 40, train=False, pixel_format=layout, matrix=matrix, range=range_)
        a, b = torch.from_numpy(yuv).cuda(), torch.from_numpy(rgb).cuda()
        u8 = _same(xf_yuv, xf_rgb, a, b, entries=([4, 4, 0],))
        assert u8.view(-1, 3).min(0).values.tolist() == u8.view(-1, 3).max(0).values.tolist() == colour
        u8 = _same(xf_yuv, xf_rgb, a, b, boxes, entries=([4, 4, 0],))
        assert not u8[0, -1].any() and u8[0, -3].view(-1, 3)[0].tolist() == colour      # outside: zero; the picture: the colour


def test_the_same_pictures_as_nv12_and_as_i420_give_equal_bytes():
    frames = _mod()
    w, h, n = 130, 98, 4
    rng = np.random.default_rng(9)
    y = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    u, v = rng.integers(0, 256, (2, n, h // 2, w // 2), dtype=np.uint8)
    boxes = _boxes(w, h)[:n]
    got = {}
    for layout in yuv_ref.LAYOUTS:
        packed = torch.from_numpy(yuv_ref.pack(y, u, v, layout)).cuda()
        xf = frames.FrameTransform(48, 40, train=False, pixel_format=layout)
        fs = frames.FrameStream(1, hold=8, max_new=n, pixel_format=layout)
        got[layout] = (xf(packed, return_u8=True), xf(packed, return_u8=True, boxes=boxes), _ring(fs, packed), _ring(fs, packed, boxes))
    assert not torch.equal(torch.from_numpy(yuv_ref.pack(y, u, v, "nv12")), torch.from_numpy(yuv_ref.pack(y, u, v, "i420")))
    for a, b in zip(got["nv12"], got["i420"]):
        for p, q in zip(a, b) if isinstance(a, tuple) else [(a, b)]:
            assert torch.equal(p, q)


# ---------------------------------------------------------------------------------------------- 3. a ragged schedule
def test_ragged_streams_mixed_pushes_changing_geometry_and_a_wrapping_ring():
    """Three streams bring 0 .. 3 frames per push; pushes alternate between boxed and unboxed and between three picture sizes;
    the ring has 8 slots and each stream passes more than twice that.  Every stream equals itself pushed alone and the RGB
    stream fed the converted frames."""
    frames = _mod()
    layout, sizes, rng, pool, ticks = "nv12", [(64, 48), (130, 98), (40, 36)], random.Random(4), 48, []
    used = [0, 0, 0]
    for t in range(16):
        g = t % 3
        counts = [rng.randint(0, 3) for _ in range(3)] if t else [3, 0, 1]
        assert used[g] + sum(counts) <= pool
        w, h = sizes[g]
        lo, used[g] = used[g], used[g] + sum(counts)
        bx = [(rng.randint(-9, w - 2), rng.randint(-9, h - 2)) for _ in range(sum(counts))] if t % 2 else None
        bx = [(x, y, x + rng.randint(1, 41), y + rng.randint(1, 41)) for x, y in bx] if bx is not None else None
        ticks.append((g, lo, counts, bx))
    total = [sum(c[s] for _, _, c, _ in ticks) for s in range(3)]
    assert min(total) > 16 and any(0 in c and sum(c) for _, _, c, _ in ticks)

    def run(fmt, which, streams):
        """Push the schedule's frames of ``streams``; after every push take what it brought.  -> one tensor per stream."""
        fs = frames.FrameStream(len(streams), hold=4, max_new=3, max_side=64, pixel_format=fmt)
        assert fs.ring_frames == 8
        out, seen = [[] for _ in streams], [0] * len(streams)
        for g, lo, counts, bx in ticks:
            src = _case(pool, *sizes[g], layout)[which]
            starts = [lo + sum(counts[:s]) for s in range(3)]
            rows = [i for s in streams for i in range(starts[s], starts[s] + counts[s])]
            c = [counts[s] for s in streams]
            if not rows:
                continue
            fs.push(src[rows], c, [bx[i - lo] for i in rows] if bx is not None else None)
            got, at = fs.take([(k, seen[k] + i) for k in range(len(streams)) for i in range(c[k])]), 0
            for k in range(len(streams)):
                out[k].append(got[at:at + c[k]])
                at, seen[k] = at + c[k], seen[k] + c[k]
        assert seen == [total[s] for s in streams]
        return [torch.cat(o) for o in out]

    together, rgb = run(layout, 0, [0, 1, 2]), run("rgb24", 1, [0, 1, 2])
    for s in range(3):
        assert torch.equal(together[s], rgb[s]), s
        assert torch.equal(together[s], run(layout, 0, [s])[0]), s


def test_hold_counts_reset_and_refusals_work_as_in_rgb_mode():
    frames = _mod()
    yuv, rgb = _case(10, 64, 48, "i420")
    fs = frames.FrameStream(2, hold=4, max_new=3, pixel_format="i420")
    fs.push(yuv[:4], [3, 1])
    state = (list(fs.frames_seen), list(fs.frames_taken))
    for bad, counts, match in ((yuv[:3], [2, 1], "exceed hold"), (yuv[:4], [1, 4], "max_new"), (yuv[:2], [1, 2], "frames for counts"),
                               (yuv[:2, :71], [1, 1], r"H \* 3 / 2"), (yuv[:2, :, :63], [1, 1], "even W"),
                               (rgb[:2], [1, 1], r"\[M, H \* 3 / 2, W\]"),
                               (yuv[:2].cpu(), [1, 1], "must be on the GPU")):
        with pytest.raises(ValueError, match=match):
            fs.push(bad, counts)
    with pytest.raises(ValueError, match="even W"):
        frames.FrameTransform(48, 40, train=False, pixel_format="i420")(yuv[:2, :, :63])
    assert state == (fs.frames_seen, fs.frames_taken)
    ref = frames.FrameTransform(48, 40, train=False)(rgb)[0]
    assert torch.equal(fs.take([(0, 2), (1, 0)]), ref[[2, 3]])
    fs.reset([0])
    fs.push(yuv[4:8], [3, 1])
    assert fs.frames_seen == [3, 2] and torch.equal(fs.take([(0, 0), (0, 1), (0, 2), (1, 1)]), ref[4:8])


# ---------------------------------------------------------------------------------------------- 4. the session
@pytest.mark.parametrize("layout,matrix,range_", [("nv12", "bt601", "limited"), ("i420", "bt709", "full")])
def test_session_on_decoder_frames_equals_the_rgb_session_on_the_converted_frames(layout, matrix, range_):
    from test_live_gpu import FPS, H, W, _drive, _model, _pcm, _ticks
    from feature_vs_text_compound_emotion_amd import live
    model, L = _model("logmel"), 4
    cases = [_case(L, W, H, layout, matrix, range_, seed=s) for s in (1, 2)]
    pcms = [_pcm(0.3, 81), _pcm(0.3, 82)]
    ticks = _ticks([L, L], [pcms[0].shape[0]] * 2, seed=1)
    kw = dict(hold=6, lead=4, max_new=2, max_samples=1024)
    got = _drive(live.AVStream(model, 2, FPS, video_format=layout, video_matrix=matrix, video_range=range_, **kw),
                 [c[0] for c in cases], pcms, ticks, [None])
    want = _drive(live.AVStream(model, 2, FPS, **kw), [c[1] for c in cases], pcms, ticks, [None])
    for g, r in zip(got, want):
        assert g.shape == (L, 7) and torch.equal(g, r)
    with pytest.raises(ValueError, match="video_format|pixel_format"):
        live.AVStream(model, 2, FPS, video_format="nv21", **kw)
