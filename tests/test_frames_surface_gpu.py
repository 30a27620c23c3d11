"""BGR(A), YUYV / UYVY, pitched surfaces and strided views on the GPU.  The invariant is the one of the 4:2:0 work: only the
pixel fetch differs, so a call on frames of any format and layout gives exactly what the ``"rgb24"`` call gives
``surface_ref.to_rgb`` of the same frames, tightly packed -- the ring bytes through ``take``, the fp32 clip output and
``return_u8``, plain, boxed and aligned.  Every comparison is ``torch.equal``; inputs sit at an odd device address."""
import functools
import math
import random

import numpy as np
import pytest
import torch

import surface_ref
import yuv_ref
from test_frames_yuv_gpu import _boxes, _on_gpu_at_an_odd_address

pytestmark = pytest.mark.gpu

PACKED = ("bgr24", "rgba32", "bgra32")
YUV422 = ("yuyv422", "uyvy422")
PAIRS = sorted(yuv_ref.COEFFICIENTS)
ALIGN = 32
ENTRIES = ([4, 4, 0], [8, 0, 1])


def _mod():
    from feature_vs_text_compound_emotion_amd import frames
    return frames


def _affines(n, w, h):
    """Pillow coefficients of three maps, repeated to n rows: the whole picture onto the face, a rotation by 25 degrees about
    the picture's centre at twice the scale, and one that is mostly outside the picture."""
    sx, sy, c, s = w / ALIGN, h / ALIGN, math.cos(math.radians(25)), math.sin(math.radians(25))
    rot = [2 * sx * c, -2 * sy * s, w / 2 - (sx * c - sy * s) * ALIGN, 2 * sx * s, 2 * sy * c, h / 2 - (sx * s + sy * c) * ALIGN]
    maps = [[sx, 0.0, 0.0, 0.0, sy, 0.0], rot, [sx, 0.0, -0.8 * w, 0.0, sy, 0.7 * h]]
    return np.array([maps[i % 3] for i in range(n)], np.float64)


@functools.lru_cache(maxsize=None)
def _tight(fmt, n, w, h, seed=0):
    """n random tightly packed frames of ``fmt`` (numpy)."""
    return np.random.default_rng(1000 * h + w + seed).integers(0, 256, surface_ref.tight_shape(fmt, n, h, w), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _want(key, w, h, n):
    """The reference side, computed once per set of RGB frames: every output of ``_run`` from the ``"rgb24"`` calls on the
    converted, tightly packed frames.  ``key`` -> the frames through ``_RGB``."""
    return _run("rgb24", _on_gpu_at_an_odd_address(_RGB[key]), w, h, n)


_RGB = {}


def _run(fmt, src, w, h, n, matrix="bt601", range_="limited", layout=None, entries=ENTRIES):
    """Every kind of call on the n frames ``src``: the clip form (floats, ``return_u8`` and the call without it, two crop
    entries with and without flip) and the ring form through ``take``, each plain, with the ten boxes and with three affines.
    -> a list of tensors, in a fixed order."""
    frames = _mod()
    kw = {} if layout is None else {"layout": layout}
    xf = frames.FrameTransform(48, 40, train=False, pixel_format=fmt, matrix=matrix, range=range_)
    boxes, aff, out = _boxes(w, h), _affines(n, w, h), []
    assert n == len(boxes)
    clip = src.unsqueeze(0)
    for entry in entries:
        for call in (lambda **k: xf(clip, crop_xyf=[entry], **k, **kw), lambda **k: xf(clip, crop_xyf=[entry], boxes=boxes, **k, **kw),
                     lambda **k: xf.aligned(clip, aff, crop_xyf=[entry], align_size=ALIGN, **k, **kw)):
            f32, u8 = call(return_u8=True)
            assert torch.equal(call(), f32) and f32.shape == (1, n, 3, 40, 40) and u8.shape == (1, n, 40, 40, 3)
            out += [f32, u8]
    assert not out[3][0, -1].any() and out[3][0, -3].any()      # the box outside the picture is RGB 0; the whole picture is not
    fs = frames.FrameStream(1, hold=3 * n, max_new=n, pixel_format=fmt, matrix=matrix, range=range_)
    fs.push(src, [n], **kw)
    fs.push(src, [n], boxes, **kw)
    fs.push_aligned(src, [n], aff, align_size=ALIGN, **kw)
    got = fs.take([(0, i) for i in range(3 * n)])
    assert torch.equal(got[:n], out[0][0]) and torch.equal(got[n:2 * n], out[2][0]) and torch.equal(got[2 * n:], out[4][0])
    return out + [got]


def _same(fmt, tight, w, h, matrix="bt601", range_="limited", layout=None, fill=None, key=None):
    """``_run`` on ``tight`` (embedded in ``layout`` over ``fill``) equals the reference side on its conversion."""
    n = tight.shape[0]
    rgb = surface_ref.to_rgb(tight, fmt, matrix, range_)
    key = key or (fmt, w, h, matrix, range_, hash(tight.tobytes()))
    _RGB.setdefault(key, rgb)
    src = tight if layout is None else surface_ref.embed(tight, layout, fill)
    got = _run(fmt, _on_gpu_at_an_odd_address(src), w, h, n, matrix, range_, layout)
    want = _want(key, w, h, n)
    assert len(got) == len(want)
    for i, (g, r) in enumerate(zip(got, want)):
        assert g.shape == r.shape and torch.equal(g, r), (fmt, w, h, i)
    return got


# ---------------------------------------------------------------------------------------------- 1. packed orders
# W x H: the smallest picture; a small one; W * 3 no multiple of 4 (the generic horizontal path); the 13-tap dword fast path
@pytest.mark.parametrize("fmt", PACKED)
@pytest.mark.parametrize("w,h", [(1, 1), (64, 48), (130, 98), (256, 256)])
def test_packed_orders_equal_the_rgb_calls_on_the_reordered_frames(w, h, fmt):
    tight = _tight(fmt, 10, w, h)
    _same(fmt, tight, w, h)
    if tight.shape[-1] == 4:        # the fourth byte never reaches a result: another alpha, the same bits
        other = tight.copy()
        other[..., 3] = _tight(fmt, 10, w, h, seed=5)[..., 3]
        assert not np.array_equal(other, tight)
        _same(fmt, other, w, h)


# ---------------------------------------------------------------------------------------------- 2. 4:2:2
@pytest.mark.parametrize("fmt", YUV422)
@pytest.mark.parametrize("w,h", [(2, 1), (64, 48), (130, 97), (256, 256)])
def test_422_equals_the_rgb_calls_on_the_converted_frames(w, h, fmt):
    _same(fmt, _tight(fmt, 10, w, h), w, h)


@pytest.mark.parametrize("fmt", YUV422)
@pytest.mark.parametrize("matrix,range_", PAIRS)
def test_422_every_matrix_and_range(matrix, range_, fmt):
    _same(fmt, _tight(fmt, 10, 64, 48), 64, 48, matrix, range_)


@pytest.mark.parametrize("value", [0, 255])
@pytest.mark.parametrize("matrix,range_", PAIRS)
def test_422_bytes_of_all_0_and_all_255_clip_both_ways(matrix, range_, value):
    w, h = 64, 48
    colour = yuv_ref.convert(value, value, value, matrix, range_).tolist()
    assert 0 in colour or 255 in colour                                   # a channel is clipped
    for fmt in YUV422:
        tight = np.full((10, h, w, 2), value, np.uint8)
        got = _same(fmt, tight, w, h, matrix, range_)
        plain, boxed = got[1], got[3]                                     # return_u8 of the first entry, plain and boxed
        assert plain.view(-1, 3).min(0).values.tolist() == plain.view(-1, 3).max(0).values.tolist() == colour
        # a box outside the picture is RGB 0, not YUV 0 converted; the picture is the colour
        assert not boxed[0, -1].any() and boxed[0, -3].view(-1, 3)[0].tolist() == colour


def test_the_same_picture_as_yuyv_and_as_uyvy_gives_equal_bytes():
    w, h, n = 130, 97, 10
    yuyv = _tight("yuyv422", n, w, h, seed=9)
    uyvy = np.ascontiguousarray(yuyv.reshape(n, h, w // 2, 4)[..., [1, 0, 3, 2]].reshape(n, h, w, 2))
    assert np.array_equal(surface_ref.to_rgb(yuyv, "yuyv422"), surface_ref.to_rgb(uyvy, "uyvy422")) and not np.array_equal(yuyv, uyvy)
    a = _run("yuyv422", _on_gpu_at_an_odd_address(yuyv), w, h, n)
    b = _run("uyvy422", _on_gpu_at_an_odd_address(uyvy), w, h, n)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


# ---------------------------------------------------------------------------------------------- 3. pitched surfaces
def _pitched(fmt, w, h, chroma="uv"):
    """Row pitch = row bytes + 7 (every row misaligned), planes padded by 3 rows, a 5-byte tail before the next frame, and
    under 4:2:0 a chroma pitch of its own."""
    frames = _mod()
    tight = frames.surface_layout(fmt, h, w)
    pitch = tight.pitch + 7
    if fmt == "nv12":
        cp = w + 11
        return frames.surface_layout(fmt, h, w, pitch=pitch, chroma_pitch=cp, offsets=(0, (h + 3) * pitch),
                                     frame_stride=(h + 3) * pitch + (h // 2 + 3) * cp + 5, chroma=chroma)
    if fmt == "i420":
        cp, c1 = w // 2 + 3, (h + 3) * pitch
        return frames.surface_layout(fmt, h, w, pitch=pitch, chroma_pitch=cp, offsets=(0, c1, c1 + (h // 2 + 3) * cp),
                                     frame_stride=c1 + 2 * (h // 2 + 3) * cp + 5, chroma=chroma)
    return frames.surface_layout(fmt, h, w, pitch=pitch, frame_stride=(h + 3) * pitch + 5)


def _fill(layout, n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, layout.frame_stride), dtype=np.uint8)


@pytest.mark.parametrize("fmt", surface_ref.FORMATS)
@pytest.mark.parametrize("w,h", [(64, 48), (130, 98)])
def test_pitched_surfaces_equal_the_tight_call_whatever_the_padding_holds(w, h, fmt):
    frames = _mod()
    tight, lay = _tight(fmt, 10, w, h), _pitched(fmt, w, h)
    for seed in (1, 2):                                            # no padding byte reaches a result
        got = _same(fmt, tight, w, h, layout=lay, fill=_fill(lay, 10, seed))
    if fmt != "rgb24":                                             # and that is the tight call of the format itself
        plain = _run(fmt, _on_gpu_at_an_odd_address(tight), w, h, 10, layout=None if fmt in PACKED + YUV422 else frames.surface_layout(fmt, h, w))
        assert all(torch.equal(p, q) for p, q in zip(got, plain))
    if fmt in yuv_ref.LAYOUTS:
        today = frames.FrameTransform(48, 40, train=False, pixel_format=fmt)(_on_gpu_at_an_odd_address(tight), crop_xyf=[ENTRIES[0]])
        assert torch.equal(today, got[0])                          # today's 4:2:0 entries on the tight frames
        # V first: the tight call on frames with U and V exchanged
        vu = _pitched(fmt, w, h, chroma="vu")
        swapped = surface_ref.swap_uv(tight, fmt)
        rgb = surface_ref.to_rgb(swapped, fmt)
        assert not np.array_equal(rgb, surface_ref.to_rgb(tight, fmt))
        key = ("vu", fmt, w, h)
        _RGB.setdefault(key, rgb)
        got = _run(fmt, _on_gpu_at_an_odd_address(surface_ref.embed(tight, vu, _fill(vu, 10, 3))), w, h, 10, layout=vu)
        assert all(torch.equal(p, q) for p, q in zip(got, _want(key, w, h, 10)))


def test_a_decoder_shaped_nv12_surface():
    """130 x 98 with pitch 256 and the luma plane padded to 112 rows: the chroma does not start at H * W."""
    frames = _mod()
    w, h = 130, 98
    lay = frames.surface_layout("nv12", h, w, pitch=256, offsets=(0, 256 * 112))
    assert lay.frame_stride == 256 * (112 + 49)
    tight = _tight("nv12", 10, w, h)
    _same("nv12", tight, w, h, layout=lay, fill=_fill(lay, 10, 4))
    # the buffer in the shape a decoder hands it out, [M, rows, pitch]
    buf = _on_gpu_at_an_odd_address(surface_ref.embed(tight, lay, _fill(lay, 10, 4)).reshape(10, 161, 256))
    fs, ref = frames.FrameStream(1, hold=16, max_new=10, pixel_format="nv12"), frames.FrameStream(1, hold=16, max_new=10, pixel_format="nv12")
    fs.push(buf, [10], layout=lay)
    ref.push(_on_gpu_at_an_odd_address(tight), [10])
    pairs = [(0, i) for i in range(10)]
    assert torch.equal(fs.take(pairs), ref.take(pairs))


# ---------------------------------------------------------------------------------------------- 4. strided views
@pytest.mark.parametrize("fmt", ("rgb24", "bgr24", "bgra32", "uyvy422"))
def test_strided_views_are_read_in_place(fmt, monkeypatch):
    from feature_vs_text_compound_emotion_amd import ops
    frames = _mod()
    w, h, n = 64, 48, 10
    chan = surface_ref.tight_shape(fmt, 1, h, w)[3]
    big = _on_gpu_at_an_odd_address(np.random.default_rng(7).integers(0, 256, (n, h + 3, w + 5, chan), dtype=np.uint8))
    view = big[:, 2:2 + h, 3:3 + w]
    assert not view.is_contiguous()
    lay = frames.SurfaceLayout.of_view(view, fmt)
    assert (lay.height, lay.width, lay.pitch, lay.frame_stride, lay.offsets) == (h, w, (w + 5) * chan, (h + 3) * (w + 5) * chan, (0,))
    fs, ref = (frames.FrameStream(1, hold=32, max_new=n, pixel_format=fmt) for _ in range(2))
    seen = []
    for name in ("frames_stream_append", "frames_stream_append_boxes", "frames_stream_append_affine"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda f, *a, _real=real, **k: (seen.append((f.data_ptr(), k.get("surface"))), _real(f, *a, **k))[1])
    boxes, aff = _boxes(w, h), _affines(n, w, h)
    fs.push(view, [n]), fs.push(view, [n], boxes), fs.push_aligned(view, [n], aff, align_size=ALIGN)
    assert [p for p, _ in seen] == [view.data_ptr()] * 3 and all(s is not None and s.layout == lay for _, s in seen)     # no copy
    packed = view.contiguous()
    ref.push(packed, [n]), ref.push(packed, [n], boxes), ref.push_aligned(packed, [n], aff, align_size=ALIGN)
    pairs = [(0, i) for i in range(3 * n)]
    want = ref.take(pairs)
    assert torch.equal(fs.take(pairs), want)
    # the wrapper itself on the view
    ring = torch.zeros_like(fs.ring)
    tables, span = fs._xf._plain(h, w, view.device)
    rs, rp = ops.stream_row_table([0], [n], view.device)
    ops.frames_stream_append(view, tables, span, 48, fs._cx, rs, rp, n, ring, surface=frames.Surface(lay, fs._xf._coef))
    assert torch.equal(ops.frames_stream_gather(ring, rs, rp), want[:n])
    with pytest.raises(ValueError, match="frames: .*strides"):
        ops.frames_stream_append(view[:, :, 1:], tables, span, 48, fs._cx, rs, rp, n, ring, surface=frames.Surface(lay, fs._xf._coef))
    # the clip form takes the view too, and a view with a last stride != 1 still works, through the copy
    xf = frames.FrameTransform(48, 40, train=False, pixel_format=fmt)
    assert torch.equal(xf(view.unsqueeze(0), crop_xyf=[ENTRIES[1]]), xf(packed.unsqueeze(0), crop_xyf=[ENTRIES[1]]))
    wide = _on_gpu_at_an_odd_address(np.random.default_rng(8).integers(0, 256, (n, h, w, 2 * chan), dtype=np.uint8))[..., ::2]
    assert wide.stride(3) == 2
    seen.clear()
    fs.push(wide, [n])
    ref.push(wide.contiguous(), [n])
    assert seen[0][0] != wide.data_ptr()
    pairs = [(0, 3 * n + i) for i in range(n)]
    assert torch.equal(fs.take(pairs), ref.take(pairs))


# ---------------------------------------------------------------------------------------------- 5. streams
def test_ragged_streams_mixed_pushes_changing_layouts_and_a_wrapping_ring():
    """Three streams bring 0 .. 3 frames per push; pushes alternate between plain, boxed and aligned, between three picture
    sizes and between a tight tensor, a pitched surface and a strided view; the ring has 8 slots and each stream passes more
    than twice that.  Equal to the RGB stream fed the converted frames."""
    frames = _mod()
    fmt, sizes, rng, pool, ticks = "bgra32", [(64, 48), (130, 98), (40, 36)], random.Random(4), 48, []
    used = [0, 0, 0]
    for t in range(18):
        g = t % 3
        counts = [rng.randint(0, 3) for _ in range(3)] if t else [3, 0, 1]
        assert used[g] + sum(counts) <= pool
        w, h = sizes[g]
        lo, used[g] = used[g], used[g] + sum(counts)
        bx = [(rng.randint(-9, w - 2), rng.randint(-9, h - 2)) for _ in range(sum(counts))]
        bx = [(x, y, x + rng.randint(1, 41), y + rng.randint(1, 41)) for x, y in bx]
        ticks.append((g, lo, counts, bx, ("plain", "boxed", "aligned")[(t // 3) % 3], ("tight", "pitched", "view")[(t + t // 3) % 3]))
    total = [sum(c[s] for _, _, c, *_ in ticks) for s in range(3)]
    assert min(total) > 16 and len({(k, how) for *_, k, how in ticks}) == 9

    def run(which):
        fs = frames.FrameStream(3, hold=4, max_new=3, max_side=64, pixel_format=which)
        assert fs.ring_frames == 8
        out, seen = [[] for _ in range(3)], [0, 0, 0]
        for g, lo, counts, bx, kind, how in ticks:
            n, (w, h) = sum(counts), sizes[g]
            if not n:
                continue
            tight, kw = _tight(fmt, pool, w, h)[lo:lo + n], {}
            if which == "rgb24":
                src = surface_ref.to_rgb(tight, fmt)
            elif how == "pitched":
                kw["layout"] = _pitched(fmt, w, h)
                src = surface_ref.embed(tight, kw["layout"], _fill(kw["layout"], n, lo))
            else:
                src = tight
            src = _on_gpu_at_an_odd_address(src)
            if which != "rgb24" and how == "view":
                big = torch.zeros((n, h + 3, w + 5, 4), dtype=torch.uint8, device="cuda")
                big[:, 1:1 + h, 5:] = src
                src = big[:, 1:1 + h, 5:]
            if kind == "plain":
                fs.push(src, counts, **kw)
            elif kind == "boxed":
                fs.push(src, counts, bx, **kw)
            else:
                fs.push_aligned(src, counts, _affines(n, w, h), align_size=ALIGN, **kw)
            got, at = fs.take([(k, seen[k] + i) for k in range(3) for i in range(counts[k])]), 0
            for k in range(3):
                out[k].append(got[at:at + counts[k]])
                at, seen[k] = at + counts[k], seen[k] + counts[k]
        assert seen == total
        return [torch.cat(o) for o in out]

    for a, b in zip(run(fmt), run("rgb24")):
        assert torch.equal(a, b)


def test_a_refused_layout_leaves_the_ints_and_the_ring_as_they_were():
    frames = _mod()
    w, h = 64, 48
    tight = _tight("yuyv422", 6, w, h)
    lay = _pitched("yuyv422", w, h)
    buf = _on_gpu_at_an_odd_address(surface_ref.embed(tight, lay, _fill(lay, 6, 1)))
    fs = frames.FrameStream(2, hold=8, max_new=4, pixel_format="yuyv422")
    fs.push(buf[:4], [3, 1], layout=lay)
    state, ring = (list(fs.frames_seen), list(fs.frames_taken)), fs.ring.clone()
    aff = _affines(2, w, h)
    for f, counts, layout, match in ((buf[:2], [1, 1], _pitched("uyvy422", w, h), "layout: .*pixel_format"),
                                     (buf[:2, :-1], [1, 1], lay, "frames: .*frame_stride"), (buf[:2], [1, 1], "yuyv422", "layout: .*SurfaceLayout"),
                                     (buf[:2], [1, 1], frames.surface_layout("yuyv422", h, w), "frames: .*frame_stride"),
                                     (buf[:3], [1, 1], lay, "frames for counts"), (buf[:2].cpu(), [1, 1], lay, "must be on the GPU"),
                                     (buf[:2], [5, 0], lay, "max_new")):
        for call in (lambda: fs.push(f, counts, layout=layout), lambda: fs.push(f, counts, [[0, 0, 4, 4]] * 2, layout=layout),
                     lambda: fs.push_aligned(f, counts, aff, align_size=ALIGN, layout=layout), lambda: fs.check_push(f, counts, layout=layout)):
            with pytest.raises(ValueError, match=match):
                call()
    assert state == (fs.frames_seen, fs.frames_taken) and torch.equal(ring, fs.ring)
    ref = frames.FrameTransform(48, 40, train=False)(_on_gpu_at_an_odd_address(surface_ref.to_rgb(tight, "yuyv422")).unsqueeze(0))[0]
    fs.push(buf[4:], [1, 1], layout=lay)
    assert torch.equal(fs.take([(0, 0), (0, 1), (0, 2), (1, 0), (0, 3), (1, 1)]), ref)


# ---------------------------------------------------------------------------------------------- 6. the session
class _Surfaces:
    """A session fed through ``video_layout=``: every push of tight frames is embedded into a pitched surface first."""

    def __init__(self, sess, layout):
        self.sess, self.layout, self.streams, self.pushes = sess, layout, sess.streams, 0

    def push(self, video, video_counts, audio, audio_counts, extra=None):
        if video is None:
            return self.sess.push(None, None, audio, audio_counts, extra=extra)
        self.pushes += 1
        buf = surface_ref.embed(video.cpu().numpy(), self.layout, _fill(self.layout, video.shape[0], self.pushes))
        return self.sess.push(_on_gpu_at_an_odd_address(buf), video_counts, audio, audio_counts, extra=extra, video_layout=self.layout)

    def finish(self, group):
        return self.sess.finish(group)


@pytest.mark.parametrize("fmt,matrix,range_", [("bgra32", "bt601", "limited"), ("yuyv422", "bt709", "full")])
def test_session_on_surfaces_equals_the_rgb_session_on_the_converted_frames(fmt, matrix, range_):
    from test_live_gpu import FPS, H, W, _drive, _model, _pcm, _ticks
    from feature_vs_text_compound_emotion_amd import live
    model, L = _model("logmel"), 4
    tights = [_tight(fmt, L, W, H, seed=s) for s in (1, 2)]
    rgbs = [torch.from_numpy(surface_ref.to_rgb(t, fmt, matrix, range_)).cuda() for t in tights]
    pcms = [_pcm(0.3, 81), _pcm(0.3, 82)]
    ticks = _ticks([L, L], [pcms[0].shape[0]] * 2, seed=1)
    kw = dict(hold=6, lead=4, max_new=2, max_samples=1024)
    lay = _pitched(fmt, W, H)
    sess = live.AVStream(model, 2, FPS, video_format=fmt, video_matrix=matrix, video_range=range_, **kw)
    fed = _Surfaces(sess, lay)
    got = _drive(fed, [torch.from_numpy(t).cuda() for t in tights], pcms, ticks, [None])
    want = _drive(live.AVStream(model, 2, FPS, **kw), rgbs, pcms, ticks, [None])
    assert fed.pushes > 1
    for g, r in zip(got, want):
        assert g.shape == (L, 7) and torch.equal(g, r)
    # a refused layout changes no stage's state
    before = (list(sess.frames_seen), list(sess.examples_seen), list(sess.paired), list(sess.frame_stream.frames_seen))
    bad = torch.zeros((2, lay.frame_stride - 1), dtype=torch.uint8, device="cuda")
    for layout, match in ((lay, "frame_stride"), (_pitched("bgr24", W, H), "pixel_format")):
        with pytest.raises(ValueError, match=match):
            sess.push(bad, [1, 1], pcms[0][:160 * 2].repeat(2), [320, 320], video_layout=layout)
    with pytest.raises(ValueError, match="video_layout without video"):
        sess.push(audio=pcms[0][:640], audio_counts=[320, 320], video_layout=lay)
    assert before == (sess.frames_seen, sess.examples_seen, sess.paired, sess.frame_stream.frames_seen)
