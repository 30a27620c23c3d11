"""Per-frame affine maps on full camera frames, on the GPU (csrc/frames_affine.hip).  Frame f with affine a must give exactly
the bytes, and the floats, that today's ``FrameTransform`` gives the A x A picture ``affine_ref.warp_affine`` (Pillow's AFFINE
transform with BILINEAR sampling, restated and held to Pillow in tests/test_frames_affine_cpu.py) makes of that frame: the warp
is the same float64 operations in the same order and the two passes are the same integer sums, so every comparison is
``torch.equal``."""
import functools
import random

import numpy as np
import pytest
import torch

import yuv_ref
from affine_ref import GOLDEN_AFFINES, GOLDEN_ALIGN, similarity, warp_all
from helpers import golden

pytestmark = pytest.mark.gpu

OUTSIDE = [1.0, 0.0, 500.0, 0.0, 1.0, -300.0]      # no pixel of any frame used here
GEOMETRIES = [(33, 47, 8, 12, 8), (33, 47, 21, 48, 40), (90, 120, 32, 48, 40), (90, 120, 21, 12, 8), (33, 47, 32, 12, 8)]


def _mod():
    from feature_vs_text_compound_emotion_amd import frames, ops
    return frames, ops


def _on_gpu_at_an_odd_address(arr):
    t = torch.from_numpy(np.ascontiguousarray(arr))
    buf = torch.empty(t.numel() + 1, dtype=torch.uint8, device="cuda")
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    return view


def _random_affines(n, h, w, align, seed):
    """Rotations to +-35 degrees, scales 0.3 .. 4 (in units of the frame's share of the face), centres in and a little
    around the frame: most faces hang over an edge."""
    rng = random.Random(seed)
    unit = min(h, w) / align
    return [similarity(rng.uniform(-35, 35), rng.uniform(0.3, 4.0) * unit / 2, rng.uniform(-0.1 * w, 1.1 * w),
                       rng.uniform(-0.1 * h, 1.1 * h), align) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def _case(n, h, w, align, seed=0):
    """(frames [n, h, w, 3] on the GPU, affines float64 [n, 6], the restatement's warped faces [n, align, align, 3] on the GPU).
    The 90 x 120, align 32 case is the Pillow fixture itself, its frame repeated."""
    if (n, h, w, align, seed) == (len(GOLDEN_AFFINES), 90, 120, GOLDEN_ALIGN, 0):
        g = golden("frames_affine.npz")
        frames = np.repeat(g["frame"][None], n, axis=0)
        return _on_gpu_at_an_odd_address(frames), g["affines"], torch.from_numpy(g["warped"]).cuda()
    frames = np.random.default_rng(1000 * h + w + seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    affines = np.array(_random_affines(n, h, w, align, seed=100 * align + seed), np.float64)
    affines[-1] = OUTSIDE
    return _on_gpu_at_an_odd_address(frames), affines, torch.from_numpy(warp_all(frames, affines, align)).cuda()


def _entries(xf):
    size, crop = xf.size, xf.crop
    return xf.draw(1)[0].tolist(), [size - crop, 1, 1], [0, size - crop, 1]      # centre; two corners, flipped


# ---------------------------------------------------------------------------------------------- 1. the clip form
@pytest.mark.parametrize("h,w,align,size,crop", GEOMETRIES)
def test_aligned_equals_todays_path_on_the_warped_faces(h, w, align, size, crop):
    frames, _ = _mod()
    clip, affines, warped = _case(8, h, w, align)
    xf = frames.FrameTransform(size, crop, train=False)
    for entry in _entries(xf):
        out, u8 = xf.aligned(clip, affines, crop_xyf=[entry], return_u8=True, align_size=align)
        ref, ref_u8 = xf(warped, crop_xyf=[entry], return_u8=True)
        assert out.shape == (1, 8, 3, crop, crop) and u8.shape == (1, 8, crop, crop, 3)
        assert torch.equal(u8, ref_u8) and torch.equal(out, ref), (entry,)
        assert not u8[0, -1].any()                                                        # the map outside the frame
        assert torch.equal(xf.aligned(clip, affines, crop_xyf=[entry], align_size=align), ref)      # without the uint8 output
    # [B, L]: one crop entry per clip, affines [B, L, 6]
    cx = [[size - crop, 0, 1], [1, size - crop, 0]]
    out, u8 = xf.aligned(clip.view(2, 4, h, w, 3), affines.reshape(2, 4, 6), crop_xyf=cx, return_u8=True, align_size=align)
    ref, ref_u8 = xf(warped.view(2, 4, align, align, 3), crop_xyf=cx, return_u8=True)
    assert torch.equal(u8, ref_u8) and torch.equal(out, ref)


def test_aligned_equals_the_pillow_fixture_through_todays_path():
    frames, _ = _mod()
    clip, affines, warped = _case(len(GOLDEN_AFFINES), 90, 120, GOLDEN_ALIGN)
    assert torch.equal(warped, torch.from_numpy(golden("frames_affine.npz")["warped"]).cuda())
    xf = frames.FrameTransform(48, 40, train=False)
    out, u8 = xf.aligned(clip, GOLDEN_AFFINES, return_u8=True, align_size=GOLDEN_ALIGN)      # a list of lists
    ref, ref_u8 = xf(warped, return_u8=True)
    assert torch.equal(u8, ref_u8) and torch.equal(out, ref)
    train = frames.FrameTransform(48, 40, train=True)                                        # drawn crop and flip
    random.seed(4)
    out = train.aligned(clip, affines, align_size=GOLDEN_ALIGN)
    random.seed(4)
    assert torch.equal(out, train(warped))


def test_aligned_at_the_default_align_size():
    """256 -> 48: the 13-tap geometry of the reference's data, on a frame smaller than the face."""
    frames, _ = _mod()
    clip, _, _ = _case(8, 33, 47, 8)
    affines = np.array([similarity(10.0, 0.9 * 33 / 256, 23.5, 16.5, 256), similarity(-25.0, 1.4 * 33 / 256, 30.0, 10.0, 256)])
    warped = torch.from_numpy(warp_all(clip[:2].cpu().numpy(), affines, 256)).cuda()
    xf = frames.FrameTransform(48, 40, train=False)
    out, u8 = xf.aligned(clip[:2], affines, return_u8=True)
    ref, ref_u8 = xf(warped, return_u8=True)
    assert torch.equal(u8, ref_u8) and torch.equal(out, ref) and u8[0, 0].any() and u8[0, 1].any()


# ---------------------------------------------------------------------------------------------- 2. the ring form
N, H, W, ALIGN = 12, 33, 47, 21


@functools.lru_cache(maxsize=None)
def _stream_case(seed):
    """(frames [N, H, W, 3], affines [N, 6], warped [N, ALIGN, ALIGN, 3], what ``push`` of the warped faces then ``take``
    gives [N, 3, 40, 40])."""
    frames, _ = _mod()
    clip, affines, warped = _case(N, H, W, ALIGN, seed)
    fs = frames.FrameStream(1, hold=16, max_new=N)
    fs.push(warped, [N])
    return clip, affines, warped, fs.take([(0, i) for i in range(N)])


@pytest.mark.parametrize("size,crop", [(48, 40), (12, 8)])
def test_push_aligned_then_take_equals_push_of_the_warped_faces(size, crop):
    frames, _ = _mod()
    clip, affines, warped = _case(N, H, W, ALIGN, 1)
    cx = [[size - crop, 1, 1]]
    a, b = (frames.FrameStream(1, size=size, crop=crop, hold=4, max_new=2, crop_xyf=cx) for _ in range(2))
    assert a.ring_frames == 8                              # 12 frames: the ring wraps
    for i in range(0, N, 2):
        a.push_aligned(clip[i:i + 2], [2], affines[i:i + 2], align_size=ALIGN)
        b.push(warped[i:i + 2], [2])
        pairs = [(0, i), (0, i + 1)]
        assert torch.equal(a.take(pairs), b.take(pairs)), i
    assert a.frames_seen == [N] and torch.equal(a.ring, b.ring)


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
    fs = frames.FrameStream(3, hold=16, max_new=3)
    alone = [frames.FrameStream(1, hold=16, max_new=3) for _ in range(3)]
    for start, c in ticks:
        if not sum(c):
            continue
        fs.push_aligned(torch.cat([cases[s][0][start[s]:start[s] + c[s]] for s in range(3)]), c,
                        np.concatenate([cases[s][1][start[s]:start[s] + c[s]] for s in range(3)]), ALIGN)
        for s in range(3):
            if c[s]:
                alone[s].push_aligned(cases[s][0][start[s]:start[s] + c[s]], [c[s]], cases[s][1][start[s]:start[s] + c[s]], ALIGN)
    got = fs.take([(s, i) for s in range(3) for i in range(N)]).view(3, N, 3, 40, 40)
    for s in range(3):
        assert torch.equal(got[s], alone[s].take([(0, i) for i in range(N)])) and torch.equal(got[s], cases[s][3])


def test_aligned_boxed_and_plain_pushes_alternate_and_untouched_slots_keep_their_bytes():
    frames, _ = _mod()
    clip, affines, warped, ref = _stream_case(1)
    xf = frames.FrameTransform(48, 40, train=False, max_side=64)
    boxes = [(3, 2, 30, 31)] * N
    boxed, plain = xf(clip, boxes=boxes)[0], xf(clip)[0]
    fs = frames.FrameStream(2, hold=4, max_new=2, max_side=64)
    fs.push(clip[:1], [1, 0])                              # allocates the ring
    fs.take([(0, 0)])
    fs.reset()
    fs.ring.fill_(0x5A)
    kinds = ["aligned", "boxed", "plain", "aligned", "plain", "aligned"]      # 12 frames through 8 slots of stream 1
    for t, kind in enumerate(kinds):
        i = 2 * t
        if kind == "aligned":
            fs.push_aligned(clip[i:i + 2], [0, 2], affines[i:i + 2], ALIGN)
        else:
            fs.push(clip[i:i + 2], [0, 2], boxes[i:i + 2] if kind == "boxed" else None)
        want = {"aligned": ref, "boxed": boxed, "plain": plain}[kind][i:i + 2]
        assert torch.equal(fs.take([(1, i), (1, i + 1)]), want), (t, kind)
    assert fs.frames_seen == [0, N] and bool((fs.ring[0] == 0x5A).all())      # stream 0 had no row: every slot as set
    one = frames.FrameStream(2, hold=4, max_new=2)
    one.push(clip[:1], [1, 0])
    one.reset()
    one.ring.fill_(0x5A)
    one.push_aligned(clip[:3], [1, 2], affines[:3], ALIGN)
    assert bool((one.ring[0, 1:] == 0x5A).all()) and bool((one.ring[1, 2:] == 0x5A).all())
    assert torch.equal(one.take([(0, 0), (1, 0), (1, 1)]), ref[:3])


# ---------------------------------------------------------------------------------------------- 3. NV12 and I420
@pytest.mark.parametrize("layout", yuv_ref.LAYOUTS)
def test_420_frames_equal_the_rgb_aligned_path_on_the_converted_frames(layout):
    frames, _ = _mod()
    n, h, w, align = 6, 90, 120, 21
    yuv = np.random.default_rng(77).integers(0, 256, (n, h * 3 // 2, w), dtype=np.uint8)
    rgb = yuv_ref.yuv_to_rgb(yuv, layout)
    affines = np.array(_random_affines(n, h, w, align, seed=9), np.float64)
    yuv_gpu, rgb_gpu = _on_gpu_at_an_odd_address(yuv), _on_gpu_at_an_odd_address(rgb)
    warped = torch.from_numpy(warp_all(rgb, affines, align)).cuda()
    xf_yuv, xf_rgb = frames.FrameTransform(48, 40, train=False, pixel_format=layout), frames.FrameTransform(48, 40, train=False)
    for entry in ([4, 4, 0], [8, 0, 1]):
        out, u8 = xf_yuv.aligned(yuv_gpu, affines, crop_xyf=[entry], return_u8=True, align_size=align)
        ref, ref_u8 = xf_rgb.aligned(rgb_gpu, affines, crop_xyf=[entry], return_u8=True, align_size=align)
        assert torch.equal(u8, ref_u8) and torch.equal(out, ref)
        assert torch.equal(out, xf_rgb(warped, crop_xyf=[entry]))
    fs = frames.FrameStream(1, hold=8, max_new=3, pixel_format=layout)
    for i in range(0, n, 3):
        fs.push_aligned(yuv_gpu[i:i + 3], [3], affines[i:i + 3], align)
    assert torch.equal(fs.take([(0, i) for i in range(n)]), xf_rgb(warped)[0])


# ---------------------------------------------------------------------------------------------- 4. edge cases
def test_a_one_pixel_frame_align_size_one_dyadic_coefficients_and_a_map_outside():
    frames, _ = _mod()
    xf = frames.FrameTransform(12, 8, train=False)
    rng = random.Random(3)
    # a 1 x 1 frame: every sample inside it is that pixel; half of these maps leave it
    one = torch.tensor([[[[200, 17, 99]]]], dtype=torch.uint8).expand(4, 1, 1, 3).contiguous().cuda()
    a = np.array([[0.125, 0, 0, 0, 0.125, 0], [0.25, 0, -0.5, 0, 0.25, -0.5], [1, 0, 0, 0, 1, 0], [0.05, 0.01, 0.3, -0.01, 0.05, 0.2]])
    warped = warp_all(one.cpu().numpy(), a, 8)
    assert warped[0].all() and warped[1].any() and not warped[1].all() and warped[2, 0, 0].all() and not warped[2, 1:].any()
    assert torch.equal(xf.aligned(one, a, return_u8=True, align_size=8)[1], xf(torch.from_numpy(warped).cuda(), return_u8=True)[1])
    # align_size 1: one sample per frame, resized to the whole picture
    clip, _, _ = _case(8, 33, 47, 8)
    a = np.array(_random_affines(8, 33, 47, 1, seed=2))
    warped = warp_all(clip.cpu().numpy(), a, 1)
    out, u8 = xf.aligned(clip, a, return_u8=True, align_size=1)
    assert torch.equal(u8, xf(torch.from_numpy(warped).cuda(), return_u8=True)[1]) and u8.any()
    assert bool((u8[0, :, :, :, :] == u8[0, :, :1, :1, :]).all())
    # dyadic coefficients: X and Y land exactly on 0, W, H, integers and halves
    a = np.array([[rng.randint(-8, 8) / 4 for _ in range(6)] for _ in range(8)])
    a[:, 2], a[:, 5] = [rng.randint(-47, 94) / 4 for _ in range(8)], [rng.randint(-33, 66) / 4 for _ in range(8)]
    a[0], a[1] = [1, 0, 0, 0, 1, 0], [0.5, 0, 47 - 3.75, 0, 0.5, 33 - 3.75]      # the corner; the last sample sits exactly on W, H
    warped = warp_all(clip.cpu().numpy(), a, 8)
    assert warped[0].any() and warped[2:].any() and warped[1, :7, :7].any() and not warped[1, 7].any() and not warped[1, :, 7].any()
    for size, crop in ((12, 8), (48, 40)):
        x = frames.FrameTransform(size, crop, train=False)
        out, u8 = x.aligned(clip, a, return_u8=True, align_size=8)
        ref, ref_u8 = x(torch.from_numpy(warped).cuda(), return_u8=True)
        assert torch.equal(u8, ref_u8) and torch.equal(out, ref)
    # wholly outside: the bytes of the all-zero picture
    out, u8 = xf.aligned(clip, [OUTSIDE] * 8, return_u8=True, align_size=21)
    ref, ref_u8 = xf(torch.zeros((8, 21, 21, 3), dtype=torch.uint8, device="cuda"), return_u8=True)
    assert torch.equal(u8, ref_u8) and torch.equal(out, ref) and not u8.any()


def test_affines_on_the_gpu_are_refused_and_the_state_stays():
    frames, _ = _mod()
    clip, affines, _ = _case(8, 33, 47, 8)
    fs = frames.FrameStream(1, hold=8, max_new=8)
    with pytest.raises(ValueError, match="GPU tensor"):
        fs.push_aligned(clip, [8], torch.from_numpy(affines).cuda(), 8)
    with pytest.raises(ValueError, match="GPU tensor"):
        frames.FrameTransform(12, 8, train=False).aligned(clip, torch.from_numpy(affines).cuda(), align_size=8)
    with pytest.raises(ValueError, match="align_size = 2048"):
        fs.push_aligned(clip, [8], affines, 2048)
    assert fs.frames_seen == [0] and fs.ring is None


# ---------------------------------------------------------------------------------------------- 5. tables are clamped
def test_device_tables_nobody_vetted_give_the_all_zero_picture_and_stay_inside():
    """Affines handed straight to ``ops``, on the device: NaN, +-inf and 1e300 in every position.  The restatement defines
    such a row -- every coordinate fails the inside test -- as the all-zero picture.  The packed frames sit between guard
    frames of 255, the ring and the clip outputs between sentinel slabs; row tables name streams -1 and S and positions past
    the ring.  The sane rows of the same launch keep their bits and nothing is written outside."""
    frames, ops = _mod()
    S, rf, size, crop, h, w, n, align = 2, 8, 12, 8, 33, 47, 3, 21
    slab, fb, sent = rf * crop * crop * 3, h * w * 3, 0x5A
    big_ring = torch.full(((S + 2) * slab,), sent, device="cuda", dtype=torch.uint8)
    big_in = torch.full(((n + 4) * fb,), 255, device="cuda", dtype=torch.uint8)
    ring = big_ring[slab:(S + 1) * slab].view(S, rf, crop, crop, 3)
    packed = big_in[2 * fb:(2 + n) * fb].view(n, h, w, 3)
    ring.fill_(0x33)
    clip, good, _ = _case(8, h, w, align)
    packed.copy_(clip[:n])
    nan, inf, big = float("nan"), float("inf"), 1e300
    ident = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    wild = [[nan] * 6, [inf, 0, 0, 0, 1, 0], [1, 0, -inf, 0, 1, 0], [big, big, big, big, big, big], [1, 0, 0, big, big, 0],
            [1, nan, 0, 0, 1, 0], [1, 0, 0, 0, 1, inf], [-big, 0, big, 0, 1, 0]]
    assert not warp_all(clip[0].cpu().numpy(), wild, align).any()          # what the restatement makes of them
    table =torch.tensor(wild + [ident, good[0].tolist()], dtype=torch.float64, device="cuda")
    rows = [(0, 0), (0, 1), (1, 9), (-1, 3), (S, 4), (1, 5), (0, 6), (1, 7), (0, 4), (1, 2)]      # -1 is stream 0, S is S - 1, 9 is slot 1
    slots = [(0, 0), (0, 1), (1, 1), (0, 3), (1, 4), (1, 5), (0, 6), (1, 7), (0, 4), (1, 2)]
    source = [0, 1, 2, 2, 2, 2, 2, 2, 2, 2]                               # a row past the packed input reads its last frame
    cx = torch.tensor([[size - crop + 3, -3, 1], [-2, size - crop + 5, 0]], dtype=torch.int32, device="cuda")
    entries = [[size - crop, 0, 1], [0, size - crop, 0]]                  # what the crop entries are clamped to
    geom = frames.affine_geometry(align, size)
    row_stream, row_pos = ops.stream_pair_table(rows, "cuda")
    ops.frames_stream_append_affine(packed, table, geom, size, cx, row_stream, row_pos, 5, ring)
    big_out = torch.full(((n + 2) * 3 * crop * crop,), 7.0, device="cuda")
    big_u8 = torch.full(((n + 2) * 3 * crop * crop,), sent, device="cuda", dtype=torch.uint8)
    out = big_out[3 * crop * crop:(n + 1) * 3 * crop * crop].view(n, 3, crop, crop)
    out_u8 = big_u8[3 * crop * crop:(n + 1) * 3 * crop * crop].view(n, crop, crop, 3)
    ops.frames_transform_affine(packed, table[[0, 3, 9]].contiguous(), geom, size, cx[:1].contiguous(), 3, 0.5, 0.5, out, out_u8)
    torch.cuda.synchronize()
    for guard, lo, hi, v in ((big_ring, slab, (S + 1) * slab, sent), (big_in, 2 * fb, (2 + n) * fb, 255),
                             (big_u8, 3 * crop * crop, (n + 1) * 3 * crop * crop, sent),
                             (big_out, 3 * crop * crop, (n + 1) * 3 * crop * crop, 7.0)):
        assert bool((guard[:lo] == v).all()) and bool((guard[hi:] == v).all())
    xf = frames.FrameTransform(size, crop, train=False)
    zero = torch.zeros((1, align, align, 3), dtype=torch.uint8, device="cuda")
    for i, ((s, slot), src) in enumerate(zip(slots, source)):
        if i < len(wild):
            assert not ring[s, slot].any(), (i, wild[i])                # the all-zero picture, resized: zero bytes
        else:
            a = table[i].cpu().numpy()[None]
            want = torch.from_numpy(warp_all(packed[src:src + 1].cpu().numpy(), a, align)).cuda()
            assert torch.equal(ring[s, slot], xf(want, crop_xyf=[entries[s]], return_u8=True)[1][0, 0]), i
    assert ring[0, 4].any()                                                  # the identity row: the frame's corner
    named = set(slots)
    for s in range(S):
        for slot in range(rf):
            if (s, slot) not in named:
                assert bool((ring[s, slot] == 0x33).all()), (s, slot)      # no row named them
    ref, ref_u8 = xf(zero, crop_xyf=[entries[0]], return_u8=True)
    for i in (0, 1):
        assert torch.equal(out[i], ref[0, 0]) and torch.equal(out_u8[i], ref_u8[0, 0]) and not out_u8[i].any()
    want = torch.from_numpy(warp_all(packed[2:3].cpu().numpy(), good[:1], align)).cuda()
    ref, ref_u8 = xf(want, crop_xyf=[entries[0]], return_u8=True)
    assert torch.equal(out[2], ref[0, 0]) and torch.equal(out_u8[2], ref_u8[0, 0])


# ---------------------------------------------------------------------------------------------- 6. the session
def test_session_push_aligned_equals_push_of_the_warped_faces():
    """A ``logmel`` LFAN on two ragged streams of full 64 x 56 camera frames, a new affine per frame: the logits are the bits
    ``push`` gives the faces warped beforehand, under two different chunkings of video and audio."""
    from test_live_gpu import FPS, NCLS, _cat, _model, _pcm, _raw, _ticks
    from feature_vs_text_compound_emotion_amd import live
    model, L, align = _model("logmel"), 4, 32
    raws, pcms = [_raw(L, 1), _raw(L, 2)], [_pcm(0.3, 81), _pcm(0.3, 82)]
    affines = [np.array(_random_affines(L, 64, 56, align, seed=21 + s)) for s in range(2)]
    faces = [torch.from_numpy(warp_all(r.cpu().numpy(), a, align)).cuda() for r, a in zip(raws, affines)]

    def drive(ticks, aligned):
        sess = live.AVStream(model, 2, FPS, hold=6, lead=4, max_new=2, max_samples=1024)
        out, fv, fa = [[], []], [0, 0], [0, 0]

        def collect(logits, counts):
            at = 0
            for s, c in enumerate(counts):
                out[s].append(logits[at:at + c])
                at += c

        for vc, ac in ticks:
            audio = _cat([p[f:f + c] for p, f, c in zip(pcms, fa, ac)], pcms[0]) if sum(ac) else None
            acn = ac if sum(ac) else None
            if not sum(vc):
                collect(*sess.push(None, None, audio, acn))
            elif aligned:
                video = _cat([r[f:f + c] for r, f, c in zip(raws, fv, vc)], raws[0])
                aff = np.concatenate([a[f:f + c] for a, f, c in zip(affines, fv, vc)])
                collect(*sess.push_aligned(video, vc, aff, audio, acn, align_size=align))
            else:
                collect(*sess.push(_cat([r[f:f + c] for r, f, c in zip(faces, fv, vc)], faces[0]), vc, audio, acn))
            fv, fa = [a + b for a, b in zip(fv, vc)], [a + b for a, b in zip(fa, ac)]
        collect(*sess.finish())
        return torch.stack([torch.cat(o) for o in out])

    total = pcms[0].shape[0]
    ref = drive(_ticks([L, L], [total] * 2, seed=1), aligned=False)
    assert ref.shape == (2, L, NCLS)
    for seed in (1, 2):
        assert torch.equal(drive(_ticks([L, L], [total] * 2, seed=seed), aligned=True), ref), seed
