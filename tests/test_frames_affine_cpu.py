"""Per-frame affine maps without a GPU: what an affine means (``affine_ref``, Pillow's AFFINE transform with BILINEAR sampling
restated) against Pillow itself and against a fixture recorded from it (tools/gen_golden_frames_affine.py); the similarity fit
of five landmarks; the four C entries and every refusal that must come before a launch; the stand-alone argument-check program
under the host sanitizers.  Every comparison of bytes is for equality."""
import ctypes
import inspect
import math
import os
import random
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import affine_ref
from affine_ref import GOLDEN_AFFINES, GOLDEN_ALIGN, TEMPLATE, fit_similarity, similarity, warp_affine, warp_all
from helpers import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cer_frames_transform_affine", "cer_frames_stream_append_affine", "cer_frames_transform_affine_yuv",
           "cer_frames_stream_append_affine_yuv")


def _frames():
    from feature_vs_text_compound_emotion_amd import frames
    return frames


# ---------------------------------------------------------------------------------------------- 1. the restatement
def _cases(n, seed):
    """(frame, affine, align): frames 1 x 1 .. 90 x 90, align 1 .. 40, rotations to +-35 degrees, scales 0.3 .. 4; every
    fifth case has dyadic coefficients (multiples of 1/4: X lands exactly on 0, W, integers and halves), every seventh maps
    wholly outside the frame."""
    rng, out = random.Random(seed), []
    for i in range(n):
        h, w = (1, 1) if i == 0 else (rng.randint(1, 90), rng.randint(1, 90))
        align = 1 if i == 1 else rng.randint(1, 40)
        frame = np.random.default_rng(seed * 1000 + i).integers(0, 256, (h, w, 3), dtype=np.uint8)
        if i % 5 == 0:
            a = [rng.randint(-8, 8) / 4 for _ in range(6)]
            a[2], a[5] = rng.randint(-4 * w, 8 * w) / 4, rng.randint(-4 * h, 8 * h) / 4
            if i % 10 == 0:
                a[0], a[1], a[3], a[4] = rng.choice([0.25, 0.5, 1.0, 2.0]), 0.0, 0.0, rng.choice([0.25, 0.5, 1.0, 2.0])
        else:
            a = similarity(rng.uniform(-35, 35), rng.uniform(0.3, 4.0), rng.uniform(-0.2 * w, 1.2 * w), rng.uniform(-0.2 * h, 1.2 * h),
                           align)
        if i % 7 == 3:
            a[2] += rng.choice([-1, 1]) * (w + 5.0 * align * (abs(a[0]) + abs(a[1])) + 3)
        out.append((frame, a, align))
    return out


def test_restatement_equals_pillow():
    from PIL import Image
    cases = _cases(140, seed=11)
    assert cases[0][0].shape == (1, 1, 3) and cases[1][2] == 1
    differ = total = outside = touched = 0
    for frame, a, align in cases:
        want = np.asarray(Image.fromarray(frame).transform((align, align), Image.AFFINE, tuple(a), resample=Image.BILINEAR))
        got = warp_affine(frame, a, align)
        assert got.shape == want.shape == (align, align, 3) and got.dtype == np.uint8
        differ += int((got != want).sum())
        total += want.size
        outside += not want.any()
        touched += bool(want.any())
    assert differ == 0, (differ, total)
    assert total > 100000 and outside >= 10 and touched >= 80      # both kinds of map were in the draw


def test_restatement_equals_the_pillow_fixture():
    g = golden("frames_affine.npz")
    assert g["frame"].shape == (90, 120, 3) and int(g["align"][0]) == GOLDEN_ALIGN == 32
    assert np.array_equal(g["affines"], np.array(GOLDEN_AFFINES, np.float64))
    assert g["warped"].shape == (len(GOLDEN_AFFINES), 32, 32, 3)
    assert np.array_equal(warp_all(g["frame"], g["affines"], 32), g["warped"])
    assert np.array_equal(g["warped"][0], g["frame"][:32, :32])                  # the identity
    assert not g["warped"][-1].any() and all(w.any() for w in g["warped"][:-1])   # the map wholly outside
    assert not g["warped"][3].all(axis=2).all()                                   # the rotation that leaves the frame


def test_non_finite_and_huge_coefficients_are_outside():
    frame = np.full((5, 7, 3), 200, np.uint8)
    for bad in (float("nan"), float("inf"), -float("inf"), 1e300, -1e300):
        for i in range(6):
            a = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
            a[i] = bad
            out = warp_affine(frame, a, 4)
            assert out.shape == (4, 4, 3) and not out.any(), (bad, i)
    assert warp_affine(frame, [1.0, 0.0, 0.0, 0.0, 1.0, 0.0], 4).all()


# ---------------------------------------------------------------------------------------------- 2. the similarity fit
def _known(angle, scale, tx, ty):
    """(a, b, tx, ty) of u = a x - b y + tx, v = b x + a y + ty."""
    return scale * math.cos(math.radians(angle)), scale * math.sin(math.radians(angle)), tx, ty


@pytest.mark.parametrize("align", [112, 256, 32])
def test_landmarks_made_from_a_known_similarity_are_recovered(align):
    frames = _frames()
    q = TEMPLATE * align / 112.0
    rng, lm, want = random.Random(align), [], []
    for _ in range(12):
        a, b, tx, ty = _known(rng.uniform(-60, 60), rng.uniform(0.2, 3.0), rng.uniform(-300, 300), rng.uniform(-300, 300))
        s = a * a + b * b
        # the landmarks whose image under the forward map is the template: p = A^-1 (q - t)
        u, v = q[:, 0] - tx, q[:, 1] - ty
        lm.append(np.stack([(a * u + b * v) / s, (-b * u + a * v) / s], axis=1))
        ia, ib, itx, ity = a / s, b / s, -(a * tx + b * ty) / s, -(-b * tx + a * ty) / s
        want.append([ia, ib, itx - 0.5 * (ia + ib) + 0.5, -ib, ia, ity - 0.5 * (-ib + ia) + 0.5])
    got = frames.similarity_from_landmarks(np.stack(lm), align)
    assert got.shape == (12, 6) and got.dtype == np.float64
    assert np.abs(got - np.array(want)).max() <= 1e-9
    assert np.abs(got - np.stack([fit_similarity(p, align) for p in lm])).max() <= 1e-9      # the restated fit agrees
    assert np.array_equal(frames.similarity_from_landmarks(lm[3], align), got[3:4])          # one face, [5, 2]


def test_template_landmarks_give_the_identity_at_112():
    frames = _frames()
    assert np.array_equal(np.array(frames.ARCFACE_TEMPLATE), TEMPLATE)
    got = frames.similarity_from_landmarks(TEMPLATE[None], 112)
    assert np.abs(got - np.array([[1.0, 0, 0, 0, 1.0, 0]])).max() <= 1e-9
    # at 256 the same landmarks are a pure magnification by 256 / 112 about the half-pixel origin
    k = 112.0 / 256.0
    got = frames.similarity_from_landmarks(TEMPLATE[None], 256)
    assert np.abs(got - np.array([[k, 0, -0.5 * k + 0.5, 0, k, -0.5 * k + 0.5]])).max() <= 1e-9
    assert inspect.signature(frames.similarity_from_landmarks).parameters["align_size"].default == 256


def test_half_pixel_conversion_follows_the_formula():
    """u = A x + t between integer pixel centres; Pillow evaluates A' (x + 0.5) + t' and reads centres at + 0.5: the two agree
    on every pixel when a2 = t_x - 0.5 (a0 + a1) + 0.5, a5 likewise."""
    frames = _frames()
    rng = random.Random(5)
    a, b, tx, ty = _known(21.0, 1.7, 40.0, -12.0)
    s = a * a + b * b
    q = TEMPLATE * 64 / 112.0
    u, v = q[:, 0] - tx, q[:, 1] - ty
    lm = np.stack([(a * u + b * v) / s, (-b * u + a * v) / s], axis=1)
    c = frames.similarity_from_landmarks(lm, 64)[0]
    for _ in range(20):
        x, y = rng.randint(0, 63), rng.randint(0, 63)
        # where output pixel centre (x, y) comes from under the inverse of the fitted map, in integer-centre coordinates
        src = ((a * (x - tx) + b * (y - ty)) / s, (-b * (x - tx) + a * (y - ty)) / s)
        X = c[0] * (x + 0.5) + c[1] * (y + 0.5) + c[2] - 0.5
        Y = c[3] * (x + 0.5) + c[4] * (y + 0.5) + c[5] - 0.5
        assert abs(X - src[0]) <= 1e-9 and abs(Y - src[1]) <= 1e-9


def test_degenerate_and_malformed_landmarks_are_refused():
    frames = _frames()
    with pytest.raises(ValueError, match="coincide"):
        frames.similarity_from_landmarks([[[3.0, 4.0]] * 5])
    with pytest.raises(ValueError, match="coincide"):
        frames.similarity_from_landmarks(np.stack([TEMPLATE, np.full((5, 2), 7.0)]))
    for bad in (np.zeros((2, 4, 2)), np.zeros((5, 3)), np.zeros(10)):
        with pytest.raises(ValueError, match="five"):
            frames.similarity_from_landmarks(bad)
    with pytest.raises(ValueError, match="finite"):
        frames.similarity_from_landmarks(np.where(np.arange(10).reshape(5, 2) == 3, np.nan, TEMPLATE))
    for bad in (0, -1, 2.5, True, (1 << 14) + 1):
        with pytest.raises(ValueError, match="align_size"):
            frames.similarity_from_landmarks(TEMPLATE, bad)


# ---------------------------------------------------------------------------------------------- 3. C entries
def test_the_four_entries_are_declared_exported_and_bound():
    from feature_vs_text_compound_emotion_amd import _lib, ops
    import feature_vs_text_compound_emotion_amd as pkg
    text = open(os.path.join(ROOT, "include", "cer_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _lib.exported_symbols() and getattr(raw, name) is not None
        assert getattr(_lib.load(), name).argtypes == _lib._SIGNATURES[name][1]
    assert callable(ops.frames_transform_affine) and callable(ops.frames_stream_append_affine)
    frames = _frames()
    assert pkg.similarity_from_landmarks is frames.similarity_from_landmarks and pkg.check_affines is frames.check_affines
    assert pkg.FrameTransform is frames.FrameTransform and pkg.ARCFACE_TEMPLATE is frames.ARCFACE_TEMPLATE


def test_c_entries_refuse_before_any_launch():
    from feature_vs_text_compound_emotion_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64 + 16)
    base = (ctypes.addressof(buf) + 15) & ~15
    p = ctypes.c_void_p(base)      # never dereferenced: every case below is refused first
    desc = _lib.Yuv420Desc(_lib.YUV_NV12, 19077, 26149, -6419, -13320, 33050, 16)

    def clip(name, how, frames=p, affines=p, bounds=p, coef=p, n=1, h=8, w=8, ks=3, align=8, span=8, size=6, crop=4, out=p, group=1,
             **_):
        return getattr(lib, name)(frames, *how, n, h, w, affines, bounds, coef, ks, align, span, size, crop, p, group, 0.5, 0.5, out,
                                  None, None)

    def ring(name, how, frames=p, affines=p, bounds=p, coef=p, n=1, h=8, w=8, ks=3, align=8, span=8, size=6, crop=4, rows=1,
             max_count=1, u8=p, s=1, rf=8, **_):
        return getattr(lib, name)(frames, *how, n, h, w, affines, bounds, coef, ks, align, span, size, crop, p, p, p, rows, max_count,
                                  u8, s, rf, None)

    shared = [({"frames": None}, b"null"), ({"affines": None}, b"null"), ({"bounds": None}, b"null"), ({"coef": None}, b"null"),
              ({"affines": ctypes.c_void_p(base + 4)}, b"8-byte aligned"),
              ({"crop": 7}, b"exceeds size"), ({"n": 65536, "rows": 65536}, b"65535"), ({"n": 0}, b">= 1"), ({"rows": 0, "n": 0}, b">= 1"),
              ({"rows": -1, "n": -1}, b">= 1"),
              ({"align": 0}, b"align_size"), ({"align": -3}, b"align_size"), ({"span": 9}, b"align_size"), ({"ks": 20}, b"align_size"),
              # 2048 -> 48: 87 taps and 430 band rows of 2048 pixels are 2.6 MB; 256 -> 48 fits (checked below)
              ({"align": 2048, "span": 430, "ks": 87, "size": 48, "crop": 40}, b"align_size = 2048"),
              ({"align": 2048, "span": 430, "ks": 87, "size": 48, "crop": 40}, b"LDS")]
    rgb_only = [({"h": 0}, b">= 1"), ({"w": 0}, b">= 1")]
    yuv_only = [({"h": 7}, b"even"), ({"w": 0}, b"even")]
    for name in ENTRIES:
        is_ring, is_yuv = "stream_append" in name, name.endswith("_yuv")
        call, how = (ring if is_ring else clip), ((ctypes.byref(desc),) if is_yuv else ())
        own = [({"u8": None}, b"null"), ({"rf": 6}, b"power of two"), ({"rf": 0}, b"power of two"), ({"max_count": 9}, b"exceed Rf"),
               ({"s": 0}, b">= 1")] if is_ring else [({"out": None}, b"null"), ({"group": 0}, b">= 1")]
        for kw, text in shared + own + (yuv_only if is_yuv else rgb_only):
            assert call(name, how, **kw) != 0, (name, kw)
            msg = lib.cer_last_error()
            assert msg.startswith(name[4:].encode() + b":") and text in msg, (name, kw, msg)
        if is_yuv:
            assert call(name, (None,)) != 0 and lib.cer_last_error().startswith(name[4:].encode() + b": null")


def test_lds_need_is_bounded_by_the_geometry_and_the_default_fits():
    frames = _frames()
    from feature_vs_text_compound_emotion_amd import _lib
    band = _lib.load().cer_frames_band_rows()
    g = frames.affine_geometry(256, 48)
    assert g is frames.affine_geometry(256, 48) and (g.ks, g.align_size, g.size) == (13, 256, 48)
    hb, hk = frames.resample_tables(256, 48)
    assert np.array_equal(g.bounds, hb) and np.array_equal(g.coef, hk)
    assert g.span == max(int(hb[min(48, y0 + band) - 1].sum() - hb[y0, 0]) for y0 in range(48))
    need = ((g.span * 256 * 3 + 15) & ~15) + ((g.span * 40 * 3 + 15) & ~15) + (40 + band) * 13 * 4 + 40 * 2 * 4
    assert g.lds_bytes(40) == need <= 64 * 1024
    g.check_crop(40)
    for align, size, crop in ((8, 12, 8), (21, 48, 40), (32, 12, 8), (1, 48, 40), (384, 48, 40)):
        frames.affine_geometry(align, size).check_crop(crop)
    with pytest.raises(ValueError, match="align_size = 2048.*LDS"):
        frames.affine_geometry(2048, 48).check_crop(40)


# ---------------------------------------------------------------------------------------------- 4. host refusals
GOOD = [[1.0, 0.0, 0.0, 0.0, 1.0, 0.0], [0.5, 0.1, 3.0, -0.1, 0.5, 2.0]]
BAD_AFFINES = [
    ([GOOD[0]], "per frame"),                                            # one row for two frames
    (GOOD + GOOD[:1], "per frame"),
    ([[1.0, 0.0, 0.0, 0.0, 1.0]] * 2, "per frame"),                      # five columns
    (sum(GOOD, []), "per frame"),                                        # flat
    ([GOOD[0], [1.0, 0.0, float("nan"), 0.0, 1.0, 0.0]], "not finite"),
    ([[float("inf"), 0.0, 0.0, 0.0, 1.0, 0.0], GOOD[1]], "not finite"),
    (np.array([GOOD[0], [1.0, 0.0, 0.0, 0.0, -np.inf, 0.0]]), "not finite"),
    (torch.tensor([GOOD[0], [1.0, 0.0, 0.0, float("nan"), 1.0, 0.0]], dtype=torch.float64), "not finite"),
    (np.zeros((2, 6), np.complex128), "real numbers"),
    (torch.zeros((2, 6), dtype=torch.bool), "real numbers"),
    ([["a"] * 6] * 2, "real numbers"),
]


@pytest.mark.parametrize("affines,match", BAD_AFFINES)
def test_frame_stream_refuses_bad_affines_with_the_ints_unchanged(affines, match):
    frames = _frames()
    fs = frames.FrameStream(2, hold=4, max_new=3)
    fs.frames_seen, fs.frames_taken = [3, 1], [2, 0]
    u8 = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)      # a CPU tensor: refused too, but the affines are looked at first
    for call in (fs.check_push_aligned, fs.push_aligned):
        with pytest.raises(ValueError, match="affines: .*" + match):
            call(u8, [1, 1], affines)
        with pytest.raises(ValueError, match="affines: .*" + match):
            call(u8, [1, 1], affines=affines, align_size=32)
    assert fs.frames_seen == [3, 1] and fs.frames_taken == [2, 0] and fs.ring is None
    xf = frames.FrameTransform(48, 40, train=False)
    with pytest.raises(ValueError, match="affines: .*" + match):
        xf.aligned(u8, affines)


def test_affines_on_the_gpu_are_refused_without_looking_at_them(monkeypatch):
    """A GPU tensor cannot be checked without a synchronisation; ``is_cuda`` is all that is asked of it.  (A real one:
    tests/test_frames_affine_gpu.py.)"""
    frames = _frames()
    fake = types.SimpleNamespace(is_cuda=True)
    orig = torch.is_tensor
    monkeypatch.setattr(torch, "is_tensor", lambda x: x is fake or orig(x))
    fs = frames.FrameStream(2, hold=4, max_new=3)
    for call in (lambda: frames.check_affines(fake, 2), lambda: fs.push_aligned(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), [1, 1], fake)):
        with pytest.raises(ValueError, match="affines: .*GPU tensor"):
            call()
    assert fs.frames_seen == [0, 0] and fs.ring is None


def test_good_affines_pass_the_host_check_and_the_frames_are_refused_next():
    frames = _frames()
    for affines in (GOOD, np.array(GOOD, np.float32).astype(np.float64), torch.tensor(GOOD, dtype=torch.float64),
                    [tuple(GOOD[0]), np.array(GOOD[1])], [[1, 0, 0, 0, 1, 0], GOOD[1]]):
        got = frames.check_affines(affines, 2)
        assert got.dtype == np.float64 and got.shape == (2, 6) and got.flags["C_CONTIGUOUS"]
        assert got[1].tolist() == pytest.approx(GOOD[1]) and got[0].tolist() == GOOD[0]
    assert frames.check_affines(np.zeros((2, 3, 6)), 6).shape == (6, 6)      # [B, L, 6]
    assert frames.check_affines([], 0).shape == (0, 6)
    fs = frames.FrameStream(2, hold=4, max_new=3)
    with pytest.raises(ValueError, match="frames: expected raw RGB frames"):      # good affines: the CPU tensor is refused
        fs.push_aligned(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), [1, 1], GOOD)
    with pytest.raises(ValueError, match="counts"):
        fs.push_aligned(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), [1, 4], GOOD)
    for bad in (0, -2, 2.5, True, 1 << 15):
        with pytest.raises(ValueError, match="align_size"):
            fs.push_aligned(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), [1, 1], GOOD, align_size=bad)
    with pytest.raises(ValueError, match="align_size = 2048.*LDS"):
        fs.check_push_aligned(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), [1, 1], GOOD, 2048)
    assert fs.frames_seen == [0, 0] and fs.ring is None
    xf = frames.FrameTransform(48, 40, train=False)
    with pytest.raises((RuntimeError, ValueError), match="CUDA|GPU"):              # CPU frames, good affines
        xf.aligned(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), GOOD)
    with pytest.raises(ValueError, match="align_size = 2048.*LDS"):
        xf.aligned(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), GOOD, align_size=2048)


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_odd_sized_420_pictures_are_refused(fmt):
    frames = _frames()
    fs = frames.FrameStream(2, hold=4, max_new=3, pixel_format=fmt)
    xf = frames.FrameTransform(48, 40, train=False, pixel_format=fmt)
    for shape, match in (((2, 10, 8), "rows are not"), ((2, 12, 7), "even W"), ((2, 12, 8, 3), "uint8 tensor")):
        with pytest.raises(ValueError, match=match):
            fs.push_aligned(torch.zeros(shape, dtype=torch.uint8), [1, 1], GOOD)
        if len(shape) == 3:
            with pytest.raises(ValueError, match=match):
                xf.aligned(torch.zeros(shape, dtype=torch.uint8), GOOD)
    with pytest.raises(ValueError, match="must be on the GPU"):
        xf.aligned(torch.zeros((2, 12, 8), dtype=torch.uint8), GOOD)
    with pytest.raises(ValueError, match="must be on the GPU"):
        fs.push_aligned(torch.zeros((2, 12, 8), dtype=torch.uint8), [1, 1], GOOD)
    assert fs.frames_seen == [0, 0] and fs.ring is None


class _Audio:
    """An audio stage that counts every call that could change its state."""
    calls = 0

    def check_push(self, *a):
        raise AssertionError("the video side is checked first")

    def push(self, *a):
        type(self).calls += 1

    finish = reset = push


def _session():
    from feature_vs_text_compound_emotion_amd import live
    frames = _frames()
    sess = object.__new__(live.AVStream)
    sess.streams = 2
    sess.model_stream = types.SimpleNamespace(modalities=["video", "logmel"], _check_keys=lambda x: None)
    sess.frame_stream = frames.FrameStream(2, hold=4, max_new=3)
    sess.audio_stream = _Audio()
    sess.frames_seen, sess.examples_seen, sess.paired = [5, 0], [4, 0], [4, 0]
    sess.frame_stream.frames_seen, sess.frame_stream.frames_taken = [5, 0], [4, 0]
    return sess


@pytest.mark.parametrize("affines,match", BAD_AFFINES[:6])
def test_session_refuses_bad_video_affines_before_any_stage_moves(affines, match):
    sess = _session()
    u8, pcm = torch.zeros((2, 8, 8, 3), dtype=torch.uint8), torch.zeros(320, dtype=torch.int16)
    with pytest.raises(ValueError, match="affines: .*" + match):
        sess.push_aligned(u8, [1, 1], affines, pcm, [160, 160])
    with pytest.raises(ValueError, match="video_affines without video"):
        sess.push_aligned(None, None, GOOD, audio=pcm, audio_counts=[160, 160])
    with pytest.raises(ValueError, match="come together"):
        sess.push_aligned(u8, None, GOOD, pcm, [160, 160])
    with pytest.raises(ValueError, match="frames: expected raw RGB frames"):       # good affines, CPU frames
        sess.push_aligned(u8, [1, 1], GOOD, pcm, [160, 160])
    assert _Audio.calls == 0 and sess.frame_stream.ring is None
    assert (sess.frames_seen, sess.examples_seen, sess.paired) == ([5, 0], [4, 0], [4, 0])
    assert sess.frame_stream.frames_seen == [5, 0] and sess.frame_stream.frames_taken == [4, 0]


def test_public_signatures():
    from feature_vs_text_compound_emotion_amd import live
    frames = _frames()
    sig = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    assert sig(frames.FrameTransform.aligned) == ["self", "frames", "affines", "crop_xyf", "return_u8", "align_size"]
    assert sig(frames.FrameStream.push_aligned) == ["self", "frames_u8", "counts", "affines", "align_size"]
    assert sig(frames.FrameStream.check_push_aligned) == ["self", "frames_u8", "counts", "affines", "align_size"]
    assert sig(live.AVStream.push_aligned) == ["self", "video", "video_counts", "video_affines", "audio", "audio_counts", "extra",
                                               "align_size"]
    for f in (frames.FrameTransform.aligned, frames.FrameStream.push_aligned, live.AVStream.push_aligned):
        assert inspect.signature(f).parameters["align_size"].default == 256
    # the two kinds of session push share one body: neither touches a stage itself
    for f in (live.AVStream.push, live.AVStream.push_aligned):
        src = inspect.getsource(f)
        assert "self._push(" in src and "audio_stream" not in src and "_emit" not in src


def test_row_and_affine_table_is_one_upload():
    from feature_vs_text_compound_emotion_amd import ops
    aff = np.array([[1.5, 0.25, -3.0, -0.25, 1.5, 7.0], [0.1, 0.2, 0.3, 0.4, 0.5, 0.6], [1e-300, -1e300, 0, 1, 2, 3]], np.float64)
    for counts, first in (([2, 0, 1], [(1 << 30) - 1, 7, 3]), ([1, 1, 1], [0, 0, 0])):
        rs, rp, af = ops.stream_row_affine_table(first, counts, aff, "cpu")
        want = ops.stream_row_table(first, counts, "cpu")
        assert torch.equal(rs, want[0]) and torch.equal(rp, want[1])
        assert af.dtype == torch.float64 and af.shape == (3, 6) and af.is_contiguous() and np.array_equal(af.numpy(), aff)
        assert rs.dtype == rp.dtype == torch.int32
        assert rs.untyped_storage().data_ptr() == rp.untyped_storage().data_ptr() == af.untyped_storage().data_ptr()
        assert af.data_ptr() % 8 == 0 and af.data_ptr() == af.untyped_storage().data_ptr()      # the doubles lead the upload
    with pytest.raises(ValueError):
        ops.stream_row_affine_table([0, 0], [1, 1], aff, "cpu")


# ---------------------------------------------------------------------------------------------- 5. the stand-alone program
def test_stand_alone_argument_checks_run_clean_under_the_host_sanitizers(tmp_path):
    """tools/frames_affine_args_check.cpp has its own ``main`` and calls the four entries with bad arguments; compiled with
    the kernels' translation unit and the error recorder under AddressSanitizer and UndefinedBehaviorSanitizer on the host
    side only, and run here as a program of its own.  No GPU is touched: every call is refused first."""
    from feature_vs_text_compound_emotion_amd import build
    csrc = os.path.join(ROOT, "feature_vs_text_compound_emotion_amd", "csrc")
    exe = str(tmp_path / "frames_affine_args_check")
    cmd = [build.HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tools", "frames_affine_args_check.cpp"), os.path.join(csrc, "frames_affine.hip"),
           os.path.join(csrc, "cer_common.hip"), "-o", exe]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and re.search(r"^ok: \d+ refusals$", run.stdout, flags=re.M), (run.stdout[-2000:], run.stderr[-2000:])
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-2000:]
