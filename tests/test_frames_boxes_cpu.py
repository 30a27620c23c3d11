"""Per-frame face boxes without a GPU: what a box means (PIL's crop of an integer box, zero outside the picture, then PIL's
resize) against a fixture recorded from Pillow itself (tools/gen_golden_frames_boxes.py); the table store of the boxed kernel
against ``resample_tables`` for every side it holds; the two C entries and every refusal that must come before a launch."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from frames_box_ref import GOLDEN_BOXES, pad_slice
from helpers import golden
from oracle.frames import resize_bilinear_u8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cer_frames_transform_boxes", "cer_frames_stream_append_boxes")


def _frames():
    from feature_vs_text_compound_emotion_amd import frames
    return frames


def test_oracle_on_the_zero_padded_slice_equals_pil_crop_then_resize():
    g = golden("frames_boxes.npz")
    assert g["frame"].shape == (90, 120, 3) and [tuple(b) for b in g["boxes"].tolist()] == GOLDEN_BOXES
    for box, want in zip(GOLDEN_BOXES, g["resized"]):
        cut = pad_slice(g["frame"], box)
        assert cut.shape == (box[3] - box[1], box[2] - box[0], 3) and cut.flags["C_CONTIGUOUS"]
        assert np.array_equal(resize_bilinear_u8(cut, 48), want), box
    # numpy and torch agree on the slice, and what leaves the frame is zero
    f = g["frame"]
    assert np.array_equal(pad_slice(torch.from_numpy(f), (-7, -3, 40, 50)).numpy(), pad_slice(f, (-7, -3, 40, 50)))
    assert not pad_slice(f, (-7, -3, 40, 50))[:3].any() and not pad_slice(f, (-7, -3, 40, 50))[:, :7].any()
    assert np.array_equal(pad_slice(f, (0, 0, 120, 90)), f) and not pad_slice(f, (200, 200, 210, 215)).any()


@pytest.mark.parametrize("size,max_side", [(48, 1024), (8, 200)])
def test_table_store_rows_equal_resample_tables_for_every_side(size, max_side):
    frames = _frames()
    from feature_vs_text_compound_emotion_amd import _lib
    store = frames.box_tables(size, max_side)
    assert store is frames.box_tables(size, max_side)            # built once
    band = _lib.load().cer_frames_band_rows()
    assert store.meta.shape == (max_side + 1, 4) and store.meta.dtype == store.data.dtype == np.int32
    at = 0
    for n in range(1, max_side + 1):
        hb, hk = frames.resample_tables(n, size)
        sb, sk = store.rows(n)
        assert np.array_equal(sb, hb) and np.array_equal(sk, hk), n
        boff, koff, ks, span = (int(v) for v in store.meta[n])
        assert (boff, koff, ks) == (at, at + 2 * size, hk.shape[1]), n      # concatenated, nothing between the rows
        at = koff + size * ks
        want = max(int(hb[min(size, y0 + band) - 1].sum() - hb[y0, 0]) for y0 in range(size))
        assert span == want and 1 <= span <= n, n
        assert (hb[:, 0] >= 0).all() and (hb[:, 1] >= 1).all() and (hb.sum(1) <= n).all() and (hb[:, 1] <= ks).all()
        assert (np.diff(hb[:, 0]) >= 0).all()                                 # a band's first row is its first output's
    assert at == store.data.shape[0] and store.meta[0].tolist() == store.meta[1].tolist()
    assert store.max_rows == store.meta[1:, 3].max() and store.max_ks == store.meta[1:, 2].max()
    assert store.max_ks == 2 * -(-max_side // size) + 1
    if size == 48:
        assert [int(store.meta[n, 2]) for n in (256, 512, 1024)] == [13, 23, 45]


def test_store_is_built_by_the_first_boxed_call_only():
    frames = _frames()
    frames._BOX_TABLES.pop((48, 77), None)
    fs = frames.FrameStream(2, max_side=77)
    xf = frames.FrameTransform(48, 40, train=False, max_side=77)
    assert fs.max_side == xf.max_side == 77 and (48, 77) not in frames._BOX_TABLES
    for bad in (0, -1, 2.5, True, (1 << 20) + 1):
        with pytest.raises(ValueError, match="max_side"):
            frames.FrameStream(2, max_side=bad)


def test_both_entries_are_declared_exported_and_bound():
    from feature_vs_text_compound_emotion_amd import _lib, ops
    text = open(os.path.join(ROOT, "include", "cer_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _lib.exported_symbols() and getattr(raw, name) is not None
        assert getattr(_lib.load(), name).argtypes == _lib._SIGNATURES[name][1]
    assert callable(ops.frames_transform_boxes) and callable(ops.frames_stream_append_boxes)


def test_c_entries_refuse_before_any_launch():
    from feature_vs_text_compound_emotion_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))      # never dereferenced: every case below is refused first

    def clip(frames=p, boxes=p, meta=p, data=p, n=1, h=8, w=8, max_side=16, span=8, ks=7, size=6, crop=4, out=p, group=1):
        return lib.cer_frames_transform_boxes(frames, n, h, w, boxes, meta, data, max_side, span, ks, size, crop, p, group, 0.5, 0.5,
                                              out, None, None)

    def ring(frames=p, boxes=p, meta=p, data=p, n=1, h=8, w=8, max_side=16, span=8, ks=7, size=6, crop=4, rows=1, max_count=1,
             u8=p, s=1, rf=8):
        return lib.cer_frames_stream_append_boxes(frames, n, h, w, boxes, meta, data, max_side, span, ks, size, crop, p, p, p, rows,
                                                  max_count, u8, s, rf, None)

    shared = [({"frames": None}, b"null"), ({"boxes": None}, b"null"), ({"meta": None}, b"null"), ({"data": None}, b"null"),
              ({"crop": 7}, b"exceeds size"), ({"n": 65536}, b"65535"), ({"max_side": 0}, b"max_side"),
              ({"max_side": -3}, b"max_side"), ({"span": 17}, b"max_side"), ({"n": 0}, b">= 1"), ({"h": 0}, b">= 1"),
              # max_side 1024, size 112 -> 83 band rows, 21 taps: fits at crop 100 (checked below); 4096 rows x 112 do not
              ({"max_side": 4096, "span": 4096, "ks": 75, "size": 112, "crop": 112}, b"LDS"),
              ({"max_side": 1 << 20, "span": 300, "ks": 1 << 19, "size": 6, "crop": 4}, b"LDS")]
    for kw, text in shared + [({"out": None}, b"null"), ({"group": 0}, b">= 1")]:
        assert clip(**kw) != 0, kw
        msg = lib.cer_last_error()
        assert msg.startswith(b"frames_transform_boxes:") and text in msg, (kw, msg)
    for kw, text in shared + [({"u8": None}, b"null"), ({"rf": 6}, b"power of two"), ({"rf": 0}, b"power of two"),
                              ({"max_count": 9}, b"exceed Rf"), ({"rows": 65536}, b"65535"), ({"s": 0}, b">= 1")]:
        assert ring(**kw) != 0, kw
        msg = lib.cer_last_error()
        assert msg.startswith(b"frames_stream_append_boxes:") and text in msg, (kw, msg)


def test_lds_need_at_the_largest_supported_geometry_fits():
    """max_side = 1024, size = 112, crop = 100: the band tile [span][crop][3] bytes, the coefficient rows [crop + band][ksize]
    and the bounds [crop][2] int32 -- the expression of frames_box_lds_bytes (csrc/frames_box.hip) -- stay inside 160 KiB, and
    the need does not depend on the camera frame."""
    frames = _frames()
    from feature_vs_text_compound_emotion_amd import _lib
    band = _lib.load().cer_frames_band_rows()
    for size, crop in ((112, 100), (48, 40), (8, 6)):
        store = frames.box_tables(size, 1024)
        need = ((store.max_rows * crop * 3 + 15) & ~15) + (crop + band) * store.max_ks * 4 + crop * 2 * 4
        assert need <= 160 * 1024, (size, crop, need)
        assert store.max_rows <= 1024 and store.max_ks <= 2 * 1024 + 1


BAD_BOXES = [
    ([[0, 0, 4, 4]], "one .* per frame"),                               # one row for two frames
    ([[0, 0, 4, 4]] * 3, "one .* per frame"),
    ([[0, 0, 4], [0, 0, 4]], "one .* per frame"),                       # three columns
    ([0, 0, 4, 4, 0, 0, 4, 4], "one .* per frame"),                     # flat
    ([[0.0, 0.0, 4.0, 4.0]] * 2, "integers"),
    (np.zeros((2, 4), np.float32), "integers"),
    (torch.zeros((2, 4)), "integers"),
    (torch.zeros((2, 4), dtype=torch.bool), "integers"),
    ([[0, 0, 4, 4], [5, 0, 5, 4]], "empty"),                            # x1 == x0
    ([[0, 0, 4, 4], [5, 0, 3, 4]], "empty"),                            # x1 < x0
    ([[0, 0, 4, 4], [0, 7, 4, 7]], "empty"),                            # y1 == y0
    ([[0, 0, 4, 4], [0, 9, 4, 2]], "empty"),
    ([[0, 0, 4, 4], [0, 0, 33, 4]], "max_side = 32"),
    ([[0, 0, 4, 4], [-20, 0, 4, 33]], "max_side = 32"),
    ([[0, 0, 4, 4], [1 << 21, 0, (1 << 21) + 4, 4]], "beyond"),
]


@pytest.mark.parametrize("boxes,match", BAD_BOXES)
def test_frame_stream_refuses_bad_boxes_with_the_ints_unchanged(boxes, match):
    frames = _frames()
    fs = frames.FrameStream(2, hold=4, max_new=3, max_side=32)
    fs.frames_seen, fs.frames_taken = [3, 1], [2, 0]
    u8 = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)      # a CPU tensor: refused too, but the boxes are looked at first
    for call in (fs.check_push, fs.push):
        with pytest.raises(ValueError, match="boxes: .*" + match):
            call(u8, [1, 1], boxes)
        with pytest.raises(ValueError, match="boxes: .*" + match):
            call(u8, [1, 1], boxes=boxes)
    assert fs.frames_seen == [3, 1] and fs.frames_taken == [2, 0] and fs.ring is None
    assert (48, 32) not in frames._BOX_TABLES                # and no table store was built for a refused push


def test_good_boxes_pass_the_host_check():
    frames = _frames()
    for boxes in ([[0, 0, 32, 32], [-5, -9, 1, 1]], np.array([[0, 0, 32, 32], [-5, -9, 1, 1]], np.int16),
                  torch.tensor([[0, 0, 32, 32], [-5, -9, 1, 1]]), [(np.int64(0), 0, 32, 32), (-5, -9, 1, 1)]):
        got = frames.check_boxes(boxes, 2, 32)
        assert got.dtype == np.int32 and got.tolist() == [[0, 0, 32, 32], [-5, -9, 1, 1]]
    assert frames.check_boxes(np.zeros((2, 3, 4), np.int64) + [0, 0, 1, 1], 6, 32).shape == (6, 4)      # [B, L, 4]
    assert frames.check_boxes([], 0, 32).shape == (0, 4)
    fs = frames.FrameStream(2, hold=4, max_new=3, max_side=32)
    with pytest.raises(ValueError, match="frames: expected raw RGB frames"):      # good boxes: the CPU tensor is what is refused
        fs.push(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), [1, 1], [[0, 0, 32, 32], [-5, -9, 1, 1]])


class _Audio:
    """An audio stage that counts every call that could change its state."""
    calls = 0

    def check_push(self, *a):
        raise AssertionError("the video side is checked first")

    def push(self, *a):
        type(self).calls += 1

    finish = reset = push


@pytest.mark.parametrize("boxes,match", BAD_BOXES)
def test_session_refuses_bad_video_boxes_before_any_stage_moves(boxes, match):
    """``AVStream.push`` with the stages it checks first: a real ``FrameStream`` and an audio stage that fails the test if it is
    asked to do anything.  (The session on the GPU: tests/test_frames_boxes_gpu.py.)"""
    from feature_vs_text_compound_emotion_amd import live
    frames = _frames()
    sess = object.__new__(live.AVStream)
    sess.streams = 2
    sess.model_stream = types.SimpleNamespace(modalities=["video", "logmel"], _check_keys=lambda x: None)
    sess.frame_stream = frames.FrameStream(2, hold=4, max_new=3, max_side=32)
    sess.audio_stream = _Audio()
    sess.frames_seen, sess.examples_seen, sess.paired = [5, 0], [4, 0], [4, 0]
    sess.frame_stream.frames_seen, sess.frame_stream.frames_taken = [5, 0], [4, 0]
    u8 = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    pcm = torch.zeros(320, dtype=torch.int16)
    with pytest.raises(ValueError, match="boxes: .*" + match):
        sess.push(u8, [1, 1], pcm, [160, 160], video_boxes=boxes)
    with pytest.raises(ValueError, match="video_boxes without video"):
        sess.push(audio=pcm, audio_counts=[160, 160], video_boxes=[[0, 0, 4, 4]])
    assert _Audio.calls == 0 and sess.frame_stream.ring is None
    assert (sess.frames_seen, sess.examples_seen, sess.paired) == ([5, 0], [4, 0], [4, 0])
    assert sess.frame_stream.frames_seen == [5, 0] and sess.frame_stream.frames_taken == [4, 0]


def test_public_signatures_take_the_boxes_last():
    import inspect
    from feature_vs_text_compound_emotion_amd import live
    frames = _frames()
    assert list(inspect.signature(frames.FrameTransform.__call__).parameters) == ["self", "frames", "crop_xyf", "return_u8", "boxes"]
    assert list(inspect.signature(frames.FrameStream.push).parameters) == ["self", "frames_u8", "counts", "boxes"]
    assert list(inspect.signature(frames.FrameStream.check_push).parameters) == ["self", "frames_u8", "counts", "boxes"]
    assert list(inspect.signature(live.AVStream.push).parameters)[-1] == "video_boxes"
    assert inspect.signature(frames.FrameStream.__init__).parameters["max_side"].default == 1024
    assert inspect.signature(live.AVStream.__init__).parameters["max_side"].default == 1024


def test_row_and_box_table_is_one_upload():
    from feature_vs_text_compound_emotion_amd import ops
    boxes = np.array([[1, 2, 3, 4], [5, 6, 7, 8], [-9, -10, 11, 12]], np.int32)
    rs, rp, bx = ops.stream_row_box_table([(1 << 30) - 1, 7, 3], [2, 0, 1], boxes, "cpu")
    assert rs.tolist() == [0, 0, 2] and rp.tolist() == [(1 << 30) - 1, 0, 3] and bx.tolist() == boxes.tolist()
    assert rs.dtype == rp.dtype == bx.dtype == torch.int32 and bx.is_contiguous()
    assert rs.untyped_storage().data_ptr() == rp.untyped_storage().data_ptr() == bx.untyped_storage().data_ptr()
    want = ops.stream_row_table([(1 << 30) - 1, 7, 3], [2, 0, 1], "cpu")
    assert torch.equal(rs, want[0]) and torch.equal(rp, want[1])
    with pytest.raises(ValueError):
        ops.stream_row_box_table([0, 0], [1, 1], boxes, "cpu")
