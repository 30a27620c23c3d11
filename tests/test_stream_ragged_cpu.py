"""Ragged streaming (per-stream positions, the row-table entry points, ``CANStream``) without a GPU: the two new C entry points
are declared and exported and refuse invalid descriptors before any launch, ``stream_row_table`` packs rows in the documented
order, and the host classes refuse what they cannot run."""
import ctypes

import pytest
import torch

ROWS_ENTRIES = ("cer_tcn_stream_conv_rows", "cer_tcn_stream_append_rows")


def _lib():
    from feature_vs_text_compound_emotion_amd import _lib
    from feature_vs_text_compound_emotion_amd.build import build
    build(verbose=False)
    return _lib, _lib.load()


def test_row_table_entry_points_are_declared_and_exported():
    import test_abi_cpu
    mod, lib = _lib()
    for name in ROWS_ENTRIES:
        assert name in mod.exported_symbols() and name in test_abi_cpu._header_functions()
        assert getattr(ctypes.CDLL(mod.LIB_PATH), name) is not None
    text = open(test_abi_cpu.os.path.join(test_abi_cpu.ROOT, "include", "cer_hip.h")).read()
    assert "consecutive positions and must not exceed max_count" in " ".join(text.replace("*", " ").split())


def test_rows_descriptor_has_the_fields_the_header_declares():
    mod, _ = _lib()
    assert [n for n, _ in mod.TcnStreamRowsDesc._fields_] == ["S", "M", "max_count", "Cin", "Cout", "k", "dil", "R", "res_C",
                                                              "res_R", "out_R", "slope"]


# non-null pointers the library must never dereference on these paths: host buffers, 16-byte aligned / off by one float
_BUF = (ctypes.c_float * 64)()
_P = ctypes.c_void_p((ctypes.addressof(_BUF) + 15) & ~15)
_P_OFF = ctypes.c_void_p(_P.value + 4)
_POINTERS = ("row_stream", "row_pos", "ring", "w", "bias", "res_ring", "res_w", "res_bias", "out_ring", "out_dense")


def _desc(mod, **kw):
    base = dict(S=2, M=5, max_count=3, Cin=8, Cout=8, k=5, dil=2, R=16, res_C=8, res_R=16, out_R=16, slope=0.01)
    base.update(kw)
    return mod.TcnStreamRowsDesc(**base)


def _conv_rows(lib, d, args):
    return lib.cer_tcn_stream_conv_rows(ctypes.byref(d), *[args[n] for n in _POINTERS], None)


@pytest.mark.parametrize("what,kw,ptrs", [
    ("null row_stream", {}, {"row_stream": None}),
    ("null row_pos", {}, {"row_pos": None}),
    ("null ring", {}, {"ring": None}),
    ("null weights", {}, {"w": None}),
    ("null bias", {}, {"bias": None}),
    ("no output", {}, {"out_ring": None, "out_dense": None}),
    ("a projection without its bias", {}, {"res_bias": None}),
    ("M = 0", {"M": 0}, {}),
    ("M < 0", {"M": -3}, {}),
    ("R = 12 is no power of two", {"R": 12}, {}),
    ("R = 0", {"R": 0}, {}),
    ("R = 2^31 - 1 is above 2^30", {"R": 2 ** 31 - 1}, {}),
    ("out_R = 24 is no power of two", {"out_R": 24}, {}),
    ("res_R = 20 is no power of two", {"res_R": 20}, {}),
    ("(k - 1) dil + max_count = 17 > R = 16", {"max_count": 9}, {}),
    ("max_count = 3 > out_R = 2", {"out_R": 2}, {}),
    ("max_count = 3 > res_R = 2", {"res_R": 2}, {}),
    ("max_count = 0", {"max_count": 0}, {}),
    ("identity residual of another width", {"res_C": 4}, {"res_w": None, "res_bias": None}),
    ("weights off a 16-byte boundary", {}, {"w": _P_OFF}),
    ("projection weights off a 16-byte boundary", {}, {"res_w": _P_OFF}),
    ("ceil(M / 8) = 65536 tiles", {"M": 8 * 65535 + 1}, {}),
])
def test_conv_rows_refuses_invalid_descriptors_without_a_gpu(what, kw, ptrs):
    mod, lib = _lib()
    args = {n: _P for n in _POINTERS}
    args.update(ptrs)
    rc = _conv_rows(lib, _desc(mod, **kw), args)
    assert rc == -1 and b"tcn_stream_conv_rows" in lib.cer_last_error(), what


def test_conv_rows_refuses_a_null_descriptor():
    _, lib = _lib()
    assert lib.cer_tcn_stream_conv_rows(None, *([_P] * 10), None) == -1 and b"tcn_stream_conv_rows" in lib.cer_last_error()


@pytest.mark.parametrize("what,rows,ring,row_stream,row_pos,s,m,most,ch,r", [
    ("null rows", None, _P, _P, _P, 1, 1, 1, 4, 8),
    ("null ring", _P, None, _P, _P, 1, 1, 1, 4, 8),
    ("null row_stream", _P, _P, None, _P, 1, 1, 1, 4, 8),
    ("null row_pos", _P, _P, _P, None, 1, 1, 1, 4, 8),
    ("M = 0", _P, _P, _P, _P, 1, 0, 1, 4, 8),
    ("S = 0", _P, _P, _P, _P, 0, 1, 1, 4, 8),
    ("R = 6 is no power of two", _P, _P, _P, _P, 1, 1, 1, 4, 6),
    ("R = 2^31 - 1 is above 2^30", _P, _P, _P, _P, 1, 1, 1, 4, 2 ** 31 - 1),
    ("max_count = 9 > R", _P, _P, _P, _P, 1, 9, 9, 4, 8),
    ("max_count = 0", _P, _P, _P, _P, 1, 1, 0, 4, 8),
])
def test_append_rows_refuses_invalid_arguments_without_a_gpu(what, rows, ring, row_stream, row_pos, s, m, most, ch, r):
    _, lib = _lib()
    assert lib.cer_tcn_stream_append_rows(rows, ring, row_stream, row_pos, s, m, most, ch, r, None) == -1, what
    assert b"tcn_stream_append_rows" in lib.cer_last_error(), what


def test_row_table_is_stream_major_in_time_order_and_wraps_at_2_to_the_30():
    from feature_vs_text_compound_emotion_amd import ops
    row_stream, row_pos = ops.stream_row_table([5, 9, 2 ** 30 - 1], [2, 0, 3], "cpu")
    assert row_stream.dtype == torch.int32 and row_pos.dtype == torch.int32
    assert row_stream.is_contiguous() and row_pos.is_contiguous()
    assert row_stream.tolist() == [0, 0, 2, 2, 2]
    assert row_pos.tolist() == [5, 6, 2 ** 30 - 1, 0, 1]
    # a position far beyond 2^30 lands on the same slot of every ring: all ring lengths divide 2^30
    _, far = ops.stream_row_table([5 * 2 ** 30 + 77], [2], "cpu")
    assert far.tolist() == [77, 78]
    empty_s, empty_p = ops.stream_row_table([4, 4], [0, 0], "cpu")
    assert empty_s.shape == (0,) and empty_p.shape == (0,) and empty_s.dtype == torch.int32
    with pytest.raises(ValueError, match=">= 0"):
        ops.stream_row_table([0, 0], [1, -1], "cpu")
    with pytest.raises(ValueError, match=">= 0"):
        ops.stream_row_table([0, -2], [1, 1], "cpu")
    with pytest.raises(ValueError, match="positions"):
        ops.stream_row_table([0], [1, 1], "cpu")


def test_row_wrappers_reject_cpu_and_non_int32_tables():
    from feature_vs_text_compound_emotion_amd import ops
    ring, rows = torch.zeros(1, 8, 4), torch.zeros(2, 4)
    table = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU"):
        ops.tcn_stream_append_rows(rows, ring, table, table, 2)
    with pytest.raises(ValueError, match="GPU"):
        ops.tcn_stream_conv_rows(ring, table, table, 2, torch.zeros(4, 5, 4), torch.zeros(4), 5, 1, out_ring=torch.zeros(1, 8, 4))
    # the table check itself, on a stand-in for a ring that passed its own check
    for bad in (table, table.long(), table.float()):
        with pytest.raises(ValueError, match="int32 vector on the GPU"):
            ops._row_table(bad, bad, ring)


def _cpu_can(training=False, modalities=("vggish", "bert")):
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.fusion_heads import CAN
    m = CAN(task="CLASSIFICATION", modalities=list(modalities), tcn_settings=synth.TCN_SETTINGS, backbone_settings={},
            output_dim=7, root_dir="", device="cpu", load_backbone=False)
    return m.train(training)


def test_can_stream_refuses_a_training_model_a_cpu_model_and_a_jmt():
    from feature_vs_text_compound_emotion_amd import CANStream, LFANStream, stream_forward, synth
    from feature_vs_text_compound_emotion_amd.fusion_heads import JMT
    with pytest.raises(RuntimeError, match="train mode"):
        CANStream(_cpu_can(training=True), 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CANStream(_cpu_can(), 1)
    with pytest.raises(ValueError, match="encoder_batch"):
        CANStream(_cpu_can(), 1, encoder_batch=0)
    jmt = JMT(task="CLASSIFICATION", modalities=["video", "vggish"], tcn_settings=synth.TCN_SETTINGS, backbone_settings={},
              output_dim=7, root_dir="", device="cpu", model_name="JMT", load_backbone=False).eval()
    with pytest.raises(TypeError, match="CAN .JMT / MT attend over time and are not causal., got JMT"):
        CANStream(jmt, 1)
    with pytest.raises(TypeError, match="LFANStream needs an LFAN .JMT / MT attend over time and are not causal., got JMT"):
        stream_forward(jmt, {"video": torch.zeros(1, 2, 3, 8, 8), "vggish": torch.zeros(1, 1, 2, 128)})
    with pytest.raises(TypeError, match="LFAN"):
        LFANStream(_cpu_can(), 1)
    # a CAN reaches CANStream through stream_forward (and stops there: the model is on the CPU)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stream_forward(_cpu_can(), {"vggish": torch.zeros(1, 1, 2, 128), "bert": torch.zeros(1, 1, 2, 768)})


def test_new_public_names_are_exported():
    import feature_vs_text_compound_emotion_amd as pkg
    from feature_vs_text_compound_emotion_amd import ops, streaming
    assert pkg.CANStream is streaming.CANStream
    assert issubclass(streaming.CANStream, streaming._ModelStream) and issubclass(streaming.LFANStream, streaming._ModelStream)
    for name in ("push", "push_features", "push_ragged", "push_features_ragged", "reset", "frames_seen"):
        assert hasattr(streaming.CANStream, name) and hasattr(streaming.LFANStream, name), name
    assert callable(streaming.TCNStream.push_ragged) and callable(streaming.block_push_rows)
    for name in ("tcn_stream_conv_rows", "tcn_stream_append_rows", "stream_row_table"):
        assert callable(getattr(ops, name)), name


def test_counts_are_checked_on_the_host():
    from feature_vs_text_compound_emotion_amd.streaming import _check_counts
    assert _check_counts((2, 0, 8), 3, 8) == [2, 0, 8]
    for bad in ([1, 2], [1, 2, 3, 4], [1, -1, 0], [1, 9, 0], 5):
        with pytest.raises(ValueError, match="counts"):
            _check_counts(bad, 3, 8)
