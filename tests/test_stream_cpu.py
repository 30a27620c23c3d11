"""Streaming TCN / LFAN without a GPU: the C entry points refuse invalid descriptors before any launch, the host classes refuse
what they cannot run, and the exact cases of ``tests/test_stream_gpu.py`` meet their precondition (see ``stream_ref``)."""
import ctypes

import pytest
import torch

import stream_ref
from stream_ref import BLOCK_CASES, LIMIT


def _lib():
    from feature_vs_text_compound_emotion_amd import _lib
    from feature_vs_text_compound_emotion_amd.build import build
    build(verbose=False)
    return _lib, _lib.load()


def _desc(mod, **kw):
    base = dict(S=2, c=3, Cin=8, Cout=8, k=5, dil=2, R=16, head=5, res_C=8, res_R=16, res_head=5, out_R=16, out_head=5, slope=0.01)
    base.update(kw)
    return mod.TcnStreamDesc(**base)


def test_streaming_entry_points_are_declared_and_exported():
    import test_abi_cpu
    mod, lib = _lib()
    for name in ("cer_tcn_stream_conv", "cer_tcn_stream_append"):
        assert name in mod.exported_symbols() and name in test_abi_cpu._header_functions()
        assert getattr(ctypes.CDLL(mod.LIB_PATH), name) is not None


# a non-null pointer the library must never dereference on these paths: a host buffer, 16-byte aligned
_BUF = (ctypes.c_float * 64)()
_P = ctypes.c_void_p((ctypes.addressof(_BUF) + 15) & ~15)


@pytest.mark.parametrize("what,kw,nulls", [
    ("null ring", {}, ("ring",)),
    ("null weights", {}, ("w",)),
    ("null bias", {}, ("bias",)),
    ("no output", {}, ("out_ring", "out_dense")),
    ("R = 12 is no power of two", {"R": 12}, ()),
    ("R = 0", {"R": 0}, ()),
    ("out_R = 24 is no power of two", {"out_R": 24}, ()),
    ("head = R", {"head": 16}, ()),
    ("head < 0", {"head": -1}, ()),
    ("out_head = out_R", {"out_head": 16}, ()),
    ("res_head = res_R", {"res_head": 16}, ()),
    ("c = 9 > R - (k - 1) d = 8", {"c": 9}, ()),
    ("c = 0", {"c": 0}, ()),
    ("k = 0", {"k": 0}, ()),
    ("identity residual of another width", {"res_C": 4}, ("res_w", "res_bias")),
])
def test_conv_entry_point_refuses_invalid_descriptors_without_a_gpu(what, kw, nulls):
    mod, lib = _lib()
    args = {n: _P for n in ("ring", "w", "bias", "res_ring", "res_w", "res_bias", "out_ring", "out_dense")}
    for n in nulls:
        args[n] = None
    d = _desc(mod, **kw)
    rc = lib.cer_tcn_stream_conv(ctypes.byref(d), args["ring"], args["w"], args["bias"], args["res_ring"], args["res_w"],
                                 args["res_bias"], args["out_ring"], args["out_dense"], None)
    assert rc == -1 and b"tcn_stream_conv" in lib.cer_last_error(), what
    assert lib.cer_tcn_stream_conv(None, *([_P] * 8), None) == -1 and b"tcn_stream_conv" in lib.cer_last_error()


@pytest.mark.parametrize("what,rows,ring,s,c,ch,r,head", [
    ("null rows", None, _P, 1, 1, 4, 8, 0),
    ("null ring", _P, None, 1, 1, 4, 8, 0),
    ("R = 6 is no power of two", _P, _P, 1, 1, 4, 6, 0),
    ("head = R", _P, _P, 1, 1, 4, 8, 8),
    ("head < 0", _P, _P, 1, 1, 4, 8, -1),
    ("c = 9 > R", _P, _P, 1, 9, 4, 8, 0),
    ("S = 0", _P, _P, 0, 1, 4, 8, 0),
])
def test_append_entry_point_refuses_invalid_descriptors_without_a_gpu(what, rows, ring, s, c, ch, r, head):
    _, lib = _lib()
    assert lib.cer_tcn_stream_append(rows, ring, s, c, ch, r, head, None) == -1, what
    assert b"tcn_stream_append" in lib.cer_last_error(), what


def test_wrappers_reject_cpu_tensors():
    from feature_vs_text_compound_emotion_amd import ops
    ring = torch.zeros(1, 8, 4)
    with pytest.raises(ValueError, match="GPU"):
        ops.tcn_stream_append(torch.zeros(1, 1, 4), ring, 0)
    with pytest.raises(ValueError, match="GPU"):
        ops.tcn_stream_conv(ring, 0, 1, torch.zeros(4, 5, 4), torch.zeros(4), 5, 1, out_ring=torch.zeros(1, 8, 4))
    with pytest.raises(ValueError, match="GPU"):
        ops.pack_tcn_stream_weight(torch.zeros(4, 4, 5))


def _cpu_lfan(training=False):
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.lfan import LFAN
    m = LFAN(backbone_settings={}, output_dim=7, task="CLASSIFICATION", modality=["vggish"], example_length=4,
             tcn_channel=synth.TCN_CHANNELS, root_dir="", device="cpu")
    m.init()
    return m.train(training)


def test_public_names_are_exported_from_the_package():
    import feature_vs_text_compound_emotion_amd as pkg
    from feature_vs_text_compound_emotion_amd import streaming
    assert pkg.TCNStream is streaming.TCNStream and pkg.LFANStream is streaming.LFANStream
    assert pkg.stream_forward is streaming.stream_forward


def test_lfan_stream_on_a_cpu_model_raises():
    from feature_vs_text_compound_emotion_amd import LFANStream, TCNStream
    model = _cpu_lfan()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LFANStream(model, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TCNStream(model.temporal["vggish"], 1)


def test_lfan_stream_refuses_a_training_model_and_other_models():
    from feature_vs_text_compound_emotion_amd import LFANStream, TCNStream, synth
    from feature_vs_text_compound_emotion_amd.fusion_heads import JMT
    with pytest.raises(RuntimeError, match="train mode"):
        LFANStream(_cpu_lfan(training=True), 1)
    jmt = JMT(task="CLASSIFICATION", modalities=["video", "vggish"], tcn_settings=synth.TCN_SETTINGS, backbone_settings={},
              output_dim=7, root_dir="", device="cpu", model_name="JMT", load_backbone=False)
    with pytest.raises(TypeError, match="LFAN"):
        LFANStream(jmt.eval(), 1)
    with pytest.raises(TypeError, match="TemporalConvNet"):
        TCNStream(torch.nn.Linear(2, 2), 1)


def test_ring_length_is_the_power_of_two_that_holds_history_and_new_frames():
    from feature_vs_text_compound_emotion_amd.streaming import ring_frames
    for k, dil, max_new, want in ((5, 8, 32, 64), (5, 8, 33, 128), (5, 1, 1, 8), (5, 1, 4, 8), (5, 1, 5, 16), (1, 8, 1, 1),
                                  (1, 1, 3, 4), (2, 8, 3, 16)):
        assert ring_frames(k, dil, max_new) == want == stream_ref.ring_frames(k, dil, max_new)
        assert want >= (k - 1) * dil + max_new and (want == 1 or want // 2 < (k - 1) * dil + max_new)


def test_block_case_table_reaches_what_the_issue_lists():
    pairs = {(c.cin, c.cout) for c in BLOCK_CASES}
    assert {(5, 3), (39, 32), (128, 32), (32, 130)} <= pairs
    assert {c.k for c in BLOCK_CASES} == {1, 2, 5} and {c.dil for c in BLOCK_CASES} == {1, 8}
    assert {c.s for c in BLOCK_CASES} == {1, 3, 33} and {c.max_new for c in BLOCK_CASES} == {1, 3}
    assert {c.ds for c in BLOCK_CASES} == {True, False} and {c.mixed for c in BLOCK_CASES} == {True, False}
    assert len({c.name for c in BLOCK_CASES}) == len(BLOCK_CASES)
    for c in BLOCK_CASES:
        r = stream_ref.ring_frames(c.k, c.dil, c.max_new)
        chunks = stream_ref.chunks_of(c, stream_ref.frames_of(c))
        assert stream_ref.frames_of(c) >= 3 * r and sum(chunks) == stream_ref.frames_of(c)
        assert max(chunks) == (c.max_new if c.mixed else 1) and min(chunks) >= 1
        assert all(n <= r - (c.k - 1) * c.dil for n in chunks)


@pytest.mark.parametrize("case", BLOCK_CASES, ids=[c.name for c in BLOCK_CASES])
def test_exact_cases_meet_their_precondition(case):
    """Every intermediate of the block, in its dyadic unit, and the sum of |products| behind every output stay below 2^24:
    any fp32 summation order is exact, so the GPU test may ask for bit equality with the float64 reference."""
    d = stream_ref.make_block(case)
    assert d["x"].abs().max() <= 2 and all(d[n].abs().max() <= 1 for n in ("w1", "w2"))
    for name, v in stream_ref.exact_margins(case, d).items():
        assert v < LIMIT, (name, v)


@pytest.mark.parametrize("case", BLOCK_CASES, ids=[c.name for c in BLOCK_CASES])
def test_ring_recurrence_equals_the_whole_sequence_block(case):
    """The entry points' semantics (restated on the CPU) pushed chunk by chunk over rings that wrap at least twice return the
    whole-sequence block, exactly: in float64 and -- the values being exact -- in float32 too."""
    d = stream_ref.make_block(case)
    ref = stream_ref.block_ref(d["x"], d["w1"], d["b1"], d["w2"], d["b2"], d["dsw"], d["dsb"], case.k, case.dil)["out"]
    assert torch.equal(stream_ref.stream_block_emulated(case, d), ref)
    assert torch.equal(stream_ref.stream_block_emulated(case, d, torch.float32).double(), ref)
