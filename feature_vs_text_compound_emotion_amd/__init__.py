"""MI355X-native hot path for feature-based compound emotion recognition.

Host-side mirror of the reference's ``models/`` surface (LFAN & co.) on top of
libcer_hip.so -- hand-written HIP kernels for gfx950 behind the C-ABI declared
in ``include/cer_hip.h``.
"""
__version__ = "0.1.0"


def __getattr__(name):
    # the streaming interface, imported on first use (it pulls in torch and the whole host package)
    if name in ("TCNStream", "LFANStream", "CANStream", "stream_forward"):
        from . import streaming
        return getattr(streaming, name)
    if name == "LogMelStream":
        from . import audio_stream
        return audio_stream.LogMelStream
    if name in ("FrameStream", "FrameTransform", "similarity_from_landmarks", "check_affines", "ARCFACE_TEMPLATE"):
        from . import frames
        return getattr(frames, name)
    if name == "AVStream":
        from . import live
        return live.AVStream
    if name == "TextStream":
        from . import text_stream
        return text_stream.TextStream
    if name == "DecisionStream":
        from . import decisions
        return decisions.DecisionStream
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
