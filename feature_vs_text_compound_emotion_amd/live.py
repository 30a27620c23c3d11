"""Live audio-visual sessions: raw camera frames and raw PCM of S independent streams in, logits out.

``AVStream`` owns the three streamed stages and pairs them: a ``FrameStream`` (raw uint8 frames -> the cropped bytes, held on
the device), a ``LogMelStream`` (PCM at any rate -> VGGish examples, hop 1 / fps) and an ``LFANStream`` or ``CANStream``.  Example
e belongs to video frame e but is complete only 0.975 s after that frame's time, so frames wait on the device for their
examples; when the video side lags, examples wait for their frames.  Every stage is bit-identical to its offline counterpart
and the holds copy bits, so the logits of a stream are the bits ``stream_forward`` gives the offline-prepared clip, under any
chunking of either side and any number of neighbouring streams.

The pairing rule (``pair_schedule``, a pure function of ints).  A stream has F frames pushed, E examples emitted, P pairs
emitted.  After every push, frames P .. min(F, E) - 1 are emitted, frame i with example i.  When the stream ends, the audio
stage brings E to its final n (the reference's count for the padded signal) and frames P .. F - 1 are emitted with example
min(i, n - 1): later frames repeat the last example and examples >= F are dropped, which is ``use = min(n, L)`` and "repeat the
last row" of ``MultimodalFeatureExtractor.audio_features``.

State.  Host: the three ints per stream.  Device: the ``FrameStream`` ring [S, Rf, crop, crop, 3] uint8; an example ring
[S, Re, win * 64] float32; one ring [S, Rf, E_m] float32 per further modality (``bert`` rows that come with the frames and wait
as long as they do, or, with a text leg, the rows a ``TextStream`` made of finished sentences, see the class text).  The
float rings are written with ``ops.tcn_stream_append_rows`` and read with ``ops.gather_rows``: no kernel of their own.
Rf = ``hold_ring(hold, max_new)``: at most ``hold`` frames wait when a push brings at most ``max_new``.
Re = ``hold_ring(lead, examples_per_step(...))``: at most ``lead`` examples wait when a push completes at most
``examples_per_step`` new ones (``hold + lead`` with a text leg).  Example e sits in slot e mod Re; a stream's last example
stays in its slot until the stream is reset.

Examples per step.  A push (or one padding step of the audio stage's ``finish``) adds at most ``max_out`` 16 kHz samples to a
stream (``max_samples``, or the resampler's ``max_outputs``), hence at most r = max_out // 160 + 1 STFT rows.  Example e
becomes complete when round(hop e) + win <= rows, so the new ones have round(hop e) in an integer interval of length r, hop e
in a real interval of length at most r + 1, and there are at most floor((r + 1) / hop) + 1 of them (hop in rows, >= 1).
"""
import torch

from . import ops
from .audio_stream import ROW_HOP, LogMelStream
from .feature_stats import as_standardizer
from .frames import FrameStream, hold_ring, takes_layout
from .fusion_heads import CAN, JMT
from .lfan import LFAN
from .streaming import CANStream, LFANStream

AUDIO_KEYS = ("logmel", "vggish")


def pair_schedule(frames, examples, paired, final=None):
    """The (frame, example) pairs a stream with ``frames`` frames pushed, ``examples`` examples emitted and ``paired`` pairs
    emitted owes now.  ``final``: the stream has ended with that many examples in all (0: it never received a sample, and
    its frames are dropped).  Python ints, no GPU."""
    if final is None:
        return [(i, i) for i in range(paired, min(frames, examples))]
    return [(i, min(i, final - 1)) for i in range(paired, frames)] if final > 0 else []


def pair_schedule_text(frames, examples, text, paired, final=None):
    """``pair_schedule`` for a session with a text leg: ``text`` is the number of frames whose text row is final.  Before the
    end a frame is emitted once its example AND its text row exist: frames paired .. min(frames, examples, text) - 1.  At the
    end (``final``) the session first advances the text to ``frames`` with zero rows (a frame whose sentence never came has no
    word), so nothing waits for text any more and the pairs are ``pair_schedule``'s.  Python ints, no GPU."""
    if final is None:
        return pair_schedule(min(frames, text), examples, paired)
    return pair_schedule(frames, examples, paired, final=final)


def check_text_waiting(text_seen, new, paired, ring_frames):
    """What ``AVStream.push_text`` refuses for one stream, as ints: the text rows of frames ``paired`` .. ``text_seen + new``
    - 1 wait in a ring of ``ring_frames`` slots (slot = frame number masked), so text may not run further ahead of the pairing
    than the ring holds.  Returns the rows that wait after the call, before pairing."""
    waiting = text_seen + new - paired
    if waiting > ring_frames:
        raise ValueError(f"{text_seen - paired} text rows wait for their frames and {new} more exceed the ring of {ring_frames}")
    return waiting


def examples_per_step(max_out, hop_frames):
    """The most examples that ``max_out`` new 16 kHz samples of one stream can complete (derivation in the module text)."""
    return int((max_out // ROW_HOP + 2) / hop_frames) + 1


def check_waiting(frames, examples, paired, new_frames, examples_after, hold, lead):
    """What ``AVStream.push`` refuses for one stream, as ints: the frames that wait plus the new ones (they count as waiting
    until the call has paired them) may not exceed ``hold``; the examples still ahead of their frames after the push may not
    exceed ``lead``.  Returns (frames waiting before pairing, examples waiting after it)."""
    waiting_frames = frames - paired + new_frames
    waiting_examples = max(examples_after - (frames + new_frames), 0)
    if waiting_frames > hold:
        raise ValueError(f"{frames - paired} frames wait for their audio and {new_frames} more exceed hold = {hold}")
    if waiting_examples > lead:
        raise ValueError(f"{waiting_examples} examples would wait for their frames, more than lead = {lead}")
    return waiting_frames, waiting_examples


class AVStream:
    """An eval-mode LFAN or CAN on ``streams`` live audio-visual streams at ``fps`` frames per second.

      push(video=None, video_counts=None, audio=None, audio_counts=None, extra=None, video_boxes=None)
            video [M, H, W, 3] uint8 raw frames, ``video_counts[s]`` (0 .. max_new) of stream s, packed stream-major; audio
            int16 PCM as ``LogMelStream.push`` takes it with ``audio_counts``; either side may be absent.  ``extra[m]``
            [M, embedding_dim[m]] float32: the rows of every further modality of the model (``bert``) for the new frames.
            ``video_boxes`` [M, 4] host integers: ``video`` holds full camera frames and frame m is cropped to its face box
            (x0, y0, x1, y1) first, as ``FrameStream.push(..., boxes=)`` does (sides up to ``max_side``).  A session built
            with ``video_format="nv12"`` or ``"i420"`` (and ``video_matrix``, ``video_range``: ``FrameStream``'s
            ``pixel_format``, ``matrix``, ``range``) takes the decoder's 4:2:0 frames instead, uint8 [M, H * 3 / 2, W]; with
            ``"bgr24"``, ``"rgba32"``, ``"bgra32"``, ``"yuyv422"`` or ``"uyvy422"`` what a capture API hands out, [M, H, W, C].
            ``video_layout=`` (keyword, on ``push_aligned`` too): the ``frames.surface_layout`` of this push's frames, a
            pitched or padded surface read in place as ``FrameStream.push(..., layout=)`` reads it; a refused layout changes
            no stage's state.
            -> (logits [P, n_cls], counts): every frame that became paired in this call, stream-major, each stream's frames in
            time order (the row order of ``push_ragged``); counts[s] of them belong to stream s.  Nothing paired: an empty
            [0, n_cls] and no model launch.
      push_aligned(video, video_counts, video_affines, audio=None, audio_counts=None, extra=None, align_size=256)
            ``push`` of full camera frames with one affine map per frame, ``video_affines`` [M, 6] host float64
            (``frames.similarity_from_landmarks`` of the detector's five landmarks): frame m is warped to an ``align_size``
            face first, as ``FrameStream.push_aligned`` does.  The two share one body and may alternate.
      finish(streams=None)   the streams have ended: the same pair for their remaining frames (the audio stage's one second of
            edge padding, the last example repeated, examples past the last frame dropped); those streams are reset.  A stream
            that received frames but never a sample emits nothing for them.
      reset(streams=None)    forget those streams.
      push_text(sentences, upto=None)   with ``text=``: finished sentences with their frame spans, as ``TextStream.push`` takes
            them -> (logits, counts) like ``push``: text arriving can release frames that were waiting for it.
      frames_seen, examples_seen, paired, emitted   host lists, one int per stream; with ``text=`` also text_seen.
      decisions              with ``decisions=`` (a dict of ``DecisionStream`` keyword arguments, ``{}`` for the defaults): a
            ``DecisionStream`` the session owns and feeds every logit row it emits, in ``push`` and in ``finish``;
            ``av.decisions.decide()`` gives the running video-level decisions.  ``finish`` leaves a stream's decisions
            standing, to be read; they are forgotten by ``reset``, or when that stream emits its next row.  Its ``max_new``
            defaults to the session's and may not be smaller, so it refuses nothing the session emits: what it does refuse
            (its own arguments) it refuses here, at construction.

    The model's modalities must contain ``video`` and exactly one of ``logmel`` / ``vggish``.  Under ``vggish`` the session runs
    ``audio_backbone`` (default: the model's ``spatial["audio"]``) on the examples itself, ``encoder_batch`` at a time like
    the encoders inside the model, so a row's bits do not depend on how many frames a push paired.  The dict handed to the model
    stream is keyed in the model's own modality order.

    The text leg.  ``text=TextStream(encoder, streams, ...)`` makes the session produce the ``bert`` rows itself: ``bert`` leaves
    ``extra_keys`` (``extra`` for it is refused) and a frame is emitted once its example and its text row exist
    (``pair_schedule_text``).  Text rows wait in the [S, Rf, 768] ring that ``extra`` rows use, slot = frame number masked with
    Rf - 1, written at ``text_seen``; ``push_text`` refuses text that runs more than Rf rows ahead of the pairing
    (``check_text_waiting``).  Frames now wait for their sentence as well, so ``hold`` has to cover an utterance (e.g. 512 at
    30 fps), and a stream can have up to ``hold`` examples whose frames are unpaired plus ``lead`` ahead of the frames: the
    example ring is ``hold_ring(hold + lead, examples_per_step)`` slots of win * 64 floats, 24.6 KB per example (1024
    slots, 25 MB per stream, at hold = 512).  ``finish`` advances the stream's text to its last frame with zero rows first.
    Tokenisation and speech recognition are the caller's, and spans are frame numbers.

    The window rule.  ``window=(window_length, hop_length)`` makes the model stage a ``WindowStream`` (window_stream.py): the
    session then takes an LFAN, a CAN, a JMT or an MT, and a paired frame's logits come out once ``window_length`` more paired
    frames of its stream have followed it (the evaluator's windows, overlaps averaged); ``finish`` flushes the stream's tail
    window after its last pairs.  ``push`` / ``push_text`` / ``finish`` return the rows emitted and their counts, ``decisions``
    receives exactly those rows, ``paired`` keeps its meaning (frames handed to the model) and ``emitted`` counts the rows that
    came out.  Without ``window=`` every paired frame is emitted at once and ``emitted`` equals ``paired``.

    Standardised rows.  ``mean_std=`` ({feature: {"mean", "std"}} or a ``feature_stats.FeatureStandardizer``) makes the session
    hand the model ``(row - mean) / std`` per component, the reference's ``transforms.Normalize`` (base/dataset.py:516-539),
    for the rows it produces itself: ``vggish`` from its audio backbone and ``bert`` from its text leg (a frame without a word
    becomes ``(0 - mean) / std``).  One in-place launch per such modality where the model's input is formed; the rings hold
    raw rows.  A key for ``video``, ``logmel``, a modality the model lacks or one that arrives through ``extra=`` (the
    caller's finished rows) is a ValueError at construction; a modality without a key stays raw.

    A push that would let more than ``hold`` frames or ``lead`` examples wait, and any argument one of the stages refuses,
    raises ValueError before any launch and changes no state, the stages' included.  A stream's counts above ``max_new`` in one
    call reach the model in several pushes, in time order."""

    def __init__(self, model, streams, fps, *, sample_rate=16000, channels=1, resample=None, size=48, crop=40, hold=64, lead=8,
                 max_new=32, max_samples=4096, encoder_batch=8, audio_backbone=None, decisions=None,
                 max_side=1024, video_format="rgb24", video_matrix="bt601", video_range="limited", text=None, window=None,
                 mean_std=None):
        cls = CANStream if isinstance(model, CAN) else LFANStream
        if window is not None:
            from .window_stream import WindowStream
            try:
                window_length, hop_length = (int(v) for v in window)
            except (TypeError, ValueError):
                raise ValueError(f"window: expected (window_length, hop_length), got {window!r}") from None
            if not isinstance(model, (LFAN, CAN, JMT)):
                raise TypeError(f"AVStream(window=) needs an LFAN, a CAN, a JMT or an MT, got {type(model).__name__}")
        elif not isinstance(model, cls._model_class):
            raise TypeError(f"AVStream needs an LFAN or a CAN (JMT / MT attend over time and are not causal), got "
                            f"{type(model).__name__}")
        if model.training:
            raise RuntimeError("AVStream: the model is in train mode; batch statistics are undefined frame by frame -- call .eval()")
        mods = list(model.modality if isinstance(model, LFAN) else model.modalities)
        audio_keys = [m for m in mods if m in AUDIO_KEYS]
        if "video" not in mods or len(audio_keys) != 1:
            raise ValueError(f"AVStream needs a model with 'video' and exactly one of {AUDIO_KEYS}, got {mods}")
        if not fps > 0:
            raise ValueError(f"fps = {fps!r}: must be positive")
        if isinstance(lead, bool) or int(lead) != lead or lead < 1:
            raise ValueError(f"lead = {lead!r}: must be an integer >= 1")
        self.audio_key = audio_keys[0]
        self.text = text
        if text is not None:
            from .text_stream import TextStream
            if not isinstance(text, TextStream):
                raise TypeError(f"text: expected a TextStream, got {type(text).__name__}")
            if "bert" not in mods:
                raise ValueError(f"AVStream: a text leg needs a model with 'bert', got {mods}")
            if text.streams != int(streams):
                raise ValueError(f"text: a TextStream of {text.streams} streams for a session of {int(streams)}")
        self.extra_keys = [m for m in mods if m != "video" and m != self.audio_key and not (m == "bert" and text is not None)]
        # standardised are the rows the session makes itself: vggish from its audio backbone, bert from its text leg
        own = {m: 128 if m == "vggish" else text.hidden for m in mods if m == "vggish" or (m == "bert" and text is not None)}
        if mean_std is not None:
            for m in getattr(mean_std, "keys", lambda: ())():
                if m in self.extra_keys:
                    raise ValueError(f"AVStream(mean_std=): {m!r} arrives through extra=, which takes the caller's finished rows")
                if m not in mods:
                    raise ValueError(f"AVStream(mean_std=): the model has no {m!r} (its modalities: {mods})")
        self.standardizer = as_standardizer(mean_std, dims=own, allowed=tuple(own), who="AVStream(mean_std=)")
        self.audio_backbone = None
        if self.audio_key == "vggish":
            spatial = getattr(model, "spatial", {})
            self.audio_backbone = audio_backbone if audio_backbone is not None else (spatial["audio"] if "audio" in spatial else None)
            if self.audio_backbone is None:
                raise ValueError("AVStream: the model takes 'vggish' rows and has no audio backbone of its own: pass audio_backbone=")
        self.model, self.streams, self.fps, self.hold, self.lead, self.max_new = model, int(streams), fps, int(hold), int(lead), int(max_new)
        device = next(model.parameters()).device
        self.frame_stream = FrameStream(streams, size=size, crop=crop, hold=hold, max_new=max_new, device=device,
                                        max_side=max_side, pixel_format=video_format, matrix=video_matrix, range=video_range)
        self.audio_stream = LogMelStream(streams, 1.0 / fps, max_samples=max_samples, device=device, sample_rate=sample_rate,
                                         channels=channels, resample=resample)   # hop_sec: the expression of audio_features
        self.window = None if window is None else (window_length, hop_length)
        if window is None:
            self.model_stream = cls(model, streams, max_new=max_new, encoder_batch=encoder_batch)
        else:
            self.model_stream = WindowStream(model, streams, window_length, hop_length, max_new=max_new, encoder_batch=encoder_batch)
        self.device, self.win = device, self.audio_stream.win
        max_out = max_samples if resample is None else self.audio_stream.max_outputs
        self.examples_per_step = examples_per_step(max_out, self.audio_stream.hop_frames)
        self.ring_frames = self.frame_stream.ring_frames
        # with a text leg the examples of up to ``hold`` unpaired frames wait too, not only the ``lead`` ahead of the frames
        self.ring_examples = hold_ring(self.lead + (self.hold if text is not None else 0), self.examples_per_step)
        self.extra_dims = {m: self.model_stream._cin(m) for m in self.extra_keys}
        self._ring_dims = dict(self.extra_dims)   # every float ring of frame rows: the extra modalities and the text leg's
        if text is not None:
            self._ring_dims["bert"] = self.model_stream._cin("bert")
            if text.hidden != self._ring_dims["bert"]:
                raise ValueError(f"text: the encoder's hidden size {text.hidden} is not the model's 'bert' embedding dim "
                                 f"{self._ring_dims['bert']}")
            if text.device != device:
                raise ValueError(f"text: the encoder is on {text.device}, the model on {device}")
            text.reset()
        for m, e in self._ring_dims.items():
            if e % 4:
                raise ValueError(f"{m}: embedding dim {e} is not a multiple of 4 (the row gather moves float4)")
        if self.standardizer is not None:
            for m in self.standardizer.keys():
                if self.standardizer.dim(m) != self.model_stream._cin(m):
                    raise ValueError(f"AVStream(mean_std=): {m!r} has {self.standardizer.dim(m)} components, the model's "
                                     f"embedding dim is {self.model_stream._cin(m)}")
            self.standardizer.to(device)
        self.frames_seen, self.examples_seen, self.paired = [0] * self.streams, [0] * self.streams, [0] * self.streams
        self.emitted = [0] * self.streams
        self._exring, self._extra = None, {}   # allocated by the first push that needs them
        self.decisions, self._ended = None, set()   # _ended: finished streams whose decisions still stand
        if decisions is not None:
            from .decisions import DecisionStream
            kw = dict(decisions)
            if "task" in kw or "device" in kw:
                raise ValueError("decisions: the task and the device are the model's")
            kw.setdefault("max_new", self.max_new)
            if int(kw["max_new"]) < self.max_new:
                raise ValueError(f"decisions: max_new = {kw['max_new']} is below the session's {self.max_new}")
            self.decisions = DecisionStream(self.model_stream._n_out(), self.streams, task=model.task, device=device, **kw)

    # ------------------------------------------------------------------------------------------------ checks (no launch)
    def _indices(self, streams):
        return self.frame_stream._indices(streams)

    def _check_extra(self, extra, rows):
        extra = {} if extra is None else dict(extra)
        if not rows and not extra:
            return extra
        if sorted(extra) != sorted(self.extra_keys):
            raise ValueError(f"extra: expected rows for {self.extra_keys} next to the new frames, got {sorted(extra)}")
        for m, x in extra.items():
            if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
                    and tuple(x.shape) == (rows, self.extra_dims[m])):
                raise ValueError(f"extra[{m!r}]: expected float32 [{rows}, {self.extra_dims[m]}] on the GPU, one row per new frame, "
                                 f"got {(x.dtype, x.device, tuple(x.shape)) if torch.is_tensor(x) else type(x)}")
        return extra

    # ------------------------------------------------------------------------------------------------ the holds
    def _alloc(self):
        if self._exring is None:
            self._exring = torch.zeros((self.streams, self.ring_examples, self.win * 64), device=self.device, dtype=torch.float32)
            self._extra = {m: torch.zeros((self.streams, self.ring_frames, e), device=self.device, dtype=torch.float32)
                           for m, e in self._ring_dims.items()}

    def _hold_rows(self, rows, ring, positions, counts):
        row_stream, row_pos = ops.stream_row_table(positions, counts, self.device)
        ops.tcn_stream_append_rows(rows.contiguous(), ring, row_stream, row_pos, max(counts))

    def _held_rows(self, ring, pairs):
        """ring [S, R, C], pairs (stream, position) -> [len(pairs), C]."""
        r = ring.shape[1]
        index = torch.tensor([s * r + (p & (r - 1)) for s, p in pairs], dtype=torch.int64, device=self.device)
        return ops.gather_rows(ring.view(-1, ring.shape[2]), index)

    def _emit(self, owed, example_rows):
        """owed[s]: the (frame, example) pairs of stream s, in time order; ``example_rows``: (stream, example) list ->
        [n, win * 64].  Takes the frames, runs the model ``max_new`` frames of a stream at a time -> parts[s]: the rows the
        model stream emitted for stream s (every paired frame's; with ``window=`` those that became final), for ``_result``."""
        counts = [len(p) for p in owed]
        parts, at = [[] for _ in owed], [0] * self.streams
        while any(a < c for a, c in zip(at, counts)):
            step = [min(self.max_new, c - a) for a, c in zip(at, counts)]
            rows = [(s, f, e) for s in range(self.streams) for f, e in owed[s][at[s]:at[s] + step[s]]]
            X = {}
            for m in self.model_stream.modalities:   # the model's own order
                if m == "video":
                    X[m] = self.frame_stream.take([(s, f) for s, f, _ in rows])
                elif m == self.audio_key:
                    ex = example_rows([(s, e) for s, _, e in rows]).view(len(rows), self.win, 64)
                    X[m] = ex.transpose(1, 2) if m == "logmel" else self.model_stream._in_groups(self.audio_backbone, ex)
                else:
                    X[m] = self._held_rows(self._extra[m], [(s, f) for s, f, _ in rows])
                if self.standardizer is not None and m in self.standardizer:   # fresh rows of this call: in place
                    self.standardizer(m, X[m], out=X[m])
            logits = self.model_stream.push_ragged(X, step)
            self._deliver(parts, *(logits if self.window is not None else (logits, step)))
            at = [a + c for a, c in zip(at, step)]
        for s, c in enumerate(counts):
            self.paired[s] += c
        return parts

    def _deliver(self, parts, logits, got):
        """The rows the model stream gave, ``got[s]`` of stream s: to the decisions and into ``parts[s]``."""
        rows, k = [None] * self.streams, 0
        for s, c in enumerate(got):
            if c:
                rows[s] = logits[k:k + c]
                parts[s].append(rows[s])
                k += c
        if self.decisions is None or not k:
            return
        stale = [s for s in self._ended if got[s]]
        self.decisions.reset(stale)
        self._ended.difference_update(stale)
        step, at = self.decisions.max_new, [0] * self.streams
        if max(got) <= step:
            self.decisions.push_ragged(logits, got)
            return
        while any(a < c for a, c in zip(at, got)):   # a finish can flush up to a window of rows per stream
            take = [min(step, c - a) for a, c in zip(at, got)]
            self.decisions.push_ragged(torch.cat([rows[s][at[s]:at[s] + t] for s, t in enumerate(take) if t]), take)
            at = [a + t for a, t in zip(at, take)]

    def _result(self, parts):
        """parts[s]: the rows stream s emitted in this call, in time order -> (logits [P, n_out], counts), stream-major."""
        counts = [sum(p.shape[0] for p in per) for per in parts]
        for s, c in enumerate(counts):
            self.emitted[s] += c
        flat = [p for per in parts for p in per]
        if not flat:
            return torch.empty((0, self.model_stream._n_out()), device=self.device, dtype=torch.float32), counts
        return (torch.cat(flat) if len(flat) > 1 else flat[0]), counts

    # ------------------------------------------------------------------------------------------------ the session
    @takes_layout("video", "video_layout")
    @torch.no_grad()
    def push(self, video=None, video_counts=None, audio=None, audio_counts=None, extra=None, video_boxes=None):
        if video is None and video_counts is None and video_boxes is not None:
            raise ValueError("push: video_boxes without video")
        fs = self.frame_stream
        return self._push(video, video_counts, audio, audio_counts, extra, fs.check_push, fs.push, (video_boxes,))

    @takes_layout("video", "video_layout")
    @torch.no_grad()
    def push_aligned(self, video, video_counts, video_affines, audio=None, audio_counts=None, extra=None, align_size=256):
        """``push`` of full camera frames with one affine map per frame: ``video_affines`` [M, 6] host float64, Pillow's
        coefficients (``frames.similarity_from_landmarks`` makes them from the detector's five landmarks); frame m is warped
        to an ``align_size`` face first, as ``FrameStream.push_aligned`` does.  Everything else is ``push``."""
        if video is None:
            raise ValueError("push_aligned: video_affines without video" if video_affines is not None else
                             "push_aligned: no video; a push without frames is push()")
        fs = self.frame_stream
        return self._push(video, video_counts, audio, audio_counts, extra, fs.check_push_aligned, fs.push_aligned,
                          (video_affines, align_size))

    def _push(self, video, video_counts, audio, audio_counts, extra, check_frames, push_frames, how):
        """The one body of ``push`` and ``push_aligned``: ``check_frames(video, counts, *how)`` and
        ``push_frames(video, counts, *how)`` are the ``FrameStream``'s pair for this kind of frames."""
        zeros = [0] * self.streams
        if (video is None) != (video_counts is None) or (audio is None) != (audio_counts is None):
            raise ValueError("push: video and video_counts come together, and so do audio and audio_counts")
        self.model_stream._check_keys(dict.fromkeys(self.model_stream.modalities))   # the model may have left eval mode
        vcounts = check_frames(video, video_counts, *how) if video is not None else zeros
        extra = self._check_extra(extra, sum(vcounts))
        pcm, acounts = self.audio_stream.check_push(audio, audio_counts) if audio is not None else (None, zeros)
        for s in range(self.streams):
            after = self.audio_stream.examples_after(s, acounts[s]) if acounts[s] else self.examples_seen[s]
            try:
                check_waiting(self.frames_seen[s], self.examples_seen[s], self.paired[s], vcounts[s], after, self.hold, self.lead)
            except ValueError as err:
                raise ValueError(f"stream {s}: {err}") from None
        # nothing below refuses
        self._alloc()
        if sum(acounts):
            examples, got = self.audio_stream.push(pcm, acounts)
            if sum(got):
                self._hold_rows(examples.view(-1, self.win * 64), self._exring, self.examples_seen, got)
                self.examples_seen = [e + g for e, g in zip(self.examples_seen, got)]
        if sum(vcounts):
            push_frames(video, vcounts, *how)
            for m in self.extra_keys:
                self._hold_rows(extra[m], self._extra[m], self.frames_seen, vcounts)
            self.frames_seen = [f + c for f, c in zip(self.frames_seen, vcounts)]
        return self._emit_owed()

    @property
    def text_seen(self):
        """Per stream, the frames whose text row is final (the ``TextStream``'s ``covered``); None without a text leg."""
        return None if self.text is None else self.text.covered

    def _emit_owed(self):
        """Pair what every stream owes now and run it."""
        if self.text is None:
            owed = [pair_schedule(f, e, p) for f, e, p in zip(self.frames_seen, self.examples_seen, self.paired)]
        else:
            owed = [pair_schedule_text(f, e, t, p)
                    for f, e, t, p in zip(self.frames_seen, self.examples_seen, self.text.covered, self.paired)]
        return self._result(self._emit(owed, lambda pairs: self._held_rows(self._exring, pairs)))

    def _hold_text(self, rows, counts, before):
        """The new text rows of a ``TextStream`` call into their ring slots, at the frame numbers ``before`` (+ i)."""
        if sum(counts):
            self._hold_rows(rows, self._extra["bert"], before, counts)

    @torch.no_grad()
    def push_text(self, sentences, upto=None):
        if self.text is None:
            raise ValueError("push_text: the session has no text leg (AVStream(..., text=TextStream(...)))")
        self.model_stream._check_keys(dict.fromkeys(self.model_stream.modalities))
        plan = self.text.check_push(sentences, upto)
        for s, new in enumerate(plan[2]):
            try:
                check_text_waiting(self.text.covered[s], new, self.paired[s], self.ring_frames)
            except ValueError as err:
                raise ValueError(f"stream {s}: {err}") from None
        # nothing below refuses
        self._alloc()
        before = list(self.text.covered)
        self._hold_text(*self.text._run(plan), before)
        return self._emit_owed()

    @torch.no_grad()
    def finish(self, streams=None):
        idx = sorted(set(self._indices(streams)))
        self.model_stream._check_keys(dict.fromkeys(self.model_stream.modalities))
        self._alloc()
        if self.text is not None:   # frames whose sentence never came have no word: zero rows, written over the slots' stale ones
            upto = {s: self.frames_seen[s] for s in idx if self.text.covered[s] < self.frames_seen[s]}
            plan, at = self.text.check_push([], upto), list(self.text.covered)
            self._hold_text(*self.text._run(plan), at)
        before = list(self.examples_seen)
        last, got = self.audio_stream.finish(idx)   # every remaining example of those streams, stream-major
        first, at = {}, 0
        for s in idx:
            first[s], at = at, at + got[s]
            self.examples_seen[s] += got[s]
        owed = [pair_schedule(self.frames_seen[s], self.examples_seen[s], self.paired[s], final=self.examples_seen[s])
                if s in first else [] for s in range(self.streams)]
        re, tail = self.ring_examples, last.view(-1, self.win * 64)

        def example_rows(pairs):
            # an example emitted before the end sits in its ring slot (without a text leg only the last one can be asked for:
            # the earlier ones were paired when they came, or belong to frames that never came; with one, any example from
            # ``paired`` on, whose frame was still waiting for its text); one the end produced is a row of ``last``
            index = [s * re + (e & (re - 1)) if e < before[s] else self.streams * re + first[s] + e - before[s] for s, e in pairs]
            src = self._exring.view(-1, self.win * 64)
            if any(i < self.streams * re for i in index):
                src = torch.cat([src, tail])
            else:
                src, index = tail, [i - self.streams * re for i in index]
            return ops.gather_rows(src.contiguous(), torch.tensor(index, dtype=torch.int64, device=self.device))

        parts = self._emit(owed, example_rows)
        if self.window is not None:   # the frames still waiting for their window: the tail or the short window
            self._deliver(parts, *self.model_stream.finish(idx))
        out = self._result(parts)
        self._reset_stages(idx)
        self._ended.update(idx)
        return out

    def reset(self, streams=None):
        idx = self._indices(streams)
        self._reset_stages(idx)
        if self.decisions is not None:
            self.decisions.reset(idx)
            self._ended.difference_update(idx)

    def _reset_stages(self, idx):
        self.frame_stream.reset(idx)
        self.audio_stream.reset(idx)
        self.model_stream.reset(idx)
        if self.text is not None:
            self.text.reset(idx)
        for s in idx:
            self.frames_seen[s] = self.examples_seen[s] = self.paired[s] = self.emitted[s] = 0
