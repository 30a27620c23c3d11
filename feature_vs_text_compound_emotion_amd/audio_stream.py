"""Streaming audio front end: 16 kHz int16 PCM chunks of S live streams -> VGGish log-mel examples, on the device.

``VGGish.wav_int16_to_examples`` needs the whole signal.  Here STFT row r (samples 160 r .. 160 r + 399) is computed once, when
its last sample has arrived, and kept in a ring; example e (rows round(hop e) .. + win - 1) is emitted when its last row
exists; the reference's one second of edge padding is applied when a stream ends (``finish``).  The rows come from the device
function the offline kernel runs (csrc/logmel_row.h), so the examples of a stream are the same bits as
``wav_int16_to_examples`` of the whole signal under any chunking, any number of streams and any number of ring wraps.

State (csrc/logmel_stream.hip): a sample ring [S, Rs] int16 and a log-mel ring [S, Rm, 64] float32 on the device, and three
Python ints per stream on the host (samples, rows computed, examples emitted).  ``schedule`` turns those ints and a count
of new samples into the rows and examples that become complete: a pure function, no GPU.  A push uploads one int32 table and
runs at most three launches (append, rows, examples), whatever the number of streams.

Ring sizes (``ring_sizes``).  After a push a stream carries at most 399 samples that belong to no finished row (row ``rows``
starts at 160 rows > samples - 400), and the next push adds at most ``max_samples``: Rs is the power of two >=
399 + max_samples.  An example that is still pending starts after ``rows - win``, and a push adds at most
``max_samples // 160 + 1`` rows: Rm is the power of two >= win + max_samples // 160 + 1.

Other rates and channel counts (``resample="kaiser_best"`` / ``"kaiser_fast"``).  The polyphase resampler of the offline path
(``ops.resample_pcm``, ``resample_taps``) is as streamable as the rows: with L / M = 16000 / rate in lowest terms and a table of T
taps per phase, J = (T - 2) / 2, output n reads the T inputs q - J .. q + J + 1, q = (n M) div L, and nothing else.  The stream
keeps a mixed-input ring [S, Rin] float64 (the channel mean at the input rate) and a 16 kHz ring [S, Rs] float64 in place of
the int16 one; output n is computed once, when input q + J + 1 has arrived (``resample_schedule``, pure), by the device
function the offline kernel runs (csrc/resample_row.h), and the new 16 kHz samples go through ``schedule`` as above.  The one
second of edge padding is ``sample_rate`` copies at the input rate; after it ``finish`` emits the outputs up to
``resampled_length(samples + sample_rate, sample_rate)`` whose last inputs lie past the padding and read as zero, as offline.
A push uploads one int32 table and runs at most four launches (mix-append, resample, rows, examples).

Ring sizes (``resample_ring_sizes``).  The first output that is not complete after a push has q + J + 1 >= inputs, so its first
input q - J is at most T - 1 = 2 J + 1 behind the newest, and the next push adds at most ``max_samples``: Rin is the power of two
>= T - 1 + max_samples.  A push completes the outputs from ceil((a - J - 1) L / M) to ceil((b - J - 1) L / M) for input counts
a <= b <= a + max_samples, at most ``max_samples * L // M + 1`` of them; the tail of ``finish`` starts at
ceil((F - J - 1) L / M) for the F padded inputs and ends at int(F * (16000.0 / rate)) <= F L / M + 1, at most
``(J + 1) * L // M + 2``.  With ``max_out`` the larger of the two, Rs and Rm are ``ring_sizes(win, max_out)``: 399 pending
samples + max_out, and win + max_out // 160 + 1 rows.

Delay.  Output n waits for input q + J + 1: the resampler adds J + 1 input samples of algorithmic delay (``delay_sec``), 4.0 ms
at 48 kHz with ``kaiser_best`` (J = 192) and 1.0 ms with ``kaiser_fast`` (J = 48), on top of the 0.975 s the alignment of an
example with its video frame already needs.
"""
import math

import torch

from . import ops
from .audio_backbone import RESAMPLE_FILTERS, SAMPLE_RATE, mel_matrix, resample_taps, resampled_length

ROW_SAMPLES, ROW_HOP, PAD_SAMPLES, LOG_OFFSET = 400, 160, SAMPLE_RATE, 0.01


def num_rows(samples):
    """STFT rows of ``samples`` unpadded samples: ``cer_logmel_num_frames(samples, 0)`` for any Python int."""
    return 0 if samples < ROW_SAMPLES else 1 + (samples - ROW_SAMPLES) // ROW_HOP


def ring_sizes(win, max_samples):
    """(Rs, Rm) for examples of ``win`` rows and pushes of up to ``max_samples`` samples per stream (derivation above)."""
    return ops.pow2_at_least(ROW_SAMPLES - 1 + max_samples), ops.pow2_at_least(win + max_samples // ROW_HOP + 1)


def num_examples(rows, win, hop_frames):
    """How many examples ``example_starts(rows, win, hop_frames)`` has (the reference's 1 + floor((rows - win) / hop))."""
    return max(1 + int(math.floor((rows - win) / hop_frames)), 0)


def pad_chunks(max_samples, pad=PAD_SAMPLES):
    """The counts of the internal pushes in which ``finish`` writes the one second of padding (``pad`` samples at the input
    rate): at most ``max_samples`` each."""
    return [min(max_samples, pad - done) for done in range(0, pad, max_samples)]


def outputs_complete(frames, L, M, T):
    """How many 16 kHz outputs a stream with ``frames`` input frames has complete: output n reads inputs up to
    (n M) div L + J + 1, J = (T - 2) / 2, so it is complete when (n M) div L + J + 1 < frames, i.e. n M < (frames - J - 1) L."""
    reach = frames - (T - 2) // 2 - 1
    return -(-reach * L // M) if reach > 0 else 0


def resample_schedule(frames, produced, count, L, M, T, final=None):
    """What ``count`` new input frames complete in a stream that has ``frames`` input frames and ``produced`` 16 kHz samples:
    (frames + count, n0, n1), the outputs n0 <= n < n1 become complete (``outputs_complete``).  ``final``: the stream has
    ended and every output below ``final`` is due, whatever inputs it lacks (``finish``: they read as zero).  Python ints,
    unbounded; no GPU."""
    frames += count
    n1 = outputs_complete(frames, L, M, T) if final is None else final
    return frames, produced, max(produced, n1)


def resampled_step(state, count, offset, L, M, T, win, hop_frames, limit=None, final=None):
    """One stream's share of a resampled push, from its ints ``state`` = (input frames, 16 kHz samples, rows, examples) and
    ``count`` new frames at frame ``offset`` of the packed input (None: copies of the last mixed frame): (new state, the
    mix segment (position, count, offset) or None, the output segment (n0, count, r0, q0, input frames) or None with
    q0, r0 = divmod(n0 M, L) in unbounded ints, the new rows' numbers, the new examples' start rows).  The segments are
    what ``ops.resample_stream_tables`` takes after the stream index.  Pure."""
    frames, produced, rows, examples = state
    new_frames, n0, n1 = resample_schedule(frames, produced, count, L, M, T, final)
    (produced, rows, examples), new_rows, starts = schedule(produced, rows, examples, n1 - n0, win, hop_frames, limit)
    q0, r0 = divmod(n0 * M, L)
    return ((new_frames, produced, rows, examples), (frames, count, offset) if count else None,
            (n0, n1 - n0, r0, q0, new_frames) if n1 > n0 else None, new_rows, starts)


def resample_ring_sizes(win, max_samples, L, M, T):
    """(Rin, Rs, Rm, max_out) for pushes of up to ``max_samples`` input frames per stream through an [L, T] tap table
    (derivation above); ``max_out``: the most 16 kHz samples one push or the tail of ``finish`` adds to a stream."""
    max_out = max(max_samples * L // M + 1, (T // 2) * L // M + 2)
    rs, rm = ring_sizes(win, max_out)
    return ops.pow2_at_least(T - 1 + max_samples), rs, rm, max_out


def schedule(samples, rows, examples, count, win, hop_frames, limit=None):
    """What ``count`` new samples complete in a stream that has ``samples`` samples, ``rows`` rows and ``examples`` examples:
    (new state (samples, rows, examples), the new rows' numbers, the new examples' start rows).  Example e starts at
    ``round(hop_frames * e)`` (Python's half-to-even, like ``example_starts``) and is complete when its last row exists;
    ``limit`` caps the example count (``finish``: the reference's count for the padded signal)."""
    samples += count
    new_rows = list(range(rows, num_rows(samples)))
    rows += len(new_rows)
    starts = []
    while limit is None or examples < limit:
        start = round(hop_frames * examples)
        if start + win > rows:
            break
        starts.append(start)
        examples += 1
    return (samples, rows, examples), new_rows, starts


class LogMelStream:
    """``VGGish.wav_int16_to_examples`` for ``streams`` live streams of 16 kHz mono int16 PCM, a chunk at a time.

      push(pcm_int16 [M], counts)  stream s brings ``counts[s]`` (0 .. max_samples) new samples, packed stream-major in
                                   ascending stream order -> (examples [E, win, 64] float32, example_counts): every example
                                   that became complete, stream-major, each stream's in time order; example_counts[s] of them
                                   belong to stream s.  All-zero counts launch nothing and return [0, win, 64].
      finish(streams=None)         the same after the reference's one second of edge padding (16 000 copies of the stream's
                                   last sample, written on the device); those streams are reset.  A stream that never
                                   received a sample emits nothing.
      reset(streams=None)          forget those streams.
      samples_seen, examples_emitted   host lists, one int per stream.

    Bad arguments raise ValueError before any launch and leave the state as it was.

    With ``resample`` = "kaiser_best" / "kaiser_fast" any positive integer ``sample_rate`` and ``channels`` >= 1 are taken, and
    the examples are the bits of ``VGGish.wav_int16_to_examples(pcm, sample_rate, ..., resample=...)`` on the whole signal:
    ``push`` takes [M] int16 for one channel and interleaved [M, C] for more, ``counts[s]`` is in input frames
    (0 .. max_samples), the padding of ``finish`` is ``sample_rate`` copies of the last mixed frame, and ``samples_seen`` counts
    input frames (``resampled``: the 16 kHz samples computed).  16 kHz multi-channel input goes through the same path with the
    identity table, as offline.  The resampler delays the examples by ``delay_sec`` (J + 1 input samples: 4.0 ms at 48 kHz
    with "kaiser_best").  Without ``resample`` only 16 kHz mono is taken, as before.

    With the model streams: ``examples.transpose(1, 2)`` is the packed [M, 64, 96] view ``LFANStream.push_ragged`` takes
    under ``logmel`` (with ``example_counts`` as its counts), and ``model.spatial["audio"](examples)`` gives the 128-d rows for
    ``push_features_ragged`` under ``vggish``.  Example e belongs to video frame e and needs audio up to 0.975 s after that
    frame's time (the reference's alignment, not a property of this class): video frames have to wait until
    ``examples_emitted`` has reached them.  Buffering video is not done here; ``live.AVStream`` holds the frames and pairs them."""

    def __init__(self, streams, hop_sec, window_sec=0.96, max_samples=4096, device="cuda", sample_rate=SAMPLE_RATE, channels=1,
                 resample=None):
        if resample is None:
            if sample_rate != SAMPLE_RATE or channels != 1:
                raise ValueError(f"LogMelStream takes {SAMPLE_RATE} Hz mono int16 only without resample=, got {sample_rate} Hz, "
                                 f"{channels!r} channel(s): pass resample='kaiser_best' / 'kaiser_fast', or give the whole "
                                 "file to VGGish.wav_int16_to_examples(resample=...)")
        elif resample not in RESAMPLE_FILTERS:
            raise ValueError(f"unknown resampling filter {resample!r}: one of {sorted(RESAMPLE_FILTERS)}")
        elif isinstance(channels, bool) or int(channels) != channels or channels < 1:
            raise ValueError(f"channels = {channels!r}: must be an integer >= 1")
        if int(streams) != streams or streams < 1 or int(max_samples) != max_samples or max_samples < 1:
            raise ValueError(f"streams = {streams!r}, max_samples = {max_samples!r}: both must be integers >= 1")
        self.win = int(round(window_sec * 100.0))
        self.hop_frames = hop_sec * 100.0   # the expressions of wav_int16_to_examples
        if not self.hop_frames >= 1.0:
            raise ValueError(f"hop_sec = {hop_sec!r}: less than one STFT row (0.01 s) per example, which the reference never "
                             "produces")
        if self.win < 1:
            raise ValueError(f"window_sec = {window_sec!r}: less than one STFT row")
        self.streams, self.max_samples, self.device = int(streams), int(max_samples), torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"LogMelStream runs on the HIP kernels only (no CPU fallback), got device {device!r}")
        self.resample, self.sample_rate, self.channels = resample, int(sample_rate), int(channels)
        if resample is None:
            self.ring_samples, self.ring_rows = ring_sizes(self.win, self.max_samples)
        else:   # resample_taps refuses a bad rate and a table over MAX_RESAMPLE_TAPS; host memory only
            self._taps_host, self.L, self.M = resample_taps(sample_rate, resample)
            self.T = self._taps_host.shape[1]
            self.ring_inputs, self.ring_samples, self.ring_rows, self.max_outputs = resample_ring_sizes(
                self.win, self.max_samples, self.L, self.M, self.T)
            self.delay_sec = (self.T // 2) / float(self.sample_rate)
            self.resampled = [0] * self.streams
        self.samples_seen = [0] * self.streams
        self.rows_done = [0] * self.streams
        self.examples_emitted = [0] * self.streams
        self._ring = self._melring = self._mel = self._no_pcm = None   # allocated by the first push that launches
        self._inring = self._taps = None

    def _alloc(self):
        if self._ring is None:
            if self.resample is not None:
                self._inring = torch.zeros((self.streams, self.ring_inputs), device=self.device, dtype=torch.float64)
                self._taps = torch.from_numpy(self._taps_host).to(self.device).contiguous()
            self._ring = torch.zeros((self.streams, self.ring_samples), device=self.device,
                                     dtype=torch.int16 if self.resample is None else torch.float64)
            self._melring = torch.zeros((self.streams, self.ring_rows, 64), device=self.device, dtype=torch.float32)
            self._mel = torch.from_numpy(mel_matrix()).to(self.device).contiguous()
            self._no_pcm = torch.zeros(1, device=self.device, dtype=torch.int16)   # the packed input of a pure-padding push

    def _indices(self, streams):
        idx = list(range(self.streams)) if streams is None else [int(s) for s in streams]
        for s in idx:
            if not 0 <= s < self.streams:
                raise IndexError(f"stream {s} of {self.streams}")
        return idx

    def reset(self, streams=None):
        """Forget ``streams`` (indices; None = all).  Only host ints change: a stream reads no slot it has not written
        since."""
        for s in self._indices(streams):
            self.samples_seen[s] = self.rows_done[s] = self.examples_emitted[s] = 0
            if self.resample is not None:
                self.resampled[s] = 0

    def _empty(self):
        return torch.empty((0, self.win, 64), device=self.device, dtype=torch.float32)

    def _step(self, packed, counts, offsets, limits):
        """One append / rows / examples round: stream s gets ``counts[s]`` samples from ``packed`` at ``offsets[s]`` (None:
        copies of its last sample).  Returns (examples or None, example counts)."""
        segs, rows, exs, emitted, state = [], [], [], [0] * self.streams, {}
        for s, c in enumerate(counts):
            if not c:
                continue
            state[s], new_rows, starts = schedule(self.samples_seen[s], self.rows_done[s], self.examples_emitted[s], c, self.win,
                                                  self.hop_frames, limits[s])
            segs.append((s, self.samples_seen[s], c, offsets[s]))
            rows += [(s, ROW_HOP * r, r) for r in new_rows]
            exs += [(s, start) for start in starts]
            emitted[s] = len(starts)
        self._alloc()
        seg_t, row_t, ex_t = ops.logmel_stream_tables(segs, rows, exs, self.device)
        ops.logmel_stream_append(packed, seg_t, max(counts), self._ring)
        if row_t is not None:
            ops.logmel_stream_rows(self._ring, row_t, self._mel, self._melring, LOG_OFFSET)
        out = ops.logmel_stream_examples(self._melring, ex_t, self.win) if ex_t is not None else None
        for s, (n, r, e) in state.items():
            self.samples_seen[s], self.rows_done[s], self.examples_emitted[s] = n, r, e
        return out, emitted

    def _step_resampled(self, packed, counts, offsets, limits, finals):
        """One mix-append / resample / rows / examples round: stream s gets ``counts[s]`` input frames from ``packed`` at frame
        ``offsets[s]`` (None: copies of its last mixed frame); ``finals[s]`` (not None) ends it at that many 16 kHz samples.
        Returns (examples or None, example counts)."""
        mix, outs, rows, exs, emitted, state = [], [], [], [], [0] * self.streams, {}
        for s, c in enumerate(counts):
            if not c and finals[s] is None:
                continue
            state[s], seg, out_seg, new_rows, starts = resampled_step(
                (self.samples_seen[s], self.resampled[s], self.rows_done[s], self.examples_emitted[s]), c, offsets[s], self.L,
                self.M, self.T, self.win, self.hop_frames, limits[s], finals[s])
            if seg is not None:
                mix.append((s,) + seg)
            if out_seg is not None:
                outs.append((s,) + out_seg)
            rows += [(s, ROW_HOP * r, r) for r in new_rows]
            exs += [(s, start) for start in starts]
            emitted[s] = len(starts)
        out = None
        if mix or outs:
            self._alloc()
            mix_t, out_t, row_t, ex_t = ops.resample_stream_tables(mix, outs, rows, exs, self.device)
            if mix_t is not None:
                ops.resample_stream_append(packed, mix_t, max(counts), self.T - 1, self._inring)
            if out_t is not None:
                ops.resample_stream_outputs(self._inring, out_t, max(o[2] for o in outs), self._taps, self.L, self.M, self._ring)
            if row_t is not None:
                ops.logmel_stream_rows_f64(self._ring, row_t, self._mel, self._melring, LOG_OFFSET)
            if ex_t is not None:
                out = ops.logmel_stream_examples(self._melring, ex_t, self.win)
        for s, (f, n, r, e) in state.items():
            self.samples_seen[s], self.resampled[s], self.rows_done[s], self.examples_emitted[s] = f, n, r, e
        return out, emitted

    def check_push(self, pcm_int16, counts):
        """Everything ``push`` refuses, without a launch or a change of state.  Returns (pcm as a tensor, counts as ints)."""
        pcm = torch.as_tensor(pcm_int16)
        if self.resample is not None:
            dims = (1, 2) if self.channels == 1 else (2,)
            if pcm.dtype != torch.int16 or pcm.dim() not in dims or (pcm.dim() == 2 and pcm.shape[1] != self.channels):
                raise ValueError(f"pcm: expected int16 frames of {self.channels} channel(s) packed as "
                                 f"{'[M]' if self.channels == 1 else f'[M, {self.channels}]'}, got {pcm.dtype} {tuple(pcm.shape)}")
        elif pcm.dtype != torch.int16 or pcm.dim() != 1:
            raise ValueError(f"pcm: expected {SAMPLE_RATE} Hz mono int16 samples packed as [M], got {pcm.dtype} "
                             f"{tuple(pcm.shape)} (other formats: VGGish.wav_int16_to_examples(resample=...) on the whole file)")
        try:
            counts = [int(c) for c in counts]
        except TypeError:
            raise ValueError(f"counts: expected a sequence of {self.streams} ints, got {type(counts).__name__}") from None
        if len(counts) != self.streams:
            raise ValueError(f"counts: expected one count per stream ({self.streams}), got {len(counts)}")
        for s, c in enumerate(counts):
            if not 0 <= c <= self.max_samples:
                raise ValueError(f"counts: stream {s} brings {c} samples, outside 0 .. max_samples = {self.max_samples}")
        if pcm.shape[0] != sum(counts):
            raise ValueError(f"pcm: {pcm.shape[0]} samples for counts that sum to {sum(counts)}")
        return pcm, counts

    def examples_after(self, s, count):
        """``examples_emitted[s]`` as it will stand after a push that brings stream ``s`` ``count`` samples: host ints only."""
        if self.resample is None:
            return schedule(self.samples_seen[s], self.rows_done[s], self.examples_emitted[s], count, self.win,
                            self.hop_frames)[0][2]
        return resampled_step((self.samples_seen[s], self.resampled[s], self.rows_done[s], self.examples_emitted[s]), count, 0,
                              self.L, self.M, self.T, self.win, self.hop_frames)[0][3]

    @torch.no_grad()
    def push(self, pcm_int16, counts):
        pcm, counts = self.check_push(pcm_int16, counts)
        if not sum(counts):
            return self._empty(), [0] * self.streams
        offsets, at = [], 0
        for c in counts:
            offsets.append(at)
            at += c
        none = [None] * self.streams
        if self.resample is None:
            out, emitted = self._step(pcm.to(self.device).contiguous(), counts, offsets, none)
        else:
            out, emitted = self._step_resampled(pcm.to(self.device).contiguous(), counts, offsets, none, none)
        return (out if out is not None else self._empty()), emitted

    @torch.no_grad()
    def finish(self, streams=None):
        idx = [s for s in sorted(set(self._indices(streams))) if self.samples_seen[s] > 0]
        emitted, parts = [0] * self.streams, {s: [] for s in idx}
        limits, finals, none = [None] * self.streams, [None] * self.streams, [None] * self.streams
        for s in idx:   # the reference's example count for the padded signal
            if self.resample is None:
                limits[s] = num_examples(num_rows(self.samples_seen[s] + PAD_SAMPLES), self.win, self.hop_frames)
            else:
                finals[s] = resampled_length(self.samples_seen[s] + self.sample_rate, self.sample_rate)
                limits[s] = num_examples(num_rows(finals[s]), self.win, self.hop_frames)
        steps = []
        if idx and self.resample is None:
            steps = [(n, none) for n in pad_chunks(self.max_samples)]
        elif idx:   # the padding at the input rate, then the outputs whose last inputs lie past it
            steps = [(n, none) for n in pad_chunks(self.max_samples, self.sample_rate)] + [(0, finals)]
        for n, final in steps:
            counts = [n if s in parts else 0 for s in range(self.streams)]
            self._alloc()
            if self.resample is None:
                out, got = self._step(self._no_pcm, counts, none, limits)
            else:
                out, got = self._step_resampled(self._no_pcm, counts, none, limits, final)
            at = 0
            for s in idx:
                if got[s]:
                    parts[s].append(out[at:at + got[s]])
                    at += got[s]
                    emitted[s] += got[s]
        self.reset(self._indices(streams))
        flat = [p for s in idx for p in parts[s]]
        return (torch.cat(flat) if flat else self._empty()), emitted
