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
"""
import math

import torch

from . import ops
from .audio_backbone import SAMPLE_RATE, mel_matrix

ROW_SAMPLES, ROW_HOP, PAD_SAMPLES, LOG_OFFSET = 400, 160, SAMPLE_RATE, 0.01


def num_rows(samples):
    """STFT rows of ``samples`` unpadded samples: ``cer_logmel_num_frames(samples, 0)`` for any Python int."""
    return 0 if samples < ROW_SAMPLES else 1 + (samples - ROW_SAMPLES) // ROW_HOP


def _pow2(need):
    r = 1
    while r < need:
        r *= 2
    return r


def ring_sizes(win, max_samples):
    """(Rs, Rm) for examples of ``win`` rows and pushes of up to ``max_samples`` samples per stream (derivation above)."""
    return _pow2(ROW_SAMPLES - 1 + max_samples), _pow2(win + max_samples // ROW_HOP + 1)


def num_examples(rows, win, hop_frames):
    """How many examples ``example_starts(rows, win, hop_frames)`` has (the reference's 1 + floor((rows - win) / hop))."""
    return max(1 + int(math.floor((rows - win) / hop_frames)), 0)


def pad_chunks(max_samples):
    """The counts of the internal pushes in which ``finish`` writes the one second of padding: at most ``max_samples`` each."""
    return [min(max_samples, PAD_SAMPLES - done) for done in range(0, PAD_SAMPLES, max_samples)]


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

    Bad arguments raise ValueError before any launch and leave the state as it was.  Other rates and multi-channel input are
    refused: the polyphase resampler carries state of its own, ``VGGish.wav_int16_to_examples(resample=...)`` takes such
    input as a whole file.

    With the model streams: ``examples.transpose(1, 2)`` is the packed [M, 64, 96] view ``LFANStream.push_ragged`` takes
    under ``logmel`` (with ``example_counts`` as its counts), and ``model.spatial["audio"](examples)`` gives the 128-d rows for
    ``push_features_ragged`` under ``vggish``.  Example e belongs to video frame e and needs audio up to 0.975 s after that
    frame's time (the reference's alignment, not a property of this class): the caller holds video frames back until
    ``examples_emitted`` has reached them.  Buffering video is not done here."""

    def __init__(self, streams, hop_sec, window_sec=0.96, max_samples=4096, device="cuda", sample_rate=SAMPLE_RATE):
        if sample_rate != SAMPLE_RATE:
            raise ValueError(f"LogMelStream takes {SAMPLE_RATE} Hz mono int16 only, got {sample_rate} Hz: resample first, or "
                             "give the whole file to VGGish.wav_int16_to_examples(resample='kaiser_best' / 'kaiser_fast')")
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
        self.ring_samples, self.ring_rows = ring_sizes(self.win, self.max_samples)
        self.samples_seen = [0] * self.streams
        self.rows_done = [0] * self.streams
        self.examples_emitted = [0] * self.streams
        self._ring = self._melring = self._mel = self._no_pcm = None   # allocated by the first push that launches

    def _alloc(self):
        if self._ring is None:
            self._ring = torch.zeros((self.streams, self.ring_samples), device=self.device, dtype=torch.int16)
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

    @torch.no_grad()
    def push(self, pcm_int16, counts):
        pcm = torch.as_tensor(pcm_int16)
        if pcm.dtype != torch.int16 or pcm.dim() != 1:
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
        if not sum(counts):
            return self._empty(), [0] * self.streams
        offsets, at = [], 0
        for c in counts:
            offsets.append(at)
            at += c
        out, emitted = self._step(pcm.to(self.device).contiguous(), counts, offsets, [None] * self.streams)
        return (out if out is not None else self._empty()), emitted

    @torch.no_grad()
    def finish(self, streams=None):
        idx = [s for s in sorted(set(self._indices(streams))) if self.samples_seen[s] > 0]
        emitted, parts = [0] * self.streams, {s: [] for s in idx}
        limits = [None] * self.streams
        for s in idx:   # the reference's example count for the padded signal
            limits[s] = num_examples(num_rows(self.samples_seen[s] + PAD_SAMPLES), self.win, self.hop_frames)
        for n in pad_chunks(self.max_samples) if idx else []:
            counts = [n if s in parts else 0 for s in range(self.streams)]
            self._alloc()
            out, got = self._step(self._no_pcm, counts, [None] * self.streams, limits)
            at = 0
            for s in idx:
                if got[s]:
                    parts[s].append(out[at:at + got[s]])
                    at += got[s]
                    emitted[s] += got[s]
        self.reset(self._indices(streams))
        flat = [p for s in idx for p in parts[s]]
        return (torch.cat(flat) if flat else self._empty()), emitted
