"""Live text: finished sentences with their frame spans in, per-frame ``bert`` rows out.

The text of a frame exists only after its sentence has been spoken and transcribed, so text arrives a sentence at a time and
late.  ``TextStream`` takes each finished, tokenised sentence with the frames it was spoken over, runs ``BertEncoderHIP`` on
it (the sum of the last four hidden states, speech.py:617-624), drops [CLS] and [SEP] (``exclude_padding``, speech.py:567-586)
and spreads the sentence's words over its frames as the reference spreads a clip's words over the clip
(``align_word_embedding_new``, speech.py:690-738: contiguous blocks, the first ones one frame longer, words beyond the frame
count dropped).  Frames between sentences get zero rows, which is what the reference gives a frame without a word.

One push is: host checks, one upload of the padded ids, BERT in calls of a fixed shape, one ``ops.text_spread_rows`` that forms
every frame row of the call (the index plan is made in the kernel).  The device keeps no state; the host keeps one int per
stream, ``covered[s]``: the frames of stream s whose text row is final.

Fixed call shape.  BERT runs in calls of exactly [sentence_batch, max_tokens]: the GEMM wrappers pick split-K, and with it the
order of their K sums, from the number of rows of a call, so with every call the same size a sentence's rows are the same bits
however many sentences a push brought (the reason the encoders get ``encoder_batch`` frames per call).  Unused rows of a call
repeat that call's first sentence and are dropped: a row without an attended token would make its softmax NaN.

Not built here: tokenisation and speech recognition are the caller's; spans are frame numbers (``frames_of_seconds`` is the
one-line conversion); the reference's word-timestamp alignment (``align_word_embedding``) and its sub-word merging are not
reproduced."""
import numpy as np
import torch

from . import ops


def frames_of_seconds(start_sec, end_sec, fps):
    """(first_frame, num_frames) of the frames whose time i / fps lies in [start_sec, end_sec)."""
    first, end = int(np.ceil(start_sec * fps)), int(np.ceil(end_sec * fps))
    return first, end - first


def spread_index(n_tokens, n_frames):
    """j(i) of ``cer_text_spread_rows`` for i in range(n_frames), in closed form: the list that
    ``feature_extractor.align_tokens_to_frames`` builds block by block (empty when there is no token)."""
    n = min(n_tokens, n_frames)
    if n <= 0:
        return []
    q, r = divmod(n_frames, n)
    return [i // (q + 1) if i < r * (q + 1) else r + (i - r * (q + 1)) // q for i in range(n_frames)]


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


class TextStream:
    """``encoder`` (a ``BertEncoderHIP`` in eval mode on the GPU) for ``streams`` live transcripts.

      push(sentences, upto=None) -> (rows [M, hidden] float32, counts)
            ``sentences``: a list of (stream, token_ids, first_frame, num_frames).  ``token_ids``: the host ints of one
            tokenised sentence, [CLS] first and [SEP] last, 2 <= len <= max_tokens - 1 (the reference refuses a sentence that
            fills every slot).  The spans of one stream come in ascending order, do not overlap and start at or after
            ``covered[s]``.  Frames between ``covered[s]`` and a span and between spans get zero rows; inside a span the
            sentence's words (``ids[1:-1]``) are spread over its frames.  ``upto`` (a list, one frame number or None per
            stream, or a dict stream -> frame number) then advances ``covered[s]`` to that frame with zero rows: silence.  It
            may not lie below the stream's coverage after the call's spans.
            Rows are packed stream-major in ascending stream order, a stream's frames in time order (the convention of
            ``push_ragged``); ``counts[s]`` is how far ``covered[s]`` moved.  Nothing new: an empty [0, hidden], no launch.
      check_push(sentences, upto=None)   everything ``push`` refuses, without a launch or a change of state.
      reset(streams=None)                forget those streams (``covered[s]`` = 0).
      covered                            host list, one int per stream.

    Everything wrong raises ValueError before any launch and changes nothing: spans, ids outside the vocabulary, lengths, an
    encoder on the CPU or in train mode (these two are looked at last, so the host rules can be exercised without a GPU)."""

    def __init__(self, encoder, streams, *, max_tokens=64, sentence_batch=4, last_n_sum=4):
        for v, name, low in ((streams, "streams", 1), (max_tokens, "max_tokens", 4), (sentence_batch, "sentence_batch", 1),
                             (last_n_sum, "last_n_sum", 1)):
            if not _is_int(v) or v < low:
                raise ValueError(f"{name} = {v!r}: must be an integer >= {low}")
        emb = encoder.embeddings
        self.vocab, self.hidden = emb.word_embeddings.weight.shape[0], int(encoder.hidden)
        if max_tokens > emb.position_embeddings.weight.shape[0]:
            raise ValueError(f"max_tokens = {max_tokens} exceeds the encoder's {emb.position_embeddings.weight.shape[0]} positions")
        if self.hidden % 4:
            raise ValueError(f"hidden = {self.hidden} is not a multiple of 4 (the row copy moves float4)")
        self.encoder, self.streams = encoder, int(streams)
        self.max_tokens, self.sentence_batch, self.last_n_sum = int(max_tokens), int(sentence_batch), int(last_n_sum)
        self.covered = [0] * self.streams

    @property
    def device(self):
        return self.encoder.embeddings.word_embeddings.weight.device

    def _indices(self, streams):
        idx = list(range(self.streams)) if streams is None else [int(s) for s in streams]
        for s in idx:
            if not 0 <= s < self.streams:
                raise IndexError(f"stream {s} of {self.streams}")
        return idx

    def reset(self, streams=None):
        """Forget ``streams`` (indices; None = all).  Only host ints change."""
        for s in self._indices(streams):
            self.covered[s] = 0

    # ------------------------------------------------------------------------------------------------ checks (no launch)
    def _upto(self, upto):
        if upto is None:
            return {}
        if isinstance(upto, dict):
            items = list(upto.items())
        else:
            upto = list(upto)
            if len(upto) != self.streams:
                raise ValueError(f"upto: expected one entry per stream ({self.streams}), got {len(upto)}")
            items = [(s, u) for s, u in enumerate(upto) if u is not None]
        for s, u in items:
            if not _is_int(s) or not 0 <= s < self.streams:
                raise ValueError(f"upto: stream {s!r} of {self.streams}")
            if not _is_int(u) or u < 0:
                raise ValueError(f"upto[{s}] = {u!r}: must be a frame number >= 0")
        return {int(s): int(u) for s, u in items}

    def check_push(self, sentences, upto=None):
        """Everything ``push`` refuses, without a launch or a change of state.  Returns the plan of the call:
        (ids per sentence in the order given, per stream the list of (first_frame, num_frames, sentence or None for zeros),
        counts)."""
        try:
            sentences = list(sentences)
        except TypeError:
            raise ValueError(f"sentences: expected a list of (stream, token_ids, first_frame, num_frames), got {type(sentences)}") from None
        upto = self._upto(upto)
        at, spans, all_ids = list(self.covered), [[] for _ in range(self.streams)], []
        for k, item in enumerate(sentences):
            try:
                s, ids, first, num = item
                ids = list(ids)
            except (TypeError, ValueError):
                raise ValueError(f"sentence {k}: expected (stream, token_ids, first_frame, num_frames), got {item!r}") from None
            if not _is_int(s) or not 0 <= s < self.streams:
                raise ValueError(f"sentence {k}: stream {s!r} of {self.streams}")
            if not 2 <= len(ids) <= self.max_tokens - 1:
                raise ValueError(f"sentence {k}: {len(ids)} token ids ([CLS] and [SEP] included); a sentence has 2 .. "
                                 f"max_tokens - 1 = {self.max_tokens - 1} (one that fills every slot is refused, as in the reference)")
            for t in ids:
                if not _is_int(t) or not 0 <= t < self.vocab:
                    raise ValueError(f"sentence {k}: token id {t!r} outside the {self.vocab}-row word-embedding table")
            if not _is_int(first) or not _is_int(num) or num < 1 or first < 0:
                raise ValueError(f"sentence {k}: span first_frame = {first!r}, num_frames = {num!r}: ints, first >= 0, num >= 1")
            s, first, num = int(s), int(first), int(num)
            if first < at[s]:
                raise ValueError(f"sentence {k}: its span starts at frame {first}, before frame {at[s]} up to which the text of "
                                 f"stream {s} is final (covered, or an earlier span of this call: spans ascend and do not overlap)")
            if first > at[s]:
                spans[s].append((at[s], first - at[s], None))
            spans[s].append((first, num, len(all_ids)))
            all_ids.append([int(t) for t in ids])
            at[s] = first + num
        for s, u in upto.items():
            if u < at[s]:
                raise ValueError(f"upto[{s}] = {u} lies below frame {at[s]} up to which the text of stream {s} is final")
            if u > at[s]:
                spans[s].append((at[s], u - at[s], None))
            at[s] = u
        counts = [a - c for a, c in zip(at, self.covered)]
        if sum(counts) >= 1 << 31:
            raise ValueError(f"{sum(counts)} frame rows in one call")
        # the encoder's state last: what is above needs no GPU
        if self.encoder.training:
            raise ValueError("TextStream: the encoder is in train mode -- call .eval()")
        if self.device.type != "cuda":
            raise ValueError("TextStream: the encoder is on the CPU; BertEncoderHIP runs on the HIP kernels only (no CPU fallback)")
        return all_ids, spans, counts

    # ------------------------------------------------------------------------------------------------ the launches
    def encode(self, all_ids):
        """Host id lists -> the token rows [calls * sentence_batch * max_tokens, hidden]: sentence k's token t is row
        k * max_tokens + t (the unused rows of the last call repeat its first sentence)."""
        g, t = self.sentence_batch, self.max_tokens
        calls = (len(all_ids) + g - 1) // g
        host = np.zeros((2, calls * g, t), np.int64)    # ids | mask, one upload
        for k in range(calls * g):
            ids = all_ids[k] if k < len(all_ids) else all_ids[k - k % g]
            host[0, k, :len(ids)] = ids
            host[1, k, :len(ids)] = 1
        dev = torch.from_numpy(host).to(self.device)
        outs = [self.encoder(dev[0, c * g:(c + 1) * g], dev[1, c * g:(c + 1) * g], self.last_n_sum).view(g * t, self.hidden)
                for c in range(calls)]
        return outs[0] if calls == 1 else torch.cat(outs)

    def _run(self, plan):
        all_ids, spans, counts = plan
        total = sum(counts)
        if not all_ids:     # silence only, or nothing at all: no launch
            rows = torch.zeros((total, self.hidden), device=self.device, dtype=torch.float32)
        else:
            tok, segments, base = self.encode(all_ids), [], 0
            for s in range(self.streams):
                for first, num, k in spans[s]:
                    words = [] if k is None else range(k * self.max_tokens + 1, k * self.max_tokens + len(all_ids[k]) - 1)
                    segments.append((base + first - self.covered[s], num, list(words)))
                base += counts[s]
            # every row belongs to one segment, so the output needs no clearing
            rows = ops.text_spread_rows(tok, segments, total, out=torch.empty((total, self.hidden), device=self.device))
        self.covered = [c + n for c, n in zip(self.covered, counts)]
        return rows, counts

    @torch.no_grad()
    def push(self, sentences, upto=None):
        return self._run(self.check_push(sentences, upto))
