"""Windowed live inference: the evaluator's window rule on live streams, for LFAN, CAN, JMT and MT.

The reference scores a long video by its window rule (``Trainer.inference_forward_windows``, ``trainer.windowing``): a window of
W frames every H frames plus a tail window ``x[-W:]``, every window's TCN starting from zero padding, the outputs summed in
window order and divided by the overlap count.  ``WindowStream`` does the same on streams that are still running, so a live
session gives the numbers the model was validated with (LFAN), and a model that attends over time (JMT / MT, whose forward
needs a whole window) can run live at all.  The reference itself evaluates JMT / MT on whole videos in one forward; windowed
live inference is this project's live counterpart for them, not a reference protocol.  For LFAN it is the reference's.

The rule (``window_schedule``, a pure function of ints).  A stream has received N frames, 1 <= H <= W.
Regular window i covers [i H, i H + W) and is complete once i H + W <= N.  The offline rule for a final length n >= N may still
add the tail window [n - W, n), which reaches no frame below N - W.  So frame f is final exactly when f < N - W: every regular
window over it is complete and no tail can reach it.  A live stream emits frame f once W more frames have followed it: the
latency of the protocol, W / fps seconds (10 s at W = 300 and 30 fps).  ``finish`` knows n: it runs the tail window when
n >= W and (n - W) % H != 0, the single short window [0, n) when n < W, and emits the rest.  Emitted values are
``eval_device.stitch_windows`` of the same window outputs on ``windowing(range(n), W, H)``, bit for bit.

State.  Per modality a ring [S, Re, E_m] of encoder embeddings, Re the power of two >= W + ``max_new`` (a window that a push
completes starts less than W + ``max_new`` frames before the push's last frame), written with ``ops.tcn_stream_append_rows``
and read back with ``ops.gather_rows``: every frame goes through its encoder ONCE, where the offline evaluator encodes a
frame once per window that covers it (about W / H times).  ``wring`` [S, K, W, n_out] holds each stream's last window outputs
(csrc/window_stream.hip): regular window i in slot i % (K - 1), the tail or short window in slot K - 1, K = ``ring_windows(W,
H)`` = ceil(W / H) + 1, S K W n_out 4 bytes in all.

A window forward is the model's own eval forward behind the encoders (``forward_rows`` of the model: the TCNs from zero
padding, eval BatchNorm, the head; tanh per window for REGRESSION, as offline) on the W gathered rows.  JMT / MT take one
window per call: their final attention spans all tokens of a call (the reference asserts bsz == 1 at inference).  LFAN and CAN
work row by row behind the TCN, so ``window_batch`` windows of any streams share a call; every call carries exactly
``window_batch`` windows (unused places repeat the first and are dropped), because the conv kernels key their split of K on
the row count of a call.  With ``window_batch`` = 1 a call is the offline evaluator's call with ``eval_frame_budget`` = W.
"""
import torch

from . import ops
from .fusion_heads import CAN, JMT
from .lfan import LFAN
from .streaming import _ModelStream, _TIME_AXIS


def ring_windows(window_length, hop_length):
    """K, the slots of a stream in ``wring``: ceil(W / H) regular slots and the tail's.  Before window j runs, the frames
    below j H are emitted (they are final: j H + W <= N); the window whose slot it takes, j - ceil(W / H), ends at
    j H - ceil(W / H) H + W <= j H.  One slot fewer fails: when window j completes, frame j H is unemitted and windows
    j - ceil(W / H) + 1 .. j all cover it."""
    return -(-window_length // hop_length) + 1


def window_schedule(seen, new, window_length, hop_length, done, final=None):
    """What a stream that had ``seen`` frames and ``done`` regular windows run owes after ``new`` more frames: (the starts of
    the windows to run, in order; emit-up-to: frames below it are final).  ``final``: the stream ends with that many frames
    (``seen + new``); the tail window or the short window closes the list and every frame is emitted.  Python ints, no
    torch: the one place the window rule lives."""
    w, h, n = int(window_length), int(hop_length), int(seen) + int(new)
    if w < 1 or not 1 <= h <= w:
        raise ValueError(f"window_length = {window_length}, hop_length = {hop_length}: need 1 <= hop_length <= window_length")
    if seen < 0 or new < 0 or done < 0:
        raise ValueError(f"seen = {seen}, new = {new}, done = {done}: none may be negative")
    complete = (n - w) // h + 1 if n >= w else 0
    starts = [i * h for i in range(done, complete)]
    if final is None:
        return starts, max(n - w, 0)
    if int(final) != n:
        raise ValueError(f"final = {final}: the stream has {n} frames")
    if n >= w and (n - w) % h:
        starts.append(n - w)
    elif 0 < n < w:
        starts.append(0)
    return starts, n


def emit_before(start, window_length, hop_length, emitted):
    """Up to which frame a stream that has emitted ``emitted`` frames must emit BEFORE its regular window at ``start`` runs:
    that window takes the slot of window start / H - (K - 1), whose frames must all be out; the frames below ``start`` are
    final by then (start + W <= N), so they can go.  ``emitted`` itself when nothing has to.  Python ints."""
    old = start // hop_length - (ring_windows(window_length, hop_length) - 1)
    return start if old >= 0 and emitted < old * hop_length + window_length else emitted


class WindowStream(_ModelStream):
    """An eval-mode LFAN, CAN, JMT or MT on ``streams`` live streams under the evaluator's window rule, with the surface of
    ``LFANStream``: ``push``, ``push_features``, ``push_ragged`` and ``push_features_ragged`` take what theirs take and return
    (logits [P, n_out], counts): the frames that became final in this call, stream-major, each stream's in time order,
    ``counts[s]`` of them of stream s (tanh-ed per window for REGRESSION).  ``finish(streams=None)`` returns the same pair for
    the rest of those streams (the tail or short window) and resets them; ``reset(streams=None)`` forgets them.  Host lists:
    ``frames_seen``, ``emitted``, ``windows_done`` (regular windows run).  A CAN pairs the modalities with ``fuse.attn[i]``
    in the key order of the latest push, as ``CAN.forward`` does with its caller's dict."""

    frames_seen = ring_frames = None   # plain attributes here (``_ModelStream`` derives them from its TCN streams)

    def __init__(self, model, streams, window_length, hop_length, max_new=32, encoder_batch=8, window_batch=1):
        if not isinstance(model, (LFAN, CAN, JMT)):
            raise TypeError(f"WindowStream needs an LFAN, a CAN, a JMT or an MT, got {type(model).__name__}")
        w, h = int(window_length), int(hop_length)
        if w < 1 or h < 1 or h > w:
            raise ValueError(f"window_length = {window_length}, hop_length = {hop_length}: need 1 <= hop_length <= window_length")
        if int(streams) < 1 or int(max_new) < 1 or int(window_batch) < 1:
            raise ValueError(f"streams = {streams}, max_new = {max_new}, window_batch = {window_batch}: all must be >= 1")
        if encoder_batch is not None and encoder_batch < 1:
            raise ValueError(f"encoder_batch = {encoder_batch}: a positive number of frames per encoder call, or None")
        if isinstance(model, JMT) and int(window_batch) != 1:
            raise ValueError(f"window_batch = {window_batch}: a JMT / MT attends over all tokens of a call, one window per call")
        if model.training:
            raise RuntimeError("WindowStream: the model is in train mode; batch statistics are undefined window by window "
                               "-- call .eval()")
        p = next(model.parameters())
        if p.device.type != "cuda":
            raise RuntimeError("WindowStream runs on the HIP kernels only: move the model to a GPU (no CPU fallback)")
        self.model, self.streams, self.max_new, self.encoder_batch = model, int(streams), int(max_new), encoder_batch
        self.window_length, self.hop_length, self.window_batch, self.device = w, h, int(window_batch), p.device
        self.modalities = list(model.modality if isinstance(model, LFAN) else model.modalities)
        self._order_keys = list(self.modalities)
        self.dims = {m: model.temporal[m].network[0].cin for m in self.modalities}
        for m, e in self.dims.items():
            if e % 4:
                raise ValueError(f"{m}: embedding dim {e} is not a multiple of 4 (the row gather moves float4)")
        self.n_out = (model.regressor if isinstance(model, LFAN) else model.fc2).weight.shape[0]
        self.ring_frames = ops.pow2_at_least(w + self.max_new)
        self.ring_windows = ring_windows(w, h)
        self.rings = {m: torch.zeros((self.streams, self.ring_frames, e), device=self.device, dtype=torch.float32)
                      for m, e in self.dims.items()}
        self.wring = torch.zeros((self.streams, self.ring_windows, w, self.n_out), device=self.device, dtype=torch.float32)
        self.frames_seen, self.emitted, self.windows_done = [0] * self.streams, [0] * self.streams, [0] * self.streams
        self._tail = [-1] * self.streams

    # ------------------------------------------------------------------------------------------------ what _ModelStream asks
    def _cin(self, m):
        return self.dims[m]

    def _n_out(self):
        return self.n_out

    def _nothing(self):
        return torch.empty((0, self.n_out), device=self.device, dtype=torch.float32), [0] * self.streams

    def _indices(self, streams):
        idx = list(range(self.streams)) if streams is None else [int(s) for s in streams]
        for s in idx:
            if not 0 <= s < self.streams:
                raise IndexError(f"stream {s} of {self.streams}")
        return sorted(set(idx))

    def reset(self, streams=None):
        """Forget ``streams`` (indices; None = all).  Nothing on the device needs clearing: a ring slot is read only after
        the stream has written it again."""
        for s in self._indices(streams):
            self.frames_seen[s] = self.emitted[s] = self.windows_done[s] = 0
            self._tail[s] = -1

    # ------------------------------------------------------------------------------------------------ windows
    def _forward_windows(self, wins):
        """wins: (stream, start, length) of windows of one length -> their outputs [len(wins), length, n_out]: one call of the
        model's ``forward_rows`` per ``window_batch`` windows, each exactly that many."""
        g, length, mask, outs = self.window_batch, wins[0][2], self.ring_frames - 1, []
        for i in range(0, len(wins), g):
            part = wins[i:i + g]
            full = part + [part[0]] * (g - len(part))
            index = torch.tensor([s * self.ring_frames + ((start + r) & mask) for s, start, _ in full for r in range(length)],
                                 dtype=torch.int64, device=self.device)
            rows = {m: ops.gather_rows(self.rings[m].view(-1, self.dims[m]), index) for m in self._order_keys}
            out = self.model.forward_rows(rows, g, length)
            outs.append((out[0] if isinstance(out, tuple) else out)[:len(part)])
        return outs[0] if len(outs) == 1 else torch.cat(outs)

    def _emit(self, upto, parts):
        """Stitch frames ``emitted[s]`` .. ``upto[s]`` - 1 of every stream in ``upto`` (one launch) into ``parts[s]``."""
        rows = [(s, f) for s in sorted(upto) for f in range(self.emitted[s], upto[s])]
        if not rows:
            return
        out, at = ops.window_stitch_stream(self.wring, self.hop_length, rows, self.windows_done, self._tail), 0
        for s in sorted(upto):
            c = upto[s] - self.emitted[s]
            if c > 0:
                parts[s].append(out[at:at + c])
                at, self.emitted[s] = at + c, upto[s]

    def _advance(self, counts, parts, final=()):
        """The frames of this step are in the rings: run the windows every stream owes, a round per window of a stream and in
        ascending order, and emit what became final.  ``final``: the streams that end here."""
        w, h, k = self.window_length, self.hop_length, self.ring_windows
        pending, target = {}, {}
        for s in range(self.streams):
            if counts[s] or s in final:
                n = self.frames_seen[s] + counts[s]
                starts, target[s] = window_schedule(self.frames_seen[s], counts[s], w, h, self.windows_done[s],
                                                    final=n if s in final else None)
                self.frames_seen[s] = n
                if starts:
                    pending[s] = starts
        while pending:
            turn = [(s, starts.pop(0)) for s, starts in sorted(pending.items())]
            pending = {s: starts for s, starts in pending.items() if starts}
            # a regular window takes the slot of window i - (K - 1): every frame of that one must have been emitted.  The
            # frames below a complete window's start are final, so they can go first
            early = {}
            for s, start in turn:
                if start % h == 0 and start + w <= self.frames_seen[s]:
                    early[s] = emit_before(start, w, h, self.emitted[s])
            self._emit(early, parts)
            by_length = {}
            for s, start in turn:
                by_length.setdefault(min(w, self.frames_seen[s] - start), []).append((s, start))
            for length, wins in sorted(by_length.items()):
                out = self._forward_windows([(s, start, length) for s, start in wins])
                for b, (s, start) in enumerate(wins):
                    regular = start % h == 0 and length == w
                    if regular:
                        i = start // h
                        if i != self.windows_done[s] or (i >= k - 1 and self.emitted[s] < (i - (k - 1)) * h + w):
                            raise RuntimeError(f"WindowStream: window {i} of stream {s} would overwrite unemitted frames")
                        slot, self.windows_done[s] = i % (k - 1), i + 1
                    else:
                        slot, self._tail[s] = k - 1, start
                    self.wring[s, slot, :length].copy_(out[b])
        self._emit(target, parts)

    def _hold(self, feats, counts):
        """feats[m] [M, E_m], stream-major: into the embedding rings at the streams' frame numbers."""
        row_stream, row_pos = ops.stream_row_table(self.frames_seen, counts, self.device)
        for m in self.modalities:
            ops.tcn_stream_append_rows(feats[m].detach().contiguous(), self.rings[m], row_stream, row_pos, max(counts))

    @staticmethod
    def _result(parts, nothing):
        flat = [p for per in parts for p in per]
        counts = [sum(p.shape[0] for p in per) for per in parts]
        return (torch.cat(flat) if len(flat) > 1 else flat[0]) if flat else nothing[0], counts

    def _run(self, feats, c=None, counts=None):
        """feats[m] [M, E_m] rows (a dense push: M = S c, stream-major) -> (logits [P, n_out], counts)."""
        self._order_keys = list(feats) if isinstance(self.model, CAN) else self.modalities
        parts = [[] for _ in range(self.streams)]
        if counts is not None:
            self._hold(feats, counts)
            self._advance(counts, parts)
        else:
            for c0 in range(0, c, self.max_new):
                n = min(self.max_new, c - c0)
                step = {m: x.view(self.streams, c, -1)[:, c0:c0 + n].reshape(self.streams * n, -1) for m, x in feats.items()}
                self._hold(step, [n] * self.streams)
                self._advance([n] * self.streams, parts)
        return self._result(parts, self._nothing())

    @torch.no_grad()
    def finish(self, streams=None):
        """``streams`` (indices; None = all) have ended: their tail window (n >= W and (n - W) % H != 0) or their short window
        (n < W) runs, the rest of their frames is emitted -> (logits, counts), and they are reset."""
        idx = self._indices(streams)
        self._check_keys(dict.fromkeys(self.modalities))
        parts = [[] for _ in range(self.streams)]
        self._advance([0] * self.streams, parts, final=set(idx))
        self.reset(idx)
        return self._result(parts, self._nothing())


def window_forward(model, X, window_length, hop_length, chunk=32, encoder_batch=8):
    """A whole video of any length T through an eval-mode LFAN, CAN, JMT or MT under the evaluator's window rule, ``chunk``
    frames at a time, every frame through its encoder once: [B, T, n_out], for an LFAN what
    ``Trainer.inference_forward_windows`` gives video by video.  The sibling of ``stream_forward``.  X is left as it is."""
    first = next(iter(X.values()))
    bsz = first.shape[0]
    stream = WindowStream(model, bsz, window_length, hop_length, max_new=chunk, encoder_batch=encoder_batch)
    stream._check_keys(X)
    total = {m: x.shape[_TIME_AXIS.get(m, 2)] for m, x in X.items()}
    if len(set(total.values())) != 1:
        raise ValueError(f"the modalities have different lengths: {total}")
    total = next(iter(total.values()))
    per = [[] for _ in range(bsz)]

    def collect(logits, counts):
        at = 0
        for s, c in enumerate(counts):
            per[s].append(logits[at:at + c])
            at += c

    for t0 in range(0, total, chunk):
        collect(*stream.push({m: x.narrow(_TIME_AXIS.get(m, 2), t0, min(chunk, total - t0)) for m, x in X.items()}))
    collect(*stream.finish())
    return torch.stack([torch.cat(p) for p in per])
