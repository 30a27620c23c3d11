"""Streaming inference: the causal TCN run a few frames at a time over device-side rings of past frames, and LFAN or CAN on
top.

Everything in LFAN is causal or per frame (the TCN pads left only, eval BatchNorm1d is a per-row affine, the cross-modal
attention mixes modalities and not time, LayerNorm and the regressor are per row), so frame t's output is a function of frames
<= t: pushing the frames of a sequence in any chunking returns what the whole-sequence forward returns.  The same holds for CAN
(the same TCN front; AttentionFusion, fc1, eval bn1 and fc2 work row by row).  JMT / MT attend over time and cannot stream
this way; ``window_stream.WindowStream`` runs them, and the evaluator's window rule for all four heads, on live streams.

State of one ``TemporalBlock`` for S streams (csrc/tcn_stream.hip): ``xring`` [S, R, Cin] holds its past inputs and ``hring``
[S, R, Cout] its past first-conv activations, fp32 channels-last, R the power of two >= (k - 1) d + max_new.  Each stream
advances on its own: the host keeps one integer per stream (frames pushed so far), which gives that stream's write position in
every ring; a reset stream's rings are zero, which is the reference's left zero-pad.  While all streams stand at one position a
dense push runs the lockstep launches (one ``head`` per ring); otherwise, and for every ragged push, the host uploads a row
table (stream and position of each new row) that all launches of the push share.  The bits are the same either way.  Per push
of up to max_new frames per stream a block costs two launches:

  phase A   hring[new] = leaky(conv(xring) + b1)
  phase B   next block's xring[new] (or the dense output) = leaky(leaky(conv(hring) + b2) + res(xring[new]))

An output value depends on its own stream's history only: not on S, c, the ring position or the neighbouring streams.
"""
import torch

from . import ops
from .fusion_heads import BN_EPS as CAN_BN_EPS, BN_MOMENTUM as CAN_BN_MOMENTUM, CAN
from .lfan import BN_EPS, BN_MOMENTUM, LFAN, LN_EPS, REGRESSION, _packed
from .temporal_convnet import TemporalConvNet


def ring_frames(k, dil, max_new):
    """Smallest power of two that holds the (k - 1) d frames of history a conv reaches back plus ``max_new`` new ones."""
    return ops.pow2_at_least((k - 1) * dil + max_new)


class _Lockstep(tuple):
    """(pos, c, out_pos): where the rows of a push sit when all streams stand at frame count ``pos`` and bring ``c`` frames.
    Every ring's head is ``pos & (R - 1)``; the ring a block leaves its output in stands at ``out_pos`` (``block_push``)."""

    def append(self, x, ring):
        ops.tcn_stream_append(x, ring, self[0] & (ring.shape[1] - 1))

    def conv(self, ring, w, b, k, dil, slope, out_ring, out_dense=None, res_ring=None, res_w=None, res_bias=None):
        pos, c, out_pos = self
        if res_ring is None:   # a block's first conv writes the block's own hring, which stands at pos
            out_pos = pos
        ops.tcn_stream_conv(ring, pos & (ring.shape[1] - 1), c, w, b, k, dil, res_ring=res_ring,
                            res_head=0 if res_ring is None else pos & (res_ring.shape[1] - 1), res_w=res_w, res_bias=res_bias,
                            out_ring=out_ring, out_head=0 if out_ring is None else out_pos & (out_ring.shape[1] - 1),
                            out_dense=out_dense, slope=slope)


class _Rows(tuple):
    """(row_stream, row_pos, max_count): where they sit when each row names its stream and position, the table of
    ``ops.stream_row_table`` and the most rows any one stream has in it."""

    def append(self, x, ring):
        ops.tcn_stream_append_rows(x, ring, *self)

    def conv(self, ring, w, b, k, dil, slope, out_ring, out_dense=None, res_ring=None, res_w=None, res_bias=None):
        ops.tcn_stream_conv_rows(ring, *self, w, b, k, dil, res_ring=res_ring, res_w=res_w, res_bias=res_bias, out_ring=out_ring,
                                 out_dense=out_dense, slope=slope)


def _block(pack, xring, hring, place, out_ring, out_dense, slope):
    """Phase A and phase B of one block over the rows ``place`` names, already written to ``xring``."""
    k, dil = pack["k"], pack["dil"]
    place.conv(xring, pack["w1"], pack["b1"], k, dil, slope, hring)
    place.conv(hring, pack["w2"], pack["b2"], k, dil, slope, out_ring, out_dense, xring, pack["dsw"], pack["dsb"])


def block_push(pack, xring, hring, pos, c, out_ring=None, out_pos=0, out_dense=None, slope=ops.LEAKY_SLOPE):
    """The two launches of one block over the ``c`` frames already written to ``xring`` at frame count ``pos``.
    ``pack``: dict(k, dil, w1, b1, w2, b2, dsw, dsb) with packed filters (``dsw`` None: identity residual)."""
    _block(pack, xring, hring, _Lockstep((pos, c, out_pos)), out_ring, out_dense, slope)


def block_push_rows(pack, xring, hring, row_stream, row_pos, max_count, out_ring=None, out_dense=None, slope=ops.LEAKY_SLOPE):
    """``block_push`` over the rows of a row table (``ops.stream_row_table``) already written to ``xring``: the same two
    launches, each stream at its own position."""
    _block(pack, xring, hring, _Rows((row_stream, row_pos, max_count)), out_ring, out_dense, slope)


def _check_tensor(x, name):
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32):
        raise ValueError(f"{name}: expected a float32 tensor on the GPU, got "
                         f"{(x.dtype, x.device) if torch.is_tensor(x) else type(x)}")


def _check_rows(x, name, streams, channels):
    _check_tensor(x, name)
    if x.dim() != 3 or x.shape[0] != streams or x.shape[2] != channels or x.shape[1] < 1:
        raise ValueError(f"{name}: expected [{streams} streams, c >= 1 new frames, {channels}], got {tuple(x.shape)}")


def _check_counts(counts, streams, max_new):
    """``counts``: how many new frames each of ``streams`` streams brings, 0 .. ``max_new`` each.  Returns them as ints."""
    try:
        counts = [int(c) for c in counts]
    except TypeError:
        raise ValueError(f"counts: expected a sequence of {streams} ints, got {type(counts).__name__}") from None
    if len(counts) != streams:
        raise ValueError(f"counts: expected one count per stream ({streams}), got {len(counts)}")
    for s, c in enumerate(counts):
        if not 0 <= c <= max_new:
            raise ValueError(f"counts: stream {s} brings {c} frames, outside 0 .. max_new = {max_new}")
    return counts


def _check_packed(x, name, rows, tail):
    """x [M, *tail] with M = ``rows``, the sum of the counts."""
    _check_tensor(x, name)
    if tuple(x.shape[1:]) != tuple(tail) or x.dim() != 1 + len(tail):
        raise ValueError(f"{name}: expected [M, {', '.join(str(t) for t in tail)}], got {tuple(x.shape)}")
    if x.shape[0] != rows:
        raise ValueError(f"{name}: {x.shape[0]} rows for counts that sum to {rows}")


class TCNStream:
    """``TemporalConvNet`` in eval mode, a few frames at a time, for ``streams`` parallel sequences.  Every stream has its
    own write position: ``push_rows`` advances all of them by the same c frames, ``push_ragged`` each by its own count."""

    def __init__(self, net, streams, max_new=32):
        if not isinstance(net, TemporalConvNet):
            raise TypeError(f"TCNStream needs a TemporalConvNet, got {type(net).__name__}")
        if streams < 1 or max_new < 1:
            raise ValueError(f"streams = {streams}, max_new = {max_new}: both must be >= 1")
        p = next(net.parameters())
        if p.device.type != "cuda":
            raise RuntimeError("TCNStream runs on the HIP kernels only: move the module to a GPU (no CPU fallback)")
        self.net, self.streams, self.max_new, self.device = net, streams, max_new, p.device
        alloc = (lambda shape: torch.zeros(shape, device=self.device, dtype=torch.float32))
        self.ring_frames = [ring_frames(b.k, b.dilation, max_new) for b in net.network]
        self.xrings = [alloc((streams, r, b.cin)) for b, r in zip(net.network, self.ring_frames)]
        self.hrings = [alloc((streams, r, b.cout)) for b, r in zip(net.network, self.ring_frames)]
        self.cin, self.cout = net.network[0].cin, net.network[-1].cout
        self.frames_seen = [0] * streams
        self._pos = [0] * streams   # frames pushed per stream since construction: stream s writes ring l at _pos[s] & (R_l - 1)
        self._packs, self._key = None, None

    def _pack(self):
        key = tuple((p.data_ptr(), p._version) for p in self.net.parameters())
        if self._packs is None or key != self._key:
            packs = []
            for b in self.net.network:
                w1, _ = ops.weight_norm_fwd(b.conv1.weight_v.detach(), b.conv1.weight_g.detach())
                w2, _ = ops.weight_norm_fwd(b.conv2.weight_v.detach(), b.conv2.weight_g.detach())
                ds = b.downsample
                packs.append({"k": b.k, "dil": b.dilation,
                              "w1": ops.pack_tcn_stream_weight(w1), "b1": b.conv1.bias.detach(),
                              "w2": ops.pack_tcn_stream_weight(w2), "b2": b.conv2.bias.detach(),
                              "dsw": ops.pack_tcn_stream_weight(ds.weight) if ds is not None else None,
                              "dsb": ds.bias.detach() if ds is not None else None})
            self._packs, self._key = packs, key
        return self._packs

    def reset(self, streams=None):
        """Forget the past of ``streams`` (indices; None = all): their rings become the zero left-pad again.  Their write
        positions stay where they are: a zeroed ring is an empty past at any position."""
        idx = list(range(self.streams)) if streams is None else [int(s) for s in streams]
        for s in idx:
            if not 0 <= s < self.streams:
                raise IndexError(f"stream {s} of {self.streams}")
        if not idx:
            return
        sel = torch.tensor(idx, device=self.device)
        for ring in self.xrings + self.hrings:
            ring.index_fill_(0, sel, 0.0)
        for s in idx:
            self.frames_seen[s] = 0

    def _check_eval(self):
        if self.net.training:
            raise RuntimeError("TCNStream: the net is in train mode (dropout); call .eval() first")

    def _push(self, x, place, dense):
        """x: the new frames, stream-major, the rows ``place`` names ([S, c, Cin] in lockstep, [M, Cin] for a table) -> dense
        [M, Cout]: one append and two launches per block."""
        last = len(self.xrings) - 1
        place.append(x, self.xrings[0])
        for lvl, pack in enumerate(self._pack()):
            _block(pack, self.xrings[lvl], self.hrings[lvl], place, self.xrings[lvl + 1] if lvl < last else None,
                   dense if lvl == last else None, ops.LEAKY_SLOPE)

    def _table(self, counts):
        """One table upload for a push in which stream s brings ``counts[s]`` frames, each stream at its own position."""
        return _Rows(ops.stream_row_table(self._pos, counts, self.device) + (max(counts),))

    def _advance(self, counts):
        self._pos = [p + c for p, c in zip(self._pos, counts)]
        self.frames_seen = [f + c for f, c in zip(self.frames_seen, counts)]

    @torch.no_grad()
    def push_rows(self, x):
        """x [S, c, Cin]: the next c frames of every stream -> [S, c, Cout], the net's output at those frames.  While the
        streams share one position this is the lockstep launches; after ragged pushes it goes through the row table, with
        the same bits."""
        self._check_eval()
        _check_rows(x, "x", self.streams, self.cin)
        x = x.contiguous()
        c = x.shape[1]
        out = torch.empty((self.streams, c, self.cout), device=self.device, dtype=torch.float32)
        for c0 in range(0, c, self.max_new):
            n = min(self.max_new, c - c0)
            whole = n == c
            chunk = x if whole else x[:, c0:c0 + n].contiguous()
            dense = out if whole else torch.empty((self.streams, n, self.cout), device=self.device, dtype=torch.float32)
            if len(set(self._pos)) == 1:
                place = _Lockstep((self._pos[0], n, self._pos[0]))
            else:
                place, chunk = self._table([n] * self.streams), chunk.view(self.streams * n, self.cin)
            self._push(chunk, place, dense.view(self.streams * n, self.cout))
            if not whole:
                out[:, c0:c0 + n] = dense
            self._advance([n] * self.streams)
        return out

    @torch.no_grad()
    def push_ragged(self, x, counts):
        """x [M, Cin]: ``counts[s]`` (0 .. max_new) new frames of stream s, packed stream-major in ascending stream order,
        each stream's frames in time order, M = sum(counts) -> [M, Cout] in the same row order.  A stream that brings nothing
        is left as it is; all-zero counts return an empty [0, Cout] without a launch."""
        self._check_eval()
        counts = _check_counts(counts, self.streams, self.max_new)
        _check_packed(x, "x", sum(counts), (self.cin,))
        out = torch.empty((x.shape[0], self.cout), device=self.device, dtype=torch.float32)
        if x.shape[0]:
            self._push(x.contiguous(), self._table(counts), out)
            self._advance(counts)
        return out


class _ModelStream:
    """What ``LFANStream`` and ``CANStream`` share: one ``TCNStream`` per modality behind the model's encoders, the key, shape
    and count checks, and the four ways to push.  A subclass names the model class it runs, the order in which the TCN outputs
    meet its head, and the head itself on rows."""

    _model_class, _needs = None, ""

    def __init__(self, model, streams, max_new=32, encoder_batch=8):
        name = type(self).__name__
        if encoder_batch is not None and encoder_batch < 1:
            raise ValueError(f"encoder_batch = {encoder_batch}: a positive number of frames per encoder call, or None")
        self.encoder_batch = encoder_batch
        if not isinstance(model, self._model_class):
            raise TypeError(f"{name} needs {self._needs} (JMT / MT attend over time and are not causal), got {type(model).__name__}")
        if model.training:
            raise RuntimeError(f"{name}: the model is in train mode; batch statistics are undefined frame by frame -- call .eval()")
        self.model, self.streams, self.max_new = model, streams, max_new
        self.modalities = list(self._modalities(model))
        self.tcn = {m: TCNStream(model.temporal[m], streams, max_new) for m in self.modalities}

    @property
    def frames_seen(self):
        return self.tcn[self.modalities[0]].frames_seen

    @property
    def ring_frames(self):
        return {m: t.ring_frames for m, t in self.tcn.items()}

    def reset(self, streams=None):
        for t in self.tcn.values():
            t.reset(streams)

    def _cin(self, m):
        """The embedding dim of modality m: what its TCN takes."""
        return self.tcn[m].cin

    def _check_keys(self, X):
        model = self.model
        if model.training:
            raise RuntimeError(f"{type(self).__name__}: the model is in train mode; batch statistics are undefined frame by frame "
                               "-- call .eval()")
        for m in X:
            if m not in model.temporal:
                raise KeyError(m)
        for m in self.modalities:
            if m not in X:
                raise KeyError(m)

    def _check_input(self, m, x):
        _check_tensor(x, m)
        s = self.streams
        if m == "video":
            ok, c = x.dim() == 5 and x.shape[0] == s and x.shape[2] == 3, x.shape[1] if x.dim() == 5 else 0
            want = f"[{s}, c, 3, H, W]"
        elif m == "logmel":
            ok, c = x.dim() == 4 and x.shape[0] == s and x.shape[1] == 64 and x.shape[3] == 96, x.shape[2] if x.dim() == 4 else 0
            want = f"[{s}, 64, c, 96]"
        else:
            e = self._cin(m)
            ok, c = x.dim() == 4 and x.shape[0] == s and x.shape[1] == 1 and x.shape[3] == e, x.shape[2] if x.dim() == 4 else 0
            want = f"[{s}, 1, c, {e}]"
        if not ok or c < 1:
            raise ValueError(f"{m}: expected {want} for {s} streams, got {tuple(x.shape)}")
        return c

    def _check_packed_input(self, m, x, rows):
        if m == "video":
            hw = tuple(x.shape[2:]) if torch.is_tensor(x) and x.dim() == 4 else ("H", "W")
            _check_packed(x, m, rows, (3,) + hw)
        elif m == "logmel":
            _check_packed(x, m, rows, (64, 96))
        else:
            _check_packed(x, m, rows, (self._cin(m),))

    @staticmethod
    def _one_count(cs):
        if len(set(cs.values())) != 1:
            raise ValueError(f"the modalities bring different numbers of new frames: {cs}")
        return next(iter(cs.values()))

    def _in_groups(self, encoder, frames):
        """``encoder`` over ``frames`` [N, ...] in calls of exactly ``encoder_batch`` frames, the last call filled up with zero
        frames whose rows are dropped.  The conv kernels pick their tile variant, and with it the order of their K sums, from
        the number of rows of a call; with every call the same size, a frame's embedding is the same bits however many frames
        the push brought.  ``encoder_batch`` None: one call per push (fewer launches; the bits then depend on the push size)."""
        g, n = self.encoder_batch, frames.shape[0]
        if g is None:
            return encoder(frames)
        outs = []
        for i in range(0, n, g):
            part = frames[i:i + g]
            if part.shape[0] < g:
                full = frames.new_zeros((g,) + tuple(frames.shape[1:]))
                full[:part.shape[0]] = part
                part = full
            outs.append(encoder(part.contiguous()))
        return torch.cat(outs)[:n]

    def _encode(self, X, packed):
        """The encoders as the model's forward runs them, ``encoder_batch`` frames per call: X[m] -> rows
        [M, embedding_dim[m]] (M = S c, stream-major)."""
        model = self.model
        if "visual" in model.spatial:
            model.spatial["visual"].backbone.check_sync_release()
        feats = {}
        for m in X:
            x = X[m]
            if m == "video":
                vis = model.spatial["visual"]
                vis.backbone.dropout_seed = model.dropout_seed
                feats[m] = self._in_groups(lambda f: vis(f, None), x if packed else x.reshape(-1, *x.shape[2:]))
            elif m == "logmel":
                frames = x.permute(0, 2, 1) if packed else x.permute(0, 2, 3, 1)
                feats[m] = self._in_groups(model.spatial["audio"], frames.contiguous().view(-1, 96, 64))
            else:
                feats[m] = x.reshape(-1, x.shape[-1])
        return feats

    def _run(self, feats, c=None, counts=None):
        """feats[m] [M, E_m] rows -> logits: [S, c, n_cls] of a dense push, [M, n_cls] of a ragged one."""
        order = self._order(feats)
        if counts is None:
            t = [self.tcn[m].push_rows(feats[m].detach().view(self.streams, c, -1)).view(self.streams * c, -1) for m in order]
        else:
            t = [self.tcn[m].push_ragged(feats[m].detach(), counts) for m in order]
        logits = self._head(order, t)
        out = logits if counts is not None else logits.view(self.streams, c, -1)
        return ops.tanh_fwd(out) if self.model.task == REGRESSION else out

    def _nothing(self):
        """No stream brought a frame: no rows, no launch."""
        return torch.empty((0, self._n_out()), device=self.tcn[self.modalities[0]].device, dtype=torch.float32)

    @torch.no_grad()
    def push(self, X):
        """X keyed like the model's ``forward`` dict with c new frames in place of L (video [S,c,3,H,W], vggish [S,1,c,128],
        bert [S,1,c,768], logmel [S,64,c,96]) -> logits [S, c, n_cls] (tanh-ed for REGRESSION).  X is left as it is."""
        self._check_keys(X)
        c = self._one_count({m: self._check_input(m, X[m]) for m in X})
        return self._run(self._encode(X, packed=False), c=c)

    @torch.no_grad()
    def push_features(self, F):
        """F[m] [S, c, embedding_dim[m]]: per-modality embeddings of the next c frames (``video``: the 512-d encoder output)
        -> logits [S, c, n_cls].  Skips the encoders."""
        self._check_keys(F)
        for m in F:
            _check_rows(F[m], m, self.streams, self._cin(m))
        c = self._one_count({m: F[m].shape[1] for m in F})
        return self._run({m: F[m].contiguous().view(self.streams * c, -1) for m in F}, c=c)

    @torch.no_grad()
    def push_ragged(self, X, counts):
        """Stream s brings ``counts[s]`` (0 .. max_new) new frames.  X[m] holds the M = sum(counts) frames without the stream
        axis, stream-major in ascending stream order, each stream's frames in time order: video [M,3,H,W], logmel [M,64,96],
        any other modality [M, embedding_dim[m]] -> logits [M, n_cls] in the same row order (tanh-ed for REGRESSION)."""
        self._check_keys(X)
        counts = _check_counts(counts, self.streams, self.max_new)
        for m in X:
            self._check_packed_input(m, X[m], sum(counts))
        if not sum(counts):
            return self._nothing()
        return self._run(self._encode(X, packed=True), counts=counts)

    @torch.no_grad()
    def push_features_ragged(self, F, counts):
        """``push_ragged`` on per-modality embeddings F[m] [M, embedding_dim[m]]: skips the encoders."""
        self._check_keys(F)
        counts = _check_counts(counts, self.streams, self.max_new)
        for m in F:
            _check_packed(F[m], m, sum(counts), (self._cin(m),))
        if not sum(counts):
            return self._nothing()
        return self._run({m: F[m].contiguous() for m in F}, counts=counts)


class LFANStream(_ModelStream):
    """An eval-mode ``LFAN`` on live streams: ``push`` the next c frames of ``streams`` sequences, get their logits;
    ``push_ragged`` when the streams bring different numbers of frames.  The model's ``example_length`` plays no part."""

    _model_class, _needs = LFAN, "an LFAN"

    @staticmethod
    def _modalities(model):
        return model.modality

    def _order(self, feats):
        return self.modalities

    def _n_out(self):
        return self.model.regressor.weight.shape[0]

    def _head(self, mods, t):
        model, rows = self.model, t[0].shape[0]
        attn, norm1 = model.fusion.layers.self_attn, model.fusion.layers.norm1
        # the head of LFANHeadFunction.forward in eval mode, on the same row kernels; BatchNorm of the leader and the
        # LayerNorm write straight into their column slices of the regressor's input
        enc0, d = t[0].shape[1], attn.num_heads * attn.head_dim * len(mods)
        z = torch.empty((rows, enc0 + d), device=t[0].device, dtype=torch.float32)
        qkvs = []
        for i, m in enumerate(mods):
            bn, proj = model.bn[m], attn.qkv_proj[m]
            y, _, _ = ops.bn_rows_fwd(t[i], bn.weight, bn.bias, bn.running_mean, bn.running_var, False, BN_EPS, BN_MOMENTUM,
                                      out=z[:, :enc0] if i == 0 else None)
            qkvs.append(ops.linear(y, _packed(proj.weight), bias=proj.bias))
        vals, _ = ops.lfan_attn_fwd(qkvs, attn.num_heads, attn.head_dim)
        o = ops.linear(vals, _packed(attn.o_proj.weight), bias=attn.o_proj.bias)
        ops.layernorm_fwd(o, norm1.weight, norm1.bias, eps=LN_EPS, out=z[:, enc0:], save=False)
        return ops.linear(z, _packed(model.regressor.weight), bias=model.regressor.bias)


class CANStream(_ModelStream):
    """An eval-mode ``CAN`` on live streams, with ``LFANStream``'s surface.  CAN is as causal as LFAN: the same TCN front, and
    behind it ``AttentionFusion``, ``fc1``, eval ``bn1`` and ``fc2`` all work row by row.  As in ``CAN.forward``, the caller's
    key order pairs the modalities with ``fuse.attn[i]``."""

    _model_class, _needs = CAN, "a CAN"

    @staticmethod
    def _modalities(model):
        return model.modalities

    def _order(self, feats):
        return list(feats)

    def _n_out(self):
        return self.model.fc2.weight.shape[0]

    def _head(self, mods, t):
        model, rows = self.model, t[0].shape[0]
        fuse, bn1 = model.fuse, model.bn1
        # CAN.forward's tail in eval mode on the same row kernels; the per-modality projections write straight into their
        # column slices of the concatenation
        width = fuse.attn[0].weight.shape[0]
        cat = torch.empty((rows, width * len(mods)), device=t[0].device, dtype=torch.float32)
        for i, m in enumerate(mods):
            bn, lin = model.bn[m], fuse.attn[i]
            y, _, _ = ops.bn_rows_fwd(t[i], bn.weight, bn.bias, bn.running_mean, bn.running_var, False, CAN_BN_EPS,
                                      CAN_BN_MOMENTUM)
            ops.linear(y, _packed(lin.weight), bias=lin.bias, out=cat[:, i * width:(i + 1) * width])
        gate = ops.linear(cat, _packed(fuse.weights.weight), bias=fuse.weights.bias)
        c, _ = ops.softmax_gate_fwd(gate, cat)
        c = ops.linear(c, _packed(model.fc1.weight), bias=model.fc1.bias)
        c, _, _ = ops.bn_rows_fwd(c, bn1.weight, bn1.bias, bn1.running_mean, bn1.running_var, False, CAN_BN_EPS, CAN_BN_MOMENTUM)
        return ops.linear(ops.leaky_relu(c), _packed(model.fc2.weight), bias=model.fc2.bias)


_TIME_AXIS = {"video": 1}   # every other modality: axis 2


def stream_forward(model, X, chunk=32, encoder_batch=8):
    """A whole clip or video of any length T through an eval-mode LFAN or CAN, causally, ``chunk`` frames at a time:
    [B, T, n_cls], what ``model(X)`` returns when it is built with ``example_length = T``.  X is left as it is."""
    first = next(iter(X.values()))
    stream = (CANStream if isinstance(model, CAN) else LFANStream)(model, first.shape[0], max_new=chunk,
                                                                   encoder_batch=encoder_batch)
    stream._check_keys(X)
    total = {m: x.shape[_TIME_AXIS.get(m, 2)] for m, x in X.items()}
    if len(set(total.values())) != 1:
        raise ValueError(f"the modalities have different lengths: {total}")
    total = next(iter(total.values()))
    outs = [stream.push({m: x.narrow(_TIME_AXIS.get(m, 2), t0, min(chunk, total - t0)) for m, x in X.items()})
            for t0 in range(0, total, chunk)]
    return outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)
