"""Streaming inference: the causal TCN run a few frames at a time over device-side rings of past frames, and LFAN on top.

Everything in LFAN is causal or per frame (the TCN pads left only, eval BatchNorm1d is a per-row affine, the cross-modal
attention mixes modalities and not time, LayerNorm and the regressor are per row), so frame t's output is a function of frames
<= t: pushing the frames of a sequence in any chunking returns what the whole-sequence forward returns.

State of one ``TemporalBlock`` for S streams (csrc/tcn_stream.hip): ``xring`` [S, R, Cin] holds its past inputs and ``hring``
[S, R, Cout] its past first-conv activations, fp32 channels-last, R the power of two >= (k - 1) d + max_new.  The streams advance
together, so one host integer (frames pushed so far) gives every ring's write position; a reset stream's rings are zero, which
is the reference's left zero-pad.  Per push of c <= max_new frames a block costs two launches:

  phase A   hring[new] = leaky(conv(xring) + b1)
  phase B   next block's xring[new] (or the dense output) = leaky(leaky(conv(hring) + b2) + res(xring[new]))

An output value depends on its own stream's history only: not on S, c, the ring position or the neighbouring streams.
"""
import torch

from . import ops
from .lfan import BN_EPS, BN_MOMENTUM, LFAN, LN_EPS, REGRESSION, _packed
from .temporal_convnet import TemporalConvNet


def ring_frames(k, dil, max_new):
    """Smallest power of two that holds the (k - 1) d frames of history a conv reaches back plus ``max_new`` new ones."""
    need, r = (k - 1) * dil + max_new, 1
    while r < need:
        r *= 2
    return r


def block_push(pack, xring, hring, pos, c, out_ring=None, out_pos=0, out_dense=None, slope=ops.LEAKY_SLOPE):
    """The two launches of one block over the ``c`` frames already written to ``xring`` at frame count ``pos``.
    ``pack``: dict(k, dil, w1, b1, w2, b2, dsw, dsb) with packed filters (``dsw`` None: identity residual)."""
    head = pos & (xring.shape[1] - 1)
    ops.tcn_stream_conv(xring, head, c, pack["w1"], pack["b1"], pack["k"], pack["dil"], out_ring=hring, out_head=head, slope=slope)
    ops.tcn_stream_conv(hring, head, c, pack["w2"], pack["b2"], pack["k"], pack["dil"], res_ring=xring, res_head=head,
                        res_w=pack["dsw"], res_bias=pack["dsb"], out_ring=out_ring,
                        out_head=out_pos & (out_ring.shape[1] - 1) if out_ring is not None else 0, out_dense=out_dense, slope=slope)


def _check_rows(x, name, streams, channels):
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32):
        raise ValueError(f"{name}: expected a float32 tensor on the GPU, got "
                         f"{(x.dtype, x.device) if torch.is_tensor(x) else type(x)}")
    if x.dim() != 3 or x.shape[0] != streams or x.shape[2] != channels or x.shape[1] < 1:
        raise ValueError(f"{name}: expected [{streams} streams, c >= 1 new frames, {channels}], got {tuple(x.shape)}")


class TCNStream:
    """``TemporalConvNet`` in eval mode, a few frames at a time, for ``streams`` parallel sequences."""

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
        self._pos = 0          # frames pushed since construction: ring l writes at _pos & (R_l - 1)
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
        """Forget the past of ``streams`` (indices; None = all): their rings become the zero left-pad again."""
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

    @torch.no_grad()
    def push_rows(self, x):
        """x [S, c, Cin]: the next c frames of every stream -> [S, c, Cout], the net's output at those frames."""
        if self.net.training:
            raise RuntimeError("TCNStream: the net is in train mode (dropout); call .eval() first")
        _check_rows(x, "x", self.streams, self.cin)
        x = x.contiguous()
        packs, c, last = self._pack(), x.shape[1], len(self.xrings) - 1
        out = torch.empty((self.streams, c, self.cout), device=self.device, dtype=torch.float32)
        for c0 in range(0, c, self.max_new):
            n = min(self.max_new, c - c0)
            whole = n == c
            ops.tcn_stream_append(x if whole else x[:, c0:c0 + n].contiguous(), self.xrings[0],
                                  self._pos & (self.ring_frames[0] - 1))
            dense = out if whole else torch.empty((self.streams, n, self.cout), device=self.device, dtype=torch.float32)
            for lvl, pack in enumerate(packs):
                if lvl < last:
                    block_push(pack, self.xrings[lvl], self.hrings[lvl], self._pos, n, out_ring=self.xrings[lvl + 1],
                               out_pos=self._pos)
                else:
                    block_push(pack, self.xrings[lvl], self.hrings[lvl], self._pos, n,
                               out_dense=dense.view(self.streams * n, self.cout))
            if not whole:
                out[:, c0:c0 + n] = dense
            self._pos += n
        self.frames_seen = [f + c for f in self.frames_seen]
        return out


class LFANStream:
    """An eval-mode ``LFAN`` on live streams: ``push`` the next c frames of ``streams`` sequences, get their logits.
    The model's ``example_length`` plays no part."""

    def __init__(self, model, streams, max_new=32):
        if not isinstance(model, LFAN):
            raise TypeError(f"LFANStream needs an LFAN (JMT / MT attend over time and are not causal), got {type(model).__name__}")
        if model.training:
            raise RuntimeError("LFANStream: the model is in train mode; batch statistics are undefined frame by frame -- call .eval()")
        self.model, self.streams, self.max_new = model, streams, max_new
        self.tcn = {m: TCNStream(model.temporal[m], streams, max_new) for m in model.modality}

    @property
    def frames_seen(self):
        return self.tcn[self.model.modality[0]].frames_seen

    @property
    def ring_frames(self):
        return {m: t.ring_frames for m, t in self.tcn.items()}

    def reset(self, streams=None):
        for t in self.tcn.values():
            t.reset(streams)

    def _check_keys(self, X):
        model = self.model
        if model.training:
            raise RuntimeError("LFANStream: the model is in train mode; batch statistics are undefined frame by frame -- call .eval()")
        for m in X:
            if m not in model.temporal:
                raise KeyError(m)
        for m in model.modality:
            if m not in X:
                raise KeyError(m)

    def _check_input(self, m, x):
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32):
            raise ValueError(f"{m}: expected a float32 tensor on the GPU, got "
                             f"{(x.dtype, x.device) if torch.is_tensor(x) else type(x)}")
        s = self.streams
        if m == "video":
            ok, c = x.dim() == 5 and x.shape[0] == s and x.shape[2] == 3, x.shape[1] if x.dim() == 5 else 0
            want = f"[{s}, c, 3, H, W]"
        elif m == "logmel":
            ok, c = x.dim() == 4 and x.shape[0] == s and x.shape[1] == 64 and x.shape[3] == 96, x.shape[2] if x.dim() == 4 else 0
            want = f"[{s}, 64, c, 96]"
        else:
            e = self.model.embedding_dim[m]
            ok, c = x.dim() == 4 and x.shape[0] == s and x.shape[1] == 1 and x.shape[3] == e, x.shape[2] if x.dim() == 4 else 0
            want = f"[{s}, 1, c, {e}]"
        if not ok or c < 1:
            raise ValueError(f"{m}: expected {want} for {s} streams, got {tuple(x.shape)}")
        return c

    @torch.no_grad()
    def push(self, X):
        """X keyed like ``LFAN.forward``'s dict with c new frames in place of L (video [S,c,3,H,W], vggish [S,1,c,128],
        bert [S,1,c,768], logmel [S,64,c,96]) -> logits [S, c, n_cls] (tanh-ed for REGRESSION).  X is left as it is."""
        self._check_keys(X)
        model, s = self.model, self.streams
        cs = {m: self._check_input(m, X[m]) for m in X}
        if len(set(cs.values())) != 1:
            raise ValueError(f"the modalities bring different numbers of new frames: {cs}")
        c = next(iter(cs.values()))
        if "visual" in model.spatial:
            model.spatial["visual"].backbone.check_sync_release()
        feats = {}
        for m in X:   # the encoders exactly as LFAN.forward runs them
            x = X[m]
            if m == "video":
                vis = model.spatial["visual"]
                vis.backbone.dropout_seed = model.dropout_seed
                feats[m] = vis(x.reshape(-1, *x.shape[2:]), None).view(s, c, -1)
            elif m == "logmel":
                feats[m] = model.spatial["audio"](x.permute(0, 2, 3, 1).contiguous().view(-1, 96, 64)).view(s, c, -1)
            else:
                feats[m] = x.reshape(s, c, x.shape[-1])
        return self._tail(feats, c)

    @torch.no_grad()
    def push_features(self, F):
        """F[m] [S, c, embedding_dim[m]]: per-modality embeddings of the next c frames (``video``: the 512-d encoder output)
        -> logits [S, c, n_cls].  Skips the encoders."""
        self._check_keys(F)
        for m in F:
            _check_rows(F[m], m, self.streams, self.model.embedding_dim[m])
        cs = {m: F[m].shape[1] for m in F}
        if len(set(cs.values())) != 1:
            raise ValueError(f"the modalities bring different numbers of new frames: {cs}")
        return self._tail({m: F[m].contiguous() for m in F}, next(iter(cs.values())))

    def _tail(self, feats, c):
        model, mods, rows = self.model, list(self.model.modality), self.streams * c
        t = [self.tcn[m].push_rows(feats[m].detach()).view(rows, -1) for m in mods]
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
        logits = ops.linear(z, _packed(model.regressor.weight), bias=model.regressor.bias)
        out = logits.view(self.streams, c, -1)
        return ops.tanh_fwd(out) if model.task == REGRESSION else out


_TIME_AXIS = {"video": 1}   # every other modality: axis 2


def stream_forward(model, X, chunk=32):
    """A whole clip or video of any length T through an eval-mode LFAN, causally, ``chunk`` frames at a time:
    [B, T, n_cls], what ``model(X)`` returns when it is built with ``example_length = T``.  X is left as it is."""
    first = next(iter(X.values()))
    stream = LFANStream(model, first.shape[0], max_new=chunk)
    stream._check_keys(X)
    total = {m: x.shape[_TIME_AXIS.get(m, 2)] for m, x in X.items()}
    if len(set(total.values())) != 1:
        raise ValueError(f"the modalities have different lengths: {total}")
    total = next(iter(total.values()))
    outs = [stream.push({m: x.narrow(_TIME_AXIS.get(m, 2), t0, min(chunk, total - t0)) for m, x in X.items()})
            for t0 in range(0, total, chunk)]
    return outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)
