"""VGGish audio encoder + log-mel front end on the HIP kernels.

Mirror of the reference's ``VGG`` / ``VGGish`` / ``AudioBackbone`` (models/backbone.py:16-66,
133-145; pre-processing twin abaw5_pre_processing/base/vggish/vggish.py) and of the numpy front
end ``waveform_to_examples`` / ``wavfile_to_examples`` (vggish_input.py:37-98), its channel mixdown
and resampling to 16 kHz included: same state-dict keys (``features.N`` / ``embeddings.N``),
``forward(x [n,96,64]) -> [n,128]``.

Pipeline: the 1-channel stem conv reads the log-mel patch directly (small-Cin gather path), every
conv fuses bias + ReLU, max-pools are NHWC kernels, and the reference's two transposes before the
flatten are free because the activations already are (H, W, C).
"""
import math

import numpy as np
import torch
from torch import nn

from . import ops

SAMPLE_RATE = 16000
CONV_IDX = (0, 3, 6, 8, 11, 13)
POOL_AFTER = (0, 3, 8, 13)


def _make_layers():
    layers, cin = [], 1
    for v in [64, "M", 128, "M", 256, 256, "M", 512, 512, "M"]:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    return nn.Sequential(*layers)


def hertz_to_mel(f):
    return 1127.0 * np.log(1.0 + f / 700.0)


def mel_matrix(num_mel_bins=64, num_bins=257, sample_rate=16000, lower=125.0, upper=7500.0):
    """HTK mel weights, DC row zeroed (mel_features.py:134-204) -- a host-side constant."""
    bins_mel = hertz_to_mel(np.linspace(0.0, sample_rate / 2.0, num_bins))
    edges = np.linspace(hertz_to_mel(lower), hertz_to_mel(upper), num_mel_bins + 2)
    w = np.empty((num_bins, num_mel_bins))
    for i in range(num_mel_bins):
        lo, ce, up = edges[i:i + 3]
        w[:, i] = np.maximum(0.0, np.minimum((bins_mel - lo) / (ce - lo), (up - bins_mel) / (up - ce)))
    w[0, :] = 0.0
    return w


def example_starts(num_frames, window_frames, hop_frames):
    """my_frame (mel_features.py:21-49): Python round() -> half to even, fractional hop."""
    n = 1 + int(np.floor((num_frames - window_frames) / hop_frames))
    return [round(hop_frames * i) for i in range(max(n, 0))]


# resampy's windowed-sinc filters: (zero crossings per side, Kaiser beta, roll-off as a share of Nyquist)
RESAMPLE_FILTERS = {"kaiser_best": (64, 14.769656459379492, 0.9475937167399596),
                    "kaiser_fast": (16, 8.555504641634386, 0.85)}
MAX_RESAMPLE_TAPS = 1 << 22


def resampled_length(n_in, sr_in):
    """resampy's output length: the Python float expression, not an integer floor (the two can differ by one)."""
    return int(n_in * (float(SAMPLE_RATE) / sr_in))


def resample_taps(sr_in, filter):
    """Polyphase table of the band-limited interpolation  y[n] = scale sum_k x[k] h(scale (n / ratio - k)),
    ratio = 16000 / sr_in, scale = min(1, ratio),  h(u) = rolloff sinc(rolloff u) I0(beta sqrt(1 - (u / zeros)^2)) / I0(beta)
    inside |u| < zeros  (resampy.resample's definition with the continuous window: resampy itself interpolates linearly in
    a sampled one).  With L / M = ratio in lowest terms, output n sits at input position q + r / L (q, r = divmod(n M, L)):
    ``taps[r][j] = scale h(scale (r / L + J - j))`` multiplies input q - J + j, J = ceil(zeros / scale), j < T = 2 J + 2.
    Returns (taps [L, T] float64, L, M).  At 16 kHz the reference does not filter at all: the table is the identity."""
    if filter not in RESAMPLE_FILTERS:
        raise ValueError(f"unknown resampling filter {filter!r}: one of {sorted(RESAMPLE_FILTERS)}")
    if int(sr_in) != sr_in or sr_in <= 0:
        raise ValueError(f"sample rate must be a positive integer, got {sr_in!r}")
    sr_in = int(sr_in)
    if sr_in == SAMPLE_RATE:
        return np.array([[1.0, 0.0]]), 1, 1
    zeros, beta, rolloff = RESAMPLE_FILTERS[filter]
    g = math.gcd(SAMPLE_RATE, sr_in)
    L, M = SAMPLE_RATE // g, sr_in // g
    scale = min(1.0, float(SAMPLE_RATE) / sr_in)
    J = int(math.ceil(zeros / scale))
    T = 2 * J + 2
    if L * T > MAX_RESAMPLE_TAPS:
        raise ValueError(f"resampling {sr_in} Hz -> {SAMPLE_RATE} Hz with {filter!r} needs a {L} x {T} tap table, more than "
                         f"{MAX_RESAMPLE_TAPS} entries: resample to a rate with a larger common divisor first")
    # r / L + J - j as ONE rounded quotient of an exact integer
    u = scale * ((np.arange(L)[:, None] + (J - np.arange(T)[None, :]) * L) / float(L))
    inside = np.abs(u) < zeros
    window = np.i0(beta * np.sqrt(np.where(inside, 1.0 - (u / zeros) ** 2, 0.0))) / np.i0(beta)
    return np.where(inside, scale * rolloff * np.sinc(rolloff * u) * window, 0.0), L, M


def _fc_split_k(n):
    return max(1, min(8, 512 // max(1, (n + 127) // 128 * 32)))


def _rows2d(t):
    """[n, 1, 1, C] (or [n, C]) fp32 tensor / 16-bit plane / Split -> the [n, C] view."""
    n, c = t.shape[0], t.shape[-1]
    return t.view(n, c)


class _ReleasedEmbeddings(torch.autograd.Function):
    """VGGish's embedding stack (Linear 12288->4096, ReLU, Linear 4096->4096, ReLU, Linear 4096->128; backbone.py:16-31)
    WITH its backward, for the audio groups of the reference's gradual release (base/parameter_control.py:58,85-103:
    parameters 16-17, then 14-15, then 12-13 -- always a suffix of the stack, top first).

    Forward: exactly the kernels of the frozen forward (``VGGish._embed``), so the output is the same bits.  It keeps the
    input of every released layer as the planes the forward already made (fp32, ``Split`` or one 16-bit plane); the input
    of the layer above a ReLU is that ReLU's output, i.e. the mask of the layer below.

    Backward, top layer down: ``ops.fc_bwd`` (ReLU mask + split + bias gradient in one pass), the weight gradient as a 1x1
    conv weight gradient over the rows (the bf16x3 kernel on split operands; the fp32 kernel in "fp32"), and -- only while a
    lower layer is released -- the data gradient as a 1x1 conv on the transposed weight in the encoder's arithmetic.  An fp16
    encoder runs its data gradients on the bf16x3 kernels (fp32 range: un-scaled gradients cannot underflow), like the
    released IR-50 units.  No gradient reaches the convolutions (never released)."""

    @staticmethod
    def forward(ctx, e, vgg, depth, w0, b0, w2, b2, w4, b4):
        out, acts = vgg._embed(e)
        ctx.acts = [None] * (3 - depth) + acts[3 - depth:]      # the inputs of the released layers only
        ctx.weights = (w2.detach() if depth >= 3 else None, w4.detach() if depth >= 2 else None)   # data gradients
        ctx.prec, ctx.depth = vgg.precision, depth
        return out

    @staticmethod
    def backward(ctx, dout):
        prec, depth, acts = ctx.prec, ctx.depth, ctx.acts
        w_of = {2: ctx.weights[0], 4: ctx.weights[1]}
        dprec = "bf16x3" if prec == "fp16" else prec
        grads = {}
        da = dout.contiguous()
        n = da.shape[0]
        for j, (layer, k) in enumerate(((4, 2), (2, 1), (0, 0))[:depth]):
            x_in = acts[k]
            mask = _rows2d(acts[k + 1]) if layer != 4 else None
            r = ops.fc_bwd(da, mask, out_split=prec != "fp32", out_f32=prec == "fp32")
            cout, cin = da.shape[1], x_in.shape[-1]
            if prec == "fp32":
                dw = ops.conv2d_wgrad(r["f32"].view(n, 1, 1, cout), x_in.view(n, 1, 1, cin), 1, 1)
            else:
                xs = x_in if isinstance(x_in, ops.Split) else ops.split_bf16(ops.from_n16(x_in))   # exact for bf16 / fp16
                dw = ops.conv2d_wgrad(r["split"].view(n, 1, 1, cout), xs.view(n, 1, 1, cin), 1, 1)
            grads[layer] = (dw.view(cout, cin), r["db"])
            if j + 1 < depth:   # the data gradient feeds the next released layer down
                wt = ops.pack_conv_weight(w_of[layer].view(cout, cin, 1, 1).contiguous(), transpose=True)   # [cin, cout]
                split = max(1, min(8, cout // 512))
                if dprec == "fp32":
                    da = ops.linear(r["f32"], wt, split_k=split)
                elif dprec == "bf16x3":
                    da = ops.conv2d_b3(r["split"].view(n, 1, 1, cout), ops.split_bf16(wt), 1, 1, split_k=split, out_f32=True,
                                       out_split=False)["y"].view(n, cin)
                else:   # bf16 storage: the hi plane IS bf16(dz) (round-to-nearest-even, like ops.to_n16)
                    da = ops.conv2d_n16(r["split"].hi.view(n, 1, 1, cout), ops.to_n16(wt, torch.bfloat16), 1, 1, split_k=split,
                                        out_f32=True, out_n16=False)["y"].view(n, cin)
            del r
        g0, g2, g4 = grads.get(0, (None, None)), grads.get(2, (None, None)), grads.get(4, (None, None))
        return None, None, None, g0[0], g0[1], g2[0], g2[1], g4[0], g4[1]


class VGGish(nn.Module):
    def __init__(self):
        super().__init__()
        self.features = _make_layers()
        self.embeddings = nn.Sequential(nn.Linear(512 * 4 * 6, 4096), nn.ReLU(True), nn.Linear(4096, 4096), nn.ReLU(True),
                                        nn.Linear(4096, 128))
        self._packed, self._key = None, None
        self._mel = None
        self._taps = {}   # (sample rate, filter) -> (device tap table, L, M)
        # "bf16x3": convs 2-6 and the three FCs on the split-bf16 kernels (<= 2^-15 relative per product); "fp32": exact fp32;
        # "bf16" / "fp16": narrow storage (one 16-bit plane per tensor, one MFMA per product, fp32 accumulate) -- what the
        # reference's autocast computes (trainer.py:367) and BASELINE cfg5's "bf16" asks of the whole tri-modal step
        self.precision = "bf16x3"

    def _pack(self):
        key = tuple((p.data_ptr(), p._version) for p in self.parameters())
        if self._packed is None or key != self._key:
            if self.features[0].weight.device.type != "cuda":
                raise RuntimeError("VGGish runs on the HIP kernels only: move the module to a GPU (no CPU fallback)")
            convs = [ops.pack_conv_weight(self.features[i].weight.detach().contiguous()) for i in CONV_IDX]
            self._packed = {"convs": convs, "convs_b3": [None] + [ops.split_bf16(w) for w in convs[1:]],
                            "fc_b3": [ops.split_bf16(self.embeddings[i].weight.detach().contiguous()) for i in (0, 2, 4)]}
            self._key = key
        return self._packed

    def _pack_n16(self, dtype):
        packed = self._pack()
        if packed.get("n16_dtype") != dtype:
            packed["convs_n16"] = [None] + [ops.to_n16(w, dtype) for w in packed["convs"][1:]]
            packed["fc_n16"] = [ops.to_n16(self.embeddings[i].weight.detach().contiguous(), dtype) for i in (0, 2, 4)]
            packed["n16_dtype"] = dtype
        return packed

    def __deepcopy__(self, memo):
        import copy
        packed, self._packed = self._packed, None
        try:
            new = self.__class__.__new__(self.__class__)
            memo[id(self)] = new
            new.__dict__ = copy.deepcopy(self.__dict__, memo)
        finally:
            self._packed = packed
        return new

    def _release_depth(self):
        """How many embedding layers train (base/parameter_control.py:57-58,85-103 releases parameters 16-17 =
        ``embeddings.4``, then 14-15 = ``embeddings.2``, then 12-13 = ``embeddings.0``): 0 (frozen, or no autograd), 1, 2 or 3.
        Anything the reference cannot produce fails loudly here, before any launch."""
        if not torch.is_grad_enabled():
            return 0
        if any(p.requires_grad for p in self.features.parameters()):
            raise NotImplementedError("the VGGish convolutions have no backward on the HIP path (the reference releases "
                                      "only the embedding layers, parameters 12..17 of the audio encoder)")
        flags = []
        for i in (0, 2, 4):
            f = [p.requires_grad for p in self.embeddings[i].parameters()]
            if any(f) and not all(f):
                raise NotImplementedError("release whole embedding layers (weight and bias) or nothing")
            flags.append(all(f))
        first = len(flags)
        while first > 0 and flags[first - 1]:
            first -= 1
        if any(flags[:first]):
            raise NotImplementedError("released embedding layers must form a suffix of the stack (the reference releases "
                                      "from the top: embeddings.4, then embeddings.2, then embeddings.0)")
        return len(flags) - first

    def forward(self, x, fs=None):
        """x: [n,96,64] log-mel examples (tensor or numpy, like the reference) -> [n,128]."""
        depth = self._release_depth()
        if self.precision not in ("bf16x3", "bf16", "fp16", "fp32"):
            raise ValueError(f"unknown precision {self.precision!r}")
        dev = self.features[0].weight.device
        x = torch.as_tensor(x).to(dev).float().contiguous()
        with torch.no_grad():   # the conv trunk is never released
            e = self._trunk(x)
        if depth == 0:
            return self._embed(e)[0]
        fc = self.embeddings
        return _ReleasedEmbeddings.apply(e, self, depth, fc[0].weight, fc[0].bias, fc[2].weight, fc[2].bias, fc[4].weight,
                                         fc[4].bias)

    def _trunk(self, x):
        """The six convs and four max-pools: the flattened (H, W, C) feature [n, 12288] as the precision mode carries it
        into the embedding stack (fp32, ``Split`` or one 16-bit plane)."""
        packed = self._pack()
        n = x.shape[0]
        if self.precision == "bf16x3":
            return self._trunk_b3(x, packed, n)
        if self.precision in ("bf16", "fp16"):
            return self._trunk_n16(x, n, torch.bfloat16 if self.precision == "bf16" else torch.float16)
        packed = packed["convs"]
        y = x.view(n, 1, x.shape[1], x.shape[2])  # NCHW with C = 1
        for j, i in enumerate(CONV_IDX):
            y = ops.conv2d(y, packed[j], 3, 3, pad=(1, 1), bias=self.features[i].bias.detach(), act1=ops.ACT_RELU,
                           x_nchw=(j == 0))
            if i in POOL_AFTER:
                y = ops.maxpool2x2_nhwc(y)
        return y.view(n, -1)  # (H, W, C) flatten == the reference's transposes + view

    def _embed(self, e):
        """The three embedding layers on the trunk's output.  Returns (output [n, 128], [e0, e1, e2]): the inputs of
        ``embeddings.0`` / ``.2`` / ``.4`` as the forward made them (e1 / e2 are also the post-ReLU outputs of .0 / .2)."""
        fc = self.embeddings
        if self.precision == "fp32":
            n = e.shape[0]
            split = _fc_split_k(n)
            e1 = ops.linear(e, fc[0].weight.detach(), bias=fc[0].bias.detach(), act=ops.ACT_RELU, split_k=split)
            e2 = ops.linear(e1, fc[2].weight.detach(), bias=fc[2].bias.detach(), act=ops.ACT_RELU, split_k=split)
            return ops.linear(e2, fc[4].weight.detach(), bias=fc[4].bias.detach(), split_k=split), [e, e1, e2]
        if self.precision == "bf16x3":
            packed = self._pack()
            n = e.shape[0]
            split = _fc_split_k(n)
            e1 = ops.conv2d_b3(e, packed["fc_b3"][0], 1, 1, bias=fc[0].bias.detach(), act1=ops.ACT_RELU, split_k=split)["split"]
            e2 = ops.conv2d_b3(e1, packed["fc_b3"][1], 1, 1, bias=fc[2].bias.detach(), act1=ops.ACT_RELU, split_k=split)["split"]
            out = ops.conv2d_b3(e2, packed["fc_b3"][2], 1, 1, bias=fc[4].bias.detach(), split_k=split, out_f32=True,
                                out_split=False)["y"].view(n, -1)
            return out, [e, e1, e2]
        packed = self._pack_n16(e.dtype)
        n = e.shape[0]
        split = _fc_split_k(n)
        e1 = ops.conv2d_n16(e, packed["fc_n16"][0], 1, 1, bias=fc[0].bias.detach(), act1=ops.ACT_RELU, split_k=split)["n16"]
        e2 = ops.conv2d_n16(e1, packed["fc_n16"][1], 1, 1, bias=fc[2].bias.detach(), act1=ops.ACT_RELU, split_k=split)["n16"]
        out = ops.conv2d_n16(e2, packed["fc_n16"][2], 1, 1, bias=fc[4].bias.detach(), split_k=split, out_f32=True,
                             out_n16=False)["y"].view(n, -1)
        return out, [e, e1, e2]

    def _trunk_b3(self, x, packed, n):
        """Layer 1 (Cin = 1) on the fp32 small-Cin kernel, everything else on the bf16x3 kernels.  Max-pooling
        needs the fp32 value, so a conv that feeds a pool writes fp32 and the pooled map is re-split."""
        feats = self.features
        y = ops.conv2d(x.view(n, 1, x.shape[1], x.shape[2]), packed["convs"][0], 3, 3, pad=(1, 1),
                       bias=feats[0].bias.detach(), act1=ops.ACT_RELU, x_nchw=True)
        cur = ops.split_bf16(ops.maxpool2x2_nhwc(y))
        for j, i in list(enumerate(CONV_IDX))[1:]:
            pooled = i in POOL_AFTER
            r = ops.conv2d_b3(cur, packed["convs_b3"][j], 3, 3, pad=(1, 1), bias=feats[i].bias.detach(), act1=ops.ACT_RELU,
                              out_f32=pooled, out_split=not pooled)
            cur = ops.split_bf16(ops.maxpool2x2_nhwc(r["y"])) if pooled else r["split"]
        k = cur.hi.numel() // n
        return cur.view(n, 1, 1, k)  # (H, W, C) flatten == the reference's transposes + view

    def _trunk_n16(self, x, n, dtype):
        """Narrow storage: layer 1 (Cin = 1) on the fp32 small-Cin kernel, convs 2-6 and the FCs on the narrow kernels.  A
        conv that feeds a max-pool writes fp32 (pooling wants the un-rounded value) and the pooled map is rounded once."""
        packed = self._pack_n16(dtype)
        feats = self.features
        y = ops.conv2d(x.view(n, 1, x.shape[1], x.shape[2]), packed["convs"][0], 3, 3, pad=(1, 1),
                       bias=feats[0].bias.detach(), act1=ops.ACT_RELU, x_nchw=True)
        cur = ops.to_n16(ops.maxpool2x2_nhwc(y), dtype)
        for j, i in list(enumerate(CONV_IDX))[1:]:
            pooled = i in POOL_AFTER
            r = ops.conv2d_n16(cur, packed["convs_n16"][j], 3, 3, pad=(1, 1), bias=feats[i].bias.detach(), act1=ops.ACT_RELU,
                               out_f32=pooled, out_n16=not pooled)
            cur = ops.to_n16(ops.maxpool2x2_nhwc(r["y"]), dtype) if pooled else r["n16"]
        k = cur.numel() // n
        return cur.view(n, 1, 1, k)

    # ---------------------------------------------------------------- front end
    def _resample_table(self, sample_rate, filter, dev):
        hit = self._taps.get((sample_rate, filter))
        if hit is None or hit[0].device != dev:
            taps, L, M = resample_taps(sample_rate, filter)
            hit = self._taps[(sample_rate, filter)] = (torch.from_numpy(taps).to(dev).contiguous(), L, M)
        return hit

    def wav_int16_to_examples(self, pcm_int16, sample_rate, window_sec=0.96, hop_sec=0.96, resample=None):
        """wavfile_to_examples for PCM already in memory: pcm [clips, S] (or [S]) int16 at 16 kHz ->
        [clips, n_examples, 96, 64] float32 on the GPU.

        With ``resample`` = "kaiser_best" / "kaiser_fast" any positive integer rate and interleaved multi-channel PCM
        [clips, S, C] are taken as well: channel mean, one second of edge padding at the input rate, band-limited
        interpolation to 16 kHz (``resample_taps``), then the log-mel on the float64 samples."""
        if resample is None:
            if sample_rate != SAMPLE_RATE:
                raise ValueError(f"{sample_rate} Hz PCM needs resample='kaiser_best' or 'kaiser_fast' (the reference resamples "
                                 "with resampy); without it only 16 kHz is taken")
        elif resample not in RESAMPLE_FILTERS:
            raise ValueError(f"unknown resampling filter {resample!r}: one of {sorted(RESAMPLE_FILTERS)}")
        elif int(sample_rate) != sample_rate or sample_rate <= 0:
            raise ValueError(f"sample rate must be a positive integer, got {sample_rate!r}")
        dev = self.features[0].weight.device
        pcm = torch.as_tensor(pcm_int16).to(dev)
        if pcm.dim() == 1:
            pcm = pcm[None]
        if self._mel is None or self._mel.device != dev:
            self._mel = torch.from_numpy(mel_matrix()).to(dev).contiguous()
        if resample is None or (sample_rate == SAMPLE_RATE and pcm.dim() == 2):
            lm = ops.logmel(pcm.contiguous(), sample_rate, self._mel, 0.01)  # pad = one second of edge samples
        else:
            sample_rate = int(sample_rate)
            taps, L, M = self._resample_table(sample_rate, resample, dev)
            n_out = resampled_length(pcm.shape[1] + sample_rate, sample_rate)
            samples = ops.resample_pcm(pcm.contiguous(), pcm.dim() == 3, sample_rate, taps, L, M, n_out)
            lm = ops.logmel_f64(samples, self._mel, 0.01)
        win = int(round(window_sec * 100.0))
        starts = example_starts(lm.shape[1], win, hop_sec * 100.0)
        return ops.frame_examples(lm, starts, win)   # host list: bounds-checked there before the launch


class AudioBackbone(nn.Module):
    def __init__(self):
        super().__init__()
        self.backbone = VGGish()
        for p in self.backbone.parameters():
            p.requires_grad = False

    def forward(self, x, extract_vggish=False):
        return self.backbone(x)
